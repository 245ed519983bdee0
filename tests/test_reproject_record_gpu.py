"""GPU: dh_reproject called directly with a record, against the positional entry of the same call, on poisoned outputs and a
poisoned workspace: every byte of every output, counts, bg_counts and the rows past the counts.  The positional entries are
prefixes of one another, so a case names how many of the widest entry's arguments its entry takes.  Smallest shapes that reach
each arm: res 64 (the bit-row morphology) and 50 (the byte morphology), two masks of a few hundred pixels, K = 2."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_moves_ref as CM  # noqa: E402
import multi_object_ref as R  # noqa: E402
import object_insertion_ref as I  # noqa: E402
import similarity_ref as S  # noqa: E402
import test_camera_moves_gpu as CG  # noqa: E402  (helpers only: _setup, _view_rows, dev)
import test_object_copies_gpu as OC  # noqa: E402  (helpers only: _rows)
from diffusionhandles_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
dev = CG.dev
I32P, U8P, F64P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_double)
K = 2
# entry, its workspace query and the sizes the query takes, by the number of arguments the entry takes of dh_reproject_bend_edits'
ENTRIES = {27: ("dh_reproject_similarity_edits", "dh_reproject_objects_workspace_bytes", "res n_fg K M"),
           30: ("dh_reproject_footprint_edits", "dh_reproject_footprints_workspace_bytes", "res n_fg K M footprints"),
           33: ("dh_reproject_instance_edits", "dh_reproject_instances_workspace_bytes", "res n_pts K M N footprints"),
           35: ("dh_reproject_donor_edits", "dh_reproject_donor_workspace_bytes", "res n_pts K M N footprints"),
           40: ("dh_reproject_camera_edits", "dh_reproject_camera_workspace_bytes", "res n_pts K M N footprints"),
           41: ("dh_reproject_border_edits", "dh_reproject_instances_workspace_bytes", "res n_pts K M N footprints"),
           43: ("dh_reproject_surface_edits", "dh_reproject_surface_ws_bytes", "res n_pts K M N view_surfaces"),
           45: ("dh_reproject_bend_edits", "dh_reproject_bend_ws_bytes", "res n_pts K M N view_surfaces footprints n_bones")}
# name -> (arguments of the entry, what the call has beyond the plain one)
CASES = {
    "plain": (27, dict()),
    "footprints with a ratio": (30, dict(footprints=1, max_ratio=1.5)),
    "a table with a copy": (33, dict(inst=[0, 1, 0])),
    "a donor mask": (35, dict(inst=[0, 1, 2], donor=True)),
    "a view in one edit": (40, dict(inst=[0, 1], cameras=["pan", None])),
    "reflect border": (41, dict(inst=[0, 1], infill_border=1)),
    "view surfaces": (43, dict(inst=[0, 1], cameras=[None, "orbit"], view_surfaces=1, surface_max_ratio=1.25)),
    "two bones": (45, dict(inst=[0, 1], n_bones=2)),
}


def _poisoned(res, n_pts, cap):
    nan = float("nan")
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=dev())
    return dict(zmap=full((K, res, res), nan, torch.float32), disparity=full((K, res, res), nan, torch.float32),
                raw_mask=full((K, res, res), 0xFF, torch.uint8), clean_mask=full((K, res, res), 0xFF, torch.uint8),
                vis=full((K, max(n_pts, 1)), 0xFF, torch.uint8), target_xy=full((K, max(n_pts, 1), 2), -7, torch.int32),
                corr=full((K, max(cap, 1), 4), -1, torch.int64), corr_inst=full((K, max(cap, 1)), 0xFF, torch.uint8),
                counts=full((K, 4), -1, torch.int32), bg_corr=full((K, res * res, 4), -1, torch.int64), bg_counts=full((K,), -1, torch.int32))


def _same(a, b, what):
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), f"{what}: {k}"


def _workspace(L, query, *sizes):
    nb = ctypes.c_size_t()
    assert getattr(L, query)(*sizes, ctypes.byref(nb)) == 0, L.dh_last_error()
    return torch.full((nb.value,), 0xFF, dtype=torch.uint8, device=dev()), nb.value


@pytest.mark.parametrize("res", [64, 50])
@pytest.mark.parametrize("case", list(CASES))
def test_the_record_entry_is_the_positional_entry_of_the_same_call(case, res):
    n_args, c = CASES[case]
    depth, bg, masks = R.two_spheres(res)
    donor = I.donor_scene(res, "disjoint") if c.get("donor") else None
    s = CG._setup(depth, bg, masks, donor=donor)
    L, M, R2 = s.L, s.M, res * res
    inst = c.get("inst", list(range(M)))
    N, B = len(inst), c.get("n_bones", 1)
    sizes = np.diff(s.obj_start)
    n_pts = int(sum(int(sizes[o]) for o in inst))
    footprints, surfaces, border = c.get("footprints", 0), c.get("view_surfaces", 0), c.get("infill_border", 0)
    cap = R2 if footprints or surfaces else n_pts
    tfs = S.edits_for(res, depth)
    flat = [[tfs[(e + n) % len(tfs)][inst[n] % 2] for n in range(N) for _ in range(B)] for e in range(K)]
    if B > 1:          # the second bone of every instance turns a little further
        flat = [[tf if j % B == 0 else (tf[0] + 20.0,) + tuple(tf[1:]) for j, tf in enumerate(row)] for row in flat]
    rows = OC._rows(flat)
    bone_w = None
    if B > 1:
        g = torch.Generator().manual_seed(3)
        w0 = torch.rand((K, n_pts, 1), generator=g)
        bone_w = torch.cat([w0, 1.0 - w0], dim=2).to(torch.float32).to(dev()).contiguous()
    cams = CM.cameras_for(depth)
    views, has_view = CG._view_rows([None if n is None else cams[n] for n in c["cameras"]]) if "cameras" in c else (None, None)
    tab = np.asarray(inst, dtype=np.int32)
    as_p = lambda arr, t: None if arr is None else arr.ctypes.data_as(t)
    n_host = s.n_host if donor is not None else M

    # the positional entry, on the workspace of its own query
    entry, query, names = ENTRIES[n_args]
    have = dict(res=res, n_fg=s.n_fg, n_pts=n_pts, K=K, M=M, N=N, footprints=footprints, view_surfaces=surfaces, n_bones=B)
    ws, nb = _workspace(L, query, *[have[k] for k in names.split()])
    o = _poisoned(res, n_pts, cap)
    args = (_lib.ptr(s.d), _lib.ptr(s.b), _lib.ptr(s.fg_pix), s.n_fg, M, as_p(s.obj_start, I32P), res, _lib.ptr(s.gx), _lib.ptr(s.gy),
            s.ifx, s.ify, s.fx, s.fy, K, as_p(rows, F64P), None, _lib.ptr(o["zmap"]), _lib.ptr(o["raw_mask"]), _lib.ptr(o["clean_mask"]),
            _lib.ptr(o["disparity"]), _lib.ptr(o["vis"]), _lib.ptr(o["target_xy"]), _lib.ptr(o["corr"]), _lib.ptr(o["counts"]), _lib.ptr(ws), nb,
            s.st, footprints, c.get("max_ratio", 0.0), cap, N, as_p(tab, I32P), _lib.ptr(o["corr_inst"]), _lib.ptr(s.donor), n_host,
            as_p(views, F64P), as_p(has_view, U8P), _lib.ptr(s.bg_valid), _lib.ptr(o["bg_corr"]), _lib.ptr(o["bg_counts"]), border,
            surfaces, c.get("surface_max_ratio", 0.0), B, _lib.ptr(bone_w))
    assert getattr(L, entry)(*args[:n_args]) == 0, L.dh_last_error()

    # the record: zero beyond what the case has (no table below the instance entry), on the workspace of the record query
    r = _poisoned(res, n_pts, cap)
    a = _lib.ReprojectArgs(res=res, n_fg=s.n_fg, n_objects=M, n_edits=K, corr_capacity=cap, footprints=footprints,
                           max_ratio=c.get("max_ratio", 0.0), infill_border=border, view_surfaces=surfaces,
                           surface_max_ratio=c.get("surface_max_ratio", 0.0), n_donor_objects=M - n_host, inv_fx=s.ifx, inv_fy=s.ify,
                           fx=s.fx, fy=s.fy, depth=_lib.ptr(s.d), bg_depth=_lib.ptr(s.b), fg_pix=_lib.ptr(s.fg_pix), grid_x=_lib.ptr(s.gx),
                           grid_y=_lib.ptr(s.gy), zmap=_lib.ptr(r["zmap"]), raw_mask=_lib.ptr(r["raw_mask"]), clean_mask=_lib.ptr(r["clean_mask"]),
                           disparity=_lib.ptr(r["disparity"]), vis=_lib.ptr(r["vis"]), target_xy=_lib.ptr(r["target_xy"]), corr=_lib.ptr(r["corr"]),
                           counts=_lib.ptr(r["counts"]), stream=s.st)
    a.obj_start, a.xforms_host = as_p(s.obj_start, I32P), as_p(rows, F64P)
    if n_args >= 33:
        a.n_instances, a.inst_obj, a.corr_inst = N, as_p(tab, I32P), _lib.ptr(r["corr_inst"])
    if donor is not None:
        a.donor_depth = _lib.ptr(s.donor)
    if views is not None:
        a.views, a.has_view = as_p(views, F64P), as_p(has_view, U8P)
        a.bg_valid, a.bg_corr, a.bg_counts = _lib.ptr(s.bg_valid), _lib.ptr(r["bg_corr"]), _lib.ptr(r["bg_counts"])
    if B > 1:
        a.n_bones, a.bone_w = B, _lib.ptr(bone_w)
    nbytes = ctypes.c_size_t()
    assert L.dh_reproject_workspace(ctypes.byref(a), ctypes.byref(nbytes)) == 0, L.dh_last_error()
    assert nbytes.value <= nb, "the record query asks for more than the positional query"
    wr = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device=dev())
    a.workspace, a.workspace_bytes = _lib.ptr(wr), nbytes.value
    assert L.dh_reproject(ctypes.byref(a)) == 0, L.dh_last_error()
    _same(r, o, f"{case}, res {res}")
    counts = o["counts"].cpu()
    assert (counts[:, 0] > 0).all() and (counts[:, 3] >= 0).all(), counts          # rows, and an in-fill that did not fail
    if views is None:
        assert bool((o["bg_counts"] == -1).all()) and bool((o["bg_corr"] == -1).all()), "background rows written without a view"
    else:
        assert [int(v) > 0 for v in o["bg_counts"].cpu()] == [bool(h) for h in has_view]
    assert (n_args < 33) == bool((o["corr_inst"] == 0xFF).all()), "the instance column: written with a table, and only then"


@pytest.mark.parametrize("res", [64, 50])
@pytest.mark.parametrize("view", [False, True])
def test_the_record_entry_without_a_foreground_point(view, res):
    """n_fg = 0 against dh_reproject_background (no view) and dh_reproject_camera_background (a view)"""
    depth, bg, masks = R.two_spheres(res)
    s = CG._setup(depth, bg, masks)
    L = s.L
    views, has_view = CG._view_rows([CM.cameras_for(depth)["pan"]])
    as_p = lambda arr, t: arr.ctypes.data_as(t)
    ws, nb = _workspace(L, "dh_reproject_background_workspace_bytes", res)
    o = {k: v[:1] for k, v in _poisoned(res, 0, 0).items() if k in ("zmap", "disparity", "counts", "bg_corr", "bg_counts")}
    args = (_lib.ptr(s.b), res, _lib.ptr(s.gx), _lib.ptr(s.gy), s.ifx, s.ify, s.fx, s.fy, None, _lib.ptr(o["zmap"]), _lib.ptr(o["disparity"]),
            _lib.ptr(o["counts"]), _lib.ptr(ws), nb, s.st)
    if view:
        rc = L.dh_reproject_camera_background(*args, as_p(views, F64P), _lib.ptr(s.bg_valid), _lib.ptr(o["bg_corr"]), _lib.ptr(o["bg_counts"]))
    else:
        rc = L.dh_reproject_background(*args)
    assert rc == 0, L.dh_last_error()
    r = {k: v[:1] for k, v in _poisoned(res, 0, 0).items() if k in o}
    a = _lib.ReprojectArgs(res=res, n_fg=0, n_edits=1, inv_fx=s.ifx, inv_fy=s.ify, fx=s.fx, fy=s.fy, bg_depth=_lib.ptr(s.b),
                           grid_x=_lib.ptr(s.gx), grid_y=_lib.ptr(s.gy), zmap=_lib.ptr(r["zmap"]), disparity=_lib.ptr(r["disparity"]),
                           counts=_lib.ptr(r["counts"]), stream=s.st)
    if view:
        a.views, a.has_view = as_p(views, F64P), as_p(has_view, U8P)
        a.bg_valid, a.bg_corr, a.bg_counts = _lib.ptr(s.bg_valid), _lib.ptr(r["bg_corr"]), _lib.ptr(r["bg_counts"])
    nbytes = ctypes.c_size_t()
    assert L.dh_reproject_workspace(ctypes.byref(a), ctypes.byref(nbytes)) == 0, L.dh_last_error()
    assert nbytes.value == nb
    wr = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev())
    a.workspace, a.workspace_bytes = _lib.ptr(wr), nb
    assert L.dh_reproject(ctypes.byref(a)) == 0, L.dh_last_error()
    _same(r, o, f"no foreground point, view = {view}, res {res}")
    counts = o["counts"].cpu()
    assert counts[0, :2].tolist() == [0, 0] and int(counts[0, 3]) >= 0
    assert (int(o["bg_counts"].cpu()[0]) > 0) if view else bool((o["bg_corr"] == -1).all())
