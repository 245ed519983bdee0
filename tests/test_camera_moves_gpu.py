"""GPU: camera moves (dh_reproject_camera_edits, dh_reproject_camera_background, dh_cells_from_correspondences_rows,
depth_transform.reproject_camera_edits / orbit_cameras, losses.process_correspondences(row_kind=...), the planned energy with
background rows, prepare_guidance / guided_inference[_batch] with row_kind, transform_foreground_objects[_batch] / transform_foregrounds
with a camera) against the test-side reference tests/camera_moves_ref.py: two_spheres at 128 and 256 pixels with edit 0 of
similarity_ref.edits_for and the six cameras of camera_moves_ref.cameras_for, grid 64 -- the sizes of the other geometry tests
(CLOSE element res // 50 >= 2, bit-row morphology, more than one workgroup per kernel).  The C entries write into outputs that
are NaN / 0xFF / -1 before the call."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_moves_ref as CM  # noqa: E402
import multi_object_ref as R  # noqa: E402
import object_copies_ref as C  # noqa: E402
import object_insertion_ref as I  # noqa: E402
import object_removal_ref as RM  # noqa: E402
import reproject_calls as RC  # noqa: E402
import similarity_ref as S  # noqa: E402
import test_object_copies_gpu as OC  # noqa: E402  (helpers only: _setup, _rows, _t)

pytestmark = pytest.mark.gpu
GRID = CM.GRID
DH_ERR_ARG = -1
SCALE = 64.0
OUTPUTS = ("zmap", "disp", "raw", "clean", "vis", "txy", "corr", "inst", "counts")


def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


_t = OC._t


def _setup(depth, bg, masks, removed=(), donor=None):
    """The device inputs of the C entry: host (and donor) masks concatenated in one pixel list, the donor depth, and bg_valid
    (0 under the host's masks and the removed masks)."""
    dmasks = [] if donor is None else list(donor[1])
    s = OC._setup(depth, bg, list(masks) + dmasks)
    s.donor = None if donor is None else donor[0].to(dev(), torch.float32).contiguous()
    s.n_host = len(masks)
    covered = torch.zeros(s.res * s.res, dtype=torch.bool)
    for m in list(masks) + list(removed):
        covered |= (m != 0).reshape(-1)
    s.bg_valid = (~covered).to(torch.uint8).to(dev()).contiguous()
    return s


def _view_rows(cameras):
    """(views [K, 16] f64, has_view [K] u8) of a list of cameras / None, through the host's one builder."""
    from diffusionhandles_amd import depth_transform as DT
    views = np.zeros((len(cameras), 16), dtype=np.float64)
    has = np.zeros(len(cameras), dtype=np.uint8)
    for e, c in enumerate(cameras):
        if c is not None:
            views[e], has[e] = DT.view_row(DT.check_camera(c)), 1
    return views, has


def _call(s, rows, inst, views=None, has_view=None, entry="camera", footprints=0, null=(), small_ws=False):
    """dh_reproject_camera_edits (or, entry="donor", dh_reproject_donor_edits) on poisoned outputs.  null: names of the
    background arguments to pass as NULL; small_ws: the donor entry's workspace (enough for a call without a view)."""
    from diffusionhandles_amd import _lib
    L, res, M = s.L, s.res, s.M
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    N = len(inst)
    K = rows.shape[0] // N
    sizes = np.diff(s.obj_start)
    n_pts = int(sum(int(sizes[o]) for o in inst))
    cap = res * res if footprints else n_pts
    nb = ctypes.c_size_t()
    if entry == "donor" or small_ws:
        _lib.check(L.dh_reproject_donor_workspace_bytes(res, n_pts, K, M, N, footprints, ctypes.byref(nb)))
    else:
        _lib.check(L.dh_reproject_camera_workspace_bytes(res, n_pts, K, M, N, footprints, ctypes.byref(nb)))
    ws = torch.full((nb.value,), 0xFF, dtype=torch.uint8, device=dev())
    nan = float("nan")
    o = SimpleNamespace(
        zmap=torch.full((K, res, res), nan, device=dev()), disp=torch.full((K, res, res), nan, device=dev()),
        raw=torch.full((K, res, res), 0xFF, dtype=torch.uint8, device=dev()),
        clean=torch.full((K, res, res), 0xFF, dtype=torch.uint8, device=dev()),
        vis=torch.full((K, n_pts), 0xFF, dtype=torch.uint8, device=dev()),
        txy=torch.full((K, n_pts, 2), -7, dtype=torch.int32, device=dev()),
        corr=torch.full((K, cap, 4), -1, dtype=torch.int64, device=dev()),
        inst=torch.full((K, cap), 0xFF, dtype=torch.uint8, device=dev()),
        counts=torch.full((K, 4), -1, dtype=torch.int32, device=dev()),
        bg_corr=torch.full((K, res * res, 4), -1, dtype=torch.int64, device=dev()),
        bg_counts=torch.full((K,), -1, dtype=torch.int32, device=dev()), n_pts=n_pts, K=K, N=N)
    tab = np.asarray(inst, dtype=np.int32)
    args = (_lib.ptr(s.d), _lib.ptr(s.b), _lib.ptr(s.fg_pix), s.n_fg, M, s.obj_start.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            res, _lib.ptr(s.gx), _lib.ptr(s.gy), s.ifx, s.ify, s.fx, s.fy, K, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            None, _lib.ptr(o.zmap), _lib.ptr(o.raw), _lib.ptr(o.clean), _lib.ptr(o.disp), _lib.ptr(o.vis), _lib.ptr(o.txy),
            _lib.ptr(o.corr), _lib.ptr(o.counts), _lib.ptr(ws), nb.value, s.st, footprints, 0.0, cap, N,
            tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _lib.ptr(o.inst), _lib.ptr(s.donor), s.n_host if s.donor is not None else M)
    if entry == "donor":
        o.rc = L.dh_reproject_donor_edits(*args)
    else:
        v = None if views is None else np.ascontiguousarray(views, dtype=np.float64)
        h = None if has_view is None else np.ascontiguousarray(has_view, dtype=np.uint8)
        o.rc = L.dh_reproject_camera_edits(
            *args, None if v is None else v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            None if h is None else h.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
            None if "bg_valid" in null else _lib.ptr(s.bg_valid), None if "bg_corr" in null else _lib.ptr(o.bg_corr),
            None if "bg_counts" in null else _lib.ptr(o.bg_counts))
    o.err = L.dh_last_error().decode() if o.rc != 0 else ""
    torch.cuda.synchronize()
    o.counts_h = o.counts.cpu()
    o.bg_h = o.bg_counts.cpu().tolist()
    if o.rc == 0:
        assert torch.isfinite(o.disp).all() and not torch.isnan(o.zmap).any()
        assert int(o.raw.max()) <= 1 and int(o.clean.max()) <= 1 and int(o.vis.max()) <= 1
        assert int(o.txy.min()) >= -1 and int(o.txy.max()) < res
        assert (o.counts_h[:, 3] >= 0).all(), "in-fill: a negative slot"
        for e in range(K):
            n = int(o.counts_h[e, 0])
            assert 0 < n <= cap and bool((o.corr[e, n:] == -1).all()) and bool((o.inst[e, n:] == 0xFF).all())
            assert int(o.corr[e, :n].min()) >= 0 and int(o.corr[e, :n].max()) < res and int(o.inst[e, :n].max()) < N
    return o


def _untouched(o):
    assert torch.isnan(o.zmap).all() and torch.isnan(o.disp).all()
    assert bool((o.raw == 0xFF).all()) and bool((o.clean == 0xFF).all()) and bool((o.vis == 0xFF).all())
    assert bool((o.txy == -7).all()) and bool((o.corr == -1).all()) and bool((o.counts == -1).all()) and bool((o.inst == 0xFF).all())
    assert bool((o.bg_corr == -1).all()) and bool((o.bg_counts == -1).all())


def _same_bytes(a, ea, b, eb, what):
    """Edit ea of call a against edit eb of call b, every output of the donor entry."""
    for k in OUTPUTS:
        x, y = getattr(a, k)[ea].contiguous().view(torch.uint8), getattr(b, k)[eb].contiguous().view(torch.uint8)
        assert torch.equal(x, y), f"{what}: {k}"


def _check(o, e, ref, what):
    """Every integer output bit-exact, the (-1, -1) of the discarded points included; the instance rows and the background
    rows with their order; the disparity within the 2e-3 (of 255) of the point-mode tests."""
    disp_r, corr_r, g = ref
    n, nb = int(o.counts_h[e, 0]), int(o.bg_h[e])
    corr_r = corr_r.numpy()
    assert n == g["n_instance_rows"] and nb == g["n_background"], f"{what}: {n} + {nb} rows, the reference has " \
        f"{g['n_instance_rows']} + {g['n_background']}"
    assert np.array_equal(o.corr[e, :n].cpu().numpy(), corr_r[:n]), f"{what}: instance rows (order included)"
    assert np.array_equal(o.inst[e, :n].cpu().numpy(), g["corr_inst"][:n]), f"{what}: corr_inst"
    assert np.array_equal(o.bg_corr[e, :nb].cpu().numpy(), corr_r[n:]), f"{what}: background rows (order included)"
    assert bool((o.bg_corr[e, nb:] == -1).all()), f"{what}: a row written past the count"
    assert np.array_equal(o.zmap[e].cpu().numpy(), g["zmap"]), f"{what}: zmap"
    assert np.array_equal(o.raw[e].cpu().numpy() != 0, g["raw_mask"]), f"{what}: raw mask"
    assert np.array_equal(o.clean[e].cpu().numpy() != 0, g["cleaned"] != 0), f"{what}: clean mask"
    assert np.array_equal(o.vis[e].cpu().numpy() != 0, g["vis"]), f"{what}: vis"
    txy = o.txy[e].cpu().numpy()
    assert np.array_equal(txy[:, 0], g["tx"]) and np.array_equal(txy[:, 1], g["ty"]), f"{what}: target_xy"
    assert int(o.counts_h[e, 1]) == int(g["vis"].sum()), f"{what}: visible count"
    assert int(o.counts_h[e, 2]) == int(g["inpaint"].sum()), f"{what}: in-fill count"
    err = float((o.disp[e].cpu() - disp_r[0, 0]).abs().max())
    print(f"{what}: {n} + {nb} rows, {int(g['gone'].sum())} points out of frame, {int(o.counts_h[e, 2])} in-fill pixels, "
          f"disparity max abs err {err:.2e}")
    assert err < 2e-3, f"{what}: disparity {err}"


# ---- 1. re-projection against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [128, 256])
def test_six_cameras_against_the_reference(res):
    """K = 6 in one call, one camera per edit, and each camera in a K = 1 call of its own (the bytes of its slice)."""
    fx = CM.fixture(res)
    s = _setup(fx["depth"], fx["bg_depth"], fx["masks"])
    names = list(CM.CAMERA_NAMES)
    cams = [fx["cameras"][n] for n in names]
    views, has = _view_rows(cams)
    rows1 = OC._rows([fx["transforms"]])
    o = _call(s, np.tile(rows1, (6, 1)), [0, 1], views, has)
    assert o.rc == 0, o.err
    for e, name in enumerate(names):
        _check(o, e, fx["geo"][name], f"res {res} K 6 {name}")
        one = _call(s, rows1, [0, 1], views[e:e + 1], has[e:e + 1])
        assert one.rc == 0, one.err
        _same_bytes(one, 0, o, e, f"res {res} K 1 {name}")
        nb = one.bg_h[0]
        assert nb == o.bg_h[e] and torch.equal(one.bg_corr[0, :nb], o.bg_corr[e, :nb])
    # the host layer: the instance rows, then the background rows with instance index N = 2
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    intr = D.intrinsics_f32()
    res_list, dbg = DT.reproject_camera_edits(fx["depth"].to(dev()), fx["bg_depth"].to(dev()), [m.to(dev()) for m in fx["masks"]], intr,
                                              [[_t(tf) for tf in fx["transforms"]]] * 6, cameras=cams, return_debug=True)
    for e, name in enumerate(names):
        disp, corr, inst = res_list[e]
        ref = fx["geo"][name]
        assert torch.equal(corr, ref[1]) and np.array_equal(inst.numpy(), ref[2]["corr_inst"]), name
        assert torch.equal(disp[0, 0].to(dev()), o.disp[e]), name
        assert dbg["n_background"][e] == ref[2]["n_background"]
        assert np.array_equal(dbg["row_background"][e].cpu().numpy(), (ref[2]["row_kind"] == 2).astype(np.uint8))
    # orbit_cameras: a turntable about the centre pixel is the fixture's orbit camera
    orbit, = DT.orbit_cameras(fx["depth"].to(dev()), intr, res // 2, res // 2, [8.0])
    assert np.array_equal(DT.view_row(orbit), CM.view_row(fx["cameras"]["orbit"]))
    with pytest.raises(ValueError, match="outside"):
        DT.orbit_cameras(fx["depth"].to(dev()), intr, res, 0, [8.0])


@pytest.mark.parametrize("res", [128, 256])
def test_mixed_call_of_view_and_no_view_edits(res):
    """The four edits of similarity_ref.edits_for, edits 0 and 2 with a camera: those against the reference, edits 1 and 3
    byte for byte what they are in the donor entry's call, with no background rows."""
    depth, bg, masks = R.two_spheres(res)
    edits = S.edits_for(res, depth)
    cams_all = CM.cameras_for(depth)
    cams = [cams_all["pan"], None, cams_all["general"], None]
    s = _setup(depth, bg, masks)
    views, has = _view_rows(cams)
    rows = OC._rows(edits)
    o = _call(s, rows, [0, 1], views, has)
    assert o.rc == 0, o.err
    plain = _call(s, rows, [0, 1], entry="donor")
    assert plain.rc == 0, plain.err
    for e in (1, 3):
        _same_bytes(o, e, plain, e, f"res {res} no-view edit {e} of the mixed call")
        assert o.bg_h[e] == 0 and bool((o.bg_corr[e] == -1).all())
    for e in (0, 2):
        ref = OC._refs(("camera mixed", res, e), lambda: CM.transform_camera(depth, bg, masks, [0, 1], edits[e], cams[e]))
        _check(o, e, ref, f"res {res} mixed edit {e}")
        assert not torch.equal(o.zmap[e], plain.zmap[e])


# ---- 2. calls without a view -------------------------------------------------------------------------------------------------
def _no_view_cases():
    depth, bg, masks = R.two_spheres(128)
    inst, edits = C.SET_A
    yield "instances", _setup(depth, bg, masks), OC._rows(edits), inst
    fx = RM.fixture(128, "A")
    yield "removal", _setup(fx["depth"], fx["bg_depth"], [fx["masks"][0]], removed=[fx["masks"][1]]), \
        OC._rows([fx["transforms"], RM.SECOND_EDIT]), [0]
    fx = I.fixture(128, "overlap")
    yield "donor", _setup(fx["depth"], fx["bg_depth"], fx["masks"], donor=(fx["donor_depth"], fx["donor_masks"])), \
        OC._rows(fx["edits"]), fx["instances"]


def test_has_view_all_zero_is_the_donor_entry():
    """Every output byte, with the donor entry's workspace; the background arguments are neither read nor written (NULL too)."""
    for what, s, rows, inst in _no_view_cases():
        base = _call(s, rows, inst, entry="donor")
        assert base.rc == 0, base.err
        K = base.K
        garbage = np.full((K, 16), np.nan)
        for how, kw in (("zero flags", dict(views=garbage, has_view=np.zeros(K, dtype=np.uint8))),
                        ("null views", dict(views=None, has_view=None)),
                        ("null background arguments", dict(views=garbage, has_view=np.zeros(K, dtype=np.uint8),
                                                           null=("bg_valid", "bg_corr", "bg_counts")))):
            o = _call(s, rows, inst, small_ws=True, **kw)
            assert o.rc == 0, (what, how, o.err)
            for e in range(K):
                _same_bytes(o, e, base, e, f"{what}, {how}, edit {e}")
            assert bool((o.bg_corr == -1).all()) and bool((o.bg_counts == -1).all()), (what, how)


def test_donor_with_a_view_against_the_reference():
    fx = I.fixture(128, "overlap")
    cam = CM.cameras_for(fx["depth"])["orbit"]
    s = _setup(fx["depth"], fx["bg_depth"], fx["masks"], donor=(fx["donor_depth"], fx["donor_masks"]))
    views, has = _view_rows([cam])
    o = _call(s, OC._rows(fx["edits"][:1]), fx["instances"], views, has)
    assert o.rc == 0, o.err
    ref = OC._refs(("camera donor", 128), lambda: CM.transform_camera(
        fx["depth"], fx["bg_depth"], fx["masks"], fx["instances"], fx["edits"][0], cam, donor=(fx["donor_depth"], fx["donor_masks"])))
    _check(o, 0, ref, "donor with a view")
    n = int(o.counts_h[0, 0])
    assert int((ref[2]["row_kind"][:n] == 1).sum()) >= 50 and ref[2]["n_background"] >= 5000
    # the host layer composes them: instance column 3 on the background rows, row_donor beside the instance rows
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    (disp, corr, inst), = DT.reproject_camera_edits(
        fx["depth"].to(dev()), fx["bg_depth"].to(dev()), [m.to(dev()) for m in fx["masks"]], D.intrinsics_f32(),
        [[_t(tf) for tf in fx["edits"][0]]], fx["instances"], donor_depth=fx["donor_depth"].to(dev()),
        donor_masks=[m.to(dev()) for m in fx["donor_masks"]], cameras=[cam])
    assert torch.equal(corr, ref[1]) and np.array_equal(inst.numpy(), ref[2]["corr_inst"])


# ---- 3. the background entry -------------------------------------------------------------------------------------------------
def _background_call(bg, view, bg_valid, entry="camera", null=()):
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    L = _lib.lib()
    res = bg.shape[-1]
    b = bg.to(dev(), torch.float32).contiguous()
    gx, gy = DT._grids(res, res, dev())
    intr = D.intrinsics_f32()
    ifx, ify = DT._inv_focal(intr)
    nb = ctypes.c_size_t()
    _lib.check(L.dh_reproject_background_workspace_bytes(res, ctypes.byref(nb)))
    ws = torch.full((nb.value,), 0xFF, dtype=torch.uint8, device=dev())
    o = SimpleNamespace(zmap=torch.full((res, res), float("nan"), device=dev()), disp=torch.full((res, res), float("nan"), device=dev()),
                        counts=torch.full((4,), -1, dtype=torch.int32, device=dev()),
                        bg_corr=torch.full((res * res, 4), -1, dtype=torch.int64, device=dev()),
                        bg_counts=torch.full((1,), -1, dtype=torch.int32, device=dev()))
    args = (_lib.ptr(b), res, _lib.ptr(gx), _lib.ptr(gy), ifx, ify, float(intr[0, 0]), float(intr[1, 1]), None, _lib.ptr(o.zmap),
            _lib.ptr(o.disp), _lib.ptr(o.counts), _lib.ptr(ws), nb.value, _lib.stream_ptr())
    if entry == "background":
        o.rc = L.dh_reproject_background(*args)
    else:
        v = None if view is None else np.ascontiguousarray(view, dtype=np.float64)
        o.rc = L.dh_reproject_camera_background(
            *args, None if v is None else v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            None if "bg_valid" in null else _lib.ptr(bg_valid), None if "bg_corr" in null else _lib.ptr(o.bg_corr),
            None if "bg_counts" in null else _lib.ptr(o.bg_counts))
    o.err = L.dh_last_error().decode() if o.rc != 0 else ""
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("name", ["pan", "dolly_in"])
@pytest.mark.parametrize("res", [128, 256])
def test_background_entry_with_a_view_against_the_reference(res, name):
    """The pure camera move with both spheres removed: bg_valid is 0 under them."""
    depth, bg, masks = R.two_spheres(res)
    cam = CM.cameras_for(depth)[name]
    ref = OC._refs(("camera pure", res, name), lambda: CM.background_camera(bg, cam, removed_masks=masks))
    covered = (masks[0] != 0) | (masks[1] != 0)
    bg_valid = (~covered).reshape(-1).to(torch.uint8).to(dev()).contiguous()
    views, _ = _view_rows([cam])
    o = _background_call(bg, views[0], bg_valid)
    assert o.rc == 0, o.err
    disp_r, corr_r, g = ref
    c = o.counts.tolist()
    nb = int(o.bg_counts[0])
    assert c[0] == 0 and c[1] == 0 and c[2] == int(g["inpaint"].sum()) and c[3] >= 0
    assert nb == len(corr_r) >= 5000 and np.array_equal(o.bg_corr[:nb].cpu().numpy(), corr_r.numpy())
    assert bool((o.bg_corr[nb:] == -1).all())
    assert np.array_equal(o.zmap.cpu().numpy(), g["zmap"]) and int(g["unowned"].sum()) >= 500
    err = float((o.disp.cpu() - disp_r[0, 0]).abs().max())
    print(f"pure {name} at {res}: {nb} rows, {c[2]} in-fill pixels, disparity max abs err {err:.2e}")
    assert err < 2e-3
    # the host layer: fg_masks = [], empty transform lists
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    (disp, corr, inst), = DT.reproject_camera_edits(depth.to(dev()), bg.to(dev()), [], D.intrinsics_f32(), [[]],
                                                    removed_masks=[m.to(dev()) for m in masks], cameras=[cam])
    assert torch.equal(corr, corr_r) and torch.equal(disp[0, 0].to(dev()), o.disp) and bool((inst == 0).all())


@pytest.mark.parametrize("res", [128, 256])
def test_background_entry_without_a_view_is_dh_reproject_background(res):
    _, bg, _ = R.two_spheres(res)
    base = _background_call(bg, None, None, entry="background")
    assert base.rc == 0, base.err
    o = _background_call(bg, None, None, null=("bg_valid", "bg_corr", "bg_counts"))
    assert o.rc == 0, o.err
    for k in ("zmap", "disp", "counts"):
        assert torch.equal(getattr(o, k).view(torch.uint8), getattr(base, k).view(torch.uint8)), k


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    fx = CM.fixture(128)
    s = _setup(fx["depth"], fx["bg_depth"], fx["masks"])
    rows = OC._rows([fx["transforms"]])
    views, has = _view_rows([fx["cameras"]["general"]])

    def bad(k, v):
        out = views.copy()
        out[0, k] = v
        return out
    cases = [("footprints", dict(views=views, footprints=1)), ("null bg_valid", dict(views=views, null=("bg_valid",))),
             ("null bg_corr", dict(views=views, null=("bg_corr",))), ("null bg_counts", dict(views=views, null=("bg_counts",))),
             ("scale 0", dict(views=bad(8, 0.0))), ("NaN translation", dict(views=bad(6, np.nan))),
             ("infinite pivot", dict(views=bad(12, np.inf))), ("flag 2", dict(views=bad(14, 2.0)))]
    for what, kw in cases:
        o = _call(s, rows, [0, 1], has_view=has, **kw)
        assert o.rc == DH_ERR_ARG and o.err, what
        _untouched(o)
        print(f"{what}: {o.err}")
    # the background entry
    _, bg, _ = R.two_spheres(128)
    valid = torch.ones(128 * 128, dtype=torch.uint8, device=dev())
    for what, view, null in (("null bg_corr", views[0], ("bg_corr",)), ("null bg_valid", views[0], ("bg_valid",)),
                             ("scale 0", bad(8, 0.0)[0], ())):
        o = _background_call(bg, view, valid, null=null)
        assert o.rc == DH_ERR_ARG and o.err, what
        assert torch.isnan(o.zmap).all() and torch.isnan(o.disp).all() and bool((o.counts == -1).all())
        assert bool((o.bg_corr == -1).all()) and bool((o.bg_counts == -1).all())


# ---- 5. cells ----------------------------------------------------------------------------------------------------------------
def _cells_call(corr, res, erosion, kinds, entry="rows"):
    from diffusionhandles_amd import _lib
    L = _lib.lib()
    c = torch.as_tensor(np.asarray(corr)).reshape(-1, 4).to(dev(), torch.int64).contiguous()
    n = c.shape[0]
    nb = ctypes.c_size_t()
    _lib.check(L.dh_cells_workspace_bytes(n, GRID, ctypes.byref(nb)))
    ws = torch.full((nb.value,), 0xFF, dtype=torch.uint8, device=dev())
    o = SimpleNamespace(pairs=torch.full((max(n, 1), 2), -1, dtype=torch.int32, device=dev()),
                        lists=torch.full((3, GRID * GRID), -1, dtype=torch.int32, device=dev()),
                        masks=torch.full((3, GRID * GRID), 0xFF, dtype=torch.uint8, device=dev()),
                        counts=torch.full((4,), -1, dtype=torch.int32, device=dev()))
    flags = None if kinds is None else torch.as_tensor(np.asarray(kinds)).to(dev(), torch.uint8).contiguous()
    fn = L.dh_cells_from_correspondences_rows if entry == "rows" else L.dh_cells_from_correspondences_donor
    o.rc = fn(_lib.ptr(c), n, res, GRID, erosion, _lib.ptr(o.pairs), _lib.ptr(o.lists), _lib.ptr(o.masks), _lib.ptr(o.counts),
              _lib.ptr(ws), nb.value, _lib.stream_ptr(), None, _lib.ptr(flags))
    o.err = L.dh_last_error().decode() if o.rc != 0 else ""
    torch.cuda.synchronize()
    return o


def _cells_same(a, b, what):
    c = a.counts.tolist()
    assert c == b.counts.tolist(), what
    assert torch.equal(a.masks, b.masks) and torch.equal(a.pairs[:c[0]], b.pairs[:c[0]]), what
    for k in range(3):
        assert torch.equal(a.lists[k, :c[1 + k]], b.lists[k, :c[1 + k]]), what


@pytest.mark.parametrize("er", [0, 5])
@pytest.mark.parametrize("res", [128, 256])
def test_cells_with_row_kinds_against_the_reference(res, er):
    """The donor fixture under the orbit camera at 128 (kinds 0, 1 and 2 in one call), the two-sphere fixture at 256."""
    if res == 128:
        fx = I.fixture(128, "overlap")
        cam = CM.cameras_for(fx["depth"])["orbit"]
        _, corr, g = OC._refs(("camera donor", 128), lambda: CM.transform_camera(
            fx["depth"], fx["bg_depth"], fx["masks"], fx["instances"], fx["edits"][0], cam, donor=(fx["donor_depth"], fx["donor_masks"])))
        assert set(g["row_kind"].tolist()) == {0, 1, 2}
    else:
        _, corr, g = CM.fixture(256)["geo"]["general"]
    corr, kind = corr.numpy(), g["row_kind"]
    ref = CM.cells(corr, res, kind, None, er)
    o = _cells_call(corr, res, er, kind)
    assert o.rc == 0, o.err
    c = o.counts.tolist()
    assert c[0] == len(ref["original_x"]) == len(corr)
    pairs = o.pairs[:c[0]].cpu().numpy()
    assert np.array_equal(pairs[:, 0], ref["original_y"] * GRID + ref["original_x"])
    assert np.array_equal(pairs[:, 1], ref["transformed_y"] * GRID + ref["transformed_x"])
    assert np.array_equal(o.masks.cpu().numpy().reshape(3, GRID, GRID), ref["masks"])
    for k, key in enumerate(("", "_orig", "_trans")):
        want = ref[f"background_y{key}"] * GRID + ref[f"background_x{key}"]
        assert c[1 + k] == len(want) and np.array_equal(o.lists[k, :c[1 + k]].cpu().numpy(), want)
    # without the kinds the background rows would clear their cells
    plain = _cells_call(corr, res, er, None)
    assert int(plain.masks[1].sum()) < int(o.masks[1].sum()) and int(plain.masks[2].sum()) < int(o.masks[2].sum())
    # the host layer
    from diffusionhandles_amd.losses import process_correspondences
    pc = process_correspondences(corr, res, er, grid=GRID, device=dev(), row_kind=kind, pair_instances=g["corr_inst"])
    for key in RM.CELL_KEYS:
        assert np.array_equal(pc[key], ref[key]), key
    assert np.array_equal(pc["object"], g["corr_inst"].astype(np.int64))


@pytest.mark.parametrize("er", [0, 5])
def test_cells_null_and_kinds_0_1_are_the_donor_entry(er):
    fx = I.fixture(128, "overlap")
    corr, flags = fx["geo"][0][1].numpy(), fx["geo"][0][2]["row_donor"]
    assert set(flags.tolist()) == {0, 1}
    for kinds in (None, flags, np.zeros(len(corr), dtype=np.uint8)):
        base = _cells_call(corr, 128, er, kinds, entry="donor")
        assert base.rc == 0, base.err
        _cells_same(_cells_call(corr, 128, er, kinds), base, "kinds 0 / 1")
    o = _cells_call(corr, 100, 0, flags)          # 100 is no multiple of the grid
    assert o.rc == DH_ERR_ARG and o.err
    assert bool((o.pairs == -1).all()) and bool((o.lists == -1).all()) and bool((o.masks == 0xFF).all()) and bool((o.counts == -1).all())


# ---- 6. energy: the background rows as instance N -----------------------------------------------------------------------------
def _energy_setup():
    from diffusionhandles_amd.losses import process_correspondences
    _, corr, g = CM.fixture(128)["geo"]["orbit"]
    corr = corr.numpy()
    pc = process_correspondences(corr, 128, 0, grid=GRID, device=dev(), row_kind=g["row_kind"], pair_instances=g["corr_inst"])
    objects = g["corr_inst"].astype(np.int64)[I.kept_rows(corr, 128)]
    assert np.array_equal(pc["object"], objects) and set(objects.tolist()) == {0, 1, 2}
    counts = np.bincount(objects)
    assert counts[2] >= 5 * (counts[0] + counts[1])          # the background's rows outnumber the objects' (README)
    return pc, CM.cells(corr, 128, g["row_kind"], None, 0), objects


def _maps(Cn, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(GRID, GRID, Cn, generator=gen).to(dtype).to(dev()) for _ in range(2))


def _check_energy(loss, grad, ref_loss, ref_grad, what):
    """The tolerances of tests/test_object_insertion_gpu.py: loss 2e-5 relative, gradient 1e-4 of its largest entry."""
    got = [float(v) for v in loss.cpu()]
    ref = ref_grad.double() * SCALE
    err, top = float((grad.double().cpu() - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: loss {got} / {list(ref_loss)}; gradient max abs err {err:.3e} (bound {1e-4 * top:.3e})")
    for a, r in zip(got, ref_loss):
        assert abs(a - r) <= 2e-5 * abs(r) + 1e-12, (what, got, ref_loss)
    assert err <= 1e-4 * top, what


@pytest.mark.parametrize("Cn", (64, 320))
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_energy_with_background_rows_against_the_reference(dtype, Cn):
    """Weighted plan ("equal" and explicit weights, the background as object 2) and the unweighted plan, against the fp64
    reference of object_weights_ref (through object_insertion_ref.energy_and_grad without donor objects)."""
    from diffusionhandles_amd.losses import EnergyPlan, energy_and_grad_planned
    pc, cells, objects = _energy_setup()
    act, orig = _maps(Cn, dtype, 900 + Cn)

    def run(plan, fw, bw):
        out = torch.full(act.shape, float("nan"), dtype=torch.float32, device=dev())
        loss, grad = energy_and_grad_planned(act, orig, plan, fw, bw, grad_scale=SCALE, want_loss=True, out=out,
                                             grad_dtype=torch.float32)
        torch.cuda.synchronize()
        assert torch.isfinite(grad).all() and torch.isfinite(loss).all()
        return loss, grad
    for ow in ("equal", [2.0, 1.0, 0.25]):
        plan = EnergyPlan(pc, GRID, dev(), object_weights=ow)
        assert plan.weighted and plan.n_objects == 3
        w = [1.0] * 3 if ow == "equal" else ow
        for fw, bw in ((7.5, 1.5), (7.5, 0.0)):
            ref_loss, ref_grad = I.energy_and_grad(act, orig, orig, cells, objects, set(), w, fw, bw, (GRID, GRID))
            loss, grad = run(plan, fw, bw)
            _check_energy(loss, grad, ref_loss, ref_grad, f"{dtype} C {Cn} weights {ow} ({fw}, {bw})")
    plan = EnergyPlan(pc, GRID, dev())
    assert not plan.weighted and plan.n_pairs == len(objects)
    ref_loss, ref_grad = I.energy_and_grad(act, orig, orig, cells, objects, set(), None, 7.5, 1.5, (GRID, GRID))
    loss, grad = run(plan, 7.5, 1.5)
    _check_energy(loss, grad, ref_loss, ref_grad, f"{dtype} C {Cn} unweighted")
    # the background rows are in the plan: without them the gradient is another one
    from diffusionhandles_amd.losses import process_correspondences
    _, corr, g = CM.fixture(128)["geo"]["orbit"]
    n = g["n_instance_rows"]
    pc0 = process_correspondences(corr.numpy()[:n], 128, 0, grid=GRID, device=dev(), row_kind=g["row_kind"][:n])
    _, grad0 = run(EnergyPlan(pc0, GRID, dev()), 7.5, 1.5)
    assert not torch.equal(grad0, grad)


# ---- 7. the loop on the TINY rig ----------------------------------------------------------------------------------------------
RES = 512
LOOP_TFS = [(15.0, R.Y, (0.1, 0.0, -0.05)), (-20.0, R.Y, (-0.15, 0.05, 0.1))]
SECOND_TFS = [(0.0, R.Y, (-0.1, 0.0, 0.0)), (10.0, R.Y, (0.1, 0.0, 0.0))]
CAMERA = (6.0, (0.3, 0.9, -0.2), (0.1, -0.05, 0.15))
SECOND_CAMERA = (-4.0, R.Y, (0.0, 0.0, 0.2))


@pytest.fixture(scope="module")
def tiny():
    from diffusionhandles_amd import DiffusionHandles
    from diffusionhandles_amd import conf as CF
    from diffusionhandles_amd.unet import HipUNet
    from oracle import unet_torch as U
    ref = U.init_synthetic_(U.UNetTorch(U.TINY), seed=0).to(dev()).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.half().float())
    hip = HipUNet(dict(U.TINY, text_len=77), dtype=torch.float16, max_batch=4)
    hip.load_state_dict(ref.state_dict())
    dh = DiffusionHandles(CF.load_default(), unet=hip, unet_config=dict(U.TINY, text_len=77)).to(dev())
    g = torch.Generator().manual_seed(11)
    noise = torch.randn(1, 4, RES // 8, RES // 8, generator=g).to(dev())
    Dm = dh.diffuser.unet.cfg["cross_attention_dim"]
    unc = (dh.diffuser._encode([""])[None].expand(50, -1, -1, -1) + 0.05 * torch.randn(50, 1, 77, Dm, generator=g).to(dev())).contiguous()
    depth, bg, masks = R.two_spheres(RES)
    depth, bg, masks = depth.to(dev()), bg.to(dev()), [m.to(dev()) for m in masks]
    prompt = "two spheres on a plane"
    null_text, noise, acts, _ = dh.generate_input_image(depth, prompt, unc, noise)
    two = SimpleNamespace(depth=depth, bg_depth=dh.set_foreground(depth, masks, bg), masks=masks, null_text=null_text, noise=noise,
                          acts=acts, prompt=prompt)
    return SimpleNamespace(dh=dh, gd=dh.diffuser, two=two)


def _common(im):
    return dict(depth=im.depth, prompt=im.prompt, bg_depth=im.bg_depth, null_text_emb=im.null_text, init_noise=im.noise,
                activations=im.acts)


def _loop_geometry(tiny, edits, cameras, device_correspondences=False):
    from diffusionhandles_amd import depth_transform as DT
    t = tiny.two
    return DT.reproject_camera_edits(t.depth, t.bg_depth, t.masks, tiny.gd.get_depth_intrinsics(device=dev()),
                                     [[_t(tf) for tf in tfs] for tfs in edits], cameras=cameras,
                                     device_correspondences=device_correspondences)


def test_transform_foreground_objects_with_a_camera(tiny):
    """The edit is guided_inference on the re-projection's rows with their kinds; two runs are byte-identical; the first recorded
    gradient differs from the run without the camera; camera=None is the call without the keyword."""
    dh, gd, t = tiny.dh, tiny.gd, tiny.two
    tfs = [_t(tf) for tf in LOOP_TFS]
    img, disp = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=tfs, camera=CAMERA)
    img, lat = img.clone(), gd.last_latents.clone()
    assert img.shape == (1, 3, RES, RES) and torch.isfinite(img).all()
    (d, c, rows), = _loop_geometry(tiny, [LOOP_TFS], [CAMERA])
    kinds = (rows == 2).to(torch.uint8) * 2
    assert torch.equal(d, disp) and int((rows == 2).sum()) >= 50000 and int((rows == 0).sum()) >= 100 and int((rows == 1).sum()) >= 100
    rec = {}
    ref = gd.guided_inference(t.noise, d, t.null_text, t.prompt, t.acts, c, row_kind=kinds, record=rec)
    assert torch.equal(gd.last_latents, lat) and torch.equal(ref, img)
    again, _ = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=tfs, camera=CAMERA)
    assert torch.equal(again, img) and torch.equal(gd.last_latents, lat)
    # without the camera: another disparity, another first gradient; camera=None is the call without the keyword
    plain, pdisp = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=tfs)
    plain, plat = plain.clone(), gd.last_latents.clone()
    none, ndisp = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=tfs, camera=None)
    assert torch.equal(none, plain) and torch.equal(ndisp, pdisp) and torch.equal(gd.last_latents, plat)
    assert not torch.equal(pdisp, disp)
    from diffusionhandles_amd import depth_transform as DT
    (_, pc), = DT.reproject_object_edits(t.depth, t.bg_depth, t.masks, gd.get_depth_intrinsics(device=dev()), [tfs])
    rec_plain = {}
    gd.guided_inference(t.noise, pdisp, t.null_text, t.prompt, t.acts, pc, record=rec_plain)
    assert torch.equal(gd.last_latents, plat)
    assert torch.isfinite(rec["grad"][0]).all() and not torch.equal(rec["grad"][0], rec_plain["grad"][0])


def test_camera_edit_with_weights_and_the_automatic_gradient_scale(tiny):
    """With object_weights the background is instance 2 of the weighted plan; grad_scale 'auto' takes its bound from the plan."""
    dh, gd, t = tiny.dh, tiny.gd, tiny.two
    tfs = [_t(tf) for tf in LOOP_TFS]
    img, _ = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=tfs, camera=CAMERA)
    img = img.clone()
    (d, c, rows), = _loop_geometry(tiny, [LOOP_TFS], [CAMERA])
    kinds = (rows == 2).to(torch.uint8) * 2
    weighted, _ = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=tfs, camera=CAMERA, object_weights="equal")
    weighted = weighted.clone()
    ref = gd.guided_inference(t.noise, d, t.null_text, t.prompt, t.acts, c, row_kind=kinds, pair_instances=rows,
                              object_weights=[1.0, 1.0, 1.0])
    assert torch.equal(ref, weighted) and not torch.equal(weighted, img)
    old = gd.grad_scale_mode
    gd.grad_scale_mode = "auto"
    try:
        auto, _ = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=tfs, camera=CAMERA, object_weights="equal")
        assert torch.isfinite(auto).all()
        auto, _ = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=tfs, camera=CAMERA)
        assert torch.isfinite(auto).all()
    finally:
        gd.grad_scale_mode = old


def test_camera_refusals_of_the_edit_calls(tiny):
    dh, t = tiny.dh, tiny.two
    tfs = [_t(tf) for tf in LOOP_TFS]
    args = dict(_common(t), fg_masks=t.masks, transforms=tfs, camera=CAMERA)
    with pytest.raises(ValueError, match="at most 7 instances"):
        dh.transform_foreground_objects(**dict(args, transforms=tfs * 4), instances=[0, 1] * 4, object_weights="equal")
    with pytest.raises(ValueError, match="3 entries|one weight per instance and one for the background"):
        dh.transform_foreground_objects(**args, object_weights=[1.0, 1.0])
    with pytest.raises(ValueError, match="transform_foreground_objects: edit 0: camera: rot_axis must not be zero"):
        dh.transform_foreground_objects(**dict(args, camera=(1.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))))
    with pytest.raises(NotImplementedError, match="donor"):
        dh.transform_foreground_objects(**args, donor=dict(depth=t.depth, masks=t.masks, activations=t.acts))
    for key, value, name in (("background_lock", True, "background_lock"), ("depth_transform_footprints", True, "footprints")):
        dh.conf[key] = value
        try:
            with pytest.raises(NotImplementedError, match=name):
                dh.transform_foreground_objects(**args)
            with pytest.raises(NotImplementedError, match=name):
                dh.transform_foreground_objects_batch(**_common(t), fg_masks=t.masks, edits=[tfs], cameras=[CAMERA])
        finally:
            dh.conf.pop(key, None)
    mode = dh.conf["depth_transform_mode"]
    dh.conf["depth_transform_mode"] = "mesh"
    try:
        with pytest.raises(NotImplementedError, match="mesh"):
            dh.transform_foreground_objects(**args)
    finally:
        dh.conf["depth_transform_mode"] = mode


def test_camera_edits_in_a_batch_the_pure_move_and_mixed_batches(tiny):
    """K = 2 with two cameras is guided_inference_batch on the re-projections with the per-edit kinds; the pure camera move
    runs; a camera edit and a plain edit share a transform_foregrounds batch."""
    dh, gd, t = tiny.dh, tiny.gd, tiny.two
    edits = [[_t(tf) for tf in LOOP_TFS], [_t(tf) for tf in SECOND_TFS]]
    cams = [CAMERA, SECOND_CAMERA]
    imgs, disps = dh.transform_foreground_objects_batch(**_common(t), fg_masks=t.masks, edits=edits, cameras=cams)
    imgs, lat = imgs.clone(), gd.last_latents.clone()
    assert imgs.shape == (2, 3, RES, RES) and torch.isfinite(imgs).all()
    rp = _loop_geometry(tiny, [LOOP_TFS, SECOND_TFS], cams, device_correspondences=True)
    assert all(torch.equal(a, b[0]) for a, b in zip(disps, rp)) and not torch.equal(disps[0], disps[1])
    kinds = [(r[2] == 2).to(torch.uint8) * 2 for r in rp]
    assert all(int((k == 2).sum()) >= 50000 for k in kinds)
    ref = gd.guided_inference_batch(t.noise, [r[0] for r in rp], t.null_text, t.prompt, t.acts, [r[1] for r in rp], row_kind=kinds)
    assert torch.equal(ref, imgs) and torch.equal(gd.last_latents, lat)
    # the pure camera move: no mask, no transform, every row a background row
    pure, pdisp = dh.transform_foreground_objects(depth=t.depth, prompt=t.prompt, bg_depth=t.depth, null_text_emb=t.null_text,
                                                  init_noise=t.noise, activations=t.acts, fg_masks=[], transforms=[], camera=CAMERA)
    assert torch.isfinite(pure).all() and torch.isfinite(pdisp).all() and not torch.equal(pdisp, disps[0])
    # edits with and without a camera share a transform_foregrounds batch (and, being of one image, its re-projection call)
    base = dict(depth=t.depth, prompt=t.prompt, bg_depth=t.bg_depth, null_text_emb=t.null_text, init_noise=t.noise,
                activations=t.acts, fg_masks=t.masks)
    both, bd = dh.transform_foregrounds([dict(base, transforms=edits[0], camera=CAMERA), dict(base, transforms=edits[1])])
    assert both.shape == (2, 3, RES, RES) and torch.isfinite(both).all()
    assert torch.equal(bd[0], disps[0])
    _, plain_disp = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=edits[1])
    assert torch.equal(bd[1], plain_disp)
    nocam, _ = dh.transform_foregrounds([dict(base, transforms=edits[0]), dict(base, transforms=edits[1])])
    assert not torch.equal(nocam[0], both[0])


def _run_edit_module():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_edit_tool", os.path.join(root, "tools", "run_edit.py"))
    run_edit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run_edit)
    return run_edit


def test_run_edit_passes_the_camera_of_a_scene_directory(tiny, tmp_path):
    """A two-mask scene whose transforms.json has the entries `plain` and `orbit` (a camera with a pivot pixel): run_scene hands
    the resolved camera to transform_foreground_objects for `orbit` alone; the three refusals come before any identity."""
    import argparse
    import json
    from diffusionhandles_amd import depth_transform as DT
    from diffusionhandles_amd.scene_io import read_png, write_png
    run_edit = _run_edit_module()
    scene = tmp_path / "set" / "two_spheres"
    scene.mkdir(parents=True)
    depth, bg, masks = R.two_spheres(RES)
    np.save(scene / "depth.npy", depth[0, 0].numpy())
    np.save(scene / "bg_depth.npy", bg[0, 0].numpy())
    for m, mask in enumerate(masks):
        write_png(str(scene / f"mask_{m}.png"), mask[0, 0].numpy())
    write_png(str(scene / "input.png"), np.full((RES, RES, 3), 0.5, dtype=np.float32))
    (scene / "prompt.txt").write_text("two spheres on a plane\n")
    member = lambda tf: dict(rotation_angle=tf[0], rotation_axis=list(tf[1]), translation=list(tf[2]))
    objs = [member(LOOP_TFS[0]), member(LOOP_TFS[1])]
    (scene / "transforms.json").write_text(json.dumps({
        "plain": {"objects": objs},
        "orbit": {"objects": objs, "camera": {"rot_angle": 8.0, "pivot_pixel": [RES // 2, RES // 2]}}}))
    args = argparse.Namespace(res=RES, mode="pc", skip_inversion=True, no_identity_cache=False, identity_cache=None, skip_existing=False,
                              max_edits=0, identity_batch=1, edit_batch=1, edit_batch_images=0, background_lock=False)
    seen = []
    dh = tiny.dh
    inner = dh.transform_foreground_objects
    dh.transform_foreground_objects = lambda *a, **kw: (seen.append(kw.get("camera")), inner(*a, **kw))[1]
    try:
        out = tmp_path / "one"
        report = run_edit.run_scene(args, dh.conf, lambda res: dh, str(scene), str(out), None)
    finally:
        del dh.transform_foreground_objects
    assert [e["name"] for e in report["edits"]] == ["plain", "orbit"]
    pivot = DT.pivot_at_pixel(depth.to(dev()), dh.diffuser.get_depth_intrinsics(device=dev()), RES // 2, RES // 2)
    assert seen[0] is None and seen[1] == (8.0, (0.0, 1.0, 0.0), (0.0, 0.0, 0.0), tuple(float(v) for v in pivot))
    plain, orbit = (read_png(str(out / f"{n}_disparity.png")).astype(np.float64) for n in ("plain", "orbit"))
    assert read_png(str(out / "orbit.png")).std() > 0 and (plain != orbit).mean() > 0.01
    # the refusals, before any identity: mesh mode, footprints, the background lock
    called = []
    for kw, name in ((dict(mode="mesh"), "mode mesh"), (dict(footprint_report=dict(footprints=True)), "footprints"),
                     (dict(background_lock=True), "background-lock")):
        bad = argparse.Namespace(**dict(vars(args), **kw))
        with pytest.raises(NotImplementedError, match="moves the camera.*" + name):
            run_edit.run_scene(bad, dh.conf, lambda res: called.append(res), str(scene), str(tmp_path / "refused"), None)
    assert not called


def test_the_host_plan_is_what_the_run_does_and_every_name_is_the_one_call():
    """depth_transform.reproject_plan against the run it plans (DESIGN.md "One host path for the re-projection"), at 64 pixels:
    an instance call with a dropped empty mask, a donor call and a camera call.  The plan's point and row counts and offsets are
    the debug dictionary's, the instance column names survivors only, and the named function returns the bits of `reproject`
    called with the same keywords."""
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    res = 64
    depth, bg, masks = R.two_spheres(res)
    d, b, m = depth.to(dev()), bg.to(dev()), [x.to(dev()) for x in masks]
    tfs = [_t(tf) for tf in S.edits_for(res, depth)[0]]
    donor_depth, donor_masks = I.donor_scene(res, "disjoint")
    donor = dict(donor_depth=donor_depth.to(dev()), donor_masks=[x.to(dev()) for x in donor_masks])
    cam = CM.cameras_for(depth)["pan"]
    calls = [(DT.reproject_instance_edits, RC.INSTANCE, [m[0], torch.zeros_like(m[0]), m[1]], [[tfs[0], tfs[1], tfs[1], tfs[0]]],
              dict(instances=[2, 1, 0, 0], return_instances=True), [0, 2, 3]),
             (DT.reproject_donor_edits, RC.DONOR, m, [tfs + [tfs[0][:3] + (0.8, None)]], donor, [0, 1, 2]),
             (DT.reproject_camera_edits, RC.CAMERA, m, [tfs, tfs], dict(cameras=[cam, None]), [0, 1])]
    for named, call, fg, edits, kw, caller in calls:
        p = DT.reproject_plan(d, fg, edits, **kw)
        assert p.kind == "objects" and RC.fields(p) == call and p.caller == caller
        out, dbg = named(d, b, fg, D.intrinsics_f32(), edits, return_debug=True, **kw)
        assert dbg["vis"].shape[1] == p.n_pts and dbg["corr_dev"].shape[1] == p.cap
        assert np.array_equal(dbg["obj_start"], p.obj_start) and np.array_equal(dbg["inst_start"], p.inst_start)
        for e in range(len(edits)):
            n = int(dbg["counts"][e, 0])
            assert n > 0 and set(dbg["corr_inst"][e, :n].tolist()) <= set(p.caller), (named.__name__, e)
        direct = DT.reproject(d, b, fg, D.intrinsics_f32(), edits, **kw)
        assert len(direct) == len(out) == len(edits)
        for e, (x, y) in enumerate(zip(out, direct)):
            assert len(x) == len(y) == 3 and all(torch.equal(s, t) for s, t in zip(x, y)), (named.__name__, e)
