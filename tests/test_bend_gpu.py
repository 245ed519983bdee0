"""GPU: bend edits (dh_reproject_bend_edits, dh_reproject_bend_ws_bytes, depth_transform.reproject with a `Bend`,
transform_foreground_objects with a `bend_chain`) against the test-side reference tests/bend_ref.py.  Every call of the entry
goes through the C ABI into outputs that are NaN / 0xFF / -1 before it.  The two-sphere scene at res 64 (the smallest the CLOSE
element admits on the bit-row path; 17 workgroups of k_points) and 128.  Helpers of tests/test_camera_moves_gpu.py,
tests/test_object_copies_gpu.py and tests/test_workspace_guards_gpu.py as they are."""
import ctypes
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bend_ref as BR  # noqa: E402
import camera_moves_ref as CM  # noqa: E402
import infill_border_ref as IB  # noqa: E402
import multi_object_ref as R  # noqa: E402
import object_insertion_ref as OI  # noqa: E402
import reproject_calls as RC  # noqa: E402
import similarity_ref as S  # noqa: E402
import test_camera_moves_gpu as CG  # noqa: E402  (helpers only: _setup, _view_rows, _check, _untouched, tiny, _common)
import test_object_copies_gpu as OC  # noqa: E402  (helpers only: _rows, _t)
import test_workspace_guards_gpu as WG  # noqa: E402  (helpers only: _reproject)

pytestmark = pytest.mark.gpu
dev = CG.dev
_t = OC._t
Y = R.Y
Z = (0.0, 0.0, 1.0)
Z0 = (0.0, 0.0, 0.0)
ALL = CG.OUTPUTS + ("bg_corr", "bg_counts")


def _ws_bytes(query, *sizes):
    from diffusionhandles_amd import _lib
    nb = ctypes.c_size_t()
    _lib.check(getattr(_lib.lib(), query)(*sizes, ctypes.byref(nb)), query)
    return nb.value


def _pack(masks_np, inst, edits, B):
    """Reference-side edits (K lists of N tuples / bend_ref.Bend) -> rows [K * N * B, 16] f64, padded with copies of bone 0, and
    the weights [K, n_pts, B] f32 by point-list position (an ordinary transform: 1 on bone 0; the padding: 0)."""
    flat, ws = [], []
    for tfs in edits:
        per = []
        for n, tf in enumerate(tfs):
            m = masks_np[inst[n]].reshape(-1)
            bones = list(tf.bones) if isinstance(tf, BR.Bend) else [tf]
            flat += bones + [bones[0]] * (B - len(bones))
            w = np.zeros((int(m.sum()), B), dtype=np.float32)
            if isinstance(tf, BR.Bend):
                w[:, :len(bones)] = tf.weights.reshape(len(bones), -1)[:, m].T
            else:
                w[:, 0] = 1.0
            per.append(w)
        ws.append(np.concatenate(per))
    return OC._rows([flat]), np.stack(ws)


def _call(s, rows, inst, n_bones=1, bone_w=None, views=None, has_view=None, vs=0, ratio=0.0, border=0, footprints=0, cap=None,
          entry="bend", ws_bytes=None):
    """dh_reproject_bend_edits (entry="surface": dh_reproject_surface_edits with its own query) on poisoned outputs and a
    poisoned workspace.  bone_w: None, a numpy array [K, n_pts, n_bones] or a device tensor to pass as it is."""
    from diffusionhandles_amd import _lib
    L, res, M = s.L, s.res, s.M
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    N = len(inst)
    K = rows.shape[0] // (N * max(n_bones, 1)) if entry == "bend" and 1 <= n_bones <= 4 else rows.shape[0] // N
    sizes = np.diff(s.obj_start)
    n_pts = int(sum(int(sizes[o]) for o in inst))
    if cap is None:
        cap = res * res if footprints or vs else n_pts
    if ws_bytes is not None:
        nb = ws_bytes
    elif entry == "surface":
        nb = _ws_bytes("dh_reproject_surface_ws_bytes", res, n_pts, K, M, N, 1 if vs == 1 else 0)
    else:
        nb = _ws_bytes("dh_reproject_bend_ws_bytes", res, n_pts, K, M, N, 1 if vs == 1 else 0, footprints, min(max(n_bones, 1), 4))
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev())
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
        bg_counts=torch.full((K,), -1, dtype=torch.int32, device=dev()), n_pts=n_pts, K=K, N=N, ws_bytes=nb)
    if isinstance(bone_w, np.ndarray):
        assert bone_w.shape == (K, n_pts, n_bones) and bone_w.dtype == np.float32
        bone_w = torch.from_numpy(np.ascontiguousarray(bone_w)).to(dev())
    o.bone_w = bone_w
    tab = np.asarray(inst, dtype=np.int32)
    v = None if views is None else np.ascontiguousarray(views, dtype=np.float64)
    h = None if has_view is None else np.ascontiguousarray(has_view, dtype=np.uint8)
    args = (_lib.ptr(s.d), _lib.ptr(s.b), _lib.ptr(s.fg_pix), s.n_fg, M, s.obj_start.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            res, _lib.ptr(s.gx), _lib.ptr(s.gy), s.ifx, s.ify, s.fx, s.fy, K, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            None, _lib.ptr(o.zmap), _lib.ptr(o.raw), _lib.ptr(o.clean), _lib.ptr(o.disp), _lib.ptr(o.vis), _lib.ptr(o.txy),
            _lib.ptr(o.corr), _lib.ptr(o.counts), _lib.ptr(ws), nb, s.st, footprints, 0.0, cap, N,
            tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _lib.ptr(o.inst), _lib.ptr(s.donor), s.n_host if s.donor is not None else M,
            None if v is None else v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            None if h is None else h.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), _lib.ptr(s.bg_valid), _lib.ptr(o.bg_corr),
            _lib.ptr(o.bg_counts), border, vs, ratio)
    if entry == "surface":
        o.rc = L.dh_reproject_surface_edits(*args)
    else:
        o.rc = L.dh_reproject_bend_edits(*args, n_bones, None if bone_w is None else _lib.ptr(bone_w))
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
            assert 0 < n <= cap and bool((o.corr[e, n:] == -1).all()) and bool((o.inst[e, n:] == 0xFF).all()), "a row past the count"
            assert int(o.corr[e, :n].min()) >= 0 and int(o.corr[e, :n].max()) < res and int(o.inst[e, :n].max()) < N
    return o


def _all_bytes(a, b, what):
    for k in ALL:
        x, y = getattr(a, k).contiguous().view(torch.uint8), getattr(b, k).contiguous().view(torch.uint8)
        assert torch.equal(x, y), f"{what}: {k}"


def _check(o, e, ref, what, any_view):
    """tests/test_camera_moves_gpu.py's _check: every integer output bit-exact (rows with their order), the disparity within its
    2e-3.  A call without a view leaves the background rows and their counts as they were."""
    if not any_view:
        assert o.bg_h[e] == -1 and bool((o.bg_corr[e] == -1).all()), f"{what}: background rows written without a view"
        o.bg_h[e] = 0
    CG._check(o, e, ref, what)


# ---- the cases of the parity test: built once per (name, res), the reference's in-fill included --------------------------------
def _pivot(depth, x, y):
    from oracle import depth_ref as D
    return tuple(float(v) for v in D.unproject(depth[0, 0].numpy())[y, x])


def _sphere_line(res, sphere):
    """A vertical line through the centre of sphere `sphere` ((x, y) pixels) and the pixel of its centre."""
    cx, cy, rad, _ = R.SPHERES[sphere]
    k = res / 512.0
    x, y = int(cx * k), int(cy * k)
    return (x, int((cy - rad) * k)), (x, int((cy + rad) * k)), (x, y)


@functools.lru_cache(maxsize=None)
def case(name, res):
    """-> SimpleNamespace(depth, bg, masks (host), donor, inst, edits (K lists of N tuples / Bend), B, cams, vs, border, footprints,
    refs (K reference results))."""
    depth, bg, masks = R.two_spheres(res)
    base = S.edits_for(res, depth)[0]
    p0, p1, (cx, cy) = _sphere_line(res, 0)
    q0, q1, (dx, dy) = _sphere_line(res, 1)
    piv0, piv1 = _pivot(depth, cx, cy), _pivot(depth, dx, dy)
    width = res / 8.0
    c = SimpleNamespace(depth=depth, bg=bg, masks=masks, donor=None, inst=[0, 1], cams=None, vs=0, border=0, footprints=0)
    if name == "scale":          # K = 1, B = 2: the second bone a similarity with a scale and its own pivot
        w = BR.chain_weights((res, res), p0, p1, width, 2)
        bend = BR.Bend([(0.0, Y, Z0), (35.0, Z, (0.05, 0.0, -0.1), (1.2, 0.9, 1.0), piv0)], w)
        c.edits, c.B = [[bend, base[1]]], 2
    elif name == "copies":       # K = 3, B = 4: two copies of mask 0 bent differently (4 bones; 2 bones, padded), sphere 1 rigid or bent
        c.inst = [0, 0, 1]
        four = BR.chain(depth, masks[0], p0, p1, width, 60.0, Z, (0.0, -0.1, 0.0), piv0, 4)
        two = BR.chain(depth, masks[0], p1, p0, width * 2, -40.0, Y, (0.0, 0.9, 0.2), None, 2)
        three = BR.chain(depth, masks[1], q0, q1, width, 45.0, Z, Z0, piv1, 3)
        c.edits = [[four, two, base[1]], [two, four, three], [base[0], (25.0, Y, (0.0, -0.9, 0.3)), three]]
        c.B = 4
    elif name == "footprints":   # K = 1, B = 2: the triangles stretch over the outside of the bend
        c.footprints = 1
        c.edits, c.B = [[BR.chain(depth, masks[0], p0, p1, width, 50.0, Z, Z0, piv0, 2), base[1]]], 2
    elif name == "surfaces":     # K = 3, B = 4: two edits under a camera with view surfaces, one without a view
        cams = CM.cameras_for(depth)
        c.cams, c.vs = [cams["general"], None, cams["dolly_in"]], 1
        four = BR.chain(depth, masks[1], q0, q1, width, 60.0, Z, Z0, piv1, 4)
        two = BR.chain(depth, masks[0], p0, p1, width, 30.0, Z, Z0, piv0, 2)
        c.edits, c.B = [[base[0], four], [two, four], [two, base[1]]], 4
    elif name == "reflect":      # K = 1, B = 2 under a camera (the in-fill reaches the frame), the reflecting border
        c.cams, c.border = [CM.cameras_for(depth)["truck"]], 1
        c.edits, c.B = [[BR.chain(depth, masks[0], p0, p1, width, 40.0, Z, Z0, piv0, 2), base[1]]], 2
    elif name == "donor":        # K = 1, B = 2: the donor's instance is the bent one
        ddepth, dmasks = OI.donor_scene(res, "overlap")
        c.bg = torch.where(masks[1] > 0, depth, bg)
        c.masks, c.donor = [masks[0]], (ddepth, list(dmasks))
        c.inst = list(range(1 + len(dmasks)))
        dm = dmasks[0][0, 0].numpy() != 0
        ys, xs = np.nonzero(dm)
        mid = (int(xs.mean()), int(ys.mean()))
        bend = BR.chain(ddepth, dmasks[0], (mid[0], int(ys.min())), (mid[0], int(ys.max())), width, 45.0, Z, (0.0, 0.0, -0.1),
                        _pivot(ddepth, *mid), 2)
        c.edits, c.B = [[base[0], bend] + [(0.0, Y, Z0)] * (len(dmasks) - 1)], 2
    else:
        raise KeyError(name)
    refs = []
    for e, tfs in enumerate(c.edits):
        cam = None if c.cams is None else c.cams[e]
        ref = BR.transform_bend(c.depth, c.bg, c.masks, c.inst, tfs, camera=cam, footprints=bool(c.footprints),
                                view_surfaces=bool(c.vs), donor=c.donor)
        if c.border:
            ref = (torch.from_numpy(IB.camera_fill(ref, "reflect"))[None, None], ref[1], ref[2])
        refs.append(ref)
    c.refs = refs
    return c


def _run_case(c):
    s = CG._setup(c.depth, c.bg, c.masks, donor=c.donor)
    all_masks = [m[0, 0].numpy() != 0 for m in list(c.masks) + ([] if c.donor is None else list(c.donor[1]))]
    rows, w = _pack(all_masks, c.inst, c.edits, c.B)
    views, has = (None, None) if c.cams is None else CG._view_rows(c.cams)
    return s, rows, w, _call(s, rows, c.inst, c.B, w, views, has, vs=c.vs, border=c.border, footprints=c.footprints)


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scale", "copies", "footprints", "surfaces", "reflect", "donor"])
@pytest.mark.parametrize("res", [64, 128])
def test_bend_edits_against_the_reference(res, name):
    """raw_mask, clean_mask, vis, target_xy, corr, corr_inst, counts[0..2], bg_corr, bg_counts and zmap bit-equal to bend_ref (row
    order included); the disparity within the project's 2e-3 (tests/test_camera_moves_gpu.py, _check)."""
    c = case(name, res)
    _, _, w, o = _run_case(c)
    assert o.rc == 0, o.err
    assert w.shape[2] == c.B and any(isinstance(tf, BR.Bend) for tfs in c.edits for tf in tfs)
    for e, ref in enumerate(c.refs):
        _check(o, e, ref, f"res {res} {name} edit {e}", c.cams is not None)
    if name == "footprints":
        # the bend is not the rigid edit: the rows differ from those of bone 1 alone
        rigid = BR.transform_bend(c.depth, c.bg, c.masks, c.inst, [c.edits[0][0].bones[1], c.edits[0][1]], footprints=True, infill=False)
        assert not np.array_equal(rigid[2]["raw_mask"], c.refs[0][2]["raw_mask"])


# ---- 2. the call without bones, and bones that change nothing ------------------------------------------------------------------
@pytest.mark.parametrize("res", [64, 128])
def test_one_bone_without_weights_is_the_surface_entry(res):
    """n_bones = 1, bone_w = NULL: every output byte of dh_reproject_surface_edits and its workspace size -- K = 3 mixing two
    views (with view surfaces) and none; then the point path with footprints."""
    depth, bg, masks = R.two_spheres(res)
    edits = S.edits_for(res, depth)[:3]
    cams = CM.cameras_for(depth)
    views, has = CG._view_rows([cams["general"], None, cams["dolly_in"]])
    s = CG._setup(depth, bg, masks)
    rows = OC._rows(edits)
    for kw in (dict(views=views, has_view=has, vs=1), dict(views=views, has_view=has, vs=0, border=1), dict()):
        a = _call(s, rows, [0, 1], entry="surface", **kw)
        b = _call(s, rows, [0, 1], 1, None, **kw)
        assert a.rc == 0 and b.rc == 0, (a.err, b.err)
        assert a.ws_bytes == b.ws_bytes
        _all_bytes(a, b, f"res {res} {sorted(kw)}")
    nb = _ws_bytes("dh_reproject_camera_workspace_bytes", res, int(s.n_fg), 3, 2, 2, 1)
    a = _call(s, rows, [0, 1], entry="surface", footprints=1, ws_bytes=nb)
    b = _call(s, rows, [0, 1], 1, None, footprints=1)
    assert a.rc == 0 and b.rc == 0, (a.err, b.err)
    assert b.ws_bytes == nb
    _all_bytes(a, b, f"res {res} footprints")


@pytest.mark.parametrize("res", [64, 128])
def test_padded_rigid_instances_are_the_plain_call(res):
    """B = 4, every instance one-hot on bone 0 and padded with copies of it -- and all weights 0, which is bone 0 with weight 1;
    bones 1 .. 3 OTHER rows at weight 0: the outputs of the plain call, byte for byte.  B = 1 with weights (1) likewise."""
    depth, bg, masks = R.two_spheres(res)
    four = S.edits_for(res, depth)
    edits = four[:3]
    s = CG._setup(depth, bg, masks)
    plain = _call(s, OC._rows(edits), [0, 1], entry="surface")
    assert plain.rc == 0, plain.err
    n_pts = plain.n_pts
    w = np.zeros((3, n_pts, 4), dtype=np.float32)
    w[:, :, 0] = 1.0
    padded = OC._rows([[tf for tfs in edits for tf in tfs for _ in range(4)]])
    other = OC._rows([[b for tfs in edits for tf in tfs for b in (tf, (70.0, Z, (0.3, 0.2, 0.1)), four[3][1], (5.0, Y, Z0, 2.0, None))]])
    for what, rows, ww in (("one-hot, padded", padded, w), ("all weights zero", padded, np.zeros_like(w)), ("other rows at weight 0", other, w)):
        o = _call(s, rows, [0, 1], 4, ww)
        assert o.rc == 0, o.err
        for k in CG.OUTPUTS:
            assert torch.equal(getattr(o, k).contiguous().view(torch.uint8), getattr(plain, k).contiguous().view(torch.uint8)), (what, k)
    one = _call(s, OC._rows(edits), [0, 1], 1, np.ones((3, n_pts, 1), dtype=np.float32))
    assert one.rc == 0, one.err
    _all_bytes(one, plain, "B = 1 with weights")
    # the growth of the workspace: only the device copy of the extra rows (K * N * (B - 1) rows of 128 bytes, 256-aligned takes)
    extra = o.ws_bytes - plain.ws_bytes
    assert 3 * 2 * 3 * 128 <= extra < 3 * 2 * 3 * 128 + 256, extra


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    c = case("scale", 64)
    s = CG._setup(c.depth, c.bg, c.masks)
    all_masks = [m[0, 0].numpy() != 0 for m in c.masks]
    rows, w = _pack(all_masks, c.inst, c.edits, 2)
    good = _call(s, rows, c.inst, 2, w)
    assert good.rc == 0, good.err
    wd = torch.from_numpy(w).to(dev())
    big = torch.zeros(w.size + 4, dtype=torch.float32, device=dev())
    nan = float("nan")

    def broken(row, k, value):
        r = rows.copy()
        r[row, k] = value
        return r
    last = rows.shape[0] - 1
    for what, kw in (("n_bones 0", dict(n_bones=0, bone_w=wd)), ("n_bones 5", dict(n_bones=5, bone_w=wd)),
                     ("n_bones -1", dict(n_bones=-1, bone_w=wd)), ("n_bones 2 without weights", dict(n_bones=2, bone_w=None)),
                     ("weights off a 16-byte boundary", dict(n_bones=2, bone_w=big[1:])),
                     ("a scale of 0 in bone 1", dict(n_bones=2, bone_w=wd, rows=broken(1, 8, 0.0))),
                     ("a NaN pivot in the last bone", dict(n_bones=2, bone_w=wd, rows=broken(last, 12, nan))),
                     ("a has-pivot flag of 2 in the last bone", dict(n_bones=2, bone_w=wd, rows=broken(last, 14, 2.0))),
                     ("footprints with view surfaces", dict(n_bones=2, bone_w=wd, footprints=1, vs=1, ws_bytes=good.ws_bytes)),
                     ("half the workspace", dict(n_bones=2, bone_w=wd, ws_bytes=good.ws_bytes // 2))):
        kw = dict(kw)
        o = _call(s, kw.pop("rows", rows), c.inst, **kw)
        assert o.rc == CG.DH_ERR_ARG and o.err, what
        CG._untouched(o)
    from diffusionhandles_amd import _lib
    L = _lib.lib()
    nb = ctypes.c_size_t(12345)
    for sizes in ((64, 100, 1, 1, 1, 0, 0, 0), (64, 100, 1, 1, 1, 0, 0, 5), (64, 100, 1, 1, 1, 2, 0, 1), (64, 100, 1, 1, 1, 1, 1, 2),
                  (64, 100, 1, 1, 9, 0, 0, 1)):
        assert L.dh_reproject_bend_ws_bytes(*sizes, ctypes.byref(nb)) == CG.DH_ERR_ARG and nb.value == 12345, sizes
    assert _ws_bytes("dh_reproject_bend_ws_bytes", 64, 100, 2, 2, 3, 1, 0, 1) == _ws_bytes("dh_reproject_surface_ws_bytes", 64, 100, 2, 2, 3, 1)
    assert _ws_bytes("dh_reproject_bend_ws_bytes", 64, 100, 2, 2, 3, 0, 0, 1) == _ws_bytes("dh_reproject_surface_ws_bytes", 64, 100, 2, 2, 3, 0)


# ---- 4. guard bands and stale workspaces ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["points", "footprints", "views"])
def test_guard_bands_and_stale_workspaces(monkeypatch, what):
    """tests/test_workspace_guards_gpu.py's four runs (three fills and a plain call) of depth_transform.reproject with a Bend at
    64: no byte outside the buffers, no byte of the arena's gaps, the same digest from a workspace full of stale bytes."""
    from diffusionhandles_amd import depth_transform as DT
    res = 64
    depth, bg, masks = R.two_spheres(res)
    p0, p1, (cx, cy) = _sphere_line(res, 0)
    mk = lambda bones, angle: DT.Bend(BR.chain(depth, masks[0], p0, p1, 8.0, angle, Z, Z0, _pivot(depth, cx, cy), bones).bones,
                                      torch.from_numpy(BR.chain_weights((res, res), p0, p1, 8.0, bones)))
    edits = [[mk(4, 60.0), WG.THREE[0][1]], [WG.THREE[1][0], WG.THREE[1][1]], [mk(2, -30.0), WG.THREE[2][1]]]
    kw = {}
    if what == "footprints":
        kw = dict(footprints=True)
    if what == "views":
        c = CM.cameras_for(depth)
        kw = dict(cameras=[c["general"], None, c["dolly_in"]], view_surfaces=True)
    counts = WG._reproject(monkeypatch, dev(), depth, bg, masks, edits, **kw)
    assert int(counts[:, 0].min()) > 0
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd import losses as LS
    import guarded as G
    G.arena_reset(_lib.lib())
    LS._WS.clear()


# ---- 5. the host call and the edit call ----------------------------------------------------------------------------------------
def test_host_call_against_the_reference_and_an_unbent_call_is_the_call_it_was():
    """depth_transform.reproject with Bends (the rows and weights the host plan builds: padding, the gather at fg_pix) gives the
    reference's rows; without a Bend the plan names the entry it named and the results are those of reproject_surface_edits."""
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    c = case("copies", 64)
    to_dt = lambda tf: DT.Bend([_t(b) for b in tf.bones], tf.weights) if isinstance(tf, BR.Bend) else _t(tf)
    args = (c.depth.to(dev()), c.bg.to(dev()), [m.to(dev()) for m in c.masks], D.intrinsics_f32())
    res_list = DT.reproject_bend_edits(*args, [[to_dt(tf) for tf in tfs] for tfs in c.edits], instances=c.inst, return_instances=True)
    for e, ref in enumerate(c.refs):
        disp, corr, inst = res_list[e]
        assert torch.equal(corr, ref[1]) and np.array_equal(inst.numpy(), ref[2]["corr_inst"]), e
        assert float((disp[0, 0].cpu() - ref[0][0, 0]).abs().max()) < 2e-3, e
    plain = [[_t(tf) for tf in tfs] for tfs in S.edits_for(64, c.depth)[:2]]
    a = DT.reproject_surface_edits(*args, plain)
    b = DT.reproject_bend_edits(*args, plain)
    for x, y in zip(a, b):
        assert all(torch.equal(u, v) for u, v in zip(x, y))
    assert RC.fields(DT.reproject_plan(c.depth, c.masks, plain)) == RC.FOOTPRINT


tiny = CG.tiny


def test_transform_foreground_objects_with_a_bend_chain(tiny, monkeypatch):
    """One edit call with a bend_chain on the synthetic identity: it runs, its outputs are finite, the correspondences are those
    of `reproject`, and the image is guided_inference on them."""
    from diffusionhandles_amd import depth_transform as DT
    dh, gd, t = tiny.dh, tiny.gd, tiny.two
    res = t.depth.shape[-1]
    p0, p1, _ = _sphere_line(res, 0)
    intr = gd.get_depth_intrinsics(device=dev())
    bend = DT.bend_chain(t.depth, intr, t.masks[0], p0, p1, res / 8.0, 50.0, torch.tensor(Z), bones=3)
    tfs = [bend, _t(CG.LOOP_TFS[1])]
    seen = []
    prepare = gd.prepare_guidance

    def spy(depth, prompt, acts, correspondences, *a, **kw):
        seen.append(torch.as_tensor(correspondences).clone())
        return prepare(depth, prompt, acts, correspondences, *a, **kw)
    with monkeypatch.context() as mp:
        mp.setattr(gd, "prepare_guidance", spy)
        img, disp = dh.transform_foreground_objects(**CG._common(t), fg_masks=t.masks, transforms=tfs)
    assert torch.isfinite(img).all() and torch.isfinite(disp).all()
    (rdisp, corr), = DT.reproject(t.depth, t.bg_depth, t.masks, intr, [tfs])
    assert len(seen) == 1 and torch.equal(seen[0].cpu(), corr) and len(corr) > 100
    assert torch.equal(disp, rdisp)
    rigid, _ = dh.transform_foreground_objects(**CG._common(t), fg_masks=t.masks, transforms=[_t(CG.LOOP_TFS[0]), _t(CG.LOOP_TFS[1])])
    assert not torch.equal(rigid, img)
