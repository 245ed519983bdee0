"""GPU: view surfaces (dh_reproject_surface_edits, dh_reproject_surface_background, their workspace queries,
depth_transform.reproject_surface_edits, the conf key depth_transform_view_surfaces of DiffusionHandles) against the test-side
reference tests/view_surfaces_ref.py.  res 64 (the smallest the CLOSE element admits on the bit-row path: one workgroup of
the compaction per 2048 pixels, 31 workgroups of the triangle kernel) and 128; the C entries write into outputs that are NaN /
0xFF / -1 before the call.  Helpers of tests/test_camera_moves_gpu.py and tests/test_workspace_guards_gpu.py as they are."""
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
import object_insertion_ref as OI  # noqa: E402
import similarity_ref as S  # noqa: E402
import test_camera_moves_gpu as CG  # noqa: E402  (helpers only: _setup, _view_rows, _check, _untouched, _same_bytes, tiny)
import test_object_copies_gpu as OC  # noqa: E402  (helpers only: _rows, _t)
import test_workspace_guards_gpu as WG  # noqa: E402  (helpers only: guarded_runs and the re-projection's digest)
import view_surfaces_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu
dev = CG.dev
_t = OC._t
INT_MAX = 2147483647
NAMES = list(CM.CAMERA_NAMES) + ["dolly_in_1", "none"]          # the K = 8 call: six cameras, the dolly in by 1.0, no view


@pytest.fixture(autouse=True)
def hooks_at_their_defaults():
    yield
    from diffusionhandles_amd import _lib
    _lib.lib().dh_dbg_footprint_tier(0)


def _ws_bytes(query, *sizes):
    from diffusionhandles_amd import _lib
    nb = ctypes.c_size_t()
    _lib.check(getattr(_lib.lib(), query)(*sizes, ctypes.byref(nb)), query)
    return nb.value


def _call(s, rows, inst, views=None, has_view=None, vs=1, ratio=0.0, border=0, entry="surface", footprints=0, fp_ratio=0.0, cap=None):
    """dh_reproject_surface_edits (or, entry="border", dh_reproject_border_edits with the camera query's workspace) on poisoned
    outputs; cap: the correspondence capacity (default: res * res)."""
    from diffusionhandles_amd import _lib
    L, res, M = s.L, s.res, s.M
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    N = len(inst)
    K = rows.shape[0] // N
    sizes = np.diff(s.obj_start)
    n_pts = int(sum(int(sizes[o]) for o in inst))
    cap = res * res if cap is None else cap
    if entry == "border":
        nb = _ws_bytes("dh_reproject_camera_workspace_bytes", res, n_pts, K, M, N, footprints)
    else:
        nb = _ws_bytes("dh_reproject_surface_ws_bytes", res, n_pts, K, M, N, 1 if vs == 1 else 0)
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
    tab = np.asarray(inst, dtype=np.int32)
    v = None if views is None else np.ascontiguousarray(views, dtype=np.float64)
    h = None if has_view is None else np.ascontiguousarray(has_view, dtype=np.uint8)
    args = (_lib.ptr(s.d), _lib.ptr(s.b), _lib.ptr(s.fg_pix), s.n_fg, M, s.obj_start.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            res, _lib.ptr(s.gx), _lib.ptr(s.gy), s.ifx, s.ify, s.fx, s.fy, K, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            None, _lib.ptr(o.zmap), _lib.ptr(o.raw), _lib.ptr(o.clean), _lib.ptr(o.disp), _lib.ptr(o.vis), _lib.ptr(o.txy),
            _lib.ptr(o.corr), _lib.ptr(o.counts), _lib.ptr(ws), nb, s.st, footprints, fp_ratio, cap, N,
            tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _lib.ptr(o.inst), _lib.ptr(s.donor), s.n_host if s.donor is not None else M,
            None if v is None else v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            None if h is None else h.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), _lib.ptr(s.bg_valid), _lib.ptr(o.bg_corr),
            _lib.ptr(o.bg_counts), border)
    o.rc = L.dh_reproject_border_edits(*args) if entry == "border" else L.dh_reproject_surface_edits(*args, vs, ratio)
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
            assert 0 <= n <= cap and bool((o.corr[e, n:] == -1).all()) and bool((o.inst[e, n:] == 0xFF).all()), "a row past the count"
            if n:
                assert int(o.corr[e, :n].min()) >= 0 and int(o.corr[e, :n].max()) < res and int(o.inst[e, :n].max()) < N
    return o


def _all_bytes(a, b, what):
    """Every output of two calls, the background rows and their counts included, byte for byte."""
    for k in CG.OUTPUTS + ("bg_corr", "bg_counts"):
        x, y = getattr(a, k).contiguous().view(torch.uint8), getattr(b, k).contiguous().view(torch.uint8)
        assert torch.equal(x, y), f"{what}: {k}"


def _scene(res, instances=(0, 1), removed=False):
    """The fixture of the reference and the device inputs and rows of its K = 8 call."""
    fx = V.fixture(res, tuple(instances), removed)
    s = CG._setup(fx["depth"], fx["bg_depth"], fx["masks"], removed=fx["removed"])
    cams = [fx["cameras"].get(n) for n in NAMES]
    views, has = CG._view_rows(cams)
    rows = np.tile(OC._rows([fx["transforms"]]), (len(NAMES), 1))
    return fx, s, rows, views, has


# ---- 1. the setting off is the border entry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", [0, 1])
def test_flag_zero_is_the_border_entry(border):
    """K = 3 mixing two views and none: view_surfaces = 0 through the new entry, every output byte and the workspace size."""
    depth, bg, masks = R.two_spheres(64)
    edits = S.edits_for(64, depth)[:3]
    c = CM.cameras_for(depth)
    views, has = CG._view_rows([c["general"], None, c["dolly_in"]])
    s = CG._setup(depth, bg, masks)
    rows = OC._rows(edits)
    n_pts = int(s.n_fg)
    base = _call(s, rows, [0, 1], views, has, border=border, entry="border", cap=n_pts)
    new = _call(s, rows, [0, 1], views, has, vs=0, border=border, cap=n_pts)
    assert base.rc == 0 and new.rc == 0, (base.err, new.err)
    assert new.ws_bytes == base.ws_bytes
    _all_bytes(new, base, f"border {border}")
    assert base.bg_h[1] == 0 and base.bg_h[0] > 0
    # the setting on, no edit with a view: the same call (launch for launch: nothing of the larger workspace is carved)
    plain = _call(s, rows, [0, 1], None, None, border=border, entry="border", cap=n_pts)
    on = _call(s, rows, [0, 1], views, np.zeros(3, dtype=np.uint8), vs=1, border=border, cap=n_pts)
    assert plain.rc == 0 and on.rc == 0, (plain.err, on.err)
    _all_bytes(on, plain, f"border {border}, the setting on without a view")
    # the background entry
    bg_valid = torch.ones(64 * 64, dtype=torch.uint8, device=dev())
    a = _background(bg, views[0], bg_valid, entry="border", border=border)
    b = _background(bg, views[0], bg_valid, vs=0, border=border)
    assert a.rc == 0 and b.rc == 0, (a.err, b.err)
    assert a.ws_bytes == b.ws_bytes == _ws_bytes("dh_reproject_background_workspace_bytes", 64)
    for k in ("zmap", "disp", "counts", "bg_corr", "bg_counts"):
        assert torch.equal(getattr(a, k).view(torch.uint8), getattr(b, k).view(torch.uint8)), k


# ---- 2. against the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["two_objects", "copies", "removed"])
@pytest.mark.parametrize("res", [64, 128])
def test_eight_edits_against_the_reference(res, what):
    """K = 8 in one call -- the six fixture cameras, the dolly in by 1.0 and one edit without a view -- with no pixel excluded:
    corr, corr_inst, bg_corr, both counts, zmap, both masks, vis and target_xy bit-exact (row order included), the disparity
    within 2e-3 (of 255).  copies: instances [0, 0, 1]; removed: sphere 1 is a removed mask."""
    inst = (0, 0, 1) if what == "copies" else (0, 1)
    fx, s, rows, views, has = _scene(res, inst, what == "removed")
    o = _call(s, rows, fx["instances"], views, has)
    assert o.rc == 0, o.err
    worst = 0.0
    for e, name in enumerate(NAMES):
        ref = fx["geo"][name]
        CG._check(o, e, ref, f"res {res} {what} {name}")
        worst = max(worst, float((o.disp[e].cpu() - ref[0][0, 0]).abs().max()))
        if name != "none":
            g = ref[2]
            assert g["n_background"] > 0 and g["n_instance_rows"] > 0
    print(f"res {res} {what}: disparity max abs err over the 8 edits {worst:.3e} (bound 2e-3)")
    # the edit without a view is the point path, byte for byte: the border entry's call of that edit alone
    e = NAMES.index("none")
    one = _call(s, rows[e * len(fx["instances"]):(e + 1) * len(fx["instances"])], fx["instances"], None, None, entry="border")
    assert one.rc == 0, one.err
    CG._same_bytes(o, e, one, 0, f"res {res} {what}: the edit without a view")
    assert o.bg_h[e] == 0 and bool((o.bg_corr[e] == -1).all())
    # fewer unowned pixels than the points leave, and no background seen through an instance: the counts of the reference
    if what == "two_objects" and res == 128:
        unowned = {n: int(fx["geo"][n][2]["unowned"].sum()) for n in NAMES[:-1]}
        assert unowned["dolly_in"] == 0 and unowned["dolly_in_1"] == 0 and unowned["dolly_out"] == 1806, unowned


def test_host_call_against_the_reference():
    """depth_transform.reproject_surface_edits: the instance rows, then the background rows with instance index N; the ratio."""
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    fx = V.fixture(64)
    cams = [fx["cameras"].get(n) for n in NAMES]
    args = (fx["depth"].to(dev()), fx["bg_depth"].to(dev()), [m.to(dev()) for m in fx["masks"]], D.intrinsics_f32(),
            [[_t(tf) for tf in fx["transforms"]]] * len(NAMES))
    res_list, dbg = DT.reproject_surface_edits(*args, cameras=cams, view_surfaces=True, return_debug=True)
    for e, name in enumerate(NAMES):
        disp, corr, inst = res_list[e]
        ref = fx["geo"][name]
        assert torch.equal(corr, ref[1]) and np.array_equal(inst.numpy(), ref[2]["corr_inst"]), name
        assert dbg["n_background"][e] == ref[2]["n_background"], name
        assert float((disp[0, 0].cpu() - ref[0][0, 0]).abs().max()) < 2e-3, name
    # a ratio reaches the kernels: the orbit with ratio 1.02 against the reference with it
    ref = V.transform_surfaces(fx["depth"], fx["bg_depth"], fx["masks"], [0, 1], fx["transforms"], fx["cameras"]["orbit"], (), True, 1.02,
                               infill=False)
    (_, corr, inst), = DT.reproject_surface_edits(*args[:4], args[4][:1], cameras=[fx["cameras"]["orbit"]], view_surfaces=True,
                                                  view_surface_max_ratio=1.02)
    assert torch.equal(corr, ref[1]) and not torch.equal(corr, fx["geo"]["orbit"][1])
    # off, and on without a camera: the calls they were
    off = DT.reproject_border_edits(*args, cameras=cams)
    same = DT.reproject_surface_edits(*args, cameras=cams, view_surfaces=False)
    for a, b in zip(off, same):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    plain = DT.reproject_border_edits(*args)
    same = DT.reproject_surface_edits(*args, view_surfaces=True)
    for a, b in zip(plain, same):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 3. tiers and repeats ------------------------------------------------------------------------------------------------------
def test_tier_thresholds_and_a_second_call_give_the_same_bytes():
    """The thread tier draws boxes up to the threshold, the wave tier the rest: 1 (every triangle with more than one candidate
    on the wave tier's list), the default and INT_MAX (no list) give the same bytes; so does a second call."""
    from diffusionhandles_amd import _lib
    fx, s, rows, views, has = _scene(64)
    L = _lib.lib()
    first = _call(s, rows, fx["instances"], views, has)
    assert first.rc == 0, first.err
    again = _call(s, rows, fx["instances"], views, has)
    _all_bytes(again, first, "a second call")
    for tier in (1, INT_MAX):
        assert L.dh_dbg_footprint_tier(tier) == 0
        o = _call(s, rows, fx["instances"], views, has)
        assert o.rc == 0, o.err
        _all_bytes(o, first, f"tier {tier}")
    assert L.dh_dbg_footprint_tier(0) == 0


# ---- 4. the background entry ---------------------------------------------------------------------------------------------------
def _background(bg, view, bg_valid, vs=1, ratio=0.0, border=0, entry="surface"):
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    L = _lib.lib()
    res = bg.shape[-1]
    b = bg.to(dev(), torch.float32).contiguous()
    gx, gy = DT._grids(res, res, dev())
    intr = D.intrinsics_f32()
    ifx, ify = DT._inv_focal(intr)
    if entry == "border":
        nb = _ws_bytes("dh_reproject_background_workspace_bytes", res)
    else:
        nb = _ws_bytes("dh_reproject_surface_background_ws_bytes", res, 1 if vs == 1 else 0)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev())
    o = SimpleNamespace(zmap=torch.full((res, res), float("nan"), device=dev()), disp=torch.full((res, res), float("nan"), device=dev()),
                        counts=torch.full((4,), -1, dtype=torch.int32, device=dev()),
                        bg_corr=torch.full((res * res, 4), -1, dtype=torch.int64, device=dev()),
                        bg_counts=torch.full((1,), -1, dtype=torch.int32, device=dev()), ws_bytes=nb)
    v = None if view is None else np.ascontiguousarray(view, dtype=np.float64)
    args = (_lib.ptr(b), res, _lib.ptr(gx), _lib.ptr(gy), ifx, ify, float(intr[0, 0]), float(intr[1, 1]), None, _lib.ptr(o.zmap),
            _lib.ptr(o.disp), _lib.ptr(o.counts), _lib.ptr(ws), nb, _lib.stream_ptr(),
            None if v is None else v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _lib.ptr(bg_valid), _lib.ptr(o.bg_corr),
            _lib.ptr(o.bg_counts), border)
    o.rc = L.dh_reproject_border_background(*args) if entry == "border" else L.dh_reproject_surface_background(*args, vs, ratio)
    o.err = L.dh_last_error().decode() if o.rc != 0 else ""
    torch.cuda.synchronize()
    return o


def _background_untouched(o):
    assert torch.isnan(o.zmap).all() and torch.isnan(o.disp).all() and bool((o.counts == -1).all())
    assert bool((o.bg_corr == -1).all()) and bool((o.bg_counts == -1).all())


@pytest.mark.parametrize("camera", ["truck", "dolly"])
@pytest.mark.parametrize("ratio", [None, 1.1])
def test_step_background_through_the_background_entry(ratio, camera):
    """The pure camera move over the stepped background at 64: without a ratio the sheet bridges the step, with 1.1 it is cut."""
    res = 64
    bg = V.step_background(res)
    cam = V.STEP_TRUCK if camera == "truck" else V.STEP_DOLLY
    disp_r, corr_r, g = V.background_surfaces(bg, cam, max_ratio=ratio)
    assert int(g["unowned"].sum()) == {("truck", None): 320, ("truck", 1.1): 384, ("dolly", None): 0, ("dolly", 1.1): 18}[camera, ratio]
    views, _ = CG._view_rows([cam])
    bg_valid = torch.ones(res * res, dtype=torch.uint8, device=dev())
    o = _background(bg, views[0], bg_valid, ratio=0.0 if ratio is None else ratio)
    assert o.rc == 0, o.err
    nb = int(o.bg_counts[0])
    c = o.counts.tolist()
    assert nb == g["n_background"] == len(corr_r) and np.array_equal(o.bg_corr[:nb].cpu().numpy(), corr_r.numpy())
    assert bool((o.bg_corr[nb:] == -1).all())
    assert np.array_equal(o.zmap.cpu().numpy(), g["zmap"])
    assert c[0] == 0 and c[1] == 0 and c[2] == int(g["inpaint"].sum()) == int(g["unowned"].sum()) and c[3] >= 0
    err = float((o.disp.cpu() - disp_r[0, 0]).abs().max())
    print(f"step {camera} ratio {ratio}: {nb} rows, {c[2]} in-fill pixels, disparity max abs err {err:.2e}")
    assert err < 2e-3


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    fx, s, rows, views, has = _scene(64)
    inst = fx["instances"]
    nan, inf = float("nan"), float("inf")
    for what, kw in (("flag 2", dict(vs=2)), ("flag -1", dict(vs=-1)), ("ratio 1", dict(ratio=1.0)), ("ratio 0.5", dict(ratio=0.5)),
                     ("ratio -2", dict(ratio=-2.0)), ("ratio nan", dict(ratio=nan)), ("ratio inf", dict(ratio=inf)),
                     ("ratio without the flag", dict(vs=0, ratio=1.5)), ("footprints", dict(footprints=1)),
                     ("capacity", dict(cap=64 * 64 - 1))):
        o = _call(s, rows, inst, views, has, **kw)
        assert o.rc == CG.DH_ERR_ARG and o.err, what
        CG._untouched(o)
    # the capacity is the point path's where no edit has a view
    o = _call(s, rows, inst, views, np.zeros(len(NAMES), dtype=np.uint8), cap=int(s.n_fg))
    assert o.rc == 0, o.err
    # a donor mask
    depth, bg, masks = R.two_spheres(64)
    ddepth, dmasks = OI.donor_scene(64, "overlap")
    host_bg = torch.where(masks[1] > 0, depth, bg)
    sd = CG._setup(depth, host_bg, [masks[0]], donor=(ddepth, dmasks))
    rows_d = OC._rows([[(0.0, R.Y, (0.0, 0.0, 0.0))] * sd.M])
    v1, h1 = CG._view_rows([fx["cameras"]["pan"]])
    for hv in (h1, np.zeros(1, dtype=np.uint8)):          # (refused whether or not an edit has a view)
        o = _call(sd, rows_d, list(range(sd.M)), v1, hv)
        assert o.rc == CG.DH_ERR_ARG and "donor" in o.err
        CG._untouched(o)
    # the queries and the background entry
    from diffusionhandles_amd import _lib
    L = _lib.lib()
    nb = ctypes.c_size_t(12345)
    assert L.dh_reproject_surface_ws_bytes(64, 100, 1, 1, 1, 2, ctypes.byref(nb)) == CG.DH_ERR_ARG and nb.value == 12345
    assert L.dh_reproject_surface_background_ws_bytes(64, -1, ctypes.byref(nb)) == CG.DH_ERR_ARG and nb.value == 12345
    bg_valid = torch.ones(64 * 64, dtype=torch.uint8, device=dev())
    for what, kw in (("flag 2", dict(vs=2)), ("ratio 1", dict(ratio=1.0)), ("ratio nan", dict(ratio=nan)),
                     ("ratio without the flag", dict(vs=0, ratio=1.5))):
        o = _background(fx["bg_depth"], views[0], bg_valid, **kw)
        assert o.rc == CG.DH_ERR_ARG and o.err, what
        _background_untouched(o)


# ---- 6. guard bands and stale workspaces ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["views_and_none", "pure_camera"])
def test_guard_bands_and_stale_workspaces(monkeypatch, what):
    """tests/test_workspace_guards_gpu.py's four runs (three fills and a plain call) of the two new entries at 64."""
    res = 64
    depth, bg, masks = R.two_spheres(res)
    c = CM.cameras_for(depth)
    cams = [c["general"], None, V.DOLLY_IN_1]
    if what == "views_and_none":
        counts = WG._reproject(monkeypatch, dev(), depth, bg, masks, WG.THREE, cameras=cams, view_surfaces=True,
                               view_surface_max_ratio=1.5)
        assert int(counts[:, 0].min()) > 0
    else:          # (every edit with a view: the calls of one frame then carve the one workspace alike, which the frame's check needs)
        WG._reproject(monkeypatch, dev(), depth, depth, [], [[], [], []], cameras=[c["general"], c["orbit"], V.DOLLY_IN_1],
                      view_surfaces=True)
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd import losses as LS
    import guarded as G
    G.arena_reset(_lib.lib())
    LS._WS.clear()


# ---- 7. the edit call ----------------------------------------------------------------------------------------------------------
tiny = CG.tiny


def test_transform_foreground_objects_with_the_conf_key(tiny, monkeypatch):
    """transform_foreground_objects(camera=...) with depth_transform_view_surfaces: true is guided_inference on the reference's
    rows; two runs are byte-equal; prepare_guidance sees as many rows as the reference has; without the key the call is what it
    was."""
    dh, gd, t = tiny.dh, tiny.gd, tiny.two
    tfs = [_t(tf) for tf in CG.LOOP_TFS]
    plain, pdisp = dh.transform_foreground_objects(**CG._common(t), fg_masks=t.masks, transforms=tfs, camera=CG.CAMERA)
    plain, plat = plain.clone(), gd.last_latents.clone()
    seen = []
    prepare = gd.prepare_guidance

    def spy(depth, prompt, acts, correspondences, *a, **kw):
        seen.append(int(torch.as_tensor(correspondences).shape[0]))
        return prepare(depth, prompt, acts, correspondences, *a, **kw)
    dh.conf["depth_transform_view_surfaces"] = True
    try:
        monkeypatch.setattr(gd, "prepare_guidance", spy)
        img, disp = dh.transform_foreground_objects(**CG._common(t), fg_masks=t.masks, transforms=tfs, camera=CG.CAMERA)
        monkeypatch.setattr(gd, "prepare_guidance", prepare)
        img, lat = img.clone(), gd.last_latents.clone()
        again, _ = dh.transform_foreground_objects(**CG._common(t), fg_masks=t.masks, transforms=tfs, camera=CG.CAMERA)
        assert torch.equal(again, img) and torch.equal(gd.last_latents, lat)
        # no camera: the setting changes nothing
        a, ad = dh.transform_foreground_objects(**CG._common(t), fg_masks=t.masks, transforms=tfs)
        a = a.clone()
    finally:
        del dh.conf["depth_transform_view_surfaces"]
    b, bd = dh.transform_foreground_objects(**CG._common(t), fg_masks=t.masks, transforms=tfs)
    assert torch.equal(a, b) and torch.equal(ad, bd)
    # the reference's rows (geometry only: no in-fill on the CPU at 512)
    depth, bg, masks = t.depth.cpu(), t.bg_depth.cpu(), [m.cpu() for m in t.masks]
    _, corr_r, g = V.transform_surfaces(depth, bg, masks, [0, 1], CG.LOOP_TFS, CG.CAMERA, (), True, None,
                                        K=gd.get_depth_intrinsics(device="cpu"), infill=False)
    assert seen == [len(corr_r)], (seen, len(corr_r))
    kinds = torch.from_numpy(g["row_kind"])
    assert int((kinds == 2).sum()) >= 50000 and int((kinds == 0).sum()) >= 100
    ref = gd.guided_inference(t.noise, disp, t.null_text, t.prompt, t.acts, corr_r, row_kind=(kinds == 2).to(torch.uint8) * 2)
    assert torch.equal(gd.last_latents, lat) and torch.equal(ref, img)
    assert not torch.equal(disp, pdisp) and not torch.equal(img, plain)
    # without the key the call is what it was, byte for byte
    after, adisp = dh.transform_foreground_objects(**CG._common(t), fg_masks=t.masks, transforms=tfs, camera=CG.CAMERA)
    assert torch.equal(after, plain) and torch.equal(adisp, pdisp) and torch.equal(gd.last_latents, plat)
