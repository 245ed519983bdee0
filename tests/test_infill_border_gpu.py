"""GPU: the in-fill's image border (dh_reproject_border_edits, dh_reproject_border_background, dh_laplacian_blend_border;
depth_transform.reproject(infill_border=...), reproject_border_edits, laplacian_depth_blend(infill_border=...); the conf key
depth_transform_infill_border) against the test-side statement tests/infill_border_ref.py.

The three CG kernels are reached one system per launch through the blend with dilate_iterations = 0, with the gates of
tests/test_infill_solvers_gpu.py on the REFLECT system, at the smallest shapes per solver class whose holes touch the frame; the
re-projection runs the two-sphere fixture of tests/camera_moves_ref.py at 128 pixels, where a reflecting border changes the
disparity of the in-fill components that touch the frame and no integer output.  The C entries write into outputs that are
NaN / 0xFF / -1 before the call (the helpers of tests/test_camera_moves_gpu.py, with the border entries behind the names of the
entries they extend)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_moves_ref as CM  # noqa: E402
import footprints_ref as F  # noqa: E402
import infill_border_ref as IB  # noqa: E402
import reproject_calls as RC  # noqa: E402
import multi_object_ref as R  # noqa: E402
import object_removal_ref as RM  # noqa: E402
import test_camera_moves_gpu as TC  # noqa: E402  (helpers only: _setup, _view_rows, _call, _check, _untouched, _background_call, tiny)
import test_object_copies_gpu as OC  # noqa: E402  (helpers only: _rows, _t)
import test_workspace_guards_gpu as WG  # noqa: E402  (helpers only: guarded_runs, _reproject, _cams, THREE)

from diffusionhandles_amd import _lib  # noqa: E402
from diffusionhandles_amd import depth_transform as DT  # noqa: E402
from oracle import depth_ref as D  # noqa: E402

pytestmark = pytest.mark.gpu
dev = TC.dev
tiny = TC.tiny                                  # the module-scoped TINY rig of the camera tests, built once for this module
hooks_at_their_defaults = WG.hooks_at_their_defaults
RES = 128
NAMES = ("pan", "dolly_out", "truck")
DH_ERR_ARG = -1
Y = R.Y
Z0 = (0.0, 0.0, 0.0)


class BorderLib:
    """The library with the border entries behind the names of the entries they extend, at one border value: the callers of
    tests/test_camera_moves_gpu.py (poisoned outputs, the checks of a successful call) then drive the new entries."""

    def __init__(self, border):
        self._L, self._border = _lib.lib(), border

    def __getattr__(self, name):
        return getattr(self._L, name)

    def dh_reproject_camera_edits(self, *args):
        return self._L.dh_reproject_border_edits(*args, self._border)

    def dh_reproject_camera_background(self, *args):
        return self._L.dh_reproject_border_background(*args, self._border)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _only_the_frame_components_differ(reflect, zero, inpaint, what):
    """Two disparities of one edit under the two borders.  The known pixels carry the same bits.  The in-fill components that do
    not touch the frame are the same linear system under both borders, but an edit is ONE CG solve over all of its components, so
    their iterates differ: both are f32 roundings of one f64 solution (the project's rule, 4 * 2^-24 * max |x|, twice).  The
    components at the frame differ by whole disparity units."""
    touch, rest = IB.touching(inpaint)
    assert np.array_equal(_u32(reflect[~inpaint]), _u32(zero[~inpaint])), what
    if rest.any():
        bound = 2 * 4.0 * 2.0 ** -24 * float(np.abs(zero[rest]).max())
        assert float(np.abs(reflect.astype(np.float64) - zero)[rest].max()) <= bound, what
    assert float(np.abs(reflect - zero)[touch].max()) > 1.0, what


# ---- 1. the three solvers on reflect systems -----------------------------------------------------------------------------------
def _blend(depth, bg, mask, **kw):
    t = lambda a: torch.from_numpy(np.array(a))[None, None].to(dev())      # (a copy: the cached references are read-only)
    out, its = DT.laplacian_depth_blend(t(depth), t(bg), t(mask), dilate_iterations=0, return_iterations=True, **kw)
    return out[0, 0].cpu().numpy(), its


@pytest.mark.parametrize("name", list(IB.SOLVER_CASES))
def test_infill_solver_reflect_vs_f64_reference(name):
    res, _, n_expected, solver = IB.SOLVER_CASES[name]
    depth, bg, mask, ref, its_ref, _, _ = IB.solver_reference(name)
    n = int(mask.sum())
    assert n == n_expected and IB.solver_of(n) == solver, (n, IB.solver_of(n))
    assert (mask & IB.frame_edge(mask.shape)).any()
    out, its = _blend(depth, bg, mask, infill_border="reflect")
    finite = bool(np.isfinite(out).all())
    err = float(np.abs(out.astype(np.float64) - ref).max()) if finite else float("nan")
    bound = IB.bound(ref, mask)
    print(f"reflect in-fill {name}: res {res}, n {n} ({solver}), its_ref {its_ref}, iterations {its}, max abs err {err:.3e} "
          f"(bound {bound:.3e})")
    assert its >= 0, its
    assert its <= 1.05 * its_ref + 5, (name, its, its_ref)
    assert finite
    assert err <= bound, (name, err, bound)
    assert np.array_equal(_u32(out[~mask]), _u32(depth[~mask]))          # outside the mask: the input's bits
    out2, its2 = _blend(depth, bg, mask, infill_border="reflect")
    assert its2 == its and np.array_equal(_u32(out2), _u32(out))
    # and the border is in play: the zero-border solution of the same hole is another one
    zero, _ = _blend(depth, bg, mask)
    assert float(np.abs(zero.astype(np.float64) - ref)[mask].max()) > 100 * bound


# ---- 2. zero mode is the call without the keyword -----------------------------------------------------------------------------
def _k3(**kw):
    fx = CM.fixture(RES)
    to = lambda t: t.to(dev())
    cams = [fx["cameras"][n] for n in NAMES]
    return DT.reproject(to(fx["depth"]), to(fx["bg_depth"]), [to(m) for m in fx["masks"]], D.intrinsics_f32(),
                        [[OC._t(tf) for tf in fx["transforms"]]] * 3, cameras=cams, return_debug=True, device_correspondences=True, **kw)


def _same_reprojection(a, b, disparity=True):
    (out_a, dbg_a), (out_b, dbg_b) = a, b
    for ra, rb in zip(out_a, out_b):
        for j, (x, y) in enumerate(zip(ra, rb)):
            if j or disparity:
                assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
    for k in ("zmap", "raw_mask", "clean_mask", "vis", "target_xy", "bg_counts", "bg_valid"):
        assert torch.equal(dbg_a[k].contiguous().view(torch.uint8), dbg_b[k].contiguous().view(torch.uint8)), k
    assert torch.equal(dbg_a["counts"][:, :3], dbg_b["counts"][:, :3])
    if disparity:
        assert torch.equal(dbg_a["counts"], dbg_b["counts"])


def test_zero_none_and_the_omitted_keyword_are_one_call():
    depth, bg, mask, _, _, _, _ = IB.solver_reference("multi_corner_92")
    base, its = _blend(depth, bg, mask)
    assert its > 0
    for value in ("zero", None):
        out, its_v = _blend(depth, bg, mask, infill_border=value)
        assert its_v == its and np.array_equal(_u32(out), _u32(base)), value
    plain = _k3()
    assert int(plain[1]["counts"][:, 2].min()) > 0 and int(plain[1]["counts"][:, 3].min()) > 0
    for value in ("zero", None):
        _same_reprojection(_k3(infill_border=value), plain)
    # the named call of the camera tests, and the new name without its keyword
    fx = CM.fixture(RES)
    to = lambda t: t.to(dev())
    args = (to(fx["depth"]), to(fx["bg_depth"]), [to(m) for m in fx["masks"]], D.intrinsics_f32(), [[OC._t(tf) for tf in fx["transforms"]]] * 3)
    kw = dict(cameras=[fx["cameras"][n] for n in NAMES], return_debug=True, device_correspondences=True)
    _same_reprojection(DT.reproject_camera_edits(*args, **kw), plain)
    _same_reprojection(DT.reproject_border_edits(*args, **kw), plain)


# ---- 3. re-projection: K = 3 cameras -------------------------------------------------------------------------------------------
def _reflect_ref(geo):
    """the reference of an edit with the reflect fill: the geometry's integer outputs, its disparity re-filled"""
    return torch.from_numpy(IB.camera_fill(geo, "reflect"))[None, None], geo[1], geo[2]


def test_three_cameras_in_one_call_against_the_reference():
    fx = CM.fixture(RES)
    s = TC._setup(fx["depth"], fx["bg_depth"], fx["masks"])
    cams = [fx["cameras"][n] for n in NAMES]
    views, has = TC._view_rows(cams)
    rows = np.tile(OC._rows([fx["transforms"]]), (3, 1))
    zero = TC._call(s, rows, [0, 1], views, has)
    s.L = BorderLib(1)
    o = TC._call(s, rows, [0, 1], views, has)
    assert o.rc == 0 and zero.rc == 0, o.err
    for e, name in enumerate(NAMES):
        geo = fx["geo"][name]
        TC._check(o, e, _reflect_ref(geo), f"reflect K 3 {name}")          # every integer output bit-exact, the disparity to 2e-3
        _only_the_frame_components_differ(o.disp[e].cpu().numpy(), zero.disp[e].cpu().numpy(), geo[2]["inpaint"], name)
        for k in ("zmap", "raw", "clean", "vis", "txy", "corr", "inst"):
            assert torch.equal(getattr(o, k)[e].contiguous().view(torch.uint8), getattr(zero, k)[e].contiguous().view(torch.uint8)), (name, k)
        assert torch.equal(o.counts_h[e, :3], zero.counts_h[e, :3]) and o.bg_h[e] == zero.bg_h[e]
        print(f"{name}: CG iterations zero {int(zero.counts_h[e, 3])} -> reflect {int(o.counts_h[e, 3])}")
    # the border entry with border 0 is the camera entry
    s.L = BorderLib(0)
    again = TC._call(s, rows, [0, 1], views, has)
    for e in range(3):
        TC._same_bytes(again, e, zero, e, f"border 0, edit {e}")
    # the host layer
    out, dbg = _k3(infill_border="reflect")
    for e, name in enumerate(NAMES):
        disp, corr, inst = out[e]
        assert torch.equal(disp[0, 0], o.disp[e]) and torch.equal(corr.cpu(), fx["geo"][name][1]), name
    _same_reprojection((out, dbg), _k3(), disparity=False)
    assert torch.equal(dbg["counts"], o.counts_h)


# ---- 4. the background entry: the pure camera move and a pure removal ---------------------------------------------------------
@pytest.mark.parametrize("name", ["pan", "dolly_out"])
def test_pure_camera_move_against_the_reference(monkeypatch, name):
    depth, bg, masks = R.two_spheres(RES)
    cam = CM.cameras_for(depth)[name]
    geo = OC._refs(("camera pure", RES, name), lambda: CM.background_camera(bg, cam, removed_masks=masks))
    disp_r = IB.camera_fill(geo, "reflect")
    g = geo[2]
    touch, _ = IB.touching(g["inpaint"])
    assert touch.sum() >= 500
    covered = (masks[0] != 0) | (masks[1] != 0)
    bg_valid = (~covered).reshape(-1).to(torch.uint8).to(dev()).contiguous()
    views, _ = TC._view_rows([cam])
    zero = TC._background_call(bg, views[0], bg_valid)
    with monkeypatch.context() as m:
        m.setattr(_lib, "lib", lambda L=BorderLib(1): L)
        o = TC._background_call(bg, views[0], bg_valid)
    assert o.rc == 0 and zero.rc == 0, o.err
    c, nb = o.counts.tolist(), int(o.bg_counts[0])
    assert c[:3] == [0, 0, int(g["inpaint"].sum())] and c[3] >= 0 and c[:3] == zero.counts.tolist()[:3]
    assert nb == len(geo[1]) and np.array_equal(o.bg_corr[:nb].cpu().numpy(), geo[1].numpy()) and bool((o.bg_corr[nb:] == -1).all())
    assert np.array_equal(o.zmap.cpu().numpy(), g["zmap"])
    err = float(np.abs(o.disp.cpu().numpy() - disp_r).max())
    apart = float(np.abs(o.disp.cpu().numpy() - zero.disp.cpu().numpy())[touch].max())
    print(f"pure {name}: {c[2]} in-fill pixels ({int(touch.sum())} touching the frame), CG iterations zero {zero.counts.tolist()[3]} -> "
          f"reflect {c[3]}, disparity max abs err {err:.2e}, reflect - zero up to {apart:.1f}")
    assert err < 2e-3 and apart > 1.0
    (disp, corr, inst), = DT.reproject(depth.to(dev()), bg.to(dev()), [], D.intrinsics_f32(), [[]], removed_masks=[m.to(dev()) for m in masks],
                                       cameras=[cam], infill_border="reflect")
    assert torch.equal(corr, geo[1]) and torch.equal(disp[0, 0].to(dev()), o.disp) and bool((inst == 0).all())


def test_pure_removal_of_an_object_at_the_frame():
    """An object that touches the left border is deleted: set_foreground's blend fills its hole with the reflecting border (its
    dilated mask touches the frame), then the background alone is re-projected through dh_reproject_border_background without a
    view.  (The re-projection of a pure removal in-fills only pixels no background point owns; the removed region itself is
    the blend's.)  Around the object the depth is one unit nearer than the background depth says -- a ring mismatch of -1:
    under reflect it spreads as the constant it is, out = bg - 1 inside; under zero it is forced to 0 at the frame."""
    _, bg, _ = R.two_spheres(RES)
    m, near = np.zeros((RES, RES), dtype=bool), np.zeros((RES, RES), dtype=bool)
    m[40:80, 0:25] = True
    near[30:90, 0:40] = True
    mask = torch.from_numpy(m)[None, None].to(torch.float32)
    depth = torch.where(torch.from_numpy(near)[None, None], bg - 1.0, bg).contiguous()
    import scipy.ndimage
    grown = scipy.ndimage.binary_dilation(m, iterations=3)
    assert not (scipy.ndimage.binary_dilation(grown) & ~near).any()
    want = IB.laplacian_blend(depth[0, 0].numpy(), bg[0, 0].numpy(), grown, "reflect")
    got, its = DT.laplacian_depth_blend(depth.to(dev()), bg.to(dev()), mask.to(dev()), dilate_iterations=3, return_iterations=True,
                                        infill_border="reflect")
    bound = 4.0 * 2.0 ** -24 * float(np.abs(want).max())
    err = float(np.abs(got[0, 0].cpu().numpy().astype(np.float64) - want).max())
    assert its > 0 and err <= bound, err
    inside = torch.from_numpy(grown)
    assert float((got.cpu() - (bg - 1.0))[0, 0][inside].abs().max()) <= 2 * bound          # (the rounding of bg - 1 itself, and the solve's)
    zero = DT.laplacian_depth_blend(depth.to(dev()), bg.to(dev()), mask.to(dev()), dilate_iterations=3)
    assert float((zero - got)[0, 0].cpu()[inside].abs().max()) > 0.1          # the mismatch is no longer forced to 0 at the frame
    bg2 = got.cpu()
    ref, g = RM.background_alone(bg2)
    ref = IB.harmonic_fill(g["disparity"], g["unowned"], "reflect").astype(np.float32)
    p = DT.reproject_plan(depth, [], [[], []], removed_masks=[mask], infill_border="reflect")
    assert (p.kind, RC.fields(p)) == ("pure_removal", RC.border(RC.BACKGROUND))
    out, dbg = DT.reproject(depth.to(dev()), got, [], D.intrinsics_f32(), [[], []], removed_masks=[mask.to(dev())], infill_border="reflect",
                            return_debug=True)
    assert len(out) == 2 and all(len(r[1]) == 0 for r in out)
    assert np.array_equal(dbg["zmap"][0].cpu().numpy(), g["zmap"]) and int(dbg["counts"][0, 2]) == int(g["unowned"].sum())
    assert float(np.abs(out[0][0][0, 0].cpu().numpy() - ref).max()) < 2e-3
    assert torch.equal(out[0][0], out[1][0])


# ---- 5. edits without a camera -----------------------------------------------------------------------------------------------
SHIFT = (0.9, 0.0, 0.0)          # sphere 0 pushed to the right border: the mask clean-up's in-fill pixels reach the frame


def test_object_edit_whose_infill_touches_the_frame():
    depth, bg, masks = R.two_spheres(RES)
    tfs = [(0.0, Y, SHIFT), (0.0, Y, Z0)]
    geo = OC._refs(("border shift", RES), lambda: CM.transform_camera(depth, bg, masks, [0, 1], tfs, None))
    touch, rest = IB.touching(geo[2]["inpaint"])
    assert touch.any() and rest.any()
    args = (depth.to(dev()), bg.to(dev()), [m.to(dev()) for m in masks], D.intrinsics_f32(), [[OC._t(tf) for tf in tfs]])
    p = DT.reproject_plan(depth, masks, [[OC._t(tf) for tf in tfs]], infill_border="reflect")
    assert RC.fields(p) == RC.border(RC.INSTANCE) and not p.with_table
    ((disp, corr),), dbg = DT.reproject(*args, infill_border="reflect", return_debug=True)
    ((disp0, corr0),), dbg0 = DT.reproject(*args, return_debug=True)
    assert torch.equal(corr, geo[1]) and torch.equal(corr, corr0)
    for k in ("zmap", "raw_mask", "clean_mask", "vis", "target_xy"):
        assert torch.equal(dbg[k], dbg0[k]), k
    assert "corr_inst" not in dbg and torch.equal(dbg["counts"][:, :3], dbg0["counts"][:, :3])
    a, b = disp[0, 0].cpu().numpy(), disp0[0, 0].cpu().numpy()
    err = float(np.abs(a - IB.camera_fill(geo, "reflect")).max())
    print(f"shifted sphere: {int(touch.sum())} of {int(geo[2]['inpaint'].sum())} in-fill pixels in components at the frame, "
          f"disparity max abs err {err:.2e}, reflect - zero up to {float(np.abs(a - b).max()):.1f}")
    assert err < 2e-3
    _only_the_frame_components_differ(a, b, geo[2]["inpaint"], "shifted sphere")
    assert float(np.abs(b - geo[0][0, 0].numpy()).max()) < 2e-3


def test_footprints_with_the_reflecting_border():
    depth, bg, masks = R.two_spheres(RES)
    tfs = [(0.0, Y, SHIFT, 1.8, None), (0.0, Y, Z0, 1.0, None)]
    ref = OC._refs(("border footprints", RES), lambda: F.transform_objects(depth, bg, masks, tfs, footprints=True))
    g = ref[2]
    touch, _ = IB.touching(g["inpaint"])
    assert touch.any()
    want = IB.harmonic_fill(g["disparity"], g["inpaint"], "reflect").astype(np.float32)
    args = (depth.to(dev()), bg.to(dev()), [m.to(dev()) for m in masks], D.intrinsics_f32(), [[OC._t(tf) for tf in tfs]])
    ((disp, corr),), dbg = DT.reproject(*args, footprints=True, infill_border="reflect", return_debug=True)
    (disp0, corr0), = DT.reproject_object_edits(*args, footprints=True)
    assert torch.equal(corr, ref[1]) and torch.equal(corr, corr0) and int(dbg["counts"][0, 2]) == int(g["inpaint"].sum())
    a, b = disp[0, 0].cpu().numpy(), disp0[0, 0].cpu().numpy()
    err = float(np.abs(a - want).max())
    print(f"footprints: {int(touch.sum())} of {int(g['inpaint'].sum())} in-fill pixels at the frame, disparity max abs err {err:.2e}")
    assert err < 2e-3
    _only_the_frame_components_differ(a, b, g["inpaint"], "footprints")
    # input-depth normalisation composes: the bounds change the values the fill sees, not the rule
    (dn, cn), = DT.reproject(*args, infill_border="reflect", use_input_depth_normalization=True)
    (dn0, _), = DT.reproject(*args, use_input_depth_normalization=True)
    assert torch.isfinite(dn).all() and not torch.equal(dn, dn0)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_a_border_other_than_0_or_1_is_refused_with_the_outputs_untouched(monkeypatch):
    fx = CM.fixture(RES)
    s = TC._setup(fx["depth"], fx["bg_depth"], fx["masks"])
    views, has = TC._view_rows([fx["cameras"]["pan"]])
    rows = OC._rows([fx["transforms"]])
    for bad in (2, -1):
        s.L = BorderLib(bad)
        o = TC._call(s, rows, [0, 1], views, has)
        assert o.rc == DH_ERR_ARG and "infill_border" in o.err, (bad, o.err)
        TC._untouched(o)
        _, bg, _ = R.two_spheres(RES)
        valid = torch.ones(RES * RES, dtype=torch.uint8, device=dev())
        with monkeypatch.context() as m:
            m.setattr(_lib, "lib", lambda L=BorderLib(bad): L)
            o = TC._background_call(bg, views[0], valid)
        assert o.rc == DH_ERR_ARG and "infill_border" in o.err, (bad, o.err)
        assert torch.isnan(o.zmap).all() and torch.isnan(o.disp).all() and bool((o.counts == -1).all())
        assert bool((o.bg_corr == -1).all()) and bool((o.bg_counts == -1).all())
        # the blend
        L = _lib.lib()
        res = 64
        depth, bgf = IB.fields(res)
        d, b = torch.from_numpy(depth).to(dev()), torch.from_numpy(bgf).to(dev())
        mk = torch.from_numpy(IB.corner(res, 20).astype(np.uint8)).to(dev())
        out = torch.full((res, res), float("nan"), device=dev())
        counts = torch.full((4,), -1, dtype=torch.int32, device=dev())
        nb = ctypes.c_size_t()
        _lib.check(L.dh_laplacian_blend_workspace_bytes(res, ctypes.byref(nb)))
        ws = torch.full((nb.value,), 0xFF, dtype=torch.uint8, device=dev())
        rc = L.dh_laplacian_blend_border(_lib.ptr(d), _lib.ptr(b), _lib.ptr(mk), res, 0, _lib.ptr(out), _lib.ptr(counts), _lib.ptr(ws),
                                         nb.value, _lib.stream_ptr(), bad)
        err = L.dh_last_error().decode()
        torch.cuda.synchronize()
        assert rc == DH_ERR_ARG and "infill_border" in err, (bad, err)
        assert torch.isnan(out).all() and bool((counts == -1).all()) and bool((ws == 0xFF).all())


# ---- 7. the whole image ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", ["reflect", "zero"])
def test_whole_image_mask_returns_zeros_with_count_0(border):
    """The one component without a known neighbour.  The blend's right-hand side is minus the background's Laplacian: a constant
    background has none under replicate padding (reflect), a zero background none under zero padding; then b = 0, (b, b) = 0, the
    loop never starts -- no code path of its own."""
    res = 64
    depth, _ = IB.fields(res)
    bg = np.full((res, res), 3.0 if border == "reflect" else 0.0, dtype=np.float32)
    assert not IB.laplacian_f32(bg, border).any()
    out, its = _blend(depth, bg, np.ones((res, res), dtype=bool), infill_border=border)
    assert its == 0 and not out.any() and IB.solver_of(res * res) == "lds"


# ---- 8. guard bands and stale workspaces -------------------------------------------------------------------------------------
def test_guards_border_edits(monkeypatch):
    depth, bg, masks = R.two_spheres(64)
    WG._reproject(monkeypatch, dev(), depth, bg, masks, WG.THREE, cameras=WG._cams(depth), infill_border="reflect")


def test_guards_border_background(monkeypatch):
    depth, bg, masks = R.two_spheres(64)
    WG._reproject(monkeypatch, dev(), depth, depth, [], [[], [], []], cameras=WG._cams(depth), infill_border="reflect")


def test_guards_blend_border(monkeypatch):
    res = 64
    depth, bg = IB.fields(res)
    t = lambda a: torch.from_numpy(np.array(a))[None, None].to(dev())
    d, b, m = t(depth), t(bg), t(IB.corner(res, 40))
    call = lambda: DT.laplacian_depth_blend(d, b, m, dilate_iterations=3, return_iterations=True, infill_border="reflect")
    WG.guarded_runs(monkeypatch, dev(), [DT], call, lambda r: dict(out=r[0], iterations=np.int64(r[1])))


# ---- 9. the facade ---------------------------------------------------------------------------------------------------------------
def test_the_conf_key_is_the_explicit_call(tiny):
    """With depth_transform_infill_border: reflect an edit is reproject(..., infill_border="reflect") + guided_inference, and
    set_foreground is the reflect blend; without the key (and with zero) both are what they were."""
    dh, gd, t = tiny.dh, tiny.gd, tiny.two
    tfs = [OC._t((0.0, Y, SHIFT)), OC._t((0.0, Y, Z0))]
    intr = gd.get_depth_intrinsics(device=dev())
    common = TC._common(t)
    assert "depth_transform_infill_border" not in dh.conf

    def explicit(**kw):
        (d, c), = DT.reproject(t.depth, t.bg_depth, t.masks, intr, [tfs], **kw)
        img = gd.guided_inference(t.noise, d, t.null_text, t.prompt, t.acts, c)
        return img.clone(), d, gd.last_latents.clone()

    plain, pdisp = dh.transform_foreground_objects(**common, fg_masks=t.masks, transforms=tfs)
    plain, plat = plain.clone(), gd.last_latents.clone()
    img0, d0, lat0 = explicit()
    assert torch.equal(pdisp, d0) and torch.equal(plain, img0) and torch.equal(plat, lat0)
    (dq, _), = DT.reproject_object_edits(t.depth, t.bg_depth, t.masks, intr, [tfs])
    assert torch.equal(dq, pdisp)
    blend0 = dh.set_foreground(t.depth, t.masks, t.bg_depth)
    try:
        dh.conf["depth_transform_infill_border"] = "zero"
        assert torch.equal(dh.set_foreground(t.depth, t.masks, t.bg_depth), blend0)
        dh.conf["depth_transform_infill_border"] = "reflect"
        img, disp = dh.transform_foreground_objects(**common, fg_masks=t.masks, transforms=tfs)
        img, lat = img.clone(), gd.last_latents.clone()
        img1, d1, lat1 = explicit(infill_border="reflect")
        assert torch.equal(disp, d1) and torch.equal(img, img1) and torch.equal(lat, lat1)
        assert not torch.equal(disp, pdisp)
        # set_foreground: a mask that touches the frame, the blend with the key and the explicit one
        edge = torch.zeros_like(t.masks[0])
        edge[..., 200:300, 0:60] = 1
        far = t.bg_depth + 0.5          # (a ring mismatch of -0.5: with depth == bg_depth around the mask both borders give bg_depth)
        got = dh.set_foreground(t.depth, edge, far)
        assert torch.equal(got, DT.laplacian_depth_blend(t.depth, far, edge, dilate_iterations=15, infill_border="reflect"))
        assert not torch.equal(got, DT.laplacian_depth_blend(t.depth, far, edge, dilate_iterations=15))
    finally:
        dh.conf.pop("depth_transform_infill_border", None)
