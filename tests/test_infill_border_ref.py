"""CPU: the in-fill's image border ("In-fill border") -- the rule of tests/infill_border_ref.py against the oracle and
against itself, the f64 model of the pipelined solver on the reflect systems, and the host side of the setting (validator,
parameter lists, mesh refusals, conf key, command line).  No GPU."""
import inspect
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_moves_ref as CM  # noqa: E402
import infill_border_ref as IB  # noqa: E402
import multi_object_ref as R  # noqa: E402
import reproject_calls as RC  # noqa: E402

from oracle import depth_ref as D  # noqa: E402

Y = R.Y
Z3 = (0.0, 0.0, 0.0)


def _field(res, seed=3):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(res, dtype=np.float64), np.arange(res, dtype=np.float64), indexing="ij")
    return (100.0 + 40.0 * np.sin(xx / 7.0) + 30.0 * yy / res + rng.standard_normal((res, res))).astype(np.float32)


# ---- 1. zero mode is the oracle ---------------------------------------------------------------------------------------------
def test_zero_mode_is_the_oracle_exactly():
    res = 48
    img, bg = _field(res), _field(res, 4)
    for mask in (IB.corner(res, 20), IB.strip_columns(res, 5), IB.frame(res, 6), np.pad(np.ones((10, 12), bool), ((9, 29), (20, 16)))):
        assert mask.shape == (res, res)
        a, b = IB.harmonic_fill(img, mask, "zero"), D.harmonic_fill(img, mask.astype(np.uint8))
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        a, b = IB.laplacian_blend(img, bg, mask, "zero"), D.laplacian_blend(img, bg, mask)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the f32-rounded Laplacian of the solver tests, zero padding: infill_ref's
    import infill_ref as I
    assert np.array_equal(IB.laplacian_f32(bg, "zero"), I.laplacian_f32(bg))
    A0, b0, _, _ = I.system(img, IB.corner(res, 20), I.laplacian_f32(bg))
    A1, b1, _, _ = IB.system(img, IB.corner(res, 20), IB.laplacian_f32(bg, "zero"), "zero")
    assert (A0 != A1).nnz == 0 and np.array_equal(b0, b1)


# ---- 2. the defining property: a constant ring gives a constant fill ---------------------------------------------------------
@pytest.mark.parametrize("name,make", [("one border", lambda r: np.pad(np.ones((10, 14), bool), ((0, r - 10), (9, r - 23)))),
                                       ("two borders", lambda r: IB.corner(r, 17)),
                                       ("three borders", lambda r: IB.strip_columns(r, 6)),
                                       ("four borders", lambda r: IB.frame(r, 5))])
def test_constant_ring_fills_constant_under_reflect_only(name, make):
    res, c = 40, 37.5
    mask = make(res)
    img = np.full((res, res), c)
    img[mask] = -1000.0                                   # never read: only known values enter
    fill = IB.harmonic_fill(img, mask, "reflect")
    assert float(np.abs(fill - c).max()) <= 1e-9, name
    zero = IB.harmonic_fill(img, mask, "zero")
    edge = mask & IB.frame_edge(mask.shape)
    print(f"{name}: zero border fills to mean {zero[mask].mean():.2f}, {zero[edge].mean():.2f} on the frame edge (ring {c})")
    assert zero[edge].mean() < 0.75 * c and zero[mask].min() < 0.5 * c, name
    assert np.array_equal(zero[~mask], img[~mask]) and np.array_equal(fill[~mask], img[~mask])


# ---- 3. the mirror statement -------------------------------------------------------------------------------------------------
def test_reflect_is_the_zero_border_fill_of_the_mirrored_image():
    """A corner hole (top right): the image and the mask mirrored across the top and the right border give a 2x image in
    which the hole is interior; its zero-border fill, restricted to the original quadrant, is the reflect fill."""
    res, side = 36, 15
    img = _field(res).astype(np.float64)
    mask = IB.corner(res, side)
    big = np.block([[img[::-1, :], img[::-1, ::-1]], [img, img[:, ::-1]]])           # original = bottom left quadrant
    bigm = np.block([[mask[::-1, :], mask[::-1, ::-1]], [mask, mask[:, ::-1]]])
    assert not (bigm & IB.frame_edge(bigm.shape)).any()                               # interior: the border rule is not in play
    mirrored = IB.harmonic_fill(big, bigm, "zero")[res:, :res]
    assert np.array_equal(IB.harmonic_fill(big, bigm, "zero"), IB.harmonic_fill(big, bigm, "reflect"))
    fill = IB.harmonic_fill(img, mask, "reflect")
    assert float(np.abs(fill - mirrored).max()) <= 1e-9 * float(np.abs(img).max())
    assert float(np.abs(IB.harmonic_fill(img, mask, "zero") - mirrored).max()) > 1.0


# ---- 4. the blend's fixed point ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", IB.BORDERS)
def test_blend_of_equal_depths_is_the_background(border):
    res = 40
    bg = _field(res, 7)
    for mask in (IB.corner(res, 13), IB.strip_rows(res, 4), IB.frame(res, 3)):
        out = IB.laplacian_blend(bg.copy(), bg, mask, border)
        assert out.dtype == np.float32
        err = float(np.abs(out.astype(np.float64) - bg).max())
        assert err <= 4.0 * 2.0 ** -24 * float(np.abs(bg).max()), (border, err)
    # replicate padding: a constant image has no Laplacian anywhere, a zero-padded one has one on the frame
    one = np.full((8, 8), 3.0, dtype=np.float32)
    assert not IB.laplacian_f32(one, "reflect").any() and IB.laplacian_f32(one, "zero")[0, 0] == -6.0
    assert np.array_equal(IB.laplacian(one.astype(np.float64), "reflect"), IB.laplacian_f32(one, "reflect"))
    assert IB.degree(5, 7)[0, 0] == 2 and IB.degree(5, 7)[0, 3] == 3 and IB.degree(5, 7)[2, 3] == 4 and IB.degree(5, 7).sum() == 4 * 35 - 24


def test_whole_image_mask_is_all_zeros():
    """The only component without a known neighbour: b = 0, so (b, b) = 0 and no solver enters its loop."""
    img = _field(16)
    m = np.ones((16, 16), dtype=bool)
    for border in IB.BORDERS:
        A, b, _, _ = IB.system(img, m, None, border)
        assert not b.any() and IB.classic_cg_iterations(A, b) == 0 and IB.pipelined_cg_iterations(A, b) == 0
        assert not IB.harmonic_fill(img, m, border).any()
    A, _, _, _ = IB.system(img, m, None, "reflect")
    assert float(np.abs(A @ np.ones(256)).max()) == 0.0          # singular: the constants; every other component has a known neighbour


# ---- 5. the six-camera fixture -----------------------------------------------------------------------------------------------
# (in-fill pixels, in components touching the frame, ring mean, frame-edge mean zero / reflect, classic CG iterations zero / reflect)
CAMERA_TABLE = {
    "pan": (2153, 1522, 31.7, 7.1, 27.1, 115, 192),
    "orbit": (1921, 871, 46.1, 15.3, 44.2, 79, 129),
    "dolly_in": (2682, 1808, 32.1, 5.1, 7.7, 28, 32),
    "dolly_out": (2159, 1806, 28.6, 5.6, 28.9, 56, 101),
    "truck": (1462, 916, 32.7, 2.2, 13.5, 69, 117),
    "general": (2299, 700, 30.0, 11.8, 30.5, 62, 104),
}


@pytest.mark.parametrize("name", CM.CAMERA_NAMES)
def test_six_cameras_at_128(name):
    geo = CM.fixture(128)["geo"][name]
    g = geo[2]
    row = IB.camera_table_row(geo)
    print(f"{name}: in-fill {row[0]} ({row[1]} touching the frame), ring mean {row[2]:.1f}, frame-edge mean zero {row[3]:.1f} / "
          f"reflect {row[4]:.1f}, classic CG iterations {row[5]} -> {row[6]}")
    want = CAMERA_TABLE[name]
    assert row[:2] == want[:2] and all(abs(a - b) <= 2 for a, b in zip(row[5:], want[5:])), (row, want)      # (counts: +- a summation order)
    assert all(abs(a - b) <= 0.05 + 1e-9 for a, b in zip(row[2:5], want[2:5])), (row, want)
    zero, refl = IB.camera_fill(geo, "zero"), IB.camera_fill(geo, "reflect")
    assert np.array_equal(zero.view(np.uint32), geo[0][0, 0].numpy().view(np.uint32))          # the fixture's own fill is the zero border
    touch, rest = IB.touching(g["inpaint"])
    assert rest.any() and touch.any()
    assert np.array_equal(zero[rest].view(np.uint32), refl[rest].view(np.uint32))              # untouched components: bit for bit
    assert np.array_equal(zero[~g["inpaint"]].view(np.uint32), refl[~g["inpaint"]].view(np.uint32))
    if name in ("pan", "orbit", "dolly_out", "general"):
        ring, at_zero, at_reflect = row[2:5]
        assert abs(at_reflect - ring) <= 0.25 * ring, (name, at_reflect, ring)
        assert at_zero < 0.5 * ring, (name, at_zero, ring)


# ---- 6. the pipelined recurrence on the reflect systems -----------------------------------------------------------------------
# (classic CG / the pipelined model with replacement / without, f64, on the fields of infill_border_ref.fields -- DESIGN.md
# "In-fill border" records them: 414 / 414 / 415, 393 / 393 / 393, 663 / 663 / 719; the counts themselves are not pinned: a
# BLAS with another summation order may move them by an iteration)
@pytest.mark.parametrize("name", [n for n, c in IB.SOLVER_CASES.items() if c[3] == "multi"] + list(IB.MODEL_CASES))
def test_pipelined_model_keeps_classic_iteration_counts(name):
    _, _, mask, _, its_ref, A, b = IB.solver_reference(name)
    if name in IB.SOLVER_CASES:
        assert int(mask.sum()) == IB.SOLVER_CASES[name][2]
    its = IB.pipelined_cg_iterations(A, b)
    bare = IB.pipelined_cg_iterations(A, b, replace=0, cap=4 * its_ref)
    print(f"{name}: n {int(mask.sum())}, classic {its_ref}, pipelined with replacement {its}, without "
          f"{'breakdown' if bare == IB.BREAKDOWN else bare}")
    assert its is not None and its >= 0, its
    assert its <= 1.05 * its_ref + 5, (name, its, its_ref)


def test_solver_cases_have_their_sizes():
    for name, (res, make, n, _) in IB.SOLVER_CASES.items():
        m = make()
        assert m.shape == (res, res) and int(m.sum()) == n and (m & IB.frame_edge(m.shape)).any(), name
    assert IB.frame(128, 20)[0, 0] and IB.frame(128, 20)[127, 127] and not IB.frame(128, 20)[64, 64]


# ---- 7. validator, parameter lists, facade ------------------------------------------------------------------------------------
def test_check_infill_border():
    from diffusionhandles_amd import depth_transform as DT
    assert DT.check_infill_border(None) == 0 and DT.check_infill_border("zero") == 0 and DT.check_infill_border("reflect") == 1
    assert list(inspect.signature(DT.check_infill_border).parameters) == ["value", "what"]
    assert inspect.signature(DT.check_infill_border).parameters["what"].default == "infill_border"
    for bad in ("Reflect", "mirror", "", 0, 1, 2, True, False, 1.0, b"reflect", ["reflect"], ("zero",), float("nan")):
        with pytest.raises(ValueError, match="my_call: infill_border"):
            DT.check_infill_border(bad, "my_call")
    depth, bg, masks = R.two_spheres(64)
    K, tf = torch.eye(3), (10.0, Y, Z3)
    for bad in ("mirror", 1, True):
        with pytest.raises(ValueError, match="infill_border"):
            DT.reproject(depth, bg, masks, K, [[tf, tf]], infill_border=bad)
        with pytest.raises(ValueError, match="infill_border"):
            DT.reproject_plan(depth, masks, [[tf, tf]], infill_border=bad)
        with pytest.raises(ValueError, match="infill_border"):
            DT.reproject_border_edits(depth, bg, masks, K, [[tf, tf]], infill_border=bad)
        with pytest.raises(ValueError, match="laplacian_depth_blend: infill_border"):
            DT.laplacian_depth_blend(depth, bg, masks[0], infill_border=bad)


def test_parameter_lists():
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd import depth_transform as DT
    cam = list(inspect.signature(DT.reproject_camera_edits).parameters)
    new = inspect.signature(DT.reproject_border_edits).parameters
    assert list(new) == cam + ["infill_border"] and new["infill_border"].default == "zero"
    for f in (DT.reproject, DT.reproject_plan):
        p = inspect.signature(f).parameters["infill_border"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "zero"
    ps = inspect.signature(DT.laplacian_depth_blend).parameters
    assert list(ps) == ["depth", "bg_depth", "fg_mask", "dilate_iterations", "return_iterations", "infill_border"]
    assert ps["infill_border"].default == "zero"
    # the mesh calls keep their lists (tests/test_footprints_ref.py, tests/test_similarity_ref.py): they take no border
    for f in (DT.transform_depth_mesh, DT.transform_depth, DT.transform_depth_pc, DT.transform_depth_footprints, DT.reproject_edits,
              DT.reproject_object_edits, DT.reproject_camera_edits):
        assert "infill_border" not in inspect.signature(f).parameters, f.__name__
    sig = _lib.SIGNATURES
    for new_name, old_name in (("dh_reproject_border_edits", "dh_reproject_camera_edits"),
                               ("dh_reproject_border_background", "dh_reproject_camera_background"),
                               ("dh_laplacian_blend_border", "dh_laplacian_blend")):
        assert sig[new_name][1] == sig[old_name][1] + [_lib.c_i] and sig[new_name][0] == sig[old_name][0]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diffhandles_hip.h")).read()
    for name in ("dh_reproject_border_edits", "dh_reproject_border_background", "dh_laplacian_blend_border"):
        assert f"int {name}(" in header
    assert "do NOT grow" in header


def test_the_plan_carries_the_border_and_names_the_border_entries():
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, masks = R.two_spheres(64)
    tf = (10.0, Y, Z3)
    cam = (4.0, Y, Z3, None)
    zero = DT.reproject_plan(depth, masks, [[tf, tf]])
    assert zero.infill_border == 0 and RC.fields(zero) == RC.FOOTPRINT
    for value in (None, "zero"):
        p = DT.reproject_plan(depth, masks, [[tf, tf]], infill_border=value)
        assert (p.infill_border, RC.fields(p)) == (0, RC.fields(zero))
    # (the border call is the call it extends with the border, sized as that call is: without a camera the instance call)
    for kw, call in ((dict(), RC.INSTANCE), (dict(footprints=True), RC.INSTANCE), (dict(instances=[0, 1, 0]), RC.INSTANCE),
                     (dict(cameras=[cam]), RC.CAMERA)):
        n = 3 if "instances" in kw else 2
        p = DT.reproject_plan(depth, masks, [[tf] * n], infill_border="reflect", **kw)
        assert (p.kind, p.infill_border, RC.fields(p)) == ("objects", 1, RC.border(call)), kw
        q = DT.reproject_plan(depth, masks, [[tf] * n], **kw)
        assert q.infill_border == 0 and RC.fields(q) != RC.fields(p) and (q.n_pts, q.cap, q.with_table) == (p.n_pts, p.cap, p.with_table)
    p = DT.reproject_plan(depth, [], [[]], removed_masks=masks, infill_border="reflect")
    assert (p.kind, RC.fields(p), p.infill_border) == ("pure_removal", RC.border(RC.BACKGROUND), 1)
    p = DT.reproject_plan(depth, [], [[]], cameras=[cam], infill_border="reflect")
    assert (p.kind, RC.fields(p)) == ("pure_camera", RC.border(RC.CAMERA_BACKGROUND))
    p = DT.reproject_plan(depth, [torch.zeros_like(masks[0])], [[tf]], infill_border="reflect")
    assert p.kind == "empty"
    with pytest.raises(ValueError, match="launches nothing"):
        DT.reproject_record(p, 1)


def test_mesh_mode_refuses_reflect_before_any_device_work():
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, masks = R.two_spheres(64)
    K = torch.eye(3)
    with pytest.raises(NotImplementedError, match="my_call: depth_transform_mode 'mesh' has no reflecting in-fill border"):
        DT.mesh_has_no_infill_border("reflect", "my_call")
    with pytest.raises(ValueError, match="my_call: infill_border"):
        DT.mesh_has_no_infill_border("mirror", "my_call")
    assert DT.mesh_has_no_infill_border("zero", "x") is None and DT.mesh_has_no_infill_border(None, "x") is None
    import test_footprints_ref as FP
    for name, call in FP._every_edit_call(FP._handles("mesh", depth_transform_infill_border="reflect")):
        with pytest.raises(NotImplementedError, match="depth_transform_infill_border"):
            call()
    with pytest.raises(NotImplementedError, match="set_foreground: conf depth_transform_infill_border"):
        FP._handles("mesh", depth_transform_infill_border="reflect").set_foreground(depth, masks[0], bg)
    for name, call in FP._every_edit_call(FP._handles("pc", depth_transform_infill_border="mirror")):
        with pytest.raises(ValueError, match=f"{name}: conf depth_transform_infill_border"):
            call()
    # zero in mesh mode is no error of this setting, and the footprint helper's dict is what it was
    assert FP._handles("mesh", depth_transform_infill_border="zero")._infill_border("x") == "zero"
    assert FP._handles("pc")._infill_border("x") == "zero" and FP._handles("pc", depth_transform_infill_border="reflect")._infill_border("x") == "reflect"
    assert FP._handles("pc", depth_transform_infill_border="reflect")._footprints("x") == dict(footprints=False, footprint_max_ratio=None)
    dh = FP._handles("pc")
    dh.conf = SimpleNamespace(depth_transform_mode="pc")                    # a conf without .get
    assert dh._reproject_keywords("x") == dict(footprints=False, footprint_max_ratio=None, infill_border="zero")
    from diffusionhandles_amd import conf as C
    assert "depth_transform_infill_border" not in C.load_default()


def test_the_conf_key_reaches_the_plan_of_every_edit_call_and_the_blend(monkeypatch):
    from diffusionhandles_amd import depth_transform as DT
    from diffusionhandles_amd import diffusion_handles as DHM
    import test_footprints_ref as FP

    class Reached(Exception):
        pass

    seen = []

    def run_plan(p, *a, **kw):
        seen.append(p.infill_border)
        raise Reached

    def blend(depth, bg_depth, fg_mask, dilate_iterations=15, return_iterations=False, infill_border="zero"):
        seen.append(infill_border)
        raise Reached

    monkeypatch.setattr(DT, "_run_plan", run_plan)
    monkeypatch.setattr(DHM, "laplacian_depth_blend", blend)
    depth, bg, masks = R.two_spheres(128)
    for keys, want, blend_want in ((dict(), 0, "zero"), (dict(depth_transform_infill_border="zero"), 0, "zero"),
                                   (dict(depth_transform_infill_border="reflect"), 1, "reflect"),
                                   (dict(depth_transform_infill_border="reflect", depth_transform_footprints=True), 1, "reflect")):
        dh = FP._handles("pc", **keys)
        for name, call in FP._every_edit_call(dh):
            seen.clear()
            with pytest.raises(Reached):
                call()
            assert seen == [want], (name, keys, seen)
        seen.clear()
        with pytest.raises(Reached):
            dh.set_foreground(depth, masks, bg)
        assert seen == [blend_want]


def test_run_edit_infill_border_argument():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import run_edit
    from diffusionhandles_amd import conf as C
    for extra in ([], ["--test-set", "t.json"], ["--test-set", "t.json", "--edit-batch", "2"]):
        conf = C.load_default()
        assert run_edit.apply_border_args(run_edit.parse(["--scene", "x"] + extra), conf) == {}
        assert "depth_transform_infill_border" not in conf
        conf = C.load_default()
        args = run_edit.parse(["--scene", "x", "--infill-border", "reflect"] + extra)
        assert run_edit.apply_border_args(args, conf) == dict(infill_border="reflect") == args.border_report
        assert conf.depth_transform_infill_border == "reflect"
        conf = C.load_default()
        assert run_edit.apply_border_args(run_edit.parse(["--scene", "x", "--infill-border", "zero"] + extra), conf) == {}
    with pytest.raises(SystemExit):
        run_edit.parse(["--scene", "x", "--infill-border", "mirror"])
    conf = C.load_default()
    conf.depth_transform_mode = "mesh"
    with pytest.raises(NotImplementedError, match="infill_border"):
        run_edit.apply_border_args(run_edit.parse(["--scene", "x", "--infill-border", "reflect"]), conf)
    assert run_edit.apply_border_args(run_edit.parse(["--scene", "x", "--infill-border", "zero"]), conf) == {}
    # a configuration file that carries the key is honoured without the flag, and a malformed one is refused
    conf = C.load_default()
    conf["depth_transform_infill_border"] = "reflect"
    assert run_edit.apply_border_args(run_edit.parse(["--scene", "x"]), conf) == dict(infill_border="reflect")
    conf["depth_transform_infill_border"] = "mirror"
    with pytest.raises(ValueError, match="--infill-border"):
        run_edit.apply_border_args(run_edit.parse(["--scene", "x"]), conf)
