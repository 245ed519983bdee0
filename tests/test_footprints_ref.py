"""CPU: footprint splatting -- the test-side reference tests/footprints_ref.py (off = similarity_ref, the identity edit,
the contrast with the point path that motivates the mode, the rules on a hand-made triangle), the host layers (keywords,
refusals before any device work, conf keys, tools/run_edit.py arguments) and the C ABI's declarations."""
import inspect
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_object_ref as R  # noqa: E402
import similarity_ref as S  # noqa: E402
import footprints_ref as F  # noqa: E402
from oracle import depth_ref as D  # noqa: E402

Y, Z3 = R.Y, (0.0, 0.0, 0.0)
_CACHE = {}


def ref(res, name, footprints):
    """One reference per (resolution, edit, setting), computed once under the written-out dot order."""
    key = (res, name, footprints)
    if key not in _CACHE:
        depth, bg, masks = R.two_spheres(res)
        D.DOT_ORDER = "explicit"
        try:
            _CACHE[key] = F.transform_objects(depth, bg, masks, getattr(F, name), footprints=footprints)
        finally:
            D.DOT_ORDER = "blas"
    return _CACHE[key]


# ---- the reference ------------------------------------------------------------------------------------------------------------
def test_footprints_off_is_the_similarity_reference():
    depth, bg, masks = R.two_spheres(128)
    D.DOT_ORDER = "explicit"
    try:
        want = S.transform_objects(depth, bg, masks, F.SCALE3)
    finally:
        D.DOT_ORDER = "blas"
    got = ref(128, "SCALE3", False)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for k in ("zmap", "raw_mask", "cleaned", "vis", "tx", "ty", "inpaint", "disparity", "points", "obj_start"):
        assert np.array_equal(got[2][k], want[2][k]), k


@pytest.mark.parametrize("res,n_corr,n_fill", [(128, 2119, 168), (256, 8854, 0)])
def test_identity_edit_gives_the_point_path(res, n_corr, n_fill):
    """Nothing moves: every triangle covers its own three pixels at the depth of their points, so the footprints change
    nothing -- the same correspondences (the order is the target's: compared as sets), the same masks and the same in-fill.
    The depth map is the point path's only up to this: the identity still rounds q = P - c to float32, so a point lands
    within |du| + |dv| <= 2 * (res / 2) * fx * 2^-24 * |q| / Z < 3e-6 pixels of its pixel centre (|q| < 0.5, Z > 2, fx < 2), and
    a triangle covering that centre mixes in at most that weight of its other vertices, whose depths differ by less than 0.6
    (the spheres are 0.5 deep): |dz| < 4e-6, and 255 / (max - min) * dz / z^2 < 1e-3 in the normalised disparity."""
    (d0, c0, g0), (d1, c1, g1) = ref(res, "IDENTITY", False), ref(res, "IDENTITY", True)
    assert len(c0) == len(c1) == n_corr and int(g0["inpaint"].sum()) == int(g1["inpaint"].sum()) == n_fill
    rows = lambda c: sorted(map(tuple, c.numpy().tolist()))
    assert rows(c0) == rows(c1)
    assert all(tuple(r[:2]) == tuple(r[2:]) for r in c1.numpy().tolist())
    for k in ("raw_mask", "cleaned", "vis", "inpaint"):
        assert np.array_equal(g0[k], g1[k]), k
    dz, dd = float(np.abs(g0["zmap"] - g1["zmap"]).max()), float((d0 - d1).abs().max())
    print(f"identity at {res}: depth map within {dz:.2e}, disparity within {dd:.2e}")
    assert dz < 4e-6 and dd < 1e-3
    # row-major in the target
    t = c1.numpy()[:, 3] * res + c1.numpy()[:, 2]
    assert (np.diff(t) > 0).all()


def test_contrast_with_the_point_path_on_an_enlarged_object():
    """Object 0 at scale 3 with a turn, 256 x 256: the points leave most of the cleaned mask to the harmonic in-fill and a
    sparse sample of correspondences; the footprints fill the silhouette (conditions on the reference alone)."""
    (_, c0, g0), (_, c1, g1) = ref(256, "SCALE3", False), ref(256, "SCALE3", True)
    share0, share1 = F.infill_share(g0), F.infill_share(g1)
    print(f"in-fill share: points {share0:.3f}, footprints {share1:.4f}; correspondences {len(c0)} / {len(c1)}")
    assert share1 < 0.02 and share0 > 0.5
    assert len(c1) >= 4 * len(c0)
    assert len(c1) > int(g1["obj_start"][-1])                  # more rows than foreground points
    # at 128 the CLOSE element no longer bridges the gaps of the point path: the mask breaks up
    (_, _, h0), (_, _, h1) = ref(128, "SCALE3", False), ref(128, "SCALE3", True)
    assert int((h0["cleaned"] != 0).sum()) < 0.3 * int((h1["cleaned"] != 0).sum())


@pytest.mark.parametrize("name", ["SCALE3", "IDENTITY"])
def test_every_correspondence_starts_in_the_mask_of_its_object(name):
    masks = R.two_spheres(128)[2]
    _, corr, dbg = ref(128, name, True)
    c = corr.numpy()
    per = S.pairs_per_object(corr, masks)
    assert sum(per) == len(c) and min(per) > 0
    # the owner of the target pixel is the point the row starts at, and that point is visible
    owner = dbg["owner"].reshape(128, 128)[c[:, 3], c[:, 2]] - 128 * 128
    assert (owner >= 0).all() and dbg["vis"][owner].all()
    src = np.concatenate([np.nonzero(m[0, 0].numpy().reshape(-1) > 0.5)[0] for m in masks])
    assert np.array_equal(src[owner], c[:, 1] * 128 + c[:, 0])
    obj = np.searchsorted(dbg["obj_start"], owner, side="right") - 1
    for m in range(2):
        assert (masks[m][0, 0].numpy()[c[obj == m, 1], c[obj == m, 0]] > 0.5).all()
    assert int(dbg["vis"].sum()) >= len(np.unique(owner))          # (a point may own pixels outside the cleaned mask only)


def test_rules_on_one_hand_made_quad():
    """A 2 x 2 source quad whose points land on (0,0) (2,0) (0,2) (2,2) of a 4 x 4 target: the box, the inclusive edges, the
    affine depth, the bidder (largest weight, ties to the earlier vertex), the back face, the ratio guard."""
    res = 4
    src = np.array([0, 1, 4, 5])                                          # v00 v01 v10 v11
    u, v = np.array([0.0, 2.0, 0.0, 2.0]), np.array([0.0, 0.0, 2.0, 2.0])
    z = np.array([1.0, 2.0, 3.0, 4.0])
    obj = np.zeros(4, dtype=np.int64)
    depth = np.full(16, 2.0, dtype=np.float32)
    pix, zz, who = F.footprint_bids(u, v, z, src, obj, depth, res)
    bids = sorted(zip(pix.tolist(), zz.tolist(), who.tolist()))
    # half 0 = (v10, v11, v01): the pixels with x + y >= 2; half 1 = (v10, v01, v00): x + y <= 2; the diagonal belongs to both
    lower = {(x, y) for x in range(3) for y in range(3) if x + y >= 2}
    upper = {(x, y) for x in range(3) for y in range(3) if x + y <= 2}
    assert sorted(p for p, _, _ in bids) == sorted([y * res + x for x, y in lower] + [y * res + x for x, y in upper])
    plane = lambda x, y: 1.0 + 0.5 * x + 1.0 * y                          # the quad's four depths lie in one plane
    for p, d, _ in bids:
        assert d == plane(p % res, p // res)
    at = lambda x, y: [w for p, _, w in bids if p == y * res + x]
    assert at(0, 0) == [0] and at(2, 2) == [3]
    assert at(0, 2) == [2, 2] and at(2, 0) == [1, 1]
    assert at(1, 1) == [2, 2]                  # w of v10 and v01 tie on the diagonal's middle: the earlier vertex, v10, bids
    assert at(1, 2) == [2] and at(1, 0) == [1]         # ties between v10 / v11 and v01 / v00: the earlier of the order
    # mirrored (the quad seen from behind): both triangles have area < 0 and are dropped
    assert len(F.footprint_bids(2.0 - u, v, z, src, obj, depth, res)[0]) == 0
    # Z <= 0 or a non-finite coordinate drops the triangles of that vertex; here v10, a vertex of both
    for bad in (dict(z=np.array([1.0, 2.0, 0.0, 4.0])), dict(u=np.array([0.0, 2.0, np.inf, 2.0]))):
        a = dict(u=u, v=v, z=z)
        a.update(bad)
        assert len(F.footprint_bids(a["u"], a["v"], a["z"], src, obj, depth, res)[0]) == 0
    # the ratio guard reads the SOURCE depths as float32: 2.0 against 2.3 passes 1.2 and fails 1.1
    depth[5] = 2.3
    assert len(F.footprint_bids(u, v, z, src, obj, depth, res, 1.2)[0]) == len(bids)
    assert len(F.footprint_bids(u, v, z, src, obj, depth, res, 1.1)[0]) == len(upper)           # half 0 has v11
    # two objects: no triangle across them
    assert len(F.footprint_bids(u, v, z, src, np.array([0, 0, 0, 1]), depth, res)[0]) == len(upper)
    # the box is clipped to the image: the quad stretched over (-1, -1) .. (3, 3) bids at the 16 pixels of 4 x 4 and nowhere else
    pix2, _, _ = F.footprint_bids(2 * u - 1, 2 * v - 1, z, src, obj, np.full(16, 2.0, dtype=np.float32), res)
    assert set(pix2.tolist()) == set(range(16))


def test_step_scene_guard_removes_the_sheets():
    depth, bg, masks = F.step_scene(64)
    owned = {}
    for ratio in (None, 1.1):
        _, corr, dbg = F.transform_objects(depth, bg, masks, F.STEP_TURN, footprints=True, max_ratio=ratio, infill=False)
        owned[ratio] = int(dbg["raw_mask"].sum())
    assert owned[1.1] < owned[None]


# ---- the host layers --------------------------------------------------------------------------------------------------------
BAD_RATIOS = [1.0, 0.5, -3.0, 0.0, float("nan"), float("inf"), 1e39, "wide", (1.5, 2.0)]


@pytest.mark.parametrize("bad", BAD_RATIOS)
def test_bad_ratios_raise_before_any_device_work(bad):
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, masks = R.two_spheres(128)
    K, tf = torch.eye(3), (10.0, Y, Z3)
    with pytest.raises(ValueError, match="footprint_max_ratio"):
        DT.check_footprints(True, bad)
    with pytest.raises(ValueError, match="footprint_max_ratio"):
        DT.reproject_edits(depth, bg, masks[0], K, [tf], footprints=True, footprint_max_ratio=bad)
    with pytest.raises(ValueError, match="footprint_max_ratio"):
        DT.reproject_object_edits(depth, bg, masks, K, [[tf, tf]], footprints=True, footprint_max_ratio=bad)
    with pytest.raises(ValueError, match="footprint_max_ratio"):
        DT.transform_depth_footprints(depth, bg, masks[0], K, 10.0, footprints=True, footprint_max_ratio=bad)
    with pytest.raises(ValueError, match="footprint_max_ratio"):
        DT.transform_depth_mesh(depth, bg, masks[0], K, 10.0, footprints=True, footprint_max_ratio=bad)


def _handles(mode, **keys):
    from diffusionhandles_amd import DiffusionHandles
    from diffusionhandles_amd import conf as C
    dh = object.__new__(DiffusionHandles)
    dh.conf = C.Conf(depth_transform_mode=mode, **keys)
    dh.diffuser = SimpleNamespace(get_depth_intrinsics=lambda device=None: torch.eye(3), unet=None)
    return dh


def _every_edit_call(dh):
    """The five edit entries of DiffusionHandles, as thunks (name, call)."""
    depth, bg, masks = R.two_spheres(128)
    tf = (10.0, Y, Z3)
    common = dict(depth=depth, prompt="two spheres", bg_depth=bg, null_text_emb=None, init_noise=None, activations=[depth])
    return [
        ("transform_foreground", lambda: dh.transform_foreground(depth, "two spheres", masks[0], bg, None, None, None, rot_angle=10.0)),
        ("transform_foreground_batch", lambda: dh.transform_foreground_batch(depth, "two spheres", masks[0], bg, None, None, None, [tf, tf])),
        ("transform_foreground_objects", lambda: dh.transform_foreground_objects(depth, "two spheres", masks, bg, None, None, None, [tf, tf])),
        ("transform_foreground_objects_batch",
         lambda: dh.transform_foreground_objects_batch(depth, "two spheres", masks, bg, None, None, None, [[tf, tf]])),
        ("transform_foregrounds", lambda: dh.transform_foregrounds([dict(common, fg_mask=masks[0]),
                                                                    dict(common, fg_masks=masks, transforms=[tf, tf])])),
    ]


def test_ratio_without_footprints_and_mesh_mode_are_refused_before_any_device_work():
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, masks = R.two_spheres(128)
    K, tf = torch.eye(3), (10.0, Y, Z3)
    assert DT.check_footprints(False, None) == (False, None) and DT.check_footprints(1, None) == (True, None)
    assert DT.check_footprints(True, 1.5) == (True, 1.5) and DT.check_footprints(True, 1.1)[1] == float(np.float32(1.1))
    with pytest.raises(ValueError, match="without footprints"):
        DT.reproject_edits(depth, bg, masks[0], K, [tf], footprint_max_ratio=1.5)
    with pytest.raises(ValueError, match="without footprints"):
        DT.reproject_object_edits(depth, bg, masks, K, [[tf, tf]], footprints=False, footprint_max_ratio=2.0)
    with pytest.raises(ValueError, match="without footprints"):
        DT.transform_depth_footprints(depth, bg, masks[0], K, 10.0, footprint_max_ratio=1.5)
    # mesh mode has no footprints: the setting is named
    with pytest.raises(NotImplementedError, match="footprints"):
        DT.transform_depth_mesh(depth, bg, masks[0], K, 10.0, footprints=True)
    with pytest.raises(NotImplementedError, match="footprints"):
        DT.transform_depth_mesh(depth, bg, masks[0], K, 10.0, footprints=True, footprint_max_ratio=1.5)
    for name, call in _every_edit_call(_handles("mesh", depth_transform_footprints=True)):
        with pytest.raises(NotImplementedError, match="depth_transform_footprints"):
            call()
    # the conf keys are checked like the keywords, in every entry
    for keys, word in ((dict(depth_transform_footprints=True, depth_transform_footprint_max_ratio=0.9), "footprint_max_ratio"),
                       (dict(depth_transform_footprint_max_ratio=1.5), "without footprints")):
        for name, call in _every_edit_call(_handles("pc", **keys)):
            with pytest.raises(ValueError, match=word):
                call()
    # absent keys = off; a false key in mesh mode is no error of this setting
    assert _handles("pc")._footprints("x") == dict(footprints=False, footprint_max_ratio=None)
    assert _handles("mesh", depth_transform_footprints=False)._footprints("x") == dict(footprints=False, footprint_max_ratio=None)
    assert _handles("pc", depth_transform_footprints=True, depth_transform_footprint_max_ratio=1.25)._footprints("x") == dict(
        footprints=True, footprint_max_ratio=1.25)
    dh = _handles("pc")
    dh.conf = SimpleNamespace(depth_transform_mode="pc")                    # a conf without .get
    assert dh._footprints("x") == dict(footprints=False, footprint_max_ratio=None)
    # without a GPU a well-formed call gets as far as the device and fails loudly there
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            DT.reproject_edits(depth, bg, masks[0], K, [tf], footprints=True, footprint_max_ratio=1.5)
        for name, call in _every_edit_call(_handles("pc", depth_transform_footprints=True)):
            with pytest.raises(RuntimeError):
                call()


def test_default_configuration_does_not_carry_the_keys():
    from diffusionhandles_amd import conf as C
    conf = C.load_default()
    assert "depth_transform_footprints" not in conf and "depth_transform_footprint_max_ratio" not in conf
    assert conf.get("depth_transform_footprints", False) is False


def test_signatures():
    from diffusionhandles_amd import depth_transform as DT
    tail = ["footprints", "footprint_max_ratio"]
    ref8 = ["depth", "bg_depth", "fg_mask", "intrinsics", "rot_angle", "rot_axis", "translation", "use_input_depth_normalization"]
    for f in (DT.reproject_edits, DT.reproject_object_edits, DT.transform_depth_footprints, DT.transform_depth_mesh):
        sig = inspect.signature(f)
        assert list(sig.parameters)[-2:] == tail, f.__name__
        assert sig.parameters["footprints"].default is False and sig.parameters["footprint_max_ratio"].default is None
    assert list(inspect.signature(DT.reproject_edits).parameters)[:-2] == [
        "depth", "bg_depth", "fg_mask", "intrinsics", "transforms", "use_input_depth_normalization", "return_debug", "device_correspondences"]
    assert list(inspect.signature(DT.reproject_object_edits).parameters)[:-2] == [
        "depth", "bg_depth", "fg_masks", "intrinsics", "edits", "use_input_depth_normalization", "return_debug", "device_correspondences"]
    # the reference's parameters stay a prefix; transform_depth / transform_depth_pc keep the lists they had
    assert list(inspect.signature(DT.transform_depth_footprints).parameters) == ref8 + ["scale", "pivot"] + tail
    assert list(inspect.signature(DT.transform_depth_pc).parameters) == ref8 + ["scale", "pivot"]
    assert list(inspect.signature(DT.transform_depth).parameters)[:8] == ref8
    assert list(inspect.signature(DT.transform_depth_mesh).parameters)[:8] == ref8


def test_header_table_and_library_have_the_entries():
    from diffusionhandles_amd import _lib
    raw = open(os.path.join(ROOT, "include", "diffhandles_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"int\s+dh_reproject_footprint_edits\s*\(([^;]*)\)\s*;", code)
    s = re.search(r"int\s+dh_reproject_similarity_edits\s*\(([^;]*)\)\s*;", code)
    assert m and s
    norm = lambda t: [re.sub(r"\s+", " ", a.strip()) for a in t.split(",")]
    assert norm(m.group(1)) == norm(s.group(1)) + ["int footprints", "float max_ratio", "int corr_capacity"]
    assert re.search(r"int\s+dh_reproject_footprints_workspace_bytes\s*\(\s*int res, int n_fg, int n_edits, int n_objects, int footprints, "
                     r"size_t\* bytes\)", code)
    sim, fp = _lib.SIGNATURES["dh_reproject_similarity_edits"], _lib.SIGNATURES["dh_reproject_footprint_edits"]
    assert fp[1][:len(sim[1])] == sim[1] and fp[1][len(sim[1]):] == [_lib.c_i, _lib.c_f, _lib.c_i]
    assert "dh_reproject_footprints_workspace_bytes" in _lib.SIGNATURES and "dh_dbg_footprint_tier" in _lib.DEBUG_SIGNATURES
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        assert L.dh_missing_symbols == []
        import ctypes
        a, b = ctypes.c_size_t(), ctypes.c_size_t()
        assert L.dh_reproject_objects_workspace_bytes(128, 1000, 3, 2, ctypes.byref(a)) == 0
        assert L.dh_reproject_footprints_workspace_bytes(128, 1000, 3, 2, 0, ctypes.byref(b)) == 0 and a.value == b.value
        assert L.dh_reproject_footprints_workspace_bytes(128, 1000, 3, 2, 1, ctypes.byref(b)) == 0 and b.value > a.value
        assert L.dh_reproject_footprints_workspace_bytes(128, 1000, 3, 2, 2, ctypes.byref(b)) != 0


# ---- tools/run_edit.py ------------------------------------------------------------------------------------------------------
def test_run_edit_arguments():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import run_edit
    from diffusionhandles_amd import conf as C
    for extra in ([], ["--test-set", "set.json"], ["--test-set", "set.json", "--edit-batch", "4"]):
        args = run_edit.parse(["--scene", "x"] + extra)
        assert args.footprints is False and args.footprint_max_ratio is None
        conf = C.load_default()
        assert run_edit.apply_footprint_args(args, conf) == dict(footprints=False, footprint_max_ratio=None)
        assert "depth_transform_footprints" not in conf
        args = run_edit.parse(["--scene", "x", "--footprints", "--footprint-max-ratio", "1.25"] + extra)
        conf = C.load_default()
        assert run_edit.apply_footprint_args(args, conf) == dict(footprints=True, footprint_max_ratio=1.25)
        assert conf.depth_transform_footprints is True and conf.depth_transform_footprint_max_ratio == 1.25
        assert args.footprint_report == dict(footprints=True, footprint_max_ratio=1.25)
    conf = C.load_default()
    with pytest.raises(ValueError, match="without footprints"):
        run_edit.apply_footprint_args(run_edit.parse(["--scene", "x", "--footprint-max-ratio", "1.5"]), conf)
    conf = C.load_default()
    with pytest.raises(ValueError, match="footprint_max_ratio"):
        run_edit.apply_footprint_args(run_edit.parse(["--scene", "x", "--footprints", "--footprint-max-ratio", "1.0"]), conf)
    conf = C.load_default()
    conf.depth_transform_mode = "mesh"
    with pytest.raises(NotImplementedError, match="footprints"):
        run_edit.apply_footprint_args(run_edit.parse(["--scene", "x", "--footprints"]), conf)
    # a configuration file that carries the key is honoured without the flag
    conf = C.load_default()
    conf["depth_transform_footprints"] = True
    assert run_edit.apply_footprint_args(run_edit.parse(["--scene", "x"]), conf)["footprints"] is True
