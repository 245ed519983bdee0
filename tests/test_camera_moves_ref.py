"""CPU: camera moves ("Camera moves") -- the reference statement tests/camera_moves_ref.py against itself and
against the geometry, the host's view row and validator, the cells with row kinds, the parameter lists.  No GPU."""
import inspect

import numpy as np
import pytest
import torch

import camera_moves_ref as CM
import multi_object_ref as R
import object_removal_ref as RM
import similarity_ref as S
from oracle import depth_ref as D

from diffusionhandles_amd import depth_transform as DT
from diffusionhandles_amd import losses

SIZES = (128, 256)


def plain_f64_view(points, camera):
    """The plain f64 composition: the exact inverse of the camera's motion, P' = R(-theta) (P - c - t) + c, with no f32
    rounding of the points or of the translation."""
    angle, axis, trans = camera[:3]
    pivot = camera[3] if len(camera) == 4 else None
    a = np.asarray(axis, dtype=np.float32)
    a = (a / np.linalg.norm(a)).astype(np.float64)
    t = np.asarray(trans, dtype=np.float32).astype(np.float64)
    c = np.zeros(3) if pivot is None else np.asarray(pivot, dtype=np.float32).astype(np.float64)
    th = np.radians(-float(angle))
    q = np.asarray(points, dtype=np.float64) - c - t
    return q * np.cos(th) + np.cross(a, q) * np.sin(th) + a * (q @ a)[:, None] * (1.0 - np.cos(th)) + c


@pytest.mark.parametrize("name", CM.CAMERA_NAMES)
def test_every_fixture_leaves_the_trivial_case(name):
    f = CM.fixture(128)
    _, corr, dbg = f["geo"][name]
    assert int(dbg["unowned"].sum()) >= 500
    assert dbg["n_background"] >= 5000
    per = np.bincount(dbg["corr_inst"][:dbg["n_instance_rows"]].astype(np.int64), minlength=2)
    assert per.min() >= 50, per
    assert (dbg["corr_inst"][dbg["n_instance_rows"]:] == 2).all() and (dbg["row_kind"][dbg["n_instance_rows"]:] == 2).all()
    assert corr.shape[0] == dbg["n_instance_rows"] + dbg["n_background"]
    # the background rows are in ascending source pixel order and start outside the masks
    b = corr.numpy()[dbg["n_instance_rows"]:]
    src = b[:, 1] * 128 + b[:, 0]
    assert (np.diff(src) > 0).all()
    union = sum((m[0, 0].numpy() != 0) for m in f["masks"])
    assert not union[b[:, 1], b[:, 0]].any()
    # a discarded foreground point: not visible, target (-1, -1)
    gone = dbg["gone"][128 * 128:]
    assert not dbg["vis"][gone].any() and (dbg["tx"][gone] == -1).all() and (dbg["ty"][gone] == -1).all()


def test_the_discard_is_exercised():
    f = CM.fixture(128)
    for name in ("pan", "dolly_in", "general"):
        assert int(f["geo"][name][2]["gone"].sum()) >= 500, name
    assert int(f["geo"]["dolly_out"][2]["gone"].sum()) == 0
    assert int(f["geo"]["none"][2]["gone"].sum()) == 0 and f["geo"]["none"][2]["n_background"] == 0


@pytest.mark.parametrize("res", SIZES)
def test_owner_map_is_tied_to_the_plain_f64_composition(res):
    """A cap, not a tolerance: the f32-rounded composition and a plain f64 one give the same pixel owner on all but at most
    1e-3 of the pixels (measured: DESIGN.md, "Camera moves")."""
    f = CM.fixture(res)
    worst = 0.0
    for name in CM.CAMERA_NAMES:
        cam = f["cameras"][name]
        _, _, plain = CM.transform_camera(f["depth"], f["bg_depth"], f["masks"], [0, 1], f["transforms"], cam, infill=False,
                                          view_fn=plain_f64_view)
        share = float((plain["owner"] != f["geo"][name][2]["owner"]).mean())
        print(f"owner map vs plain f64, {name} at {res}: {share:.2e}")
        worst = max(worst, share)
        assert share <= 1e-3, (name, share)
    print(f"worst share at {res}: {worst:.2e}")


def test_edit_without_a_camera_is_the_instance_reference():
    import object_copies_ref as C
    f = CM.fixture(128)
    disp, corr, dbg = f["geo"]["none"]
    d2, c2, g2 = C.transform_instances(f["depth"], f["bg_depth"], f["masks"], [0, 1], f["transforms"])
    assert torch.equal(corr, c2) and torch.equal(disp, d2)
    assert np.array_equal(dbg["vis"], g2["vis"]) and np.array_equal(dbg["tx"], g2["tx"]) and np.array_equal(dbg["zmap"], g2["zmap"])
    assert np.array_equal(dbg["corr_inst"], g2["corr_inst"])


@pytest.mark.parametrize("res", SIZES)
def test_pure_case_with_the_identity_view_is_the_pure_removal(res):
    depth, bg, masks = R.two_spheres(res)
    identity = (0.0, R.Y, (0.0, 0.0, 0.0), None)
    disp, corr, dbg = CM.background_camera(bg, identity, removed_masks=masks)
    ref, rdbg = RM.background_alone(bg)
    assert np.array_equal(dbg["zmap"], rdbg["zmap"]) and np.array_equal(dbg["unowned"], rdbg["unowned"])
    assert not dbg["gone"].any()
    if not rdbg["unowned"].any():
        assert torch.equal(disp, ref)
    # every background pixel outside the removed masks that owns its pixel yields the identity row
    c = corr.numpy()
    assert (c[:, 0] == c[:, 2]).all() and (c[:, 1] == c[:, 3]).all() and (dbg["row_kind"] == 2).all()
    union = sum((m[0, 0].numpy() != 0) for m in masks)
    assert len(c) == int((~union.astype(bool)).sum())


@pytest.mark.parametrize("name", CM.CAMERA_NAMES)
def test_view_inverts_the_camera_motion(name):
    f = CM.fixture(128)
    cam = f["cameras"][name]
    pts = D.unproject(f["bg_depth"][0, 0].numpy()).reshape(-1, 3).astype(np.float64)
    back = CM.view_apply(CM.camera_move(pts, cam), cam)
    assert np.abs(back - pts).max() <= 1e-5
    # and the host's row is the reference's, double for double
    assert np.array_equal(DT.view_row(DT.check_camera(cam)), CM.view_row(cam))


@pytest.mark.parametrize("erosion", (0, 5))
def test_cells_background_rows_leave_both_masks(erosion):
    f = CM.fixture(128)
    _, corr, dbg = f["geo"]["orbit"]
    c, kind, n = corr.numpy(), dbg["row_kind"], dbg["n_instance_rows"]
    with_bg = CM.cells(c, 128, kind, None, erosion)
    without = CM.cells(c[:n], 128, kind[:n], None, erosion)
    assert np.array_equal(with_bg["masks"], without["masks"])
    for k in RM.CELL_KEYS[4:]:
        assert np.array_equal(with_bg[k], without[k]), k
    assert len(with_bg["original_x"]) == len(c) and len(without["original_x"]) == n
    # as plain rows they WOULD clear cells: the kind is what keeps the lists
    plain = CM.cells(c, 128, None, None, erosion)
    assert plain["masks"][1].sum() < with_bg["masks"][1].sum()


BAD_CAMERAS = [
    ((1.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), "rot_axis must not be zero"),
    ((float("nan"), R.Y, (0.0, 0.0, 0.0)), "rot_angle must be finite"),
    ((float("inf"), R.Y, (0.0, 0.0, 0.0)), "rot_angle must be finite"),
    ((1.0, (0.0, float("nan"), 0.0), (0.0, 0.0, 0.0)), "rot_axis must be finite"),
    ((1.0, R.Y, (0.0, float("inf"), 0.0)), "translation must be finite"),
    ((1.0, R.Y, (0.0, 0.0, 0.0), (0.0, float("nan"), 1.0)), "pivot must be finite"),
    ((1.0, R.Y, (0.0, 0.0)), "translation must be three numbers"),
    ((1.0, R.Y, (0.0, 0.0, 0.0), (1.0, 2.0)), "pivot must be three numbers"),
    ((1.0, R.Y), "expected"),
    (5.0, "expected"),
]


@pytest.mark.parametrize("camera,msg", BAD_CAMERAS)
def test_check_camera_raises_naming_the_call_and_the_edit(camera, msg):
    with pytest.raises(ValueError, match="reproject_camera_edits: edit 1.*" + msg):
        DT.check_camera(camera, "reproject_camera_edits: edit 1")
    # through the public call, before any device work (no GPU here): the second edit's camera is the bad one
    depth, bg, masks = R.two_spheres(128)
    tfs = S.edits_for(128, depth)[0]
    with pytest.raises(ValueError, match="reproject_camera_edits: edit 1.*" + msg):
        DT.reproject_camera_edits(depth, bg, masks, D.intrinsics_f32(), [tfs, tfs], cameras=[None, camera])


def test_check_camera_accepts_and_normalises():
    assert DT.check_camera(None) is None
    ang, ax, tr, pv = DT.check_camera((torch.tensor(4.0), torch.tensor([0.0, 2.0, 0.0]), np.array([0.1, 0.2, 0.3])))
    assert ang == 4.0 and ax == [0.0, 2.0, 0.0] and pv is None and tr == [float(np.float32(v)) for v in (0.1, 0.2, 0.3)]
    row = DT.view_row((ang, ax, tr, pv))
    assert row[14] == 1.0 and row[15] == 0.0 and (row[8:11] == 1.0).all() and (row[11:14] == 0.0).all()
    assert row[3] == np.cos(np.radians(-4.0)) and row[4] == np.sin(np.radians(-4.0)) and list(row[0:3]) == [0.0, 1.0, 0.0]


def test_refusals_and_list_lengths_before_any_device_work():
    depth, bg, masks = R.two_spheres(128)
    tfs = S.edits_for(128, depth)[0]
    cam = (4.0, R.Y, (0.0, 0.0, 0.0))
    K = D.intrinsics_f32()
    with pytest.raises(NotImplementedError, match="footprints with a camera"):
        DT.reproject_camera_edits(depth, bg, masks, K, [tfs], footprints=True, cameras=[cam])
    with pytest.raises(ValueError, match="cameras has 2 entries for 1 edits"):
        DT.reproject_camera_edits(depth, bg, masks, K, [tfs], cameras=[cam, cam])
    with pytest.raises(ValueError, match="no foreground mask"):
        DT.reproject_camera_edits(depth, bg, [], K, [tfs], cameras=[cam])


def test_parameter_lists():
    ps = inspect.signature(DT.reproject_camera_edits).parameters
    donor = inspect.signature(DT.reproject_donor_edits).parameters
    assert list(ps)[:-1] == list(donor) and list(ps)[-1] == "cameras" and ps["cameras"].default is None
    ps = inspect.signature(losses.process_correspondences).parameters
    assert ps["row_kind"].default is None and ps["row_donor"].default is None
    assert list(ps)[-3:] == ["vacated", "object_labels", "pair_instances"]
    assert list(inspect.signature(DT.orbit_cameras).parameters) == ["depth", "intrinsics", "x", "y", "angles", "axis"]
    assert list(inspect.signature(DT.check_camera).parameters) == ["camera", "what"]


def test_row_kind_checks_before_any_device_work():
    corr = np.zeros((3, 4), dtype=np.int64)
    with pytest.raises(ValueError, match="row_kind has 2 entries for 3"):
        losses.process_correspondences(corr, 128, row_kind=np.zeros(2, dtype=np.uint8))
    with pytest.raises(ValueError, match="mutually exclusive"):
        losses.process_correspondences(corr, 128, row_donor=np.zeros(3, dtype=np.uint8), row_kind=np.zeros(3, dtype=np.uint8))


def test_header_declares_the_camera_entries():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "diffhandles_hip.h")).read()
    from diffusionhandles_amd import _lib
    for name in ("dh_reproject_camera_edits", "dh_reproject_camera_workspace_bytes", "dh_reproject_camera_background",
                 "dh_cells_from_correspondences_rows"):
        assert name + "(" in txt and name in _lib.SIGNATURES
    donor, cam = _lib.SIGNATURES["dh_reproject_donor_edits"][1], _lib.SIGNATURES["dh_reproject_camera_edits"][1]
    assert cam[:len(donor)] == donor and len(cam) == len(donor) + 5
    assert len(_lib.SIGNATURES["dh_reproject_camera_background"][1]) == len(_lib.SIGNATURES["dh_reproject_background"][1]) + 4


# ---- scene directories ------------------------------------------------------------------------------------------------------
def _write_scene(path, transforms, multi=False):
    import json
    from diffusionhandles_amd.scene_io import write_png
    depth, bg, masks = R.two_spheres(128)
    path.mkdir(parents=True, exist_ok=True)
    np.save(path / "depth.npy", depth[0, 0].numpy())
    np.save(path / "bg_depth.npy", bg[0, 0].numpy())
    if multi:
        for m, mask in enumerate(masks):
            write_png(str(path / f"mask_{m}.png"), mask[0, 0].numpy())
    else:
        write_png(str(path / "mask.png"), masks[0][0, 0].numpy())
    (path / "transforms.json").write_text(json.dumps(transforms))


def test_scene_syntax_camera_entries(tmp_path):
    from diffusionhandles_amd import scene_io
    cam = {"rot_angle": 6.0, "rot_axis": [0.3, 0.9, -0.2], "translation": [0.1, -0.05, 0.15], "pivot_pixel": [64, 64]}
    plain = {"rotation_angle": 10.0, "translation": [0.1, 0.0, 0.0]}
    _write_scene(tmp_path / "one", {"plain": plain, "both": dict(plain, camera=cam), "pure": {"camera": {"rot_angle": 4.0}}})
    geo = scene_io.load_scene_geometry(str(tmp_path / "one"), 128)
    args = {n: scene_io.transform_args(t) for n, t in geo["transforms"].items()}
    assert "camera" not in args["plain"] and set(args["plain"]) == {"rot_angle", "rot_axis", "translation"}
    assert args["both"]["camera"] == dict(rot_angle=6.0, rot_axis=(0.3, 0.9, -0.2), translation=(0.1, -0.05, 0.15), pivot_pixel=(64, 64))
    assert args["both"]["rot_angle"] == 10.0 and "camera_only" not in args["both"]
    assert args["pure"] == dict(camera=dict(rot_angle=4.0, rot_axis=(0.0, 1.0, 0.0), translation=(0.0, 0.0, 0.0)), camera_only=True)
    assert scene_io.is_pure_camera({"camera": {}}) and not scene_io.is_pure_camera(dict(plain, camera={}))
    # a multi-object scene: the camera stands beside "objects"; without the key the entry gives what it gave
    objs = {"objects": [{}, {"rotation_angle": -20.0}], "object_weights": "equal"}
    _write_scene(tmp_path / "two", {"plain": objs, "cam": dict(objs, camera={"translation": [0.0, 0.0, 0.3], "pivot": [0.0, 0.0, 3.0]})},
                 multi=True)
    geo = scene_io.load_scene_geometry(str(tmp_path / "two"), 128)
    a, b = (scene_io.object_transform_args(geo["transforms"][n]) for n in ("plain", "cam"))
    assert "camera" not in a and b["camera"] == dict(rot_angle=0.0, rot_axis=(0.0, 1.0, 0.0), translation=(0.0, 0.0, 0.3),
                                                    pivot=(0.0, 0.0, 3.0))
    assert b["object_weights"] == a["object_weights"] == "equal" and len(b["transforms"]) == len(a["transforms"]) == 2
    # malformed entries raise when the scene is loaded, naming the scene and the entry
    for k, (bad, msg) in enumerate([({"camera": 3}, "must be an object"), ({"camera": {"rot_axis": [0, 0, 0]}}, "must not be zero"),
                                    ({"camera": {"fov": 1}}, "unknown keys"), ({"camera": {"rot_angle": "x"}}, "finite number"),
                                    ({"camera": {"translation": [0, 1]}}, "3 finite numbers"),
                                    ({"camera": {"pivot": [0, 0, 1], "pivot_pixel": [1, 2]}}, "both"),
                                    ({"camera": {"pivot_pixel": [1.5, 2]}}, "two integers")]):
        _write_scene(tmp_path / f"bad{k}", {"e": bad})
        with pytest.raises(ValueError, match=f"bad{k}: transform 'e'.*{msg}"):
            scene_io.load_scene_geometry(str(tmp_path / f"bad{k}"), 128)
    _write_scene(tmp_path / "badm", {"e": {"objects": [{"camera": {}}, {}]}}, multi=True)
    with pytest.raises(ValueError, match="belongs to the entry"):
        scene_io.load_scene_geometry(str(tmp_path / "badm"), 128)


def test_edit_call_parameter_lists():
    from diffusionhandles_amd import DiffusionHandles, GuidedStableDiffuser
    tail = ["donor", "removed_masks", "instances", "release_mask"]
    ps = inspect.signature(DiffusionHandles.transform_foreground_objects).parameters
    assert list(ps)[-5:] == ["camera"] + tail and ps["camera"].default is None
    ps = inspect.signature(DiffusionHandles.transform_foreground_objects_batch).parameters
    assert list(ps)[-5:] == ["cameras"] + tail and ps["cameras"].default is None
    assert "camera" not in inspect.signature(DiffusionHandles.transform_foreground).parameters
    for name in ("prepare_guidance", "guided_inference", "guided_inference_batch"):
        ps = inspect.signature(getattr(GuidedStableDiffuser, name)).parameters
        assert list(ps)[-4:] == ["row_kind", "donor", "vacated", "lock"] and ps["row_kind"].default is None, name
