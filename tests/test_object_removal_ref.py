"""CPU: the test-side reference of object removal (tests/object_removal_ref.py) against the oracle functions it is composed
from; the conditions under which the GPU comparison of tests/test_object_removal_gpu.py means something, for every fixture that
test uses; the host checks of removed masks, which all come before any device work; the "remove" key of scene directories;
the parameter lists."""
import inspect
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_object_ref as R  # noqa: E402
import object_copies_ref as O  # noqa: E402
import object_removal_ref as RR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y = torch.tensor(R.Y)
Z3 = torch.zeros(3)
GOOD = (10.0, Y, Z3)


@pytest.fixture(autouse=True)
def explicit_dot():
    from oracle import depth_ref as D
    D.DOT_ORDER = "explicit"
    yield
    D.DOT_ORDER = "blas"


def _handles(mode="pc"):
    from diffusionhandles_amd import DiffusionHandles
    dh = object.__new__(DiffusionHandles)
    dh.conf = SimpleNamespace(depth_transform_mode=mode)
    dh.diffuser = SimpleNamespace(get_depth_intrinsics=lambda device=None: torch.eye(3), unet=None)
    return dh


# ---- the cells reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("er", [0, 5])
def test_cells_without_a_vacated_pixel_are_the_oracle(er):
    from oracle import guidance_ref as G
    f = RR.fixture(128, "A")
    corr = f["corr"].numpy()
    ref = G.cells_from_correspondences(corr, 128, er)
    for vac in (None, np.zeros((128, 128), dtype=bool)):
        got = RR.cells(corr, 128, vac, er)
        for k in ref:
            assert np.array_equal(got[k], ref[k]), (er, k)
    empty = np.zeros((0, 4), dtype=np.int64)
    ref = G.cells_from_correspondences(empty, 128, er)
    got = RR.cells(empty, 128, None, er)
    for k in ref:
        assert np.array_equal(got[k], ref[k]), (er, k)


def test_vacated_cells_leave_the_original_list_only():
    f = RR.fixture(128, "A")
    vc = RR.vacated_cells(f["vacated"])
    with_v, without = f["cells0"], f["plain0"]
    gone = np.zeros((64, 64), dtype=bool)
    gone[without["background_y_orig"], without["background_x_orig"]] = True
    gone[with_v["background_y_orig"], with_v["background_x_orig"]] = False
    assert np.array_equal(gone, vc)                                   # set A: no pair starts in a vacated cell, so exactly these
    for k in ("original_x", "original_y", "transformed_x", "transformed_y", "background_x_trans", "background_y_trans"):
        assert np.array_equal(with_v[k], without[k]), k
    assert np.array_equal(with_v["masks"][0], with_v["masks"][1] & with_v["masks"][2])
    # the erosion pushes the background away from the vacated region as from an object
    far = with_v["masks"][1].astype(bool) & ~f["cells5"]["masks"][1].astype(bool)
    assert far.any() and not (f["cells5"]["masks"][1].astype(bool) & vc).any()


def test_border_blob_meets_the_erosion_border():
    vac, corr = RR.border_blob(128)
    vc = RR.vacated_cells(vac)
    assert vc[0, 0] and vc[:, -1].any() and vc.sum() >= 20
    for er in (0, 5):
        a, b = RR.cells(corr, 128, vac, er), RR.cells(corr, 128, None, er)
        assert len(a["background_x_orig"]) < len(b["background_x_orig"])
        assert np.array_equal(a["background_x_trans"], b["background_x_trans"])
        assert not (a["masks"][1].astype(bool) & vc).any()
    m5 = RR.cells(corr, 128, vac, 5)["masks"][1]
    assert not m5[:5].any() and not m5[:, :5].any()                   # border_value 0


# ---- the fixtures of the GPU tests ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [128, 256])
@pytest.mark.parametrize("which", ["A", "B"])
def test_fixture_conditions(res, which):
    f = RR.fixture(res, which)
    vc = RR.vacated_cells(f["vacated"])
    assert vc.sum() >= 20
    for er in (0, 5):
        a, b = f[f"cells{er}"], f[f"plain{er}"]
        assert not np.array_equal(a["background_x_orig"], b["background_x_orig"]) or \
            not np.array_equal(a["background_y_orig"], b["background_y_orig"]), er
    target = np.zeros((64, 64), dtype=bool)
    target[f["cells0"]["transformed_y"], f["cells0"]["transformed_x"]] = True
    both = int((vc & target).sum())
    assert both >= 10 if which == "B" else both == 0, both
    assert len(f["corr"]) >= 100
    # the moved sphere alone: the geometry reference of the edit is the copies reference on the remaining mask
    d, c, _ = O.transform_instances(f["depth"], f["bg_depth"], [f["masks"][0]], [0], f["transforms"])
    assert torch.equal(d, f["disparity"]) and torch.equal(c, f["corr"])


@pytest.mark.parametrize("res", [128, 256])
def test_background_alone_owns_every_pixel_on_the_fixtures(res):
    """Every background point projects back onto its own pixel, so no pixel is left without an owner: the in-fill has nothing
    to do on the fixtures, zmap is bg_depth and the result is its normalised disparity -- not the input's."""
    from oracle import depth_ref as D
    depth, bg, masks = R.two_spheres(res)
    disp, dbg = RR.background_alone(bg)
    assert int(dbg["unowned"].sum()) == 0
    assert np.array_equal(dbg["zmap"], bg[0, 0].numpy())
    assert torch.equal(disp, D.normalize_depth(1.0 / bg)[0])
    empty_mask_result = D.normalize_depth(1.0 / depth)[0]
    on_object = masks[1][0, 0].bool()
    # (the two maps are normalised with different bounds and cross on a thin ring; the sphere's body is tens of 255 away)
    assert float((disp - empty_mask_result)[0, 0][on_object].abs().median()) > 10.0
    lo_hi = D.normalize_depth(1.0 / depth)[1]
    bounded, _ = RR.background_alone(bg, bounds=lo_hi)
    assert torch.equal(bounded, D.normalize_depth(1.0 / bg, lo_hi)[0])


# ---- errors, all before any device work ---------------------------------------------------------------------------------------------
def test_removed_mask_errors_raise_without_a_device():
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, masks = R.two_spheres(128)
    K = torch.eye(3)
    small = torch.zeros((1, 1, 64, 64))
    empty = torch.zeros_like(masks[0])
    half = masks[1].clone()
    half[..., :, :88] = 0                                             # a part of mask 1: overlaps it, not mask 0
    with pytest.raises(ValueError, match="reproject_removal_edits: removed_masks: removed mask 0 overlaps foreground mask 1"):
        DT.reproject_removal_edits(depth, bg, masks, K, [[GOOD, GOOD]], removed_masks=[half])
    with pytest.raises(ValueError, match="removed mask 1 overlaps removed mask 0"):
        DT.reproject_removal_edits(depth, bg, [masks[0]], K, [[GOOD]], removed_masks=[masks[1], half])
    with pytest.raises(ValueError, match="removed mask 1 overlaps removed mask 0"):
        DT.reproject_removal_edits(depth, bg, [], K, [[]], removed_masks=[masks[1], half])
    with pytest.raises(ValueError, match="removed_masks: removed mask 1 is 64 x 64, the other masks are 128 x 128"):
        DT.reproject_removal_edits(depth, bg, [masks[0]], K, [[GOOD]], removed_masks=[masks[1], small])
    with pytest.raises(ValueError, match="removed_masks: expected a list of masks"):
        DT.reproject_removal_edits(depth, bg, [masks[0]], K, [[GOOD]], removed_masks=masks[1])
    # M = 0 without a non-empty removed mask: the message zero masks always had
    for removed in (None, [], [empty]):
        with pytest.raises(ValueError, match="Expected 1 to 8 foreground masks, got 0"):
            DT.reproject_removal_edits(depth, bg, [], K, [[]], removed_masks=removed)
    with pytest.raises(ValueError, match="Expected 1 to 8 foreground masks, got 0"):
        DT.reproject_instance_edits(depth, bg, [], K, [[]])
    with pytest.raises(ValueError, match="reproject_removal_edits: edit 1 has 1 transforms, but there is no foreground mask"):
        DT.reproject_removal_edits(depth, bg, [], K, [[], [GOOD]], removed_masks=[masks[1]])
    with pytest.raises(ValueError, match="instances=.* given without a foreground mask"):
        DT.reproject_removal_edits(depth, bg, [], K, [[]], instances=[0], removed_masks=[masks[1]])
    # the handles calls name themselves
    dh = _handles()
    args = (depth, "two spheres")
    tail = (bg, None, None, None)
    with pytest.raises(ValueError, match="transform_foreground_objects: removed_masks: removed mask 0 is 64 x 64"):
        dh.transform_foreground_objects(*args, [masks[0]], *tail, [GOOD], removed_masks=[small])
    with pytest.raises(ValueError, match="transform_foreground_objects_batch: removed_masks: removed mask 0 is 64 x 64"):
        dh.transform_foreground_objects_batch(*args, [masks[0]], *tail, [[GOOD]], removed_masks=[small])
    with pytest.raises(ValueError, match="removed mask 0 overlaps foreground mask 1"):
        dh.transform_foreground_objects(*args, masks, *tail, [GOOD, GOOD], removed_masks=[half])
    with pytest.raises(ValueError, match="Expected 1 to 8 foreground masks, got 0"):
        dh.transform_foreground_objects(*args, [], *tail, [], removed_masks=[])
    with pytest.raises(ValueError, match="transform_foreground_objects: edit 0 has 1 transforms, but there is no foreground mask"):
        dh.transform_foreground_objects(*args, [], *tail, [GOOD], removed_masks=[masks[1]])
    with pytest.raises(ValueError, match="object_weights=.* given without a foreground mask"):
        dh.transform_foreground_objects(*args, [], *tail, [], removed_masks=[masks[1]], object_weights="equal")
    common = dict(depth=depth, prompt="two spheres", bg_depth=bg, null_text_emb=None, init_noise=None, activations=[depth])
    with pytest.raises(ValueError, match="edit 1: removed_masks: removed mask 0 is 64 x 64"):
        dh.transform_foregrounds([dict(common, fg_mask=masks[0]),
                                  dict(common, fg_masks=[masks[0]], transforms=[GOOD], removed_masks=[small])])
    with pytest.raises(ValueError, match="edit 0 has no foreground mask .a pure removal., but gives transforms"):
        dh.transform_foregrounds([dict(common, fg_masks=[], transforms=[GOOD], removed_masks=[masks[1]])])
    with pytest.raises(ValueError, match="edit 0: fg_masks must be a non-empty list"):
        dh.transform_foregrounds([dict(common, fg_masks=[], transforms=[], removed_masks=[])])
    with pytest.raises(ValueError, match="edit 0 mixes"):
        dh.transform_foregrounds([dict(common, fg_mask=masks[0], removed_masks=[masks[1]])])
    # the guidance's keyword
    from diffusionhandles_amd.losses import process_correspondences
    with pytest.raises(ValueError, match="process_correspondences: vacated has shape .64, 64., expected one 128 x 128 image"):
        process_correspondences(torch.zeros((5, 4), dtype=torch.int64), 128, vacated=torch.zeros(64, 64))
    # without a GPU a well-formed call gets as far as the device and fails loudly there
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            DT.reproject_removal_edits(depth, bg, [masks[0]], K, [[GOOD]], removed_masks=[masks[1]])
        with pytest.raises(RuntimeError):
            DT.reproject_removal_edits(depth, bg, [], K, [[]], removed_masks=[masks[1]])


def test_mesh_mode_has_no_removal():
    depth, bg, masks = R.two_spheres(128)
    dh = _handles("mesh")
    args = (depth, "two spheres")
    tail = (bg, None, None, None)
    with pytest.raises(NotImplementedError, match="depth_transform_mode 'mesh' has no object removal"):
        dh.transform_foreground_objects(*args, [masks[0]], *tail, [GOOD], removed_masks=[masks[1]])
    with pytest.raises(NotImplementedError, match="depth_transform_mode 'mesh' has no object removal"):
        dh.transform_foreground_objects_batch(*args, [], *tail, [[]], removed_masks=[masks[1]])


def test_vacated_image_is_the_union():
    from diffusionhandles_amd import depth_transform as DT
    _, _, masks = R.two_spheres(128)
    assert DT.vacated_image(None) is None and DT.vacated_image([]) is None
    v = DT.vacated_image(masks)
    assert v.dtype == torch.uint8 and tuple(v.shape) == (128, 128)
    assert np.array_equal(v.numpy().astype(bool), RR.vacated_pixels([m[0, 0].numpy() for m in masks], 128))


# ---- parameter lists ------------------------------------------------------------------------------------------------------------------
def test_signatures():
    from diffusionhandles_amd import DiffusionHandles as DH
    from diffusionhandles_amd import GuidedStableDiffuser as GD
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd import depth_transform as DT
    from diffusionhandles_amd.losses import process_correspondences
    old = list(inspect.signature(DT.reproject_instance_edits).parameters)
    new = list(inspect.signature(DT.reproject_removal_edits).parameters)
    assert "removed_masks" not in old and new == old[:6] + ["removed_masks"] + old[6:] and old[5] == "instances"
    assert inspect.signature(DT.reproject_removal_edits).parameters["removed_masks"].default is None
    assert list(inspect.signature(process_correspondences).parameters)[-3:] == ["vacated", "object_labels", "pair_instances"]
    for name in ("prepare_guidance", "guided_inference", "guided_inference_batch", "guided_inference_lanes",
                 "guided_inference_batch_lanes", "_edit_steps", "_batch_edit_steps"):
        ps = inspect.signature(getattr(GD, name)).parameters
        assert list(ps)[-2:] == ["vacated", "lock"] and ps["vacated"].default is None, name
    for name in ("transform_foreground_objects", "transform_foreground_objects_batch"):
        ps = inspect.signature(getattr(DH, name)).parameters
        assert list(ps)[-3:] == ["removed_masks", "instances", "release_mask"] and ps["removed_masks"].default is None, name
    assert list(inspect.signature(DH.transform_foreground).parameters) == [
        "self", "depth", "prompt", "fg_mask", "bg_depth", "null_text_emb", "init_noise", "activations", "rot_angle", "rot_axis",
        "translation", "fg_weight", "bg_weight", "use_input_depth_normalization", "scale", "pivot"]
    txt = open(os.path.join(ROOT, "include", "diffhandles_hip.h")).read()
    for name, nargs in (("dh_cells_from_correspondences_vacated", 13), ("dh_reproject_background", 15),
                        ("dh_reproject_background_workspace_bytes", 2)):
        assert name + "(" in txt and len(_lib.SIGNATURES[name][1]) == nargs, name
    cells, vac = _lib.SIGNATURES["dh_cells_from_correspondences"][1], _lib.SIGNATURES["dh_cells_from_correspondences_vacated"][1]
    assert vac == cells + [_lib.c_p]
    if os.path.exists(_lib.LIB_PATH):
        assert _lib.lib().dh_missing_symbols == []


# ---- scene directories ----------------------------------------------------------------------------------------------------------------
def _write_scene(path, transforms, n_masks=2, full=False):
    from diffusionhandles_amd import scene_io as IO
    os.makedirs(path, exist_ok=True)
    depth, bg, masks = R.two_spheres(64)
    np.save(os.path.join(path, "depth.npy"), depth[0, 0].numpy())
    np.save(os.path.join(path, "bg_depth.npy"), bg[0, 0].numpy())
    if n_masks:
        for m in range(n_masks):
            IO.write_png(os.path.join(path, f"mask_{m}.png"), masks[m][0, 0].numpy())
    else:
        IO.write_png(os.path.join(path, "mask.png"), masks[0][0, 0].numpy())
    if full:
        IO.write_png(os.path.join(path, "input.png"), np.zeros((64, 64, 3), dtype=np.float32))
        with open(os.path.join(path, "prompt.txt"), "w") as f:
            f.write("two spheres\n")
    with open(os.path.join(path, "transforms.json"), "w") as f:
        json.dump(transforms, f)
    return str(path)


def test_scene_entries_with_remove(tmp_path):
    from diffusionhandles_amd import scene_io as IO
    move = {"translation": [0.0, -0.9, 0.3], "rotation_angle": 25.0}
    entries = {
        "plain": {"objects": [{}, {"rotation_angle": -30.0}]},
        "drop1": {"objects": [move, {"remove": True}], "object_weights": [2.0]},
        "drop0": {"objects": [{"remove": True}, {"scale": 1.5}], "object_weights": "equal"},
        "drop0_copy": {"objects": [{"remove": True}, {}, dict(move, mask=1)], "object_weights": [1.0, 3.0]},
        "drop_all": {"objects": [{"remove": True}, {"remove": True}]},
    }
    geo = IO.load_scene_geometry(_write_scene(tmp_path / "ok", entries), 64)
    assert len(geo["fg_masks"]) == 2
    plain = IO.object_transform_args(geo["transforms"]["plain"])
    assert set(plain) == {"transforms", "object_weights"} and len(plain["transforms"]) == 2          # what it gave before
    d1 = IO.object_transform_args(geo["transforms"]["drop1"])
    assert d1["remove"] == [1] and len(d1["transforms"]) == 1 and d1["object_weights"] == [2.0] and "instances" not in d1
    assert d1["transforms"][0][0] == 25.0
    d0 = IO.object_transform_args(geo["transforms"]["drop0"])
    assert d0["remove"] == [0] and len(d0["transforms"]) == 1 and d0["transforms"][0][3] == 1.5 and "instances" not in d0
    dc = IO.object_transform_args(geo["transforms"]["drop0_copy"])
    assert dc["remove"] == [0] and dc["instances"] == [0, 0] and len(dc["transforms"]) == 2 and dc["object_weights"] == [1.0, 3.0]
    da = IO.object_transform_args(geo["transforms"]["drop_all"])
    assert da["remove"] == [0, 1] and da["transforms"] == [] and da["object_weights"] is None
    # a single-mask scene: the entry {"remove": true} deletes the one object
    one = IO.load_scene_geometry(_write_scene(tmp_path / "one", {"gone": {"remove": True}, "turn": {"rotation_angle": 20.0}}, 0), 64)
    assert IO.transform_args(one["transforms"]["gone"]) == dict(remove=True)
    assert set(IO.transform_args(one["transforms"]["turn"])) == {"rot_angle", "rot_axis", "translation"}


BAD_SCENES = [
    ({"e": {"objects": [{}, {"remove": False}]}}, 2, "transform 'e', object 1: \"remove\" must be true"),
    ({"e": {"objects": [{}, {"remove": 1}]}}, 2, "object 1: \"remove\" must be true"),
    ({"e": {"objects": [{}, {"remove": True, "rotation_angle": 5.0}]}}, 2, "object 1: a removed object takes no other key.*rotation_angle"),
    ({"e": {"objects": [{}, {"remove": True, "mask": 1}]}}, 2, "object 1: a removed object takes no other key.*mask"),
    ({"e": {"objects": [{"mask": 1}, {"remove": True}]}}, 2, "object 0: draws mask 1, which object 1 removes"),
    ({"e": {"objects": [{}, {}, {"remove": True}]}}, 2, "object 2: \"remove\" deletes the mask of its own position"),
    ({"e": {"objects": [{"mask": 0}, {"remove": True}, {"mask": 3}]}}, 2, "mask 3 does not exist"),
    ({"e": {"objects": [{}, {"remove": True}], "object_weights": [1.0, 1.0]}}, 2, "2 object_weights for 1 remaining"),
    ({"e": {"objects": [{"remove": True}, {"remove": True}], "object_weights": "equal"}}, 2, "removes every object and gives object_weights"),
    ({"e": {"remove": True, "objects": [{}, {}]}}, 2, "\"remove\" belongs inside a member"),
    ({"e": {"remove": True, "rotation_angle": 3.0}}, 0, "exactly .\"remove\": true."),
    ({"e": {"remove": "yes"}}, 0, "exactly .\"remove\": true."),
]


@pytest.mark.parametrize("entries,n_masks,word", BAD_SCENES)
def test_malformed_remove_entries_raise_at_load_time(tmp_path, entries, n_masks, word):
    from diffusionhandles_amd import scene_io as IO
    path = _write_scene(tmp_path / "bad", entries, n_masks)
    with pytest.raises(ValueError, match=word) as err:
        IO.load_scene_geometry(path, 64)
    assert "bad" in str(err.value) and "'e'" in str(err.value)          # the scene and the entry


def test_files_without_remove_load_unchanged(tmp_path):
    """The entries of the copies and the similarity tests, read again: the dicts they gave."""
    from diffusionhandles_amd import scene_io as IO
    move = {"translation": [0.0, -0.9, 0.3], "rotation_angle": 25.0}
    entries = {"plain": {"objects": [{}, {"rotation_angle": -30.0}]},
               "copy": {"objects": [{}, {"rotation_angle": -30.0}, dict(move, mask=0)], "object_weights": [1.0, 1.0, 2.0]}}
    geo = IO.load_scene_geometry(_write_scene(tmp_path / "multi", entries), 64)
    assert json.loads(json.dumps(geo["transforms"])) == entries
    copy = IO.object_transform_args(geo["transforms"]["copy"])
    assert set(copy) == {"transforms", "object_weights", "instances"} and copy["instances"] == [0, 1, 0]
    assert IO.entry_removal(entries["copy"]["objects"], 2) is None
    with pytest.raises(ValueError, match="no object draws mask 1 .removing an object is not supported."):
        IO.load_scene_geometry(_write_scene(tmp_path / "gap", {"e": {"objects": [{"mask": 0}, {"mask": 0}]}}), 64)


def test_run_edit_refuses_removal_in_mesh_mode_before_the_identity(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import run_edit
    args = SimpleNamespace(res=64, mode="mesh", background_lock=False, max_edits=0)
    multi = _write_scene(tmp_path / "multi", {"e": {"objects": [{}, {"remove": True}]}}, 2, full=True)
    with pytest.raises(NotImplementedError, match="transform 'e' removes an object .*--mode mesh has no object removal"):
        run_edit.prepare_scene(args, multi, str(tmp_path / "out"), None)
    one = _write_scene(tmp_path / "one", {"gone": {"remove": True}}, 0, full=True)
    with pytest.raises(NotImplementedError, match="transform 'gone' removes an object"):
        run_edit.prepare_scene(args, one, str(tmp_path / "out"), None)
    args.mode = "pc"
    p = run_edit.prepare_scene(args, multi, str(tmp_path / "out"), None)
    assert p["transforms"][0]["remove"] == [1] and len(p["transforms"][0]["transforms"]) == 1
    sp = run_edit.split_removed(p["masks"], p["transforms"][0]["remove"])
    assert len(sp["fg_masks"]) == 1 and len(sp["removed_masks"]) == 1 and sp["removed_masks"][0] is p["masks"][1]
    assert run_edit.prepare_scene(args, one, str(tmp_path / "out"), None)["transforms"][0]["remove"] is True
