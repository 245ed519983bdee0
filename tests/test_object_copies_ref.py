"""CPU: the test-side reference of object copies (tests/object_copies_ref.py) against the references it generalises; the
tie rule; the conditions under which the GPU comparison of tests/test_object_copies_gpu.py means something, for every edit
that test uses -- at least 100 kept pairs per instance and no pixel where points of two instances have exactly the same depth
(set C excepted: it is the tie rule's own test); the host checks of the instance table, which all come before any device work;
the "mask" key of scene directories."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprints_ref as F  # noqa: E402
import multi_object_ref as R  # noqa: E402
import object_copies_ref as O  # noqa: E402
import similarity_ref as S  # noqa: E402

Y = torch.tensor(R.Y)
Z3 = torch.zeros(3)
KEYS = ("zmap", "raw_mask", "cleaned", "vis", "inpaint", "disparity", "points", "obj_start")


@pytest.fixture(autouse=True)
def explicit_dot():
    from oracle import depth_ref as D
    D.DOT_ORDER = "explicit"
    yield
    D.DOT_ORDER = "blas"


def _same(a, b, keys=KEYS):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in keys:
        assert np.array_equal(a[2][k], b[2][k]), k


# ---- the identity table ---------------------------------------------------------------------------------------------------------
def test_identity_table_is_the_multi_object_reference():
    depth, bg, masks = R.two_spheres(128)
    for tfs in (R.OCCLUDING, [(15.0, R.Y, (0.1, 0.0, -0.05)), (-20.0, (0.0, 1.0, 0.0), (-0.15, 0.05, 0.1))]):
        a = O.transform_instances(depth, bg, masks, [0, 1], tfs)
        _same(a, R.transform_objects(depth, bg, masks, tfs))
        c = a[1].numpy()
        assert np.array_equal(a[2]["corr_inst"], (masks[1][0, 0].numpy() > 0.5)[c[:, 1], c[:, 0]].astype(np.uint8))
        # tx / ty of EVERY point here, of the visible ones there
        assert np.array_equal(a[2]["tx"][a[2]["vis"]], R.transform_objects(depth, bg, masks, tfs)[2]["tx"])


def test_identity_table_is_the_similarity_and_the_footprint_reference():
    depth, bg, masks = R.two_spheres(128)
    for tfs in S.edits_for(128, depth)[1:]:
        _same(O.transform_instances(depth, bg, masks, [0, 1], tfs), S.transform_objects(depth, bg, masks, tfs))
    for tfs, ratio in ((F.SCALE3, None), (F.EDITS[1], 1.05)):
        a = O.transform_instances(depth, bg, masks, [0, 1], tfs, footprints=True, max_ratio=ratio)
        b = F.transform_objects(depth, bg, masks, tfs, footprints=True, max_ratio=ratio)
        _same(a, b, KEYS + ("owner", "tx", "ty"))
    # a permuted table is the permuted call
    tfs = list(R.OCCLUDING)
    a = O.transform_instances(depth, bg, masks, [1, 0], tfs[::-1])
    b = R.transform_objects(depth, bg, masks[::-1], tfs[::-1])
    _same(a, b)


def test_empty_masks_are_dropped_with_their_instances_and_the_indices_stay_the_callers():
    depth, bg, masks = R.two_spheres(128)
    empty = torch.zeros_like(masks[0])
    inst, edits = O.SET_A
    a = O.transform_instances(depth, bg, [masks[0], empty, masks[1]], [0, 1, 0, 1, 2], [edits[0][0], edits[0][0], edits[0][1], edits[0][1], edits[0][2]])
    b = O.transform_instances(depth, bg, masks, inst, edits[0])
    _same(a, b)
    assert a[2]["inst_kept"] == [0, 2, 4]
    lut = np.asarray([0, 255, 1, 255, 2])
    assert np.array_equal(lut[a[2]["corr_inst"]], b[2]["corr_inst"])


# ---- the tie rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,pairs,ties", [(128, 1095, 1252), (256, 4546, 5013)])
def test_two_instances_with_one_transform_give_the_one_instance_result(res, pairs, ties):
    """Set C: equal depths go to the earlier instance, so the later one gets no pair and hides nothing."""
    inst, edits = O.SET_C
    depth, bg, masks = R.two_spheres(res)
    two = O.transform_instances(depth, bg, masks[:1], inst, edits[0])
    one = O.transform_instances(depth, bg, masks[:1], [0], edits[0][:1])
    assert torch.equal(two[0], one[0]) and torch.equal(two[1], one[1])
    for k in ("zmap", "raw_mask", "cleaned", "inpaint"):
        assert np.array_equal(two[2][k], one[2][k]), k
    n = len(one[2]["vis"])
    assert np.array_equal(two[2]["vis"][:n], one[2]["vis"]) and not two[2]["vis"][n:].any()
    assert O.pairs_per_instance(two[2], 2) == [pairs, 0]
    assert O.z_ties_between_instances(two[2], res) == ties          # every occupied pixel of the object is a tie


# ---- the GPU comparison means something -------------------------------------------------------------------------------------------
TABLE = {("A", 128): [[1207, 713, 646]], ("A", 256): [[5013, 3162, 2855]],
         ("B", 128): [[792, 1085, 766, 428]], ("B", 256): [[3380, 4412, 3100, 1917]]}


@pytest.mark.parametrize("res", [128, 256])
@pytest.mark.parametrize("name", ["A", "B"])
def test_every_edit_of_the_gpu_test_has_pairs_for_every_instance_and_no_ties(name, res):
    inst, edits = O.SET_A if name == "A" else O.SET_B
    depth, bg, masks = R.two_spheres(res)
    for e, tfs in enumerate(edits):
        _, corr, dbg = O.transform_instances(depth, bg, masks, inst, tfs)
        per = O.pairs_per_instance(dbg, len(inst))
        print(f"set {name}, res {res}, edit {e}: kept pairs per instance {per}, {int(dbg['inpaint'].sum())} in-fill pixels")
        assert min(per) >= 100 and sum(per) == len(corr)
        assert O.z_ties_between_instances(dbg, res) == 0
        if e == 0:
            assert per == TABLE[name, res][0]
        # a source pixel appears once per visible, kept instance: mask 0 is drawn twice
        c = corr.numpy()
        src = c[:, 1] * res + c[:, 0]
        assert len(np.unique(src)) < len(src) and len(np.unique(np.stack([src, dbg["corr_inst"]]), axis=1).T) == len(src)
    if (name, res) == ("A", 128):
        assert int(dbg["inpaint"].sum()) == 946 and int(O.transform_instances(depth, bg, masks, inst, edits[0])[2]["inpaint"].sum()) == 759


@pytest.mark.parametrize("ratio", [None, 1.02])
def test_the_footprint_edit_of_the_gpu_test(ratio):
    """Set A with instance 1 at scale 2, at 128: every instance keeps at least 100 rows, no ties between the points of two
    instances, the enlarged copy has more rows than its mask has points, and the ratio guard changes the result."""
    inst, edits = O.SET_A_FP
    depth, bg, masks = R.two_spheres(128)
    _, corr, dbg = O.transform_instances(depth, bg, masks, inst, edits[0], footprints=True, max_ratio=ratio)
    per = O.pairs_per_instance(dbg, 3)
    print(f"footprints, ratio {ratio}: rows per instance {per}")
    assert min(per) >= 100 and O.z_ties_between_instances(dbg, 128) == 0
    assert per[1] > int((masks[0] > 0.5).sum())
    assert per == ([1206, 3034, 935] if ratio is None else [1204, 2546, 817])
    # a triangle joins points of ONE instance: the pixels between instance 0 and its moved copy stay background
    owner = dbg["owner"]
    fg = owner[owner >= 128 * 128] - 128 * 128
    assert set(np.searchsorted(dbg["inst_start"], fg, side="right") - 1) == {0, 1, 2}


# ---- host checks, before any device work ------------------------------------------------------------------------------------------
def _handles(mode="pc"):
    from diffusionhandles_amd import DiffusionHandles
    dh = object.__new__(DiffusionHandles)
    dh.conf = SimpleNamespace(depth_transform_mode=mode)
    dh.diffuser = SimpleNamespace(get_depth_intrinsics=lambda device=None: torch.eye(3), unet=None)
    return dh


BAD_TABLES = [([0] * 5 + [1] * 4, "1 to 8 instances"), ([0, 2, 1], "instance 1 names mask 2"), ([0, -1, 1], "instance 1 names mask -1"),
              ([0, 1.0, 1], "instance 1"), ([0, True, 1], "instance 1"), ([0, 0, 0], "mask 1 has no instance"), ([1, 1], "mask 0 has no instance"),
              ([], "1 to 8 instances"), (3, "list of mask indices")]


@pytest.mark.parametrize("inst,word", BAD_TABLES)
def test_bad_instance_tables_raise_before_any_device_work(inst, word):
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, masks = R.two_spheres(128)
    good = (10.0, Y, Z3)
    n = len(inst) if isinstance(inst, list) else 1
    with pytest.raises(ValueError, match=word):
        DT.check_instances(inst, 2)
    with pytest.raises(ValueError, match="instances.*" + word):
        DT.reproject_instance_edits(depth, bg, masks, torch.eye(3), [[good] * n], instances=inst)
    dh = _handles()
    with pytest.raises(ValueError, match="transform_foreground_objects: instances.*" + word):
        dh.transform_foreground_objects(depth, "two spheres", masks, bg, None, None, None, [good] * n, instances=inst)
    with pytest.raises(ValueError, match="transform_foreground_objects_batch: instances.*" + word):
        dh.transform_foreground_objects_batch(depth, "two spheres", masks, bg, None, None, None, [[good] * n], instances=inst)
    common = dict(depth=depth, prompt="two spheres", bg_depth=bg, null_text_emb=None, init_noise=None, activations=[depth])
    with pytest.raises(ValueError, match="edit 1: instances.*" + word):
        dh.transform_foregrounds([dict(common, fg_mask=masks[0]), dict(common, fg_masks=masks, transforms=[good] * n, instances=inst)])


def test_transform_lists_and_weights_follow_the_instances():
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, masks = R.two_spheres(128)
    good = (10.0, Y, Z3)
    inst = [0, 0, 1]
    with pytest.raises(ValueError, match="Edit 1 has 2 transforms for 3 instances"):
        DT.reproject_instance_edits(depth, bg, masks, torch.eye(3), [[good] * 3, [good] * 2], instances=inst)
    with pytest.raises(ValueError, match="edit 0, instance 2.*scale"):
        DT.reproject_instance_edits(depth, bg, masks, torch.eye(3), [[good, good, (10.0, Y, Z3, -1.0, None)]], instances=inst)
    # without a table the message is what it was
    with pytest.raises(ValueError, match="Edit 0 has 3 transforms for 2 foreground masks"):
        DT.reproject_object_edits(depth, bg, masks, torch.eye(3), [[good] * 3])
    dh = _handles()
    args = (depth, "two spheres", masks, bg, None, None, None)
    with pytest.raises(ValueError, match="Edit 0 has 2 transforms for 3 instances"):
        dh.transform_foreground_objects(*args, [good] * 2, instances=inst)
    with pytest.raises(ValueError, match="instances.*2 entries for 3 objects.*per instance"):
        dh.transform_foreground_objects(*args, [good] * 3, instances=inst, object_weights=[1.0, 1.0])
    with pytest.raises(ValueError, match="instances.*2 entries for 3"):
        dh.transform_foreground_objects_batch(*args, [[good] * 3], instances=inst, object_weights=[1.0, 1.0])
    with pytest.raises(ValueError, match="3 entries for 2 objects"):
        dh.transform_foreground_objects(*args, [good] * 2, object_weights=[1.0, 1.0, 1.0])          # (no table: per mask, as before)
    common = dict(depth=depth, prompt="two spheres", bg_depth=bg, null_text_emb=None, init_noise=None, activations=[depth])
    with pytest.raises(ValueError, match="edit 0 has 2 transforms for 3 instances"):
        dh.transform_foregrounds([dict(common, fg_masks=masks, transforms=[good] * 2, instances=inst)])
    with pytest.raises(ValueError, match="edit 0.*2 entries for 3"):
        dh.transform_foregrounds([dict(common, fg_masks=masks, transforms=[good] * 3, instances=inst, object_weights=[1.0, 2.0])])
    with pytest.raises(ValueError, match="edit 0 mixes"):
        dh.transform_foregrounds([dict(common, fg_mask=masks[0], instances=[0])])
    # the guidance: one weight per instance, the instances in place of the label image
    from diffusionhandles_amd.losses import process_correspondences
    corr = torch.zeros((5, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match="mutually exclusive"):
        process_correspondences(corr, 128, pair_instances=torch.zeros(5, dtype=torch.uint8), object_labels=torch.zeros(128, 128, dtype=torch.uint8))
    with pytest.raises(ValueError, match="pair_instances has 4 entries for 5"):
        process_correspondences(corr, 128, pair_instances=torch.zeros(4, dtype=torch.uint8))
    # without a GPU a well-formed call gets as far as the device and fails loudly there
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            DT.reproject_instance_edits(depth, bg, masks, torch.eye(3), [[good] * 3], instances=inst)


def test_mesh_mode_has_no_copies():
    depth, bg, masks = R.two_spheres(128)
    good = (10.0, Y, Z3)
    dh = _handles("mesh")
    with pytest.raises(NotImplementedError, match="depth_transform_mode 'mesh' has no copies"):
        dh.transform_foreground_objects(depth, "two spheres", masks, bg, None, None, None, [good] * 3, instances=[0, 0, 1])
    with pytest.raises(NotImplementedError, match="depth_transform_mode 'mesh' has no copies"):
        dh.transform_foreground_objects_batch(depth, "two spheres", masks, bg, None, None, None, [[good] * 3], instances=[0, 0, 1])
    with pytest.raises(NotImplementedError, match="multi-object"):          # (without a table: the message it had)
        dh.transform_foreground_objects(depth, "two spheres", masks, bg, None, None, None, [good] * 2)


def test_signatures_keep_their_prefix():
    import inspect
    from diffusionhandles_amd import DiffusionHandles
    from diffusionhandles_amd import depth_transform as DT
    from diffusionhandles_amd.losses import process_correspondences
    old = list(inspect.signature(DT.reproject_object_edits).parameters)
    new = list(inspect.signature(DT.reproject_instance_edits).parameters)
    assert "instances" not in old and new == old[:5] + ["instances"] + old[5:] + ["return_instances"]
    assert list(inspect.signature(process_correspondences).parameters)[-2:] == ["object_labels", "pair_instances"]
    assert list(inspect.signature(DiffusionHandles.transform_foreground_objects).parameters)[-2:] == ["instances", "release_mask"]
    assert list(inspect.signature(DiffusionHandles.transform_foreground_objects_batch).parameters)[-2:] == ["instances", "release_mask"]
    assert "instances" not in inspect.signature(DiffusionHandles.transform_foreground).parameters


# ---- scene directories ------------------------------------------------------------------------------------------------------------
def _write_scene(path, transforms, n_masks=2):
    from diffusionhandles_amd import scene_io as IO
    os.makedirs(path, exist_ok=True)
    depth, bg, masks = R.two_spheres(64)
    np.save(os.path.join(path, "depth.npy"), depth[0, 0].numpy())
    np.save(os.path.join(path, "bg_depth.npy"), bg[0, 0].numpy())
    for m in range(n_masks):
        IO.write_png(os.path.join(path, f"mask_{m}.png"), masks[m][0, 0].numpy())
    with open(os.path.join(path, "transforms.json"), "w") as f:
        json.dump(transforms, f)
    return str(path)


def test_scene_entries_with_a_mask_key(tmp_path):
    from diffusionhandles_amd import scene_io as IO
    move = {"translation": [0.0, -0.9, 0.3], "rotation_angle": 25.0}
    entries = {
        "plain": {"objects": [{}, {"rotation_angle": -30.0}]},
        "copy": {"objects": [{}, {"rotation_angle": -30.0}, dict(move, mask=0)], "object_weights": [1.0, 1.0, 2.0]},
        "named": {"objects": [{"mask": 1}, {"mask": 0, "scale": 2.0}, dict(move, mask=0)], "object_weights": "equal"},
    }
    geo = IO.load_scene_geometry(_write_scene(tmp_path / "ok", entries), 64)
    assert len(geo["fg_masks"]) == 2
    plain = IO.object_transform_args(geo["transforms"]["plain"])
    assert set(plain) == {"transforms", "object_weights"} and len(plain["transforms"]) == 2          # what it gave before
    copy = IO.object_transform_args(geo["transforms"]["copy"])
    assert copy["instances"] == [0, 1, 0] and len(copy["transforms"]) == 3 and copy["object_weights"] == [1.0, 1.0, 2.0]
    assert copy["transforms"][2][0] == 25.0 and copy["transforms"][2][2].tolist() == pytest.approx([0.0, -0.9, 0.3])
    named = IO.object_transform_args(geo["transforms"]["named"])
    assert named["instances"] == [1, 0, 0] and named["object_weights"] == "equal" and named["transforms"][1][3] == 2.0
    assert IO.entry_instances(entries["plain"]["objects"], 2) is None
    bad = [({"objects": [{}, {}, {"mask": 2}]}, "object 2: mask 2 does not exist"),
           ({"objects": [{}, {}, {"mask": -1}]}, "object 2.*integer >= 0"),
           ({"objects": [{}, {}, {"mask": 0.0}]}, "object 2.*integer >= 0"),
           ({"objects": [{}, {}, {"mask": True}]}, "object 2.*integer >= 0"),
           ({"objects": [{}, {}, {"mask": "0"}]}, "object 2.*integer >= 0"),
           ({"objects": [{"mask": 1}, {}]}, "no object draws mask 0"),
           ({"objects": [{}, {}, {}]}, "lists 3 objects"),          # longer lists need the key
           ({"objects": [{}] * 2 + [{"mask": 0}] * 7}, "9 instances"),
           ({"objects": [{}, {}, {"mask": 0}], "object_weights": [1.0, 1.0]}, "2 object_weights for 3 instances"),
           ({"objects": [{}, {}, {"mask": 0, "scale": -1.0}]}, "object 2.*scale")]
    for i, (entry, word) in enumerate(bad):
        with pytest.raises(ValueError, match="bad%d.*'e'.*%s" % (i, word)):
            IO.load_scene_geometry(_write_scene(tmp_path / f"bad{i}", {"e": entry}), 64)


def test_run_edit_refuses_mesh_on_a_scene_with_copies_before_the_identity(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import run_edit
    from diffusionhandles_amd import scene_io as IO
    scene = _write_scene(tmp_path / "copies", {"copy": {"objects": [{}, {}, {"mask": 0, "translation": [0.0, -0.9, 0.3]}]}})
    with open(os.path.join(scene, "prompt.txt"), "w") as f:
        f.write("two spheres on a plane\n")
    IO.write_png(os.path.join(scene, "input.png"), np.zeros((64, 64, 3), dtype=np.float32))
    args = SimpleNamespace(res=64, mode="mesh", max_edits=0, background_lock=False)
    with pytest.raises(NotImplementedError, match="'copy' places copies of an object.*--mode mesh"):
        run_edit.prepare_scene(args, scene, str(tmp_path / "out"), None)
    args.mode = "pc"
    p = run_edit.prepare_scene(args, scene, str(tmp_path / "out"), None)
    assert p["transforms"][0]["instances"] == [0, 1, 0] and len(p["transforms"][0]["transforms"]) == 3
