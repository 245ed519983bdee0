"""CPU: the test-side statement of object insertion (tests/object_insertion_ref.py) against the statements it is composed
from; the conditions under which the GPU comparison of tests/test_object_insertion_gpu.py means something, for every fixture
that file uses; every host-side error (none needs a device); the scene syntax; the parameter lists that must stay."""
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
import object_insertion_ref as I  # noqa: E402
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


def _handles(mode="pc", footprints=False):
    from diffusionhandles_amd import DiffusionHandles
    dh = object.__new__(DiffusionHandles)
    dh.conf = SimpleNamespace(depth_transform_mode=mode, depth_transform_footprints=footprints)
    dh.diffuser = SimpleNamespace(get_depth_intrinsics=lambda device=None: torch.eye(3), unet=None)
    return dh


# ---- the reference's own consistency ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [128, 256])
def test_disjoint_donor_is_the_copies_reference_on_the_composite(res):
    """A donor mask that shares no pixel with a host mask: the donor edit equals object_copies_ref.transform_instances on the
    composite depth with the masks concatenated -- integer outputs and the disparity, both edits."""
    fx = I.fixture(res, "disjoint")
    pasted, masks = I.composite(fx["depth"], fx["masks"], fx["donor_depth"], fx["donor_masks"])
    for tfs, (disp, corr, dbg) in zip(fx["edits"], fx["geo"]):
        disp_c, corr_c, dbg_c = O.transform_instances(pasted, fx["bg_depth"], masks, fx["instances"], tfs)
        assert torch.equal(corr, corr_c) and torch.equal(disp, disp_c)
        for k in ("zmap", "raw_mask", "cleaned", "vis", "tx", "ty", "corr_inst", "inpaint", "inst_start"):
            assert np.array_equal(dbg[k], dbg_c[k]), k
        assert np.array_equal(dbg["row_donor"], (dbg_c["corr_inst"] == 2).astype(np.uint8))


@pytest.mark.parametrize("pure", [False, True])
@pytest.mark.parametrize("which", ["overlap", "disjoint"])
@pytest.mark.parametrize("res", [128, 256])
def test_fixture_conditions(res, which, pure):
    """What the GPU comparison relies on: the overlap fixture's donor mask shares pixels with host sphere 0 (the composite cannot
    express it), every instance keeps at least 50 pairs in both edits, and no two instances tie in depth at a pixel."""
    fx = I.fixture(res, which, pure)
    dm = fx["donor_masks"][0][0, 0].numpy() != 0
    host = R.two_spheres(res)[2]
    shared = int((dm & (host[0][0, 0].numpy() != 0)).sum())
    assert (shared > 0) == (which == "overlap") and not (dm & (host[1][0, 0].numpy() != 0)).any()
    if which == "overlap":
        with pytest.raises(AssertionError, match="shares a pixel"):
            I.composite(fx["depth"], host, fx["donor_depth"], fx["donor_masks"])
    n_inst = len(fx["instances"])
    for disp, corr, dbg in fx["geo"]:
        counts = O.pairs_per_instance(dbg, n_inst)
        assert min(counts) >= 50, counts
        assert dbg["row_donor"].sum() == counts[-1] and torch.isfinite(disp).all()
        assert O.z_ties_between_instances(dbg, res) == 0
        # a donor row's source pixel is a pixel of the DONOR mask
        src = corr.numpy()[dbg["row_donor"] != 0]
        assert dm[src[:, 1], src[:, 0]].all()


# ---- cells ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("er", [0, 5])
@pytest.mark.parametrize("which", ["overlap", "disjoint"])
@pytest.mark.parametrize("res", [128, 256])
def test_cells(res, which, er):
    fx = I.fixture(res, which)
    corr, flags = fx["geo"][0][1].numpy(), fx["geo"][0][2]["row_donor"]
    plain = RR.cells(corr, res, None, er)
    for none in (None, np.zeros(len(corr), dtype=np.uint8)):
        got = I.cells(corr, res, none, None, er)
        for k in RR.CELL_KEYS:
            assert np.array_equal(got[k], plain[k]), k
        assert np.array_equal(got["masks"], plain["masks"])
    flagged = fx[f"cells{er}"]
    differ = int((flagged["masks"][1] != plain["masks"][1]).sum())
    print(f"res {res} {which} erosion {er}: the original mask differs in {differ} cells")
    assert differ >= 1 and np.array_equal(flagged["masks"][2], plain["masks"][2])
    assert (flagged["masks"][1] >= plain["masks"][1]).all()          # flagged rows only ever leave cells in
    for k in ("original_x", "original_y", "transformed_x", "transformed_y"):
        assert np.array_equal(flagged[k], plain[k]), k


# ---- errors, all before any device work ---------------------------------------------------------------------------------------------
def test_donor_errors_raise_without_a_device():
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, masks = R.two_spheres(128)
    ddepth, dmasks = I.donor_scene(128, "overlap")
    K = torch.eye(3)
    small = torch.zeros((1, 1, 64, 64))
    empty = torch.zeros_like(masks[0])
    half = dmasks[0].clone()
    half[..., :, :50] = 0
    three = [GOOD, GOOD, GOOD]
    call = lambda **kw: DT.reproject_donor_edits(depth, bg, masks, K, [kw.pop("tfs", three)], **kw)
    with pytest.raises(ValueError, match="reproject_donor_edits: donor: masks without a depth"):
        call(donor_masks=dmasks)
    with pytest.raises(ValueError, match="reproject_donor_edits: donor: a depth without masks"):
        call(donor_depth=ddepth)
    with pytest.raises(ValueError, match="donor: masks: the list is empty"):
        call(donor_depth=ddepth, donor_masks=[])
    with pytest.raises(ValueError, match="donor: depth has shape .*another resolution"):
        call(donor_depth=small, donor_masks=dmasks)
    with pytest.raises(ValueError, match="donor: mask 0 has shape .*another resolution"):
        call(donor_depth=ddepth, donor_masks=[small])
    with pytest.raises(ValueError, match="donor: mask 1 overlaps donor mask 0"):
        call(donor_depth=ddepth, donor_masks=[dmasks[0], half], tfs=three + [GOOD])
    with pytest.raises(ValueError, match="donor: mask 1 is empty"):
        call(donor_depth=ddepth, donor_masks=[dmasks[0], empty], tfs=three + [GOOD])
    with pytest.raises(ValueError, match="donor: 2 host masks and 7 donor masks, at most 8"):
        parts = [torch.zeros_like(empty) for _ in range(7)]
        for i, part in enumerate(parts):
            part[..., 10 * i:10 * i + 5, :20] = 1
        call(donor_depth=ddepth, donor_masks=parts)
    with pytest.raises(ValueError, match="reproject_donor_edits: instances: mask 2 has no instance"):
        call(donor_depth=ddepth, donor_masks=dmasks, instances=[0, 1, 1])
    with pytest.raises(ValueError, match="Edit 0 has 2 transforms for 3 foreground masks"):
        call(donor_depth=ddepth, donor_masks=dmasks, tfs=[GOOD, GOOD])
    with pytest.raises(NotImplementedError, match="footprints with a donor"):
        call(donor_depth=ddepth, donor_masks=dmasks, footprints=True)
    # the row flags of the guidance
    from diffusionhandles_amd.losses import process_correspondences
    with pytest.raises(ValueError, match="process_correspondences: row_donor has 3 entries for 5 correspondences"):
        process_correspondences(torch.zeros((5, 4), dtype=torch.int64), 128, row_donor=torch.zeros(3))
    # the handles calls name themselves, the donor and the member
    dh = _handles()
    acts = [torch.zeros(50, 4, 8, 8)] * 3
    args, tail = (depth, "two spheres"), (bg, None, None, acts)
    good = dict(depth=ddepth, masks=dmasks, activations=acts)
    for name, tfs in (("transform_foreground_objects", three), ("transform_foreground_objects_batch", [three])):
        fn = getattr(dh, name)
        for member in ("depth", "masks", "activations"):
            with pytest.raises(ValueError, match=f"{name}: donor: no {member}"):
                fn(*args, masks, *tail, tfs, donor={k: v for k, v in good.items() if k != member})
        with pytest.raises(ValueError, match=f"{name}: donor: expected a dict"):
            fn(*args, masks, *tail, tfs, donor=(ddepth, dmasks, acts))
        with pytest.raises(ValueError, match=f"{name}: donor: depth has shape .*another resolution"):
            fn(*args, masks, *tail, tfs, donor=dict(good, depth=small))
        with pytest.raises(ValueError, match=f"{name}: donor: mask 1 overlaps donor mask 0"):
            fn(*args, masks, *tail, tfs, donor=dict(good, masks=[dmasks[0], half]))
        with pytest.raises(ValueError, match=f"{name}: donor: mask 1 is empty"):
            fn(*args, masks, *tail, tfs, donor=dict(good, masks=[dmasks[0], empty]))
        with pytest.raises(ValueError, match=f"{name}: donor: activations of 2 layers, the host's have 3"):
            fn(*args, masks, *tail, tfs, donor=dict(good, activations=acts[:2]))
        with pytest.raises(ValueError, match=f"{name}: donor: activations of layer 0 hold 20 timesteps, the host's 50"):
            fn(*args, masks, *tail, tfs, donor=dict(good, activations=[torch.zeros(20, 4, 8, 8)] + acts[1:]))
        with pytest.raises(ValueError, match=f"{name}: instances: mask 2 has no instance"):
            fn(*args, masks, *tail, tfs, donor=good, instances=[0, 1, 1])
        with pytest.raises(ValueError, match="object_weights has 2 entries for 3 objects"):
            fn(*args, masks, *tail, tfs, donor=good, object_weights=[1.0, 1.0])
    with pytest.raises(NotImplementedError, match="depth_transform_mode 'mesh' has no object insertion"):
        _handles("mesh").transform_foreground_objects(*args, masks, *tail, three, donor=good)
    with pytest.raises(NotImplementedError, match="depth_transform_footprints: true has no object insertion"):
        _handles("pc", True).transform_foreground_objects(*args, masks, *tail, three, donor=good)
    common = dict(depth=depth, prompt="two spheres", bg_depth=bg, null_text_emb=None, init_noise=None, activations=acts)
    with pytest.raises(NotImplementedError, match="transform_foregrounds: edit 0: donor"):
        dh.transform_foregrounds([dict(common, fg_masks=masks, transforms=three, donor=good)])
    # without a GPU a well-formed call gets as far as the device and fails loudly there
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            call(donor_depth=ddepth, donor_masks=dmasks)


def test_check_donor_says_when_there_is_no_donor():
    from diffusionhandles_amd import depth_transform as DT
    ddepth, dmasks = I.donor_scene(128, "overlap")
    empty = torch.zeros_like(dmasks[0])
    assert DT.check_donor(None, None, 128, 2) is None
    assert DT.check_donor(ddepth, [empty, empty], 128, 2) is None          # all masks empty: the call without the keyword
    d, m = DT.check_donor(ddepth, dmasks, 128, 2)
    assert d is ddepth and len(m) == 1


# ---- parameter lists ------------------------------------------------------------------------------------------------------------------
def test_signatures():
    from diffusionhandles_amd import DiffusionHandles as DH
    from diffusionhandles_amd import GuidedStableDiffuser as GD
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd import depth_transform as DT
    from diffusionhandles_amd import losses
    old = list(inspect.signature(DT.reproject_removal_edits).parameters)
    new = list(inspect.signature(DT.reproject_donor_edits).parameters)
    assert "donor_depth" not in old and new == old[:7] + ["donor_depth", "donor_masks"] + old[7:] and old[6] == "removed_masks"
    for name in ("donor_depth", "donor_masks"):
        assert inspect.signature(DT.reproject_donor_edits).parameters[name].default is None
    ps = inspect.signature(losses.process_correspondences).parameters
    assert ps["row_donor"].default is None and list(ps)[-3:] == ["vacated", "object_labels", "pair_instances"]
    for name in ("prepare_guidance", "guided_inference", "guided_inference_batch", "guided_inference_lanes",
                 "guided_inference_batch_lanes", "_edit_steps", "_batch_edit_steps"):
        ps = inspect.signature(getattr(GD, name)).parameters
        assert list(ps)[-3:] == ["donor", "vacated", "lock"] and ps["donor"].default is None, name
    for name in ("transform_foreground_objects", "transform_foreground_objects_batch"):
        ps = inspect.signature(getattr(DH, name)).parameters
        assert list(ps)[-4:] == ["donor", "removed_masks", "instances", "release_mask"] and ps["donor"].default is None, name
    assert list(inspect.signature(DH.transform_foreground).parameters) == [
        "self", "depth", "prompt", "fg_mask", "bg_depth", "null_text_emb", "init_noise", "activations", "rot_angle", "rot_axis",
        "translation", "fg_weight", "bg_weight", "use_input_depth_normalization", "scale", "pivot"]
    assert callable(losses.energy_and_grad_planned_donor) and callable(losses.energy_and_grad_planned_donor_batch)
    txt = open(os.path.join(ROOT, "include", "diffhandles_hip.h")).read()
    for name, nargs in (("dh_reproject_donor_edits", 35), ("dh_reproject_donor_workspace_bytes", 7),
                        ("dh_cells_from_correspondences_donor", 14), ("dh_energy_fwd_bwd_planned_donor", 23),
                        ("dh_energy_fwd_bwd_planned_donor_batch", 9)):
        assert name + "(" in txt and len(_lib.SIGNATURES[name][1]) == nargs, name
    S = _lib.SIGNATURES
    assert S["dh_reproject_donor_edits"][1] == S["dh_reproject_instance_edits"][1] + [_lib.c_p, _lib.c_i]
    assert S["dh_cells_from_correspondences_donor"][1] == S["dh_cells_from_correspondences_vacated"][1] + [_lib.c_p]
    assert S["dh_energy_fwd_bwd_planned_donor"][1] == S["dh_energy_fwd_bwd_planned_objects"][1] + [_lib.c_p, _lib.ctypes.c_uint32]
    assert [f[0] for f in _lib.EnergyDonorItem._fields_] == ["item", "donor", "donor_objects"]
    assert "dh_energy_donor_item" in txt
    if os.path.exists(_lib.LIB_PATH):
        assert _lib.lib().dh_missing_symbols == []


# ---- scene directories ----------------------------------------------------------------------------------------------------------------
def _write_scene(path, transforms, n_donor=1, full=False, donor_dir=True):
    from diffusionhandles_amd import scene_io as IO
    os.makedirs(path, exist_ok=True)
    depth, bg, masks = R.two_spheres(64)
    np.save(os.path.join(path, "depth.npy"), depth[0, 0].numpy())
    np.save(os.path.join(path, "bg_depth.npy"), bg[0, 0].numpy())
    for m in range(2):
        IO.write_png(os.path.join(path, f"mask_{m}.png"), masks[m][0, 0].numpy())
    if donor_dir:
        os.makedirs(os.path.join(path, "donor"), exist_ok=True)
        ddepth, dmasks = I.donor_scene(64, "overlap")
        np.save(os.path.join(path, "donor", "depth.npy"), ddepth[0, 0].numpy())
        for d in range(n_donor):
            IO.write_png(os.path.join(path, "donor", f"mask_{d}.png"), dmasks[0][0, 0].numpy())
    if full:
        for sub, prompt in (("", "two spheres\n"), ("donor", "a ball\n")):
            IO.write_png(os.path.join(path, sub, "input.png"), np.zeros((64, 64, 3), dtype=np.float32))
            with open(os.path.join(path, sub, "prompt.txt"), "w") as f:
                f.write(prompt)
    with open(os.path.join(path, "transforms.json"), "w") as f:
        json.dump(transforms, f)
    return str(path)


def test_scene_entries_with_a_donor(tmp_path):
    from diffusionhandles_amd import scene_io as IO
    put = {"donor": 0, "translation": [0.4, 0.5, 0.2], "scale": 0.8}
    entries = {
        "plain": {"objects": [{}, {"rotation_angle": -30.0}]},
        "insert": {"objects": [{}, {"rotation_angle": -30.0}, put], "object_weights": "equal"},
        "twice": {"objects": [{}, {}, put, {"donor": 0}], "object_weights": [1.0, 1.0, 2.0, 2.0]},
        "swap": {"objects": [{"remove": True}, {}, put]},
        "copy": {"objects": [{}, {}, {"mask": 0, "rotation_angle": 5.0}, put]},
    }
    geo = IO.load_scene_geometry(_write_scene(tmp_path / "ok", entries), 64)
    assert len(geo["fg_masks"]) == 2 and len(geo["donor"]["masks"]) == 1 and tuple(geo["donor"]["depth"].shape) == (1, 1, 64, 64)
    assert np.array_equal(geo["donor"]["masks"][0].numpy(), I.donor_scene(64, "overlap")[1][0].numpy())
    plain = IO.object_transform_args(geo["transforms"]["plain"])
    assert set(plain) == {"transforms", "object_weights"}
    ins = IO.object_transform_args(geo["transforms"]["insert"])
    assert ins["donor"] == [0] and ins["instances"] == [0, 1, 2] and len(ins["transforms"]) == 3 and ins["object_weights"] == "equal"
    assert ins["transforms"][2][3] == 0.8 and ins["transforms"][1][0] == -30.0
    tw = IO.object_transform_args(geo["transforms"]["twice"])
    assert tw["donor"] == [0, 0] and tw["instances"] == [0, 1, 2, 2] and tw["object_weights"] == [1.0, 1.0, 2.0, 2.0]
    sw = IO.object_transform_args(geo["transforms"]["swap"])
    assert sw["remove"] == [0] and sw["instances"] == [0, 1] and sw["donor"] == [0] and len(sw["transforms"]) == 2
    cp = IO.object_transform_args(geo["transforms"]["copy"])
    assert cp["instances"] == [0, 1, 0, 2] and cp["donor"] == [0]
    full = IO.load_scene(_write_scene(tmp_path / "full", entries, full=True), 64)
    assert full["donor"]["prompt"] == "a ball" and tuple(full["donor"]["img"].shape) == (1, 3, 64, 64)


BAD_SCENES = [
    ({"e": {"objects": [{}, {}, {"donor": True}]}}, 1, True, "object 2: \"donor\" must be the index of a donor mask"),
    ({"e": {"objects": [{}, {}, {"donor": -1}]}}, 1, True, "object 2: \"donor\" must be the index"),
    ({"e": {"objects": [{}, {}, {"donor": 0, "mask": 1}]}}, 1, True, "object 2: a donor member takes no \"mask\""),
    ({"e": {"objects": [{}, {}, {"donor": 0, "remove": True}]}}, 1, True, "object 2: a donor member takes no \"remove\""),
    ({"e": {"objects": [{}, {"donor": 0}, {}]}}, 1, True, "object 2: a member of the host image stands behind a donor member"),
    ({"e": {"objects": [{}, {}, {"donor": 1}]}}, 1, True, "donor mask 1 does not exist"),
    ({"e": {"objects": [{}, {}, {"donor": 0}]}}, 2, True, "no member draws donor mask 1"),
    ({"e": {"objects": [{}, {}, {"donor": 0}]}}, 0, False, "the scene has no donor/ directory"),
    ({"e": {"objects": [{}, {}, {"donor": 0}], "object_weights": [1.0, 1.0]}}, 1, True, "2 object_weights for 3 instances"),
    ({"e": {"objects": [{}, {"donor": 0}]}}, 1, True, "lists 1 objects, the scene has 2 object masks"),
    ({"e": {"objects": [{}, {}, {"donor": 0, "scale": -1.0}]}}, 1, True, "\"scale\" must be positive"),
]


@pytest.mark.parametrize("entries,n_donor,donor_dir,word", BAD_SCENES)
def test_malformed_donor_entries_raise_at_load_time(tmp_path, entries, n_donor, donor_dir, word):
    from diffusionhandles_amd import scene_io as IO
    path = _write_scene(tmp_path / "bad", entries, n_donor, donor_dir=donor_dir)
    with pytest.raises(ValueError, match=word) as err:
        IO.load_scene_geometry(path, 64)
    assert "bad" in str(err.value) and "'e'" in str(err.value)


def test_files_without_donor_load_unchanged(tmp_path):
    from diffusionhandles_amd import scene_io as IO
    move = {"translation": [0.0, -0.9, 0.3], "rotation_angle": 25.0}
    entries = {"plain": {"objects": [{}, {"rotation_angle": -30.0}]},
               "copy": {"objects": [{}, {"rotation_angle": -30.0}, dict(move, mask=0)], "object_weights": [1.0, 1.0, 2.0]},
               "drop": {"objects": [move, {"remove": True}]}}
    with_dir = IO.load_scene_geometry(_write_scene(tmp_path / "a", entries), 64)
    without = IO.load_scene_geometry(_write_scene(tmp_path / "b", entries, donor_dir=False), 64)
    assert "donor" in with_dir and "donor" not in without and set(without) == {"transforms", "fg_mask", "depth", "bg_depth", "fg_masks"}
    assert json.loads(json.dumps(with_dir["transforms"])) == entries == json.loads(json.dumps(without["transforms"]))
    for name in entries:
        a, b = IO.object_transform_args(with_dir["transforms"][name]), IO.object_transform_args(without["transforms"][name])
        assert set(a) == set(b) and "donor" not in a
    assert IO.entry_donor(entries["copy"]["objects"], 1) is None


def test_run_edit_refuses_a_donor_before_the_identity(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import run_edit
    entries = {"e": {"objects": [{}, {}, {"donor": 0}]}}
    scene = _write_scene(tmp_path / "multi", entries, full=True)
    args = SimpleNamespace(res=64, mode="mesh", background_lock=False, max_edits=0, edit_batch=1)
    with pytest.raises(NotImplementedError, match="transform 'e' inserts a donor object .*--mode mesh has no object insertion"):
        run_edit.prepare_scene(args, scene, str(tmp_path / "out"), None)
    args.mode, args.footprint_report = "pc", dict(footprints=True, footprint_max_ratio=None)
    with pytest.raises(NotImplementedError, match="transform 'e' inserts a donor object .*--footprints"):
        run_edit.prepare_scene(args, scene, str(tmp_path / "out"), None)
    args.footprint_report = dict(footprints=False, footprint_max_ratio=None)
    p = run_edit.prepare_scene(args, scene, str(tmp_path / "out"), None)
    assert p["transforms"][0]["donor"] == [0] and p["transforms"][0]["instances"] == [0, 1, 2] and len(p["donor"]["masks"]) == 1
    assert run_edit.parse(["--scene", scene, "--identity-batch", "2"]).identity_batch == 2
