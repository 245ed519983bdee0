"""CPU: the background lock's host side -- the keep-map rules on hand-worked grids (tests/background_lock_ref.py, which the
GPU tests hold dh_keep_map to), the conf keys and argument checks (ValueError naming the call, before any device work), the
signatures, background_lock.composite, and tools/run_edit.py's arguments and release.png at the prepare_scene level."""
import argparse
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import background_lock_ref as B  # noqa: E402
import multi_object_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- hand-worked maps -------------------------------------------------------------------------------------------------------
def test_one_cell_in_the_middle_gives_the_rings():
    """9 x 9 cells of 2 x 2 pixels, one mask pixel in cell (4, 4), dilate 1, feather 2: rings 0, 0, 1/3, 2/3, 1."""
    mask = np.zeros((18, 18), dtype=np.uint8)
    mask[9, 8] = 255
    keep = B.keep_map(None, mask, None, 18, 9, 1, 2)
    assert keep.dtype == np.float32 and keep.shape == (9, 9)
    ring = [F(0), F(0), F(1) / F(3), F(2) / F(3), F(1)]
    for y in range(9):
        for x in range(9):
            assert keep[y, x] == ring[max(abs(y - 4), abs(x - 4))], (y, x)


def test_region_in_a_corner_clips_the_window():
    corr = np.array([[0, 0, 1, 1]])                        # source and target in cell (0, 0) of a 6 x 6 grid of 4-pixel cells
    keep = B.keep_map(corr, None, None, 24, 6, 0, 1)
    want = np.ones((6, 6), dtype=np.float32)
    want[0, 0] = 0.0
    want[0, 1] = want[1, 0] = want[1, 1] = 0.5
    assert np.array_equal(keep, want)


def test_release_image_alone_and_with_a_mask():
    rel = np.zeros((16, 16), dtype=np.uint8)
    rel[15, 15] = 1                                        # cell (3, 3) of 4 x 4
    keep = B.keep_map(None, None, rel, 16, 4, 0, 0)
    want = np.ones((4, 4), dtype=np.float32)
    want[3, 3] = 0.0
    assert np.array_equal(keep, want)
    mask = np.zeros((16, 16), dtype=np.uint8)
    mask[0, 0] = 1
    want[0, 0] = 0.0
    assert np.array_equal(B.keep_map(None, mask, rel, 16, 4, 0, 0), want)
    assert np.array_equal(B.keep_map(np.zeros((0, 4), dtype=np.int64), None, np.ones((16, 16)), 16, 4, 2, 2), np.zeros((4, 4), dtype=np.float32))


def test_targets_outside_the_image_mark_nothing():
    corr = np.array([[5, 5, -1, 5], [5, 5, 5, 16], [5, 5, 16, -3], [5, 5, 12, 0]])
    region = B.region_cells(corr, None, None, 16, 4)
    want = np.zeros((4, 4), dtype=bool)
    want[1, 1] = True                                      # the sources
    want[0, 3] = True                                      # the one target inside
    assert np.array_equal(region, want)


def test_no_region_is_all_ones_and_a_reach_beyond_the_grid_is_clipped():
    assert np.array_equal(B.keep_map(None, None, None, 16, 4, 3, 3), np.ones((4, 4), dtype=np.float32))
    assert np.array_equal(B.keep_map(np.zeros((0, 4), dtype=np.int64), np.zeros((16, 16)), None, 16, 4, 0, 0), np.ones((4, 4), dtype=np.float32))
    mask = np.zeros((16, 16), dtype=np.uint8)
    mask[0, 0] = 1
    keep = B.keep_map(None, mask, None, 16, 4, 1, 30)      # dilate + feather = 31 on a 4 x 4 grid
    for y in range(4):
        for x in range(4):
            d = max(y, x)
            assert keep[y, x] == (F(0) if d <= 1 else F(d - 1) / F(31)), (y, x)


def test_blend_statement():
    o = np.array([1.0, 2.0, np.nan, 4.0], dtype=np.float32)
    r = np.array([10.0, 20.0, 30.0, 40.0], dtype=np.float32)
    out = B.blend(o, r, np.array([0.0, 1.0, 1.0, 0.25], dtype=np.float32))
    assert out.tolist() == [1.0, 20.0, 30.0, 13.0]


# ---- conf keys and argument checks ------------------------------------------------------------------------------------------
def _handles(**keys):
    from diffusionhandles_amd import DiffusionHandles
    from diffusionhandles_amd import conf as C
    conf = C.load_default()
    for k, v in keys.items():
        conf[k] = v
    return DiffusionHandles(conf)          # on the CPU: any device work would raise RuntimeError, not ValueError


def _calls(dh, acts, release=None):
    """Every edit call of the facade on host tensors, as (name, thunk)."""
    depth, bg, masks = R.two_spheres(64)
    tf = (10.0, torch.tensor([0.0, 1.0, 0.0]), torch.zeros(3))
    common = (depth, "p", masks[0], bg, None, None, acts)
    rel = {} if release is None else dict(release_mask=release)
    edit = dict(depth=depth, prompt="p", fg_mask=masks[0], bg_depth=bg, null_text_emb=None, init_noise=None, activations=acts,
                rot_angle=10.0, **rel)
    calls = [("transform_foreground_batch", lambda: dh.transform_foreground_batch(*common, [tf], **rel)),
             ("transform_foreground_objects", lambda: dh.transform_foreground_objects(depth, "p", masks, bg, None, None, acts, [tf, tf], **rel)),
             ("transform_foreground_objects_batch",
              lambda: dh.transform_foreground_objects_batch(depth, "p", masks, bg, None, None, acts, [[tf, tf]], **rel)),
             ("transform_foregrounds: edit 0", lambda: dh.transform_foregrounds([edit]))]
    if release is None:
        calls.append(("transform_foreground", lambda: dh.transform_foreground(*common, rot_angle=10.0)))
    return calls


@pytest.mark.parametrize("keys,word", [(dict(background_lock="yes"), "background_lock"), (dict(background_lock=1), "background_lock"),
                                       (dict(background_lock=True, background_lock_dilate=-1), "dilate"),
                                       (dict(background_lock=True, background_lock_dilate=1.5), "dilate"),
                                       (dict(background_lock=True, background_lock_feather=True), "feather"),
                                       (dict(background_lock=True, background_lock_feather="2"), "feather"),
                                       (dict(background_lock=True, background_lock_dilate=16, background_lock_feather=16), "dilate \\+ feather"),
                                       (dict(background_lock_dilate=1), "without background_lock"),
                                       (dict(background_lock=False, background_lock_feather=3), "without background_lock")])
def test_malformed_conf_values_raise_naming_the_call(keys, word):
    from diffusionhandles_amd.background_lock import Activations
    acts = Activations([torch.zeros(1)] * 3, trajectory=torch.zeros(50, 4, 8, 8))
    for name, call in _calls(_handles(**keys), acts):
        with pytest.raises(ValueError, match=name + ".*" + word):
            call()


def test_conf_defaults_and_bounds():
    from diffusionhandles_amd import background_lock as BL
    assert BL.lock_conf({}, "x") is None and BL.lock_conf(dict(background_lock=False), "x") is None
    assert BL.lock_conf(dict(background_lock=True), "x") == (2, 2) == (BL.DEFAULT_DILATE, BL.DEFAULT_FEATHER)
    assert BL.lock_conf(dict(background_lock=True, background_lock_dilate=0, background_lock_feather=31), "x") == (0, 31)
    assert BL.lock_conf(dict(background_lock=True, background_lock_dilate=31, background_lock_feather=0), "x") == (31, 0)
    with pytest.raises(ValueError):
        BL.check_reach(0, 32, "x")


def test_missing_trajectory_raises_naming_the_call_and_what_to_recompute():
    dh = _handles(background_lock=True)
    for name, call in _calls(dh, [torch.zeros(1)] * 3):          # a plain list, as an old cache gives
        with pytest.raises(ValueError, match=name + ".*trajectory.*recompute the identity"):
            call()


@pytest.mark.parametrize("shape", [(32, 32), (64, 32), (2, 64, 64), (64,)])
def test_bad_release_mask_shape_raises_naming_the_call(shape):
    from diffusionhandles_amd.background_lock import Activations
    acts = Activations([torch.zeros(1)] * 3, trajectory=torch.zeros(50, 4, 8, 8))
    for name, call in _calls(_handles(background_lock=True), acts, release=torch.zeros(shape)):
        with pytest.raises(ValueError, match=name + ".*release_mask"):
            call()


def test_release_mask_without_the_lock_raises():
    for name, call in _calls(_handles(), [torch.zeros(1)] * 3, release=torch.zeros(64, 64)):
        with pytest.raises(ValueError, match=name + ".*release_mask needs conf background_lock"):
            call()


def test_prepare_locks_checks_shapes_and_shares_the_copy():
    from diffusionhandles_amd import background_lock as BL
    cpu = torch.device("cpu")
    traj = torch.arange(3 * 4 * 2 * 2, dtype=torch.float32).reshape(3, 4, 2, 2)
    keep = torch.ones(2, 2)
    assert BL.prepare_locks(None, 3, cpu, 2, 3, "x") == [None, None, None]
    a, b, c = BL.prepare_locks([(keep, traj), None, (keep * 0, traj)], 3, cpu, 2, 3, "x")
    assert b is None and a.ref is c.ref and a.ref.shape == (3, 2, 2, 4) and a.ref.is_contiguous()
    assert torch.equal(a.ref.permute(0, 3, 1, 2), traj) and torch.equal(c.keep, keep * 0)
    view = a.ref.permute(0, 3, 1, 2)                        # the view the initial inference returns: used in place
    assert BL.prepare_locks((keep, view), 1, cpu, 2, 3, "x")[0].ref.data_ptr() == a.ref.data_ptr()
    assert BL.prepare_locks(a, 2, cpu, 2, 3, "x") == [a, a]
    for bad in ([(keep, traj)] * 2, (torch.ones(3, 3), traj), (keep, traj[:2]), (keep, traj[..., :1]), (keep,)):
        with pytest.raises(ValueError, match="x"):
            BL.prepare_locks(bad, 3 if isinstance(bad, list) else 1, cpu, 2, 3, "x")


# ---- signatures -------------------------------------------------------------------------------------------------------------
def test_signatures():
    from diffusionhandles_amd import DiffusionHandles as DH
    from diffusionhandles_amd import GuidedStableDiffuser as GD
    assert list(inspect.signature(DH.transform_foreground).parameters) == [
        "self", "depth", "prompt", "fg_mask", "bg_depth", "null_text_emb", "init_noise", "activations", "rot_angle", "rot_axis",
        "translation", "fg_weight", "bg_weight", "use_input_depth_normalization", "scale", "pivot"]
    for name in ("transform_foreground_batch", "transform_foreground_objects", "transform_foreground_objects_batch"):
        ps = inspect.signature(getattr(DH, name)).parameters
        assert list(ps)[-1] == "release_mask" and ps["release_mask"].default is None, name
    for name in ("prepare_guidance", "guided_inference", "guided_inference_batch", "guided_inference_lanes",
                 "guided_inference_batch_lanes", "_edit_steps", "_batch_edit_steps"):
        ps = inspect.signature(getattr(GD, name)).parameters
        assert list(ps)[-1] == "lock" and ps["lock"].default is None, name
    ps = inspect.signature(GD.ddim_step).parameters
    assert ps["out"].default is None and list(ps)[:5] == ["self", "x", "eps_u", "eps_c", "t"]
    for name in ("generate_input_image", "generate_input_images"):
        assert "trajectory" not in inspect.signature(getattr(DH, name)).parameters


def test_abi_declares_the_two_entries():
    from diffusionhandles_amd import _lib
    txt = open(os.path.join(ROOT, "include", "diffhandles_hip.h")).read()
    for name, nargs in (("dh_keep_map", 12), ("dh_ddim_cfg_step_locked", 16)):
        assert name + "(" in txt and len(_lib.SIGNATURES[name][1]) == nargs
    assert [f[0] for f in _lib.LockItem._fields_] == ["keep", "ref"]


# ---- composite --------------------------------------------------------------------------------------------------------------
def test_composite_on_a_hand_worked_map():
    """keep [[0, 1], [1, 0]] up-sampled bilinearly (align_corners=False) to 4 x 4: pixel centres at 0.25 and 0.75 of a cell, so a
    row of weights is 0, 0.25, 0.75, 1 between the two cells (clamped at the border)."""
    from diffusionhandles_amd.background_lock import composite
    keep = torch.tensor([[0.0, 1.0], [1.0, 0.0]])
    w = np.array([0.0, 0.25, 0.75, 1.0], dtype=np.float32)
    up = np.empty((4, 4), dtype=np.float32)
    for y in range(4):
        for x in range(4):
            top = (1 - w[x]) * 0.0 + w[x] * 1.0
            bot = (1 - w[x]) * 1.0 + w[x] * 0.0
            up[y, x] = (1 - w[y]) * top + w[y] * bot
    edited = torch.full((1, 3, 4, 4), 2.0)
    original = torch.arange(48, dtype=torch.float32).reshape(1, 3, 4, 4)
    got = composite(edited, original, keep)
    want = B.composite(edited.numpy(), original.numpy(), up)
    assert got.shape == (1, 3, 4, 4) and np.allclose(got.numpy(), want, rtol=0, atol=1e-5)
    assert torch.equal(composite(edited, original, torch.zeros(2, 2)), edited)
    assert torch.equal(composite(edited, original, torch.ones(2, 2)), original)
    with pytest.raises(ValueError, match="composite"):
        composite(edited, original[:, :2], keep)
    with pytest.raises(ValueError, match="composite"):
        composite(edited, original, torch.ones(1, 2, 2))


# ---- tools/run_edit.py ------------------------------------------------------------------------------------------------------
def _run_edit():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import run_edit
    return run_edit


def test_run_edit_arguments():
    run_edit = _run_edit()
    for extra in ([], ["--test-set", "t.json", "--edit-batch", "4"]):
        args = run_edit.parse(["--scene", "x"] + extra)
        conf = run_edit.load_config(None)
        assert run_edit.apply_lock_args(args, conf) == {} and args.background_lock is False
        assert "background_lock" not in conf
        args = run_edit.parse(["--scene", "x", "--background-lock"] + extra)
        conf = run_edit.load_config(None)
        assert run_edit.apply_lock_args(args, conf) == dict(background_lock=True, background_lock_dilate=2, background_lock_feather=2)
        assert args.background_lock is True and conf["background_lock"] is True
        args = run_edit.parse(["--scene", "x", "--background-lock", "--lock-dilate", "0", "--lock-feather", "5"] + extra)
        conf = run_edit.load_config(None)
        assert run_edit.apply_lock_args(args, conf) == dict(background_lock=True, background_lock_dilate=0, background_lock_feather=5)
        assert conf["background_lock_dilate"] == 0 and conf["background_lock_feather"] == 5
    with pytest.raises(ValueError, match="--background-lock.*without background_lock"):
        run_edit.apply_lock_args(run_edit.parse(["--scene", "x", "--lock-dilate", "1"]), run_edit.load_config(None))
    with pytest.raises(ValueError, match="--background-lock.*dilate \\+ feather"):
        run_edit.apply_lock_args(run_edit.parse(["--scene", "x", "--background-lock", "--lock-dilate", "30", "--lock-feather", "2"]),
                                 run_edit.load_config(None))
    with pytest.raises(ValueError, match="feather"):
        run_edit.apply_lock_args(run_edit.parse(["--scene", "x", "--background-lock", "--lock-feather", "-1"]), run_edit.load_config(None))


def _write_scene(path):
    from diffusionhandles_amd import scene_io as IO
    os.makedirs(path, exist_ok=True)
    depth, bg, masks = R.two_spheres(64)
    np.save(os.path.join(path, "depth.npy"), depth[0, 0].numpy())
    np.save(os.path.join(path, "bg_depth.npy"), bg[0, 0].numpy())
    IO.write_png(os.path.join(path, "mask.png"), masks[0][0, 0].numpy())
    IO.write_png(os.path.join(path, "input.png"), np.zeros((64, 64, 3), dtype=np.uint8))
    with open(os.path.join(path, "transforms.json"), "w") as f:
        json.dump({"turn": {"rotation_angle": 20.0}}, f)
    with open(os.path.join(path, "prompt.txt"), "w") as f:
        f.write("a ball\n")
    return str(path)


def test_run_edit_reads_release_png_only_with_the_lock(tmp_path):
    from diffusionhandles_amd import scene_io as IO
    run_edit = _run_edit()
    scene = _write_scene(tmp_path / "ball")
    out = str(tmp_path / "out")
    locked = argparse.Namespace(res=64, mode="pc", max_edits=0, background_lock=True)
    plain = argparse.Namespace(res=64, mode="pc", max_edits=0)
    assert run_edit.prepare_scene(locked, scene, out, None)["release"] is None          # no release.png
    rel = np.zeros((64, 64), dtype=np.float32)
    rel[40:, :10] = 1.0
    IO.write_png(os.path.join(scene, "release.png"), rel)
    p = run_edit.prepare_scene(locked, scene, out, None)
    assert p["release"].shape == (64, 64) and np.array_equal(p["release"].numpy(), rel)
    assert run_edit.prepare_scene(plain, scene, out, None)["release"] is None            # lock off: not read
    assert run_edit.prepare_scene(locked, None, out, None)["release"] is None            # the synthetic scene has none


def test_run_edit_cache_without_the_trajectory_is_not_usable(tmp_path):
    run_edit = _run_edit()
    cache = str(tmp_path / "identity.npz")
    locked, plain = argparse.Namespace(background_lock=True), argparse.Namespace()
    assert not run_edit.cache_usable(locked, cache) and not run_edit.cache_usable(plain, cache)
    np.savez(cache, latent_image=np.zeros(2))
    assert run_edit.cache_usable(plain, cache) and not run_edit.cache_usable(locked, cache)
    np.savez(cache, latent_image=np.zeros(2), trajectory=np.zeros(3))
    assert run_edit.cache_usable(plain, cache) and run_edit.cache_usable(locked, cache)
