"""CPU: scene directories with several object masks (scene_io.load_scene_geometry / load_scene / object_transform_args):
mask_0.png .. mask_{M-1}.png and transforms.json entries {"objects": [...], "object_weights": ...}."""
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_object_ref as R  # noqa: E402

from diffusionhandles_amd import scene_io as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 64
OBJECTS = [dict(rotation_angle=a, rotation_axis=list(ax), translation=list(tr)) for a, ax, tr in R.OCCLUDING]
ENTRIES = {"plain": {"objects": OBJECTS},
           "equal": {"objects": OBJECTS, "object_weights": "equal"},
           "listed": {"objects": [{}, {"translation": [0.1, 0.0, 0.0]}], "object_weights": [1, 2.5]}}


@pytest.fixture()
def scene(tmp_path):
    depth, bg, masks = R.two_spheres(RES)
    d = tmp_path / "two_spheres"
    d.mkdir()
    np.save(d / "depth.npy", depth[0, 0].numpy())
    np.save(d / "bg_depth.npy", bg[0, 0].numpy())
    for m, mask in enumerate(masks):
        S.write_png(str(d / f"mask_{m}.png"), mask[0, 0].numpy())
    S.write_png(str(d / "input.png"), np.full((RES, RES, 3), 0.5, dtype=np.float32))
    (d / "prompt.txt").write_text("two spheres on a plane\n")
    (d / "transforms.json").write_text(json.dumps(ENTRIES))
    return d, depth, bg, masks


def test_multi_mask_scene_loads_its_masks_and_their_union(scene):
    d, depth, bg, masks = scene
    # a mask.png beside the numbered masks is not read
    S.write_png(str(d / "mask.png"), np.ones((RES, RES), dtype=np.float32))
    geo = S.load_scene_geometry(str(d), RES)
    assert set(geo) == {"transforms", "fg_mask", "fg_masks", "depth", "bg_depth"}
    assert len(geo["fg_masks"]) == 2
    for got, want in zip(geo["fg_masks"], masks):
        assert got.dtype == torch.float32 and got.shape == (1, 1, RES, RES) and torch.equal(got, want)
    assert torch.equal(geo["fg_mask"], ((masks[0] != 0) | (masks[1] != 0)).float())
    assert 0 < float(geo["fg_mask"].sum()) == float(masks[0].sum() + masks[1].sum())
    assert torch.equal(geo["depth"], depth) and torch.equal(geo["bg_depth"], bg)
    assert list(geo["transforms"]) == ["plain", "equal", "listed"]
    sc = S.load_scene(str(d), RES)
    assert set(sc) == set(geo) | {"prompt", "img"} and sc["prompt"] == "two spheres on a plane"
    assert all(torch.equal(a, b) for a, b in zip(sc["fg_masks"], masks)) and torch.equal(sc["fg_mask"], geo["fg_mask"])
    # resized like mask.png: masks of another resolution stay {0, 1} maps of the asked size
    small = S.load_scene_geometry(str(d), 32)
    assert all(m.shape == (1, 1, 32, 32) and set(m.unique().tolist()) <= {0.0, 1.0} for m in small["fg_masks"])


def test_object_transform_args(scene):
    d = scene[0]
    tr = S.load_scene_geometry(str(d), RES)["transforms"]
    a = S.object_transform_args(tr["plain"])
    assert set(a) == {"transforms", "object_weights"} and a["object_weights"] is None and len(a["transforms"]) == 2
    for (ang, ax, t), (ra, rax, rt) in zip(a["transforms"], R.OCCLUDING):
        assert ang == float(ra) and isinstance(ang, float)
        assert ax.dtype == torch.float32 and torch.equal(ax, torch.tensor(rax, dtype=torch.float32))
        assert t.dtype == torch.float32 and torch.equal(t, torch.tensor(rt, dtype=torch.float32))
    assert S.object_transform_args(tr["equal"])["object_weights"] == "equal"
    b = S.object_transform_args(tr["listed"])
    assert b["object_weights"] == [1.0, 2.5] and all(isinstance(w, float) for w in b["object_weights"])
    ang, ax, t = b["transforms"][0]                                        # {} leaves the object in place: the defaults
    assert ang == 0.0 and ax.tolist() == [0.0, 1.0, 0.0] and t.tolist() == [0.0, 0.0, 0.0]
    assert b["transforms"][1][0] == 0.0 and torch.allclose(b["transforms"][1][2], torch.tensor([0.1, 0.0, 0.0]))
    with pytest.raises(ValueError, match="objects"):
        S.object_transform_args({"rotation_angle": 3.0})


def test_malformed_object_scenes_raise_naming_the_scene_and_the_entry(scene, tmp_path):
    d = scene[0]

    def write(entries):
        (d / "transforms.json").write_text(json.dumps(entries))
    # no "objects" in a multi-mask scene
    write({"plain": ENTRIES["plain"], "flat": {"rotation_angle": 10.0}})
    with pytest.raises(ValueError, match=r"two_spheres.*'flat'"):
        S.load_scene_geometry(str(d), RES)
    # a list that is not M long
    for objs in ([OBJECTS[0]], OBJECTS + [{}], []):
        write({"plain": ENTRIES["plain"], "short": {"objects": objs}})
        with pytest.raises(ValueError, match=r"two_spheres.*'short'"):
            S.load_scene_geometry(str(d), RES)
        with pytest.raises(ValueError, match=r"two_spheres.*'short'"):
            S.load_scene(str(d), RES)
    # "objects" in a single-mask scene
    one = tmp_path / "one_mask"
    shutil.copytree(d, one)
    os.rename(one / "mask_0.png", one / "mask.png")
    os.remove(one / "mask_1.png")
    (one / "transforms.json").write_text(json.dumps({"ok": {"rotation_angle": 10.0}, "multi": ENTRIES["plain"]}))
    with pytest.raises(ValueError, match=r"one_mask.*'multi'"):
        S.load_scene_geometry(str(one), RES)
    (one / "transforms.json").write_text(json.dumps({"ok": {"rotation_angle": 10.0}}))
    assert "fg_masks" not in S.load_scene_geometry(str(one), RES)
    # the masks are consecutive: mask_0 and mask_2 make a one-object scene
    gap = tmp_path / "gap"
    shutil.copytree(d, gap)
    os.rename(gap / "mask_1.png", gap / "mask_2.png")
    (gap / "transforms.json").write_text(json.dumps({"e": {"objects": [{}]}}))
    assert len(S.load_scene_geometry(str(gap), RES)["fg_masks"]) == 1
    # more than 8 masks
    many = tmp_path / "many"
    shutil.copytree(d, many)
    for m in range(2, 9):
        shutil.copy(many / "mask_1.png", many / f"mask_{m}.png")
    with pytest.raises(ValueError, match="at most 8"):
        S.load_scene_geometry(str(many), RES)


def test_single_mask_scene_loads_as_before():
    d = os.path.join(ROOT, "tests", "golden", "scene_banana_fruits")
    geo = S.load_scene_geometry(d, 64)
    assert set(geo) == {"transforms", "fg_mask", "depth", "bg_depth"}
    sc = S.load_scene(d, 64)
    assert set(sc) == {"transforms", "prompt", "img", "fg_mask", "depth", "bg_depth"}
    mask = S.load_image(os.path.join(d, "mask.png"))[None]
    if mask.shape[1] > 1:
        mask = mask.mean(dim=1, keepdim=True)
    assert torch.equal(geo["fg_mask"], (S.crop_and_resize(mask, 64) > 0.5).float()) and torch.equal(sc["fg_mask"], geo["fg_mask"])
    assert all("objects" not in t for t in geo["transforms"].values())
