"""CPU: scale and pivot of an object transform -- the test-side reference (tests/similarity_ref.py) is the oracle's rigid
transform at scale 1 and with the pivot at the centroid, bit for bit; the C ABI declares and exports the new entry; every
argument error comes before any device work; transforms.json entries with "scale" / "pivot"."""
import argparse
import json
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_object_ref as R  # noqa: E402
import similarity_ref as S  # noqa: E402

from diffusionhandles_amd.synthetic import make_scene  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERAL = (0.3, 0.9, -0.2)


def _scenes():
    depth, _, masks = R.two_spheres(128)
    d1, _, m1 = make_scene(128)
    return [("two_spheres/0", depth, masks[0]), ("two_spheres/1", depth, masks[1]), ("make_scene", d1, m1)]


@pytest.mark.parametrize("axis,order", [(R.Y, "blas"), (R.Y, "explicit"), (GENERAL, "explicit")])
def test_scale_one_and_centroid_pivot_are_the_oracle_bit_for_bit(axis, order):
    from oracle import depth_ref as D
    D.DOT_ORDER = order
    try:
        for name, depth, mask in _scenes():
            pts = D.unproject(depth[0, 0].numpy())
            m = mask[0, 0].numpy() > 0.5
            assert m.sum() > 500
            for angle, trans in ((25.0, [0.1, -0.05, 0.2]), (-40.0, [0.0, 0.0, 0.0])):
                want = D.rigid_transform(pts, np.asarray(axis, dtype=np.float32), angle, trans, m)
                assert want.dtype == np.float64
                cen = D.masked_centroid_f32(pts, m)
                for scale, pivot in ((None, None), (1.0, None), ((1.0, 1.0, 1.0), None), (None, cen), (1.0, tuple(float(v) for v in cen))):
                    got = S.similarity_transform(pts, np.asarray(axis, dtype=np.float32), angle, trans, m, scale, pivot)
                    assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), want.view(np.int64)), (name, angle, scale, pivot)
                # and the new members do something: the masked points move
                for scale, pivot in ((1.5, None), ((1.3, 0.8, 1.0), None), (None, cen + np.float32(0.25))):
                    got = S.similarity_transform(pts, np.asarray(axis, dtype=np.float32), angle, trans, m, scale, pivot)
                    assert np.isfinite(got).all() and not np.array_equal(got[m], want[m])
    finally:
        D.DOT_ORDER = "blas"


def test_uniform_scale_about_the_centroid_scales_the_offsets():
    """Without a turn, q' = fl32(q * s): every masked point lies at s times its offset from the centroid (one f32 rounding)."""
    from oracle import depth_ref as D
    depth, _, mask = make_scene(128)
    pts = D.unproject(depth[0, 0].numpy())
    m = mask[0, 0].numpy() > 0.5
    cen = D.masked_centroid_f32(pts, m)
    got = S.similarity_transform(pts, np.asarray(R.Y, dtype=np.float32), 0.0, [0.0, 0.0, 0.0], m, (1.5, 0.5, 2.0), None)
    q = (pts - cen)[m]
    want = (q * np.asarray([1.5, 0.5, 2.0], dtype=np.float32)).astype(np.float64) + cen.astype(np.float64)
    assert np.array_equal(got[m], want)


def test_one_object_helper_at_scale_one_is_the_multi_object_helper():
    depth, bg, masks = R.two_spheres(128)
    tfs = [(15.0, R.Y, (0.1, 0.0, -0.05)), (-20.0, R.Y, (-0.15, 0.05, 0.1))]
    disp, corr, dbg = S.transform_objects(depth, bg, masks, [tfs[0] + (None, None), tfs[1] + (1.0, None)])
    disp_r, corr_r, dbg_r = R.transform_objects(depth, bg, masks, tfs)
    assert len(corr_r) > 1000 and np.array_equal(corr.numpy(), corr_r.numpy()) and torch.equal(disp, disp_r)
    for k in ("zmap", "raw_mask", "cleaned", "vis"):
        assert np.array_equal(dbg[k], dbg_r[k]), k


@pytest.mark.parametrize("res", [128, 256])
def test_gpu_comparison_edits_keep_their_conditions(res):
    """The four edits of tests/test_similarity_gpu.py, by the reference alone: at least 100 pairs per object, no depth tie
    between the objects, and the pivot pixel at the lower edge of sphere 1."""
    from oracle import depth_ref as D
    depth, bg, masks = R.two_spheres(res)
    x, y = S.lower_edge_pixel(res)
    assert masks[1][0, 0, y, x] > 0.5 and masks[1][0, 0, y + 2, x] < 0.5
    D.DOT_ORDER = "explicit"
    try:
        for e, tfs in enumerate(S.edits_for(res, depth)):
            _, corr, dbg = S.transform_objects(depth, bg, masks, tfs)
            pairs = S.pairs_per_object(corr, masks)
            print(f"res {res} edit {e}: pairs per object {pairs}")
            assert min(pairs) >= 100 and R.z_ties_between_objects(dbg, res=res) == 0
    finally:
        D.DOT_ORDER = "blas"


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_header_table_and_library_have_the_entry():
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd import depth_transform as DT
    name = "dh_reproject_similarity_edits"
    raw = open(os.path.join(ROOT, "include", "diffhandles_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\b" + name + r"\s*\(", txt) and name in _lib.SIGNATURES
    assert int(re.search(r"#define\s+DH_SIMILARITY_ROW\s+(\d+)", txt).group(1)) == DT.SIMILARITY_ROW == 16
    assert "dh_reproject_object_edits" in raw[raw.index("Similarity transforms"):raw.index("#define DH_SIMILARITY_ROW")]   # cites what it extends
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.lib()
    assert name not in lib.dh_missing_symbols and hasattr(lib, name)
    decl = re.search(name + r"\s*\((.*?)\)\s*;", txt, flags=re.S).group(1)
    old = re.search(r"dh_reproject_object_edits\s*\((.*?)\)\s*;", txt, flags=re.S).group(1)
    assert " ".join(decl.split()) == " ".join(old.split())                       # the arguments of the entry it extends
    assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]) == 27
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES["dh_reproject_object_edits"]


def test_rows_of_the_new_entry():
    from diffusionhandles_amd import depth_transform as DT
    ax, tr = torch.tensor(GENERAL), torch.tensor([0.1, -0.05, 0.2])
    rows8 = DT._xform_rows([(25.0, ax, tr)])
    assert rows8.shape == (1, 8)                                                # the rigid entries' rows are what they were
    rows = DT._xform_rows([(25.0, ax, tr), (25.0, ax, tr, None, None), (25.0, ax, tr, 0.1, (1.0, 2.0, 0.1)),
                           (25.0, ax, tr, torch.tensor([1.3, 0.8, 1.0]), np.asarray([0.5, 0.25, 3.0]))], similarity=True)
    assert rows.shape == (4, 16) and rows.dtype == np.float64
    assert np.array_equal(rows[:, :8], np.repeat(rows8, 4, axis=0))
    one = [1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    f = lambda v: float(np.float32(v))
    assert rows[0, 8:].tolist() == one and rows[1, 8:].tolist() == one
    assert rows[2, 8:].tolist() == [f(0.1)] * 3 + [1.0, 2.0, f(0.1), 1.0, 0.0]     # float32 values, widened
    assert rows[3, 8:].tolist() == [f(1.3), f(0.8), 1.0, 0.5, 0.25, 3.0, 1.0, 0.0]


# ---- argument errors, no GPU ------------------------------------------------------------------------------------------------------
Y = torch.tensor(R.Y)
Z3 = torch.zeros(3)
BAD = [((10.0, Y), "members"), ((10.0, Y, Z3, 1.0), "members"), ((10.0, Y, Z3, 1.0, None, None), "members"),
       ((10.0, Y, Z3, 0.0, None), "scale"), ((10.0, Y, Z3, -1.5, None), "scale"), ((10.0, Y, Z3, float("nan"), None), "scale"),
       ((10.0, Y, Z3, float("inf"), None), "scale"), ((10.0, Y, Z3, 1e39, None), "scale"), ((10.0, Y, Z3, 1e-50, None), "scale"),
       ((10.0, Y, Z3, (1.0, 2.0), None), "scale"), ((10.0, Y, Z3, (1.0, 0.0, 1.0), None), "scale"), ((10.0, Y, Z3, "big", None), "scale"),
       ((10.0, Y, Z3, None, (1.0, 2.0)), "pivot"), ((10.0, Y, Z3, None, (1.0, 2.0, 3.0, 4.0)), "pivot"),
       ((10.0, Y, Z3, None, (0.0, float("inf"), 0.0)), "pivot"), ((10.0, Y, Z3, None, torch.tensor([0.0, float("nan"), 0.0])), "pivot"),
       ((10.0, Y, Z3, None, 2.0), "pivot")]


@pytest.mark.parametrize("tf,word", BAD)
def test_malformed_transforms_raise_before_any_device_work(tf, word):
    from diffusionhandles_amd import DiffusionHandles
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, masks = R.two_spheres(128)
    K = torch.eye(3)
    good = (10.0, Y, Z3)
    with pytest.raises(ValueError, match=word):
        DT.check_transform(tf, "edit 3, object 1")
    with pytest.raises(ValueError, match="edit 1, object 0.*" + word):
        DT.reproject_edits(depth, bg, masks[0], K, [good, tf])
    with pytest.raises(ValueError, match="edit 0, object 1.*" + word):
        DT.reproject_object_edits(depth, bg, masks, K, [[good, tf]])
    dh = object.__new__(DiffusionHandles)
    dh.conf = SimpleNamespace(depth_transform_mode="pc")
    dh.diffuser = SimpleNamespace(get_depth_intrinsics=lambda device=None: K, unet=None)
    with pytest.raises(ValueError, match="edit 0, object 1.*" + word):
        dh.transform_foreground_objects(depth, "two spheres", masks, bg, None, None, None, [good, tf])
    with pytest.raises(ValueError, match="edit 1, object 0.*" + word):
        dh.transform_foreground_objects_batch(depth, "two spheres", masks, bg, None, None, None, [[good, good], [tf, good]])
    with pytest.raises(ValueError, match="edit 1.*" + word):
        dh.transform_foreground_batch(depth, "two spheres", masks[0], bg, None, None, None, [good, tf])
    common = dict(depth=depth, prompt="two spheres", bg_depth=bg, null_text_emb=None, init_noise=None, activations=[depth])
    with pytest.raises(ValueError, match="edit 1, object 1.*" + word):
        dh.transform_foregrounds([dict(common, fg_mask=masks[0]), dict(common, fg_masks=masks, transforms=[good, tf])])
    if len(tf) == 5:
        kw = dict(scale=tf[3], pivot=tf[4])
        with pytest.raises(ValueError, match=word):
            DT.transform_depth(depth, bg, masks[0], K, 10.0, scale=tf[3], pivot=tf[4])
        with pytest.raises(ValueError, match=word):
            DT.transform_depth(depth, bg, masks[0], K, 10.0, depth_transform_mode="mesh", **kw)
        with pytest.raises(ValueError, match=word):
            dh.transform_foreground(depth, "two spheres", masks[0], bg, None, None, None, rot_angle=10.0, **kw)
        with pytest.raises(ValueError, match="edit 1.*" + word):
            dh.transform_foregrounds([dict(common, fg_mask=masks[0]), dict(common, fg_mask=masks[0], **kw)])


def test_mode_and_form_errors_come_before_any_device_work():
    from diffusionhandles_amd import DiffusionHandles
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, masks = R.two_spheres(128)
    K = torch.eye(3)
    # mesh mode has no scale; a scale of exactly 1 is no scale
    for scale in (1.5, (1.0, 1.0, 0.9)):
        with pytest.raises(NotImplementedError, match="scale"):
            DT.transform_depth(depth, bg, masks[0], K, 10.0, depth_transform_mode="mesh", scale=scale)
        with pytest.raises(NotImplementedError, match="scale"):
            DT.transform_depth_mesh(depth, bg, masks[0], K, 10.0, scale=scale, pivot=(0.0, 0.0, 2.0))
    dh = object.__new__(DiffusionHandles)
    dh.conf = SimpleNamespace(depth_transform_mode="mesh")
    dh.diffuser = SimpleNamespace(get_depth_intrinsics=lambda device=None: K, unet=None)
    with pytest.raises(NotImplementedError, match="scale"):
        dh.transform_foreground(depth, "two spheres", masks[0], bg, None, None, None, rot_angle=10.0, scale=2.0)
    # scale / pivot belong to the one-object form of transform_foregrounds
    dh.conf = SimpleNamespace(depth_transform_mode="pc")
    common = dict(depth=depth, prompt="two spheres", bg_depth=bg, null_text_emb=None, init_noise=None, activations=[depth])
    tf = (10.0, Y, Z3)
    for extra in (dict(scale=1.5), dict(pivot=(0.0, 0.0, 2.0))):
        with pytest.raises(ValueError, match="edit 0 mixes"):
            dh.transform_foregrounds([dict(common, fg_masks=masks, transforms=[tf, tf], **extra)])
    with pytest.raises(ValueError, match="outside"):
        DT.pivot_at_pixel(depth, K, 128, 3)
    with pytest.raises(ValueError, match="outside"):
        DT.pivot_at_pixel(depth, K, 3, -1)
    # without a GPU a well-formed call gets as far as the device and fails loudly there
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            DT.transform_depth(depth, bg, masks[0], K, 10.0, scale=1.5, pivot=(0.0, 0.0, 2.0))


def test_signatures_keep_the_reference_prefix():
    import inspect
    from diffusionhandles_amd import DiffusionHandles
    from diffusionhandles_amd import depth_transform as DT
    ref = ["depth", "bg_depth", "fg_mask", "intrinsics", "rot_angle", "rot_axis", "translation", "use_input_depth_normalization"]
    assert list(inspect.signature(DT.transform_depth).parameters) == ref + ["depth_transform_mode", "scale", "pivot"]
    assert list(inspect.signature(DT.transform_depth_pc).parameters) == ref + ["scale", "pivot"]
    assert list(inspect.signature(DT.transform_depth_mesh).parameters)[:8] == ref
    p = list(inspect.signature(DiffusionHandles.transform_foreground).parameters)
    assert p[-2:] == ["scale", "pivot"] and p[:-2] == ["self", "depth", "prompt", "fg_mask", "bg_depth", "null_text_emb", "init_noise",
                                                       "activations", "rot_angle", "rot_axis", "translation", "fg_weight", "bg_weight",
                                                       "use_input_depth_normalization"]
    for f in (DT.transform_depth, DT.transform_depth_pc, DT.transform_depth_mesh, DiffusionHandles.transform_foreground):
        sig = inspect.signature(f)
        assert sig.parameters["scale"].default is None and sig.parameters["pivot"].default is None


# ---- scene directories -----------------------------------------------------------------------------------------------------------
def _write_scene(path, transforms, n_masks=0):
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
    with open(os.path.join(path, "transforms.json"), "w") as f:
        json.dump(transforms, f)
    return str(path)


def test_scene_entries_with_and_without_scale_and_pivot(tmp_path):
    from diffusionhandles_amd import scene_io as IO
    entries = {"plain": {"translation": [0.1, 0.0, 0.0], "rotation_axis": [0.0, 1.0, 0.0], "rotation_angle": 20.0},
               "grow": {"rotation_angle": 5.0, "scale": 1.5},
               "stretch": {"scale": [1.3, 0.8, 1], "pivot": [0.25, -0.5, 2.5]},
               "hinge": {"rotation_angle": 40.0, "rotation_axis": [0.0, 0.0, 1.0], "pivot": [0, 0.5, 3]}}
    geo = IO.load_scene_geometry(_write_scene(tmp_path / "one", entries), 64)
    assert "fg_masks" not in geo and list(geo["transforms"]) == list(entries)
    a = {n: IO.transform_args(t) for n, t in geo["transforms"].items()}
    assert set(a["plain"]) == {"rot_angle", "rot_axis", "translation"}                    # exactly what it gave before
    assert a["plain"]["rot_angle"] == 20.0 and a["plain"]["translation"].tolist() == pytest.approx([0.1, 0.0, 0.0])
    assert set(a["grow"]) == {"rot_angle", "rot_axis", "translation", "scale"} and a["grow"]["scale"] == 1.5
    assert a["stretch"]["scale"] == (1.3, 0.8, 1.0) and a["stretch"]["pivot"] == (0.25, -0.5, 2.5)
    assert set(a["hinge"]) == {"rot_angle", "rot_axis", "translation", "pivot"} and a["hinge"]["pivot"] == (0.0, 0.5, 3.0)
    from diffusionhandles_amd import depth_transform as DT
    for kw in a.values():                                                                  # what the edit calls accept
        DT.check_transform((kw["rot_angle"], kw["rot_axis"], kw["translation"], kw.get("scale"), kw.get("pivot")))
    # inside "objects"
    multi = {"both": {"objects": [{"rotation_angle": 10.0, "scale": 0.6}, {}], "object_weights": "equal"},
             "rigid": {"objects": [{"rotation_angle": 10.0}, {"translation": [0.0, 0.1, 0.0]}]},
             "hinge": {"objects": [{}, {"rotation_angle": 40.0, "pivot": [0.1, 0.2, 3.0]}]}}
    geo = IO.load_scene_geometry(_write_scene(tmp_path / "two", multi, n_masks=2), 64)
    assert len(geo["fg_masks"]) == 2
    o = {n: IO.object_transform_args(t) for n, t in geo["transforms"].items()}
    assert [len(t) for t in o["both"]["transforms"]] == [5, 3] and o["both"]["transforms"][0][3:] == (0.6, None)
    assert o["both"]["object_weights"] == "equal"
    assert [len(t) for t in o["rigid"]["transforms"]] == [3, 3] and o["rigid"]["object_weights"] is None
    assert [len(t) for t in o["hinge"]["transforms"]] == [3, 5] and o["hinge"]["transforms"][1][3:] == (None, (0.1, 0.2, 3.0))
    for args in o.values():
        for m, tf in enumerate(args["transforms"]):
            DT.check_transform(tf, f"object {m}")


@pytest.mark.parametrize("bad,word", [({"scale": 0}, "scale"), ({"scale": -2.0}, "scale"), ({"scale": [1.0, 2.0]}, "scale"),
                                      ({"scale": "big"}, "scale"), ({"scale": [1.0, "x", 1.0]}, "scale"), ({"scale": True}, "scale"),
                                      ({"scale": 1e39}, "scale"), ({"scale": None}, "scale"), ({"pivot": [1.0, 2.0]}, "pivot"),
                                      ({"pivot": 3.0}, "pivot"), ({"pivot": [0.0, 1e39, 0.0]}, "pivot"),
                                      ({"pivot": [0.0, None, 0.0]}, "pivot")])
def test_malformed_scene_values_raise_when_the_scene_is_loaded(tmp_path, bad, word):
    from diffusionhandles_amd import scene_io as IO
    one = _write_scene(tmp_path / "lamp", {"fine": {"scale": 1.2}, "broken": dict({"rotation_angle": 10.0}, **bad)})
    with pytest.raises(ValueError, match=r"lamp.*'broken'.*" + word):
        IO.load_scene_geometry(one, 64)
    two = _write_scene(tmp_path / "cups", {"fine": {"objects": [{}, {}]}, "broken": {"objects": [{}, bad]}}, n_masks=2)
    with pytest.raises(ValueError, match=r"cups.*'broken', object 1.*" + word):
        IO.load_scene_geometry(two, 64)
    with pytest.raises(ValueError, match=word):
        IO.transform_args(bad)


def test_single_mask_scene_of_the_reference_is_unchanged():
    from diffusionhandles_amd import scene_io as IO
    geo = IO.load_scene_geometry(os.path.join(ROOT, "tests", "golden", "scene_banana_fruits"), 64)
    assert "fg_masks" not in geo and len(geo["transforms"]) >= 3
    for t in geo["transforms"].values():
        kw = IO.transform_args(t)
        assert list(kw) == ["rot_angle", "rot_axis", "translation"]
        assert kw["rot_axis"].dtype == torch.float32 and kw["translation"].shape == (3,)


def test_run_edit_refuses_a_scale_in_mesh_mode_before_the_identity(tmp_path):
    """prepare_scene is host work only: the refusal comes before any engine is built."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import run_edit
    from diffusionhandles_amd import scene_io as IO
    scene = _write_scene(tmp_path / "cup", {"grow": {"scale": 1.5}, "hinge": {"rotation_angle": 30.0, "pivot": [0.0, 0.5, 3.0]}})
    IO.write_png(os.path.join(scene, "input.png"), np.zeros((64, 64, 3), dtype=np.uint8))
    with open(os.path.join(scene, "prompt.txt"), "w") as f:
        f.write("a cup\n")
    args = argparse.Namespace(res=64, mode="mesh", max_edits=0)
    with pytest.raises(NotImplementedError, match="'grow'.*scale"):
        run_edit.prepare_scene(args, scene, str(tmp_path / "out"), None)
    p = run_edit.prepare_scene(args, scene, str(tmp_path / "out"), ["hinge"])                # a pivot alone is fine in mesh mode
    assert [tf["name"] for tf in p["transforms"]] == ["hinge"] and p["transforms"][0]["pivot"] == (0.0, 0.5, 3.0)
    args.mode = "pc"
    p = run_edit.prepare_scene(args, scene, str(tmp_path / "out"), None)
    assert p["transforms"][0]["scale"] == 1.5 and "pivot" not in p["transforms"][0]
