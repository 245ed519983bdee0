"""CPU: bend edits ("Bend edits").  tests/bend_ref.py against the references it is composed from (one-hot and dyadic
weights are the rigid edit, a hard hinge is the two-object edit of the halves), depth_transform.bend_chain / check_bend /
Bend, the host plan, the "bend" key of transforms.json, and the refusals of mesh mode -- all before any device work."""
import ctypes
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reproject_calls as RC  # noqa: E402
import bend_ref as BR  # noqa: E402
import footprints_ref as F  # noqa: E402
import multi_object_ref as R  # noqa: E402
import object_copies_ref as OC  # noqa: E402
import similarity_ref as S  # noqa: E402
import test_arena_hooks as AH  # noqa: E402  (helpers only: the arena fixture and the size / gap / take check)
from oracle import depth_ref as D  # noqa: E402

pytestmark = pytest.mark.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y = R.Y
Z = (0.0, 0.0, 1.0)
Z0 = (0.0, 0.0, 0.0)


def _scene(res):
    depth, bg, masks = R.two_spheres(res)
    return depth, bg, masks, S.edits_for(res, depth)


def _pivot(depth, x, y):
    return tuple(float(v) for v in D.unproject(depth[0, 0].numpy())[y, x])


def _centre(res, sphere):
    cx, cy, rad, _ = R.SPHERES[sphere]
    k = res / 512.0
    return int(cx * k), int(cy * k), int(rad * k)


def _same_as_rigid(bent, rigid, what):
    """Every output array of bend_ref.transform_bend against similarity_ref.transform_objects' (its vis / tx / ty speak about the
    visible points, transform_bend's about every point)."""
    assert torch.equal(bent[1], rigid[1]), f"{what}: correspondences"
    assert np.array_equal(bent[0].numpy(), rigid[0].numpy()), f"{what}: filled disparity"
    b, r = bent[2], rigid[2]
    for k in ("zmap", "raw_mask", "cleaned", "inpaint", "disparity"):
        assert np.array_equal(b[k], r[k]), f"{what}: {k}"
    assert np.array_equal(b["vis"], r["vis"]), f"{what}: vis"
    assert np.array_equal(b["tx"][b["vis"]], r["tx"]) and np.array_equal(b["ty"][b["vis"]], r["ty"]), f"{what}: targets"


# ---- 1, 2. weights that change nothing -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [64, 128])
def test_one_hot_and_dyadic_weights_are_the_rigid_edit(res):
    depth, bg, masks, edits = _scene(res)
    m0 = masks[0][0, 0].numpy() != 0
    other = [(70.0, Z, (0.3, 0.2, 0.1)), edits[3][1], (5.0, Y, Z0, 2.0, None)]
    for e, tfs in enumerate(edits[:3]):
        rigid = S.transform_objects(depth, bg, masks, tfs)
        # one-hot on bone 0, B = 1, 2 and 4 (the other bones are OTHER transforms: their weight is 0)
        for B in (1, 2, 4):
            bend = BR.one_hot([tfs[0]] + other[:B - 1], m0)
            _same_as_rigid(BR.transform_bend(depth, bg, masks, [0, 1], [bend, tfs[1]]), rigid, f"res {res} edit {e} one-hot B={B}")
        # all bones one row, dyadic weights: the sum is exact
        for w in ((0.5, 0.5), (0.25, 0.25, 0.25, 0.25)):
            ws = np.stack([np.full((res, res), v, dtype=np.float32) for v in w])
            bend = BR.Bend([tfs[0]] * len(w), ws)
            _same_as_rigid(BR.transform_bend(depth, bg, masks, [0, 1], [bend, tfs[1]]), rigid, f"res {res} edit {e} weights {w}")
    # all weights zero: bone 0 with weight 1
    bend = BR.Bend([edits[0][0], other[0]], np.zeros((2, res, res), dtype=np.float32))
    _same_as_rigid(BR.transform_bend(depth, bg, masks, [0, 1], [bend, edits[0][1]]), S.transform_objects(depth, bg, masks, edits[0]),
                   f"res {res} all-zero weights")


# ---- 3. a hard hinge is the two-object edit of the halves ----------------------------------------------------------------------
@pytest.mark.parametrize("res", [64, 128])
def test_a_hard_hinge_is_the_edit_of_the_two_halves(res):
    depth, bg, masks, edits = _scene(res)
    cx, cy, rad = _centre(res, 0)
    pivot = _pivot(depth, cx, cy)
    m0 = masks[0][0, 0].numpy() != 0
    left = m0 & (np.arange(res)[None, :] < cx)
    right = m0 & ~left
    assert left.any() and right.any()
    bones = [(0.0, Y, Z0, None, pivot), (25.0, Z, (0.05, 0.0, -0.1), None, pivot)]
    w = np.stack([left, ~left]).astype(np.float32)          # (outside the mask the weights do not matter: one-hot on bone 1)
    t = lambda a: torch.from_numpy(a.astype(np.float32))[None, None]
    split = S.transform_objects(depth, bg, [t(left), t(right), masks[1]], bones + [edits[0][1]])
    assert R.z_ties_between_objects(split[2], res=res) == 0, "choose another angle: the split edit has a tie between objects"
    bent = BR.transform_bend(depth, bg, masks, [0, 1], [BR.Bend(bones, w), edits[0][1]])
    assert OC.z_ties_between_instances(BR.foreground_dbg(bent[2], res), res) == 0
    for k in ("zmap", "raw_mask", "cleaned", "disparity"):
        assert np.array_equal(bent[2][k], split[2][k]), k
    assert np.array_equal(bent[0].numpy(), split[0].numpy())
    rows = lambda c: sorted(map(tuple, c.numpy().tolist()))
    assert rows(bent[1]) == rows(split[1]) and len(bent[1]) > 100
    # and it is not the rigid edit of either bone
    assert not np.array_equal(bent[2]["raw_mask"], S.transform_objects(depth, bg, masks, [bones[1], edits[0][1]])[2]["raw_mask"])


# ---- 4. bend_chain and check_bend ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [64, 128])
@pytest.mark.parametrize("bones", [2, 3, 4])
def test_bend_chain_weights_and_the_fixed_side(res, bones):
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, masks, edits = _scene(res)
    cx, cy, rad = _centre(res, 0)
    p0, p1, width = (cx, cy - rad), (cx, cy + rad), res / 8.0
    pivot = _pivot(depth, cx, cy)
    bend = DT.bend_chain(depth, D.intrinsics_f32(), masks[0], p0, p1, width, 60.0, Z, (0.0, 0.1, 0.0), pivot=pivot, bones=bones)
    assert isinstance(bend, DT.Bend) and len(bend.bones) == bones and tuple(bend.weights.shape) == (bones, res, res)
    w = bend.weights.numpy()
    assert w.dtype == np.float32 and np.array_equal(w, BR.chain_weights((res, res), p0, p1, width, bones)), "the restated weights"
    assert np.abs(w.astype(np.float64).sum(axis=0) - 1.0).max() <= 1e-6 and w.min() >= 0.0
    d = BR.signed_distance((res, res), p0, p1)
    outside = np.abs(d) > width / 2
    assert np.isin(w[:, outside], (0.0, 1.0)).all() and (w[0][d < -width / 2] == 1.0).all() and (w[-1][d > width / 2] == 1.0).all()
    inside = np.abs(d) < width / 2 - 1e-9
    assert ((w > 0).sum(axis=0)[inside] <= 2).all(), "a hat has two neighbours"
    for b, tf in enumerate(bend.bones):
        assert tf[0] == 60.0 * b / (bones - 1) and tuple(tf[2]) == (0.0, float(np.float32(0.1)) * b / (bones - 1), 0.0)
        assert tf[3] is None and tuple(float(v) for v in tf[4]) == pivot
    ref = BR.chain(depth, masks[0], p0, p1, width, 60.0, Z, (0.0, 0.1, 0.0), pivot, bones)
    assert [tuple(b[2]) for b in ref.bones] == [tuple(b[2]) for b in bend.bones]
    # the fixed side's points keep their pixels
    out = BR.transform_bend(depth, bg, masks, [0, 1], [ref, (0.0, Y, Z0)], infill=False)
    m0 = masks[0][0, 0].numpy() != 0
    ys, xs = np.nonzero(m0)
    fixed = (d[m0] < -width / 2)
    n0 = int(m0.sum())
    assert fixed.sum() > 10
    assert np.array_equal(out[2]["tx"][:n0][fixed], xs[fixed]) and np.array_equal(out[2]["ty"][:n0][fixed], ys[fixed])
    moved = d[m0] > width / 2
    assert (out[2]["tx"][:n0][moved] != xs[moved]).any()
    # the checked Bend: bones through check_transform, weights float32 [B, H, W]
    checked = DT.check_bend(bend, masks[0], "x")
    assert isinstance(checked, DT.Bend) and checked.weights.dtype == torch.float32 and len(checked.bones[0]) == 5
    assert DT.check_body(bend, masks[0], "x").bones == checked.bones and DT.check_body((1.0, Y, Z0), None, "x") == DT.check_transform((1.0, Y, Z0))


def test_bend_chain_and_check_bend_refusals():
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, masks, _ = _scene(64)
    K = D.intrinsics_f32()
    piv = _pivot(depth, 20, 32)
    ok = dict(p0=(20, 10), p1=(20, 50), width=8.0, rot_angle=30.0, rot_axis=Z, pivot=piv)
    for kw, word in ((dict(width=0.0), "width"), (dict(width=-1.0), "width"), (dict(width=float("nan")), "width"),
                     (dict(p1=(20, 10)), "p0 == p1"), (dict(bones=1), "bones"), (dict(bones=5), "bones"), (dict(bones=2.0), "bones")):
        with pytest.raises(ValueError, match=f"bend_chain.*{word}"):
            DT.bend_chain(depth, K, masks[0], **dict(ok, **kw))
    good = DT.bend_chain(depth, K, masks[0], **ok)
    w = good.weights
    what = "transform_foreground_objects: edit 2, instance 1"
    nan = w.clone()
    nan[0, 0, 0] = float("nan")
    neg = w.clone()
    neg[0, 3, 3], neg[1, 3, 3] = -0.5, 1.5
    half = w * 0.5
    for bad, word in ((DT.Bend([], w[:0]), "1 to 4 bones"), (DT.Bend(list(good.bones) * 3, w.repeat(3, 1, 1)), "1 to 4 bones"),
                      (DT.Bend([(1.0, Y)], w[:1]), "bone 0"), (DT.Bend([good.bones[0], (1.0, Y, Z0, -1.0, None)], w), "bone 1.*scale"),
                      (DT.Bend(good.bones, w[:1]), r"weights must be \[2, 64, 64\]"), (DT.Bend(good.bones, w[:, :32]), "weights must be"),
                      (DT.Bend(good.bones, w[0]), "weights must be"), (DT.Bend(good.bones, "x"), "weights"),
                      (DT.Bend(good.bones, nan), "finite"), (DT.Bend(good.bones, neg), ">= 0"), (DT.Bend(good.bones, half), "sum to 1"),
                      ((1.0, Y, Z0), "expected a Bend")):
        with pytest.raises(ValueError, match=f"{what}: .*{word}"):
            DT.check_bend(bad, masks[0], what)
    # the sum is asked only on the mask's pixels; numpy weights are taken too
    off = w.clone()
    off[:, masks[0][0, 0] == 0] = 0.0
    assert DT.check_bend(DT.Bend(good.bones, off.numpy()), masks[0], what).weights.dtype == torch.float32
    # the plan names the call, the edit and the instance; the facade names its own call
    with pytest.raises(ValueError, match="reproject_bend_edits: edit 1, object 0: weights must sum to 1"):
        DT.reproject_plan(depth, masks, [[good, (0.0, Y, Z0)], [DT.Bend(good.bones, half), (0.0, Y, Z0)]])
    with pytest.raises(ValueError, match="reproject_bend_edits: edit 0, instance 2: .*weights must be"):
        DT.reproject_plan(depth, masks, [[(0.0, Y, Z0), (0.0, Y, Z0), DT.Bend(good.bones, w[:, :32])]], instances=[0, 1, 0])
    import test_footprints_ref as FP
    dh = FP._handles("pc")
    common = dict(depth=depth, prompt="p", bg_depth=bg, null_text_emb=None, init_noise=None, activations=[depth])
    for name, call in (("transform_foreground_objects",
                        lambda b: dh.transform_foreground_objects(depth, "p", masks, bg, None, None, None, [(0.0, Y, Z0), b])),
                       ("transform_foreground_objects_batch",
                        lambda b: dh.transform_foreground_objects_batch(depth, "p", masks, bg, None, None, None, [[(0.0, Y, Z0), b]])),
                       ("transform_foregrounds", lambda b: dh.transform_foregrounds([dict(common, fg_masks=masks, transforms=[(0.0, Y, Z0), b])]))):
        with pytest.raises(ValueError, match=f"{name}.*edit 0, object 1: weights must sum to 1"):
            call(DT.Bend(good.bones, half))


# ---- 5. footprints close the outside of the bend -------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [64, 128])
def test_footprints_leave_no_more_to_in_fill(res):
    """A 60 degree chain of sphere 1, width res / 8, 3 bones: the share of the cleaned mask that is in-filled, with footprints
    and without (the numbers of DESIGN.md, "Bend edits": at 128 0.0761 with, 0.1406 without; at 64 the CLOSE bridges every gap, 0 and 0)."""
    depth, bg, masks, _ = _scene(res)
    cx, cy, rad = _centre(res, 1)
    bend = BR.chain(depth, masks[1], (cx, cy - rad), (cx, cy + rad), res / 8.0, 60.0, Z, Z0, _pivot(depth, cx, cy), 3)
    tfs = [(0.0, Y, Z0), bend]
    without = F.infill_share(BR.transform_bend(depth, bg, masks, [0, 1], tfs, infill=False)[2])
    with_fp = F.infill_share(BR.transform_bend(depth, bg, masks, [0, 1], tfs, footprints=True, infill=False)[2])
    print(f"res {res}: in-fill share of the cleaned mask {with_fp:.4f} with footprints, {without:.4f} without")
    assert with_fp <= without


# ---- 6. the type, the plan, the scene key, mesh mode ---------------------------------------------------------------------------
def test_the_bend_type():
    from diffusionhandles_amd import depth_transform as DT
    w = np.zeros((2, 4, 4), dtype=np.float32)
    b = DT.Bend([[1.0, Y, Z0], (2.0, Y, Z0, None, None)], w)
    assert b.bones == ((1.0, Y, Z0), (2.0, Y, Z0, None, None)) and b.weights is w and "2 bones" in repr(b)
    for attempt in (lambda: setattr(b, "bones", ()), lambda: setattr(b, "weights", None), lambda: setattr(b, "x", 1), lambda: delattr(b, "bones")):
        with pytest.raises(AttributeError):
            attempt()
    assert DT.MAX_BONES == 4 and "#define DH_MAX_BONES 4" in open(os.path.join(ROOT, "include", "diffhandles_hip.h")).read()


def test_signatures_and_header():
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd import depth_transform as DT
    assert list(inspect.signature(DT.reproject_bend_edits).parameters) == list(inspect.signature(DT.reproject_surface_edits).parameters)
    assert list(inspect.signature(DT.bend_chain).parameters) == ["depth", "intrinsics", "mask", "p0", "p1", "width", "rot_angle", "rot_axis",
                                                                 "translation", "pivot", "bones"]
    assert inspect.signature(DT.bend_chain).parameters["bones"].default == 2
    assert list(inspect.signature(DT.check_bend).parameters) == ["bend", "mask", "what"]
    sig = _lib.SIGNATURES
    assert sig["dh_reproject_bend_edits"][1] == sig["dh_reproject_surface_edits"][1] + [_lib.c_i, _lib.c_p]
    assert sig["dh_reproject_bend_ws_bytes"][1] == sig["dh_reproject_surface_ws_bytes"][1][:-1] + [_lib.c_i, _lib.c_i] + sig["dh_reproject_surface_ws_bytes"][1][-1:]
    header = open(os.path.join(ROOT, "include", "diffhandles_hip.h")).read()
    assert "int dh_reproject_bend_edits(" in header and "int dh_reproject_bend_ws_bytes(" in header
    for words in ("The weights are the CALLER's to validate", "with no normalisation", "not in the reference", "never reads bone_w on the host"):
        assert words in header, words
    from diffusionhandles_amd.diffusion_handles import DiffusionHandles
    assert "Bend" not in str(inspect.signature(DiffusionHandles.transform_foreground)), "transform_foreground keeps the reference's list"
    L = _lib.lib()

    def q(name, *a):
        nb = ctypes.c_size_t()
        assert getattr(L, name)(*a, ctypes.byref(nb)) == 0, L.dh_last_error()
        return nb.value
    for a in ((64, 900, 3, 2, 2), (128, 20000, 8, 2, 3)):
        for vs in (0, 1):
            base = q("dh_reproject_surface_ws_bytes", *a, vs)
            assert q("dh_reproject_bend_ws_bytes", *a, vs, 0, 1) == base
            for B in (2, 3, 4):
                extra = a[2] * a[4] * (B - 1) * 128
                assert extra <= q("dh_reproject_bend_ws_bytes", *a, vs, 0, B) - base < extra + 256
        assert q("dh_reproject_bend_ws_bytes", *a, 0, 1, 1) == q("dh_reproject_camera_workspace_bytes", *a, 1)
    nb = ctypes.c_size_t(7)
    for bad in ((64, 900, 3, 2, 2, 0, 0, 0), (64, 900, 3, 2, 2, 0, 0, 5), (64, 900, 3, 2, 2, 1, 1, 2)):
        assert L.dh_reproject_bend_ws_bytes(*bad, ctypes.byref(nb)) != 0 and nb.value == 7


BEND_SIZES = [((64, 900, 3, 2, 2, 0, 0, 1), 890496), ((64, 900, 3, 2, 2, 1, 0, 1), 1383948), ((64, 900, 3, 2, 2, 0, 0, 4), 892800),
              ((60, 1, 1, 1, 1, 1, 0, 3), 426500)]
L = AH.L


@pytest.mark.parametrize("args,size", BEND_SIZES, ids=[str(a) for a, _ in BEND_SIZES])
def test_sizes_gaps_and_takes_of_the_bend_query(L, args, size):
    """tests/test_arena_hooks.py's check of a size query: at n_bones = 1 the numbers tests/test_view_surfaces_ref.py pins for the
    surface query; with bones the first take (the rows) grows by K N (B - 1) 128 bytes."""
    AH.test_sizes_gaps_and_takes(L, "dh_reproject_bend_ws_bytes", args, size)


def test_the_plan_with_and_without_a_bend():
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, masks, edits = _scene(64)
    cx, cy, rad = _centre(64, 0)
    piv = _pivot(depth, cx, cy)
    mk = lambda bones: DT.bend_chain(depth, D.intrinsics_f32(), masks[0], (cx, cy - rad), (cx, cy + rad), 8.0, 40.0, Z, pivot=piv, bones=bones)
    tf = (10.0, Y, Z0)
    p = DT.reproject_plan(depth, masks, [[mk(2), tf], [tf, tf], [mk(3), tf]])
    assert (p.kind, RC.fields(p)) == ("objects", dict(RC.INSTANCE, bones=3))          # the bones, on the instance carving
    assert p.bent is True and p.n_bones == 3 and p.cap == p.n_pts and not p.with_table
    n0, n1 = int(masks[0].sum()), int(masks[1].sum())
    fg_pix = torch.cat([torch.nonzero(m.reshape(-1) != 0)[:, 0] for m in masks]).to(torch.int32)
    rows, w = DT._bone_rows(p, fg_pix, torch.device("cpu"))
    assert rows.shape == (3 * 2 * 3, 16) and rows.dtype == np.float64 and tuple(w.shape) == (3, n0 + n1, 3) and w.dtype == torch.float32
    one = DT._xform_rows([tf], similarity=True)[0]
    assert np.array_equal(rows[3:6], np.tile(one, (3, 1))) and np.array_equal(rows[6:12], np.tile(one, (6, 1)))       # an ordinary instance: bone 0 thrice
    assert np.array_equal(rows[2], rows[0]) and not np.array_equal(rows[1], rows[0])                                  # 2 bones padded with bone 0
    assert torch.equal(w[0, :n0, :2], p.edits[0][0].weights.reshape(2, -1)[:, fg_pix[:n0].long()].t()) and bool((w[0, :n0, 2] == 0).all())
    assert bool((w[:, n0:, 0] == 1).all()) and bool((w[:, n0:, 1:] == 0).all()) and bool((w[1, :, 0] == 1).all())
    assert torch.equal(w[2, :n0], p.edits[2][0].weights.reshape(3, -1)[:, fg_pix[:n0].long()].t())
    # footprints, a camera with view surfaces, copies, a reflecting border: the one entry
    for kw, cap in ((dict(footprints=True), 64 * 64), (dict(cameras=[(4.0, Y, Z0, None)], view_surfaces=True), 64 * 64),
                    (dict(infill_border="reflect"), None), (dict(cameras=[(4.0, Y, Z0, None)]), None)):
        q = DT.reproject_plan(depth, masks, [[mk(4), tf]], **kw)
        f = RC.fields(q)
        assert (f["bones"], f["table"], q.n_bones, q.bent) == (4, True, 4, True)
        assert (f["views"], f["surfaces"], f["border"]) == ("cameras" in kw, int("view_surfaces" in kw), int("infill_border" in kw))
        assert q.cap == (q.n_pts if cap is None else cap)
    q = DT.reproject_plan(depth, masks, [[mk(2), mk(4), tf]], instances=[0, 0, 1])
    assert q.n_bones == 4 and q.with_table and q.n_pts == 2 * n0 + n1
    # without a Bend every plan is the plan it was: the entries named before this feature, one row per instance
    for kw, call in ((dict(), RC.FOOTPRINT), (dict(instances=[0, 1, 0]), RC.INSTANCE), (dict(infill_border="reflect"), RC.border(RC.INSTANCE)),
                     (dict(cameras=[(4.0, Y, Z0, None)]), RC.CAMERA), (dict(cameras=[(4.0, Y, Z0, None)], view_surfaces=True), RC.SURFACE)):
        n = 3 if "instances" in kw else 2
        q = DT.reproject_plan(depth, masks, [[tf] * n], **kw)
        assert (RC.fields(q), q.n_bones, q.bent) == (call, 1, False), kw
        assert q.edits == [[DT.check_transform(tf)] * n]


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


BEND = {"p0": [20, 10], "p1": [20, 50], "width": 8, "bones": 3}


def test_the_bend_key_of_a_scene_directory(tmp_path):
    from diffusionhandles_amd import scene_io as IO
    member = {"rotation_angle": 40.0, "rotation_axis": [0, 0, 1], "translation": [0.0, 0.1, 0.0], "bend": dict(BEND, pivot_pixel=[20, 32])}
    scene = _write_scene(tmp_path / "multi", {"plain": {"objects": [{"rotation_angle": 5.0}, {}]}, "bent": {"objects": [member, {}]},
                                               "copy": {"objects": [{}, {}, {"mask": 0, "bend": BEND, "pivot": [0.1, 0.2, 3.0]}]}})
    geo = IO.load_scene_geometry(scene, 64)
    a = IO.object_transform_args(geo["transforms"]["plain"])
    assert "bends" not in a and set(a) == {"transforms", "object_weights"}, "a file without the key loads to what it loaded to"
    a = IO.object_transform_args(geo["transforms"]["bent"])
    assert a["bends"] == [dict(p0=(20.0, 10.0), p1=(20.0, 50.0), width=8.0, bones=3, pivot_pixel=(20, 32)), None]
    assert a["transforms"][0][0] == 40.0 and len(a["transforms"][0]) == 3
    a = IO.object_transform_args(geo["transforms"]["copy"])
    assert a["instances"] == [0, 1, 0] and a["bends"][:2] == [None, None] and a["bends"][2]["bones"] == 3
    assert a["transforms"][2][4] == (0.1, 0.2, 3.0) and "pivot_pixel" not in a["bends"][2]
    assert IO.bend_args({"bend": {"p0": [1, 2], "p1": [3, 4.5], "width": 2}}) == dict(p0=(1.0, 2.0), p1=(3.0, 4.5), width=2.0, bones=2)
    assert IO.bend_args({"rotation_angle": 1.0}) is None
    # a single-mask scene: the entry itself
    single = _write_scene(tmp_path / "single", {"bent": {"rotation_angle": 30.0, "bend": BEND}, "plain": {"rotation_angle": 30.0}}, n_masks=0)
    geo = IO.load_scene_geometry(single, 64)
    a = IO.transform_args(geo["transforms"]["bent"])
    assert a["bend"] == dict(p0=(20.0, 10.0), p1=(20.0, 50.0), width=8.0, bones=3) and a["rot_angle"] == 30.0
    assert "bend" not in IO.transform_args(geo["transforms"]["plain"])
    # malformed values: ValueError naming the scene and the entry, when the scene is loaded
    for bad, word in ((dict(BEND, width=0), "width"), (dict(BEND, width="x"), "width"), (dict(BEND, p1=[20, 10]), "no line"),
                      (dict(BEND, p0=[1]), "p0"), (dict(BEND, bones=1), "bones"), (dict(BEND, bones=5), "bones"), (dict(BEND, bones=2.5), "bones"),
                      (dict(BEND, pivot_pixel=[1.5, 2]), "pivot_pixel"), (dict(BEND, angle=3), "unknown keys"), ([1, 2], "must be an object"),
                      ({"p0": [1, 2], "p1": [3, 4]}, "needs \"width\"")):
        where = _write_scene(tmp_path / "bad", {"t0": {"objects": [{}, {"bend": bad}]}})
        with pytest.raises(ValueError, match=f"bad: transform 't0', object 1: .*{word}"):
            IO.load_scene_geometry(where, 64)
    for entry, word in (({"objects": [{"scale": 2.0, "bend": BEND}, {}]}, "object 0: .*takes no \"scale\""),
                        ({"objects": [{"pivot": [0, 0, 1], "bend": dict(BEND, pivot_pixel=[1, 2])}, {}]}, "object 0: .*\"pivot_pixel\" and the entry a \"pivot\""),
                        ({"objects": [{}, {}], "bend": BEND}, ": .*belongs to one object"),
                        ({"objects": [{"remove": True, "bend": BEND}, {}]}, "object 0")):
        where = _write_scene(tmp_path / "bad", {"t0": entry})
        with pytest.raises(ValueError, match=f"bad: transform 't0'.*{word}"):
            IO.load_scene_geometry(where, 64)


def test_mesh_mode_refuses_a_bend_before_any_device_work(tmp_path):
    from diffusionhandles_amd import depth_transform as DT
    import test_footprints_ref as FP
    depth, bg, masks, _ = _scene(64)
    bend = DT.bend_chain(depth, D.intrinsics_f32(), masks[0], (20, 10), (20, 50), 8.0, 30.0, Z, pivot=_pivot(depth, 20, 32))
    dh = FP._handles("mesh")
    tf = (10.0, Y, Z0)
    common = dict(depth=depth, prompt="p", bg_depth=bg, null_text_emb=None, init_noise=None, activations=[depth])
    with pytest.raises(NotImplementedError, match="transform_foreground_objects: depth_transform_mode 'mesh' has no bend edits \\(Bend"):
        dh.transform_foreground_objects(depth, "p", masks, bg, None, None, None, [bend, tf])
    with pytest.raises(NotImplementedError, match="transform_foreground_objects_batch: depth_transform_mode 'mesh' has no bend edits \\(Bend"):
        dh.transform_foreground_objects_batch(depth, "p", masks, bg, None, None, None, [[tf, tf], [bend, tf]])
    with pytest.raises(NotImplementedError, match="mesh"):
        dh.transform_foregrounds([dict(common, fg_masks=masks, transforms=[bend, tf])])
    # without a Bend the refusal is the one it was
    with pytest.raises(NotImplementedError, match="has no multi-object re-projection"):
        dh.transform_foreground_objects(depth, "p", masks, bg, None, None, None, [tf, tf])
    # the tool: before any identity (prepare_scene reads the scene and builds nothing)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import run_edit
    for n_masks, transforms in ((2, {"t0": {"objects": [{"bend": BEND}, {}]}}), (0, {"t0": {"rotation_angle": 20.0, "bend": BEND}})):
        scene = _write_scene(tmp_path / f"s{n_masks}", transforms, n_masks=n_masks, full=True)
        args = run_edit.parse(["--scene", scene, "--mode", "mesh", "--res", "64"])
        with pytest.raises(NotImplementedError, match="transform 't0' bends an object \\(\"bend\"\\); --mode mesh has no bend edits"):
            run_edit.prepare_scene(args, scene, str(tmp_path / "out"), None)
        args = run_edit.parse(["--scene", scene, "--mode", "pc", "--res", "64"])
        p = run_edit.prepare_scene(args, scene, str(tmp_path / "out"), None)
        tf0 = p["transforms"][0]
        assert (tf0["bends"][0] if n_masks else tf0["bend"])["bones"] == 3
    # resolve_bends: the chain of the member's own motion, on host tensors with an explicit pivot
    dhp = FP._handles("pc")
    dhp.diffuser.get_depth_intrinsics = lambda device=None: D.intrinsics_f32()
    piv = _pivot(depth, 20, 32)
    entry = dict(transforms=[(40.0, torch.tensor(Z), torch.zeros(3), None, piv), tf], bends=[dict(p0=(20.0, 10.0), p1=(20.0, 50.0), width=8.0, bones=3), None])
    out = run_edit.resolve_bends(dhp, entry, depth, masks)
    assert isinstance(out[0], DT.Bend) and len(out[0].bones) == 3 and out[0].bones[2][0] == 40.0 and out[1] == tf
    assert run_edit.resolve_bends(dhp, dict(transforms=[tf, tf]), depth, masks) == [tf, tf]
