"""GPU: multi-object edits in mixed-image batches, on lanes and from scene directories -- guided_inference_items with
object_labels / object_weights against guided_inference_batch (one image, bit-identical); a batch that mixes weighted and
unweighted items through the one-launch mixed energy against the item-by-item route (bit-identical);
DiffusionHandles.transform_foregrounds with single- and multi-object edits; transform_foreground_objects_batch on lanes;
tools/run_edit.run_scene on a multi-object scene directory.  The TINY rig of tests/test_edit_items_gpu.py (max_batch 6, 512
pixels, identities from noise); the two images are the two-sphere image of tests/multi_object_ref.py and the mirrored
one-sphere image of synthetic.make_scene."""
import argparse
import importlib.util
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_object_ref as R  # noqa: E402
import object_weights_ref as W  # noqa: E402

from diffusionhandles_amd.synthetic import TRANSFORMS, make_scene  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y = torch.tensor([0.0, 1.0, 0.0])
RES = 512


def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _t(tf):
    a, ax, tr = tf
    return (float(a), torch.tensor(ax, dtype=torch.float32), torch.tensor(tr, dtype=torch.float32))


OCCLUDING = [_t(tf) for tf in R.OCCLUDING]
APART = [_t(tf) for tf in W.EDITS["apart"]]
SINGLE = (TRANSFORMS[5][0], Y, torch.tensor(TRANSFORMS[5][1]))


def _tiny_handles(ref, max_batch):
    from diffusionhandles_amd import DiffusionHandles
    from diffusionhandles_amd import conf as C
    from diffusionhandles_amd.unet import HipUNet
    from oracle import unet_torch as U
    hip = HipUNet(dict(U.TINY, text_len=77), dtype=torch.float16, max_batch=max_batch)
    hip.load_state_dict(ref.state_dict())
    return DiffusionHandles(C.load_default(), unet=hip, unet_config=dict(U.TINY, text_len=77)).to(dev())


def _identity(dh, depth, prompt, seed):
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(1, 4, RES // 8, RES // 8, generator=g).to(dev())
    D = dh.diffuser.unet.cfg["cross_attention_dim"]
    unc = (dh.diffuser._encode([""])[None].expand(50, -1, -1, -1) + 0.05 * torch.randn(50, 1, 77, D, generator=g).to(dev())).contiguous()
    null_text, noise, acts, _ = dh.generate_input_image(depth, prompt, unc, noise)
    return dict(null_text=null_text, noise=noise, acts=acts, prompt=prompt)


@pytest.fixture(scope="module")
def tiny():
    from diffusionhandles_amd.losses import object_label_image
    from oracle import unet_torch as U
    ref = U.init_synthetic_(U.UNetTorch(U.TINY), seed=0).to(dev()).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.half().float())
    dh = _tiny_handles(ref, 6)
    depth, bg, masks = R.two_spheres(RES)
    depth, bg, masks = depth.to(dev()), bg.to(dev()), [m.to(dev()) for m in masks]
    two = SimpleNamespace(depth=depth, bg_depth=dh.set_foreground(depth, masks, bg), masks=masks, labels=object_label_image(masks),
                          **_identity(dh, depth, "two spheres on a plane", 11))
    d1, b1, m1 = (t.to(dev()).flip(-1).contiguous() for t in make_scene(RES))
    one = SimpleNamespace(depth=d1, bg_depth=dh.set_foreground(d1, m1, b1), fg_mask=m1, **_identity(dh, d1, "a red ball on a wooden table", 12))
    return SimpleNamespace(ref=ref, dh=dh, gd=dh.diffuser, two=two, one=one)


def _reproject_two(tiny, edits):
    from diffusionhandles_amd.depth_transform import reproject_object_edits
    t = tiny.two
    return reproject_object_edits(t.depth, t.bg_depth, t.masks, tiny.gd.get_depth_intrinsics(device=dev()), edits,
                                  device_correspondences=True)


def _reproject_one(tiny, tfs):
    from diffusionhandles_amd.depth_transform import reproject_edits
    o = tiny.one
    return reproject_edits(o.depth, o.bg_depth, o.fg_mask, tiny.gd.get_depth_intrinsics(), tfs, device_correspondences=True)


def _item(im, d, c, **kw):
    return dict(latents=im.noise, depth=d, uncond_embeddings=im.null_text, prompt=im.prompt, activations_orig=im.acts,
                correspondences=c, **kw)


# ---- items of one image are the one-image batch -----------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["equal", None])
def test_object_items_of_one_image_are_bit_identical_to_the_one_image_batch(tiny, weights):
    gd, t = tiny.gd, tiny.two
    rp = _reproject_two(tiny, [OCCLUDING, APART])
    obj = dict(object_labels=t.labels, object_weights=weights)
    img_b = gd.guided_inference_batch(t.noise, [d for d, _ in rp], t.null_text, t.prompt, t.acts, [c for _, c in rp], **obj).clone()
    lat_b = gd.last_latents.clone()
    img_i = gd.guided_inference_items([_item(t, d, c, **obj) for d, c in rp])
    lat_i = gd.last_latents
    assert lat_i.shape == (2, 4, 64, 64) and torch.isfinite(lat_b).all()
    assert torch.equal(lat_i, lat_b) and torch.equal(img_i, img_b)


# ---- a batch that mixes weighted and unweighted items ---------------------------------------------------------------------
@pytest.mark.parametrize("grad_scale", ["static", "auto"])
def test_mixed_batch_takes_one_launch_and_equals_item_by_item(tiny, grad_scale, monkeypatch):
    from diffusionhandles_amd import losses
    gd, t, o = tiny.gd, tiny.two, tiny.one
    rp = _reproject_two(tiny, [OCCLUDING, APART])
    (d1, c1), = _reproject_one(tiny, [SINGLE])
    items = lambda w: [_item(t, *rp[0], object_labels=t.labels, object_weights=w), _item(o, d1, c1), _item(t, *rp[1])]
    calls = []
    real = losses.energy_and_grad_planned_mixed

    def counted(*a, **kw):
        calls.append(len(a[0]))
        return real(*a, **kw)
    monkeypatch.setattr(losses, "energy_and_grad_planned_mixed", counted)
    old = gd.grad_scale_mode, gd._batch_energy
    gd.grad_scale_mode = grad_scale
    try:
        assert gd._batch_energy
        gd.guided_inference_items(items("equal"))
        lat_mixed, n_mixed = gd.last_latents.clone(), len(calls)
        gd._batch_energy = False
        gd.guided_inference_items(items("equal"))
        lat_single, n_single = gd.last_latents.clone(), len(calls) - n_mixed
        gd._batch_energy = True
        gd.guided_inference_items(items(None))
        lat_plain, n_plain = gd.last_latents.clone(), len(calls) - n_mixed - n_single
    finally:
        gd.grad_scale_mode, gd._batch_energy = old
    print(f"{grad_scale}: {n_mixed} mixed energy calls, {n_single} with the switch off, {n_plain} for the all-unweighted batch")
    assert n_mixed > 0 and set(calls[:n_mixed]) == {3} and n_single == 0 and n_plain == 0
    assert torch.isfinite(lat_mixed).all() and torch.equal(lat_mixed, lat_single)
    assert not torch.equal(lat_mixed[0], lat_plain[0]) and float((lat_mixed[0] - lat_plain[0]).abs().max()) > 1e-4


# ---- the public entry ---------------------------------------------------------------------------------------------------------
def _edits(tiny):
    t, o = tiny.two, tiny.one
    common = lambda im: dict(depth=im.depth, prompt=im.prompt, bg_depth=im.bg_depth, null_text_emb=im.null_text, init_noise=im.noise,
                             activations=im.acts)
    return [dict(common(t), fg_masks=t.masks, transforms=OCCLUDING, object_weights="equal"),
            dict(common(o), fg_mask=o.fg_mask, rot_angle=SINGLE[0], rot_axis=SINGLE[1], translation=SINGLE[2]),
            dict(common(t), fg_masks=t.masks, transforms=[APART[0], (None, None, APART[1][2])])]


def test_transform_foregrounds_with_single_and_multi_object_edits(tiny):
    dh, gd, t, o = tiny.dh, tiny.gd, tiny.two, tiny.one
    edits = _edits(tiny)
    images, disps = dh.transform_foregrounds(edits)
    images, lat = images.clone(), gd.last_latents.clone()
    assert images.shape == (3, 3, 512, 512) and len(disps) == 3 and torch.isfinite(images).all()
    # the re-projections, per group as transform_foregrounds groups them (the None members take the defaults)
    rp2 = _reproject_two(tiny, [OCCLUDING, [APART[0], (0.0, Y, APART[1][2])]])
    (r1,) = _reproject_one(tiny, [SINGLE])
    rp = [rp2[0], r1, rp2[1]]
    for (d, _), got in zip(rp, disps):
        assert torch.equal(d, got)
    ref = gd.guided_inference_items([_item(t, *rp[0], object_labels=t.labels, object_weights="equal"), _item(o, *rp[1]), _item(t, *rp[2])])
    assert torch.equal(gd.last_latents, lat) and torch.equal(ref, images)
    # the weights reached their item: without them edit 0 comes out differently, the others do not move
    plain, _ = dh.transform_foregrounds([{k: v for k, v in edits[0].items() if k != "object_weights"}, edits[1], edits[2]])
    assert not torch.equal(plain[0], images[0])


def test_transform_foregrounds_refuses_malformed_edits_before_any_device_work(tiny):
    """On an engine too small for three edits: a well-formed batch reaches the engine check (RuntimeError), a malformed edit is
    refused before it (ValueError naming the edit)."""
    small = _tiny_handles(tiny.ref, 4)
    e = _edits(tiny)
    with pytest.raises(RuntimeError):
        small.transform_foregrounds(e)
    both = dict(e[0], fg_mask=tiny.one.fg_mask)
    both2 = dict(e[1], transforms=OCCLUDING)
    neither = {k: v for k, v in e[1].items() if k != "fg_mask"}
    short = dict(e[0], transforms=OCCLUDING[:1])
    none = {k: v for k, v in e[2].items() if k != "transforms"}
    badw = dict(e[0], object_weights=[1.0, 2.0, 3.0])
    for i, bad in ((0, both), (1, both2), (1, neither), (2, short), (2, none), (0, badw)):
        batch = list(e)
        batch[i] = bad
        with pytest.raises(ValueError, match=f"edit {i}"):
            small.transform_foregrounds(batch)
    small.diffuser.unet.close()


# ---- lanes ----------------------------------------------------------------------------------------------------------------------
def test_object_batch_on_lanes_is_bit_identical_to_one_stream(tiny):
    dh, gd, t = tiny.dh, tiny.gd, tiny.two
    edits = [OCCLUDING, APART, [_t((15.0, R.Y, (-0.3, 0.0, 0.0))), _t((0.0, R.Y, (0.1, 0.0, 0.0)))],
             [_t((-20.0, R.Y, (0.0, 0.0, 0.1))), _t((25.0, R.Y, (0.05, 0.0, 0.0)))]]
    args = dict(depth=t.depth, prompt=t.prompt, fg_masks=t.masks, bg_depth=t.bg_depth, null_text_emb=t.null_text, init_noise=t.noise,
                activations=t.acts, edits=edits, object_weights="equal")
    try:
        lanes = {}
        for batch in (2, 1):
            one, d_one = dh.transform_foreground_objects_batch(**args, streams=1, batch=batch)
            one = one.clone()
            two, d_two = dh.transform_foreground_objects_batch(**args, streams=2, batch=batch)
            lanes[batch] = two.clone()
            assert one.shape == (4, 3, 512, 512) and torch.isfinite(one).all()
            assert torch.equal(two, one), f"batch = {batch}: two lanes differ from one stream"
            assert all(torch.equal(a, b) for a, b in zip(d_one, d_two))
            assert not torch.equal(one[0], one[1])
        # the weights reach the lanes: without them the first edit comes out differently (the first chunk / the first two edits alone)
        for batch in (2, 1):
            plain, _ = dh.transform_foreground_objects_batch(**{**args, "object_weights": None, "edits": edits[:2]}, streams=2, batch=batch)
            assert not torch.equal(plain[0], lanes[batch][0]), f"batch = {batch}"
    finally:
        gd.release_lanes()


# ---- the harness on a multi-object scene directory --------------------------------------------------------------------------
def _run_edit_module():
    spec = importlib.util.spec_from_file_location("run_edit_tool", os.path.join(ROOT, "tools", "run_edit.py"))
    run_edit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run_edit)
    return run_edit


def _write_scene(scene):
    """The two-sphere scene as a scene directory: two masks, entries `plain` and `equal` of the OCCLUDING edit."""
    from diffusionhandles_amd.scene_io import write_png
    depth, bg, masks = R.two_spheres(RES)
    scene.mkdir()
    np.save(scene / "depth.npy", depth[0, 0].numpy())
    np.save(scene / "bg_depth.npy", bg[0, 0].numpy())
    for m, mask in enumerate(masks):
        write_png(str(scene / f"mask_{m}.png"), mask[0, 0].numpy())
    write_png(str(scene / "input.png"), np.full((RES, RES, 3), 0.5, dtype=np.float32))
    (scene / "prompt.txt").write_text("two spheres on a plane\n")
    objects = [dict(rotation_angle=a, rotation_axis=list(ax), translation=list(tr)) for a, ax, tr in R.OCCLUDING]
    (scene / "transforms.json").write_text(json.dumps({"plain": {"objects": objects},
                                                       "equal": {"objects": objects, "object_weights": "equal"}}))


def _args(**kw):
    return argparse.Namespace(**{**dict(res=RES, mode="pc", skip_inversion=True, no_identity_cache=True, identity_cache=None,
                                        skip_existing=False, max_edits=0, identity_batch=1, edit_batch=1, edit_batch_images=0), **kw})


def test_run_scene_on_a_multi_object_scene_directory(tiny, tmp_path):
    from diffusionhandles_amd.scene_io import read_png
    run_edit = _run_edit_module()
    scene = tmp_path / "two_spheres"
    _write_scene(scene)
    args = _args()
    out = tmp_path / "out"
    report = run_edit.run_scene(args, tiny.dh.conf, lambda res: tiny.dh, str(scene), str(out), None)
    assert [e["name"] for e in report["edits"]] == ["plain", "equal"] and report["mode"] == "pc"
    imgs = {}
    for name in ("plain", "equal"):
        imgs[name] = read_png(str(out / f"{name}.png"))
        disp = read_png(str(out / f"{name}_disparity.png"))
        assert imgs[name].shape == (RES, RES, 3) and disp.shape == (RES, RES)
        assert np.isfinite(imgs[name].astype(np.float64)).all() and imgs[name].std() > 0 and disp.std() > 0
    assert (imgs["plain"] != imgs["equal"]).any()                       # the weights of the entry reached the energy
    assert os.path.exists(out / "report.json") and os.path.exists(out / "recon.png")
    # mesh mode has no multi-object re-projection: refused before the identity
    args.mode = "mesh"
    with pytest.raises(NotImplementedError, match="multi-object"):
        run_edit.run_scene(args, tiny.dh.conf, lambda res: pytest.fail("the engine was asked for"), str(scene), str(tmp_path / "mesh"), None)


def test_edit_batches_pack_multi_object_scenes_with_single_object_scenes(tiny, tmp_path):
    """run_edit.py --test-set --edit-batch 3 over the two-sphere scene directory (two entries, one weighted) and a single-mask
    scene directory of the synthetic sphere: one transform_foregrounds batch, the files of the unbatched run."""
    from diffusionhandles_amd.scene_io import read_png
    run_edit = _run_edit_module()
    inp = tmp_path / "set"
    inp.mkdir()
    _write_scene(inp / "two_spheres")
    from diffusionhandles_amd.scene_io import write_png
    depth, bg, mask = make_scene(RES)
    (inp / "sphere").mkdir()
    np.save(inp / "sphere" / "depth.npy", depth[0, 0].numpy())
    np.save(inp / "sphere" / "bg_depth.npy", bg[0, 0].numpy())
    write_png(str(inp / "sphere" / "mask.png"), mask[0, 0].float().numpy())
    write_png(str(inp / "sphere" / "input.png"), np.full((RES, RES, 3), 0.5, dtype=np.float32))
    (inp / "sphere" / "prompt.txt").write_text("a sphere on a plane\n")
    (inp / "sphere" / "transforms.json").write_text(json.dumps({"edit_000": {"rotation_angle": float(TRANSFORMS[2][0]),
                                                                             "translation": [float(v) for v in TRANSFORMS[2][1]]}}))
    args = _args(edit_batch=3, out=str(tmp_path / "out"))
    names = [("two_spheres", ["plain", "equal"]), ("sphere", ["edit_000"])]
    reports, seconds = run_edit.run_test_set_batched(args, tiny.dh.conf, lambda res: tiny.dh, names, str(inp))
    assert len(seconds) == 1 and [r["scene"] for r in reports] == ["two_spheres", "sphere"]
    assert [e["name"] for e in reports[0]["edits"]] == ["plain", "equal"] and [e["name"] for e in reports[1]["edits"]] == ["edit_000"]
    imgs = {}
    for scene, name in (("two_spheres", "plain"), ("two_spheres", "equal"), ("sphere", "edit_000")):
        imgs[name] = read_png(str(tmp_path / "out" / scene / f"{name}.png"))
        disp = read_png(str(tmp_path / "out" / scene / f"{name}_disparity.png"))
        assert imgs[name].shape == (RES, RES, 3) and imgs[name].std() > 0 and disp.std() > 0
    assert (imgs["plain"] != imgs["equal"]).any()
    assert os.path.exists(tmp_path / "out" / "two_spheres" / "summary.html") and os.path.exists(tmp_path / "out" / "sphere" / "report.json")

