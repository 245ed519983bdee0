"""GPU: guided edits of DIFFERENT images in one U-Net batch -- the batched planned energy (dh_energy_fwd_bwd_planned_batch)
against the single call, bit for bit; guided_inference_items against guided_inference_batch (one image, bit-identical) and
against single guided steps (different images, full size); DiffusionHandles.transform_foregrounds; tools/run_edit.py
--edit-batch."""
import copy
import ctypes
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from diffusionhandles_amd.synthetic import TRANSFORMS, make_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y = torch.tensor([0.0, 1.0, 0.0])


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _tf(i):
    return (TRANSFORMS[i][0], Y, torch.tensor(TRANSFORMS[i][1]))


# ---- 3. the batched energy entry, exact ---------------------------------------------------------------------------------
_PLANS = {}


def _plans(grid):
    """16 plans on `grid` from real re-projections of the synthetic scene at 8 * grid pixels: the 8 transforms of
    synthetic.TRANSFORMS and 8 more, with the special items of the issue at fixed places: item 1 has no correspondences
    (n_pairs = 0), item 2 an empty transformed-background list."""
    if grid in _PLANS:
        return _PLANS[grid]
    from diffusionhandles_amd.depth_transform import reproject_edits
    from diffusionhandles_amd.guided_stable_diffuser import GuidedStableDiffuser
    from diffusionhandles_amd.losses import EnergyPlan, ProcessedCorrespondences, process_correspondences
    res = 8 * grid
    depth, bg, mask = make_scene(res)
    tfs = [_tf(i) for i in range(8)] + [(TRANSFORMS[i][0] + 7.0, Y, torch.tensor(TRANSFORMS[i][1]) * 0.5) for i in range(8)]
    edits = reproject_edits(depth.to(dev()), bg.to(dev()), mask.to(dev()), GuidedStableDiffuser.get_depth_intrinsics(), tfs,
                            device_correspondences=True)
    plans = []
    for e, (_, corr) in enumerate(edits):
        if e == 1:
            corr = corr[:0]
        pc = process_correspondences(corr, res, 0, grid=grid, device=dev())
        if e == 2:
            dl = dict(pc.device_lists)
            dl["bg_trans"] = dl["bg_trans"][:0].contiguous()
            pc = ProcessedCorrespondences(pc)
            pc.device_lists = dl
        plans.append(EnergyPlan(pc, grid, dev()))
    assert plans[1].n_pairs == 0 and plans[2].dl["bg_trans"].numel() == 0 and plans[0].n_pairs > 100
    assert len({p.n_pairs for p in plans}) > 8 and len({p.dl["bg_orig"].numel() for p in plans}) > 4        # ragged
    _PLANS[grid] = plans
    return plans


@pytest.mark.parametrize("C,grid", [(640, 64), (320, 64), (320, 96)])
@pytest.mark.parametrize("grad_dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_batched_energy_is_bit_identical_to_single_calls(dtype, grad_dtype, C, grid):
    """dh_energy_fwd_bwd_planned_batch against K calls of dh_energy_fwd_bwd_planned through the C ABI, torch.equal on every
    item's gradient and loss triple, K in {1, 3, 8, 16}; items 1 / 2 / 3 / 4 are the ragged ones (n_pairs = 0, empty
    transformed-background list, fg_w = 0, bg_w = 0); cur / grad are non-adjacent slices of larger buffers; the outputs are
    NaN before both calls."""
    from diffusionhandles_amd import _lib
    L = _lib.lib()
    plans = _plans(grid)
    code, gcode = _lib.DTYPE_CODE[dtype], _lib.DTYPE_CODE[grad_dtype]
    g = torch.Generator(device=dev()).manual_seed(1000 + C + grid)
    for K in (1, 3, 8, 16):
        cur_buf = torch.randn(2 * K + 1, grid, grid, C, generator=g, device=dev()).to(dtype)
        orig = torch.randn(K, grid, grid, C, generator=g, device=dev()).to(dtype)
        cur = [cur_buf[2 * e + 1] for e in range(K)]                     # every other map of the buffer
        fg_w = [0.0 if e == 3 else 7.5 + e for e in range(K)]
        bg_w = [0.0 if e == 4 else 1.5 + 0.25 * e for e in range(K)]
        scale = [256.0 if e % 2 else 64.0 for e in range(K)]
        ref_buf = torch.full((2 * K, grid, grid, C), float("nan"), dtype=grad_dtype, device=dev())
        ref_loss = torch.full((K, 3), float("nan"), device=dev())
        for e in range(K):
            p = plans[e]
            ws, wsb = p.workspace(C)
            _lib.check(L.dh_energy_fwd_bwd_planned(
                _lib.ptr(cur[e]), _lib.ptr(orig[e]), code, C, grid, _lib.ptr(p.buf), p.nbytes, p.n_pairs, _lib.ptr(p.dl["bg_orig"]),
                p.dl["bg_orig"].numel(), _lib.ptr(p.dl["bg_trans"]), p.dl["bg_trans"].numel(), fg_w[e], bg_w[e], scale[e],
                _lib.ptr(ref_loss[e]), _lib.ptr(ref_buf[2 * e]), gcode, _lib.ptr(ws), wsb, _lib.stream_ptr()), "single")
        out_buf = torch.full((2 * K, grid, grid, C), float("nan"), dtype=grad_dtype, device=dev())
        out_loss = torch.full((K, 3), float("nan"), device=dev())
        items = (_lib.EnergyItem * K)()
        for e, it in enumerate(items):
            p = plans[e]
            it.cur, it.orig, it.plan, it.plan_bytes = cur[e].data_ptr(), orig[e].data_ptr(), p.buf.data_ptr(), p.nbytes
            it.bg_orig, it.bg_trans = p.dl["bg_orig"].data_ptr(), p.dl["bg_trans"].data_ptr()
            it.loss_out, it.grad = out_loss[e].data_ptr(), out_buf[2 * e].data_ptr()
            it.n_pairs, it.n_bg_orig, it.n_bg_trans = p.n_pairs, p.dl["bg_orig"].numel(), p.dl["bg_trans"].numel()
            it.fg_w, it.bg_w, it.grad_scale = fg_w[e], bg_w[e], scale[e]
        nb = ctypes.c_size_t()
        _lib.check(L.dh_energy_planned_batch_workspace_bytes(C, grid, K, ctypes.byref(nb)), "workspace bytes")
        ws = torch.empty(nb.value, dtype=torch.uint8, device=dev())
        _lib.check(L.dh_energy_fwd_bwd_planned_batch(items, K, code, C, grid, gcode, _lib.ptr(ws), nb.value, _lib.stream_ptr()), "batch")
        torch.cuda.synchronize()
        for e in range(K):
            assert torch.isfinite(ref_buf[2 * e]).all() and torch.isfinite(ref_loss[e]).all(), (K, e)
            assert torch.equal(out_buf[2 * e], ref_buf[2 * e]), f"K = {K}, item {e}: gradient differs from the single call"
            assert torch.equal(out_loss[e], ref_loss[e]), f"K = {K}, item {e}: loss {out_loss[e].tolist()} != {ref_loss[e].tolist()}"
            assert torch.isnan(out_buf[2 * e + 1]).all()                                   # the maps between the items stay untouched
        if K >= 8:
            assert ref_buf[2].abs().max() > 0 and ref_buf[4].abs().max() > 0                       # ragged items still have a term
            assert ref_loss[1, 1] == 0 and ref_loss[2, 2] == 0
        # and the Python wrapper writes the same gradients (no loss asked: two launches)
        if grad_dtype == dtype:
            from diffusionhandles_amd.losses import energy_and_grad_planned_batch
            outs = [torch.full((grid, grid, C), float("nan"), dtype=dtype, device=dev()) for _ in range(K)]
            loss, grads = energy_and_grad_planned_batch(cur, [orig[e] for e in range(K)], plans[:K], fg_w, bg_w, scale, outs=outs)
            assert loss is None and all(torch.equal(grads[e], ref_buf[2 * e]) for e in range(K))


def test_batched_energy_refuses_more_than_16_items():
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd.losses import energy_and_grad_planned_batch
    L = _lib.lib()
    plans = _plans(64)
    C, grid, K = 320, 64, 17
    nb = ctypes.c_size_t()
    assert L.dh_energy_planned_batch_workspace_bytes(C, grid, K, ctypes.byref(nb)) != 0
    _lib.check(L.dh_energy_planned_batch_workspace_bytes(C, grid, 16, ctypes.byref(nb)))
    ws = torch.empty(2 * nb.value, dtype=torch.uint8, device=dev())
    cur = torch.zeros(K, grid, grid, C, dtype=torch.float16, device=dev())
    grad = torch.full_like(cur, float("nan"))
    items = (_lib.EnergyItem * K)()
    for e, it in enumerate(items):
        p = plans[e % 16]
        it.cur, it.orig, it.plan, it.plan_bytes = cur[e].data_ptr(), cur[e].data_ptr(), p.buf.data_ptr(), p.nbytes
        it.bg_orig, it.bg_trans, it.grad = p.dl["bg_orig"].data_ptr(), p.dl["bg_trans"].data_ptr(), grad[e].data_ptr()
        it.n_pairs, it.n_bg_orig, it.n_bg_trans = p.n_pairs, p.dl["bg_orig"].numel(), p.dl["bg_trans"].numel()
        it.fg_w, it.bg_w, it.grad_scale = 1.0, 1.0, 1.0
    rc = L.dh_energy_fwd_bwd_planned_batch(items, K, 0, C, grid, 0, _lib.ptr(ws), 2 * nb.value, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and b"16" in L.dh_last_error()
    assert torch.isnan(grad).all()                      # refused as a whole, nothing was launched
    with pytest.raises(ValueError):
        energy_and_grad_planned_batch([cur[e] for e in range(K)], [cur[e] for e in range(K)], [plans[e % 16] for e in range(K)],
                                      [1.0] * K, [1.0] * K, [1.0] * K)


# ---- the TINY rig (that of tests/test_loops_gpu.py, with two images) ------------------------------------------------------
def _tiny_handles(ref, max_batch):
    from diffusionhandles_amd import DiffusionHandles
    from diffusionhandles_amd import conf as C
    from diffusionhandles_amd.unet import HipUNet
    from oracle import unet_torch as U
    hip = HipUNet(dict(U.TINY, text_len=77), dtype=torch.float16, max_batch=max_batch)
    hip.load_state_dict(ref.state_dict())
    return DiffusionHandles(C.load_default(), unet=hip, unet_config=dict(U.TINY, text_len=77)).to(dev())


def _two_images(dh, res=512):
    """Two synthetic images (the sphere scene and its mirror image, with different prompts) and their identities
    (initial inference from noise, no inversion) by the product."""
    depth, bg, mask = (t.to(dev()) for t in make_scene(res))
    imgs = []
    for i, (prompt, flip) in enumerate((("a sphere on a plane", False), ("a red ball on a wooden table", True))):
        d, b, m = (t.flip(-1).contiguous() if flip else t for t in (depth, bg, mask))
        g = torch.Generator().manual_seed(11 + i)
        noise = torch.randn(1, 4, res // 8, res // 8, generator=g).to(dev())
        D = dh.diffuser.unet.cfg["cross_attention_dim"]
        unc = (dh.diffuser._encode([""])[None].expand(50, -1, -1, -1) + 0.05 * torch.randn(50, 1, 77, D, generator=g).to(dev())).contiguous()
        null_text, noise, acts, latent = dh.generate_input_image(d, prompt, unc, noise)
        imgs.append(SimpleNamespace(depth=d, bg_depth=dh.set_foreground(d, m, b), fg_mask=m, prompt=prompt, null_text=null_text,
                                    noise=noise, acts=acts))
    return imgs


@pytest.fixture(scope="module")
def tiny():
    from oracle import unet_torch as U
    ref = U.init_synthetic_(U.UNetTorch(U.TINY), seed=0).to(dev()).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.half().float())
    dh = _tiny_handles(ref, 6)
    return SimpleNamespace(ref=ref, dh=dh, gd=dh.diffuser, imgs=_two_images(dh))


# ---- 4. one image: the items path is the batch path ----------------------------------------------------------------------
@pytest.mark.parametrize("grad_scale", ["static", "auto"])
def test_items_of_one_image_are_bit_identical_to_the_one_image_batch(tiny, grad_scale):
    """K = 3 items that are three transforms of ONE image: guided_inference_items runs the passes and kernels of
    guided_inference_batch (the stacked prompt rows are K copies of one row), so the latents are bit-identical."""
    from diffusionhandles_amd.depth_transform import reproject_edits
    gd, im = tiny.gd, tiny.imgs[0]
    edits = reproject_edits(im.depth, im.bg_depth, im.fg_mask, gd.get_depth_intrinsics(), [_tf(i) for i in (2, 4, 6)],
                            device_correspondences=True)
    old = gd.grad_scale_mode
    gd.grad_scale_mode = grad_scale
    try:
        img_b = gd.guided_inference_batch(im.noise, [d for d, _ in edits], im.null_text, im.prompt, im.acts, [c for _, c in edits]).clone()
        lat_b = gd.last_latents.clone()
        img_i = gd.guided_inference_items([(im.noise, d, im.null_text, im.prompt, im.acts, c) for d, c in edits])
        lat_i = gd.last_latents
    finally:
        gd.grad_scale_mode = old
    assert lat_i.shape == (3, 4, 64, 64) and img_i.shape == (3, 3, 512, 512)
    assert torch.isfinite(lat_b).all() and rel(lat_b[0], lat_b[1]) > 1e-2
    assert torch.equal(lat_i, lat_b) and torch.equal(img_i, img_b)


# ---- 6. the public entry --------------------------------------------------------------------------------------------------
def _edit(im, i, **kw):
    a, ax, tr = _tf(i)
    return dict(depth=im.depth, prompt=im.prompt, fg_mask=im.fg_mask, bg_depth=im.bg_depth, null_text_emb=im.null_text,
                init_noise=im.noise, activations=im.acts, rot_angle=a, rot_axis=ax, translation=tr, **kw)


def test_transform_foregrounds_on_two_images(tiny):
    """Edits of two images, interleaved: results in input order, bitwise equal to guided_inference_items on the same
    re-projections (made here per image, as transform_foreground_batch makes them); the contract errors."""
    from diffusionhandles_amd.depth_transform import reproject_edits
    dh, gd = tiny.dh, tiny.gd
    a, b = tiny.imgs
    order = [(a, 2), (b, 5), (a, 6)]
    images, disps = dh.transform_foregrounds([_edit(im, i) for im, i in order])
    lat = gd.last_latents.clone()
    assert images.shape == (3, 3, 512, 512) and len(disps) == 3 and torch.isfinite(images).all()
    K = gd.get_depth_intrinsics()
    ra = reproject_edits(a.depth, a.bg_depth, a.fg_mask, K, [_tf(2), _tf(6)], device_correspondences=True)
    rb = reproject_edits(b.depth, b.bg_depth, b.fg_mask, K, [_tf(5)], device_correspondences=True)
    rp = [ra[0], rb[0], ra[1]]
    for (d, _), got in zip(rp, disps):
        assert torch.equal(d, got)
    items = [dict(latents=im.noise, depth=d, uncond_embeddings=im.null_text, prompt=im.prompt, activations_orig=im.acts,
                  correspondences=c) for (im, _), (d, c) in zip(order, rp)]
    ref = gd.guided_inference_items(items)
    assert torch.equal(gd.last_latents, lat) and torch.equal(ref, images)
    # input order: the same edits in another order give the same results, permuted
    images2, _ = dh.transform_foregrounds([_edit(im, i) for im, i in (order[1], order[0], order[2])])
    assert rel(images2[0], images[1]) < 5e-2 and rel(images2[1], images[0]) < 5e-2 and rel(images[0], images[1]) > 0.1
    # per-edit weights reach their item
    images3, _ = dh.transform_foregrounds([_edit(a, 2), _edit(b, 5, fg_weight=0.0, bg_weight=0.0), _edit(a, 6)])
    assert not torch.equal(images3[1], images[1])
    # the contract
    small = _tiny_handles(tiny.ref, 4)
    with pytest.raises(RuntimeError):
        small.transform_foregrounds([_edit(im, i) for im, i in order])
    half = SimpleNamespace(**{**vars(b), "depth": b.depth[..., ::2, ::2].contiguous(), "bg_depth": b.bg_depth[..., ::2, ::2].contiguous(),
                              "fg_mask": b.fg_mask[..., ::2, ::2].contiguous()})
    with pytest.raises(ValueError):
        dh.transform_foregrounds([_edit(a, 2), _edit(half, 5)])
    dh.conf.depth_transform_mode = "mesh"
    try:
        with pytest.raises(NotImplementedError):
            dh.transform_foregrounds([_edit(a, 2), _edit(b, 5)])
    finally:
        dh.conf.depth_transform_mode = "pc"


# ---- 5. different images at the full size, against single steps -----------------------------------------------------------
def test_guided_step_items_full_size_matches_single_steps():
    """Full-size engine (SD2-depth shape, seeded 16-bit-representable weights, max_batch 16, the rig of
    tests/test_full_size_loop_gpu.py), K = 4 items from two synthetic images x two transforms with different prompts, depths,
    start latents, per-timestep unconditional embeddings and original activations (two initial inferences by the product).
    guided_step_items against four guided_step calls from the same per-item inputs at t_idx 0, 1, 2 (the three layer phases)
    and guidance_max_step, teacher-forced from the single results: post-step latent rel-L2 <= 5e-3 per item (the gate of
    test_guided_step_batch8_full_size_matches_single_steps; the cause of the difference, batch-dependent tile selection, is the
    same).  The items differ from each other by > 10 x that error, and swapping two items' prompts, or their original
    activations, moves the result by more than the gate.
    Measured on an MI355X: worst 8.9e-4 (t_idx 0 / 1 / 2: 8.9e-4 / 7.3e-4 / 6.2e-4, unguided t_idx 38: 2.2e-4); the prompt swap
    moves the two items by 7.9e-2, the activation swap by 2.4e-2."""
    from diffusionhandles_amd import DiffusionHandles
    from diffusionhandles_amd import conf as C
    from diffusionhandles_amd.depth_transform import reproject_edits
    from diffusionhandles_amd.unet import HipUNet
    from oracle import unet_torch as U
    cfg = dict(U.SD2_DEPTH, sample_size=64)
    ref = U.init_synthetic_(U.UNetTorch(cfg), seed=0).to(dev()).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.half().float())
    hip = HipUNet(dict(cfg, text_len=77), dtype=torch.float16, max_batch=16)
    hip.load_state_dict(ref.state_dict())
    del ref
    torch.cuda.empty_cache()
    dh = DiffusionHandles(C.load_default(), unet=hip, unet_config=dict(cfg, text_len=77)).to(dev())
    gd = dh.diffuser
    imgs = _two_images(dh)
    assert imgs[0].acts[1].shape == (50, 640, 64, 64) and rel(imgs[0].acts[1][0], imgs[1].acts[1][0]) > 0.1
    gmax = gd.conf.guidance_max_step
    GATE = 5e-3
    worst = 0.0
    with torch.no_grad(), gd.on_stream():
        gd.scheduler.set_timesteps(50)
        ts = gd.scheduler.timesteps
        which, sts = [], []
        for im, pair in zip(imgs, ((2, 6), (5, 7))):
            edits = reproject_edits(im.depth, im.bg_depth, im.fg_mask, gd.get_depth_intrinsics(), [_tf(i) for i in pair],
                                    device_correspondences=True)
            for d, c in edits:
                sts.append(gd.prepare_guidance(d, im.prompt, im.acts, c, orig=sts[-1].orig if which and which[-1] is im else None))
                which.append(im)
        K = len(sts)
        assert K == 4 and all(st.plan is not None and st.n_pairs > 1000 for st in sts) and sts[0].orig is sts[1].orig
        g = torch.Generator(device=dev()).manual_seed(77)
        xb = torch.cat([im.noise.permute(0, 2, 3, 1) + 0.05 * torch.randn(1, 64, 64, 4, generator=g, device=dev()) for im in which]).contiguous()

        def uncs(i):
            return torch.cat([im.null_text[i].reshape(1, 77, -1) for im in which]).float().contiguous()
        for i in (0, 1, 2, gmax):
            singles = torch.cat([gd.guided_step(sts[e], xb[e:e + 1].contiguous(), i, ts[i], which[e].null_text[i]).clone() for e in range(K)])
            batched = gd.guided_step_items(sts, xb, i, ts[i], uncs(i)).clone()
            assert batched.shape == singles.shape == (K, 64, 64, 4) and torch.isfinite(batched).all()
            errs = [rel(batched[e], singles[e]) for e in range(K)]
            print(f"t_idx {i}: items vs single steps, post-step latent rel-L2 per item {['%.2e' % v for v in errs]}")
            worst = max(worst, max(errs))
            assert max(errs) <= GATE, f"t_idx {i}: items vs single post-step latent rel-L2 per item {['%.2e' % v for v in errs]} (gate 5e-3)"
            apart = min(rel(singles[a], singles[b]) for a in range(K) for b in range(K) if a != b)
            assert apart > 10 * max(errs), (i, apart, errs)
            if i == 0:
                # a mixed-up item index cannot pass: items 0 and 2 (different images) with their prompts swapped ...
                sw = [copy.copy(st) for st in sts]
                for st in sw:
                    st.__dict__.pop("_items_cond", None)
                sw[0].cond, sw[2].cond = sts[2].cond, sts[0].cond
                moved = gd.guided_step_items(sw, xb, i, ts[i], uncs(i)).clone()
                mp = min(rel(moved[0], singles[0]), rel(moved[2], singles[2]))
                # ... and, separately, with their original activations swapped
                sw = [copy.copy(st) for st in sts]
                for st in sw:
                    st.__dict__.pop("_items_cond", None)
                sw[0].orig, sw[2].orig = sts[2].orig, sts[0].orig
                moved = gd.guided_step_items(sw, xb, i, ts[i], uncs(i)).clone()
                ma = min(rel(moved[0], singles[0]), rel(moved[2], singles[2]))
                print(f"t_idx 0: prompts of items 0 / 2 swapped moves them by {mp:.2e}, original activations swapped by {ma:.2e} (gate {GATE:.0e})")
                assert mp > GATE and ma > GATE, (mp, ma)
                assert max(rel(moved[1], singles[1]), rel(moved[3], singles[3])) <= GATE           # the other items do not move
            xb = singles
    print(f"K = 4 items of two images, full size: worst post-step latent rel-L2 against single steps {worst:.3e} (gate 5e-3)")


# ---- 7. the harness ---------------------------------------------------------------------------------------------------------
def test_run_edit_test_set_with_edit_batch(tmp_path):
    """tools/run_edit.py --test-set over the two complete scene fixtures with --edit-batch 4: the file set of --edit-batch 1,
    and byte-identical PNGs when run twice.  (Against --edit-batch 1 the images differ in the last fp16 bits.)"""
    gold = os.path.join(ROOT, "tests", "golden")
    inp = tmp_path / "set"
    inp.mkdir()
    os.symlink(os.path.join(gold, "scene_dice"), inp / "dice")
    os.symlink(os.path.join(gold, "scene_banana_fruits"), inp / "banana_fruits")
    (inp / "two.json").write_text(json.dumps({"dice": ["edit_000", "edit_001"], "banana_fruits": ["edit_000", "edit_001", "edit_002"]}))

    def run(out, *extra):
        cmd = [sys.executable, os.path.join(ROOT, "tools", "run_edit.py"), "--test-set", str(inp / "two.json"), "--input-dir", str(inp),
               "--out", str(out), "--skip-inversion", "--no-identity-cache", *extra]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stderr[-3000:]
        files = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
        return json.loads(r.stdout.strip().splitlines()[-1]), files

    rep1, files1 = run(tmp_path / "b1")
    rep4, files4 = run(tmp_path / "b4", "--edit-batch", "4")
    assert files4 == files1 and "dice/edit_001.png" in files4 and "banana_fruits/edit_002_disparity.png" in files4
    assert rep1["edits_run"] == rep4["edits_run"] == 5 and "edit_batch" not in rep1
    assert rep4["edit_batch"] == 4 and len(rep4["batch_seconds"]) == 2                    # 5 edits: a batch of 4 and one of 1
    assert [s["scene"] for s in rep4["scenes"]] == ["dice", "banana_fruits"]
    assert [e["name"] for e in rep4["scenes"][1]["edits"]] == ["edit_000", "edit_001", "edit_002"]
    _, files4b = run(tmp_path / "b4b", "--edit-batch", "4")
    assert files4b == files4
    pngs = [f for f in files4 if f.endswith(".png")]
    assert len(pngs) >= 20
    for f in pngs:
        assert open(tmp_path / "b4" / f, "rb").read() == open(tmp_path / "b4b" / f, "rb").read(), f
    # --skip-existing removes finished edits before packing
    os.remove(tmp_path / "b4" / "banana_fruits" / "edit_001.png")
    rep, _ = run(tmp_path / "b4", "--edit-batch", "4", "--skip-existing")
    assert rep["edits_run"] == 1 and rep["edits_skipped"] == 4 and len(rep["batch_seconds"]) == 1
    assert os.path.exists(tmp_path / "b4" / "banana_fruits" / "edit_001.png")
