"""The 'auto' guidance scale on the GPU (TINY rig of tests/test_loops_gpu.py): the guarded latent update and the flagged DDIM
step through the C ABI, parity with the fp32 oracle, invariance of the unscaled gradient under power-of-two weights, the
FloatingPointError of an overflowing edit, and batches / lanes."""
import contextlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from diffusionhandles_amd.synthetic import TRANSFORMS, make_scene

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@contextlib.contextmanager
def mode(gd, m):
    old = gd.grad_scale_mode
    gd.grad_scale_mode = m
    try:
        yield gd
    finally:
        gd.grad_scale_mode = old


def _engine(ref, max_batch=2, scale_conv_in=None):
    from diffusionhandles_amd.unet import HipUNet
    from oracle import unet_torch as U
    hip = HipUNet(dict(U.TINY, text_len=77), dtype=torch.float16, max_batch=max_batch)
    sd = ref.state_dict()
    if scale_conv_in is not None:
        sd = dict(sd)
        sd["conv_in.weight"] = sd["conv_in.weight"] * scale_conv_in
    hip.load_state_dict(sd)
    return hip


@pytest.fixture(scope="module")
def rig():
    from diffusionhandles_amd import conf as C
    from diffusionhandles_amd.depth_transform import reproject_edits
    from diffusionhandles_amd.guided_stable_diffuser import GuidedStableDiffuser
    from oracle import depth_ref as D
    from oracle import loop_ref as L
    from oracle import unet_torch as U
    ref = U.init_synthetic_(U.UNetTorch(U.TINY), seed=0).to(dev()).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.half().float())
    conf = C.load_default().guided_diffuser
    gd = GuidedStableDiffuser(conf, unet=_engine(ref), unet_config=dict(U.TINY, text_len=77)).to(dev())
    depth, bg, mask = make_scene(512)
    disp = D.normalize_depth(1.0 / depth)[0]
    prompt = "a sphere on a plane"
    cond = gd._encode([prompt])
    unc = gd._encode([""])[None].expand(50, -1, -1, -1).contiguous()
    noise = torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(5)).to(dev())
    acts, _, _, _ = L.initial_inference(ref, L.DDIM(), noise, disp.to(dev()), unc, cond)
    acts = [a.float() for a in acts]
    Kint = gd.get_depth_intrinsics()
    tfs = [(TRANSFORMS[i][0], torch.tensor([0.0, 1.0, 0.0]), torch.tensor(TRANSFORMS[i][1])) for i in (2, 3, 4)]
    edits = reproject_edits(depth.to(dev()), bg.to(dev()), mask.to(dev()), Kint, tfs)
    return SimpleNamespace(ref=ref, gd=gd, conf=conf, prompt=prompt, cond=cond, unc=unc, noise=noise, acts=acts, edits=edits,
                           disp=disp)


def _guarded(x, g, gc, table, T, I, t_idx, it, status):
    from diffusionhandles_amd import _lib
    out = torch.full_like(x, float("nan"))
    K = x.shape[0]
    _lib.check(_lib.lib().dh_latent_update_guarded(_lib.ptr(out), _lib.ptr(x), _lib.ptr(g), gc, 4, 0.1, x[0].numel() // 4, K,
                                                   _lib.ptr(table), T * I, t_idx * I + it, _lib.ptr(status), None, t_idx, it,
                                                   _lib.stream_ptr()), "dh_latent_update_guarded")
    return out


@pytest.mark.parametrize("hw", [64, 96])
def test_guarded_update_through_c_abi(hw):
    from diffusionhandles_amd import _lib
    g = torch.Generator(device=dev()).manual_seed(11)
    K = 3
    x = torch.randn(K, hw, hw, 4, generator=g, device=dev())
    d = torch.randn(K, hw, hw, 5, generator=g, device=dev()) * 300.0
    d[1, hw // 3, hw // 2, 2] = float("inf")
    d[0, 0, 0, 4] = float("nan")                       # the depth channel is not read
    T, I = 5, 3
    table = torch.full((K, T, I), 256.0, device=dev())
    status = torch.zeros(K, 4, dtype=torch.int32, device=dev())
    out = _guarded(x, d, 5, table, T, I, 2, 1, status)
    ref = torch.full_like(x, float("nan"))
    _lib.check(_lib.lib().dh_latent_update_strided(_lib.ptr(ref), _lib.ptr(x), _lib.ptr(d), 5, 4, 0.1, 256.0, K * hw * hw,
                                                   _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(out[0], ref[0]) and torch.equal(out[2], ref[2])
    assert torch.equal(out[1], x[1])                    # held
    st = status.cpu().tolist()
    assert st[0] == [0, 0, 0, 0] and st[2] == [0, 0, 0, 0]
    assert st[1][0] == 1 and st[1][1] == 1 and st[1][2] == ((2 + 1) << 16 | 1 << 8 | 1)
    # a second failure keeps the first code and counts; per-edit scales divide exactly
    table[0] = 2.0 ** -7
    table[2] = 2.0 ** 9
    out2 = _guarded(x, d, 5, table, T, I, 3, 0, status)
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    assert st[1][1] == 2 and st[1][2] == ((2 + 1) << 16 | 1 << 8 | 1)
    exp0 = x[0] - (0.1 * 2.0 ** 7) * d[0, ..., :4]
    assert torch.allclose(out2[0], exp0, rtol=1e-6, atol=1e-3) and torch.equal(out2[1], x[1])


def test_flagged_ddim_step_sets_only_the_failing_edit():
    from diffusionhandles_amd import _lib
    g = torch.Generator(device=dev()).manual_seed(12)
    K, n1 = 3, 64 * 64 * 4
    x = torch.randn(K, 64, 64, 4, generator=g, device=dev())
    eu = torch.randn_like(x)
    ec = torch.randn_like(x)
    ec[2, 10, 20, 1] = float("nan")
    status = torch.zeros(K, 4, dtype=torch.int32, device=dev())
    out = torch.full_like(x, float("nan"))
    ref = torch.full_like(x, float("nan"))
    _lib.check(_lib.lib().dh_ddim_cfg_step_flagged(_lib.ptr(out), _lib.ptr(x), _lib.ptr(eu), _lib.ptr(ec), 7.5, 0.5, 0.6, x.numel(),
                                                   n1, _lib.ptr(status), 7, 3, _lib.stream_ptr()))
    _lib.check(_lib.lib().dh_ddim_cfg_step(_lib.ptr(ref), _lib.ptr(x), _lib.ptr(eu), _lib.ptr(ec), 7.5, 0.5, 0.6, x.numel(),
                                           _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(out[:2], ref[:2]) and torch.equal(torch.isnan(out[2]), torch.isnan(ref[2]))
    st = status.cpu().tolist()
    assert st[0] == [0, 0, 0, 0] and st[1] == [0, 0, 0, 0]
    assert st[2][0] == 2 and st[2][1] == 0 and st[2][2] == ((7 + 1) << 16 | 3 << 8 | 2)


def test_auto_matches_oracle(rig):
    """'auto' at the default weights within the gates of test_guided_inference_matches_oracle and of the teacher-forced test."""
    from oracle import loop_ref as L
    d, c = rig.edits[0]
    rec_p, rec_o = {}, {}
    with mode(rig.gd, "auto"):
        rig.gd.guided_inference(rig.noise, d, rig.unc, rig.prompt, rig.acts, c, record=rec_p)
    o_final = L.guided_inference(rig.ref, L.DDIM(), rig.noise, d, rig.unc, rig.cond, [a for a in rig.acts], c.cpu().numpy(),
                                 rig.conf, record=rec_o)
    e0 = rel(rec_p["opt"][0] - rig.noise, rec_o["opt"][0] - rig.noise)
    print("auto: first guidance update rel err", e0, "scales", sorted(set(rec_p["scale"])))
    assert e0 < 5e-2
    for i in range(3):
        assert rel(rec_p["step"][i], rec_o["step"][i]) < 2e-2, i
    assert rel(rig.gd.last_latents, o_final) < 0.25
    assert len(rec_p["scale"]) == 38 * 3 and all(np.log2(s) == round(np.log2(s)) for s in rec_p["scale"])
    # teacher-forced: every step from the oracle's latent
    gd = rig.gd
    worst = [0.0, 0.0, 0.0]
    with torch.no_grad(), gd.on_stream(), mode(gd, "auto"):
        gd.scheduler.set_timesteps(50)
        ts = gd.scheduler.timesteps
        st = gd.prepare_guidance(d, rig.prompt, rig.acts, c)
        for i in range(50):
            x_in = rig.noise if i == 0 else rec_o["step"][i - 1]
            rec = {}
            x_out = gd.guided_step(st, x_in.permute(0, 2, 3, 1).contiguous(), i, ts[i], rig.unc[i], record=rec)
            e = rel(x_out.permute(0, 3, 1, 2), rec_o["step"][i])
            worst[0] = max(worst[0], e)
            assert e < 5e-3, (i, e)
            if i < 38:
                eu = rel(rec["opt"][0] - x_in, rec_o["opt"][3 * i] - x_in)
                eu3 = rel(rec["opt"][2] - x_in, rec_o["opt"][3 * i + 2] - x_in)
                worst[1], worst[2] = max(worst[1], eu), max(worst[2], eu3)
                assert eu < 6e-2 and eu3 < 0.2, (i, eu, eu3)
    print("auto teacher-forced worst (step, first update, three updates)", worst)


def _one_step(rig, m, j):
    """one teacher-forced guided step at t_idx 0 with both weights times 2^j: (record, latent after the step)"""
    gd = rig.gd
    d, c = rig.edits[0]
    rec = {}
    with torch.no_grad(), gd.on_stream(), mode(gd, m):
        gd.scheduler.set_timesteps(50)
        st = gd.prepare_guidance(d, rig.prompt, rig.acts, c, fg_weight=rig.conf.fg_weight * 2.0 ** j,
                                 bg_weight=rig.conf.bg_weight * 2.0 ** j)
        x = gd.guided_step(st, rig.noise.permute(0, 2, 3, 1).contiguous(), 0, gd.scheduler.timesteps[0], rig.unc[0], record=rec)
    torch.cuda.synchronize()
    return rec, x


def _oracle_first_update(rig, j):
    from oracle import loop_ref as L
    d, c = rig.edits[0]
    rec = {}
    L.guided_inference(rig.ref, L.DDIM(), rig.noise, d, rig.unc, rig.cond, rig.acts, c.cpu().numpy(), rig.conf,
                       fg_weight=rig.conf.fg_weight * 2.0 ** j, bg_weight=rig.conf.bg_weight * 2.0 ** j, record=rec, steps=[0])
    return rec["opt"][0] - rig.noise


def test_unscaled_gradient_is_invariant_under_power_of_two_weights(rig):
    """The central property: weights x 2^j change the scale by exactly 2^-j, so the cotangent, the backward and d_sample are
    the same bits and the recorded unscaled gradient is exactly 2^j times that of j = 0.  'static' at j = 12 is the witness."""
    rec0, _ = _one_step(rig, "auto", 0)
    g0 = rec0["grad"][0]
    assert torch.isfinite(g0).all() and g0.abs().max() > 0
    for j in (-16, -8, 8, 12):
        rec, _ = _one_step(rig, "auto", j)
        assert rec["scale"][0] == rec0["scale"][0] * 2.0 ** -j, (j, rec["scale"][0], rec0["scale"][0])
        for it in range(3):
            assert torch.isfinite(rec["grad"][it]).all(), (j, it)
        assert torch.equal(rec["grad"][0], g0 * 2.0 ** j), j
    j = 12
    up_o = _oracle_first_update(rig, j)
    rec_a, _ = _one_step(rig, "auto", j)
    rec_s, _ = _one_step(rig, "static", j)
    x0 = rig.noise
    e_auto = rel(rec_a["opt"][0] - x0, up_o)
    up_s = rec_s["opt"][0] - x0
    finite_s = bool(torch.isfinite(up_s).all())
    e_static = rel(up_s, up_o) if finite_s else float("inf")
    print(f"j = {j}: auto first-update rel err {e_auto:.3e}, static {e_static:.3e} (finite {finite_s})")
    assert e_auto < 5e-2
    assert not finite_s or e_static >= 10 * e_auto


def test_overflowing_forward_raises_in_auto_and_is_silent_in_static(rig):
    from diffusionhandles_amd.guided_stable_diffuser import GuidedStableDiffuser
    from oracle import unet_torch as U
    gd = GuidedStableDiffuser(rig.conf, unet=_engine(rig.ref, scale_conv_in=2.0 ** 16),
                              unet_config=dict(U.TINY, text_len=77)).to(dev())
    d, c = rig.edits[0]
    with mode(gd, "auto"):
        with pytest.raises(FloatingPointError) as ei:
            gd.guided_inference(rig.noise, d, rig.unc, rig.prompt, rig.acts, c)
    msg = str(ei.value)
    print(msg)
    assert ei.value.edits == [0] and "edit 0" in msg and "t_idx=0," in msg
    with mode(gd, "static"):
        gd.guided_inference(rig.noise, d, rig.unc, rig.prompt, rig.acts, c)
    assert not torch.isfinite(gd.last_latents).all()


@pytest.fixture(scope="module")
def gd6(rig):
    from diffusionhandles_amd.guided_stable_diffuser import GuidedStableDiffuser
    from oracle import unet_torch as U
    return GuidedStableDiffuser(rig.conf, unet=_engine(rig.ref, max_batch=6), unet_config=dict(U.TINY, text_len=77)).to(dev())


def test_batch_with_per_edit_weights_matches_single_edits(rig, gd6):
    fw = [rig.conf.fg_weight * s for s in (1.0, 8.0, 1.0 / 16)]
    bw = [rig.conf.bg_weight * s for s in (1.0, 8.0, 1.0 / 16)]
    depths, corrs = [d for d, _ in rig.edits], [c for _, c in rig.edits]
    with torch.no_grad(), gd6.on_stream(), mode(gd6, "auto"):
        scales = [gd6.prepare_guidance(d, rig.prompt, rig.acts, c, fw[e], bw[e]).scale_host[0, 0]
                  for e, (d, c) in enumerate(rig.edits)]
    assert len(set(scales)) == 3, scales
    with mode(gd6, "auto"):
        gd6.guided_inference_batch(rig.noise, depths, rig.unc, rig.prompt, rig.acts, corrs, fg_weight=fw, bg_weight=bw)
        batched = gd6.last_latents.clone()
        for e, (d, c) in enumerate(rig.edits):
            gd6.guided_inference(rig.noise, d, rig.unc, rig.prompt, rig.acts, c, fg_weight=fw[e], bg_weight=bw[e])
            err = rel(batched[e:e + 1], gd6.last_latents)
            print("auto batched vs single edit", e, err)
            assert err < 5e-2


def test_batch_names_only_the_failing_edit(rig, gd6):
    depths, corrs = [d.clone() for d, _ in rig.edits], [c for _, c in rig.edits]
    with mode(gd6, "auto"):
        gd6.guided_inference_batch(rig.noise, depths, rig.unc, rig.prompt, rig.acts, corrs)
        clean = gd6.last_latents.clone()
        depths[1] = depths[1].clone()
        depths[1][..., 96:160, 192:256] = float("nan")      # (a block: the bicubic resize to the latent skips single pixels)
        with pytest.raises(FloatingPointError) as ei:
            gd6.guided_inference_batch(rig.noise, depths, rig.unc, rig.prompt, rig.acts, corrs)
    print(ei.value)
    assert ei.value.edits == [1] and "edit 1" in str(ei.value) and "edit 0" not in str(ei.value)
    poisoned = gd6.last_latents
    assert torch.equal(poisoned[0], clean[0]) and torch.equal(poisoned[2], clean[2]), \
        "a non-finite edit changed the other edits of its batch"


def test_auto_lanes_are_bit_identical_to_one_stream(rig, gd6):
    with mode(gd6, "auto"):
        singles = [gd6.guided_inference(rig.noise, d, rig.unc, rig.prompt, rig.acts, c).clone() for d, c in rig.edits]
        laned = gd6.guided_inference_lanes(rig.noise, rig.edits, rig.unc, rig.prompt, rig.acts, streams=2)
        chunks = [([d for d, _ in rig.edits[:2]], [c for _, c in rig.edits[:2]]), ([rig.edits[2][0]], [rig.edits[2][1]])]
        one = [gd6.guided_inference_batch(rig.noise, d, rig.unc, rig.prompt, rig.acts, c).clone() for d, c in chunks]
        two = gd6.guided_inference_batch_lanes(rig.noise, chunks, rig.unc, rig.prompt, rig.acts, streams=2)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(singles, laned))
    assert all(torch.equal(a, b) for a, b in zip(one, two))
