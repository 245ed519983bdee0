"""Batched image identities (null-text inversion + initial inference of K images in B = K / B = 2K passes) on the TINY U-Net:
the per-image masked null-text kernels bit-exact against the single-image kernels, the engine's text gradient at B = 3
against B = 1, K = 1 bit-identical to the single-image paths, K = 3 against three single runs, divergent early stops
inside one batch, and the contract errors.  Gates sit at <= 3x the value measured on the MI355X (stated per test)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from diffusionhandles_amd.synthetic import make_image, make_scene

pytestmark = pytest.mark.gpu

PROMPTS = ["a sphere on a plane", "a red ball in a bright room", "a wooden toy on a table"]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rel(a, b):
    """rel-L2 of a against b; a non-finite element in either fails."""
    a, b = a.float(), b.float()
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), "non-finite elements"
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def poisoned(shape, dtype=torch.float32):
    if dtype.is_floating_point:
        return torch.full(shape, float("nan"), dtype=dtype, device=dev())
    return torch.full(shape, -1, dtype=dtype, device=dev())


def build_diffuser(max_batch, max_diff_batch):
    from diffusionhandles_amd import conf as C
    from diffusionhandles_amd.guided_stable_diffuser import GuidedStableDiffuser
    from diffusionhandles_amd.unet import HipUNet
    from oracle import unet_torch as U
    ref = U.init_synthetic_(U.UNetTorch(U.TINY), seed=0).to(dev()).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.half().float())
    hip = HipUNet(dict(U.TINY, text_len=77), dtype=torch.float16, max_batch=max_batch, max_diff_batch=max_diff_batch)
    hip.load_state_dict(ref.state_dict())
    conf = C.load_default().guided_diffuser
    return GuidedStableDiffuser(conf, unet=hip, unet_config=dict(U.TINY, text_len=77)).to(dev())


@pytest.fixture(scope="module")
def rig():
    from diffusionhandles_amd.depth_transform import normalize_depth
    from diffusionhandles_amd.stable_null_inverter import StableNullInverter
    gd = build_diffuser(6, 3)
    inv = StableNullInverter(gd)
    depth = make_scene(512)[0]
    depths = [depth, depth.flip(-1), depth.flip(-2)]                    # the scene and two mirror images
    disps = [normalize_depth(1.0 / d).to(dev()) for d in depths]
    imgs = [make_image(512, seed=s).to(dev()) for s in (3, 11, 29)]
    return SimpleNamespace(gd=gd, inv=inv, hip=gd.unet, disps=disps, imgs=imgs, prompts=PROMPTS)


# ---- 1. kernels ----------------------------------------------------------------------------------------------------------------
def _mse_single(rec, target, k, amp):
    from diffusionhandles_amd import _lib
    loss, S, d = poisoned((1,)), poisoned((1,)), poisoned(rec.shape)
    _lib.check(_lib.lib().dh_mse_cotangent(_lib.ptr(rec), _lib.ptr(target), rec.numel(), k, amp, _lib.ptr(loss), _lib.ptr(d),
                                           _lib.ptr(S), _lib.stream_ptr()))
    return loss, d, S


def _mse_batch(rec, target, k, amp, threshold, active):
    from diffusionhandles_amd import _lib
    K = rec.shape[0]
    loss, S, d, upd = poisoned((K,)), poisoned((K,)), poisoned(rec.shape), poisoned((K,), torch.int32)
    _lib.check(_lib.lib().dh_mse_cotangent_batch(_lib.ptr(rec), _lib.ptr(target), K, rec[0].numel(), k, amp, threshold,
                                                 _lib.ptr(active), _lib.ptr(upd), _lib.ptr(loss), _lib.ptr(d), _lib.ptr(S),
                                                 _lib.stream_ptr()))
    return loss, d, S, upd


def _adam_single(p, g, S, m, v, step):
    from diffusionhandles_amd import _lib
    _lib.check(_lib.lib().dh_adam_step_scaled(_lib.ptr(p), _lib.ptr(g), _lib.ptr(S), _lib.ptr(m), _lib.ptr(v), 7e-3, 0.9, 0.999,
                                              1e-8, step, p.numel(), _lib.stream_ptr()))


def _adam_batch(p, g, S, upd, m, v, step):
    from diffusionhandles_amd import _lib
    _lib.check(_lib.lib().dh_adam_step_scaled_batch(_lib.ptr(p), _lib.ptr(g), _lib.ptr(S), _lib.ptr(upd), _lib.ptr(m),
                                                    _lib.ptr(v), 7e-3, 0.9, 0.999, 1e-8, step, p.shape[0], p[0].numel(),
                                                    _lib.stream_ptr()))


def _inputs(K=4, seed=41):
    g = torch.Generator(device=dev()).manual_seed(seed)
    rec = torch.randn(K, 64, 64, 4, generator=g, device=dev())
    mags = torch.tensor([1e-3, 1e-1, 3e-5, 1.0], device=dev())[:K].view(K, 1, 1, 1)
    target = (rec + mags * torch.randn(K, 64, 64, 4, generator=g, device=dev())).contiguous()
    p = torch.randn(K, 77, 64, generator=g, device=dev())
    grad = torch.randn(K, 77, 64, generator=g, device=dev()) * 40.0
    m = torch.randn(K, 77, 64, generator=g, device=dev()) * 1e-2
    v = torch.rand(K, 77, 64, generator=g, device=dev()) * 1e-3
    return rec, target, p, grad, m, v


def test_batched_null_text_kernels_are_bit_exact_against_the_single_kernels():
    """K = 4 images, all active: loss, d_eps, S and the Adam step of every image equal four calls of dh_mse_cotangent /
    dh_adam_step_scaled bit for bit; the poisoned outputs are fully written; nothing stops at a negative threshold."""
    rec, target, p0, grad, m0, v0 = _inputs()
    k, amp = -0.37, 16.0
    active = torch.ones(4, dtype=torch.int32, device=dev())
    loss, d, S, upd = _mse_batch(rec, target, k, amp, -1.0, active)
    assert active.tolist() == [1, 1, 1, 1] and upd.tolist() == [1, 1, 1, 1]
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(loss).all()) and bool(torch.isfinite(S).all())
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    _adam_batch(p, grad, S, upd, m, v, 3)
    for b in range(4):
        l1, d1, S1 = _mse_single(rec[b:b + 1].contiguous(), target[b:b + 1].contiguous(), k, amp)
        assert torch.equal(loss[b:b + 1], l1) and torch.equal(S[b:b + 1], S1) and torch.equal(d[b:b + 1], d1), b
        p1, m1, v1 = p0[b:b + 1].clone(), m0[b:b + 1].clone(), v0[b:b + 1].clone()
        _adam_single(p1, grad[b:b + 1].contiguous(), S1, m1, v1, 3)
        assert torch.equal(p[b:b + 1], p1) and torch.equal(m[b:b + 1], m1) and torch.equal(v[b:b + 1], v1), b
    assert len(set(S.tolist())) > 1                      # four different scales: the per-image S is per image


def test_batched_null_text_kernels_inactive_and_stopping_images():
    """Image 1 inactive on entry: d_eps = 0, S = 1, its loss written, not updated, parameters and moments untouched, still
    inactive.  Image 2's loss (3e-5 scale differences: ~1e-9) falls below the threshold: updated this step, inactive on exit.
    Images 0 and 3 stay active.  A non-finite gradient element is skipped (parameter and moments keep their values)."""
    rec, target, p0, grad, m0, v0 = _inputs()
    active = torch.tensor([1, 0, 1, 1], dtype=torch.int32, device=dev())
    loss, d, S, upd = _mse_batch(rec, target, -0.37, 16.0, 1e-8, active)
    losses = loss.tolist()
    assert losses[2] < 1e-8 < min(losses[0], losses[3]), losses
    assert upd.tolist() == [1, 0, 1, 1] and active.tolist() == [1, 0, 0, 1]
    assert bool((d[1] == 0).all()) and S[1].item() == 1.0
    l1, _, _ = _mse_single(rec[1:2].contiguous(), target[1:2].contiguous(), -0.37, 16.0)
    assert torch.equal(loss[1:2], l1)
    g = grad.clone()
    g[0, 5, 7] = float("inf")
    g[3, 0, 0] = float("nan")
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    _adam_batch(p, g, S, upd, m, v, 1)
    assert torch.equal(p[1], p0[1]) and torch.equal(m[1], m0[1]) and torch.equal(v[1], v0[1])
    for b, idx in ((0, (5, 7)), (3, (0, 0))):
        assert p[b][idx] == p0[b][idx] and m[b][idx] == m0[b][idx] and v[b][idx] == v0[b][idx]
        assert int((p[b] != p0[b]).sum()) == p[b].numel() - 1
    for b in (0, 2, 3):
        p1, m1, v1 = p0[b:b + 1].clone(), m0[b:b + 1].clone(), v0[b:b + 1].clone()
        _adam_single(p1, g[b:b + 1].contiguous(), S[b:b + 1].contiguous(), m1, v1, 1)
        assert torch.equal(p[b:b + 1], p1) and torch.equal(m[b:b + 1], m1) and torch.equal(v[b:b + 1], v1), b


def test_batched_early_stop_compares_in_double_like_the_host():
    """The threshold is a double compared against the f32 loss widened to double (the host's `loss.item() < eps + 2e-5 i`).
    Thresholds one f32 ulp either side of the loss, the loss itself, and a double between the loss and the next f32 (a
    float threshold would round it onto the loss and keep the image running)."""
    rec, target, _, _, _, _ = _inputs(K=1, seed=43)
    active = torch.ones(1, dtype=torch.int32, device=dev())
    loss, _, _, _ = _mse_batch(rec, target, -0.37, 16.0, -1.0, active)
    L32 = np.float32(loss.item())
    up, down = float(np.nextafter(L32, np.float32(np.inf))), float(np.nextafter(L32, np.float32(-np.inf)))
    between = float(L32) * (1.0 + 2.0 ** -40)
    assert float(np.float32(between)) == float(L32) and between > float(L32)
    for thr in (up, down, float(L32), between):
        active = torch.ones(1, dtype=torch.int32, device=dev())
        _mse_batch(rec, target, -0.37, 16.0, thr, active)
        host_stops = float(L32) < thr
        assert active.item() == (0 if host_stops else 1), (thr, float(L32))
    assert float(L32) < between                          # the case a float threshold gets wrong: it must stop


# ---- 2. engine text gradient at B = 3 -----------------------------------------------------------------------------------------
def test_engine_text_gradient_batch3_equals_three_batch1(rig):
    """d eps / d text of ONE saved B = 3 forward (three samples, three texts) equals the three B = 1 backward passes per
    sample: rel-L2 < 9e-3 (measured 3.2e-3: the fp16 rounding of the batch-dependent GEMM tiles and dK/dV split)."""
    hip = rig.hip
    g = torch.Generator(device=dev()).manual_seed(31)
    x = torch.randn(3, 64, 64, 5, generator=g, device=dev())
    text = torch.randn(3, 77, 64, generator=g, device=dev())
    d_eps = torch.randn(3, 64, 64, 4, generator=g, device=dev()) * 0.05
    with rig.gd.on_stream():
        hip.forward(x, 421.0, text, save_for_backward=True, want_acts=False)
        _, dt3 = hip.backward(None, d_eps, want_sample_grad=False, want_text_grad=True)
        dt3 = dt3.clone()
        errs = []
        for b in range(3):
            hip.forward(x[b:b + 1].contiguous(), 421.0, text[b:b + 1].contiguous(), save_for_backward=True, want_acts=False)
            _, dt1 = hip.backward(None, d_eps[b:b + 1].contiguous(), want_sample_grad=False, want_text_grad=True)
            errs.append(rel(dt3[b:b + 1], dt1))
    print("TINY text gradient B = 3 vs B = 1, rel-L2 per sample", errs)
    assert float(dt3.abs().max()) > 0
    assert max(errs) < 9e-3, errs


# ---- 3. K = 1 bit-identical ---------------------------------------------------------------------------------------------------
def test_k1_is_bit_identical_to_the_single_image_paths(rig):
    inv, gd = rig.inv, rig.gd
    img, disp, prompt = rig.imgs[0], rig.disps[0], rig.prompts[0]
    (_, rec_s), noise_s, unc_s = inv.invert(img, disp, prompt, num_inner_steps=5)
    taken_s = list(inv.inner_steps_taken)
    [((_, rec_b), noise_b, unc_b)] = inv.invert_batch([img], [disp], [prompt], num_inner_steps=5)
    assert inv.inner_steps_taken == [taken_s]
    assert torch.equal(noise_b, noise_s) and torch.equal(rec_b, rec_s)
    assert unc_b.shape == unc_s.shape == (50, 1, 77, 64) and torch.equal(unc_b, unc_s)
    acts_s, lat_s, _, _ = gd.initial_inference(noise_s, disp, unc_s, prompt)
    acts_s = [a.clone() for a in acts_s]
    [(acts_b, lat_b, u_b, n_b)] = gd.initial_inference_batch([noise_s], [disp], [unc_s], [prompt])
    assert u_b is unc_s and n_b is noise_s
    assert torch.equal(lat_b, lat_s)
    for a, b in zip(acts_b, acts_s):
        assert a.shape == b.shape and torch.equal(a, b)


# ---- 4. K = 3 against three single runs ---------------------------------------------------------------------------------------
def _recording(inv, name, store):
    orig = getattr(inv, name)

    def wrapped(*a, **kw):
        r = {}
        store.append(r)
        return orig(*a, record=r, **kw)
    return wrapped


def _free_running_losses(gd, inv, lat, depth_nhwc, cond, unc):
    """The product's CFG re-denoise of one image with its own unconds: mse against its DDIM latents at every timestep."""
    out = []
    cur = lat[-1]
    for i in range(50):
        t = gd.scheduler.timesteps[i]
        a_t, a_p = gd.scheduler.step_alphas(t)
        eu, ec = gd._cfg_eps(cur, depth_nhwc, t, unc[i], cond)
        cur = inv._step(cur, eu, ec, 7.5, a_t, a_p)
        out.append(torch.nn.functional.mse_loss(cur, lat[len(lat) - i - 2]).item())
    return out


def test_k3_matches_three_single_runs(rig):
    """K = 3 images (three seeds, the scene and its mirror images, three prompts), all 50 timesteps, free-running, against
    three single-image runs: the DDIM-inverted noise rel-L2 < 1e-2 (measured 3.4e-3), the reconstruction loss the product's
    CFG re-denoise reaches with each run's own unconds within 0.4 % + 2e-6 at every timestep (measured 0.15 %), the inner
    steps taken equal unless a loss lies within 3 % of the threshold; initial_inference_batch against initial_inference on
    the same inputs: activations rel-L2 < 5.5e-2 (measured 1.9e-2), final latents < 6.5e-2 (measured 2.3e-2; 50 CFG steps
    at w = 7.5 amplify the fp16 differences of the B = 6 and B = 2 passes)."""
    inv, gd = rig.inv, rig.gd
    singles = []
    for img, disp, prompt in zip(rig.imgs, rig.disps, rig.prompts):
        recs = []
        inv.null_step = _recording(inv, "null_step", recs)
        try:
            _, noise, unc = inv.invert(img, disp, prompt, num_inner_steps=5)
        finally:
            del inv.null_step
        singles.append(SimpleNamespace(noise=noise, unc=unc, taken=list(inv.inner_steps_taken), lat=inv.last_ddim_latents,
                                       loss=[r["loss"] for r in recs]))
    recs = []
    inv.null_step_batch = _recording(inv, "null_step_batch", recs)
    try:
        res = inv.invert_batch(rig.imgs, rig.disps, rig.prompts, num_inner_steps=5)
    finally:
        del inv.null_step_batch
    taken_b, lat_b = inv.inner_steps_taken, inv.last_ddim_latents
    assert len(res) == 3 and len(taken_b) == 3 and lat_b[-1].shape[0] == 3
    worst = dict(noise=0.0, loss=0.0, acts=0.0, lat=0.0)
    with gd.on_stream():
        for b, s in enumerate(singles):
            (img_b, _), noise, unc = res[b]
            assert img_b is rig.imgs[b] and unc.shape == (50, 1, 77, 64) and noise.shape == (1, 4, 64, 64)
            worst["noise"] = max(worst["noise"], rel(noise, s.noise))
            thr = [1e-5 + i * 2e-5 for i in range(50)]
            for i in range(50):
                lb = [step[b] for step, upd in zip(recs[i]["loss"], recs[i]["updated"]) if upd[b]]
                near = any(abs(x - thr[i]) < 3e-2 * thr[i] for x in s.loss[i] + lb)
                if not near:
                    assert taken_b[b][i] == s.taken[i], (b, i, s.loss[i], lb)
            depth_nhwc = gd.init_depth(rig.disps[b]).permute(0, 2, 3, 1).contiguous()
            cond = gd._encode([rig.prompts[b]])
            fs = _free_running_losses(gd, inv, s.lat, depth_nhwc, cond, s.unc)
            fb = _free_running_losses(gd, inv, [x[b:b + 1] for x in lat_b], depth_nhwc, cond, unc)
            for p_, o_ in zip(fb, fs):
                worst["loss"] = max(worst["loss"], abs(p_ - o_) / (o_ + 2e-6))
                assert abs(p_ - o_) < 4e-3 * o_ + 2e-6, (b, fb, fs)
    ii_s = []
    for b, s in enumerate(singles):
        acts, lat, _, _ = gd.initial_inference(s.noise, rig.disps[b], s.unc, rig.prompts[b])
        ii_s.append(([a.clone() for a in acts], lat.clone()))
    ii_b = gd.initial_inference_batch([s.noise for s in singles], rig.disps, [s.unc for s in singles], rig.prompts)
    for (acts_b, lat_b_, _, _), (acts_s, lat_s) in zip(ii_b, ii_s):
        worst["lat"] = max(worst["lat"], rel(lat_b_, lat_s))
        for a, c in zip(acts_b, acts_s):
            worst["acts"] = max(worst["acts"], rel(a, c))
    print("K = 3 vs single runs, worst", worst, "inner steps batch", [t[::10] for t in taken_b],
          "single", [s.taken[::10] for s in singles])
    assert worst["noise"] < 1e-2 and worst["acts"] < 5.5e-2 and worst["lat"] < 6.5e-2, worst


def test_initial_inference_batch_draws_the_noise_of_sequential_calls(rig):
    """Images without init_latents get the noise K sequential initial_inference calls draw (each re-seeds with conf.seed:
    the same noise for every image), and the generator is left where those calls leave it."""
    gd = rig.gd
    unc = gd._encode([""])[None].expand(50, -1, -1, -1)
    _, _, _, n_single = gd.initial_inference(None, rig.disps[0], unc, rig.prompts[0])
    after_single = torch.randn(4)
    res = gd.initial_inference_batch([None, None], rig.disps[:2], [unc, None], rig.prompts[:2])
    after_batch = torch.randn(4)
    assert torch.equal(res[0][3], n_single) and torch.equal(res[1][3], n_single)
    assert torch.equal(after_batch, after_single)
    assert res[1][2].shape == (50, 1, 77, 64)


# ---- 5. divergent early stops --------------------------------------------------------------------------------------------------
def test_divergent_early_stops_in_one_batch(rig):
    """One timestep's batched inner loop on two images.  A's target is its DDIM latent; B's target is the reconstruction
    B's initial uncond produces in the same B = 2 passes (plus 1e-5 noise), so B's first loss is ~1e-10 and B stops after one step while A
    runs all five: taken = [5, 1].  B's uncond after the five-step batch equals the one-step batch bit for bit (frozen while
    A continues) and a single-image run of one step within rel-L2 1.5e-2 (measured 5.1e-3: the B = 1 pass sees a loss of
    9e-7 where the B = 2 pass sees 1e-10, and Adam's first step is +-lr whatever the gradient's size); A's optimised change
    of uncond matches its single five-step run within rel-L2 1.2e-2 (measured 4.3e-3) and its losses within 1e-3 (measured
    3.2e-4)."""
    inv, gd = rig.inv, rig.gd
    with gd.on_stream(), torch.no_grad():
        depth = torch.cat([gd.init_depth(d).permute(0, 2, 3, 1) for d in rig.disps[:2]]).contiguous()
        ctx = [gd.init_prompt(p) for p in rig.prompts[:2]]
        unc0 = torch.cat([c[0:1] for c in ctx]).contiguous()
        cond = torch.cat([c[1:2] for c in ctx]).contiguous()
        lat = inv.image2latent(torch.cat(rig.imgs[:2])).permute(0, 2, 3, 1).contiguous()
        ddim = inv.ddim_loop(lat, torch.cat([unc0, cond]), depth)
        i = 3
        cur = ddim[-1 - i] if i else ddim[-1]
        target = ddim[len(ddim) - i - 2].clone()
        t = gd.scheduler.timesteps[i]
        a_t, a_p = gd.scheduler.step_alphas(t)
        eps_c = inv.get_noise_pred_single(cur, t, cond, depth)
        eps_u = inv.get_noise_pred_single(cur, t, unc0, depth, save=True)
        g = torch.Generator(device=dev()).manual_seed(51)
        # B's reconstruction plus a 1e-5 perturbation: its first loss is ~1e-10, below the threshold of 1e-9, with a gradient
        target[1] = inv._step(cur, eps_u, eps_c, 7.5, a_t, a_p)[1] + 1e-5 * torch.randn(target[1].shape, generator=g, device=dev())
        eps = 1e-9 - i * 2e-5
        u1 = unc0.clone()
        r1 = {}
        taken1 = inv.null_step_batch(cur, u1, cond, depth, i, target, 1, eps, record=r1)
        u5 = unc0.clone()
        r5 = {}
        taken5 = inv.null_step_batch(cur, u5, cond, depth, i, target, 5, eps, record=r5)
        assert r5["loss"][0][1] < 1e-9 < min(x[0] for x in r5["loss"]) and taken1 == [1, 1] and taken5 == [5, 1], (taken5, r5["loss"])
        assert r5["updated"] == [[1, 1], [1, 0], [1, 0], [1, 0], [1, 0]]
        assert torch.equal(u5[1], u1[1]) and not torch.equal(u5[1], unc0[1]) and not torch.equal(u5[0], u1[0])
        singles = []
        for b, steps in ((0, 5), (1, 1)):
            u = unc0[b:b + 1].clone()
            r = {}
            n = inv.null_step(cur[b:b + 1].contiguous(), u, cond[b:b + 1].contiguous(), depth[b:b + 1].contiguous(), i,
                              target[b:b + 1].contiguous(), steps, -1.0, record=r)
            assert n == steps
            singles.append((u, r["loss"]))
    eA, eB = rel(u5[0:1] - unc0[0:1], singles[0][0] - unc0[0:1]), rel(u5[1:2], singles[1][0])
    la = max(abs(x[0] - y) / y for x, y in zip(r5["loss"], singles[0][1]))
    print("divergent stops: A update rel-L2", eA, "B uncond rel-L2", eB, "A loss rel", la, "losses", r5["loss"])
    assert eA < 1.2e-2 and eB < 1.5e-2 and la < 1e-3, (eA, eB, la)


# ---- 6. contract errors --------------------------------------------------------------------------------------------------------
def test_contract_errors(rig):
    from diffusionhandles_amd import DiffusionHandles
    from diffusionhandles_amd.stable_null_inverter import StableNullInverter
    small = build_diffuser(2, 1)
    inv2 = StableNullInverter(small)
    with pytest.raises(RuntimeError, match="max_diff_batch >= 2"):
        inv2.invert_batch(rig.imgs[:2], rig.disps[:2], rig.prompts[:2])
    with pytest.raises(RuntimeError, match="max_batch >= 4"):
        small.initial_inference_batch(None, rig.disps[:2], None, rig.prompts[:2])
    dh = DiffusionHandles(None, unet=small.unet, unet_config=dict(small._unet_config)).to(dev())
    depth = make_scene(512)[0].to(dev())
    with pytest.raises(RuntimeError, match="max_batch >= 4"):
        dh.invert_input_images(rig.imgs[:2], [depth, depth], rig.prompts[:2])
    with pytest.raises(RuntimeError, match="max_batch >= 4"):
        dh.generate_input_images([depth, depth], rig.prompts[:2])
    small.unet.close()
    # mixed resolutions
    with pytest.raises(ValueError, match="256"):
        rig.inv.invert_batch([rig.imgs[0], make_image(256).to(dev())], rig.disps[:2], rig.prompts[:2])
    with pytest.raises(ValueError, match="32"):
        rig.gd.initial_inference_batch([None, torch.zeros(1, 4, 32, 32, device=dev())], rig.disps[:2], None, rig.prompts[:2])
    with pytest.raises(ValueError):
        rig.inv.invert_batch(rig.imgs[:2], rig.disps[:1], rig.prompts[:2])
