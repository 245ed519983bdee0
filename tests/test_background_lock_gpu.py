"""GPU: the background lock -- dh_keep_map against tests/background_lock_ref.py (exactly), dh_ddim_cfg_step_locked against
dh_ddim_cfg_step and the reference trajectory, the trajectory that rides on the identity, the locked loops (single, batched,
items, lanes; 'static' and 'auto' guidance scale) on the TINY rig of tests/test_multi_object_gpu.py, and tools/run_edit.py
--background-lock.  The C entries write into outputs that are NaN / 0xFF before the call."""
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
import background_lock_ref as B  # noqa: E402
import multi_object_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, S, T = 512, 64, 50
NAN = float("nan")


def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _t(tf):
    a, ax, tr = tf
    return (float(a), torch.tensor(ax, dtype=torch.float32), torch.tensor(tr, dtype=torch.float32))


# ---- 1. dh_keep_map ---------------------------------------------------------------------------------------------------------
def _keep_abi(corr, mask, release, res, s, dilate, feather):
    """dh_keep_map on a NaN output and a 0xFF workspace -> (return code, keep [s,s] on the host)."""
    from diffusionhandles_amd import _lib
    L = _lib.lib()
    keep = torch.full((max(s, 1), max(s, 1)), NAN, dtype=torch.float32, device=dev())
    ws = torch.full((max(s, 1) ** 2,), 0xFF, dtype=torch.uint8, device=dev())
    c = None if corr is None or len(corr) == 0 else torch.from_numpy(np.ascontiguousarray(corr, dtype=np.int64)).to(dev())
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).to(dev())
    r = None if release is None else torch.from_numpy(np.ascontiguousarray(release, dtype=np.uint8)).to(dev())
    rc = L.dh_keep_map(_lib.ptr(c), 0 if c is None else c.shape[0], _lib.ptr(m), _lib.ptr(r), res, s, dilate, feather,
                       _lib.ptr(keep), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, keep.cpu().numpy()


def _random_inputs(res, seed):
    rng = np.random.default_rng(seed)
    n = 40
    corr = np.empty((n, 4), dtype=np.int64)
    corr[:, :2] = rng.integers(res // 4, res // 2, size=(n, 2))              # sources in the image
    corr[:, 2:] = rng.integers(-res // 4, res + res // 4, size=(n, 2))       # targets in and around it
    corr[0, 2:] = (-1, 0)
    corr[1, 2:] = (0, res)
    corr[2, 2:] = (res - 1, res - 1)
    assert ((corr[:, 2:] < 0) | (corr[:, 2:] >= res)).any(axis=1).sum() >= 5
    mask = np.zeros((res, res), dtype=np.uint8)
    mask[res // 8: res // 8 + 5, res - 7:] = 255
    release = np.zeros((res, res), dtype=np.uint8)
    release[res - 3:, :11] = 1
    return corr, mask, release


@pytest.mark.parametrize("res,s", [(64, 8), (96, 12)])
def test_keep_map_equals_the_reference_exactly(res, s):
    corr, mask, release = _random_inputs(res, seed=res)
    cases = {"all": (corr, mask, release), "corr": (corr, None, None), "mask": (None, mask, None), "release": (None, None, release),
             "mask+release, N=0": (np.zeros((0, 4), dtype=np.int64), mask, release), "nothing": (None, None, None)}
    seen = set()
    for dilate in range(4):
        for feather in range(4):
            for name, (c, m, r) in cases.items():
                rc, got = _keep_abi(c, m, r, res, s, dilate, feather)
                want = B.keep_map(c, m, r, res, s, dilate, feather)
                assert rc == 0 and np.array_equal(got, want), (name, dilate, feather)
                seen.update(np.unique(got).tolist())
    assert 0.0 in seen and 1.0 in seen and len(seen) > 4          # zeros, ones and ramps were all compared
    assert np.array_equal(_keep_abi(None, None, None, res, s, 2, 2)[1], np.ones((s, s), dtype=np.float32))


def test_keep_map_with_a_reach_beyond_the_grid():
    """s = 4, dilate 3, feather 3: the window (7 cells each way) is clipped everywhere."""
    mask = np.zeros((32, 32), dtype=np.uint8)
    mask[0, 0] = 1
    for c in (None, np.array([[31, 31, 40, 40], [31, 31, 16, 0]])):
        rc, got = _keep_abi(c, mask, None, 32, 4, 3, 3)
        assert rc == 0 and np.array_equal(got, B.keep_map(c, mask, None, 32, 4, 3, 3))
    rc, got = _keep_abi(None, mask, None, 32, 4, 0, 31)
    assert rc == 0 and np.array_equal(got, B.keep_map(None, mask, None, 32, 4, 0, 31)) and got[3, 3] == np.float32(3) / np.float32(32)


@pytest.mark.parametrize("res,s,dilate,feather", [(64, 8, -1, 2), (64, 8, 2, -1), (64, 8, 16, 16), (64, 8, 0, 32), (64, 7, 2, 2),
                                                  (60, 8, 2, 2)])
def test_keep_map_refuses_bad_arguments_and_leaves_the_output_poisoned(res, s, dilate, feather):
    from diffusionhandles_amd import _lib
    mask = np.ones((res, res), dtype=np.uint8)
    rc, got = _keep_abi(None, mask, None, res, s, dilate, feather)
    assert rc != 0 and np.isnan(got).all()
    assert b"dh_keep_map" in _lib.lib().dh_last_error()


def test_keep_map_host_function(tiny_geo):
    """background_lock.keep_map on the rig's edit: masks as [1,1,R,R] float tensors, a list of masks, a release image."""
    from diffusionhandles_amd.background_lock import keep_map
    g = tiny_geo
    m0 = g.masks[0][0, 0].cpu().numpy()
    m1 = g.masks[1][0, 0].cpu().numpy()
    c = g.corr[0].cpu().numpy()
    assert np.array_equal(keep_map(g.corr[0], g.masks[0], None, RES, S).cpu().numpy(), B.keep_map(c, m0, None, RES, S, 2, 2))
    rel = torch.zeros(RES, RES)
    rel[500:, :9] = 1.0
    got = keep_map(g.corr[0].cpu(), list(g.masks), rel, RES, S, 1, 3).cpu().numpy()
    assert np.array_equal(got, B.keep_map(c, (m0 != 0) | (m1 != 0), rel.numpy(), RES, S, 1, 3)) and got[63, 0] == 0.0
    assert np.array_equal(keep_map(None, None, None, RES, S).cpu().numpy(), np.ones((S, S), dtype=np.float32))
    with pytest.raises(ValueError, match="keep_map"):
        keep_map(g.corr[0], g.masks[0], None, RES, 60)
    with pytest.raises(ValueError, match="keep_map"):
        keep_map(g.corr[0], g.masks[0], None, RES, S, 20, 12)


# ---- 2. dh_ddim_cfg_step_locked ---------------------------------------------------------------------------------------------
ALPHA_T, ALPHA_P, SCALE = 0.31, 0.47, 7.5


def _step_inputs(s, seed):
    g = torch.Generator().manual_seed(seed)
    K, C = 3, 4
    x, eu, ec, ref = (torch.randn(K, s, s, C, generator=g).to(dev()) for _ in range(4))
    levels = torch.tensor([0.0, 1.0, 1.0 / 3.0, 0.5, 2.0 / 3.0, 1.0, 0.0, np.float32(3) / np.float32(32)])
    keep0 = levels[torch.randint(0, len(levels), (s, s), generator=g)].to(dev())
    keeps = [keep0.contiguous(), None, torch.ones(s, s, device=dev())]
    return x, eu, ec, ref, keeps


def _plain_step(x, eu, ec):
    from diffusionhandles_amd import _lib
    out = torch.full_like(x, NAN)
    _lib.check(_lib.lib().dh_ddim_cfg_step(_lib.ptr(out), _lib.ptr(x), _lib.ptr(eu), _lib.ptr(ec), SCALE, ALPHA_T, ALPHA_P, x.numel(),
                                           _lib.stream_ptr()), "dh_ddim_cfg_step")
    return out


def _locked_step(x, eu, ec, ref, keeps, status=None, n_items=None, t_idx=7, iteration=3):
    from diffusionhandles_amd import _lib
    K = x.shape[0]
    out = torch.full_like(x, NAN)
    items = (_lib.LockItem * max(K, n_items or 0))()
    for e in range(K):
        if keeps[e] is not None:
            items[e].keep, items[e].ref = keeps[e].data_ptr(), ref[e].data_ptr()
    rc = _lib.lib().dh_ddim_cfg_step_locked(_lib.ptr(out), _lib.ptr(x), _lib.ptr(eu), _lib.ptr(ec), SCALE, ALPHA_T, ALPHA_P, x.numel(),
                                            x[0].numel(), x.shape[-1], items, K if n_items is None else n_items, _lib.ptr(status),
                                            t_idx, iteration, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("s", [8, 6])          # 6: 144 elements per edit, the last block of every edit is partial
def test_locked_step_against_the_plain_step(s):
    x, eu, ec, ref, keeps = _step_inputs(s, seed=s)
    base = _plain_step(x, eu, ec)
    rc, out = _locked_step(x, eu, ec, ref, keeps)
    assert rc == 0 and torch.isfinite(out).all()
    assert torch.equal(out[1], base[1])                                        # the NULL item: the plain step, bitwise
    assert torch.equal(out[2], ref[2])                                         # keep == 1 everywhere: the reference, bitwise
    k = keeps[0][..., None].expand(-1, -1, 4)
    assert int((k == 0).sum()) > 0 and int((k == 1).sum()) > 0 and int(((k > 0) & (k < 1)).sum()) > 0
    assert torch.equal(out[0][k == 0], base[0][k == 0])
    assert torch.equal(out[0][k == 1], ref[0][k == 1])
    o, r = base[0].cpu().numpy(), ref[0].cpu().numpy()
    want = B.blend(o, r, k.cpu().numpy())
    frac = ((k > 0) & (k < 1)).cpu().numpy()
    bound = np.float32(2.0 ** -22) * np.maximum(np.abs(o), np.abs(r))
    err = np.abs(out[0].cpu().numpy().astype(np.float64) - want.astype(np.float64))
    print(f"s = {s}: fractional cells, max error / bound = {float((err[frac] / bound[frac]).max()):.3f}")
    assert (err[frac] <= bound[frac]).all()
    # the plain step restated in NumPy float32 agrees to rounding (the kernels themselves are compared bitwise above)
    o_ref = B.ddim_cfg(x[0].cpu().numpy(), eu[0].cpu().numpy(), ec[0].cpu().numpy(), SCALE, ALPHA_T, ALPHA_P)
    assert np.allclose(o, o_ref, rtol=1e-5, atol=1e-5)
    # with a clean status array nothing is written to it and the output is the same
    status = torch.zeros((3, 4), dtype=torch.int32, device=dev())
    rc, out2 = _locked_step(x, eu, ec, ref, keeps, status=status)
    assert rc == 0 and torch.equal(out2, out) and int(status.abs().sum()) == 0


@pytest.mark.parametrize("s", [8, 6])
def test_locked_step_flags_a_bad_step_under_a_locked_cell(s):
    """A NaN in eps_c under a keep-1 cell: the edit's status gets bit 1 (value 2, what dh_ddim_cfg_step_flagged sets) and its
    code, the other edits' words stay clean, and the cell's output is the reference -- the flag is judged before the blend."""
    x, eu, ec, ref, keeps = _step_inputs(s, seed=10 + s)
    base = _plain_step(x, eu, ec)
    code = ((7 + 1) << 16) | (3 << 8) | 2
    ones0 = torch.nonzero(keeps[0] == 1)
    for item, (cy, cx) in ((0, ones0[0].tolist()), (2, (s - 1, s - 1)), (1, (s // 2, 1))):
        ec_bad = ec.clone()
        ec_bad[item, cy, cx, 2] = NAN
        status = torch.zeros((3, 4), dtype=torch.int32, device=dev())
        rc, out = _locked_step(x, eu, ec_bad, ref, keeps, status=status)
        st = status.cpu().tolist()
        assert rc == 0 and st[item] == [2, 0, code, 0] and all(st[e] == [0, 0, 0, 0] for e in range(3) if e != item), (item, st)
        if keeps[item] is None:                      # an unlocked edit: the plain step's NaN, as the flagged step leaves it
            assert torch.isnan(out[item, cy, cx, 2]) and int(torch.isnan(out).sum()) == 1
        else:
            assert torch.equal(out[item, cy, cx], ref[item, cy, cx]) and torch.isfinite(out).all()
        mask = torch.ones_like(out, dtype=torch.bool)
        mask[item, cy, cx, 2] = False
        rc, clean = _locked_step(x, eu, ec, ref, keeps)
        assert torch.equal(out[mask], clean[mask])
        # without a status array (static mode) the same outputs, nothing else touched
        rc, out_s = _locked_step(x, eu, ec_bad, ref, keeps)
        assert rc == 0 and torch.equal(torch.nan_to_num(out_s, nan=-7.0), torch.nan_to_num(out, nan=-7.0))
    assert torch.isfinite(base).all()


def test_locked_step_refuses_more_than_16_items_and_a_lock_without_its_reference():
    from diffusionhandles_amd import _lib
    x, eu, ec, ref, keeps = _step_inputs(6, seed=3)
    rc, out = _locked_step(x, eu, ec, ref, keeps, n_items=17)
    assert rc != 0 and torch.isnan(out).all() and b"dh_ddim_cfg_step_locked" in _lib.lib().dh_last_error()
    rc, out = _locked_step(x, eu, ec, ref, keeps, n_items=2)                  # not one item per edit
    assert rc != 0 and torch.isnan(out).all()
    out = torch.full_like(x, NAN)
    items = (_lib.LockItem * 3)()
    items[0].keep = keeps[0].data_ptr()                                        # keep without ref
    rc = _lib.lib().dh_ddim_cfg_step_locked(_lib.ptr(out), _lib.ptr(x), _lib.ptr(eu), _lib.ptr(ec), SCALE, ALPHA_T, ALPHA_P, x.numel(),
                                            x[0].numel(), 4, items, 3, None, 0, 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and torch.isnan(out).all()


# ---- the TINY rig of tests/test_multi_object_gpu.py -------------------------------------------------------------------------
def _tiny_handles(ref, max_batch):
    from diffusionhandles_amd import DiffusionHandles
    from diffusionhandles_amd import conf as C
    from diffusionhandles_amd.unet import HipUNet
    from oracle import unet_torch as U
    hip = HipUNet(dict(U.TINY, text_len=77), dtype=torch.float16, max_batch=max_batch)
    hip.load_state_dict(ref.state_dict())
    return DiffusionHandles(C.load_default(), unet=hip, unet_config=dict(U.TINY, text_len=77)).to(dev())


@pytest.fixture(scope="module")
def tiny():
    """The two-sphere image and its identity (initial inference from noise, no inversion) by the product."""
    from oracle import unet_torch as U
    ref = U.init_synthetic_(U.UNetTorch(U.TINY), seed=0).to(dev()).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.half().float())
    dh = _tiny_handles(ref, 4)
    depth, bg, masks = R.two_spheres(RES)
    depth, bg, masks = depth.to(dev()), bg.to(dev()), [m.to(dev()) for m in masks]
    g = torch.Generator().manual_seed(11)
    noise = torch.randn(1, 4, S, S, generator=g).to(dev())
    Dm = dh.diffuser.unet.cfg["cross_attention_dim"]
    unc = (dh.diffuser._encode([""])[None].expand(T, -1, -1, -1) + 0.05 * torch.randn(T, 1, 77, Dm, generator=g).to(dev())).contiguous()
    prompt = "two spheres on a plane"
    null_text, noise, acts, latent = dh.generate_input_image(depth, prompt, unc, noise)
    return SimpleNamespace(dh=dh, gd=dh.diffuser, depth=depth, bg_raw=bg, bg_depth=dh.set_foreground(depth, masks, bg), masks=masks,
                           prompt=prompt, null_text=null_text, noise=noise, acts=acts, latent=latent)


EDITS = [_t(R.OCCLUDING[0]), _t((20.0, R.Y, (0.25, 0.0, 0.0))), _t((-15.0, R.Y, (0.1, 0.0, 0.1))), _t((10.0, R.Y, (-0.3, 0.0, 0.0)))]


@pytest.fixture(scope="module")
def tiny_geo(tiny):
    """Object 0 of the two-sphere image moved four ways: disparities, device correspondences, default keep maps."""
    from diffusionhandles_amd.background_lock import keep_map
    from diffusionhandles_amd.depth_transform import reproject_edits
    rp = reproject_edits(tiny.depth, tiny.bg_depth, tiny.masks[0], tiny.gd.get_depth_intrinsics(device=dev()), EDITS,
                         device_correspondences=True)
    keeps = [keep_map(c, tiny.masks[0], None, RES, S) for _, c in rp]
    return SimpleNamespace(disp=[d for d, _ in rp], corr=[c for _, c in rp], keeps=keeps, masks=tiny.masks)


@pytest.fixture()
def locked(tiny):
    """conf background_lock: true on the rig's handles for one test."""
    tiny.dh.conf["background_lock"] = True
    yield tiny
    for k in ("background_lock", "background_lock_dilate", "background_lock_feather"):
        tiny.dh.conf.pop(k, None)


def _held(latents, traj_t, keep):
    """latents [4,s,s] equal traj_t on the keep-1 cells, bitwise"""
    one = (keep == 1)[None].expand(4, -1, -1)
    return torch.equal(latents[one], traj_t[one])


# ---- 3. the trajectory ------------------------------------------------------------------------------------------------------
def _parent_initial_inference(gd, init_latents, depths, uncs, prompts):
    """The initial inference as it was before the trajectory: the same passes, every DDIM step into a tensor of its own.
    K images in one batch (K = 1: initial_inference's passes, through _cfg_eps)."""
    from diffusionhandles_amd.guided_stable_diffuser import _nhwc
    K = len(prompts)
    with torch.no_grad(), gd.on_stream():
        gd.scheduler.set_timesteps(gd.conf.num_timesteps, device=gd.device)
        timesteps, _ = gd.get_timesteps(gd.conf.num_timesteps, 1.0)
        depth_nhwc = torch.cat([_nhwc(gd.init_depth(d.to(gd.device, torch.float32))) for d in depths])
        cond = torch.cat([gd._encode([p]) for p in prompts]).contiguous()
        x = torch.cat([_nhwc(lat.to(gd.device, torch.float32)) for lat in init_latents])
        store = [[torch.empty((len(timesteps),) + shp, dtype=gd.dtype, device=gd.device) for shp in gd.unet.act_shapes] for _ in range(K)]
        for t_idx, t in enumerate(timesteps):
            if K == 1:
                eu, ec, acts = gd._cfg_eps(x, depth_nhwc, t, uncs[0][t_idx], cond, want_acts=True)
                half = 1
            else:
                unc = torch.cat([u[t_idx].reshape(1, *cond.shape[1:]).to(gd.device, torch.float32) for u in uncs])
                sample = gd._unet_input(x, depth_nhwc).repeat(2, 1, 1, 1)
                eps, acts = gd.unet.forward(sample, float(t), torch.cat([unc, cond]).contiguous(), save_for_backward=False, want_acts=True)
                eu, ec, half = eps[:K], eps[K:], K
            for b in range(K):
                for k in range(3):
                    store[b][k][t_idx].copy_(acts[k][half + b])
            x = gd.ddim_step(x, eu, ec, t)
        return [([a.permute(0, 3, 1, 2).clone() for a in store[b]], x[b:b + 1].permute(0, 3, 1, 2).clone()) for b in range(K)]


def test_trajectory_rides_on_the_identity(tiny):
    from diffusionhandles_amd.background_lock import Activations
    from diffusionhandles_amd.depth_transform import normalize_depth
    acts, traj = tiny.acts, tiny.acts.trajectory
    assert isinstance(acts, list) and isinstance(acts, Activations) and len(acts) == 3
    assert traj.shape == (T, 4, S, S) and traj.dtype == torch.float32 and torch.isfinite(traj).all()
    assert torch.equal(traj[T - 1], tiny.latent[0])
    assert not torch.equal(traj[0], traj[1])
    (p_acts, p_lat), = _parent_initial_inference(tiny.gd, [tiny.noise], [normalize_depth(1.0 / tiny.depth)], [tiny.null_text],
                                                 [tiny.prompt])
    assert torch.equal(p_lat, tiny.latent) and all(torch.equal(a, b) for a, b in zip(p_acts, acts))
    # the diffuser's own call hands the same object through
    a2, lat2, _, _ = tiny.gd.initial_inference(tiny.noise, normalize_depth(1.0 / tiny.depth), tiny.null_text, tiny.prompt)
    assert torch.equal(a2.trajectory, traj) and torch.equal(lat2, tiny.latent)


def test_trajectory_of_the_batched_identity(tiny):
    from diffusionhandles_amd.depth_transform import normalize_depth
    dh, gd = tiny.dh, tiny.gd
    d2 = tiny.depth.flip(-1).contiguous()
    g = torch.Generator().manual_seed(5)
    noise2 = torch.randn(1, 4, S, S, generator=g).to(dev())
    res = dh.generate_input_images([tiny.depth, d2], [tiny.prompt, "spheres, mirrored"], [tiny.null_text, tiny.null_text],
                                   [tiny.noise, noise2])
    assert len(res) == 2 and all(len(r) == 4 for r in res)
    parent = _parent_initial_inference(gd, [tiny.noise, noise2], [normalize_depth(1.0 / tiny.depth), normalize_depth(1.0 / d2)],
                                       [tiny.null_text, tiny.null_text], [tiny.prompt, "spheres, mirrored"])
    for (_, _, acts, latent), (p_acts, p_lat) in zip(res, parent):
        traj = acts.trajectory
        assert traj.shape == (T, 4, S, S) and traj.dtype == torch.float32
        assert torch.equal(traj[T - 1], latent[0])
        assert torch.equal(latent, p_lat) and all(torch.equal(a, b) for a, b in zip(p_acts, acts))
    assert not torch.equal(res[0][2].trajectory, res[1][2].trajectory)


# ---- 4. the loop ------------------------------------------------------------------------------------------------------------
def _edit(tiny, geo, i, **kw):
    return tiny.gd.guided_inference(latents=tiny.noise, depth=geo.disp[i], uncond_embeddings=tiny.null_text, prompt=tiny.prompt,
                                    activations_orig=tiny.acts, correspondences=geo.corr[i], **kw)


def test_keep_map_of_the_rigs_edit_has_all_three_kinds_of_cells(tiny, tiny_geo):
    keep = tiny_geo.keeps[0].cpu().numpy()
    mask_cells = B.region_cells(None, tiny.masks[0][0, 0].cpu().numpy(), None, RES, S)      # a lower bound on the region, from the mask alone
    assert mask_cells.sum() > 100 and (keep[mask_cells] == 0).all() and (keep == 0).sum() >= mask_cells.sum()
    assert (keep == 1).sum() >= S * S // 4 and ((keep > 0) & (keep < 1)).sum() > 0


@pytest.mark.parametrize("grad_scale", ["static", "auto"])
def test_locked_edit_follows_the_reconstruction_outside_the_region(tiny, tiny_geo, grad_scale):
    gd, keep, traj = tiny.gd, tiny_geo.keeps[0], tiny.acts.trajectory
    old = gd.grad_scale_mode
    gd.grad_scale_mode = grad_scale
    try:
        rec = {}
        img = _edit(tiny, tiny_geo, 0, record=rec, lock=(keep, traj))          # ('auto': raises FloatingPointError on a bad step)
    finally:
        gd.grad_scale_mode = old
    assert torch.isfinite(img).all() and len(rec["step"]) == T
    zero = (keep == 0)[None].expand(4, -1, -1)
    for t_idx in range(T):
        assert _held(rec["step"][t_idx][0], traj[t_idx], keep), t_idx
        assert not torch.equal(rec["step"][t_idx][0][zero], traj[t_idx][zero]), t_idx
    assert torch.equal(gd.last_latents, rec["step"][-1])


def test_a_lock_that_keeps_nothing_is_the_unlocked_edit(tiny, tiny_geo):
    from diffusionhandles_amd.background_lock import keep_map
    gd = tiny.gd
    plain = _edit(tiny, tiny_geo, 0).clone()
    lat_plain = gd.last_latents.clone()
    keep0 = keep_map(tiny_geo.corr[0], tiny.masks[0], torch.ones(RES, RES), RES, S)          # everything released
    assert float(keep0.abs().max()) == 0.0
    img = _edit(tiny, tiny_geo, 0, lock=(keep0, tiny.acts.trajectory))
    assert torch.equal(gd.last_latents, lat_plain) and torch.equal(img, plain)
    # and the default lock does change the edit, outside its region only through the blend
    _edit(tiny, tiny_geo, 0, lock=(tiny_geo.keeps[0], tiny.acts.trajectory))
    assert not torch.equal(gd.last_latents, lat_plain)


# ---- 5. batches, items, lanes, the facade -----------------------------------------------------------------------------------
def _facade_args(t, **masks):
    return dict(depth=t.depth, prompt=t.prompt, bg_depth=t.bg_depth, null_text_emb=t.null_text, init_noise=t.noise,
                activations=t.acts, **masks)


def test_transform_foreground_batch_holds_the_identity_per_item(locked, tiny_geo):
    dh, gd, traj = locked.dh, locked.gd, locked.acts.trajectory
    imgs, disps = dh.transform_foreground_batch(**_facade_args(locked, fg_mask=locked.masks[0]), transforms=EDITS[:2])
    assert imgs.shape == (2, 3, RES, RES) and torch.isfinite(imgs).all() and len(dh.last_keep_maps) == 2
    for i in range(2):
        assert torch.equal(dh.last_keep_maps[i], tiny_geo.keeps[i]) and torch.equal(disps[i], tiny_geo.disp[i])
        assert _held(gd.last_latents[i], traj[T - 1], tiny_geo.keeps[i])
    assert not torch.equal(tiny_geo.keeps[0], tiny_geo.keeps[1]) and not torch.equal(gd.last_latents[0], gd.last_latents[1])
    # the lock reached the loop: the same batch at the diffuser, with and without it
    lat = gd.last_latents.clone()
    gd.guided_inference_batch(locked.noise, tiny_geo.disp[:2], locked.null_text, locked.prompt, locked.acts, tiny_geo.corr[:2],
                              lock=[(k, traj) for k in tiny_geo.keeps[:2]])
    assert torch.equal(gd.last_latents, lat)
    with pytest.raises(ValueError, match="transform_foreground_batch.*trajectory"):
        dh.transform_foreground_batch(**{**_facade_args(locked, fg_mask=locked.masks[0]), "activations": list(locked.acts)},
                                      transforms=EDITS[:2])


def test_transform_foreground_objects_batch_holds_the_identity_per_item(locked):
    from diffusionhandles_amd.background_lock import keep_map
    from diffusionhandles_amd.depth_transform import reproject_object_edits
    dh, gd, traj = locked.dh, locked.gd, locked.acts.trajectory
    edits = [[_t(tf) for tf in R.OCCLUDING], [EDITS[1], _t((0.0, R.Y, (0.0, 0.0, 0.0)))]]
    rel = torch.zeros(1, 1, RES, RES)
    rel[..., 480:, 480:] = 1.0
    imgs, _ = dh.transform_foreground_objects_batch(**_facade_args(locked, fg_masks=locked.masks), edits=edits, release_mask=rel)
    assert imgs.shape == (2, 3, RES, RES) and torch.isfinite(imgs).all()
    rp = reproject_object_edits(locked.depth, locked.bg_depth, locked.masks, gd.get_depth_intrinsics(device=dev()), edits,
                                device_correspondences=True)
    for i, (_, c) in enumerate(rp):
        keep = keep_map(c, locked.masks, rel, RES, S)
        assert torch.equal(dh.last_keep_maps[i], keep) and float(keep[63, 63]) == 0.0 and int((keep == 1).sum()) > S * S // 8
        assert _held(gd.last_latents[i], traj[T - 1], keep)
    # one edit of several objects, through transform_foreground_objects
    dh.transform_foreground_objects(**_facade_args(locked, fg_masks=locked.masks), transforms=edits[0], release_mask=rel)
    assert len(dh.last_keep_maps) == 1 and _held(gd.last_latents[0], traj[T - 1], dh.last_keep_maps[0])


def test_locked_and_unlocked_items_share_a_batch(tiny, tiny_geo):
    gd, traj = tiny.gd, tiny.acts.trajectory
    item = lambda i, **kw: dict(latents=tiny.noise, depth=tiny_geo.disp[i], uncond_embeddings=tiny.null_text, prompt=tiny.prompt,
                                activations_orig=tiny.acts, correspondences=tiny_geo.corr[i], **kw)
    gd.guided_inference_items([item(0), item(1)])
    plain = gd.last_latents.clone()
    gd.guided_inference_items([item(0, lock=(tiny_geo.keeps[0], traj)), item(1)])
    mixed = gd.last_latents.clone()
    assert torch.equal(mixed[1], plain[1])                                     # the unlocked item: as in the batch without any lock
    assert not torch.equal(mixed[0], plain[0]) and _held(mixed[0], traj[T - 1], tiny_geo.keeps[0])


def test_transform_foregrounds_locks_every_edit_to_its_own_image(locked, tiny_geo):
    dh, gd, traj = locked.dh, locked.gd, locked.acts.trajectory
    common = _facade_args(locked)
    edits = [dict(common, fg_mask=locked.masks[0], rot_angle=EDITS[i][0], rot_axis=EDITS[i][1], translation=EDITS[i][2]) for i in range(2)]
    edits[1]["release_mask"] = torch.ones(RES, RES)
    imgs, _ = dh.transform_foregrounds(edits)
    assert imgs.shape == (2, 3, RES, RES) and torch.equal(dh.last_keep_maps[0], tiny_geo.keeps[0])
    assert float(dh.last_keep_maps[1].abs().max()) == 0.0
    assert _held(gd.last_latents[0], traj[T - 1], tiny_geo.keeps[0])
    with pytest.raises(ValueError, match="transform_foregrounds: edit 1.*trajectory"):
        dh.transform_foregrounds([edits[0], dict(edits[1], activations=list(locked.acts))])


def test_locked_lanes_equal_the_one_stream_result(locked, tiny_geo):
    dh, gd, traj = locked.dh, locked.gd, locked.acts.trajectory
    args = _facade_args(locked, fg_mask=locked.masks[0])
    try:
        # single edits on two lanes against the same edits on one
        two, _ = dh.transform_foreground_batch(**args, transforms=EDITS[:2], streams=2)
        two = two.clone()
        one, _ = dh.transform_foreground_batch(**args, transforms=EDITS[:2], streams=1, batch=1)
        assert torch.isfinite(one).all() and torch.equal(one, two), "single edits: two lanes differ from one"
        # transform_foreground itself: the reference's parameter list, the lock by the conf key alone
        dh.transform_foreground(**args, rot_angle=EDITS[0][0], rot_axis=EDITS[0][1], translation=EDITS[0][2])
        assert torch.equal(dh.last_keep_maps[0], tiny_geo.keeps[0]) and _held(gd.last_latents[0], traj[T - 1], tiny_geo.keeps[0])
        # chunks of two edits on two lanes against the one-stream batches
        four, _ = dh.transform_foreground_batch(**args, transforms=EDITS, streams=2, batch=2)
        four = four.clone()
        for lo in (0, 2):
            one, _ = dh.transform_foreground_batch(**args, transforms=EDITS[lo:lo + 2])
            assert torch.equal(one, four[lo:lo + 2]), f"chunk at {lo}: the lane differs from the one-stream batch"
            assert _held(gd.last_latents[1], traj[T - 1], tiny_geo.keeps[lo + 1])
    finally:
        gd.release_lanes()


# ---- 6. tools/run_edit.py ---------------------------------------------------------------------------------------------------
def _run_edit_module():
    spec = importlib.util.spec_from_file_location("run_edit_tool", os.path.join(ROOT, "tools", "run_edit.py"))
    run_edit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run_edit)
    return run_edit


def test_run_scene_with_the_background_lock(tiny, tmp_path):
    """run_scene --background-lock on a one-mask scene directory with a release.png: a cache without the trajectory is
    recomputed (and rewritten with it), <edit>_keep.png is written, the second visit loads the cache."""
    from diffusionhandles_amd.scene_io import read_png, write_png
    run_edit = _run_edit_module()
    scene, out = tmp_path / "ball", tmp_path / "out"
    depth, bg, masks = R.two_spheres(RES)
    scene.mkdir()
    out.mkdir()
    np.save(scene / "depth.npy", depth[0, 0].numpy())
    np.save(scene / "bg_depth.npy", bg[0, 0].numpy())
    write_png(str(scene / "mask.png"), masks[0][0, 0].numpy())
    write_png(str(scene / "input.png"), np.full((RES, RES, 3), 0.5, dtype=np.float32))
    rel = np.zeros((RES, RES), dtype=np.float32)
    rel[:8, 504:] = 1.0                                                        # cell (0, 63)
    write_png(str(scene / "release.png"), rel)
    (scene / "prompt.txt").write_text("two spheres on a plane\n")
    a, ax, tr = R.OCCLUDING[0]
    (scene / "transforms.json").write_text(json.dumps({"move": dict(rotation_angle=a, rotation_axis=list(ax), translation=list(tr))}))
    # an identity cached before the lock existed: the reference's keys only
    f32 = lambda t: t.float().cpu().numpy()
    np.savez(out / "identity.npz", null_text_emb=f32(tiny.null_text), init_noise=f32(tiny.noise), activations1=f32(tiny.acts[0]),
             activations2=f32(tiny.acts[1]), activations3=f32(tiny.acts[2]), latent_image=f32(tiny.latent))
    args = run_edit.parse(["--scene", str(scene), "--out", str(out), "--res", str(RES), "--skip-inversion", "--background-lock",
                           "--lock-dilate", "1", "--lock-feather", "2"])
    args.mode = "pc"
    conf = tiny.dh.conf
    try:
        assert run_edit.apply_lock_args(args, conf)["background_lock_dilate"] == 1
        report = run_edit.run_scene(args, conf, lambda res: tiny.dh, str(scene), str(out), None)
        assert report["identity_from_cache"] is False and report["background_lock"] is True and report["background_lock_feather"] == 2
        assert [e["name"] for e in report["edits"]] == ["move"]
        with np.load(out / "identity.npz") as z:
            assert "trajectory" in z.files and z["trajectory"].shape == (T, 4, S, S) and z["trajectory"].dtype == np.float32
            assert np.array_equal(z["trajectory"][T - 1], z["latent_image"][0])
            saved = z["trajectory"].copy()
        keep = read_png(str(out / "move_keep.png"))
        assert keep.shape == (S, S) and keep.min() == 0 and keep.max() == 255 and keep[0, 63] == 0
        assert np.array_equal(keep, (tiny.dh.last_keep_maps[0].cpu().numpy() * 255.0).astype(np.uint8))          # (write_png truncates)
        assert read_png(str(out / "move.png")).shape == (RES, RES, 3)
        # the second visit: the cache serves, with its trajectory
        p = run_edit.prepare_scene(args, str(scene), str(out), None)
        *_, acts, rep2 = run_edit.scene_identity(args, tiny.dh, p, str(out))
        assert rep2["identity_from_cache"] is True and np.array_equal(acts.trajectory.cpu().numpy(), saved)
    finally:
        for k in ("background_lock", "background_lock_dilate", "background_lock_feather"):
            conf.pop(k, None)
