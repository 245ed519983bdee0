"""GPU: several rigid bodies per edit (dh_reproject_object_edits, depth_transform.reproject_object_edits,
DiffusionHandles.transform_foreground_objects[_batch]) -- one object is dh_reproject_edits bit for bit; two objects against
the test-side reference tests/multi_object_ref.py, integer outputs bit-exact; object order, dropped empty masks,
determinism; the loop level on the TINY rig.  The C entries write into outputs that are NaN / 0xFF before the call."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_object_ref as R  # noqa: E402

from diffusionhandles_amd.synthetic import TRANSFORMS, make_scene  # noqa: E402

pytestmark = pytest.mark.gpu
Y = torch.tensor([0.0, 1.0, 0.0])


def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _t(tf):
    a, ax, tr = tf
    return (float(a), torch.tensor(ax, dtype=torch.float32), torch.tensor(tr, dtype=torch.float32))


def _abi(depth, bg, masks, edits, entry):
    """The C entry `entry` ("edits": dh_reproject_edits, one mask; "objects": dh_reproject_object_edits) on masks that are
    not empty, every output buffer poisoned (NaN / 0xFF) before the call.  Returns the buffers and the counts."""
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    L = _lib.lib()
    st = _lib.stream_ptr()
    res, M, K = depth.shape[-1], len(masks), len(edits)
    R2 = res * res
    d = depth.to(dev(), torch.float32).contiguous()
    b = bg.to(dev(), torch.float32).contiguous()
    gx, gy = DT._grids(res, res, dev())
    intr = D.intrinsics_f32()
    ifx, ify = DT._inv_focal(intr)
    fx, fy = float(intr[0, 0]), float(intr[1, 1])
    fg_pix = torch.full((R2,), -1, dtype=torch.int32, device=dev())
    n_dev = torch.full((M,), -1, dtype=torch.int32, device=dev())
    ws_small = torch.empty(4096, dtype=torch.uint8, device=dev())
    start = [0]
    for m, mask in enumerate(masks):
        m8 = (mask.to(dev()) != 0).to(torch.uint8).contiguous().view(-1)
        _lib.check(L.dh_fg_pixel_list(_lib.ptr(m8), res, _lib.ptr(fg_pix[start[-1]:]), _lib.ptr(n_dev[m:]), _lib.ptr(ws_small),
                                      ws_small.numel(), st), "dh_fg_pixel_list")
        start.append(start[-1] + int(m8.sum().item()))
    assert n_dev.tolist() == [start[m + 1] - start[m] for m in range(M)] and min(n_dev.tolist()) > 0
    n_fg = start[-1]
    assert int((fg_pix >= 0).sum()) == n_fg                              # no slice wrote beyond its count
    nb = ctypes.c_size_t()
    if entry == "edits":
        assert M == 1
        _lib.check(L.dh_reproject_workspace_bytes(res, n_fg, K, ctypes.byref(nb)))
    else:
        _lib.check(L.dh_reproject_objects_workspace_bytes(res, n_fg, K, M, ctypes.byref(nb)))
    ws = torch.full((nb.value,), 0xFF, dtype=torch.uint8, device=dev())
    nan = float("nan")
    o = SimpleNamespace(
        zmap=torch.full((K, res, res), nan, device=dev()), disp=torch.full((K, res, res), nan, device=dev()),
        raw=torch.full((K, res, res), 0xFF, dtype=torch.uint8, device=dev()),
        clean=torch.full((K, res, res), 0xFF, dtype=torch.uint8, device=dev()),
        vis=torch.full((K, n_fg), 0xFF, dtype=torch.uint8, device=dev()),
        txy=torch.full((K, n_fg, 2), -1, dtype=torch.int32, device=dev()),
        corr=torch.full((K, n_fg, 4), -1, dtype=torch.int64, device=dev()),
        counts=torch.full((K, 4), -1, dtype=torch.int32, device=dev()), obj_start=np.asarray(start, dtype=np.int32),
        fg_pix=fg_pix[:n_fg], n_fg=n_fg)
    rows = np.ascontiguousarray(DT._xform_rows([_t(tf) for tfs in edits for tf in tfs]))
    assert rows.shape == (K * M, 8)
    xf = rows.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    outs = (_lib.ptr(o.zmap), _lib.ptr(o.raw), _lib.ptr(o.clean), _lib.ptr(o.disp), _lib.ptr(o.vis), _lib.ptr(o.txy),
            _lib.ptr(o.corr), _lib.ptr(o.counts), _lib.ptr(ws), nb.value, st)
    if entry == "edits":
        _lib.check(L.dh_reproject_edits(_lib.ptr(d), _lib.ptr(b), _lib.ptr(fg_pix), n_fg, res, _lib.ptr(gx), _lib.ptr(gy), ifx, ify,
                                        fx, fy, K, xf, None, *outs), "dh_reproject_edits")
    else:
        _lib.check(L.dh_reproject_object_edits(_lib.ptr(d), _lib.ptr(b), _lib.ptr(fg_pix), n_fg, M,
                                               o.obj_start.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), res, _lib.ptr(gx),
                                               _lib.ptr(gy), ifx, ify, fx, fy, K, xf, None, *outs), "dh_reproject_object_edits")
    torch.cuda.synchronize()
    # everything the contract promises was written, nothing else
    assert torch.isfinite(o.disp).all() and not torch.isnan(o.zmap).any()
    assert int(o.raw.max()) <= 1 and int(o.clean.max()) <= 1 and int(o.vis.max()) <= 1
    assert int(o.txy.min()) >= 0 and int(o.txy.max()) < res
    o.counts_h = o.counts.cpu()
    assert (o.counts_h[:, 3] >= 0).all()
    for e in range(K):
        n = int(o.counts_h[e, 0])
        assert 0 < n <= int(o.counts_h[e, 1]) <= n_fg
        assert int(o.corr[e, :n].min()) >= 0 and int(o.corr[e, :n].max()) < res and bool((o.corr[e, n:] == -1).all())
    return o


# ---- 1. one object is dh_reproject_edits -----------------------------------------------------------------------------------
def test_one_object_is_bit_identical_to_reproject_edits():
    """make_scene(256), the first three TRANSFORMS: the new C entry with one object, the old C entry, and both Python calls
    give the same bits in every output."""
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    depth, bg, mask = make_scene(256)
    tfs = [(TRANSFORMS[i][0], (0.0, 1.0, 0.0), TRANSFORMS[i][1]) for i in range(3)]
    old = _abi(depth, bg, [mask], [[tf] for tf in tfs], "edits")
    new = _abi(depth, bg, [mask], [[tf] for tf in tfs], "objects")
    K = D.intrinsics_f32()
    args = (depth.to(dev()), bg.to(dev()), mask.to(dev()))
    out_e, dbg_e = DT.reproject_edits(*args, K, [_t(tf) for tf in tfs], return_debug=True)
    out_o, dbg_o = DT.reproject_object_edits(args[0], args[1], [args[2]], K, [[_t(tf)] for tf in tfs], return_debug=True)
    assert dbg_o["obj_start"].tolist() == [0, old.n_fg]
    for got in (new, SimpleNamespace(zmap=dbg_e["zmap"], raw=dbg_e["raw_mask"], clean=dbg_e["clean_mask"], vis=dbg_e["vis"],
                                     txy=dbg_e["target_xy"], counts_h=dbg_e["counts"], fg_pix=dbg_e["fg_pix"],
                                     disp=torch.cat([d[0] for d, _ in out_e]), corr=dbg_e["corr_dev"]),
                SimpleNamespace(zmap=dbg_o["zmap"], raw=dbg_o["raw_mask"], clean=dbg_o["clean_mask"], vis=dbg_o["vis"],
                                txy=dbg_o["target_xy"], counts_h=dbg_o["counts"], fg_pix=dbg_o["fg_pix"],
                                disp=torch.cat([d[0] for d, _ in out_o]), corr=dbg_o["corr_dev"])):
        assert torch.equal(got.counts_h, old.counts_h)
        assert torch.equal(got.disp, old.disp) and torch.equal(got.zmap, old.zmap)
        assert torch.equal(got.raw, old.raw) and torch.equal(got.clean, old.clean)
        assert torch.equal(got.vis, old.vis) and torch.equal(got.txy, old.txy) and torch.equal(got.fg_pix, old.fg_pix)
        for e in range(3):
            n = int(old.counts_h[e, 0])
            assert n > 1000 and torch.equal(got.corr[e, :n], old.corr[e, :n])
    for e in range(3):
        assert torch.equal(out_o[e][1], out_e[e][1]) and torch.equal(out_o[e][1], old.corr[e, :int(old.counts_h[e, 0])].cpu())


# ---- 2. two objects against the reference helper ---------------------------------------------------------------------------
EDITS2 = [R.OCCLUDING,
          [(15.0, R.Y, (0.1, 0.0, -0.05)), (-20.0, R.Y, (-0.15, 0.05, 0.1))],
          [(25.0, R.Y, (0.2, 0.0, 0.0)), (0.0, R.Y, (0.0, 0.0, 0.0))]]
GENERAL = [[(25.0, (0.3, 0.9, -0.2), (0.1, -0.05, 0.2)), (-20.0, R.Y, (-0.15, 0.05, 0.1))]]


def _check_against_helper(o, e, disp_r, corr_r, dbg_r):
    n = int(o.counts_h[e, 0])
    assert np.array_equal(o.corr[e, :n].cpu().numpy(), corr_r.numpy()), f"edit {e}: correspondences (order included)"
    assert np.array_equal(o.zmap[e].cpu().numpy(), dbg_r["zmap"]), f"edit {e}: zmap"
    assert np.array_equal(o.raw[e].cpu().numpy() != 0, dbg_r["raw_mask"]), f"edit {e}: raw mask"
    assert np.array_equal(o.clean[e].cpu().numpy() != 0, dbg_r["cleaned"] != 0), f"edit {e}: clean mask"
    assert np.array_equal(o.vis[e].cpu().numpy() != 0, dbg_r["vis"]), f"edit {e}: vis"
    assert int(o.counts_h[e, 1]) == int(dbg_r["vis"].sum())
    err = float((o.disp[e].cpu() - disp_r[0, 0]).abs().max())
    print(f"edit {e}: {n} correspondences, disparity max abs err {err:.2e}")
    assert err < 2e-3, f"edit {e}: disparity {err}"


@pytest.mark.parametrize("res", [128, 256])
def test_two_objects_against_the_reference_helper(res):
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    depth, bg, masks = R.two_spheres(res)
    o = _abi(depth, bg, masks, EDITS2, "objects")
    per_obj = []
    for e, tfs in enumerate(EDITS2):
        disp_r, corr_r, dbg_r = R.transform_objects(depth, bg, masks, tfs)
        _check_against_helper(o, e, disp_r, corr_r, dbg_r)
        s = dbg_r["obj_start"]
        per_obj.append([int(dbg_r["vis"][s[j]:s[j + 1]].sum()) for j in range(2)])
    assert min(per_obj[1]) > 100 and per_obj[0][1] < per_obj[2][1] / 2         # the occluding edit hides object 1
    # the Python call returns the same bits
    out, dbg = DT.reproject_object_edits(depth.to(dev()), bg.to(dev()), [m.to(dev()) for m in masks], D.intrinsics_f32(),
                                         [[_t(tf) for tf in tfs] for tfs in EDITS2], return_debug=True)
    assert dbg["obj_start"].tolist() == o.obj_start.tolist()
    for e in range(3):
        assert out[e][1].device.type == "cpu" and out[e][1].dtype == torch.int64
        assert torch.equal(out[e][1], o.corr[e, :int(o.counts_h[e, 0])].cpu()) and torch.equal(out[e][0][0, 0], o.disp[e])
    assert torch.equal(dbg["zmap"], o.zmap) and torch.equal(dbg["vis"], o.vis) and torch.equal(dbg["clean_mask"], o.clean)
    # a general axis for object 0: exact against the written-out dot-product order (oracle.depth_ref.DOT_ORDER)
    g = _abi(depth, bg, masks, GENERAL, "objects")
    D.DOT_ORDER = "explicit"
    try:
        disp_r, corr_r, dbg_r = R.transform_objects(depth, bg, masks, GENERAL[0])
    finally:
        D.DOT_ORDER = "blas"
    _check_against_helper(g, 0, disp_r, corr_r, dbg_r)


# ---- 3. object order, dropped masks, determinism ----------------------------------------------------------------------------
def test_three_masks_at_512_object_order_and_determinism():
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    res = 512
    depth, bg, masks = R.two_spheres(res)
    # the scene has no exact depth tie between the objects (else the order would decide a pixel)
    _, _, dbg_r = R.transform_objects(depth, bg, masks, R.OCCLUDING)
    assert R.z_ties_between_objects(dbg_r, res=res) == 0
    K = D.intrinsics_f32()
    d, b = depth.to(dev()), bg.to(dev())
    m0, m1, none = masks[0].to(dev()), masks[1].to(dev()), torch.zeros_like(masks[0]).to(dev())
    t0, t1 = (_t(tf) for tf in R.OCCLUDING)
    tz = _t((33.0, R.Y, (0.3, 0.3, 0.3)))                               # the transform of the empty mask: dropped with it
    run = lambda ms, tfs: DT.reproject_object_edits(d, b, ms, K, [tfs], return_debug=True)
    (two, dbg2), (three, dbg3) = run([m0, m1], [t0, t1]), run([m0, none, m1], [t0, tz, t1])
    again, dbg3b = run([m0, none, m1], [t0, tz, t1])
    swapped, dbgs = run([m1, none, m0], [t1, tz, t0])
    assert dbg3["obj_start"].tolist() == [0, 20069, 20069 + 15361] == dbg2["obj_start"].tolist()
    assert dbgs["obj_start"].tolist() == [0, 15361, 20069 + 15361]
    corr = three[0][1]
    assert np.array_equal(corr.numpy(), R.transform_objects(depth, bg, masks, R.OCCLUDING)[1].numpy())
    for k in ("zmap", "raw_mask", "clean_mask", "vis", "target_xy", "fg_pix"):
        assert torch.equal(dbg3[k], dbg2[k]), k                          # the empty mask changes nothing
        assert torch.equal(dbg3[k], dbg3b[k]), k                         # two identical calls: identical bytes
    assert torch.equal(corr, two[0][1]) and torch.equal(three[0][0], two[0][0])
    assert torch.equal(corr, again[0][1]) and torch.equal(three[0][0], again[0][0]) and torch.equal(dbg3["counts"], dbg3b["counts"])
    # swapped objects: the same picture, the same pairs, the blocks permuted
    for k in ("zmap", "raw_mask", "clean_mask"):
        assert torch.equal(dbgs[k], dbg3[k]), k
    cs = swapped[0][1]
    assert len(cs) == len(corr) and set(map(tuple, cs.tolist())) == set(map(tuple, corr.tolist()))
    in0 = masks[0][0, 0][corr[:, 1], corr[:, 0]] > 0.5
    n0 = int(in0.sum())
    assert 0 < n0 < len(corr) and bool(in0[:n0].all()) and not bool(in0[n0:].any())
    assert torch.equal(cs, torch.cat([corr[n0:], corr[:n0]]))
    # all masks empty: the empty-mask result of reproject_edits
    (disp, c), = DT.reproject_object_edits(d, b, [none, none], K, [[t0, t1]])
    assert c.shape == (0, 4) and torch.equal(disp.cpu(), D.normalize_depth(1.0 / depth)[0])


# ---- 4. the loop level, on the TINY rig of tests/test_edit_items_gpu.py ------------------------------------------------------
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
    res = 512
    depth, bg, masks = R.two_spheres(res)
    depth, bg, masks = depth.to(dev()), bg.to(dev()), [m.to(dev()) for m in masks]
    g = torch.Generator().manual_seed(11)
    noise = torch.randn(1, 4, res // 8, res // 8, generator=g).to(dev())
    Dm = dh.diffuser.unet.cfg["cross_attention_dim"]
    unc = (dh.diffuser._encode([""])[None].expand(50, -1, -1, -1) + 0.05 * torch.randn(50, 1, 77, Dm, generator=g).to(dev())).contiguous()
    prompt = "two spheres on a plane"
    null_text, noise, acts, _ = dh.generate_input_image(depth, prompt, unc, noise)
    return SimpleNamespace(dh=dh, gd=dh.diffuser, depth=depth, bg_raw=bg, bg_depth=dh.set_foreground(depth, masks, bg), masks=masks,
                           prompt=prompt, null_text=null_text, noise=noise, acts=acts)


def _args(t, masks):
    return dict(depth=t.depth, prompt=t.prompt, bg_depth=t.bg_depth, null_text_emb=t.null_text, init_noise=t.noise,
                activations=t.acts, **masks)


def test_set_foreground_takes_a_list_of_masks(tiny):
    """A list of masks is their union; one tensor behaves as before."""
    dh, m = tiny.dh, tiny.masks
    assert tiny.bg_depth.shape == (1, 1, 512, 512) and torch.isfinite(tiny.bg_depth).all()
    assert torch.equal(tiny.bg_depth, dh.set_foreground(tiny.depth, ((m[0] + m[1]) > 0).float(), tiny.bg_raw))
    one = dh.set_foreground(tiny.depth, m[0], tiny.bg_raw)
    assert torch.equal(one, dh.set_foreground(tiny.depth, [m[0]], tiny.bg_raw)) and not torch.equal(one, tiny.bg_depth)


def test_transform_foreground_objects_on_the_tiny_rig(tiny):
    from diffusionhandles_amd.depth_transform import reproject_object_edits
    dh, gd = tiny.dh, tiny.gd
    t0, t1 = (_t(tf) for tf in R.OCCLUDING)
    # one mask: transform_foreground
    img1, disp1 = dh.transform_foreground(**_args(tiny, dict(fg_mask=tiny.masks[0])), rot_angle=t0[0], rot_axis=t0[1], translation=t0[2])
    img1, lat1 = img1.clone(), gd.last_latents.clone()
    img1o, disp1o = dh.transform_foreground_objects(**_args(tiny, dict(fg_masks=[tiny.masks[0]])), transforms=[t0])
    assert torch.equal(img1o, img1) and torch.equal(disp1o, disp1) and torch.equal(gd.last_latents, lat1)
    # two masks
    img2, disp2 = dh.transform_foreground_objects(**_args(tiny, dict(fg_masks=tiny.masks)), transforms=[t0, t1])
    img2, lat2 = img2.clone(), gd.last_latents.clone()
    assert img2.shape == img1.shape and torch.isfinite(img2).all()
    (d, c), = reproject_object_edits(tiny.depth, tiny.bg_depth, tiny.masks, gd.get_depth_intrinsics(device=dev()), [[t0, t1]])
    assert torch.equal(d, disp2) and len(c) > 10000
    ref = gd.guided_inference(latents=tiny.noise, depth=d, uncond_embeddings=tiny.null_text, prompt=tiny.prompt,
                              activations_orig=tiny.acts, correspondences=c)
    assert torch.equal(ref, img2) and torch.equal(gd.last_latents, lat2)
    assert not torch.equal(img2, img1) and float((lat2 - lat1).abs().max()) > 1e-3          # not the edit of object 0 alone
    # save_denoising_steps travels as in transform_foreground
    dh.conf.guided_diffuser.save_denoising_steps = True
    try:
        out = dh.transform_foreground_objects(**_args(tiny, dict(fg_masks=tiny.masks)), transforms=[t0, t1])
    finally:
        dh.conf.guided_diffuser.save_denoising_steps = False
    assert len(out) == 3 and torch.equal(out[0], img2) and set(out[2]) == {"opt", "post-opt"}


def test_transform_foreground_objects_batch_on_the_tiny_rig(tiny):
    from diffusionhandles_amd.depth_transform import reproject_object_edits
    dh, gd = tiny.dh, tiny.gd
    edits = [[_t(tf) for tf in tfs] for tfs in EDITS2[:2]]
    imgs, disps = dh.transform_foreground_objects_batch(**_args(tiny, dict(fg_masks=tiny.masks)), edits=edits)
    imgs, lat = imgs.clone(), gd.last_latents.clone()
    assert imgs.shape == (2, 3, 512, 512) and len(disps) == 2 and torch.isfinite(imgs).all() and not torch.equal(imgs[0], imgs[1])
    res = reproject_object_edits(tiny.depth, tiny.bg_depth, tiny.masks, gd.get_depth_intrinsics(device=dev()), edits,
                                 device_correspondences=True)
    for (d, _), got in zip(res, disps):
        assert torch.equal(d, got)
    ref = gd.guided_inference_batch(tiny.noise, [d for d, _ in res], tiny.null_text, tiny.prompt, tiny.acts, [c for _, c in res])
    assert torch.equal(ref, imgs) and torch.equal(gd.last_latents, lat)
    dh.conf.depth_transform_mode = "mesh"
    try:
        with pytest.raises(NotImplementedError):
            dh.transform_foreground_objects_batch(**_args(tiny, dict(fg_masks=tiny.masks)), edits=edits)
    finally:
        dh.conf.depth_transform_mode = "pc"
