"""GPU: a weight per object for the guidance energy (dh_energy_plan_build_objects, dh_energy_fwd_bwd_planned_objects[_batch],
losses.EnergyPlan(object_weights=...), prepare_guidance / transform_foreground_objects[_batch] with object_weights) against the
test-side reference tests/object_weights_ref.py on the two-sphere scene at 256 pixels, grid 32: the smallest setup in which the
objects share target cells (35) and have unequal pair counts (4155 / 795).  Every output is NaN before the call."""
import contextlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_object_ref as R  # noqa: E402
import object_weights_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu
GRID = W.GRID
WEIGHTS = ((7.5, 1.5), (7.5, 0.0), (0.0, 1.5))
DTYPES = (torch.float16, torch.bfloat16)
GRAD_DTYPES = (torch.float16, torch.bfloat16, torch.float32)
SCALE = 64.0


def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


_PC = {}


def _pc(name, keep=None, masks=(0, 1)):
    """process_correspondences of the edit `name` with the label image of the masks `masks`; keep: the objects whose
    correspondences stay."""
    key = (name, keep, masks)
    if key not in _PC:
        from diffusionhandles_amd.losses import object_label_image, process_correspondences
        corr, label, _, _ = W.scene(name)
        if keep is not None:
            c = corr.numpy()
            corr = corr[torch.from_numpy(np.isin(label[c[:, 1], c[:, 0]].astype(np.int64) - 1, list(keep)))]
        _, _, m = R.two_spheres(W.RES)
        lab = object_label_image([m[i].to(dev()) for i in masks])
        _PC[key] = process_correspondences(corr, W.RES, 0, grid=GRID, device=dev(), object_labels=lab)
    return _PC[key]


def _maps(C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    act = torch.randn(GRID, GRID, C, generator=g).to(dtype).to(dev())
    orig = torch.randn(GRID, GRID, C, generator=g).to(dtype).to(dev())
    return act, orig


def _call(act, orig, plan, fw, bw, grad_dtype):
    """One planned call into a NaN-filled gradient and loss; both finite afterwards."""
    from diffusionhandles_amd import _lib
    C = act.shape[-1]
    grad = torch.full((GRID, GRID, C), float("nan"), dtype=grad_dtype, device=dev())
    loss = torch.full((3,), float("nan"), device=dev())
    ws, wsb = plan.workspace(C)
    L = _lib.lib()
    entry = L.dh_energy_fwd_bwd_planned_objects if plan.weighted else L.dh_energy_fwd_bwd_planned
    dl = plan.dl
    _lib.check(entry(_lib.ptr(act), _lib.ptr(orig), _lib.DTYPE_CODE[act.dtype], C, GRID, _lib.ptr(plan.buf), plan.nbytes, plan.n_pairs,
                     _lib.ptr(dl["bg_orig"]), dl["bg_orig"].numel(), _lib.ptr(dl["bg_trans"]), dl["bg_trans"].numel(), fw, bw, SCALE,
                     _lib.ptr(loss), _lib.ptr(grad), _lib.DTYPE_CODE[grad_dtype], _lib.ptr(ws), wsb, _lib.stream_ptr()), "planned call")
    torch.cuda.synchronize()
    assert torch.isfinite(grad).all() and torch.isfinite(loss).all()
    return loss, grad


def _eps(grad_dtype):
    return 2.0 ** -8 if grad_dtype == torch.bfloat16 else 2.0 ** -10


def _check_grad(got, ref, grad_dtype, what):
    """got: the kernel's gradient (already times SCALE); ref: float64 [h,w,C] of the unscaled energy."""
    ref = ref.double().cpu() * SCALE
    err = float((got.double().cpu() - ref).abs().max())
    tol = _eps(grad_dtype) * float(ref.abs().max()) + 1e-9
    print(f"{what}: gradient max abs err {err:.3e} (tolerance {tol:.3e}, max |ref| {float(ref.abs().max()):.3e})")
    assert err <= tol, what


def _check_loss(got, ref, what):
    got = [float(v) for v in got.cpu()]
    print(f"{what}: loss {got} / reference {list(ref)}")
    for g, r in zip(got, ref):
        assert abs(g - r) <= 1e-4 * abs(r), (what, got, ref)


def _ordered(t):
    """the bit patterns of a float tensor as integers that are monotone in its value (ulp distance = difference)"""
    i = t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).to(torch.int64)
    top = 1 << (8 * t.element_size() - 1)
    return torch.where(i < 0, -(i + top), i)


# ---- 4. the weighted single call against the reference -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["occluding", "apart"])
@pytest.mark.parametrize("C", [64, 320])
@pytest.mark.parametrize("dtype", DTYPES)
def test_weighted_call_against_the_reference(dtype, C, name):
    from diffusionhandles_amd.losses import EnergyPlan
    _, _, cells, objects = W.scene(name)
    pc = _pc(name)
    assert np.array_equal(pc["object"], objects) and np.array_equal(pc["transformed_x"], cells["transformed_x"])
    assert name != "occluding" or np.bincount(pc["object"]).tolist() == [4155, 795]
    assert torch.equal(pc.device_lists["pair_obj"].cpu(), torch.from_numpy(objects).to(torch.uint8))
    act, orig = _maps(C, dtype, 100 + C)
    for ow in ("equal", [0.25, 2.0]):
        plan = EnergyPlan(pc, GRID, dev(), object_weights=ow)
        assert plan.weighted and plan.counts.tolist() == np.bincount(objects).tolist()
        w = [1.0, 1.0] if ow == "equal" else ow
        for fw, bw in WEIGHTS:
            ref_loss, ref_grad = W.energy_and_grad(act, orig, cells, objects, w, fw, bw)
            for gdt in GRAD_DTYPES:
                what = f"{name} C {C} {dtype} -> {gdt}, weights {ow}, (fw, bw) = ({fw}, {bw})"
                loss, grad = _call(act, orig, plan, fw, bw, gdt)
                _check_loss(loss, ref_loss, what)
                _check_grad(grad, ref_grad, gdt, what)


# ---- 5. weights (1, 0) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 320])
@pytest.mark.parametrize("grad_dtype", GRAD_DTYPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_one_zero_is_the_unweighted_call_on_object_0(dtype, grad_dtype, C):
    """Against dh_energy_fwd_bwd_planned on a plan of object 0's pairs with the union's background lists: within one unit in the last
    place of the gradient type; cells that only object 1 targets get exactly 0."""
    from diffusionhandles_amd.losses import EnergyPlan, ProcessedCorrespondences
    pc = _pc("occluding")
    _, _, cells, objects = W.scene("occluding")
    dl = dict(pc.device_lists)
    dl["pairs"] = dl["pairs"][dl["pair_obj"] == 0].contiguous()
    del dl["pair_obj"]
    pc0 = ProcessedCorrespondences(pc)
    pc0.device_lists = dl
    plan0 = EnergyPlan(pc0, GRID, dev())
    plan = EnergyPlan(pc, GRID, dev(), object_weights=[1.0, 0.0])
    assert not plan0.weighted and plan0.n_pairs == 4155 and plan.weighted and plan.n_pairs == 4950
    act, orig = _maps(C, dtype, 200 + C)
    only1 = sorted(W.target_cells(cells, objects, 1) - W.target_cells(cells, objects, 0))
    bg_t = set((cells["background_y_trans"] * GRID + cells["background_x_trans"]).tolist())
    assert len(only1) == 25 and not (set(only1) & bg_t)
    for fw, bw in WEIGHTS:
        _, g0 = _call(act, orig, plan0, fw, bw, grad_dtype)
        _, g1 = _call(act, orig, plan, fw, bw, grad_dtype)
        ulps = int((_ordered(g1) - _ordered(g0)).abs().max())
        print(f"C {C} {dtype} -> {grad_dtype} (fw, bw) = ({fw}, {bw}): largest distance {ulps} ulp, max |g| {float(g0.abs().max()):.3e}")
        assert ulps <= 1
        assert fw == 0.0 or float(g0.abs().max()) > 0
        assert bool((g1.view(GRID * GRID, C)[only1] == 0).all())
    # with equal weights those cells do get a gradient
    _, ge = _call(act, orig, EnergyPlan(pc, GRID, dev(), object_weights="equal"), 7.5, 1.5, grad_dtype)
    assert bool((ge.view(GRID * GRID, C)[only1] != 0).any(dim=-1).all())


# ---- 6. w_m = N_m is the area weighting ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["occluding", "apart"])
@pytest.mark.parametrize("C", [64, 320])
@pytest.mark.parametrize("dtype", DTYPES)
def test_weights_equal_to_the_counts_give_the_unweighted_energy(dtype, C, name):
    from diffusionhandles_amd.losses import EnergyPlan
    pc = _pc(name)
    counts = np.bincount(pc["object"]).astype(np.float64).tolist()
    plain = EnergyPlan(pc, GRID, dev())
    plan = EnergyPlan(pc, GRID, dev(), object_weights=counts)
    assert plan.weighted and not plain.weighted
    act, orig = _maps(C, dtype, 300 + C)
    for fw, bw in WEIGHTS:
        for gdt in GRAD_DTYPES:
            what = f"{name} C {C} {dtype} -> {gdt} (fw, bw) = ({fw}, {bw}), w = N"
            l0, g0 = _call(act, orig, plain, fw, bw, gdt)
            l1, g1 = _call(act, orig, plan, fw, bw, gdt)
            _check_loss(l1, [float(v) for v in l0.cpu()], what)
            _check_grad(g1, g0.double() / SCALE, gdt, what)


# ---- 7. determinism; the batched entry --------------------------------------------------------------------------------------------
def _batch_plans():
    """8 weighted plans: the two edits under several weights; item 1 has no pairs at all, item 2 no pairs of object 1 (its weight is
    renormalised away)."""
    from diffusionhandles_amd.losses import EnergyPlan
    spec = [("occluding", None, "equal"), ("occluding", (), [1.0, 1.0]), ("occluding", (0,), [1.0, 3.0]), ("apart", None, [2.0, 0.5]),
            ("apart", None, "equal"), ("occluding", None, [0.0, 1.0]), ("apart", None, [1.0, 0.0]), ("occluding", None, [3.0, 1.0])]
    plans = [EnergyPlan(_pc(n, keep), GRID, dev(), object_weights=w) for n, keep, w in spec]
    assert all(p.weighted for p in plans) and plans[1].n_pairs == 0 and plans[2].counts.tolist() == [4155, 0]
    assert plans[2].omega.tolist() == [1.0, 0.0]
    return plans


@pytest.mark.parametrize("dtype,grad_dtype,C", [(torch.float16, torch.float16, 320), (torch.bfloat16, torch.float32, 320),
                                                (torch.float16, torch.bfloat16, 64), (torch.bfloat16, torch.bfloat16, 64)])
def test_weighted_calls_are_reproducible_and_the_batch_is_the_single_call(dtype, grad_dtype, C):
    from diffusionhandles_amd.losses import EnergyPlan, energy_and_grad_planned, energy_and_grad_planned_batch
    plans = _batch_plans()
    g = torch.Generator(device=dev()).manual_seed(400 + C)
    # the item whose object 1 has no pairs is the (1, 0) plan on the same pairs
    act, orig = _maps(C, dtype, 400 + C)
    same = EnergyPlan(_pc("occluding", (0,)), GRID, dev(), object_weights=[1.0, 0.0])
    la, ga = _call(act, orig, plans[2], 7.5, 1.5, grad_dtype)
    lb, gb = _call(act, orig, same, 7.5, 1.5, grad_dtype)
    assert torch.equal(ga, gb) and torch.equal(la, lb)
    for K in (1, 3, 8):
        cur_buf = torch.randn(2 * K + 1, GRID, GRID, C, generator=g, device=dev()).to(dtype)
        origs = list(torch.randn(K, GRID, GRID, C, generator=g, device=dev()).to(dtype))
        cur = [cur_buf[2 * e + 1] for e in range(K)]
        fw = [0.0 if e == 3 else 7.5 + e for e in range(K)]
        bw = [0.0 if e == 4 else 1.5 + 0.25 * e for e in range(K)]
        scale = [256.0 if e % 2 else 64.0 for e in range(K)]
        nan = lambda: torch.full((2 * K, GRID, GRID, C), float("nan"), dtype=grad_dtype, device=dev())
        ref, again, out = nan(), nan(), nan()
        ref_loss, again_loss = [], []
        for buf, losses in ((ref, ref_loss), (again, again_loss)):
            for e in range(K):
                l, _ = energy_and_grad_planned(cur[e], origs[e], plans[e], fw[e], bw[e], grad_scale=scale[e], want_loss=True,
                                               out=buf[2 * e], grad_dtype=grad_dtype)
                losses.append(l)
        loss, grads = energy_and_grad_planned_batch(cur, origs, plans[:K], fw, bw, scale, want_loss=True,
                                                    outs=[out[2 * e] for e in range(K)], grad_dtype=grad_dtype)
        torch.cuda.synchronize()
        for e in range(K):
            assert torch.isfinite(ref[2 * e]).all() and torch.isfinite(ref_loss[e]).all(), (K, e)
            assert torch.equal(again[2 * e], ref[2 * e]) and torch.equal(again_loss[e], ref_loss[e]), f"K = {K}, item {e}: not reproducible"
            assert torch.equal(out[2 * e], ref[2 * e]), f"K = {K}, item {e}: the batch differs from the single call"
            assert torch.equal(loss[e], ref_loss[e]), f"K = {K}, item {e}: loss {loss[e].tolist()} != {ref_loss[e].tolist()}"
            assert torch.isnan(out[2 * e + 1]).all() and torch.isnan(ref[2 * e + 1]).all()          # the maps between the items
        if K >= 3:
            assert float(ref_loss[1][1]) == 0 and float(ref[2].abs().max()) > 0                       # no pairs: background only
    # a batch that mixes weighted and unweighted plans is refused by the one-launch entry (the loop routes it item by item)
    with pytest.raises(ValueError, match="weighted"):
        energy_and_grad_planned_batch(cur[:2], origs[:2], [plans[0], EnergyPlan(_pc("apart"), GRID, dev())], fw[:2], bw[:2], scale[:2])


def test_library_rejects_bad_weights_before_any_launch():
    import ctypes
    from diffusionhandles_amd import _lib
    L = _lib.lib()
    pc = _pc("occluding")
    dl = pc.device_lists
    n = int(dl["pairs"].shape[0])
    nb = ctypes.c_size_t()
    _lib.check(L.dh_energy_plan_objects_bytes(GRID, n, ctypes.byref(nb)))
    buf = torch.zeros(nb.value, dtype=torch.uint8, device=dev())

    def build(M, w, counts, nbytes=nb.value):
        return L.dh_energy_plan_build_objects(_lib.ptr(dl["pairs"]), _lib.ptr(dl["pair_obj"]), n, _lib.ptr(dl["bg_trans"]),
                                              dl["bg_trans"].numel(), GRID, M, (ctypes.c_float * len(w))(*w),
                                              (ctypes.c_int32 * len(counts))(*counts), _lib.ptr(buf), nbytes, _lib.stream_ptr())
    assert build(2, [1.0, 1.0], [4155, 795]) == 0
    torch.cuda.synchronize()
    good = buf.clone()
    for M, w, counts in ((0, [1.0], [n]), (9, [1.0] * 9, [n] + [0] * 8), (2, [1.0, -1.0], [4155, 795]),
                         (2, [float("nan"), 1.0], [4155, 795]), (2, [float("inf"), 1.0], [4155, 795]), (2, [0.0, 0.0], [4155, 795]),
                         (3, [0.0, 0.0, 5.0], [4155, 795, 0]), (2, [1.0, 1.0], [4155, 794])):
        assert build(M, w, counts) != 0, (M, w, counts)
        assert L.dh_last_error()
    assert build(2, [1.0, 1.0], [4155, 795], nb.value - 4096) != 0
    # grid 128: the dedupe histogram (grid^2 + 256 ints of LDS) passes 64 KB -- both builds refuse it, before their first memset
    too_large = b"grid too large for the dedupe histogram"
    assert L.dh_energy_plan_build_objects(_lib.ptr(dl["pairs"]), _lib.ptr(dl["pair_obj"]), n, _lib.ptr(dl["bg_trans"]),
                                          dl["bg_trans"].numel(), 128, 2, (ctypes.c_float * 2)(1.0, 1.0),
                                          (ctypes.c_int32 * 2)(4155, 795), _lib.ptr(buf), nb.value, _lib.stream_ptr()) != 0
    assert too_large in L.dh_last_error()
    assert L.dh_energy_plan_build(_lib.ptr(dl["pairs"]), n, _lib.ptr(dl["bg_trans"]), dl["bg_trans"].numel(), 128, _lib.ptr(buf),
                                  nb.value, _lib.stream_ptr()) != 0
    assert too_large in L.dh_last_error() and b"dh_energy_plan_build" in L.dh_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf, good)                                            # nothing was launched by the refused calls
    with pytest.raises(ValueError, match="positive"):
        from diffusionhandles_amd.losses import EnergyPlan
        EnergyPlan(_pc("occluding", (0,)), GRID, dev(), object_weights=[0.0, 1.0])


# ---- 8. None and a single object: the parent's path -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_weights_and_one_object_take_the_unweighted_path(dtype):
    from diffusionhandles_amd.losses import EnergyPlan, process_correspondences
    C = 320
    act, orig = _maps(C, dtype, 500)
    corr, _, _, _ = W.scene("occluding")
    plain_pc = process_correspondences(corr, W.RES, 0, grid=GRID, device=dev())          # the parent's call: no labels
    assert "object" not in plain_pc and "pair_obj" not in plain_pc.device_lists
    parent = _call(act, orig, EnergyPlan(plain_pc, GRID, dev()), 7.5, 1.5, dtype)
    for plan in (EnergyPlan(_pc("occluding"), GRID, dev()), EnergyPlan(_pc("occluding"), GRID, dev(), object_weights=None)):
        assert not plan.weighted
        loss, grad = _call(act, orig, plan, 7.5, 1.5, dtype)
        assert torch.equal(grad, parent[1]) and torch.equal(loss, parent[0])
    # M = 1: object 0's correspondences under the label image of its mask alone, any weight
    one = _pc("occluding", (0,), masks=(0,))
    assert one["object"].max() == 0 and len(one["object"]) == 4155
    base = _call(act, orig, EnergyPlan(one, GRID, dev()), 7.5, 1.5, dtype)
    for ow in ("equal", [1.0], [0.125], [37.0]):
        plan = EnergyPlan(one, GRID, dev(), object_weights=ow)
        assert not plan.weighted
        loss, grad = _call(act, orig, plan, 7.5, 1.5, dtype)
        assert torch.equal(grad, base[1]) and torch.equal(loss, base[0])
    with pytest.raises(ValueError):
        EnergyPlan(one, GRID, dev(), object_weights=[0.0])


# ---- 9. the loop level, on the TINY rig of tests/test_multi_object_gpu.py ---------------------------------------------------------
@contextlib.contextmanager
def mode(gd, m):
    old = gd.grad_scale_mode
    gd.grad_scale_mode = m
    try:
        yield gd
    finally:
        gd.grad_scale_mode = old


@pytest.fixture(scope="module")
def tiny():
    """The two-sphere image at 512 pixels and its identity (initial inference from noise, no inversion) by the product."""
    from diffusionhandles_amd import DiffusionHandles
    from diffusionhandles_amd import conf as C
    from diffusionhandles_amd.unet import HipUNet
    from oracle import unet_torch as U
    ref = U.init_synthetic_(U.UNetTorch(U.TINY), seed=0).to(dev()).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.half().float())
    hip = HipUNet(dict(U.TINY, text_len=77), dtype=torch.float16, max_batch=4)
    hip.load_state_dict(ref.state_dict())
    dh = DiffusionHandles(C.load_default(), unet=hip, unet_config=dict(U.TINY, text_len=77)).to(dev())
    res = 512
    depth, bg, masks = R.two_spheres(res)
    depth, bg, masks = depth.to(dev()), bg.to(dev()), [m.to(dev()) for m in masks]
    g = torch.Generator().manual_seed(11)
    noise = torch.randn(1, 4, res // 8, res // 8, generator=g).to(dev())
    Dm = dh.diffuser.unet.cfg["cross_attention_dim"]
    unc = (dh.diffuser._encode([""])[None].expand(50, -1, -1, -1) + 0.05 * torch.randn(50, 1, 77, Dm, generator=g).to(dev())).contiguous()
    prompt = "two spheres on a plane"
    null_text, noise, acts, _ = dh.generate_input_image(depth, prompt, unc, noise)
    return SimpleNamespace(dh=dh, gd=dh.diffuser, depth=depth, bg_depth=dh.set_foreground(depth, masks, bg), masks=masks,
                           prompt=prompt, null_text=null_text, noise=noise, acts=acts)


def _t(tf):
    a, ax, tr = tf
    return (float(a), torch.tensor(ax, dtype=torch.float32), torch.tensor(tr, dtype=torch.float32))


def rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def test_guided_step_with_object_weights_on_the_tiny_rig(tiny):
    from diffusionhandles_amd.depth_transform import reproject_object_edits
    from diffusionhandles_amd.losses import object_label_image
    dh, gd = tiny.dh, tiny.gd
    tfs = [_t(tf) for tf in R.OCCLUDING]
    (d, c), = reproject_object_edits(tiny.depth, tiny.bg_depth, tiny.masks, gd.get_depth_intrinsics(device=dev()), [tfs])
    labels = object_label_image(tiny.masks)
    assert labels.shape == (512, 512) and sorted(labels.unique().tolist()) == [0, 1, 2]
    gd.scheduler.set_timesteps(50)
    t0 = gd.scheduler.timesteps[0]
    x0 = tiny.noise.permute(0, 2, 3, 1).contiguous()

    def step(**kw):
        with torch.no_grad(), gd.on_stream():
            st = gd.prepare_guidance(d, tiny.prompt, tiny.acts, c, **kw)
            x = gd.guided_step(st, x0.clone(), 0, t0, tiny.null_text[0]).clone()
        torch.cuda.synchronize()
        assert torch.isfinite(x).all()
        return st, x
    st_none, x_none = step()
    st_lab, x_lab = step(object_labels=labels)                               # labels without weights: the unweighted path
    assert not st_none.plan.weighted and not st_lab.plan.weighted and torch.equal(x_lab, x_none)
    st_eq, x_eq = step(object_labels=labels, object_weights="equal")
    counts = st_eq.plan.counts
    print("pairs per object", counts.tolist(), "omega", st_eq.plan.omega.tolist())
    assert st_eq.plan.weighted and counts.sum() == st_none.n_pairs and 0 < counts[1] < counts[0] / 4
    assert not torch.equal(x_eq, x_none) and rel(x_eq, x_none) > 1e-6
    st_n, x_n = step(object_labels=labels, object_weights=[float(v) for v in counts])
    e = rel(x_n, x_none)
    print(f"w = N against no weights: rel-L2 {e:.3e}; 'equal' against no weights: {rel(x_eq, x_none):.3e}")
    assert st_n.plan.weighted and e <= 5e-3
    with pytest.raises(ValueError, match="object_labels"):
        gd.prepare_guidance(d, tiny.prompt, tiny.acts, c, object_weights="equal")
    # 'auto' runs with weights; a small object's larger coefficient lowers the scale where the foreground term dominates
    with mode(gd, "auto"):
        st_a, x_a = step(object_labels=labels, object_weights="equal")
        st_a0, _ = step()
        assert st_a.auto and (st_a.scale_host <= st_a0.scale_host).all() and (st_a.scale_host < st_a0.scale_host).any()
        gd.raise_on_status([(0, st_a.status[0].cpu().tolist())])


def test_transform_foreground_objects_batch_with_equal_weights(tiny):
    dh, gd = tiny.dh, tiny.gd
    edits = [[_t(tf) for tf in R.OCCLUDING], [_t(tf) for tf in W.EDITS["apart"]]]
    args = dict(depth=tiny.depth, prompt=tiny.prompt, fg_masks=tiny.masks, bg_depth=tiny.bg_depth, null_text_emb=tiny.null_text,
                init_noise=tiny.noise, activations=tiny.acts)
    imgs, disps = dh.transform_foreground_objects_batch(**args, edits=edits, object_weights="equal")
    imgs, lat = imgs.clone(), gd.last_latents.clone()
    assert imgs.shape == (2, 3, 512, 512) and len(disps) == 2 and torch.isfinite(imgs).all()
    plain, _ = dh.transform_foreground_objects_batch(**args, edits=edits)
    assert not torch.equal(imgs[0], plain[0]) and float((gd.last_latents[0] - lat[0]).abs().max()) > 1e-4
