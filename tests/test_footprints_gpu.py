"""GPU: footprint splatting (dh_reproject_footprint_edits, the footprints / footprint_max_ratio keywords of depth_transform
and the conf keys of DiffusionHandles) -- footprints = 0 is dh_reproject_similarity_edits byte for byte; five edits of the
two-sphere scene and a step scene against the test-side reference tests/footprints_ref.py, integer outputs bit-exact with
NO pixel excluded; both tiers give the same bytes; calls repeat; refused arguments leave the outputs untouched; the loop
level on the TINY rig.  The C entry writes into outputs that are NaN / 0xFF / -1 before the call."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_object_ref as R  # noqa: E402
import footprints_ref as F  # noqa: E402

pytestmark = pytest.mark.gpu
OUTPUTS = ("zmap", "raw", "clean", "vis", "txy", "corr", "counts", "disp")
INT_MAX = 2 ** 31 - 1


def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _t(tf):
    return (float(tf[0]), torch.tensor(tf[1], dtype=torch.float32), torch.tensor(tf[2], dtype=torch.float32)) + tuple(tf[3:])


def _rows(edits):
    from diffusionhandles_amd import depth_transform as DT
    rows = DT._xform_rows([_t(tf) for tfs in edits for tf in tfs], similarity=True)
    assert rows.shape == (sum(len(tfs) for tfs in edits), 16) and rows.dtype == np.float64
    return rows


def _setup(depth, bg, masks):
    """Device inputs of the C entries: the pixel lists of the masks, concatenated."""
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    L, st = _lib.lib(), _lib.stream_ptr()
    res, M = depth.shape[-1], len(masks)
    d = depth.to(dev(), torch.float32).contiguous()
    b = bg.to(dev(), torch.float32).contiguous()
    gx, gy = DT._grids(res, res, dev())
    intr = D.intrinsics_f32()
    ifx, ify = DT._inv_focal(intr)
    fg_pix = torch.full((res * res,), -1, dtype=torch.int32, device=dev())
    n_dev = torch.full((M,), -1, dtype=torch.int32, device=dev())
    ws_small = torch.empty(4096, dtype=torch.uint8, device=dev())
    start = [0]
    for m, mask in enumerate(masks):
        m8 = (mask.to(dev()) != 0).to(torch.uint8).contiguous().view(-1)
        _lib.check(L.dh_fg_pixel_list(_lib.ptr(m8), res, _lib.ptr(fg_pix[start[-1]:]), _lib.ptr(n_dev[m:]), _lib.ptr(ws_small),
                                      ws_small.numel(), st), "dh_fg_pixel_list")
        start.append(start[-1] + int(m8.sum().item()))
    assert n_dev.tolist() == [start[m + 1] - start[m] for m in range(M)] and min(n_dev.tolist()) > 0
    return SimpleNamespace(L=L, st=st, res=res, M=M, d=d, b=b, gx=gx, gy=gy, ifx=ifx, ify=ify, fx=float(intr[0, 0]),
                           fy=float(intr[1, 1]), fg_pix=fg_pix, n_fg=start[-1], obj_start=np.asarray(start, dtype=np.int32))


def _call(s, rows, footprints=1, ratio=0.0, cap=None, entry="footprint"):
    """dh_reproject_footprint_edits (or, entry="similarity", dh_reproject_similarity_edits) on poisoned outputs.  cap: the
    correspondence rows per edit (default: what the setting needs).  A call that returned 0 is checked for having written
    everything the contract promises."""
    from diffusionhandles_amd import _lib
    L, res, M, n_fg = s.L, s.res, s.M, s.n_fg
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    assert rows.ndim == 2 and rows.shape[1] == 16 and rows.shape[0] % M == 0
    K = rows.shape[0] // M
    need = res * res if footprints == 1 else n_fg
    cap = need if cap is None else cap
    nb = ctypes.c_size_t()
    if entry == "similarity":
        _lib.check(L.dh_reproject_objects_workspace_bytes(res, n_fg, K, M, ctypes.byref(nb)))
    else:
        _lib.check(L.dh_reproject_footprints_workspace_bytes(res, n_fg, K, M, 1 if footprints == 1 else 0, ctypes.byref(nb)))
    ws = torch.full((nb.value,), 0xFF, dtype=torch.uint8, device=dev())
    nan = float("nan")
    o = SimpleNamespace(
        zmap=torch.full((K, res, res), nan, device=dev()), disp=torch.full((K, res, res), nan, device=dev()),
        raw=torch.full((K, res, res), 0xFF, dtype=torch.uint8, device=dev()),
        clean=torch.full((K, res, res), 0xFF, dtype=torch.uint8, device=dev()),
        vis=torch.full((K, n_fg), 0xFF, dtype=torch.uint8, device=dev()),
        txy=torch.full((K, n_fg, 2), -1, dtype=torch.int32, device=dev()),
        corr=torch.full((K, max(cap, 1), 4), -1, dtype=torch.int64, device=dev()),
        counts=torch.full((K, 4), -1, dtype=torch.int32, device=dev()))
    args = (_lib.ptr(s.d), _lib.ptr(s.b), _lib.ptr(s.fg_pix), n_fg, M, s.obj_start.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            res, _lib.ptr(s.gx), _lib.ptr(s.gy), s.ifx, s.ify, s.fx, s.fy, K, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            None, _lib.ptr(o.zmap), _lib.ptr(o.raw), _lib.ptr(o.clean), _lib.ptr(o.disp), _lib.ptr(o.vis), _lib.ptr(o.txy),
            _lib.ptr(o.corr), _lib.ptr(o.counts), _lib.ptr(ws), nb.value, s.st)
    if entry == "similarity":
        o.rc = L.dh_reproject_similarity_edits(*args)
    else:
        o.rc = L.dh_reproject_footprint_edits(*args, footprints, ratio, cap)
    o.err = L.dh_last_error().decode() if o.rc != 0 else ""
    torch.cuda.synchronize()
    o.counts_h = o.counts.cpu()
    if o.rc == 0:
        assert torch.isfinite(o.disp).all() and not torch.isnan(o.zmap).any()
        assert int(o.raw.max()) <= 1 and int(o.clean.max()) <= 1 and int(o.vis.max()) <= 1
        assert int(o.txy.min()) >= 0 and int(o.txy.max()) < res
        assert (o.counts_h[:, 3] >= 0).all()
        for e in range(K):
            n = int(o.counts_h[e, 0])
            assert 0 < n <= cap and 0 < int(o.counts_h[e, 1]) <= n_fg
            assert int(o.corr[e, :n].min()) >= 0 and int(o.corr[e, :n].max()) < res and bool((o.corr[e, n:] == -1).all())
    return o


def _same_bytes(a, b, what):
    for k in OUTPUTS:
        x, y = getattr(a, k).contiguous().view(torch.uint8), getattr(b, k).contiguous().view(torch.uint8)
        assert torch.equal(x, y), f"{what}: {k}"


def _untouched(o):
    assert torch.isnan(o.zmap).all() and torch.isnan(o.disp).all()
    assert bool((o.raw == 0xFF).all()) and bool((o.clean == 0xFF).all()) and bool((o.vis == 0xFF).all())
    assert bool((o.txy == -1).all()) and bool((o.corr == -1).all()) and bool((o.counts == -1).all())


def _check_against_ref(o, e, ref, what):
    """Every integer output bit-exact, no pixel left out; the disparity within the 2e-3 (of 255) of the point-mode tests."""
    disp_r, corr_r, dbg_r = ref
    n = int(o.counts_h[e, 0])
    assert n == len(corr_r), f"{what}: {n} correspondences, the reference has {len(corr_r)}"
    assert np.array_equal(o.corr[e, :n].cpu().numpy(), corr_r.numpy()), f"{what}: correspondences (order included)"
    assert np.array_equal(o.zmap[e].cpu().numpy(), dbg_r["zmap"]), f"{what}: zmap"
    assert np.array_equal(o.raw[e].cpu().numpy() != 0, dbg_r["raw_mask"]), f"{what}: raw mask"
    assert np.array_equal(o.clean[e].cpu().numpy() != 0, dbg_r["cleaned"] != 0), f"{what}: clean mask"
    assert np.array_equal(o.vis[e].cpu().numpy() != 0, dbg_r["vis"]), f"{what}: vis"
    txy = o.txy[e].cpu().numpy()
    assert np.array_equal(txy[:, 0], dbg_r["tx"]) and np.array_equal(txy[:, 1], dbg_r["ty"]), f"{what}: target_xy"
    assert int(o.counts_h[e, 1]) == int(dbg_r["vis"].sum()), f"{what}: visible count"
    assert int(o.counts_h[e, 2]) == int(dbg_r["inpaint"].sum()), f"{what}: in-fill count"
    err = float((o.disp[e].cpu() - disp_r[0, 0]).abs().max())
    print(f"{what}: {n} correspondences, {int(o.counts_h[e, 2])} in-fill pixels, disparity max abs err {err:.2e}")
    assert err < 2e-3, f"{what}: disparity {err}"


_REFS = {}


def _refs(key, make):
    """A reference is computed once per session and never changed."""
    if key not in _REFS:
        from oracle import depth_ref as D
        D.DOT_ORDER = "explicit"
        try:
            _REFS[key] = make()
        finally:
            D.DOT_ORDER = "blas"
    return _REFS[key]


# ---- 1. footprints = 0 is the similarity entry ------------------------------------------------------------------------------
def test_footprints_off_is_the_similarity_entry():
    """two_spheres(128), the five edits: dh_reproject_footprint_edits with footprints = 0 against
    dh_reproject_similarity_edits, every byte of every output (the poison beyond the valid rows included); the workspace
    query with footprints = 0 is the objects query."""
    depth, bg, masks = R.two_spheres(128)
    s = _setup(depth, bg, masks)
    rows = _rows(F.EDITS)
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    assert s.L.dh_reproject_objects_workspace_bytes(128, s.n_fg, 5, 2, ctypes.byref(a)) == 0
    assert s.L.dh_reproject_footprints_workspace_bytes(128, s.n_fg, 5, 2, 0, ctypes.byref(b)) == 0 and a.value == b.value
    assert s.L.dh_reproject_footprints_workspace_bytes(128, s.n_fg, 5, 2, 1, ctypes.byref(b)) == 0 and b.value > a.value
    old = _call(s, rows, entry="similarity", footprints=0)
    new = _call(s, rows, footprints=0)
    assert old.rc == 0 and new.rc == 0, old.err + new.err
    assert min(int(old.counts_h[e, 0]) for e in range(5)) > 500
    _same_bytes(new, old, "footprints = 0")


# ---- 2. five edits in ONE call against the reference ------------------------------------------------------------------------
@pytest.mark.parametrize("res", [128, 256])
def test_five_edits_against_the_reference(res):
    """two_spheres(res), K = 5 in one call: identity, 1.5 / 0.6, scale 3 with a turn, towards the camera, OCCLUDING."""
    depth, bg, masks = R.two_spheres(res)
    s = _setup(depth, bg, masks)
    o = _call(s, _rows(F.EDITS))
    assert o.rc == 0, o.err
    refs = _refs(("spheres", res), lambda: [F.transform_objects(depth, bg, masks, tfs, footprints=True) for tfs in F.EDITS])
    for e, ref in enumerate(refs):
        _check_against_ref(o, e, ref, f"res {res}, edit {e}")
    # the enlarged object: more rows than foreground points
    assert int(o.counts_h[2, 0]) > s.n_fg
    # the Python call gives the same bits, on the host and on the device
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    args = (depth.to(dev()), bg.to(dev()), [m.to(dev()) for m in masks], D.intrinsics_f32(), [[_t(tf) for tf in tfs] for tfs in F.EDITS])
    out, dbg = DT.reproject_object_edits(*args, return_debug=True, footprints=True)
    out_d = DT.reproject_object_edits(*args, device_correspondences=True, footprints=True)
    assert dbg["corr_dev"].shape == (5, res * res, 4)
    for e in range(5):
        n = int(o.counts_h[e, 0])
        assert torch.equal(out[e][1], o.corr[e, :n].cpu()) and torch.equal(out[e][0][0, 0], o.disp[e])
        assert out_d[e][1].is_cuda and torch.equal(out_d[e][1], o.corr[e, :n])
    assert torch.equal(dbg["zmap"], o.zmap) and torch.equal(dbg["vis"], o.vis) and torch.equal(dbg["clean_mask"], o.clean)


# ---- 3. the step scene: the ratio guard, both tiers, repeated calls -----------------------------------------------------------
STEP_RES = 128


def _step():
    depth, bg, masks = F.step_scene(STEP_RES)
    return depth, bg, masks, _setup(depth, bg, masks)


def _step_ref(ratio):
    depth, bg, masks = F.step_scene(STEP_RES)
    return _refs(("step", ratio), lambda: F.transform_objects(depth, bg, masks, F.STEP_TURN, footprints=True, max_ratio=ratio))


def test_step_scene_against_the_reference_with_and_without_the_ratio_guard():
    """One mask over a square whose halves lie at depths 2 and 3, turned 40 degrees about Y: the quads across the step become
    long sheets with big boxes.  footprint_max_ratio None and 1.1 against the reference; the guard removes the sheets."""
    _, _, _, s = _step()
    rows = _rows([F.STEP_TURN])
    owned = {}
    for ratio in (None, 1.1):
        o = _call(s, rows, ratio=0.0 if ratio is None else ratio)
        assert o.rc == 0, o.err
        _check_against_ref(o, 0, _step_ref(ratio), f"step scene, ratio {ratio}")
        owned[ratio] = int(o.raw.sum())
    print(f"foreground-owned pixels: {owned}")
    assert owned[1.1] < owned[None]


def test_both_tiers_give_the_same_bytes_and_calls_repeat():
    """dh_dbg_footprint_tier at 1 (every box of more than one candidate goes to the wave tier), the default and INT_MAX (the
    thread tier draws everything): byte-equal outputs on the step scene, which are the reference's; a second call repeats."""
    _, _, _, s = _step()
    rows = _rows([F.STEP_TURN])
    outs = {}
    try:
        for tier in (1, 0, INT_MAX):
            assert s.L.dh_dbg_footprint_tier(tier) == 0
            outs[tier] = _call(s, rows)
            assert outs[tier].rc == 0, outs[tier].err
    finally:
        assert s.L.dh_dbg_footprint_tier(0) == 0
    again = _call(s, rows)
    assert again.rc == 0
    _check_against_ref(outs[1], 0, _step_ref(None), "wave tier")
    _same_bytes(outs[0], outs[1], "default tier against the wave tier")
    _same_bytes(outs[INT_MAX], outs[1], "thread tier against the wave tier")
    _same_bytes(again, outs[0], "two identical calls")
    assert s.L.dh_dbg_footprint_tier(-1) != 0


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("footprints,ratio,cap,word", [
    (1, 1.0, None, "max_ratio"), (1, 0.5, None, "max_ratio"), (1, -2.0, None, "max_ratio"), (1, float("nan"), None, "max_ratio"),
    (1, float("inf"), None, "max_ratio"), (0, 1.5, None, "without footprints"), (2, 0.0, None, "footprints"),
    (-1, 0.0, None, "footprints"), (1, 0.0, "res2-1", "capacity"), (1, 0.0, "n_fg", "capacity"), (0, 0.0, "n_fg-1", "capacity")])
def test_library_refuses_bad_arguments_before_any_launch(footprints, ratio, cap, word):
    depth, bg, masks = R.two_spheres(128)
    s = _setup(depth, bg, masks)
    cap = {None: None, "res2-1": 128 * 128 - 1, "n_fg": s.n_fg, "n_fg-1": s.n_fg - 1}[cap]
    o = _call(s, _rows([F.IDENTITY, F.SCALE3]), footprints=footprints, ratio=ratio, cap=cap)
    assert o.rc != 0 and word in o.err, o.err
    _untouched(o)


def test_python_refusals_come_before_the_library():
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    depth, bg, masks = R.two_spheres(128)
    args = (depth.to(dev()), bg.to(dev()), masks[0].to(dev()), D.intrinsics_f32())
    for bad in (1.0, 0.3, float("nan"), float("inf"), "wide"):
        with pytest.raises(ValueError, match="footprint_max_ratio"):
            DT.transform_depth_footprints(*args, 10.0, footprints=True, footprint_max_ratio=bad)
    with pytest.raises(ValueError, match="without footprints"):
        DT.transform_depth_footprints(*args, 10.0, footprint_max_ratio=1.5)
    with pytest.raises(NotImplementedError, match="footprints"):
        DT.transform_depth_mesh(*args, 10.0, footprints=True)
    # and the one-edit call is the batched one
    disp, corr = DT.transform_depth_footprints(*args, 10.0, scale=2.0, footprints=True)
    (disp_b, corr_b), = DT.reproject_edits(*args, [(10.0, torch.tensor(R.Y), torch.zeros(3), 2.0, None)], footprints=True)
    assert torch.equal(disp, disp_b) and torch.equal(corr, corr_b) and len(corr) > int((masks[0] > 0.5).sum())


# ---- 5. the loop level, on the TINY rig of tests/test_similarity_gpu.py -------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
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
    conf = C.load_default()
    conf.depth_transform_footprints = True
    dh = DiffusionHandles(conf, unet=hip, unet_config=dict(U.TINY, text_len=77)).to(dev())
    res = 512
    depth, bg, masks = R.two_spheres(res)
    cpu = SimpleNamespace(depth=depth, masks=masks)
    depth, bg, masks = depth.to(dev()), bg.to(dev()), [m.to(dev()) for m in masks]
    g = torch.Generator().manual_seed(11)
    noise = torch.randn(1, 4, res // 8, res // 8, generator=g).to(dev())
    Dm = dh.diffuser.unet.cfg["cross_attention_dim"]
    unc = (dh.diffuser._encode([""])[None].expand(50, -1, -1, -1) + 0.05 * torch.randn(50, 1, 77, Dm, generator=g).to(dev())).contiguous()
    prompt = "two spheres on a plane"
    null_text, noise, acts, _ = dh.generate_input_image(depth, prompt, unc, noise)
    return SimpleNamespace(dh=dh, gd=dh.diffuser, depth=depth, bg_depth=dh.set_foreground(depth, masks, bg), masks=masks,
                           prompt=prompt, null_text=null_text, noise=noise, acts=acts, cpu=cpu)


def _args(t, **masks):
    return dict(depth=t.depth, prompt=t.prompt, bg_depth=t.bg_depth, null_text_emb=t.null_text, init_noise=t.noise,
                activations=t.acts, **masks)


def test_footprints_at_the_loop_level(tiny):
    """A conf with depth_transform_footprints: one transform_foreground and one transform_foregrounds batch mixing a one-object
    and a two-object edit.  The images are finite, and the number of correspondences that reaches prepare_guidance is the
    reference's (more than the object has points: the rows are per target pixel)."""
    dh, gd = tiny.dh, tiny.gd
    seen = []
    inner = gd.prepare_guidance

    def spy(depth, prompt, activations_orig, correspondences, *a, **k):
        seen.append(int(correspondences.shape[0]))
        return inner(depth, prompt, activations_orig, correspondences, *a, **k)
    one = (0.0, R.Y, (0.1, 0.0, -1.0))
    two = [(10.0, R.Y, (0.1, 0.0, 0.0), 1.5, None), (0.0, R.Y, (0.0, 0.0, 0.0), 0.8, None)]
    bg_cpu = tiny.bg_depth.cpu()
    want_one = len(_refs(("loop", 1), lambda: F.transform_objects(tiny.cpu.depth, bg_cpu, tiny.cpu.masks[:1], [one], footprints=True,
                                                                   infill=False))[1])
    want_two = len(_refs(("loop", 2), lambda: F.transform_objects(tiny.cpu.depth, bg_cpu, tiny.cpu.masks, two, footprints=True,
                                                                   infill=False))[1])
    n_fg0 = int((tiny.cpu.masks[0] > 0.5).sum())
    assert want_one > n_fg0
    gd.prepare_guidance = spy
    try:
        img, disp = dh.transform_foreground(**_args(tiny, fg_mask=tiny.masks[0]), rot_angle=one[0], rot_axis=torch.tensor(one[1]),
                                            translation=torch.tensor(one[2]))
        assert img.shape == (1, 3, 512, 512) and torch.isfinite(img).all() and torch.isfinite(disp).all()
        assert seen == [want_one]
        del seen[:]
        images, disps = dh.transform_foregrounds([
            dict(_args(tiny, fg_mask=tiny.masks[0]), rot_angle=one[0], rot_axis=torch.tensor(one[1]), translation=torch.tensor(one[2])),
            dict(_args(tiny, fg_masks=tiny.masks), transforms=[_t(tf) for tf in two])])
        assert images.shape == (2, 3, 512, 512) and torch.isfinite(images).all()
        assert seen == [want_one, want_two]
        assert torch.equal(disps[0], disp)
    finally:
        del gd.prepare_guidance
