"""GPU: scale and pivot of an object transform (dh_reproject_similarity_edits, the 5-tuples of depth_transform and
DiffusionHandles) -- the rigid entries are its scale-1 / no-pivot calls byte for byte; four similarity edits of the
two-sphere scene against the test-side reference tests/similarity_ref.py, integer outputs bit-exact; a pivot at the centroid
is no pivot; refused rows leave the outputs untouched; the loop level on the TINY rig; the pivot in mesh mode.  The C
entries write into outputs that are NaN / 0xFF / -1 before the call."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_object_ref as R  # noqa: E402
import similarity_ref as S  # noqa: E402

from diffusionhandles_amd.synthetic import TRANSFORMS, make_scene  # noqa: E402

pytestmark = pytest.mark.gpu
OUTPUTS = ("zmap", "raw", "clean", "vis", "txy", "corr", "counts", "disp")


def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _t(tf):
    """A 3- or 5-tuple of plain numbers -> what the Python layers take (tensors for axis and translation)."""
    return (float(tf[0]), torch.tensor(tf[1], dtype=torch.float32), torch.tensor(tf[2], dtype=torch.float32)) + tuple(tf[3:])


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


def _call(s, rows, entry):
    """One C entry -- "edits": dh_reproject_edits, "objects": dh_reproject_object_edits (rows of 8 doubles), "similarity":
    dh_reproject_similarity_edits (rows of 16) -- on poisoned outputs.  Returns the outputs, the status and the error text;
    a call that returned 0 is checked for having written everything the contract promises."""
    from diffusionhandles_amd import _lib
    L, res, M, n_fg = s.L, s.res, s.M, s.n_fg
    width = 16 if entry == "similarity" else 8
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    assert rows.ndim == 2 and rows.shape[1] == width and rows.shape[0] % M == 0
    K = rows.shape[0] // M
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
        counts=torch.full((K, 4), -1, dtype=torch.int32, device=dev()))
    xf = rows.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    outs = (_lib.ptr(o.zmap), _lib.ptr(o.raw), _lib.ptr(o.clean), _lib.ptr(o.disp), _lib.ptr(o.vis), _lib.ptr(o.txy),
            _lib.ptr(o.corr), _lib.ptr(o.counts), _lib.ptr(ws), nb.value, s.st)
    head = (_lib.ptr(s.d), _lib.ptr(s.b), _lib.ptr(s.fg_pix), n_fg)
    tail = (res, _lib.ptr(s.gx), _lib.ptr(s.gy), s.ifx, s.ify, s.fx, s.fy, K, xf, None)
    objs = (M, s.obj_start.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    if entry == "edits":
        o.rc = L.dh_reproject_edits(*head, *tail, *outs)
    elif entry == "objects":
        o.rc = L.dh_reproject_object_edits(*head, *objs, *tail, *outs)
    else:
        o.rc = L.dh_reproject_similarity_edits(*head, *objs, *tail, *outs)
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
            assert 0 < n <= int(o.counts_h[e, 1]) <= n_fg
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


def _rows(edits):
    from diffusionhandles_amd import depth_transform as DT
    rows = DT._xform_rows([_t(tf) for tfs in edits for tf in tfs], similarity=True)
    assert rows.shape == (sum(len(tfs) for tfs in edits), 16) and rows.dtype == np.float64
    return rows


# ---- 1. the rigid entries are the scale-1 / no-pivot calls of the new one ----------------------------------------------------
def test_old_entries_are_the_scale_one_calls_of_the_new_entry():
    """make_scene(256), the first three TRANSFORMS: dh_reproject_similarity_edits with scale 1 and no pivot against
    dh_reproject_object_edits and dh_reproject_edits, every byte of every output (the poison beyond the valid rows included)."""
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, mask = make_scene(256)
    tfs = [(TRANSFORMS[i][0], (0.0, 1.0, 0.0), TRANSFORMS[i][1]) for i in range(3)]
    s = _setup(depth, bg, [mask])
    rows8 = DT._xform_rows([_t(tf) for tf in tfs])
    assert rows8.shape == (3, 8)
    rows16 = _rows([[tf] for tf in tfs])
    assert np.array_equal(rows16[:, :8], rows8) and np.array_equal(rows16[:, 8:], np.tile([1.0, 1, 1, 0, 0, 0, 0, 0], (3, 1)))
    assert np.array_equal(rows16, _rows([[tf + (None, None)] for tf in tfs])) and np.array_equal(rows16, _rows([[tf + (1.0, None)] for tf in tfs]))
    new = _call(s, rows16, "similarity")
    assert new.rc == 0, new.err
    for entry in ("objects", "edits"):
        old = _call(s, rows8, entry)
        assert old.rc == 0, old.err
        assert min(int(old.counts_h[e, 0]) for e in range(3)) > 1000
        _same_bytes(new, old, entry)


# ---- 2. four similarity edits against the reference ---------------------------------------------------------------------------
def _check_against_ref(o, e, disp_r, corr_r, dbg_r):
    n = int(o.counts_h[e, 0])
    assert np.array_equal(o.corr[e, :n].cpu().numpy(), corr_r.numpy()), f"edit {e}: correspondences (order included)"
    assert np.array_equal(o.zmap[e].cpu().numpy(), dbg_r["zmap"]), f"edit {e}: zmap"
    assert np.array_equal(o.raw[e].cpu().numpy() != 0, dbg_r["raw_mask"]), f"edit {e}: raw mask"
    assert np.array_equal(o.clean[e].cpu().numpy() != 0, dbg_r["cleaned"] != 0), f"edit {e}: clean mask"
    assert np.array_equal(o.vis[e].cpu().numpy() != 0, dbg_r["vis"]), f"edit {e}: vis"
    assert int(o.counts_h[e, 1]) == int(dbg_r["vis"].sum())
    err = float((o.disp[e].cpu() - disp_r[0, 0]).abs().max())
    print(f"edit {e}: {n} correspondences, disparity max abs err {err:.2e}")
    assert err < 2e-3, f"edit {e}: disparity {err}"                    # the gate of tests/test_multi_object_gpu.py


@pytest.mark.parametrize("res", [128, 256])
def test_similarity_edits_against_the_reference(res):
    """two_spheres(res), K = 4 edits in one call (similarity_ref.edits_for): all scale 1; uniform 1.5 / 0.6; per-axis scale with a
    25-degree turn about a general axis; a 40-degree turn about a pivot at the lower edge of sphere 1.  The reference runs under
    the written-out dot order.  Every edit keeps at least 100 pairs per object and has no depth tie between the objects."""
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    depth, bg, masks = R.two_spheres(res)
    edits = S.edits_for(res, depth)
    x, y = S.lower_edge_pixel(res)
    assert masks[1][0, 0, y, x] > 0.5 and masks[1][0, 0, y + 2, x] < 0.5
    pivot = DT.pivot_at_pixel(depth.to(dev()), D.intrinsics_f32(), x, y)
    assert pivot.dtype == torch.float32 and pivot.device.type == "cpu"
    assert np.array_equal(pivot.numpy(), np.asarray(edits[3][1][4], dtype=np.float32))          # dh_unproject's point is the oracle's
    s = _setup(depth, bg, masks)
    o = _call(s, _rows(edits), "similarity")
    assert o.rc == 0, o.err
    D.DOT_ORDER = "explicit"
    try:
        refs = [S.transform_objects(depth, bg, masks, tfs) for tfs in edits]
    finally:
        D.DOT_ORDER = "blas"
    for e, (disp_r, corr_r, dbg_r) in enumerate(refs):
        assert min(S.pairs_per_object(corr_r, masks)) >= 100 and R.z_ties_between_objects(dbg_r, res=res) == 0
        _check_against_ref(o, e, disp_r, corr_r, dbg_r)
    # the scaled edits are not the rigid ones: object 0 covers more pixels at 1.5 than at 1, object 1 fewer at 0.6
    area = lambda e, j: len({(int(c[2]), int(c[3])) for c in refs[e][1].numpy() if masks[j][0, 0, int(c[1]), int(c[0])] > 0.5})
    assert area(1, 0) > 1.05 * area(0, 0) and area(1, 1) < 0.6 * area(0, 1)
    # the Python call with 5-tuples (pivot from pivot_at_pixel) gives the same bits
    tuples = [[_t(tf) for tf in tfs] for tfs in edits]
    tuples[3][1] = tuples[3][1][:4] + (pivot,)
    out, dbg = DT.reproject_object_edits(depth.to(dev()), bg.to(dev()), [m.to(dev()) for m in masks], D.intrinsics_f32(), tuples,
                                         return_debug=True)
    for e in range(4):
        assert torch.equal(out[e][1], o.corr[e, :int(o.counts_h[e, 0])].cpu()) and torch.equal(out[e][0][0, 0], o.disp[e])
    assert torch.equal(dbg["zmap"], o.zmap) and torch.equal(dbg["vis"], o.vis) and torch.equal(dbg["clean_mask"], o.clean)


# ---- 3. pivot ---------------------------------------------------------------------------------------------------------------
def test_pivot_at_the_centroid_is_no_pivot_and_calls_repeat():
    from diffusionhandles_amd import _lib
    depth, bg, masks = R.two_spheres(256)
    s = _setup(depth, bg, masks)
    cen = torch.full((2, 3), float("nan"), device=dev())
    for m in range(2):
        a, b = int(s.obj_start[m]), int(s.obj_start[m + 1])
        _lib.check(s.L.dh_masked_centroid(_lib.ptr(s.d), _lib.ptr(s.fg_pix[a:]), b - a, s.res, _lib.ptr(s.gx), _lib.ptr(s.gy),
                                          s.ifx, s.ify, _lib.ptr(cen[m]), s.st), "dh_masked_centroid")
    cen = cen.cpu().numpy()
    assert np.isfinite(cen).all() and cen.dtype == np.float32
    base = [[(25.0, (0.3, 0.9, -0.2), (0.1, -0.05, 0.2), (1.3, 0.8, 1.0)), (-20.0, R.Y, (-0.15, 0.05, 0.1), 0.7)],
            [(-10.0, R.Y, (0.0, 0.0, 0.0), 1.0), (40.0, (0.0, 0.0, 1.0), (0.0, 0.1, 0.0), 1.2)]]
    none = _call(s, _rows([[tf + (None,) for tf in tfs] for tfs in base]), "similarity")
    rows = _rows([[tf + (tuple(float(v) for v in cen[m]),) for m, tf in enumerate(tfs)] for tfs in base])
    assert (rows[:, 14] == 1.0).all() and np.array_equal(rows[:, 11:14].astype(np.float32), np.tile(cen, (2, 1)))
    at_centroid = _call(s, rows, "similarity")
    again = _call(s, rows, "similarity")
    assert none.rc == 0 and at_centroid.rc == 0 and again.rc == 0
    _same_bytes(at_centroid, none, "pivot = centroid against no pivot")
    _same_bytes(again, at_centroid, "two identical calls")
    # and a pivot elsewhere is another result
    rows[1, 11:14] += [0.0, 0.2, 0.0]
    moved = _call(s, rows, "similarity")
    assert moved.rc == 0 and not torch.equal(moved.txy[0], none.txy[0]) and torch.equal(moved.txy[1], none.txy[1])


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col,value,word", [(8, 0.0, "scale"), (9, float("nan"), "scale"), (10, -1.0, "scale"),
                                            (10, float("inf"), "scale"), (12, float("inf"), "pivot"), (11, float("nan"), "pivot")])
def test_library_refuses_bad_rows_before_any_launch(col, value, word):
    depth, bg, masks = R.two_spheres(128)
    s = _setup(depth, bg, masks)
    rows = _rows([[(10.0, R.Y, (0.1, 0.0, 0.0)), (0.0, R.Y, (0.0, 0.0, 0.0))]] * 2)
    rows[3, col] = value                                  # the last row of the call
    if word == "pivot":
        rows[3, 14] = 1.0
    o = _call(s, rows, "similarity")
    assert o.rc != 0 and word in o.err
    _untouched(o)


# ---- 5. the loop level, on the TINY rig of tests/test_edit_items_gpu.py (one image: the two spheres) ---------------------------
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


def _args(t, **masks):
    return dict(depth=t.depth, prompt=t.prompt, bg_depth=t.bg_depth, null_text_emb=t.null_text, init_noise=t.noise,
                activations=t.acts, **masks)


def test_scale_and_pivot_at_the_loop_level(tiny):
    from diffusionhandles_amd.depth_transform import pivot_at_pixel
    dh, gd = tiny.dh, tiny.gd
    Y = torch.tensor(R.Y)
    move = dict(rot_angle=10.0, rot_axis=Y, translation=torch.tensor([0.1, 0.0, 0.0]))
    plain, disp0 = dh.transform_foreground(**_args(tiny, fg_mask=tiny.masks[0]), **move)
    plain = plain.clone()
    scaled, disp1 = dh.transform_foreground(**_args(tiny, fg_mask=tiny.masks[0]), **move, scale=1.5)
    scaled = scaled.clone()
    assert scaled.shape == plain.shape and torch.isfinite(scaled).all()
    assert not torch.equal(disp1, disp0) and rel(scaled, plain) > 1e-3
    # scale and pivot through transform_foregrounds: the same re-projection, the image within the gate of the items tests
    x, y = S.lower_edge_pixel(512, sphere=0)
    pivot = pivot_at_pixel(tiny.depth, gd.get_depth_intrinsics(device=dev()), x, y)
    turn = dict(rot_angle=30.0, rot_axis=torch.tensor([0.0, 0.0, 1.0]), translation=torch.zeros(3), scale=(1.2, 0.9, 1.0), pivot=pivot)
    single, disp2 = dh.transform_foreground(**_args(tiny, fg_mask=tiny.masks[0]), **turn)
    single = single.clone()
    images, disps = dh.transform_foregrounds([dict(_args(tiny, fg_mask=tiny.masks[0]), **move, scale=1.5),
                                              dict(_args(tiny, fg_mask=tiny.masks[0]), **turn)])
    assert torch.equal(disps[0], disp1) and torch.equal(disps[1], disp2) and not torch.equal(disp2, disp0)
    print(f"items against single calls: {rel(images[0], scaled[0]):.2e} {rel(images[1], single[0]):.2e}")
    assert rel(images[0], scaled[0]) < 5e-2 and rel(images[1], single[0]) < 5e-2
    # the multi-object form of transform_foregrounds takes 5-tuples
    t5 = [(10.0, Y, torch.tensor([0.1, 0.0, 0.0]), 1.5, None), (None, None, None, 0.8, None)]
    images_m, disps_m = dh.transform_foregrounds([dict(_args(tiny, fg_masks=tiny.masks), transforms=t5),
                                                  dict(_args(tiny, fg_mask=tiny.masks[0]), **turn)])
    assert torch.isfinite(images_m).all() and torch.equal(disps_m[1], disp2) and not torch.equal(disps_m[0], disp1)
    # transform_foreground_objects with 5-tuples under equal object weights
    img, disp = dh.transform_foreground_objects(**_args(tiny, fg_masks=tiny.masks), transforms=t5, object_weights="equal")
    assert img.shape == plain.shape and torch.isfinite(img).all() and torch.equal(disp, disps_m[0])
    imgs_b, disps_b = dh.transform_foreground_objects_batch(**_args(tiny, fg_masks=tiny.masks), edits=[t5, [t5[1], t5[0]]])
    assert imgs_b.shape == (2, 3, 512, 512) and torch.isfinite(imgs_b).all() and torch.equal(disps_b[0], disp)
    imgs_k, disps_k = dh.transform_foreground_batch(**_args(tiny, fg_mask=tiny.masks[0]),
                                                    transforms=[(10.0, Y, torch.tensor([0.1, 0.0, 0.0]), 1.5, None),
                                                                (10.0, Y, torch.tensor([0.1, 0.0, 0.0]))])
    assert torch.equal(disps_k[0], disp1) and torch.equal(disps_k[1], disp0) and torch.isfinite(imgs_k).all()


# ---- 6. mesh mode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [32, 64])
def test_mesh_pivot_matches_the_oracle_and_scale_is_refused(res):
    """The comparison and the gates of tests/test_mesh_gpu.py, with the centroid of the 11-float transform replaced by the pivot."""
    from diffusionhandles_amd import depth_transform as DT
    from diffusionhandles_amd.guided_stable_diffuser import GuidedStableDiffuser
    from oracle import mesh_ref as M
    depth, bg_depth, mask = make_scene(res)
    K = GuidedStableDiffuser.get_depth_intrinsics()
    gx = torch.linspace(-1, 1, res, dtype=torch.float32).numpy()
    lin01 = torch.linspace(0, 1, res, dtype=torch.float32).numpy()
    invf, f = float(torch.linalg.inv(K)[0, 0]), float(K[0, 0])
    ys, xs = np.nonzero(mask[0, 0].numpy() > 0.5)
    y = int(ys.max())
    x = int(xs[ys == y][0])                                              # a pixel of the object's lowest row
    args = (depth.to(dev()), bg_depth.to(dev()), mask.to(dev()), K)
    pivot = DT.pivot_at_pixel(args[0], K, x, y)
    for ang, axis, tr in [(25.0, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0)), (17.0, (0.3, 1.0, -0.2), (0.1, -0.05, -0.3))]:
        move = (ang, torch.tensor(axis), torch.tensor(tr))
        _, corr0, dbg0 = DT.transform_depth_mesh(*args, *move, return_debug=True)
        disp, corr, dbg = DT.transform_depth_mesh(*args, *move, return_debug=True, pivot=pivot)
        xform = dbg0["xform"].copy()
        xform[8:11] = pivot.numpy()
        assert np.array_equal(dbg["xform"], xform) and not np.array_equal(xform, dbg0["xform"])
        ref = M.mesh_reproject(depth[0, 0].numpy(), bg_depth[0, 0].numpy(), mask[0, 0].numpy() > 0.5, gx, lin01, invf, f,
                               xform, blur=DT.MESH_BLUR_RADIUS)
        assert np.array_equal(dbg["fg_flag"].cpu().numpy().astype(bool), ref["fg_flag"])
        assert np.array_equal(corr.numpy(), ref["corr"])
        assert np.array_equal(dbg["zmap"].cpu().numpy(), ref["zmap"])
        assert np.allclose(disp[0, 0].cpu().numpy(), ref["disparity"], rtol=0, atol=1e-4)
        assert len(corr) > 10 and not np.array_equal(corr.numpy(), corr0.numpy())
        d2, c2 = DT.transform_depth(*args, *move, depth_transform_mode="mesh", pivot=pivot, scale=1.0)
        assert torch.equal(d2, disp) and torch.equal(c2, corr)
    with pytest.raises(NotImplementedError, match="scale"):
        DT.transform_depth(*args, 10.0, depth_transform_mode="mesh", scale=1.5)
    with pytest.raises(NotImplementedError, match="scale"):
        DT.transform_depth_mesh(*args, 10.0, scale=(1.0, 1.0, 1.1))
