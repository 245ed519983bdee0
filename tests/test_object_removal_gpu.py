"""GPU: object removal (dh_cells_from_correspondences_vacated, dh_reproject_background, depth_transform.reproject_removal_edits,
losses.process_correspondences(vacated=...), the vacated keyword of the guided loops, DiffusionHandles.transform_foreground_objects
/ transform_foregrounds with removed_masks, tools/run_edit.py) against the test-side reference tests/object_removal_ref.py on
the two-sphere scene at 128 and 256 pixels, grid 64, C = 64.  tests/test_object_removal_ref.py asserts on the reference alone
that the fixtures used here have at least 20 vacated cells, an original-background list that the vacated image changes, at
least 100 kept pairs, and target cells on the vacated region in set B and none in set A.  The C entries write into outputs that
are NaN / 0xFF / -1 before the call."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_object_ref as R  # noqa: E402
import object_removal_ref as RR  # noqa: E402
import object_weights_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu
GRID = 64
G2 = GRID * GRID
C_ENERGY = 64
SCALE = 64.0
DH_ERR_ARG = -1          # include/diffhandles_hip.h


def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _t(tf):
    return (float(tf[0]), torch.tensor(tf[1], dtype=torch.float32), torch.tensor(tf[2], dtype=torch.float32)) + tuple(tf[3:])


def _fixture(res, which):
    """tests/object_removal_ref.fixture, computed once per session with the explicit dot order of the kernels."""
    from oracle import depth_ref as D
    D.DOT_ORDER = "explicit"
    try:
        return RR.fixture(res, which)
    finally:
        D.DOT_ORDER = "blas"


def _K():
    from oracle import depth_ref as D
    return D.intrinsics_f32()


# ---- 1. cells ---------------------------------------------------------------------------------------------------------------------
def _cells_call(corr, res, erosion, vacated="none", entry="vacated", ws_cut=0, grid=GRID):
    """One of the two C entries on poisoned outputs.  vacated: "none" (NULL) or a [res, res] array."""
    from diffusionhandles_amd import _lib
    L = _lib.lib()
    c = torch.as_tensor(np.ascontiguousarray(corr), dtype=torch.int64).reshape(-1, 4).to(dev()).contiguous()
    n = c.shape[0]
    nb = ctypes.c_size_t()
    _lib.check(L.dh_cells_workspace_bytes(n, grid, ctypes.byref(nb)))
    ws = torch.full((nb.value,), 0xFF, dtype=torch.uint8, device=dev())
    o = SimpleNamespace(pairs=torch.full((max(n, 1), 2), -1, dtype=torch.int32, device=dev()),
                        lists=torch.full((3, grid * grid), -1, dtype=torch.int32, device=dev()),
                        masks=torch.full((3, grid * grid), 0xFF, dtype=torch.uint8, device=dev()),
                        counts=torch.full((4,), -1, dtype=torch.int32, device=dev()))
    args = (_lib.ptr(c) if n else None, n, res, grid, erosion, _lib.ptr(o.pairs), _lib.ptr(o.lists), _lib.ptr(o.masks),
            _lib.ptr(o.counts), _lib.ptr(ws), nb.value - ws_cut, _lib.stream_ptr())
    if entry == "plain":
        o.rc = L.dh_cells_from_correspondences(*args)
    else:
        vac = None
        if not isinstance(vacated, str):
            vac = torch.as_tensor(np.ascontiguousarray(vacated).astype(np.uint8)).to(dev()).contiguous()
        o.rc = L.dh_cells_from_correspondences_vacated(*args, _lib.ptr(vac))
    o.err = L.dh_last_error().decode() if o.rc != 0 else ""
    torch.cuda.synchronize()
    return o


def _cells_untouched(o):
    assert bool((o.pairs == -1).all()) and bool((o.lists == -1).all()) and bool((o.masks == 0xFF).all()) and bool((o.counts == -1).all())


def _cells_same(a, b, what):
    for k in ("pairs", "lists", "masks", "counts"):
        assert torch.equal(getattr(a, k), getattr(b, k)), f"{what}: {k}"


def _cells_against_ref(o, ref, what):
    assert o.rc == 0, o.err
    counts = o.counts.cpu().tolist()
    n = counts[0]
    pairs = o.pairs[:n].cpu().numpy().astype(np.int64)
    assert n == len(ref["original_x"]), what
    assert np.array_equal(pairs[:, 0], ref["original_y"] * GRID + ref["original_x"]), f"{what}: source cells"
    assert np.array_equal(pairs[:, 1], ref["transformed_y"] * GRID + ref["transformed_x"]), f"{what}: target cells"
    assert bool((o.pairs[n:] == -1).all())
    for k, name in enumerate(("background", "background_orig", "background_trans")):
        y, x = (f"background_y{name[10:]}", f"background_x{name[10:]}")
        want = ref[y] * GRID + ref[x]
        assert counts[1 + k] == len(want), f"{what}: {name} count {counts[1 + k]} / {len(want)}"
        assert np.array_equal(o.lists[k, :len(want)].cpu().numpy().astype(np.int64), want), f"{what}: {name} list"
        assert bool((o.lists[k, len(want):] == -1).all())
    assert np.array_equal(o.masks.cpu().numpy().reshape(3, GRID, GRID), ref["masks"]), f"{what}: masks"


@pytest.mark.parametrize("er", [0, 5])
@pytest.mark.parametrize("res", [128, 256])
@pytest.mark.parametrize("which", ["A", "B"])
def test_cells_with_a_vacated_image_against_the_reference(which, res, er):
    f = _fixture(res, which)
    corr = f["corr"].numpy()
    o = _cells_call(corr, res, er, f["vacated"])
    _cells_against_ref(o, f[f"cells{er}"], f"set {which} at {res}, erosion {er}")
    _cells_same(o, _cells_call(corr, res, er, f["vacated"]), "second run")
    plain = _cells_call(corr, res, er, entry="plain")
    assert not torch.equal(plain.lists[1], o.lists[1]) and torch.equal(plain.lists[2], o.lists[2]) and torch.equal(plain.pairs, o.pairs)
    # NULL and an all-zero image: the entry the library always had, byte for byte
    _cells_against_ref(plain, f[f"plain{er}"], "plain entry")
    _cells_same(plain, _cells_call(corr, res, er, "none"), "NULL")
    _cells_same(plain, _cells_call(corr, res, er, np.zeros((res, res), dtype=np.uint8)), "all-zero image")


@pytest.mark.parametrize("er", [0, 5])
def test_cells_border_blob_pure_removal_and_a_full_image(er):
    vac, corr = RR.border_blob(128)
    _cells_against_ref(_cells_call(corr, 128, er, vac), RR.cells(corr, 128, vac, er), f"border blob, erosion {er}")
    # n == 0 with a vacated image: the pure removal
    empty = np.zeros((0, 4), dtype=np.int64)
    f = _fixture(128, "A")
    o = _cells_call(empty, 128, er, f["vacated"])
    ref = RR.cells(empty, 128, f["vacated"], er)
    _cells_against_ref(o, ref, f"pure removal, erosion {er}")
    assert int(o.counts[0]) == 0 and 0 < int(o.counts[2]) < G2 and int(o.counts[3]) == (G2 if er == 0 else (GRID - 2 * er) ** 2)
    # a vacated image that covers every cell: the original list is empty
    full = np.zeros((128, 128), dtype=np.uint8)
    full[::2, ::2] = 7                                                  # one pixel per 2 x 2 cell, any non-zero value
    o = _cells_call(f["corr"].numpy(), 128, er, full)
    _cells_against_ref(o, RR.cells(f["corr"].numpy(), 128, full, er), f"full image, erosion {er}")
    assert int(o.counts[2]) == 0 and int(o.counts[1]) == 0 and int(o.counts[3]) > 0


def test_cells_refusals_leave_the_outputs_untouched():
    f = _fixture(128, "A")
    corr = f["corr"].numpy()
    for kw, word in ((dict(res=100), "bad sizes"), (dict(ws_cut=4096 + 64), "workspace too small"), (dict(grid=256), "bad sizes"),
                     (dict(grid=192, res=192 * 2), "grid too large")):
        res = kw.pop("res", 128)
        vac = np.ones((res, res), dtype=np.uint8)
        o = _cells_call(corr % min(res, 128), res, 0, vac, **kw)
        assert o.rc == DH_ERR_ARG and word in o.err, (kw, o.err)
        _cells_untouched(o)


# ---- 2. geometry with M >= 1 --------------------------------------------------------------------------------------------------------
DBG_KEYS = ("zmap", "raw_mask", "clean_mask", "vis", "target_xy", "counts", "fg_pix", "corr_dev")


def _same_results(a, b, what, keys=DBG_KEYS):
    (ra, da), (rb, db) = a, b
    assert len(ra) == len(rb)
    for e, (x, y) in enumerate(zip(ra, rb)):
        assert len(x) == len(y)
        for u, v in zip(x, y):
            assert u.dtype == v.dtype and torch.equal(u.cpu(), v.cpu()), f"{what}: edit {e}"
    for k in keys:
        u, v = da[k], db[k]
        if k == "corr_dev":          # rows past the counts are not written
            for e in range(len(ra)):
                n = int(da["counts"][e, 0])
                assert torch.equal(u[e, :n], v[e, :n]), f"{what}: {k}"
            continue
        assert torch.equal(torch.as_tensor(u).cpu(), torch.as_tensor(v).cpu()), f"{what}: {k}"
    for k in ("obj_start", "inst_start"):
        if k in da or k in db:
            assert np.array_equal(da[k], db[k]), f"{what}: {k}"
    if "corr_inst" in da or "corr_inst" in db:
        for e in range(len(ra)):
            n = int(da["counts"][e, 0])
            assert torch.equal(da["corr_inst"][e, :n], db["corr_inst"][e, :n]), f"{what}: corr_inst"


@pytest.mark.parametrize("footprints", [False, True])
@pytest.mark.parametrize("res", [128, 256])
def test_removed_object_contributes_no_point(res, footprints):
    """reproject_removal_edits with sphere 1 removed = reproject_instance_edits on sphere 0 alone, every output byte: K = 2
    edits (set A and a second transform), footprints off and on, and with the instance table [0, 0]."""
    from diffusionhandles_amd import depth_transform as DT
    f = _fixture(res, "A")
    depth, bg = f["depth"].to(dev()), f["bg_depth"].to(dev())
    m0, m1 = (m.to(dev()) for m in f["masks"])
    edits = [[_t(RR.SET_A[0])], [_t(RR.SECOND_EDIT[0])]]
    kw = dict(return_debug=True, footprints=footprints)
    alone = DT.reproject_instance_edits(depth, bg, [m0], _K(), edits, **kw)
    removed = DT.reproject_removal_edits(depth, bg, [m0], _K(), edits, removed_masks=[m1], **kw)
    _same_results(removed, alone, f"{res}, footprints {footprints}")
    assert np.array_equal(removed[1]["vacated"].cpu().numpy() != 0, f["vacated"])
    if not footprints:
        assert torch.equal(removed[0][0][1], f["corr"])                  # and the reference's correspondences, order included
        assert float((removed[0][0][0].cpu() - f["disparity"]).abs().max()) < 2e-3
    two = [[_t(RR.SET_A[0]), _t(RR.SECOND_EDIT[0])], [_t(RR.SECOND_EDIT[0]), _t(RR.SET_B[0])]]
    kw2 = dict(kw, instances=[0, 0], return_instances=True)
    _same_results(DT.reproject_removal_edits(depth, bg, [m0], _K(), two, removed_masks=[m1], **kw2),
                  DT.reproject_instance_edits(depth, bg, [m0], _K(), two, **kw2), f"{res}, footprints {footprints}, table [0, 0]")
    # None, [] and all-empty masks: the parent's call (on both spheres)
    both = [[_t(RR.SET_A[0]), _t(RR.SECOND_EDIT[0])]]
    parent = DT.reproject_instance_edits(depth, bg, [m0, m1], _K(), both, **kw)
    for removed_masks in (None, [], [torch.zeros_like(m0)], [torch.zeros_like(m0), torch.zeros_like(m0)]):
        got = DT.reproject_removal_edits(depth, bg, [m0, m1], _K(), both, removed_masks=removed_masks, **kw)
        _same_results(got, parent, f"removed_masks={removed_masks if not removed_masks else 'empty masks'}")
        assert ("vacated" in got[1]) == (removed_masks is not None)
        assert removed_masks is None or not bool(got[1]["vacated"].any())


def test_overlap_is_refused_with_device_masks_before_the_library_runs():
    from diffusionhandles_amd import depth_transform as DT
    f = _fixture(128, "A")
    depth, bg = f["depth"].to(dev()), f["bg_depth"].to(dev())
    m0, m1 = (m.to(dev()) for m in f["masks"])
    with pytest.raises(ValueError, match="removed mask 0 overlaps foreground mask 0"):
        DT.reproject_removal_edits(depth, bg, [m0], _K(), [[_t(RR.SET_A[0])]], removed_masks=[m0.clone()])
    with pytest.raises(ValueError, match="removed mask 1 overlaps removed mask 0"):
        DT.reproject_removal_edits(depth, bg, [], _K(), [[]], removed_masks=[m1, m1.clone()])


# ---- 3. the pure removal ------------------------------------------------------------------------------------------------------------
def _background_call(bg, res, bounds=None, ws_cut=0, null=None, K_unproject=None):
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd import depth_transform as DT
    L = _lib.lib()
    b = bg.to(dev(), torch.float32).contiguous()
    gx, gy = DT._grids(res, res, dev())
    intr = _K()
    ifx, ify = DT._inv_focal(intr if K_unproject is None else K_unproject)
    nb = ctypes.c_size_t()
    _lib.check(L.dh_reproject_background_workspace_bytes(res, ctypes.byref(nb)))
    ws = torch.full((nb.value,), 0xFF, dtype=torch.uint8, device=dev())
    nan = float("nan")
    o = SimpleNamespace(zmap=torch.full((res, res), nan, device=dev()), disp=torch.full((res, res), nan, device=dev()),
                        counts=torch.full((4,), -1, dtype=torch.int32, device=dev()))
    bd = None if bounds is None else torch.tensor(bounds, dtype=torch.float32, device=dev())
    ptrs = dict(bg=_lib.ptr(b), zmap=_lib.ptr(o.zmap), disp=_lib.ptr(o.disp), counts=_lib.ptr(o.counts))
    if null:
        ptrs[null] = None
    o.rc = L.dh_reproject_background(ptrs["bg"], res, _lib.ptr(gx), _lib.ptr(gy), ifx, ify, float(intr[0, 0]), float(intr[1, 1]),
                                     _lib.ptr(bd), ptrs["zmap"], ptrs["disp"], ptrs["counts"], _lib.ptr(ws), nb.value - ws_cut,
                                     _lib.stream_ptr())
    o.err = L.dh_last_error().decode() if o.rc != 0 else ""
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("res", [128, 256])
def test_background_alone_against_the_reference(res, bounded):
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    f = _fixture(res, "A")
    depth, bg, masks = f["depth"], f["bg_depth"], f["masks"]
    lo_hi = D.normalize_depth(1.0 / depth)[1] if bounded else None
    ref, dbg = RR.background_alone(bg, bounds=lo_hi)
    o = _background_call(bg, res, None if lo_hi is None else [float(lo_hi[0]), float(lo_hi[1])])
    assert o.rc == 0, o.err
    assert np.array_equal(o.zmap.cpu().numpy(), dbg["zmap"]), "zmap"
    assert o.counts.cpu().tolist()[:3] == [0, 0, int(dbg["unowned"].sum())] and int(o.counts[3]) >= 0
    err = float((o.disp.cpu() - ref[0, 0]).abs().max())
    print(f"background alone at {res}, bounds {bounded}: {int(dbg['unowned'].sum())} pixels without an owner, disparity max abs err {err:.2e}")
    assert err < 2e-3
    o2 = _background_call(bg, res, None if lo_hi is None else [float(lo_hi[0]), float(lo_hi[1])])
    assert torch.equal(o2.disp, o.disp) and torch.equal(o2.zmap, o.zmap)
    # through the host call: K identical results, zero masks, no correspondences -- and not the empty-mask result
    out, d = DT.reproject_removal_edits(depth.to(dev()), bg.to(dev()), [], _K(), [[], []], removed_masks=[masks[1].to(dev())],
                                        use_input_depth_normalization=bounded, return_debug=True)
    assert len(out) == 2
    for disp, corr in out:
        assert torch.equal(disp[0, 0], o.disp) and tuple(corr.shape) == (0, 4) and corr.dtype == torch.int64
    assert not bool(d["raw_mask"].any()) and not bool(d["clean_mask"].any()) and tuple(d["raw_mask"].shape) == (2, res, res)
    assert torch.equal(d["zmap"][1], o.zmap) and tuple(d["vis"].shape) == (2, 0) and tuple(d["corr_dev"].shape) == (2, 0, 4)
    assert np.array_equal(d["vacated"].cpu().numpy() != 0, f["vacated"])
    (empty_mask, _), = DT.reproject_object_edits(depth.to(dev()), bg.to(dev()), [torch.zeros_like(masks[0]).to(dev())], _K(),
                                                 [[_t(RR.SET_A[0])]], use_input_depth_normalization=bounded)
    on_object = masks[1][0, 0].bool()
    assert float((out[0][0].cpu() - empty_mask.cpu())[0, 0][on_object].abs().median()) > 10.0
    # every fg mask empty and an object removed is the pure removal too (the empty masks are dropped with their transforms)
    (dropped, c), = DT.reproject_removal_edits(depth.to(dev()), bg.to(dev()), [torch.zeros_like(masks[0]).to(dev())], _K(),
                                               [[_t(RR.SET_A[0])]], removed_masks=[masks[1].to(dev())],
                                               use_input_depth_normalization=bounded)
    assert torch.equal(dropped, out[0][0]) and c.shape[0] == 0


@pytest.mark.parametrize("res", [128, 256])
def test_background_alone_fills_the_pixels_no_point_owns(res):
    """On the fixtures every pixel has an owner, so the in-fill of the entry has nothing to do there.  Here the entry gets the
    inverse focal terms of a longer lens than the one it projects with: the picture shrinks to 0.8 of its size, several points
    share a pixel (the z-buffer decides) and a frame of pixels is left without an owner, which the harmonic in-fill solves."""
    _, bg, _ = R.two_spheres(res)
    longer = _K().clone()
    longer[0, 0] *= 1.25
    longer[1, 1] *= 1.25
    ref, dbg = RR.background_alone(bg, K_unproject=longer)
    n = int(dbg["unowned"].sum())
    assert n > res * res // 4 and dbg["unowned"][0].all() and not dbg["unowned"][res // 2, res // 2]
    o = _background_call(bg, res, K_unproject=longer)
    assert o.rc == 0, o.err
    assert np.array_equal(o.zmap.cpu().numpy(), dbg["zmap"]), "zmap"
    counts = o.counts.cpu().tolist()
    assert counts[:3] == [0, 0, n] and counts[3] > 0
    err = float((o.disp.cpu() - ref[0, 0]).abs().max())
    print(f"background alone at {res}, shrunk picture: {n} pixels in-filled in {counts[3]} CG iterations, disparity max abs err {err:.2e}")
    assert err < 2e-3
    again = _background_call(bg, res, K_unproject=longer)
    assert torch.equal(again.disp, o.disp) and torch.equal(again.counts, o.counts)


def test_background_entry_refusals_leave_the_outputs_untouched():
    _, bg, _ = R.two_spheres(128)
    for kw, word in ((dict(ws_cut=1 << 16), "workspace too small"), (dict(null="bg"), "null input"), (dict(null="counts"), "null output")):
        o = _background_call(bg, 128, **kw)
        assert o.rc == DH_ERR_ARG and word in o.err, (kw, o.err)
        assert torch.isnan(o.zmap).all() and torch.isnan(o.disp).all() and bool((o.counts == -1).all())


# ---- 4. the energy ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def energy():
    """Sets A and B at 256 pixels and the pure removal: the correspondences of the library, the cells of the library with the
    vacated image (asserted equal to the reference's) and of the reference, maps whose ORIGINAL carries the removed object's
    features on the vacated cells (+4 on every channel there: what would pour into the background mean)."""
    from diffusionhandles_amd import depth_transform as DT
    from diffusionhandles_amd.losses import process_correspondences
    res = 256
    cases = {}
    for which in ("A", "B", "pure"):
        f = _fixture(res, "A" if which == "pure" else which)
        depth, bg = f["depth"].to(dev()), f["bg_depth"].to(dev())
        m0, m1 = (m.to(dev()) for m in f["masks"])
        if which == "pure":
            (_, corr), = DT.reproject_removal_edits(depth, bg, [], _K(), [[]], removed_masks=[m1])
            ref = {er: RR.cells(np.zeros((0, 4), dtype=np.int64), res, f["vacated"], er) for er in (0, 5)}
        else:
            (_, corr), = DT.reproject_removal_edits(depth, bg, [m0], _K(), [[_t(tf) for tf in f["transforms"]]], removed_masks=[m1])
            assert torch.equal(corr, f["corr"])
            ref = {0: f["cells0"], 5: f["cells5"]}
        vac = torch.from_numpy(f["vacated"].astype(np.uint8)).to(dev())
        pc = process_correspondences(corr, res, 0, device=dev(), vacated=vac)
        for k in RR.CELL_KEYS:
            assert np.array_equal(np.asarray(pc[k]), ref[0][k]), (which, k)
        plain = process_correspondences(corr, res, 0, device=dev())
        assert set(pc) == set(plain) and len(pc["background_x_orig"]) < len(plain["background_x_orig"])
        cases[which] = SimpleNamespace(pc=pc, plain=plain, cells=ref[0], corr=corr, vac=vac, f=f)
    maps = {}
    vc = torch.from_numpy(RR.vacated_cells(_fixture(res, "A")["vacated"]))
    for dtype in (torch.float16, torch.bfloat16):
        g = torch.Generator().manual_seed(22)
        act = torch.randn(GRID, GRID, C_ENERGY, generator=g)
        orig = torch.randn(GRID, GRID, C_ENERGY, generator=g)
        orig[vc] += 4.0
        maps[dtype] = (act.to(dtype).to(dev()), orig.to(dtype).to(dev()))
    return SimpleNamespace(cases=cases, maps=maps, vc=vc)


def _check_energy(loss, grad, ref_loss, ref_grad, what):
    """loss within 2e-5 relative, gradient within 1e-4 of its largest entry (tests/test_geometry_gpu.py)."""
    got = [float(v) for v in loss.cpu()]
    ref = ref_grad.double().cpu() * SCALE
    err, top = float((grad.double().cpu() - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: loss {got} / reference {list(ref_loss)}; gradient max abs err {err:.3e}, max |ref| {top:.3e}")
    assert torch.isfinite(grad).all()
    for g, r in zip(got, ref_loss):
        assert abs(g - r) <= 2e-5 * max(abs(r), 1e-30) or (r == 0.0 and g == 0.0), (what, got, ref_loss)
    assert top > 0 and err <= 1e-4 * top, what


def _weighted_ref(act, orig, cells, objects, weights, fw, bw):
    """tests/object_weights_ref.energy (omega-weighted foreground term) on this file's grid: ((total, fg, bg), gradient [h,w,C])."""
    a = act.detach().double().cpu().permute(2, 0, 1).contiguous().requires_grad_(True)
    o = orig.detach().double().cpu().permute(2, 0, 1).contiguous()
    tot, fg, bg = W.energy(a, o, cells, objects, weights, fw, bw, size=(GRID, GRID))
    grad, = torch.autograd.grad(tot, a)
    return (float(tot.detach()), float(fg.detach()), float(bg.detach())), grad.permute(1, 2, 0).contiguous()


def _planned(act, orig, plan, fw, bw):
    from diffusionhandles_amd.losses import energy_and_grad_planned
    out = torch.full((GRID, GRID, C_ENERGY), float("nan"), dtype=torch.float32, device=dev())
    loss, grad = energy_and_grad_planned(act, orig, plan, fw, bw, grad_scale=SCALE, want_loss=True, out=out, grad_dtype=torch.float32)
    torch.cuda.synchronize()
    return loss, grad


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("which", ["A", "B", "pure"])
def test_energy_on_the_cells_with_vacated(energy, which, dtype):
    """global_avg through the planned single entry and the general entry, local_avg through the general entry, against
    oracle.guidance_ref on the reference cells.  Without pairs the foreground term is absent and the background runs alone."""
    from diffusionhandles_amd.losses import EnergyPlan, energy_and_grad
    c = energy.cases[which]
    act, orig = energy.maps[dtype]
    fw, bw = (0.0 if which == "pure" else 7.5), 1.5
    plan = EnergyPlan(c.pc, GRID, dev())
    assert not plan.weighted and plan.n_pairs == len(c.cells["original_x"]) and (plan.n_pairs == 0) == (which == "pure")
    ref_loss, ref_grad = RR.energy_and_grad(act, orig, c.cells, fw, bw)
    loss, grad = _planned(act, orig, plan, fw, bw)
    _check_energy(loss, grad, ref_loss, ref_grad, f"{which} planned global_avg")
    for kind in ("global_avg", "local_avg"):
        if kind == "local_avg":
            ref_loss, ref_grad = RR.energy_and_grad(act, orig, c.cells, fw, bw, "local_avg")
        out = torch.full((GRID, GRID, C_ENERGY), float("nan"), dtype=torch.float32, device=dev())
        l2, g2 = energy_and_grad(act, orig, c.pc, fw, bw, bg_loss_type=kind, grad_scale=SCALE, grad_dtype=torch.float32, out=out)
        _check_energy(l2, g2, ref_loss, ref_grad, f"{which} general {kind}")
        if kind == "local_avg":
            # vacated cells carry no identity pair: no gradient of the background term lands on them unless a target does
            pure_bg = energy.vc & ~torch.from_numpy(c.cells["masks"][2] == 0)
            _, gb = energy_and_grad(act, orig, c.pc, 0.0, bw, bg_loss_type=kind, grad_scale=SCALE, grad_dtype=torch.float32)
            assert float(gb.cpu()[pure_bg].abs().max()) == 0.0
            _, gp = energy_and_grad(act, orig, c.plain, 0.0, bw, bg_loss_type=kind, grad_scale=SCALE, grad_dtype=torch.float32)
            assert float(gp.cpu()[pure_bg].abs().max()) > 0.0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_vacated_takes_the_object_out_of_the_background_mean(energy, dtype):
    """The discriminating case, set A under global_avg: the removed object's features sit on the vacated cells of the original
    maps.  Without `vacated` they are in the mean the edited background is pulled towards; with it the gradient on the
    background cells differs from that one and matches the reference."""
    from diffusionhandles_amd.losses import EnergyPlan
    c = energy.cases["A"]
    act, orig = energy.maps[dtype]
    bg_cells = torch.from_numpy(c.cells["masks"][2] != 0)
    ref_loss, ref_grad = RR.energy_and_grad(act, orig, c.cells, 7.5, 1.5)
    loss, grad = _planned(act, orig, EnergyPlan(c.pc, GRID, dev()), 7.5, 1.5)
    _check_energy(loss, grad, ref_loss, ref_grad, "set A with vacated")
    loss_p, grad_p = _planned(act, orig, EnergyPlan(c.plain, GRID, dev()), 7.5, 1.5)
    plain_loss, plain_grad = RR.energy_and_grad(act, orig, c.f["plain0"], 7.5, 1.5)
    _check_energy(loss_p, grad_p, plain_loss, plain_grad, "set A without vacated")
    diff = (grad.cpu() - grad_p.cpu())[bg_cells].abs()
    top = float(ref_grad.abs().max()) * SCALE
    print(f"gradient with / without vacated on the background cells: max abs difference {float(diff.max()):.3e} (max |ref| {top:.3e}), "
          f"{int((diff > 0).sum())} entries differ; background loss {float(loss[2]):.4f} / {float(loss_p[2]):.4f}")
    assert float(diff.max()) > 1e-2 * top and float(loss_p[2]) > 2.0 * float(loss[2])
    assert float((grad.cpu() - plain_grad.float() * SCALE)[bg_cells].abs().max()) > 1e-2 * top


def test_energy_batches_mix_removal_plain_and_pure_items(energy):
    """K = 3 in one planned batch -- a removal edit (set A), a plain edit (set B's correspondences without a vacated image) and
    the pure removal -- and the mixed weighted batch with a weighted two-object item beside them: item e is bit-identical to its
    single call, and the removal items match the reference."""
    from diffusionhandles_amd import depth_transform as DT
    from diffusionhandles_amd.losses import (EnergyPlan, energy_and_grad_planned_batch, energy_and_grad_planned_mixed,
                                             object_label_image, process_correspondences)
    act, orig = energy.maps[torch.float16]
    a2, o2 = energy.maps[torch.bfloat16]
    act2, orig2 = a2.to(torch.float16), o2.flip(0).to(torch.float16).contiguous()
    cs = energy.cases
    plans = [EnergyPlan(cs["A"].pc, GRID, dev()), EnergyPlan(cs["B"].plain, GRID, dev()), EnergyPlan(cs["pure"].pc, GRID, dev())]
    acts, origs = [act, act2, act], [orig, orig2, orig2]
    fws, bws = [7.5, 5.0, 0.0], [1.5, 1.5, 2.5]
    singles = [_planned(a, o, p, fw, bw) for a, o, p, fw, bw in zip(acts, origs, plans, fws, bws)]
    outs = [torch.full((GRID, GRID, C_ENERGY), float("nan"), dtype=torch.float32, device=dev()) for _ in range(3)]
    loss, grads = energy_and_grad_planned_batch(acts, origs, plans, fws, bws, [SCALE] * 3, want_loss=True, outs=outs,
                                                grad_dtype=torch.float32)
    for e in range(3):
        assert torch.equal(grads[e], singles[e][1]) and torch.equal(loss[e], singles[e][0]), f"batch item {e}"
    _check_energy(loss[0], grads[0], *RR.energy_and_grad(act, orig, cs["A"].cells, 7.5, 1.5), "batch item 0 (set A)")
    _check_energy(loss[2], grads[2], *RR.energy_and_grad(act, orig2, cs["pure"].cells, 0.0, 2.5), "batch item 2 (pure removal)")
    assert float(loss[2][1]) == 0.0 and float(loss[2][2]) > 0.0
    # the weighted route with a vacated image: sphere 0 cut into a left and a right object, sphere 1 removed
    f = cs["A"].f
    m0, m1 = f["masks"]
    left, right = m0.clone(), m0.clone()
    mid = int(np.nonzero(m0[0, 0].numpy().any(axis=0))[0].mean())
    left[..., mid:], right[..., :mid] = 0, 0
    tfs = [_t(RR.SET_A[0]), _t(RR.SECOND_EDIT[0])]
    (_, corr), = DT.reproject_removal_edits(f["depth"].to(dev()), f["bg_depth"].to(dev()), [left.to(dev()), right.to(dev())], _K(),
                                            [tfs], removed_masks=[m1.to(dev())])
    label = object_label_image([left, right])
    pcw = process_correspondences(corr, 256, 0, device=dev(), vacated=cs["A"].vac, object_labels=label)
    ref_cells = RR.cells(corr.numpy(), 256, f["vacated"], 0)
    for k in RR.CELL_KEYS:
        assert np.array_equal(np.asarray(pcw[k]), ref_cells[k]), k
    objects = np.asarray(pcw["object"])
    assert min(np.bincount(objects, minlength=2)) >= 100
    weighted = EnergyPlan(pcw, GRID, dev(), object_weights=[1.0, 3.0])
    assert weighted.weighted
    lw, gw = _planned(act, orig, weighted, 7.5, 1.5)          # the planned objects entry
    _check_energy(lw, gw, *_weighted_ref(act, orig, ref_cells, objects, [1.0, 3.0], 7.5, 1.5), "weighted objects entry with vacated")
    mixed_plans, mixed_acts, mixed_origs = [weighted] + plans[1:] + plans[:1], [act, act2, act, act], [orig, orig2, orig2, orig]
    mfw, mbw = [7.5, 5.0, 0.0, 7.5], [1.5, 1.5, 2.5, 1.5]
    want = [(lw, gw), singles[1], singles[2], singles[0]]
    outs = [torch.full((GRID, GRID, C_ENERGY), float("nan"), dtype=torch.float32, device=dev()) for _ in range(4)]
    loss, grads = energy_and_grad_planned_mixed(mixed_acts, mixed_origs, mixed_plans, mfw, mbw, [SCALE] * 4, want_loss=True, outs=outs,
                                                grad_dtype=torch.float32)
    for e in range(4):
        assert torch.equal(grads[e], want[e][1]) and torch.equal(loss[e], want[e][0]), f"mixed item {e}"
    # the weighted batch entry: two weighted items, one of them with the vacated image
    pcw_plain = process_correspondences(corr, 256, 0, device=dev(), object_labels=label)
    weighted_plain = EnergyPlan(pcw_plain, GRID, dev(), object_weights="equal")
    lp, gp = _planned(act2, orig2, weighted_plain, 5.0, 1.5)
    outs = [torch.full((GRID, GRID, C_ENERGY), float("nan"), dtype=torch.float32, device=dev()) for _ in range(2)]
    loss, grads = energy_and_grad_planned_batch([act, act2], [orig, orig2], [weighted, weighted_plain], [7.5, 5.0], [1.5, 1.5],
                                                [SCALE] * 2, want_loss=True, outs=outs, grad_dtype=torch.float32)
    assert torch.equal(grads[0], gw) and torch.equal(loss[0], lw) and torch.equal(grads[1], gp) and torch.equal(loss[1], lp)


# ---- 5. the loop level, on the TINY rig of tests/test_object_items_gpu.py -------------------------------------------------------------
RES = 512


@pytest.fixture(scope="module")
def tiny():
    from diffusionhandles_amd import DiffusionHandles
    from diffusionhandles_amd import conf as C
    from diffusionhandles_amd.synthetic import make_scene
    from diffusionhandles_amd.unet import HipUNet
    from oracle import unet_torch as U
    ref = U.init_synthetic_(U.UNetTorch(U.TINY), seed=0).to(dev()).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.half().float())
    hip = HipUNet(dict(U.TINY, text_len=77), dtype=torch.float16, max_batch=4)
    hip.load_state_dict(ref.state_dict())
    dh = DiffusionHandles(C.load_default(), unet=hip, unet_config=dict(U.TINY, text_len=77)).to(dev())

    def identity(depth, prompt, seed):
        g = torch.Generator().manual_seed(seed)
        noise = torch.randn(1, 4, RES // 8, RES // 8, generator=g).to(dev())
        Dm = dh.diffuser.unet.cfg["cross_attention_dim"]
        unc = (dh.diffuser._encode([""])[None].expand(50, -1, -1, -1) + 0.05 * torch.randn(50, 1, 77, Dm, generator=g).to(dev())).contiguous()
        null_text, noise, acts, _ = dh.generate_input_image(depth, prompt, unc, noise)
        return dict(null_text=null_text, noise=noise, acts=acts, prompt=prompt)
    depth, bg, masks = R.two_spheres(RES)
    depth, bg, masks = depth.to(dev()), bg.to(dev()), [m.to(dev()) for m in masks]
    two = SimpleNamespace(depth=depth, bg_depth=dh.set_foreground(depth, masks, bg), masks=masks,
                          **identity(depth, "two spheres on a plane", 11))
    d1, b1, m1 = (t.to(dev()).flip(-1).contiguous() for t in make_scene(RES))
    one = SimpleNamespace(depth=d1, bg_depth=dh.set_foreground(d1, m1, b1), fg_mask=m1, **identity(d1, "a red ball on a wooden table", 12))
    return SimpleNamespace(dh=dh, gd=dh.diffuser, two=two, one=one)


def _common(im):
    return dict(depth=im.depth, prompt=im.prompt, bg_depth=im.bg_depth, null_text_emb=im.null_text, init_noise=im.noise,
                activations=im.acts)


def _loop_tf():
    return _t(RR.SET_A[0])


def _geometry(tiny, pure, device_correspondences=False):
    """What test 2 / test 3 pin: the removal edit's re-projection (sphere 0 alone) or the background alone."""
    from diffusionhandles_amd import depth_transform as DT
    t = tiny.two
    intr = tiny.gd.get_depth_intrinsics(device=dev())
    if pure:
        (d, c), = DT.reproject_removal_edits(t.depth, t.bg_depth, [], intr, [[]], removed_masks=t.masks,
                                             device_correspondences=device_correspondences)
    else:
        (d, c), = DT.reproject_instance_edits(t.depth, t.bg_depth, [t.masks[0]], intr, [[_loop_tf()]],
                                              device_correspondences=device_correspondences)
    return d, c


def test_transform_foreground_objects_with_removed_masks(tiny):
    """One removal edit (sphere 1 deleted, sphere 0 moved) and the pure removal (both spheres deleted): the disparity fed to
    the U-Net is the pinned geometry's, the image is finite and is guided_inference on that geometry with the vacated image."""
    from diffusionhandles_amd import depth_transform as DT
    dh, gd, t = tiny.dh, tiny.gd, tiny.two
    for pure in (False, True):
        fg, removed, tfs = ([], t.masks, []) if pure else ([t.masks[0]], [t.masks[1]], [_loop_tf()])
        img, disp = dh.transform_foreground_objects(**_common(t), fg_masks=fg, transforms=tfs, removed_masks=removed)
        img, lat = img.clone(), gd.last_latents.clone()
        assert img.shape == (1, 3, RES, RES) and torch.isfinite(img).all()
        d, c = _geometry(tiny, pure)
        assert torch.equal(d, disp) and (c.shape[0] == 0) == pure
        ref = gd.guided_inference(t.noise, d, t.null_text, t.prompt, t.acts, c, vacated=DT.vacated_image(removed))
        assert torch.equal(gd.last_latents, lat) and torch.equal(ref, img)
        without = gd.guided_inference(t.noise, d, t.null_text, t.prompt, t.acts, c)
        assert torch.isfinite(without).all() and not torch.equal(gd.last_latents, lat)          # the vacated image reaches the energy
    # the pure removal under the automatic gradient scale: its bound comes from the background coefficient alone
    old = gd.grad_scale_mode
    gd.grad_scale_mode = "auto"
    try:
        img, _ = dh.transform_foreground_objects(**_common(t), fg_masks=[], transforms=[], removed_masks=t.masks)
        assert torch.isfinite(img).all()
    finally:
        gd.grad_scale_mode = old


def test_removal_in_batches_and_on_two_lanes(tiny):
    """transform_foreground_objects_batch with one list of removed masks for K = 2 edits, one stream and two lanes (bit-identical
    at the same batch), and K identical pure removals."""
    from diffusionhandles_amd import depth_transform as DT
    dh, gd, t, o = tiny.dh, tiny.gd, tiny.two, tiny.one
    edits = [[_loop_tf()], [_t(RR.SECOND_EDIT[0])]]
    args = dict(_common(t), fg_masks=[t.masks[0]], edits=edits, removed_masks=[t.masks[1]])
    imgs, disps = dh.transform_foreground_objects_batch(**args)
    imgs, lat = imgs.clone(), gd.last_latents.clone()
    assert imgs.shape == (2, 3, RES, RES) and torch.isfinite(imgs).all()
    rp = DT.reproject_instance_edits(t.depth, t.bg_depth, [t.masks[0]], gd.get_depth_intrinsics(device=dev()), edits,
                                     device_correspondences=True)
    assert all(torch.equal(a, b[0]) for a, b in zip(disps, rp))
    vac = DT.vacated_image([t.masks[1]])
    ref = gd.guided_inference_batch(t.noise, [d for d, _ in rp], t.null_text, t.prompt, t.acts, [c for _, c in rp], vacated=vac)
    assert torch.equal(ref, imgs) and torch.equal(gd.last_latents, lat)
    per_edit = gd.guided_inference_batch(t.noise, [d for d, _ in rp], t.null_text, t.prompt, t.acts, [c for _, c in rp], vacated=[vac, vac])
    assert torch.equal(per_edit, imgs)
    one_stream, _ = dh.transform_foreground_objects_batch(**args, streams=1, batch=1)
    one_stream = one_stream.clone()
    two_lanes, _ = dh.transform_foreground_objects_batch(**args, streams=2, batch=1)
    assert torch.isfinite(two_lanes).all() and torch.equal(two_lanes, one_stream)
    # K identical pure removals: computed once
    pure, pd = dh.transform_foreground_objects_batch(**_common(t), fg_masks=[], edits=[[], []], removed_masks=t.masks)
    assert torch.equal(pd[0], pd[1]) and torch.equal(pd[0], _geometry(tiny, True)[0]) and torch.equal(pure[0], pure[1])


def test_removal_beside_a_plain_edit_of_another_image(tiny):
    """transform_foregrounds with one edit that carries `removed_masks` and one that does not, in one batch: bit-identical to
    guided_inference_items on the re-projections; and a pure removal beside a plain edit."""
    from diffusionhandles_amd import depth_transform as DT
    from diffusionhandles_amd.depth_transform import reproject_edits
    dh, gd, t, o = tiny.dh, tiny.gd, tiny.two, tiny.one
    vac = DT.vacated_image([t.masks[1]])
    from diffusionhandles_amd.synthetic import TRANSFORMS
    single = (TRANSFORMS[5][0], torch.tensor(R.Y), torch.tensor(TRANSFORMS[5][1]))
    batch = [dict(_common(t), fg_masks=[t.masks[0]], transforms=[_loop_tf()], removed_masks=[t.masks[1]]),
             dict(_common(o), fg_mask=o.fg_mask, rot_angle=single[0], rot_axis=single[1], translation=single[2]),
             dict(_common(t), fg_masks=[], removed_masks=t.masks)]
    images, disps = dh.transform_foregrounds(batch[:2])
    images, lat = images.clone(), gd.last_latents.clone()
    assert images.shape == (2, 3, RES, RES) and torch.isfinite(images).all()
    d, c = _geometry(tiny, False, device_correspondences=True)
    (d1, c1), = reproject_edits(o.depth, o.bg_depth, o.fg_mask, gd.get_depth_intrinsics(), [single], device_correspondences=True)
    assert torch.equal(d, disps[0]) and torch.equal(d1, disps[1])
    item = lambda im, dd, cc, **kw: dict(latents=im.noise, depth=dd, uncond_embeddings=im.null_text, prompt=im.prompt,
                                         activations_orig=im.acts, correspondences=cc, **kw)
    ref = gd.guided_inference_items([item(t, d, c, vacated=vac), item(o, d1, c1)])
    assert torch.equal(gd.last_latents, lat) and torch.equal(ref, images)
    images, disps = dh.transform_foregrounds([batch[2], batch[1]])
    assert torch.isfinite(images).all() and torch.equal(disps[0], _geometry(tiny, True)[0]) and torch.equal(disps[1], d1)


def test_background_lock_frees_the_vacated_cells_and_holds_the_rest(tiny):
    dh, gd, t = tiny.dh, tiny.gd, tiny.two
    s = gd.unet.sample_size
    T = int(gd.conf.num_timesteps)
    traj = t.acts.trajectory
    dh.conf["background_lock"] = True
    try:
        for pure in (False, True):
            fg, removed, tfs = ([], t.masks, []) if pure else ([t.masks[0]], [t.masks[1]], [_loop_tf()])
            img, _ = dh.transform_foreground_objects(**_common(t), fg_masks=fg, transforms=tfs, removed_masks=removed)
            keep, = dh.last_keep_maps
            assert torch.isfinite(img).all()
            keep = keep.float().reshape(s, s)
            vac = torch.zeros((RES, RES), dtype=torch.bool, device=dev())
            for m in removed:
                vac |= m[0, 0] != 0
            cells = vac.reshape(s, RES // s, s, RES // s).any(dim=3).any(dim=1)
            assert int(cells.sum()) >= 20 and float(keep[cells].max()) == 0.0
            one = (keep == 1)[None].expand(4, -1, -1)
            assert int(one.sum()) > s * s // 8
            assert torch.equal(gd.last_latents[0][one].float(), traj[T - 1].to(gd.last_latents.device)[one].float())
            assert not torch.equal(gd.last_latents[0].float(), traj[T - 1].to(gd.last_latents.device).float())
    finally:
        dh.conf.pop("background_lock", None)


# ---- 6. the harness on a scene directory with a removed object -------------------------------------------------------------------------
def _run_edit_module():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_edit_tool", os.path.join(root, "tools", "run_edit.py"))
    run_edit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run_edit)
    return run_edit


def test_run_edit_removes_the_object_of_a_scene_directory(tiny, tmp_path):
    """A two-mask scene with the entries `plain`, `drop` (object 1 is {"remove": true}) and `clear` (both removed): run_scene
    and the --edit-batch path hand the removed masks to transform_foreground_objects / transform_foregrounds and write the same
    disparity; with the background lock on, <edit>_keep.png shows the freed region."""
    import argparse
    import json
    from diffusionhandles_amd.scene_io import read_png, write_png
    run_edit = _run_edit_module()
    inp = tmp_path / "set"
    scene = inp / "two_spheres"
    scene.mkdir(parents=True)
    depth, bg, masks = R.two_spheres(RES)
    np.save(scene / "depth.npy", depth[0, 0].numpy())
    np.save(scene / "bg_depth.npy", bg[0, 0].numpy())
    for m, mask in enumerate(masks):
        write_png(str(scene / f"mask_{m}.png"), mask[0, 0].numpy())
    write_png(str(scene / "input.png"), np.full((RES, RES, 3), 0.5, dtype=np.float32))
    (scene / "prompt.txt").write_text("two spheres on a plane\n")
    member = lambda tf, **kw: dict(rotation_angle=tf[0], rotation_axis=list(tf[1]), translation=list(tf[2]), **kw)
    (scene / "transforms.json").write_text(json.dumps({
        "plain": {"objects": [member(RR.SET_A[0]), {}]},
        "drop": {"objects": [member(RR.SET_A[0]), {"remove": True}]},
        "clear": {"objects": [{"remove": True}, {"remove": True}]}}))
    args = argparse.Namespace(res=RES, mode="pc", skip_inversion=True, no_identity_cache=True, identity_cache=None, skip_existing=False,
                              max_edits=0, identity_batch=1, edit_batch=1, edit_batch_images=0, background_lock=True)
    seen = []
    dh = tiny.dh
    count = lambda kw: (len(kw["fg_masks"]), None if kw.get("removed_masks") is None else len(kw["removed_masks"]))
    inner_one, inner_many = dh.transform_foreground_objects, dh.transform_foregrounds
    dh.transform_foreground_objects = lambda *a, **kw: (seen.append(count(dict(kw, fg_masks=a[2]))), inner_one(*a, **kw))[1]
    dh.transform_foregrounds = lambda edits, **kw: (seen.extend(count(e) for e in edits), inner_many(edits, **kw))[1]
    names = ["plain", "drop", "clear"]
    dh.conf["background_lock"] = True
    try:
        report = run_edit.run_scene(args, dh.conf, lambda res: dh, str(scene), str(tmp_path / "one"), None)
        assert [e["name"] for e in report["edits"]] == names and seen == [(2, None), (1, 1), (0, 2)]
        del seen[:]
        args.edit_batch, args.out = 2, str(tmp_path / "batched")
        reports, _ = run_edit.run_test_set_batched(args, dh.conf, lambda res: dh, [("two_spheres", names)], str(inp))
        assert [e["name"] for e in reports[0]["edits"]] == names and seen == [(2, None), (1, 1), (0, 2)]
        # mesh mode is refused before the identity is computed (nothing is written)
        args.mode = "mesh"
        with pytest.raises(NotImplementedError, match="removes an object"):
            run_edit.run_scene(args, dh.conf, lambda res: dh, str(scene), str(tmp_path / "mesh"), None)
        assert not os.path.exists(tmp_path / "mesh" / "recon.png")
    finally:
        del dh.transform_foreground_objects, dh.transform_foregrounds
        dh.conf.pop("background_lock", None)
    for name in names:
        one, many = read_png(str(tmp_path / "one" / f"{name}.png")), read_png(str(tmp_path / "batched" / "two_spheres" / f"{name}.png"))
        assert one.shape == (RES, RES, 3) and one.std() > 0 and many.std() > 0
        d_one = read_png(str(tmp_path / "one" / f"{name}_disparity.png"))
        assert np.array_equal(d_one, read_png(str(tmp_path / "batched" / "two_spheres" / f"{name}_disparity.png")))
    # the removed sphere is gone from the disparity, and its cells are free in the keep map
    gone = masks[1][0, 0].numpy() > 0.5
    drop, plain = (read_png(str(tmp_path / "one" / f"{n}_disparity.png")).astype(np.float64) for n in ("drop", "plain"))
    assert (drop != plain)[gone].mean() > 0.5
    keep = read_png(str(tmp_path / "one" / "drop_keep.png")).astype(np.float64)
    keep = keep.reshape(keep.shape[0], keep.shape[1], -1)[..., 0]
    s = keep.shape[0]
    cells = gone.reshape(s, RES // s, s, RES // s).any(axis=(1, 3))
    assert keep[cells].max() == 0 and keep.max() > 0
