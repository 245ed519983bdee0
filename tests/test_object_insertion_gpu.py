"""GPU: object insertion (dh_reproject_donor_edits, dh_cells_from_correspondences_donor, dh_energy_fwd_bwd_planned_donor[_batch],
depth_transform.reproject_donor_edits, losses.process_correspondences(row_donor=...), prepare_guidance / guided_inference /
transform_foreground_objects[_batch] with donor) against the test-side reference tests/object_insertion_ref.py: two_spheres as the
host and a one-sphere donor scene at 128 and 256 pixels, grid 64 -- the sizes of the other geometry tests (CLOSE element
res // 50 >= 2, bit-row morphology, more than one workgroup per kernel).  The C entries write into outputs that are NaN / 0xFF /
-1 before the call (the helpers of tests/test_object_copies_gpu.py, whose entry this one extends)."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_object_ref as R  # noqa: E402
import object_insertion_ref as I  # noqa: E402
import test_object_copies_gpu as OC  # noqa: E402  (helpers only: _setup, _rows, _call, _check_against_ref, _same_bytes, _untouched)

pytestmark = pytest.mark.gpu
GRID = I.GRID
DH_ERR_ARG = -1
SCALE = 64.0
C_ENERGY = (64, 320)          # the channel counts of tests/test_object_weights_gpu.py


def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


_t = OC._t


# ---- 1. geometry ------------------------------------------------------------------------------------------------------------------
def _setup(fx):
    """The device inputs of the C entry: host and donor masks concatenated in one pixel list, and the donor depth."""
    s = OC._setup(fx["depth"], fx["bg_depth"], list(fx["masks"]) + list(fx["donor_masks"]))
    s.donor = fx["donor_depth"].to(dev(), torch.float32).contiguous()
    s.n_host = len(fx["masks"])
    return s


def _donor_call(s, rows, inst, donor="own", n_host=None, footprints=0, null_inst=False):
    """dh_reproject_donor_edits on poisoned outputs.  donor: "own" (the setup's donor depth), None (NULL) or a tensor."""
    from diffusionhandles_amd import _lib
    L, res, M = s.L, s.res, s.M
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    N = len(inst)
    K = rows.shape[0] // N
    sizes = np.diff(s.obj_start)
    n_pts = int(sum(int(sizes[o]) for o in inst))
    cap = res * res if footprints else n_pts
    nb = ctypes.c_size_t()
    _lib.check(L.dh_reproject_donor_workspace_bytes(res, n_pts, K, M, N, footprints, ctypes.byref(nb)))
    same = ctypes.c_size_t()
    _lib.check(L.dh_reproject_instances_workspace_bytes(res, n_pts, K, M, N, footprints, ctypes.byref(same)))
    assert nb.value == same.value
    ws = torch.full((nb.value,), 0xFF, dtype=torch.uint8, device=dev())
    nan = float("nan")
    o = SimpleNamespace(
        zmap=torch.full((K, res, res), nan, device=dev()), disp=torch.full((K, res, res), nan, device=dev()),
        raw=torch.full((K, res, res), 0xFF, dtype=torch.uint8, device=dev()),
        clean=torch.full((K, res, res), 0xFF, dtype=torch.uint8, device=dev()),
        vis=torch.full((K, n_pts), 0xFF, dtype=torch.uint8, device=dev()),
        txy=torch.full((K, n_pts, 2), -1, dtype=torch.int32, device=dev()),
        corr=torch.full((K, cap, 4), -1, dtype=torch.int64, device=dev()),
        inst=torch.full((K, cap), 0xFF, dtype=torch.uint8, device=dev()),
        counts=torch.full((K, 4), -1, dtype=torch.int32, device=dev()), n_pts=n_pts)
    dd = s.donor if isinstance(donor, str) else donor
    tab = np.asarray(inst, dtype=np.int32)
    o.rc = L.dh_reproject_donor_edits(
        _lib.ptr(s.d), _lib.ptr(s.b), _lib.ptr(s.fg_pix), s.n_fg, M, s.obj_start.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
        res, _lib.ptr(s.gx), _lib.ptr(s.gy), s.ifx, s.ify, s.fx, s.fy, K, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
        None, _lib.ptr(o.zmap), _lib.ptr(o.raw), _lib.ptr(o.clean), _lib.ptr(o.disp), _lib.ptr(o.vis), _lib.ptr(o.txy),
        _lib.ptr(o.corr), _lib.ptr(o.counts), _lib.ptr(ws), nb.value, s.st, footprints, 0.0, cap, N,
        tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None if null_inst else _lib.ptr(o.inst), _lib.ptr(dd),
        s.n_host if n_host is None else n_host)
    o.err = L.dh_last_error().decode() if o.rc != 0 else ""
    torch.cuda.synchronize()
    o.counts_h = o.counts.cpu()
    if o.rc == 0:
        assert torch.isfinite(o.disp).all() and not torch.isnan(o.zmap).any()
        assert int(o.raw.max()) <= 1 and int(o.clean.max()) <= 1 and int(o.vis.max()) <= 1
        assert int(o.txy.min()) >= 0 and int(o.txy.max()) < res and (o.counts_h[:, 3] >= 0).all()
        for e in range(K):
            n = int(o.counts_h[e, 0])
            assert 0 < n <= cap and bool((o.corr[e, n:] == -1).all()) and bool((o.inst[e, n:] == 0xFF).all())
    return o


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("which", ["overlap", "disjoint"])
@pytest.mark.parametrize("res", [128, 256])
def test_donor_edits_against_the_reference(res, which, K):
    """Host spheres 0 and 1 and the donor sphere (scaled, turned about a pivot): integer maps, the correspondences with their
    order, corr_inst and the counts bit-exact, the disparity within 2e-3 of 255."""
    fx = I.fixture(res, which)
    s = _setup(fx)
    o = _donor_call(s, OC._rows(fx["edits"][:K]), fx["instances"])
    assert o.rc == 0, o.err
    for e in range(K):
        ref = fx["geo"][e]
        OC._check_against_ref(o, e, ref, f"res {res} {which} K {K} edit {e}")
        n = int(o.counts_h[e, 0])
        flags = np.asarray(fx["instances"])[o.inst[e, :n].cpu().numpy()] >= s.n_host
        assert np.array_equal(flags.astype(np.uint8), ref[2]["row_donor"]) and flags.sum() >= 50
    # the host layer: the same rows, the instance array always, row_donor in the debug dict
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    res_list, dbg = DT.reproject_donor_edits(fx["depth"].to(dev()), fx["bg_depth"].to(dev()), [m.to(dev()) for m in fx["masks"]],
                                             D.intrinsics_f32(), [[_t(tf) for tf in tfs] for tfs in fx["edits"][:K]],
                                             fx["instances"], donor_depth=fx["donor_depth"].to(dev()),
                                             donor_masks=[m.to(dev()) for m in fx["donor_masks"]], return_debug=True)
    for e, item in enumerate(res_list):
        assert len(item) == 3
        n = int(o.counts_h[e, 0])
        assert torch.equal(item[1], o.corr[e, :n].cpu()) and torch.equal(item[2], o.inst[e, :n].cpu())
        assert torch.equal(item[0][0, 0].to(dev()), o.disp[e])
        assert np.array_equal(dbg["row_donor"][e, :n].cpu().numpy(), fx["geo"][e][2]["row_donor"])


@pytest.mark.parametrize("res", [128, 256])
def test_donor_depth_equal_to_the_host_depth_is_the_instance_entry(res):
    """donor_depth == depth with n_host_objects < n_objects gives the bytes of dh_reproject_instance_edits."""
    depth, bg, masks = R.two_spheres(res)
    fx = dict(depth=depth, bg_depth=bg, masks=masks[:1], donor_masks=masks[1:], donor_depth=depth)
    s = _setup(fx)
    rows = OC._rows([I.edits_for(depth, "overlap")[0][:2], I.edits_for(depth, "overlap")[1][:2]])
    base = OC._call(s, rows, inst=[0, 1])
    assert base.rc == 0, base.err
    for n_host in (0, 1, 2):
        o = _donor_call(s, rows, [0, 1], donor=s.d, n_host=n_host)
        assert o.rc == 0, o.err
        OC._same_bytes(o, base, f"res {res} n_host {n_host}")
        assert torch.equal(o.inst, base.inst)
    o = _donor_call(s, rows, [0, 1], donor=None, n_host=2)          # the entry's own identity call
    assert o.rc == 0, o.err
    OC._same_bytes(o, base, f"res {res} NULL donor")


@pytest.mark.parametrize("which", ["overlap", "disjoint"])
@pytest.mark.parametrize("res", [128, 256])
def test_pure_insertion(res, which):
    """M = 0: no host mask, bg_depth is the host depth, the donor sphere alone is drawn into it."""
    fx = I.fixture(res, which, True)
    s = _setup(fx)
    assert s.n_host == 0
    o = _donor_call(s, OC._rows(fx["edits"]), fx["instances"])
    assert o.rc == 0, o.err
    for e in range(2):
        OC._check_against_ref(o, e, fx["geo"][e], f"pure res {res} {which} edit {e}")
        assert fx["geo"][e][2]["row_donor"].all()


def test_geometry_refusals_leave_the_outputs_untouched():
    fx = I.fixture(128, "overlap")
    s = _setup(fx)
    rows = OC._rows(fx["edits"][:1])
    inst = fx["instances"]
    for what, kw in (("null donor", dict(donor=None)), ("n_host -1", dict(n_host=-1)), ("n_host 4", dict(n_host=4)),
                     ("footprints", dict(footprints=1)), ("null corr_inst", dict(null_inst=True))):
        o = _donor_call(s, rows, inst, **kw)
        assert o.rc == DH_ERR_ARG and o.err, what
        OC._untouched(o)
        print(f"{what}: {o.err}")


# ---- 2. cells ---------------------------------------------------------------------------------------------------------------------
def _cells_call(corr, res, erosion, row_donor="none", entry="donor", vacated=None):
    """One of the C entries on poisoned outputs.  row_donor: "none" (NULL) or an [n] array."""
    from diffusionhandles_amd import _lib
    L = _lib.lib()
    c = torch.as_tensor(np.asarray(corr)).reshape(-1, 4).to(dev(), torch.int64).contiguous()
    n = c.shape[0]
    nb = ctypes.c_size_t()
    _lib.check(L.dh_cells_workspace_bytes(n, GRID, ctypes.byref(nb)))
    ws = torch.full((nb.value,), 0xFF, dtype=torch.uint8, device=dev())
    o = SimpleNamespace(pairs=torch.full((max(n, 1), 2), -1, dtype=torch.int32, device=dev()),
                        lists=torch.full((3, GRID * GRID), -1, dtype=torch.int32, device=dev()),
                        masks=torch.full((3, GRID * GRID), 0xFF, dtype=torch.uint8, device=dev()),
                        counts=torch.full((4,), -1, dtype=torch.int32, device=dev()))
    args = (_lib.ptr(c), n, res, GRID, erosion, _lib.ptr(o.pairs), _lib.ptr(o.lists), _lib.ptr(o.masks), _lib.ptr(o.counts),
            _lib.ptr(ws), nb.value, _lib.stream_ptr())
    vac = None if vacated is None else torch.as_tensor(vacated).to(dev(), torch.uint8).contiguous()
    if entry == "vacated":
        o.rc = L.dh_cells_from_correspondences_vacated(*args, _lib.ptr(vac))
    else:
        flags = None if isinstance(row_donor, str) else torch.as_tensor(np.asarray(row_donor)).to(dev(), torch.uint8).contiguous()
        o.rc = L.dh_cells_from_correspondences_donor(*args, _lib.ptr(vac), _lib.ptr(flags))
    o.err = L.dh_last_error().decode() if o.rc != 0 else ""
    torch.cuda.synchronize()
    return o


def _cells_same(a, b, what):
    c = a.counts.tolist()
    assert c == b.counts.tolist(), what
    assert torch.equal(a.masks, b.masks) and torch.equal(a.pairs[:c[0]], b.pairs[:c[0]]), what
    for k in range(3):
        assert torch.equal(a.lists[k, :c[1 + k]], b.lists[k, :c[1 + k]]), what


@pytest.mark.parametrize("er", [0, 5])
@pytest.mark.parametrize("which", ["overlap", "disjoint"])
@pytest.mark.parametrize("res", [128, 256])
def test_cells_with_donor_rows_against_the_reference(res, which, er):
    fx = I.fixture(res, which)
    corr, flags = fx["geo"][0][1].numpy(), fx["geo"][0][2]["row_donor"]
    o = _cells_call(corr, res, er, flags)
    assert o.rc == 0, o.err
    ref = fx[f"cells{er}"]
    c = o.counts.tolist()
    assert c[0] == len(ref["original_x"])
    pairs = o.pairs[:c[0]].cpu().numpy()
    assert np.array_equal(pairs[:, 0], ref["original_y"] * GRID + ref["original_x"])
    assert np.array_equal(pairs[:, 1], ref["transformed_y"] * GRID + ref["transformed_x"])
    assert np.array_equal(o.masks.cpu().numpy().reshape(3, GRID, GRID), ref["masks"])
    for k, key in enumerate(("", "_orig", "_trans")):
        want = ref[f"background_y{key}"] * GRID + ref[f"background_x{key}"]
        assert c[1 + k] == len(want) and np.array_equal(o.lists[k, :c[1 + k]].cpu().numpy(), want)
    # the donor's source cells stay original background: the masks differ from the unflagged call's
    plain = _cells_call(corr, res, er)
    assert int((o.masks[1] != plain.masks[1]).sum()) >= 1 and torch.equal(o.masks[2], plain.masks[2])
    # the host layer
    from diffusionhandles_amd.losses import process_correspondences
    pc = process_correspondences(corr, res, er, grid=GRID, device=dev(), row_donor=flags, pair_instances=fx["geo"][0][2]["corr_inst"])
    for key in I.RM.CELL_KEYS:
        assert np.array_equal(pc[key], ref[key]), key


@pytest.mark.parametrize("er", [0, 5])
def test_cells_null_and_all_zero_flags_are_the_vacated_entry(er):
    fx = I.fixture(128, "overlap")
    corr = fx["geo"][0][1].numpy()
    vac = np.zeros((128, 128), dtype=np.uint8)
    vac[10:30, 90:120] = 1
    for v in (None, vac):
        base = _cells_call(corr, 128, er, entry="vacated", vacated=v)
        assert base.rc == 0, base.err
        _cells_same(_cells_call(corr, 128, er, "none", vacated=v), base, "NULL flags")
        _cells_same(_cells_call(corr, 128, er, np.zeros(len(corr), dtype=np.uint8), vacated=v), base, "all-zero flags")


def test_cells_refusals_leave_the_outputs_untouched():
    fx = I.fixture(128, "overlap")
    corr, flags = fx["geo"][0][1].numpy(), fx["geo"][0][2]["row_donor"]
    o = _cells_call(corr, 100, 0, flags)          # 100 is no multiple of the grid
    assert o.rc == DH_ERR_ARG and o.err
    assert bool((o.pairs == -1).all()) and bool((o.lists == -1).all()) and bool((o.masks == 0xFF).all()) and bool((o.counts == -1).all())


# ---- 3. energy --------------------------------------------------------------------------------------------------------------------
def _energy_setup(res=128, which="overlap"):
    """The first edit's cells with objects = instances (0, 1 host; 2 donor), plus a hand-made pair set in which one target cell
    receives a host pair and a donor pair with the SAME source cell id."""
    from diffusionhandles_amd.losses import process_correspondences
    fx = I.fixture(res, which)
    corr, dbg = fx["geo"][0][1].numpy(), fx["geo"][0][2]
    pc = process_correspondences(corr, res, 0, grid=GRID, device=dev(), row_donor=dbg["row_donor"], pair_instances=dbg["corr_inst"])
    ok = I.kept_rows(corr, res)
    objects = dbg["corr_inst"].astype(np.int64)[ok]
    assert np.array_equal(pc["object"], objects) and set(objects.tolist()) == {0, 1, 2}
    return fx, pc, fx["cells0"], objects


def _same_cell_setup(res=128):
    """Rows of a host object (0) and a donor object (1) that share source pixels AND target pixels: every target cell receives
    a host and a donor pair with one source cell id."""
    from diffusionhandles_amd.losses import process_correspondences
    ys, xs = np.meshgrid(np.arange(20, 44), np.arange(30, 50), indexing="ij")
    one = np.stack([xs.ravel(), ys.ravel(), xs.ravel() + 40, ys.ravel() + 30], axis=-1).astype(np.int64)
    corr = np.concatenate([one, one])
    inst = np.repeat(np.array([0, 1], dtype=np.uint8), len(one))
    pc = process_correspondences(corr, res, 0, grid=GRID, device=dev(), row_donor=inst, pair_instances=inst)
    cells = I.cells(corr, res, inst, None, 0)
    return pc, cells, inst.astype(np.int64)


def _maps(C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(GRID, GRID, C, generator=g).to(dtype).to(dev()) for _ in range(3))


def _donor_energy(act, orig, donor, plan, bits, fw, bw):
    from diffusionhandles_amd.losses import energy_and_grad_planned_donor
    out = torch.full(act.shape, float("nan"), dtype=torch.float32, device=dev())
    loss, grad = energy_and_grad_planned_donor(act, orig, plan, fw, bw, donor, bits, grad_scale=SCALE, want_loss=True, out=out,
                                               grad_dtype=torch.float32)
    torch.cuda.synchronize()
    assert torch.isfinite(grad).all() and torch.isfinite(loss).all()
    return loss, grad


def _check_energy(loss, grad, ref_loss, ref_grad, what):
    """loss 2e-5 relative, gradient 1e-4 of its largest entry."""
    got = [float(v) for v in loss.cpu()]
    ref = ref_grad.double() * SCALE
    err, top = float((grad.double().cpu() - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: loss {got} / {list(ref_loss)}; gradient max abs err {err:.3e} (bound {1e-4 * top:.3e})")
    for g, r in zip(got, ref_loss):
        assert abs(g - r) <= 2e-5 * abs(r) + 1e-12, (what, got, ref_loss)
    assert err <= 1e-4 * top, what


@pytest.mark.parametrize("C", C_ENERGY)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_donor_energy_against_the_reference(dtype, C):
    from diffusionhandles_amd.losses import EnergyPlan
    _, pc, cells, objects = _energy_setup()
    act, orig, donor = _maps(C, dtype, 500 + C)
    for ow in (None, "equal", [0.5, 2.0, 1.25]):
        plan = EnergyPlan(pc, GRID, dev(), object_weights=ow, force_weighted=True)
        assert plan.weighted and plan.n_objects == 3
        w = None if ow is None else ([1.0] * 3 if ow == "equal" else ow)
        for fw, bw in ((7.5, 1.5), (7.5, 0.0)):
            ref_loss, ref_grad = I.energy_and_grad(act, orig, donor, cells, objects, {2}, w, fw, bw, (GRID, GRID))
            loss, grad = _donor_energy(act, orig, donor, plan, 0b100, fw, bw)
            _check_energy(loss, grad, ref_loss, ref_grad, f"{dtype} C {C} weights {ow} ({fw}, {bw})")
    # one target cell with a host and a donor pair of one source cell id
    pc2, cells2, objects2 = _same_cell_setup()
    plan = EnergyPlan(pc2, GRID, dev(), object_weights="equal", force_weighted=True)
    ref_loss, ref_grad = I.energy_and_grad(act, orig, donor, cells2, objects2, {1}, [1.0, 1.0], 7.5, 1.5, (GRID, GRID))
    loss, grad = _donor_energy(act, orig, donor, plan, 0b10, 7.5, 1.5)
    _check_energy(loss, grad, ref_loss, ref_grad, f"{dtype} C {C} shared source cell")
    plain_loss, plain_grad = _donor_energy(act, orig, donor, plan, 0, 7.5, 1.5)
    assert not torch.equal(plain_grad, grad)


@pytest.mark.parametrize("C", C_ENERGY)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_donor_energy_bit_identities(dtype, C):
    """donor_objects = 0 and donor == orig are dh_energy_fwd_bwd_planned_objects; batch item e is the single call."""
    from diffusionhandles_amd.losses import (EnergyPlan, energy_and_grad_planned, energy_and_grad_planned_donor_batch)
    _, pc, _, _ = _energy_setup()
    pc2, _, _ = _same_cell_setup()
    act, orig, donor = _maps(C, dtype, 600 + C)
    act2, orig2, donor2 = _maps(C, dtype, 700 + C)
    plan = EnergyPlan(pc, GRID, dev(), object_weights=[0.5, 2.0, 1.25])
    plan2 = EnergyPlan(pc2, GRID, dev(), object_weights="equal")
    out = torch.full(act.shape, float("nan"), dtype=torch.float32, device=dev())
    base_loss, base = energy_and_grad_planned(act, orig, plan, 7.5, 1.5, grad_scale=SCALE, want_loss=True, out=out, grad_dtype=torch.float32)
    base = base.clone()
    for bits, dn in ((0, donor), (0, None), (0b100, orig), (0b111, orig)):
        loss, grad = _donor_energy(act, orig, dn, plan, bits, 7.5, 1.5)
        assert torch.equal(grad, base) and torch.equal(loss, base_loss), (bits, dn is None)
    singles = [_donor_energy(act, orig, donor, plan, 0b100, 7.5, 1.5), _donor_energy(act2, orig2, donor2, plan2, 0b10, 5.0, 1.0),
               _donor_energy(act2, orig, None, plan, 0, 7.5, 0.0)]
    singles = [(l.clone(), g.clone()) for l, g in singles]
    outs = [torch.full(act.shape, float("nan"), dtype=torch.float32, device=dev()) for _ in range(3)]
    loss, grads = energy_and_grad_planned_donor_batch([act, act2, act2], [orig, orig2, orig], [plan, plan2, plan], [7.5, 5.0, 7.5],
                                                      [1.5, 1.0, 0.0], [SCALE] * 3, [donor, donor2, None], [0b100, 0b10, 0],
                                                      want_loss=True, outs=outs, grad_dtype=torch.float32)
    torch.cuda.synchronize()
    for e, (l, g) in enumerate(singles):
        assert torch.equal(grads[e], g) and torch.equal(loss[e], l), f"batch item {e}"


def test_energy_refusals_leave_the_gradient_untouched():
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd.losses import EnergyPlan, energy_and_grad_planned_donor
    _, pc, _, _ = _energy_setup()
    act, orig, donor = _maps(64, torch.float16, 800)
    plan = EnergyPlan(pc, GRID, dev(), object_weights="equal")
    with pytest.raises(ValueError, match="at or above the plan's 3"):
        energy_and_grad_planned_donor(act, orig, plan, 7.5, 1.5, donor, 0b1000)
    L = _lib.lib()
    ws, wsb = plan.workspace(64)
    dl = plan.dl
    for bits, dn in ((1 << 8, donor), (0b100, None)):
        grad = torch.full(act.shape, float("nan"), dtype=torch.float32, device=dev())
        rc = L.dh_energy_fwd_bwd_planned_donor(
            _lib.ptr(act), _lib.ptr(orig), 0, 64, GRID, _lib.ptr(plan.buf), plan.nbytes, plan.n_pairs, _lib.ptr(dl["bg_orig"]),
            dl["bg_orig"].numel(), _lib.ptr(dl["bg_trans"]), dl["bg_trans"].numel(), 7.5, 1.5, SCALE, None, _lib.ptr(grad), 2,
            _lib.ptr(ws), wsb, _lib.stream_ptr(), _lib.ptr(dn), bits)
        torch.cuda.synchronize()
        assert rc == DH_ERR_ARG and L.dh_last_error() and torch.isnan(grad).all()


# ---- 4. the loop level, on the TINY rig of tests/test_object_removal_gpu.py ---------------------------------------------------------
RES = 512


def _corner_donor(res=RES):
    """A donor scene whose one sphere lies in the top-left corner, far from both host spheres: depth [1,1,res,res], [mask]."""
    s = res / 512.0
    yy, xx = np.meshgrid(np.arange(res, dtype=np.float64), np.arange(res, dtype=np.float64), indexing="ij")
    r2 = ((yy - 60.0 * s) ** 2 + (xx - 60.0 * s) ** 2) / ((30.0 * s) ** 2)
    m = r2 < 1.0
    depth = np.where(m, 2.2 - 0.4 * np.sqrt(np.clip(1.0 - r2, 0.0, None)), 5.0 + 1.0 * xx / res)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.float32))[None, None].contiguous()
    return t(depth), [t(m)]


# host sphere 0 stays, host sphere 1 turns in place, the donor sphere is enlarged and set down at the lower right
LOOP_TFS = [(0.0, R.Y, (0.0, 0.0, 0.0)), (-30.0, R.Y, (0.0, 0.0, 0.0)), (20.0, R.Y, (-1.5, -1.5, 0.0), 1.3, None)]
SECOND_TFS = [(10.0, R.Y, (0.1, 0.0, 0.0)), (20.0, R.Y, (0.0, 0.0, 0.1)), (-15.0, R.Y, (-1.2, -1.6, 0.2), 0.9, None)]


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
    ddepth, dmasks = _corner_donor()
    ddepth, dmasks = ddepth.to(dev()), [m.to(dev()) for m in dmasks]
    donor = dict(depth=ddepth, masks=dmasks, activations=identity(ddepth, "a ball in a corner", 12)["acts"])
    return SimpleNamespace(dh=dh, gd=dh.diffuser, two=two, donor=donor)


def _common(im):
    return dict(depth=im.depth, prompt=im.prompt, bg_depth=im.bg_depth, null_text_emb=im.null_text, init_noise=im.noise,
                activations=im.acts)


def _loop_geometry(tiny, edits, device_correspondences=False):
    from diffusionhandles_amd import depth_transform as DT
    t, dn = tiny.two, tiny.donor
    return DT.reproject_donor_edits(t.depth, t.bg_depth, t.masks, tiny.gd.get_depth_intrinsics(device=dev()),
                                    [[_t(tf) for tf in tfs] for tfs in edits], [0, 1, 2], donor_depth=dn["depth"],
                                    donor_masks=dn["masks"], device_correspondences=device_correspondences)


def test_transform_foreground_objects_with_a_donor(tiny):
    """The edit is guided_inference on the re-projection's rows, instance array and donor tuple; two runs are byte-identical;
    the donor's activations reach the energy (the first recorded gradient differs from the run that is handed the host's)."""
    dh, gd, t, dn = tiny.dh, tiny.gd, tiny.two, tiny.donor
    tfs = [_t(tf) for tf in LOOP_TFS]
    img, disp = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=tfs, donor=dn)
    img, lat = img.clone(), gd.last_latents.clone()
    assert img.shape == (1, 3, RES, RES) and torch.isfinite(img).all()
    (d, c, rows), = _loop_geometry(tiny, [LOOP_TFS])
    flags = (rows >= 2).to(torch.uint8)
    assert torch.equal(d, disp) and int(flags.sum()) >= 100 and int((rows == 0).sum()) >= 100
    rec = {}
    ref = gd.guided_inference(t.noise, d, t.null_text, t.prompt, t.acts, c, pair_instances=rows, donor=(dn["activations"], flags),
                              record=rec)
    assert torch.equal(gd.last_latents, lat) and torch.equal(ref, img)
    again, _ = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=tfs, donor=dn)
    assert torch.equal(again, img) and torch.equal(gd.last_latents, lat)
    rec_host = {}
    other = gd.guided_inference(t.noise, d, t.null_text, t.prompt, t.acts, c, pair_instances=rows, donor=(t.acts, flags),
                                record=rec_host)
    assert torch.isfinite(other).all() and torch.isfinite(rec["grad"][0]).all()
    assert not torch.equal(rec["grad"][0], rec_host["grad"][0]) and not torch.equal(gd.last_latents, lat)
    # a donor whose masks are all empty is the call without the keyword
    plain, pdisp = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=tfs[:2])
    plain, plat = plain.clone(), gd.last_latents.clone()
    empty = dict(dn, masks=[torch.zeros_like(dn["masks"][0])])
    same, sdisp = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=tfs[:2], donor=empty)
    assert torch.equal(same, plain) and torch.equal(sdisp, pdisp) and torch.equal(gd.last_latents, plat)
    # the automatic gradient scale takes its bound from the weighted plan
    old = gd.grad_scale_mode
    gd.grad_scale_mode = "auto"
    try:
        auto, _ = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=tfs, donor=dn, object_weights="equal")
        assert torch.isfinite(auto).all()
    finally:
        gd.grad_scale_mode = old


def test_donor_edits_in_a_batch_and_the_pure_insertion(tiny):
    """K = 2 edits with one donor are guided_inference_batch on the re-projections with the per-edit row flags; the pure insertion
    (no host mask) runs."""
    dh, gd, t, dn = tiny.dh, tiny.gd, tiny.two, tiny.donor
    edits = [[_t(tf) for tf in LOOP_TFS], [_t(tf) for tf in SECOND_TFS]]
    imgs, disps = dh.transform_foreground_objects_batch(**_common(t), fg_masks=t.masks, edits=edits, donor=dn)
    imgs, lat = imgs.clone(), gd.last_latents.clone()
    assert imgs.shape == (2, 3, RES, RES) and torch.isfinite(imgs).all()
    rp = _loop_geometry(tiny, [LOOP_TFS, SECOND_TFS], device_correspondences=True)
    assert all(torch.equal(a, b[0]) for a, b in zip(disps, rp))
    flags = [(r[2] >= 2).to(torch.uint8) for r in rp]
    ref = gd.guided_inference_batch(t.noise, [r[0] for r in rp], t.null_text, t.prompt, t.acts, [r[1] for r in rp],
                                    pair_instances=[r[2] for r in rp], donor=(dn["activations"], flags))
    assert torch.equal(ref, imgs) and torch.equal(gd.last_latents, lat)
    # single edits on two lanes share the donor's channels-last copy: bit-identical to one stream at the same batch
    args = dict(_common(t), fg_masks=t.masks, edits=edits, donor=dn)
    one_stream, _ = dh.transform_foreground_objects_batch(**args, streams=1, batch=1)
    one_stream = one_stream.clone()
    two_lanes, _ = dh.transform_foreground_objects_batch(**args, streams=2, batch=1)
    assert torch.isfinite(two_lanes).all() and torch.equal(two_lanes, one_stream)
    pure, pdisp = dh.transform_foreground_objects(depth=t.depth, prompt=t.prompt, bg_depth=t.depth, null_text_emb=t.null_text,
                                                  init_noise=t.noise, activations=t.acts, fg_masks=[], transforms=edits[0][2:],
                                                  donor=dn)
    assert torch.isfinite(pure).all() and not torch.equal(pdisp, disps[0])


def test_background_lock_leaves_the_donor_source_cells_locked(tiny):
    """The keep map is 1 on the cells under the donor's source pixels: they are pixels of another image, far from every target
    and every host mask, so the lock holds the host there; the target cells of the donor rows are free."""
    dh, gd, t, dn = tiny.dh, tiny.gd, tiny.two, tiny.donor
    s = gd.unet.sample_size
    cs = RES // s
    dh.conf["background_lock"] = True
    try:
        img, _ = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=[_t(tf) for tf in LOOP_TFS], donor=dn)
        keep, = dh.last_keep_maps
    finally:
        dh.conf.pop("background_lock", None)
    assert torch.isfinite(img).all()
    keep = keep.float().reshape(s, s)
    (d, c, rows), = _loop_geometry(tiny, [LOOP_TFS])
    donor_rows = c[rows >= 2]
    src = torch.zeros((s, s), dtype=torch.bool)
    src[donor_rows[:, 1] // cs, donor_rows[:, 0] // cs] = True
    tgt = torch.zeros((s, s), dtype=torch.bool)
    tgt[c[:, 3] // cs, c[:, 2] // cs] = True
    for m in t.masks:
        tgt |= (m[0, 0] != 0).reshape(s, cs, s, cs).any(dim=3).any(dim=1).cpu()
    # far: no target cell and no host-mask cell within 6 cells of a donor source cell (dilate 2 + feather 2 + 1)
    near = torch.nn.functional.max_pool2d(tgt[None, None].float(), 13, 1, 6)[0, 0] > 0
    assert int(src.sum()) >= 20 and not bool((near & src).any())
    assert float(keep[src.to(keep.device)].min()) == 1.0
    dtg = torch.zeros((s, s), dtype=torch.bool)
    dtg[donor_rows[:, 3] // cs, donor_rows[:, 2] // cs] = True
    assert float(keep[dtg.to(keep.device)].max()) == 0.0


def _run_edit_module():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_edit_tool", os.path.join(root, "tools", "run_edit.py"))
    run_edit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run_edit)
    return run_edit


def test_run_edit_passes_the_donor_of_a_scene_directory(tiny, tmp_path):
    """A two-mask scene with donor/ and the entries `plain` and `insert`: run_scene computes both identities (--identity-batch 2:
    in one pass), hands the donor to transform_foreground_objects for `insert` alone, and caches the donor identity."""
    import argparse
    import json
    from diffusionhandles_amd.scene_io import read_png, write_png
    run_edit = _run_edit_module()
    scene = tmp_path / "set" / "two_spheres"
    (scene / "donor").mkdir(parents=True)
    depth, bg, masks = R.two_spheres(RES)
    ddepth, dmasks = _corner_donor()
    np.save(scene / "depth.npy", depth[0, 0].numpy())
    np.save(scene / "bg_depth.npy", bg[0, 0].numpy())
    np.save(scene / "donor" / "depth.npy", ddepth[0, 0].numpy())
    for m, mask in enumerate(masks):
        write_png(str(scene / f"mask_{m}.png"), mask[0, 0].numpy())
    write_png(str(scene / "donor" / "mask_0.png"), dmasks[0][0, 0].numpy())
    for sub, prompt in (("", "two spheres on a plane\n"), ("donor", "a ball in a corner\n")):
        write_png(str(scene / sub / "input.png"), np.full((RES, RES, 3), 0.5, dtype=np.float32))
        (scene / sub / "prompt.txt").write_text(prompt)
    member = lambda tf, **kw: dict(rotation_angle=tf[0], rotation_axis=list(tf[1]), translation=list(tf[2]), **kw)
    (scene / "transforms.json").write_text(json.dumps({
        "plain": {"objects": [{}, member(LOOP_TFS[1])]},
        "insert": {"objects": [{}, member(LOOP_TFS[1]), member(LOOP_TFS[2], donor=0, scale=LOOP_TFS[2][3])]}}))
    args = argparse.Namespace(res=RES, mode="pc", skip_inversion=True, no_identity_cache=False, identity_cache=None, skip_existing=False,
                              max_edits=0, identity_batch=2, edit_batch=1, edit_batch_images=0, background_lock=False)
    seen = []
    dh = tiny.dh
    inner = dh.transform_foreground_objects
    dh.transform_foreground_objects = lambda *a, **kw: (seen.append((len(a[2]), kw.get("donor"), kw.get("instances"))), inner(*a, **kw))[1]
    try:
        out = tmp_path / "one"
        report = run_edit.run_scene(args, dh.conf, lambda res: dh, str(scene), str(out), None)
        assert [e["name"] for e in report["edits"]] == ["plain", "insert"]
        assert seen[0] == (2, None, None) and seen[1][0] == 2 and seen[1][2] == [0, 1, 2]
        donor = seen[1][1]
        assert len(donor["masks"]) == 1 and len(donor["activations"]) == 3 and tuple(donor["depth"].shape) == (1, 1, RES, RES)
        assert os.path.exists(out / "donor_identity.npz") and os.path.exists(out / "identity.npz")
        # a second run reads both caches and writes the same disparity
        del seen[:]
        first = read_png(str(out / "insert_disparity.png"))
        args.identity_batch = 1
        run_edit.run_scene(args, dh.conf, lambda res: dh, str(scene), str(out), None)
        assert seen[1][1] is not None and np.array_equal(read_png(str(out / "insert_disparity.png")), first)
    finally:
        del dh.transform_foreground_objects
    plain, insert = (read_png(str(out / f"{n}_disparity.png")).astype(np.float64) for n in ("plain", "insert"))
    assert read_png(str(out / "insert.png")).std() > 0 and (plain != insert).mean() > 0.01
