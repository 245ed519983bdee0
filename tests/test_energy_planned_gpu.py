"""The planned guidance-energy entries (dh_energy_fwd_bwd_planned, _objects, _donor and their four batch entries: the plan
builds with k_dedupe_sources[_obj], then k_colsum_q[_batch] and k_energy_grad[_obj | _donor][_batch | _mixed_batch]) against the
float64 reference of tests/energy_planned_ref.py, element by element, on the cases of its table: C from 8 to 2048 with idle
lanes and a ragged last block, target cells with 0 to 41 distinct sources and multiplicities up to 300, background lists whose
slices take each loop of k_colsum_q, up to eight objects with folds at every step of the 8-wide loop, donor bits, and batches
of 2 and 16 items of different plans.

The maps are 16-bit values at the grid and the patch is 1, so every pair sign is exact and a gradient element is an integer
sign sum times a coefficient; the inputs make the one remaining sign, that of a channel's background mean difference, certain
(tests/test_energy_planned_ref.py holds |mean difference| >= 2^-10 for every item).  NO element is left out.  Gates, per
element, derived and not measured:
  gradient  |got - scale ref| <= ulp_TG(scale ref) + 2^-20 scale mag
            ulp_TG: one unit in the last place of a 16-bit gradient type (the rounding to nearest, and a value pushed across a
            rounding boundary by the second term); 0 for f32.  mag: the sum of the magnitudes of the element's terms; fewer
            than sixteen f32 roundings of 2^-24 (fg_norm, omega / (C N), the products, one add per object, the scale) act on
            them, and that is what remains where the terms cancel.  Where mag is 0 an f32 element is exactly 0.
  fg loss   relative 2^-20 (one f32 rounding per |d|, a double accumulation, fg_norm, the final cast)
  bg, total |d| <= 2e-5 max(1, |ref|), the gate of the general path
Gradient, loss and workspace are NaN-filled before every call; nothing may be non-finite afterwards.  DH_CLOSE_RATIOS=<file>
logs the worst error / gate ratio of every comparison."""
import ctypes
import os

import pytest
import torch

import energy_planned_ref as R
from test_engine_kernels_gpu import ulp16, within
from test_unet_kernels_gpu import dev

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _plan(it):
    from diffusionhandles_amd.losses import EnergyPlan
    kw = dict(object_weights=list(it.weights), force_weighted=it.M == 1) if it.M else {}
    plan = EnergyPlan(dict(it.cells()), it.grid, dev(), **kw)
    assert plan.weighted == bool(it.M) and plan.n_pairs == it.cells()["original_x"].size
    return plan


def _log(site, what, ratio):
    log = os.environ.get("DH_CLOSE_RATIOS")
    if log:
        with open(log, "a") as f:
            f.write(f"test_energy_planned_gpu.py:{site}\t{what}\t{ratio:.4g}\n")


def held(it, grad, loss, what):
    """The gates of the module's docstring on one item's outputs."""
    ref = it.ref()
    got, lv = grad.cpu().double(), loss.cpu().double()
    assert tuple(got.shape) == (it.grid, it.grid, it.C) and grad.dtype == it.grad_dtype
    nonfin = ~torch.isfinite(got)
    assert not bool(nonfin.any()) and bool(torch.isfinite(lv).all()), (
        f"{what}: {int(nonfin.sum())} gradient elements are not finite, the first at "
        f"{tuple(int(i) for i in nonfin.nonzero()[0]) if nonfin.any() else None}; loss {lv.tolist()}")
    want = ref["grad"] * it.scale
    tol = 2.0 ** -20 * it.scale * ref["mag"]
    if it.grad_dtype != torch.float32:
        tol = tol + ulp16(want, it.grad_dtype)
    err = (got - want).abs()
    ratio = torch.where(tol > 0, err / tol.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    _log(f"grad/{it.kind}", f"{it.types} {what}", float(ratio.max()))
    bad = ratio > 1.0
    if bool(bad.any()):
        y, x, c = (int(i) for i in bad.nonzero()[0])
        cells = bad.any(-1).view(-1).nonzero().view(-1)
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} gradient elements over the gate in {cells.numel()} cells; the first at "
            f"(y {y}, x {x}, c {c}), cell {y * it.grid + x} with {int(ref['seg'][y * it.grid + x])} distinct entries: got "
            f"{float(got[y, x, c]):.9g}, reference {float(want[y, x, c]):.9g}, gate {float(tol[y, x, c]):.3g}; segment lengths of "
            f"the bad cells {sorted(set(int(ref['seg'][int(q)]) for q in cells))[:12]}")
    within(got, want, torch.where(tol > 0, tol, torch.ones_like(tol)), f"{what} grad")
    rl = ref["loss"]
    gates = (2e-5 * max(1.0, abs(float(rl[0]))), 2.0 ** -20 * abs(float(rl[1])), 2e-5 * max(1.0, abs(float(rl[2]))))
    for k, name in enumerate(("total", "fg", "bg")):
        d = abs(float(lv[k]) - float(rl[k]))
        _log(f"loss_{name}/{it.kind}", f"{it.types} {what}", d / gates[k] if gates[k] > 0 else (0.0 if d == 0 else float("inf")))
        assert d <= gates[k], f"{what}: {name} loss {float(lv[k]):.9g}, reference {float(rl[k]):.9g}, gate {gates[k]:.3g}"


def _device_inputs(it):
    cur, org, donor = it.inputs()
    return cur.to(dev()), org.to(dev()), donor.to(dev())


@pytest.mark.parametrize("it", R.SINGLES, ids=lambda c: c.id)
def test_single_entries_vs_float64(it):
    from diffusionhandles_amd import _lib
    L = _lib.lib()
    plan = _plan(it)
    cur, org, donor = _device_inputs(it)
    g, C, dl = it.grid, it.C, plan.dl
    grad = torch.full((g, g, C), NAN, dtype=it.grad_dtype, device=dev())
    loss = torch.full((3,), NAN, device=dev())
    ws, wsb = plan.workspace(C)
    ws.fill_(0xFF)
    head = (_lib.ptr(cur), _lib.ptr(org), _lib.DTYPE_CODE[cur.dtype], C, g, _lib.ptr(plan.buf), plan.nbytes, plan.n_pairs,
            _lib.ptr(dl["bg_orig"]), dl["bg_orig"].numel(), _lib.ptr(dl["bg_trans"]), dl["bg_trans"].numel(), it.fg_w, it.bg_w,
            it.scale, _lib.ptr(loss), _lib.ptr(grad), _lib.DTYPE_CODE[it.grad_dtype], _lib.ptr(ws), wsb, _lib.stream_ptr())
    if it.kind == "donor":
        _lib.check(L.dh_energy_fwd_bwd_planned_donor(*head, _lib.ptr(donor), it.donor_bits), "dh_energy_fwd_bwd_planned_donor")
    elif it.kind == "objects":
        _lib.check(L.dh_energy_fwd_bwd_planned_objects(*head), "dh_energy_fwd_bwd_planned_objects")
    else:
        _lib.check(L.dh_energy_fwd_bwd_planned(*head), "dh_energy_fwd_bwd_planned")
    torch.cuda.synchronize()
    held(it, grad, loss, it.id)


@pytest.mark.parametrize("b", R.BATCHES, ids=lambda b: b.id)
def test_batch_entries_vs_float64(b):
    """Every item of a batch against the reference itself, not against its single call."""
    from diffusionhandles_amd import _lib
    L = _lib.lib()
    K, g, C = b.K, b.grid, b.C
    plans = [_plan(it) for it in b.items]
    maps = [_device_inputs(it) for it in b.items]
    grads = torch.full((K, g, g, C), NAN, dtype=b.grad_dtype, device=dev())
    losses = torch.full((K, 3), NAN, device=dev())
    nb = ctypes.c_size_t()
    _lib.check(L.dh_energy_planned_batch_workspace_bytes(C, g, K, ctypes.byref(nb)), "dh_energy_planned_batch_workspace_bytes")
    ws = torch.full((nb.value,), 0xFF, dtype=torch.uint8, device=dev())
    items = (_lib.EnergyItem * K)()
    for e, (row, it, p) in enumerate(zip(items, b.items, plans)):
        row.cur, row.orig, row.plan, row.plan_bytes = maps[e][0].data_ptr(), maps[e][1].data_ptr(), p.buf.data_ptr(), p.nbytes
        row.bg_orig, row.bg_trans = p.dl["bg_orig"].data_ptr(), p.dl["bg_trans"].data_ptr()
        row.loss_out, row.grad = losses[e].data_ptr(), grads[e].data_ptr()
        row.n_pairs, row.n_bg_orig, row.n_bg_trans = p.n_pairs, p.dl["bg_orig"].numel(), p.dl["bg_trans"].numel()
        row.fg_w, row.bg_w, row.grad_scale = it.fg_w, it.bg_w, it.scale
    tail = (K, _lib.DTYPE_CODE[b.in_dtype], C, g, _lib.DTYPE_CODE[b.grad_dtype], _lib.ptr(ws), nb.value, _lib.stream_ptr())
    if b.entry == "plain":
        _lib.check(L.dh_energy_fwd_bwd_planned_batch(items, *tail), "dh_energy_fwd_bwd_planned_batch")
    elif b.entry == "objects":
        _lib.check(L.dh_energy_fwd_bwd_planned_objects_batch(items, *tail), "dh_energy_fwd_bwd_planned_objects_batch")
    elif b.entry == "mixed":
        flags = (ctypes.c_uint8 * K)(*[1 if p.weighted else 0 for p in plans])
        _lib.check(L.dh_energy_fwd_bwd_planned_mixed_batch(items, flags, *tail), "dh_energy_fwd_bwd_planned_mixed_batch")
    else:
        rows = (_lib.EnergyDonorItem * K)()
        for e, it in enumerate(b.items):
            rows[e].item, rows[e].donor, rows[e].donor_objects = items[e], maps[e][2].data_ptr(), it.donor_bits
        _lib.check(L.dh_energy_fwd_bwd_planned_donor_batch(rows, *tail), "dh_energy_fwd_bwd_planned_donor_batch")
    torch.cuda.synchronize()
    for e, it in enumerate(b.items):
        held(it, grads[e], losses[e], f"{b.id} item {e} ({it.id})")
