"""GPU: weighted and unweighted guidance-energy items in ONE launch pair (dh_energy_fwd_bwd_planned_mixed_batch,
losses.energy_and_grad_planned_mixed) against the single call of each item's kind, bit for bit, on the two-sphere scene of
tests/object_weights_ref.py (256 pixels, grid 32).  Every output is NaN before the call."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_object_ref as R  # noqa: E402
import object_weights_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu
GRID = W.GRID


def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


_PC, _PLANS = {}, {}


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


def _plans():
    """16 plans, weighted (even places) and unweighted (odd places) interleaved, built once:
      0 occluding 'equal' (both objects have pairs, 4155 / 795: the fold between objects runs)   1 occluding, no weights
      2 apart, weights (2, 0.5)                                                                  3 apart, no weights
      4 weighted, object 1 has no pairs                                                          5 one object (a plain plan)
      6 weighted, no pairs at all                                                                7 plain, no pairs at all
    and the same kinds again under other weights."""
    if _PLANS:
        return _PLANS["all"]
    from diffusionhandles_amd.losses import EnergyPlan
    mk = lambda n, keep=None, w=None, masks=(0, 1): EnergyPlan(_pc(n, keep, masks), GRID, dev(), object_weights=w)
    one = lambda: mk("occluding", (0,), "equal", masks=(0,))
    plans = [mk("occluding", w="equal"), mk("occluding"), mk("apart", w=[2.0, 0.5]), mk("apart"),
             mk("occluding", (0,), [1.0, 3.0]), one(), mk("occluding", (), [1.0, 1.0]), mk("occluding", ()),
             mk("apart", w="equal"), mk("apart"), mk("occluding", w=[0.25, 2.0]), mk("occluding"),
             mk("apart", w=[1.0, 0.0]), one(), mk("occluding", w=[3.0, 1.0]), mk("apart", (1,))]
    assert [p.weighted for p in plans] == [e % 2 == 0 for e in range(16)]
    assert plans[0].counts.tolist() == [4155, 795] and plans[2].counts.min() > 0            # both objects have pairs
    assert plans[4].counts.tolist() == [4155, 0] and plans[4].omega.tolist() == [1.0, 0.0]
    assert plans[5].n_pairs == 4155 and plans[6].n_pairs == 0 and plans[7].n_pairs == 0
    _PLANS["all"] = plans
    return plans


def _items(plans, cur, orig, grads, losses, fw, bw, scale):
    from diffusionhandles_amd import _lib
    K = len(plans)
    items = (_lib.EnergyItem * K)()
    for e, it in enumerate(items):
        p = plans[e]
        it.cur, it.orig, it.plan, it.plan_bytes = cur[e].data_ptr(), orig[e].data_ptr(), p.buf.data_ptr(), p.nbytes
        it.bg_orig, it.bg_trans = p.dl["bg_orig"].data_ptr(), p.dl["bg_trans"].data_ptr()
        it.loss_out, it.grad = (losses[e].data_ptr() if losses is not None else None), grads[e].data_ptr()
        it.n_pairs, it.n_bg_orig, it.n_bg_trans = p.n_pairs, p.dl["bg_orig"].numel(), p.dl["bg_trans"].numel()
        it.fg_w, it.bg_w, it.grad_scale = fw[e], bw[e], scale[e]
    return items


def _flags(plans, flags=None):
    f = [1 if p.weighted else 0 for p in plans] if flags is None else flags
    return (ctypes.c_uint8 * len(f))(*f)


def _workspace(C, K):
    from diffusionhandles_amd import _lib
    nb = ctypes.c_size_t()
    _lib.check(_lib.lib().dh_energy_planned_batch_workspace_bytes(C, GRID, K, ctypes.byref(nb)), "workspace bytes")
    return torch.empty(nb.value, dtype=torch.uint8, device=dev()), nb.value


def _single(act, orig, plan, fw, bw, scale, grad, loss):
    """The single call of the plan's kind through the C ABI; loss: a [3] tensor or None."""
    from diffusionhandles_amd import _lib
    L = _lib.lib()
    C = act.shape[-1]
    ws, wsb = plan.workspace(C)
    entry = L.dh_energy_fwd_bwd_planned_objects if plan.weighted else L.dh_energy_fwd_bwd_planned
    dl = plan.dl
    _lib.check(entry(_lib.ptr(act), _lib.ptr(orig), _lib.DTYPE_CODE[act.dtype], C, GRID, _lib.ptr(plan.buf), plan.nbytes, plan.n_pairs,
                     _lib.ptr(dl["bg_orig"]), dl["bg_orig"].numel(), _lib.ptr(dl["bg_trans"]), dl["bg_trans"].numel(), fw, bw, scale,
                     _lib.ptr(loss), _lib.ptr(grad), _lib.DTYPE_CODE[grad.dtype], _lib.ptr(ws), wsb, _lib.stream_ptr()), "single call")


@pytest.mark.parametrize("dtype,grad_dtype", [(torch.float16, torch.float16), (torch.bfloat16, torch.float32),
                                              (torch.float16, torch.bfloat16), (torch.bfloat16, torch.bfloat16)])
@pytest.mark.parametrize("C", [64, 320])
def test_mixed_batch_is_bit_identical_to_the_single_call_of_each_kind(C, dtype, grad_dtype):
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd.losses import energy_and_grad_planned_batch, energy_and_grad_planned_mixed
    L = _lib.lib()
    plans = _plans()
    code, gcode = _lib.DTYPE_CODE[dtype], _lib.DTYPE_CODE[grad_dtype]
    g = torch.Generator(device=dev()).manual_seed(700 + C)
    for K in (2, 3, 8, 16):
        cur_buf = torch.randn(2 * K + 1, GRID, GRID, C, generator=g, device=dev()).to(dtype)
        orig = list(torch.randn(K, GRID, GRID, C, generator=g, device=dev()).to(dtype))
        cur = [cur_buf[2 * e + 1] for e in range(K)]
        fw = [0.0 if e == 3 else 7.5 + e for e in range(K)]
        bw = [0.0 if e == 4 else 1.5 + 0.25 * e for e in range(K)]
        if K < 8:                                    # the zero weights of the short batches: one on each kind
            fw[1], bw[0] = 0.0, 0.0
        scale = [256.0 if e % 2 else 64.0 + e for e in range(K)]
        nan = lambda: torch.full((2 * K, GRID, GRID, C), float("nan"), dtype=grad_dtype, device=dev())
        nanl = lambda: torch.full((K, 3), float("nan"), device=dev())
        ref, ref_nl, ref_loss = nan(), nan(), nanl()
        for e in range(K):
            _single(cur[e], orig[e], plans[e], fw[e], bw[e], scale[e], ref[2 * e], ref_loss[e])
            _single(cur[e], orig[e], plans[e], fw[e], bw[e], scale[e], ref_nl[2 * e], None)
        ws, wsb = _workspace(C, K)
        outs = []
        for want_loss in (True, True, False):        # (twice with the loss: two runs are equal)
            out, loss = nan(), (nanl() if want_loss else None)
            items = _items(plans[:K], cur, orig, [out[2 * e] for e in range(K)], loss, fw, bw, scale)
            _lib.check(L.dh_energy_fwd_bwd_planned_mixed_batch(items, _flags(plans[:K]), K, code, C, GRID, gcode, _lib.ptr(ws), wsb,
                                                               _lib.stream_ptr()), "mixed batch")
            outs.append((out, loss))
        torch.cuda.synchronize()
        for e in range(K):
            kind = "weighted" if plans[e].weighted else "unweighted"
            assert torch.isfinite(ref[2 * e]).all() and torch.isfinite(ref_loss[e]).all(), (K, e)
            assert torch.equal(ref_nl[2 * e], ref[2 * e])
            for out, loss in outs:
                assert torch.equal(out[2 * e], ref[2 * e]), f"K = {K}, item {e} ({kind}): gradient differs from the single call"
                assert loss is None or torch.equal(loss[e], ref_loss[e]), \
                    f"K = {K}, item {e} ({kind}): loss {loss[e].tolist()} != {ref_loss[e].tolist()}"
                assert torch.isnan(out[2 * e + 1]).all()                               # the slots between the items stay untouched
        assert torch.equal(outs[0][0][::2], outs[1][0][::2]) and torch.equal(outs[0][1], outs[1][1])      # run to run
        assert float(ref[0].abs().max()) > 0 and float(ref[2].abs().max()) > 0
        if K >= 8:
            assert float(ref_loss[6][1]) == 0 and float(ref_loss[7][1]) == 0 and float(ref[12].abs().max()) > 0      # no pairs: background only
        # the wrapper, gradients only (two launches) and with the loss
        souts = [torch.full((GRID, GRID, C), float("nan"), dtype=grad_dtype, device=dev()) for _ in range(K)]
        loss, grads = energy_and_grad_planned_mixed(cur, orig, plans[:K], fw, bw, scale, outs=souts, grad_dtype=grad_dtype)
        assert loss is None and all(torch.equal(grads[e], ref[2 * e]) for e in range(K))
        loss, grads = energy_and_grad_planned_mixed(cur, orig, plans[:K], fw, bw, scale, want_loss=True, grad_dtype=grad_dtype)
        assert torch.equal(loss, ref_loss) and all(torch.equal(grads[e], ref[2 * e]) for e in range(K))
    # batches of one kind through the new entry equal the existing batched entries
    for kind in (0, 1):
        sel = list(range(kind, 16, 2))
        a = energy_and_grad_planned_batch([cur[e] for e in sel], [orig[e] for e in sel], [plans[e] for e in sel], [fw[e] for e in sel],
                                          [bw[e] for e in sel], [scale[e] for e in sel], want_loss=True, grad_dtype=grad_dtype)
        b = energy_and_grad_planned_mixed([cur[e] for e in sel], [orig[e] for e in sel], [plans[e] for e in sel], [fw[e] for e in sel],
                                          [bw[e] for e in sel], [scale[e] for e in sel], want_loss=True, grad_dtype=grad_dtype)
        assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
        assert all(torch.equal(x, ref[2 * e]) for x, e in zip(b[1], sel))


def test_mixed_batch_refusals_come_before_any_launch():
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd.losses import energy_and_grad_planned_mixed
    L = _lib.lib()
    plans = _plans()
    C = 64
    cur = torch.zeros(17, GRID, GRID, C, dtype=torch.float16, device=dev())
    grad = torch.full_like(cur, float("nan"))
    loss = torch.full((17, 3), float("nan"), device=dev())
    ws, wsb = _workspace(C, 16)
    ws = torch.empty(2 * wsb, dtype=torch.uint8, device=dev())
    one = [1.0] * 17

    def call(pl, flags=None, shrink=None):
        items = _items(pl, cur, cur, grad, loss, one, one, one)
        if shrink is not None:
            items[shrink].plan_bytes -= 4096
        rc = L.dh_energy_fwd_bwd_planned_mixed_batch(items, _flags(pl, flags), len(pl), 0, C, GRID, 0, _lib.ptr(ws), 2 * wsb,
                                                     _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc
    # K = 17
    assert call([plans[e % 16] for e in range(17)]) != 0 and b"16" in L.dh_last_error()
    with pytest.raises(ValueError):
        energy_and_grad_planned_mixed(list(cur), list(cur), [plans[e % 16] for e in range(17)], one, one, one)
    # a plan buffer that is too small for its kind, weighted or not
    assert call(plans[:4], shrink=2) != 0 and b"plan buffer too small" in L.dh_last_error()
    assert call(plans[:4], shrink=1) != 0 and b"plan buffer too small" in L.dh_last_error()
    # a weighted flag on a plain plan's buffer: the weighted layout does not fit into it
    assert plans[1].nbytes < plans[0].nbytes
    assert call(plans[:4], flags=[1, 1, 1, 0]) != 0 and b"plan buffer too small" in L.dh_last_error()
    assert torch.isnan(grad).all() and torch.isnan(loss).all()                 # refused as a whole: nothing was launched
    assert call(plans[:4]) == 0 and torch.isfinite(grad[:4]).all() and torch.isnan(grad[4:]).all()
