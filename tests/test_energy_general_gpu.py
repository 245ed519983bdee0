"""The general guidance-energy entry (dh_energy_fwd_bwd through losses.energy_and_grad: k_load_map, k_pool, k_spread,
k_pair_term, k_colsum, k_global_diff, k_global_apply, k_store_grad) against the float64 reference of
tests/energy_general_ref.py, element by element, at the shapes, channel counts and types of its case table: resized maps
from 1 x 1 up to a down-sizing 128 -> 64, the ratios below 1/4 where the resize adjoint's gather window used to drop readers,
C on both sides of a wave and of the 256-thread stride, all four input / gradient type pairs, patch 1 and 3, and
correspondence sets down to a single pair at each border clamp.

An L1 gradient is a sum of signs: an element that a difference below tau = 2^-18 max|input| enters is left out, under the
caps tests/test_energy_general_ref.py holds for every case on the CPU (and check_caps repeats here).  Every other element
meets the gates of test_energy_vs_golden, plus one ulp of the stored value for a 16-bit gradient:
  loss      |d| <= 2e-5 max(1, |ref|), each of the three values
  gradient  |d| <= 2e-6 + 1e-4 max|ref| (+ 2^-10 |ref| fp16, 2^-7 |ref| bf16), on gradient / grad_scale
with no element over: close() (for the worst ratio of each site under DH_CLOSE_RATIOS, and its non-finite check) is
followed by the plain all().  The gradient buffer is NaN-filled before every call."""
import numpy as np
import pytest
import torch

import energy_general_ref as R
from test_unet_kernels_gpu import close, dev, poisoned

pytestmark = pytest.mark.gpu


def gate(got, ref, rtol, atol, what):
    close(got, ref, rtol, atol, what)
    over = (got.double() - ref.double()).abs() - (atol + rtol * ref.double().abs())
    assert float(over.max()) <= 0, f"{what}: {int((over > 0).sum())} elements over the gate, the worst by {float(over.max()):.3g}"


def run_call(case, call, cur, org, pc, cells, tau, what):
    from diffusionhandles_amd import losses as LS
    ref = R.layer(cur, org, cells, call.fg_w, call.bg_w, case.grid, case.patch, case.patch, call.bg_mode)
    R.check_caps(case, call, ref, tau)
    out = poisoned((case.h, case.w, case.C), case.grad_dtype)
    loss, grad = LS.energy_and_grad(cur.to(dev()), org.to(dev()), pc, call.fg_w, call.bg_w, case.patch, case.patch,
                                    (case.grid, case.grid), bg_loss_type=call.bg_mode, grad_scale=R.GRAD_SCALE,
                                    grad_dtype=case.grad_dtype, out=out)
    assert grad is out and grad.dtype == case.grad_dtype
    scale = ref["loss"].abs().clamp(min=1.0)
    gate(loss.cpu().double() / scale, ref["loss"] / scale, 0.0, 2e-5, f"{what} loss")
    got = grad.cpu().double() / R.GRAD_SCALE
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} gradient elements are not finite"
    skip = R.excluded(case, ref, tau)
    gate(torch.where(skip, ref["grad"], got), ref["grad"], R.STORAGE_ULP[case.grad_dtype],
         2e-6 + 1e-4 * float(ref["grad"].abs().max()), f"{what} grad")


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_general_energy_vs_float64(case):
    from diffusionhandles_amd import losses as LS
    cur, org = case.inputs()
    tau = R.tau(cur, org)
    for label, corr in case.correspondences():
        pc = LS.process_correspondences(corr, case.img_res, case.erosion, grid=case.grid)
        cells = R.cells_from_correspondences(corr.numpy(), case.img_res, case.erosion, case.grid)
        for k in cells:
            assert np.array_equal(np.asarray(pc[k]), cells[k]), (case.id, label, k)
        for call in case.calls():
            run_call(case, call, cur, org, pc, cells, tau, f"{case.id} {label} {call.name}")
