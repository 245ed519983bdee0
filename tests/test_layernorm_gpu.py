"""GPU: k_ln_fwd, k_ln_bwd, k_geglu_fwd and k_geglu_bwd element by element against the float64 references of tests/layernorm_ref.py,
in the forms the engines launch them: x at a row pitch, `add` separate, absent and aliasing dx, stats absent, the folded form's
gamma = 1 / beta = 0, the saved statistics compared, at every edge of the four chunk-count instantiations and of both block shapes
of the backward, over input families with row offsets, outlier channels, gradients with a row mean and single spikes.  Gates, families
and the case table are layernorm_ref's (tests/test_layernorm_ref.py holds them on the CPU); every output starts NaN-filled.
DH_CLOSE_RATIOS=<file> logs the worst error / gate of every comparison (profiles/layernorm/ has the table)."""
import os

import pytest
import torch

import layernorm_ref as R
from per_element import within
from test_unet_kernels_gpu import DT, L, P, dev, poisoned

pytestmark = pytest.mark.gpu

DT_IDS = {torch.float16: "f16", torch.bfloat16: "bf16"}
PAD = 64                                         # columns of NaN on either side of a pitched x


class Held:
    """within() for every output of a case: logs each worst ratio, collects the failures, raises them together"""
    def __init__(self, case):
        self.case, self.bad = case, []

    def __call__(self, group, got, ref, tol):
        log = os.environ.get("DH_CLOSE_RATIOS")
        if log:
            g = got.double()
            ratio = torch.where(torch.isfinite(g), (g - ref).abs() / tol, torch.full_like(ref, float("inf")))
            with open(log, "a") as f:
                f.write(f"{group}\t{self.case}\t{ratio.max().item():.4g}\n")
        try:
            within(got, ref, tol, f"{group} {self.case}")
        except AssertionError as e:
            self.bad.append(str(e))

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def layernorm(dtype, x, ldx, gamma, beta, y, stats, dy, add, dx, rows, C):
    L().check(L().lib().dh_dbg_layernorm_ld(DT[dtype], P(x), ldx, P(gamma), P(beta), P(y), P(stats), P(dy), P(add), P(dx), rows, C,
                                            R.EPS, L().stream_ptr()), "dh_dbg_layernorm_ld")
    torch.cuda.synchronize()


def on_device(i):
    for k, v in vars(i).items():
        setattr(i, k, v.to(dev()))
    return i


def pitched(x):
    """x as a column window of a NaN-padded tensor: (the window, the padded tensor, its pitch)"""
    rows, C = x.shape
    wide = poisoned((rows, C + 2 * PAD), x.dtype)
    wide[:, PAD:PAD + C] = x
    return wide[:, PAD:PAD + C], wide, C + 2 * PAD


@pytest.mark.parametrize("dtype", R.DTYPES, ids=DT_IDS.get)
@pytest.mark.parametrize("rows,C,family", R.CASES)
def test_layernorm_per_element(rows, C, family, dtype):
    """forward (y, mean, rstd) and backward with a separate add, no add and add aliasing dx, x dense; then forward and plain backward
    with x inside a NaN-padded tensor of pitch C + 128, whose padding must stay NaN"""
    i = on_device(R.inputs(rows, C, family, dtype))
    o = R.reference(i.x, i.gamma, i.beta, R.EPS, i.dy, i.add)
    held = Held(f"{DT_IDS[dtype]} {family} {rows}x{C}")
    gate_dx = {"separate": R.gate16(o.dx, o.mag_dx, dtype), "none": R.gate16(o.dx0, o.mag_dx0, dtype)}
    gate_dx["alias"] = gate_dx["separate"]
    gate_y = R.gate16(o.y, o.mag_y, dtype)

    def forward_held(tag, y, stats):
        held(f"y{tag}", y, o.y, gate_y)
        held(f"mean{tag}", stats[:, 0], o.mean, R.gate_mean(o))
        held(f"rstd{tag}", stats[:, 1], o.rstd, R.gate_rstd(o))

    for form in R.ADD_FORMS:
        y, stats = poisoned((rows, C), dtype), poisoned((rows, 2), torch.float32)
        if form == "alias":
            dx = i.add.clone()                   # the accumulated gradient, updated in place; the reference read the copy i.add
            add = dx
        else:
            dx, add = poisoned((rows, C), dtype), (i.add if form == "separate" else None)
        layernorm(dtype, i.x, C, i.gamma, i.beta, y, stats, i.dy, add, dx, rows, C)
        if form == "separate":
            forward_held("", y, stats)
        held(f"dx/{form}", dx, o.dx0 if form == "none" else o.dx, gate_dx[form])
    xw, wide, ldx = pitched(i.x)
    y, stats, dx = poisoned((rows, C), dtype), poisoned((rows, 2), torch.float32), poisoned((rows, C), dtype)
    layernorm(dtype, xw, ldx, i.gamma, i.beta, y, stats, i.dy, None, dx, rows, C)
    forward_held("/pitched", y, stats)
    held("dx/pitched", dx, o.dx0, gate_dx["none"])
    assert bool(torch.isnan(wide[:, :PAD]).all()) and bool(torch.isnan(wide[:, PAD + C:]).all()), "the padding of x was written"
    assert torch.equal(wide[:, PAD:PAD + C], i.x), "x was written"
    held.done()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=DT_IDS.get)
@pytest.mark.parametrize("rows,C", [(77, 64), (131, 520), (131, 1032), (515, 1544)])            # one per NCH
def test_layernorm_forward_without_stats_and_folded_form(rows, C, dtype):
    """stats = NULL (the text tower's final LayerNorm keeps none for a backward), and gamma = 1, beta = 0: the launch of the folded
    form, whose affine part lives in the consuming GEMM's weights"""
    i = on_device(R.inputs(rows, C, "offset", dtype))
    held = Held(f"{DT_IDS[dtype]} offset {rows}x{C}")
    o = R.reference(i.x, i.gamma, i.beta, R.EPS)
    y = poisoned((rows, C), dtype)
    layernorm(dtype, i.x, C, i.gamma, i.beta, y, None, None, None, None, rows, C)
    held("y/nostats", y, o.y, R.gate16(o.y, o.mag_y, dtype))
    ones, zeros = torch.ones(C, device=dev()), torch.zeros(C, device=dev())
    o = R.reference(i.x, ones, zeros, R.EPS)
    y, stats = poisoned((rows, C), dtype), poisoned((rows, 2), torch.float32)
    layernorm(dtype, i.x, C, ones, zeros, y, stats, None, None, None, rows, C)
    held("y/folded", y, o.y, R.gate16(o.y, o.mag_y, dtype))
    held("mean/folded", stats[:, 0], o.mean, R.gate_mean(o))
    held("rstd/folded", stats[:, 1], o.rstd, R.gate_rstd(o))
    held.done()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=DT_IDS.get)
@pytest.mark.parametrize("family", R.GEGLU_FAMILIES)
@pytest.mark.parametrize("rows", R.GEGLU_ROWS)
@pytest.mark.parametrize("Fd", R.GEGLU_F)
def test_geglu_per_element(Fd, rows, family, dtype):
    """y, d_value and d_gate in the torch column order; the kernels read and write the paired layout (glu_col)"""
    x, dy = (t.to(dev()) for t in R.geglu_inputs(rows, Fd, family, dtype))
    o = R.geglu_reference(x, dy, dtype)
    idx = R.glu_paired_index(Fd).to(dev())
    xp = x[:, idx].contiguous()
    y, dxp = poisoned((rows, Fd), dtype), poisoned((rows, 2 * Fd), dtype)
    L().check(L().lib().dh_dbg_geglu(DT[dtype], P(xp), P(y), P(dy), P(dxp), rows, Fd, L().stream_ptr()), "dh_dbg_geglu")
    torch.cuda.synchronize()
    dx = torch.empty_like(dxp)
    dx[:, idx] = dxp
    held = Held(f"{DT_IDS[dtype]} {family} {rows}x{Fd}")
    held("geglu y", y, o.y, o.gate_y)
    held("geglu d_value", dx[:, :Fd], o.d_value, o.gate_d_value)
    held("geglu d_gate", dx[:, Fd:], o.d_gate, o.gate_d_gate)
    held.done()
