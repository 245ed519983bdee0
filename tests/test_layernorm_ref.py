"""CPU: the float64 LayerNorm / GEGLU references of tests/layernorm_ref.py against torch autograd, the case table of
tests/test_layernorm_gpu.py against the launch forms it has to cover, and the gates against a plain f32 restatement of the kernels'
arithmetic: the restatement stays inside them in every case (the gates can be met), three mutants of it do not, where a pinned
coverage table says so (the gates, the families and the shapes can see what they are there to see)."""
import pytest
import torch
import torch.nn.functional as F

import layernorm_ref as R
from per_element import within

DT_IDS = {torch.float16: "f16", torch.bfloat16: "bf16"}


# ------------------------------------------------------------------------------------------------ references against autograd
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("rows,C", [(3, 8), (77, 64), (131, 520)])
def test_layernorm_reference_equals_autograd(rows, C, family):
    i = R.inputs(rows, C, family, torch.float16)
    o = R.reference(i.x, i.gamma, i.beta, R.EPS, i.dy, i.add)
    xr = i.x.double().requires_grad_(True)
    y = F.layer_norm(xr, (C,), i.gamma.double(), i.beta.double(), R.eps32())
    g, = torch.autograd.grad(y, xr, i.dy.double())
    assert (o.y - y.detach()).abs().max().item() <= 1e-12
    assert (o.dx0 - g).abs().max().item() <= 1e-12
    assert (o.dx - (g + i.add.double())).abs().max().item() <= 1e-12
    X = i.x.double()
    assert (o.mean - X.mean(dim=1)).abs().max().item() <= 1e-12
    assert (o.rstd - (X.var(dim=1, unbiased=False) + R.eps32()).rsqrt()).abs().max().item() <= 1e-12 * o.rstd.max().item()
    # the magnitudes bound the terms they stand for
    assert bool((o.mag_y >= o.y.abs() - 1e-12).all()) and bool((o.mag_dx >= o.dx.abs() - 1e-12).all())


@pytest.mark.parametrize("family", R.GEGLU_FAMILIES)
@pytest.mark.parametrize("rows,Fd", [(3, 16), (3, 48), (1, 1280)])
def test_geglu_reference_equals_autograd(rows, Fd, family):
    x, dy = R.geglu_inputs(rows, Fd, family, torch.float16)
    o = R.geglu_reference(x, dy, torch.float16)
    xr = x.double().requires_grad_(True)
    y = xr[:, :Fd] * F.gelu(xr[:, Fd:])
    g, = torch.autograd.grad(y, xr, dy.double())
    # (|value| reaches 200: 1e-12 relative to the size of the result, which is float64's own rounding of it)
    for got, ref in ((o.y, y.detach()), (o.d_value, g[:, :Fd]), (o.d_gate, g[:, Fd:])):
        assert ((got - ref).abs() / (1.0 + ref.abs())).max().item() <= 1e-12
    if family == "wide":
        assert x[:, :Fd].abs().max().item() > 190 and x[:, Fd:].min().item() < -11 and x[:, Fd:].max().item() > 11


def test_glu_paired_index_is_the_kernels_column_map():
    """glu_col of csrc/unet_kernels.h: output o's value at stored column 32 (o >> 4) + (o & 15), its gate 16 columns further"""
    for Fd in (16, 48, 1280):
        idx = R.glu_paired_index(Fd)
        assert sorted(idx.tolist()) == list(range(2 * Fd))
        for o in range(Fd):
            col = 32 * (o >> 4) + (o & 15)
            assert int(idx[col]) == o and int(idx[col + 16]) == Fd + o


# ------------------------------------------------------------------------------------------------------------- the case table
def test_case_table_covers_every_launch_form():
    """every (NCH, last-slot population) pair the four instantiations have at their edges, both block shapes of the backward, all
    three forms of `add`, every family in both types; the rows the issue of this table asks for"""
    pairs = {(R.nch_of(C), R.last_slot_population(C)) for _, C in R.SHAPES}
    assert pairs == {(1, 1), (1, 8), (1, 64), (2, 1), (2, 64), (3, 1), (3, 64), (8, 1), (8, 64)}
    assert {C for _, C in R.SHAPES} == {8, 64, 512, 520, 1024, 1032, 1536, 1544, 4096}
    for nch in (1, 2, 3, 8):
        assert {R.wpb_of(rows) for rows, C in R.SHAPES if R.nch_of(C) == nch} == {1, 4}
    for rows, C in R.SHAPES:
        assert rows >= C // 8 and rows % 4 != 0 and C % 8 == 0 and C <= R.LN_MAX_C
    assert set(R.CASES) == {(rows, C, f) for rows, C in R.SHAPES for f in R.FAMILIES} and len(R.CASES) == len(set(R.CASES))
    assert R.ADD_FORMS == ("separate", "none", "alias") and set(R.DTYPES) == {torch.float16, torch.bfloat16}
    # the spike family hits every chunk of every lane slot, with x and with dy
    for rows, C in R.SHAPES:
        cx, cd = R.spike_columns(rows, C)
        assert set((cx // 8).tolist()) == set(range(C // 8)) == set((cd // 8).tolist())
        assert set((cx % 8).tolist()) == set(range(min(8, rows))) == set((cd % 8).tolist())


# --------------------------------------------------------------------------------- the kernels' arithmetic, restated in f32
MUTANTS = ("drop_chunk", "s1_x0.9", "last_slot_unstored")


def row_sum(v, C, mutant):
    """k_ln_*'s row reduction in f32: every lane adds its chunks slot by slot, element by element, then the six-level wave tree.
    drop_chunk: the row's last chunk is left out."""
    rows, nch = v.shape[0], C // 8
    slots = (nch + 63) // 64
    pad = torch.zeros(rows, slots * 512, dtype=torch.float32)
    pad[:, :C] = v
    if mutant == "drop_chunk":
        pad[:, 8 * (nch - 1):8 * nch] = 0.0
    t = pad.view(rows, slots, 64, 8)
    s = torch.zeros(rows, 64, dtype=torch.float32)
    for k in range(slots):
        for e in range(8):
            s = s + t[:, k, :, e]
    for _ in range(6):
        s = s[:, 0::2] + s[:, 1::2]
    return s


def restated(i, dtype, add_form, mutant=None):
    """y, mean, rstd, dx as k_ln_fwd and k_ln_bwd compute them (f32, one rounding to the storage type), outputs NaN-filled first"""
    rows, C = i.x.shape
    x, dy, gamma, beta = i.x.float(), i.dy.float(), i.gamma, i.beta
    fC, eps = torch.tensor(float(C), dtype=torch.float32), torch.tensor(R.EPS, dtype=torch.float32)
    mean = row_sum(x, C, mutant) / fC
    d = x - mean
    rstd = torch.rsqrt(row_sum(d * d, C, mutant) / fC + eps)
    y = ((x - mean) * rstd * gamma + beta).to(dtype)
    xh = (x - mean) * rstd
    dg = dy * gamma
    s1 = row_sum(dg, C, mutant) / fC
    if mutant == "s1_x0.9":
        s1 = s1 * 0.9
    s2 = row_sum(dg * xh, C, mutant) / fC
    r = rstd * (dg - s1 - xh * s2)
    if add_form != "none":
        r = r + i.add.float()
    dx = r.to(dtype)
    if mutant == "last_slot_unstored":
        first = 512 * ((C // 8 + 63) // 64 - 1)
        y[:, first:] = float("nan")
        dx[:, first:] = float("nan")
    return y, mean[:, 0], rstd[:, 0], dx


def failures(i, o, dtype, mutant=None):
    """the outputs of one case (inputs i, reference o) that leave their gate"""
    bad = []
    for form in R.ADD_FORMS:
        y, mean, rstd, dx = restated(i, dtype, form, mutant)
        ref, mag = (o.dx0, o.mag_dx0) if form == "none" else (o.dx, o.mag_dx)
        checks = [(f"dx/{form}", dx, ref, R.gate16(ref, mag, dtype))]
        if form == "separate":
            checks += [("y", y, o.y, R.gate16(o.y, o.mag_y, dtype)), ("mean", mean, o.mean, R.gate_mean(o)), ("rstd", rstd, o.rstd, R.gate_rstd(o))]
        for what, got, want, tol in checks:
            try:
                within(got, want, tol, what)
            except AssertionError:
                bad.append(what)
    return set(bad)


ALL_DX = {"dx/separate", "dx/none", "dx/alias"}
EVERYTHING = ALL_DX | {"y", "mean", "rstd"}


# COVERAGE TABLE (pinned): the outputs a mutant must push out of their gates, in EVERY case of the table (family, shape, type); every
# other output must stay inside.
#   drop_chunk          every reduction loses eight channels: mean and rstd, and with them y and dx (spike: in the rows whose spike
#                       sits in the lost chunk)
#   s1_x0.9             dx alone, through rstd s1 / 10: s1 is of order 1 in dymean and ~ 1 / sqrt(C) elsewhere, where the elements of
#                       small |dx| (their own 16-bit spacing is the gate) still see it, behind a unit-normal `add` as well
#   last_slot_unstored  the poison stays in y and dx; the statistics are right
COVERAGE = {"drop_chunk": EVERYTHING, "s1_x0.9": ALL_DX, "last_slot_unstored": ALL_DX | {"y"}}


@pytest.mark.parametrize("dtype", R.DTYPES, ids=DT_IDS.get)
@pytest.mark.parametrize("rows,C", R.SHAPES)
def test_restated_kernels_meet_the_gates_and_mutants_do_not(rows, C, dtype):
    assert tuple(COVERAGE) == MUTANTS
    for family in R.FAMILIES:
        i = R.inputs(rows, C, family, dtype)
        o = R.reference(i.x, i.gamma, i.beta, R.EPS, i.dy, i.add)
        assert failures(i, o, dtype) == set(), (family, "the plain restatement")
        for m in MUTANTS:
            got = failures(i, o, dtype, m)
            assert got == COVERAGE[m], (m, family, got)
