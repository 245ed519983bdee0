"""GPU: every softmax-bearing attention kernel over the logit range real checkpoints produce (tests/attention_range.py: logits of
standard deviation 4 and 16, rows shifted by tens of nats, an attention sink over a thousand flat keys, flat rows, and exact
one-hot rows) against float64 -- k_attn_fwd, k_attn_bwd_dq, k_attn_bwd_dkv with k_attn_dkv_reduce and k_attn_delta through
dh_dbg_attention, the causal forward through dh_dbg_attention_causal, and the cross-attention epilogues of gemm.hip (EPI_XATTN,
EPI_XATTN_DQ) through dh_dbg_gemm_xattn / dh_dbg_gemm_xattn_dq behind an identity projection.  The gates are those of
test_attention_forward_backward, unchanged; tests/test_attention_range.py shows on the CPU that a model of the kernels' 16-bit
roundings passes them with room on these very tensors, and which launch forms the shapes reach.  The one_hot family is exact:
its outputs are compared to the bit.  Every output starts NaN-filled.

What the module found: fp16 P was rounded toward zero, which biased the forward's o and through delta took dq / dk
of the shifted and sink cases past their gates; pack8 now rounds to nearest (csrc/attn_tile.h)."""
import functools

import pytest
import torch

import attention_range as R
import test_attn_plan as T
import test_xattn_epilogue_gpu as X
from test_attention_range import ATTN_TOL, group_starts
from test_engine_kernels_gpu import ulp16, within
from test_unet_kernels_gpu import DT, L, P, close, dev, poisoned

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
# one_hot results are exact: wherever the exact value is not zero the output must equal it, which for a 16-bit output is equality
# of the bits.  Where it is zero a kernel may leave what the keys of logit 0 contribute, exp(-72) = 5e-32 each: under EXACT.
EXACT = 1e-20


def flash_case(family, dtype, shape):
    return R.make(family, dtype, *shape, dev(), group_starts=group_starts(*shape))


def run_flash(c, B, H, Nq, Nk):
    """dh_dbg_attention: forward, dQ (which leaves delta) and dK/dV with the hook's scratch; the launches equal the plans"""
    dtype, C = c["dtype"], H * 64
    o, dq = poisoned((B, Nq, C), dtype), poisoned((B, Nq, C), dtype)
    dk, dv = poisoned((B, Nk, C), dtype), poisoned((B, Nk, C), dtype)
    lse, delta = poisoned((B, H, Nq), torch.float32), poisoned((B, H, Nq), torch.float32)
    L().check(L().lib().dh_dbg_attention(DT[dtype], P(c["q"]), C, P(c["k"]), P(c["v"]), C, P(o), C, P(lse), P(c["do"]), P(delta), P(dq),
                                         P(dk), P(dv), B, H, Nq, Nk, L().stream_ptr()), "dh_dbg_attention")
    torch.cuda.synchronize()
    for kind in (T.FWD, T.DQ, T.DKV):
        planned = T.named(T.plan(kind, B, H, Nq, Nk, 0, T.DBG_SCRATCH if kind == T.DKV else 0))
        assert planned["launch"] == 1 and T.last_launch(kind) == {f: planned[f] for f in T.LAST}, (kind, planned, T.last_launch(kind))
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


def flash_cases():
    return [(s, f) for s in R.SHAPES for f in R.flash_families(s[3])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,family", flash_cases())
def test_flash_kernels_over_the_logit_range(dtype, shape, family):
    c = flash_case(family, dtype, shape)
    got, ref = run_flash(c, *shape), c["ref"]
    tol = ATTN_TOL[dtype]
    what = f"range {family} {dtype} {shape}"
    close(got["o"], ref["o"], tol, tol, what + " fwd")
    close(got["lse"], ref["lse"], 1e-3, 2e-3, what + " lse")
    for nm in ("dq", "dk", "dv"):
        close(got[nm], ref[nm], 2 * tol, 2 * tol * max(1.0, ref[nm].abs().max().item()) * 0.2, what + " " + nm)


def exact(got, want, what, residue=None):
    """got == want wherever want != 0; where want == 0, |got| <= EXACT, or <= residue (a tensor like want) where that is larger"""
    g, w = got.double(), want.double()
    assert tuple(g.shape) == tuple(w.shape), what
    slack = torch.full_like(w, EXACT) if residue is None else residue.double().clamp(min=EXACT)
    bad = ~torch.isfinite(g) | torch.where(w != 0, g != w, g.abs() > slack)
    n = int(bad.sum())
    if n:
        i = int(bad.reshape(-1).long().argmax())
        idx = tuple(int(j) for j in torch.unravel_index(torch.tensor(i), bad.shape))
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ from the exact result, the first at {idx}: got "
                             f"{g.reshape(-1)[i].item():.9g}, exact {w.reshape(-1)[i].item():.9g} (slack at zero {slack.reshape(-1)[i].item():.3g})")


def f32_residue(dtype, n_terms, abs_sum):
    """What an exact ZERO may come out as where it is the sum of several non-zero integer terms.  bf16 has f32's exponent range, so
    the weights exp(-72) of the logit-0 keys survive the rounding of P and ride along in the matrix unit's sums as addends 1e-31
    small; a sum of integers that passes through +-1 on its way to 0 then comes back as -2^-24 (measured: the causal o of two
    winners v = 1, -1; dv of a key whose rows' dO cancel), one f32 unit in the last place of a partial sum -- the addend is not
    rounded to nearest into the running sum.  Bound: one ulp, 2^-23 of the largest partial sum (<= the sum of the terms'
    magnitudes), per term.  fp16 rounds those weights to zero: no residue, EXACT holds.  A single term needs none in either type."""
    if dtype == torch.float16:
        return None
    return torch.where(n_terms >= 2, n_terms.double() * abs_sum.double() * 2.0 ** -23, torch.zeros_like(abs_sum, dtype=torch.float64))


def check_one_hot_forward(c, o, lse, what, causal=False):
    """o: the winner's v to the bit on rows of one winner (of one or two in the causal form, where the mean of two is a 16-bit
    number as well), within one 16-bit ulp of the float64 mean elsewhere; lse = 72 + ln(winners) to 1e-5 relative"""
    H, dtype = c["H"], c["dtype"]
    w = R.winners(c, causal)
    cnt = w.sum(-1)                                                                   # [B][H][Nq]
    assert int(cnt.min()) >= 1
    V = R.heads(c["v"].double(), H)
    mean = R.unheads((w.double() @ V) / cnt[..., None])                               # [B][Nq][C]
    wide = lambda t: R.unheads(t[..., None].expand(*cnt.shape, 64))
    few = wide(cnt <= (2 if causal else 1))
    assert bool(few.any())
    residue = f32_residue(dtype, wide(cnt), R.unheads(w.double() @ V.abs()))
    exact(o.double()[few], mean[few], what + " o, rows of one winner" + (" or two" if causal else ""), None if residue is None else residue[few])
    if not bool(few.all()):
        ulp = ulp16(mean, dtype) + (0.0 if residue is None else residue)              # (at a mean of 0, bf16's ulp is 9e-41)
        within(o.double()[~few], mean[~few], ulp[~few], what + " o, rows of several winners")
    want = R.ONE_HOT_LOGIT + torch.log(cnt.double())
    within(lse, want, 1e-5 * want, what + " lse")
    return w


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_flash_kernels_on_one_hot_rows(dtype, shape):
    """every row has one key of logit 72 over keys of logit 0 -- at the first and last key of tiles, wave halves and key groups, in
    the ragged last tile -- and integer v and dO: o = v[winner], dv[j] = the sum of dO over the rows key j wins, and dq = dk = 0
    because dP - delta is exactly zero on the winner.  No element is allowed off."""
    c = flash_case("one_hot", dtype, shape)
    B, H, Nq, Nk = shape
    got = run_flash(c, *shape)
    what = f"one_hot {dtype} {shape}"
    w = check_one_hot_forward(c, got["o"], got["lse"], what)
    assert torch.equal(w.long().argmax(-1), c["winner"])
    DO, wt = R.heads(c["do"].double(), H), w.double().transpose(-1, -2)
    dv = R.unheads(wt @ DO)                                                           # exact: integers
    rows_won = R.unheads(w.sum(-2)[..., None].expand(B, H, Nk, 64))
    exact(got["dv"], dv, what + " dv", f32_residue(dtype, rows_won, R.unheads(wt @ DO.abs())))
    assert bool((rows_won == 0).any()) and bool((dv[rows_won == 0] == 0).all())       # (a key that wins nothing: |dv| <= EXACT)
    exact(got["dq"], torch.zeros(got["dq"].shape, dtype=torch.float64, device=dev()), what + " dq")
    exact(got["dk"], torch.zeros_like(dv), what + " dk")


# ---------------------------------------------------------------------------------------------------------------- causal forward
def run_causal(c, B, H, N):
    dtype, C = c["dtype"], H * 64
    o, lse = poisoned((B, N, C), dtype), poisoned((B, H, N), torch.float32)
    L().check(L().lib().dh_dbg_attention_causal(DT[dtype], P(c["q"]), C, P(c["k"]), P(c["v"]), C, P(o), C, P(lse), B, H, N, N,
                                                L().stream_ptr()), "dh_dbg_attention_causal")
    torch.cuda.synchronize()
    planned = T.named(T.plan(T.FWD, B, H, N, N, 1))
    assert planned["launch"] == 1 and T.last_launch(T.FWD) == {f: planned[f] for f in T.LAST}, (planned, T.last_launch(T.FWD))
    return o, lse


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,N", R.CAUSAL_SHAPES)
def test_causal_forward_over_the_logit_range(dtype, B, H, N):
    """the mask at the diagonal key under a sharp softmax: logits of standard deviation 16, and the one_hot form in which the
    newest visible key of every row is a winner (hidden one key early, a row loses it; one key late, a row gains a winner)"""
    c = R.scaled(16.0, dtype, B, H, N, N, dev(), seed=B + H + N, causal=True)
    o, lse = run_causal(c, B, H, N)
    tol = ATTN_TOL[dtype]
    what = f"causal range scaled16 {dtype} B={B} H={H} N={N}"
    close(o, c["ref"]["o"], tol, tol, what + " fwd")
    close(lse, c["ref"]["lse"], 1e-3, 2e-3, what + " lse")
    c = R.one_hot_causal(dtype, B, H, N, dev(), seed=B + H + N)
    o, lse = run_causal(c, B, H, N)
    check_one_hot_forward(c, o, lse, f"causal one_hot {dtype} B={B} H={H} N={N}", causal=True)


# ------------------------------------------------------------------------------------------------ the cross-attention epilogues
XATTN_FAMILIES = ["scaled16", "shifted", "one_hot"]


@functools.lru_cache(maxsize=None)         # (the forward's and the twin's test share a case: a few hundred KB each)
def xattn_case(family, dtype, B, Nq, H, Nk):
    """The family's q (or dO) behind an identity projection -- K = C, W = I, no bias, no folded LayerNorm -- so the GEMM's tile IS
    the chosen tensor; K | V in one tensor with a padded row and a column offset, as the engine's hoisted text projection has them"""
    r = R.make(family, dtype, B, H, Nq, Nk, dev())
    M, C = B * Nq, 64 * H
    col, ld = 64, 2 * C + 192
    kv = torch.zeros(B * Nk, ld, dtype=dtype, device=dev())
    kv[:, col:col + C] = r["k"].reshape(B * Nk, C)
    kv[:, col + C:col + 2 * C] = r["v"].reshape(B * Nk, C)
    eye = torch.eye(C, dtype=dtype, device=dev())
    c = dict(dtype=dtype, B=B, Nq=Nq, H=H, Nk=Nk, K=C, M=M, C=C, x=r["q"].reshape(M, C).contiguous(), kv=kv, k=kv[:, col:col + C],
             v=kv[:, col + C:col + 2 * C], ld=ld, bias=None, lnf=False, W=eye)
    return c, r


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", XATTN_FAMILIES)
@pytest.mark.parametrize("B,Nq,H,Nk", R.XATTN_CASES)
def test_cross_attention_epilogue_over_the_logit_range(dtype, family, B, Nq, H, Nk):
    """EPI_XATTN: o and lse of the launch that carries the attention against float64 under the rule of
    tests/test_xattn_epilogue_gpu.py (twice the attention tolerance; lse 2e-3 / 4e-3 -- the projection is the identity, so q is
    not rounded again and that file's allowance for it is zero) and against the two-launch path of the same build at the single
    tolerance; one_hot: o to the bit"""
    c, r = xattn_case(family, dtype, B, Nq, H, Nk)
    M, C, tol = c["M"], c["C"], ATTN_TOL[dtype]
    what = f"xattn range {family} {dtype} B={B} Nq={Nq} H={H} Nk={Nk}"
    q0, o0, lse0, carried0 = X.run_xattn(c, 1, 1 | 16)
    assert carried0 == 0, what + ": stage bit 16 must switch the form off"
    for save in (1, 0):
        q, o, lse, carried = X.run_xattn(c, save, 1)
        assert carried == 1, what
        if save:
            assert torch.equal(q, c["x"]) and torch.equal(q0, c["x"]), what + ": the identity projection must return q"
        o3 = o.reshape(B, Nq, C)
        close(o3, r["ref"]["o"], 2 * tol, 2 * tol, what + f" save={save} o vs float64")
        close(lse, r["ref"]["lse"], 2e-3, 4e-3, what + f" save={save} lse vs float64")
        close(o, o0, tol, tol, what + f" save={save} o vs two launches")
        close(lse, lse0, 1e-3, 2e-3, what + f" save={save} lse vs two launches")
        if family == "one_hot":
            check_one_hot_forward(r, o3, lse, what + f" save={save}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", XATTN_FAMILIES)
@pytest.mark.parametrize("B,Nq,H,Nk", R.XATTN_CASES)
def test_cross_attention_dq_epilogue_over_the_logit_range(dtype, family, B, Nq, H, Nk):
    """EPI_XATTN_DQ: the dO tile (identity projection of the family's dO) turned into dq from the saved q, the float64 o rounded
    to the storage type and the float64 lse, against the float64 gradient (twice the attention tolerance, gradients scaled as in
    test_attention_forward_backward) and against k_attn_bwd_dq behind the unfused GEMM (the single tolerance)"""
    c, r = xattn_case(family, dtype, B, Nq, H, Nk)
    M, C, tol = c["M"], c["C"], ATTN_TOL[dtype]
    what = f"xattn dq range {family} {dtype} B={B} Nq={Nq} H={H} Nk={Nk}"
    q = c["x"]
    o = r["ref"]["o"].reshape(M, C).to(dtype).contiguous()
    lse = r["ref"]["lse"].float().contiguous()
    A = r["do"].reshape(M, C).contiguous()
    do0, dq0, carried0 = X.run_xattn_dq(c, q, o, lse, A, c["W"], 1 | 32)
    assert carried0 == 0 and torch.equal(do0, A), what + ": stage bit 32 must switch the form off; the identity projection returns dO"
    do1, dq1, carried = X.run_xattn_dq(c, q, o, lse, A, c["W"], 1)
    assert carried == 1 and bool(torch.isnan(do1).all()), what
    gq = r["ref"]["dq"].reshape(M, C)
    scale = max(1.0, gq.abs().max().item()) * 0.2
    close(dq1, gq, 2 * tol, 2 * tol * scale, what + " dq vs float64")
    close(dq1, dq0, tol, tol * scale, what + " dq vs two launches")
    if family == "one_hot":
        exact(dq1, torch.zeros_like(gq), what + " dq")
