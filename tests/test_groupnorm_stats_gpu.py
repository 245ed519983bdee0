"""GroupNorm statistics from every producer at large group means.

A GroupNorm's slice statistics come from whichever launch wrote its input: the statistics kernel (k_gn_partial), the channel
concatenation (k_concat_gn), the split-K reduce (k_splitk_reduce_gn) or the epilogue of an unsplit GEMM (k_gemm_dma gn_epi);
the apply kernels merge the slices.  Each producer is driven here through the debug hooks with group means of 0, 3, 30 and
100 standard deviations, the offset carried by a per-group bias or, with no bias, by the GEMM's inputs (a constant input column
times a per-group weight), so that a pivot taken from the bias alone cannot pass.  The reference is always the f64 statistics
of the kernel's own ROUNDED output (f64 autograd for dx); every output and the slice scratch start as NaN.  The tile report
(dh_dbg_gemm_last_tile) proves which kernel produced the statistics."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_unet_kernels_gpu import DT, L, P, close, dev, poisoned

pytestmark = pytest.mark.gpu

OFFSETS = [0.0, 3.0, 30.0, 100.0]
EPS = 1e-5
MEAN_TOL_SIGMA, MEAN_TOL_REL, RSTD_TOL = 1e-5, 5e-7, 1e-5


def last_tile():
    r = (ctypes.c_int * 9)()
    L().check(L().lib().dh_dbg_gemm_last_tile(r), "dh_dbg_gemm_last_tile")
    keys = ("bm", "bn", "kg", "stages", "mw", "splits", "pp", "gn_epi", "reduce_gn")
    return dict(zip(keys, list(r)))


def group_offsets(G, k, g):
    """k (nominal) standard deviations per group, random sign."""
    sign = torch.where(torch.rand(G, generator=g, device=dev()) < 0.5, -1.0, 1.0)
    return sign * k


def ref_stats(C, B, HW, G):
    x = C.double().reshape(B, HW, G, -1)
    mean = x.mean(dim=(1, 3))
    var = x.var(dim=(1, 3), unbiased=False)
    return mean, var, (var + EPS).rsqrt()


def check_stats(stats, C, B, HW, G, what):
    """(mean, rstd) published by the apply kernel vs f64 statistics of the rounded tensor C; returns the worst errors."""
    mean, var, rstd = ref_stats(C, B, HW, G)
    got = stats.double().view(B, G, 2)
    assert torch.isfinite(got).all(), f"{what}: non-finite statistics"
    sigma = var.sqrt()
    dm = (got[..., 0] - mean).abs()
    em = float((dm / sigma).max())
    er = float(((got[..., 1] - rstd).abs() / rstd).max())
    lim = MEAN_TOL_SIGMA * sigma + MEAN_TOL_REL * mean.abs()
    print(f"GNSTAT {what} mean_err/sigma {em:.2e} rstd_rel_err {er:.2e} |mean|/sigma {float((mean.abs() / sigma).max()):.1f}")
    assert bool((dm <= lim).all()), f"{what}: mean error {em:.3e} sigma over the gate"
    assert er <= RSTD_TOL, f"{what}: rstd relative error {er:.3e}"
    return em, er


def gn_ref(C, B, HW, N, G, gamma, beta, silu):
    y = F.group_norm(C.double().view(B, HW, N).permute(0, 2, 1), G, gamma.double(), beta.double(), EPS)
    if silu:
        y = F.silu(y)
    return y.permute(0, 2, 1)


def make_inputs(dtype, B, HW, N, K, conv, k, source, g, G=32):
    """A, W (plain [N][K]; convolutions [N][tap][Cin]) and bias: output sigma ~1 with group means of k sigma, per-channel spread
    0.5 sigma.  source 'bias': the offset rides on the bias; 'input': bias NULL, A has a constant column (a constant input channel
    of the convolution) and W's weight on it is the offset (centre tap only, so that the zero padding does not see it)."""
    M, cpg = B * HW, N // G
    off = group_offsets(G, k, g).repeat_interleave(cpg) + 0.5 * torch.randn(N, generator=g, device=dev())
    if conv:
        Cin = K // 9
        A = torch.randn(M, Cin, generator=g, device=dev())
    else:
        Cin = 0
        A = torch.randn(M, K, generator=g, device=dev())
    W = torch.randn(N, K, generator=g, device=dev()) / K ** 0.5
    bias = None
    if source == "bias":
        bias = off.float().contiguous()
    else:
        A[:, 0] = 1.0
        col = 4 * Cin if conv else 0
        W[:, col] = off
    return A.to(dtype), W.to(dtype), bias, Cin


# (B, HW, N, K, conv, residual, expected producer) -- residual: None, "R" (a separate tensor) or "C" (in place, R == C)
FWD_CASES = {
    "64x64":         (2, 1024, 640, 640, False, None, dict(bm=64, bn=64, gn_epi=1)),
    "64x64_b3_R":    (3, 1024, 640, 640, False, "R", dict(bm=64, bn=64, gn_epi=1)),
    "64x64_cpg8":    (2, 1024, 256, 1152, True, None, dict(bm=64, bn=64, gn_epi=1)),
    "128x64_kg2":    (1, 4096, 320, 2880, True, None, dict(bm=128, bn=64, kg=2, stages=3, gn_epi=1)),
    "128x64_st5":    (1, 4096, 320, 192, False, "C", dict(bm=128, bn=64, kg=1, stages=5, gn_epi=1)),
    "128x64_2cu":    (2, 4096, 320, 320, False, "R", dict(bm=128, bn=64, kg=1, stages=3, gn_epi=1)),
    "128x128_mw2":   (1, 4096, 640, 640, False, None, dict(bm=128, bn=128, mw=2, gn_epi=1)),
    "256x128_mw2":   (13, 256, 1280, 1280, False, "R", dict(bm=256, bn=128, mw=2, gn_epi=1)),   # (B = 16 runs on k_gemm_pp)
    "splitk_reduce": (1, 1024, 640, 5760, True, "R", dict(gn_epi=0, reduce_gn=1)),
    "pp_kernel":     (16, 1024, 640, 640, False, None, dict(pp=1, splits=1, gn_epi=0, reduce_gn=0)),
    "stats_kernel":  (1, 4096, 64, 320, False, None, dict(pp=0, gn_epi=0, reduce_gn=0)),
}
# (the 128x128 four-wave tiles are never dispatched: the policy gives every 128x128 launch eight waves, kMw128 = 1)


def run_fwd(dtype, case, k, source, stage=1, seed_extra=0):
    B, HW, N, K, conv, res, expect = FWD_CASES[case]
    lib = L().lib()
    G, M = 32, B * HW
    H = int(round(HW ** 0.5))
    g = torch.Generator(device=dev()).manual_seed(N + K + HW + B + int(k) + (7 if source == "bias" else 0) + seed_extra)
    A, W, bias, Cin = make_inputs(dtype, B, HW, N, K, conv, k, source, g)
    mode, lda = (1, Cin) if conv else (0, K)
    gamma = torch.randn(N, generator=g, device=dev()); beta = torch.randn(N, generator=g, device=dev())
    Rt = torch.randn(M, N, generator=g, device=dev()).to(dtype) if res else None

    def once(st):
        C = poisoned((M, N), dtype)
        R = None
        if res == "R":
            R = Rt
        elif res == "C":
            C.copy_(Rt); R = C
        Y = poisoned((M, N), dtype)
        stats = poisoned((B * G, 2), torch.float32); scratch = poisoned((1 << 20,), torch.float32)
        part = poisoned((16 << 20,), torch.float32)
        have = ctypes.c_int(-1)
        L().check(lib.dh_dbg_gemm_stage(st), "stage")
        try:
            L().check(lib.dh_dbg_gemm_groupnorm_res(DT[dtype], P(A), lda, P(W), M, N, K, mode, H, H, Cin, P(bias), P(R), N, P(C), P(part),
                                                part.numel(), HW, G, P(gamma), P(beta), EPS, 1, P(Y), P(stats), P(scratch),
                                                ctypes.byref(have), L().stream_ptr()), "dh_dbg_gemm_groupnorm_res")
            torch.cuda.synchronize()
            rep = last_tile()
        finally:
            L().check(lib.dh_dbg_gemm_stage(1), "stage")
        return C, Y, stats, have.value, rep

    C, Y, stats, have, rep = once(stage)
    return dict(B=B, HW=HW, N=N, G=G, C=C, Y=Y, stats=stats, have=have, rep=rep, expect=expect, gamma=gamma, beta=beta, once=once)


@pytest.mark.parametrize("k", OFFSETS)
@pytest.mark.parametrize("source", ["bias", "input"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("case", list(FWD_CASES))
def test_forward_statistics_by_producer(case, dtype, source, k):
    """GEMM -> GroupNorm + SiLU: the published (mean, rstd) match the f64 statistics of the rounded GEMM output at every group mean,
    y is the GroupNorm of that output, and C does not depend on whether the epilogue also left the statistics."""
    r = run_fwd(dtype, case, k, source)
    rep, expect = r["rep"], r["expect"]
    assert all(rep[key] == v for key, v in expect.items()), (case, rep)
    assert (r["have"] > 1) == (rep["gn_epi"] == 1) and (r["have"] == 1) == (rep["reduce_gn"] == 1), (case, r["have"], rep)
    B, HW, N, G = r["B"], r["HW"], r["N"], r["G"]
    check_stats(r["stats"], r["C"], B, HW, G, f"fwd {case} {str(dtype)[6:]} {source} {k:g}sigma")
    tol = 4e-3 if dtype == torch.float16 else 2.5e-2
    close(r["Y"].view(B, HW, N), gn_ref(r["C"], B, HW, N, G, r["gamma"], r["beta"], 1), tol, tol, "GroupNorm of the GEMM output")
    C0, _, _, have0, _ = r["once"](1 | 4)          # the forward statistics of the epilogue off: the kernel (or the reduce) leaves them
    assert have0 <= 1
    assert torch.equal(C0, r["C"]), "C differs with and without the GroupNorm epilogue"


def run_bwd(dtype, B, HW, N, K, conv, silu, res, k, stage):
    lib = L().lib()
    G, M = 32, B * HW
    H = int(round(HW ** 0.5))
    g = torch.Generator(device=dev()).manual_seed(N + K + HW + B + int(k) + 11)
    Cin = K // 9 if conv else 0
    A = torch.randn(M, Cin if conv else K, generator=g, device=dev()).to(dtype)
    W = (torch.randn(N, K, generator=g, device=dev()) / K ** 0.5).to(dtype)
    off = group_offsets(G, k, g).repeat_interleave(N // G) + 0.5 * torch.randn(N, generator=g, device=dev())
    x = (torch.randn(M, N, generator=g, device=dev()) + off).to(dtype)
    gamma = torch.randn(N, generator=g, device=dev()); beta = torch.randn(N, generator=g, device=dev())
    Rt = torch.randn(M, N, generator=g, device=dev()).to(dtype) if res else None
    mean, _, rstd = ref_stats(x, B, HW, G)
    stats = torch.stack([mean, rstd], dim=-1).float().contiguous()
    C = poisoned((M, N), dtype)
    R = None
    if res:
        C.copy_(Rt); R = C
    dx = poisoned((M, N), dtype)
    scratch = poisoned((1 << 20,), torch.float32); part = poisoned((16 << 20,), torch.float32)
    have = ctypes.c_int(-1)
    L().check(lib.dh_dbg_gemm_stage(stage), "stage")
    try:
        L().check(lib.dh_dbg_gemm_groupnorm_bwd_res(DT[dtype], P(A), Cin if conv else K, P(W), M, N, K, 1 if conv else 0, H, H, Cin, P(R), N,
                                                P(C), P(part), part.numel(), HW, G, P(x), P(gamma), P(beta), P(stats), silu, P(dx),
                                                P(scratch), ctypes.byref(have), L().stream_ptr()), "dh_dbg_gemm_groupnorm_bwd_res")
        torch.cuda.synchronize()
        rep = last_tile()
    finally:
        L().check(lib.dh_dbg_gemm_stage(1), "stage")
    return dict(x=x, C=C, dx=dx, have=have.value, rep=rep, gamma=gamma, beta=beta, G=G)


# (B, HW, N, K, conv, silu, R == C, expected producer)
BWD_CASES = {
    "64x64":          (2, 1024, 640, 640, False, 1, False, dict(bm=64, bn=64, gn_epi=2)),
    "64x64_b3_cpg8":  (3, 1024, 256, 1152, True, 1, False, dict(bm=64, bn=64, gn_epi=2)),
    "128x64_kg2":     (1, 4096, 320, 2880, True, 1, False, dict(bm=128, bn=64, kg=2, gn_epi=2)),
    "128x64_2cu":     (2, 4096, 320, 320, False, 0, False, dict(bm=128, bn=64, kg=1, stages=3, gn_epi=2)),
    "splitk_reduce":  (1, 1024, 640, 5760, True, 1, False, dict(reduce_gn=1)),
    "splitk_RC":      (1, 1024, 640, 5760, True, 1, True, dict(reduce_gn=1)),
    "unsplit_RC":     (1, 4096, 320, 2880, True, 1, True, dict(splits=1, gn_epi=0, reduce_gn=0)),
    "stats_kernel":   (1, 4096, 64, 320, False, 1, False, dict(gn_epi=0, reduce_gn=0)),
}


@pytest.mark.parametrize("k", OFFSETS)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("case", list(BWD_CASES))
def test_backward_statistics_by_producer(case, dtype, k):
    """input-gradient GEMM -> GroupNorm(+SiLU) backward with the GroupNorm input x at large group means: dx matches f64 autograd on
    the rounded dy, and the epilogue / reduce producer agrees with the statistics kernel."""
    B, HW, N, K, conv, silu, rc, expect = BWD_CASES[case]
    r = run_bwd(dtype, B, HW, N, K, conv, silu, rc, k, 1)
    rep = r["rep"]
    assert all(rep[key] == v for key, v in expect.items()), (case, rep)
    r0 = run_bwd(dtype, B, HW, N, K, conv, silu, rc, k, 1 | 8)        # the backward statistics from the statistics kernel (or the reduce)
    assert r0["have"] <= 1 and torch.equal(r["C"], r0["C"])
    G, M = r["G"], B * HW
    xin = r["x"].double().view(B, HW, N).permute(0, 2, 1).clone().requires_grad_(True)
    y = F.group_norm(xin, G, r["gamma"].double(), r["beta"].double(), EPS)
    if silu:
        y = F.silu(y)
    y.backward(r["C"].double().view(B, HW, N).permute(0, 2, 1))
    ref = xin.grad.permute(0, 2, 1).reshape(M, N)
    assert torch.isfinite(r["dx"].float()).all()
    scale = float(ref.abs().max())
    e_ref = float((r["dx"].double() - ref).abs().max()) / scale
    e_ab = float((r["dx"].float() - r0["dx"].float()).abs().max()) / scale
    print(f"GNSTAT bwd {case} {str(dtype)[6:]} {k:g}sigma have {r['have']} dx_vs_autograd {e_ref:.2e} vs_stats_kernel {e_ab:.2e}")
    tol = 3e-3 if dtype == torch.float16 else 2e-2
    assert e_ref < tol and e_ab <= (1e-3 if dtype == torch.float16 else 8e-3), (e_ref, e_ab)


# (Ca, Cb, HW, G) of every concatenation the SD2-depth up path builds at 64x64 latents, each fused with the GroupNorm after it
# (k_concat_gn); tests/test_groupnorm_concat_ops.py checks this list against the engine's own op list.  1280 + 640 in 60-channel
# groups and 640 + 320 in 30-channel groups put a group across the a | b boundary.
SD2_CONCATS = [(320, 320, 4096, 32), (640, 320, 1024, 32), (640, 320, 4096, 32), (640, 640, 1024, 32), (1280, 640, 256, 32),
               (1280, 640, 1024, 32), (1280, 1280, 64, 32), (1280, 1280, 256, 32)]
CONCATS = SD2_CONCATS


@pytest.mark.parametrize("k", OFFSETS)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("Ca,Cb,HW,G", CONCATS)
def test_concat_statistics(Ca, Cb, HW, G, dtype, k):
    """k_concat_gn + the apply kernel on every (Ca, Cb, HW) pair of the SD2-depth up path -- groups straddle the a | b boundary
    where Ca is not a multiple of the group width (1280 + 640 in 60-channel groups): the concatenation is bit-exact, the statistics
    and y meet the gates above."""
    lib = L().lib()
    C = Ca + Cb
    B = 1
    g = torch.Generator(device=dev()).manual_seed(C + HW + int(k))
    off = group_offsets(G, k, g).repeat_interleave(C // G) + 0.5 * torch.randn(C, generator=g, device=dev())
    full = (torch.randn(B * HW, C, generator=g, device=dev()) + off).to(dtype)
    a, b = full[:, :Ca].contiguous(), full[:, Ca:].contiguous()
    gamma = torch.randn(C, generator=g, device=dev()); beta = torch.randn(C, generator=g, device=dev())
    out = poisoned((B * HW, C), dtype); Y = poisoned((B * HW, C), dtype)
    stats = poisoned((B * G, 2), torch.float32); scratch = poisoned((1 << 20,), torch.float32)
    L().check(lib.dh_dbg_concat_groupnorm(DT[dtype], P(a), Ca, P(b), Cb, P(out), B, HW, G, P(gamma), P(beta), EPS, 1, P(Y), P(stats),
                                          P(scratch), L().stream_ptr()), "dh_dbg_concat_groupnorm")
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), full.view(torch.int16)), "concatenation is not bit-exact"
    check_stats(stats, out, B, HW, G, f"concat {Ca}+{Cb} HW {HW} {str(dtype)[6:]} {k:g}sigma")
    tol = 4e-3 if dtype == torch.float16 else 2.5e-2
    close(Y.view(B, HW, C), gn_ref(out, B, HW, C, G, gamma, beta, 1), tol, tol, "GroupNorm of the concatenation")


@pytest.mark.parametrize("case", list(FWD_CASES))
@pytest.mark.parametrize("source", ["bias", "input"])
def test_no_nan_at_300_sigma(case, source):
    """fp16 group means of 300 sigma: every producer gives finite statistics and a finite normalised tensor."""
    r = run_fwd(torch.float16, case, 300.0, source)
    assert torch.isfinite(r["stats"]).all(), (case, r["rep"])
    assert torch.isfinite(r["Y"].float()).all(), (case, r["rep"])
    assert torch.isfinite(r["C"].float()).all()


def test_no_nan_at_300_sigma_concat():
    Ca, Cb, HW, G = CONCATS[0]
    lib = L().lib()
    C = Ca + Cb
    g = torch.Generator(device=dev()).manual_seed(300)
    off = group_offsets(G, 300.0, g).repeat_interleave(C // G)
    full = (torch.randn(HW, C, generator=g, device=dev()) + off).half()
    a, b = full[:, :Ca].contiguous(), full[:, Ca:].contiguous()
    gamma = torch.ones(C, device=dev()); beta = torch.zeros(C, device=dev())
    out = poisoned((HW, C), torch.float16); Y = poisoned((HW, C), torch.float16)
    stats = poisoned((G, 2), torch.float32); scratch = poisoned((1 << 20,), torch.float32)
    L().check(lib.dh_dbg_concat_groupnorm(0, P(a), Ca, P(b), Cb, P(out), 1, HW, G, P(gamma), P(beta), EPS, 1, P(Y), P(stats), P(scratch),
                                          L().stream_ptr()), "dh_dbg_concat_groupnorm")
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all() and torch.isfinite(Y.float()).all()
