"""GPU parity of every GEMM launch class of the pinned plan table (tests/test_gemm_classes.py: CLASS_CASES, one smallest query per
class).  Each case launches its query under the shipped policy through the debug hook that matches its flags, with the outputs and
the split-K workspace NaN-filled, asserts the arm that ran (dh_dbg_gemm_last_tile against the plan of the query and the class, and
the carried flags gn_done / lnb_done / xa_done), and compares with a plain torch reference of the same op: f32, statistics in f64.
The tolerances are those of the existing test of the same epilogue (tests/test_unet_kernels_gpu.py, tests/test_xattn_epilogue_gpu.py).

The split-K reduce that applies a LayerNorm backward (k_splitk_reduce_ln_bwd) has paths the table's shapes do not select between:
LN_REDUCE_CASES walks them, and every LayerNorm-backward case must also equal the two-launch path (split GEMM writing dy, then the
LayerNorm backward kernel) bit for bit, as the kernel's comment promises.

Measured on the MI355X (DH_CLOSE_RATIOS): the worst element of any case stays at 0.32 of its tolerance (LayerNorm backward, fp16, 1856 x
1280 x 4096); by kind: gemm 0.13, gn 0.14, gn_bwd 0.12, lnf 0.30, lnf_glu 0.26, glu 0.12, glu_bwd 0.13, xattn 0.27, xattn_dq 0.18, ln_bwd 0.32.
What the first run found: the reduce's LayerNorm backward came out one 16-bit ulp off the two-launch path in about one element of 10^4
(fixed in k_splitk_reduce_ln_bwd), and the GroupNorm apply kernels loaded past x, gamma and beta in the threads behind the last chunk
whenever HW * C / 8 is no multiple of 256 (cases 09 and 10 here; none of the traced passes, but the 10 x 10 level of a 640-pixel image is one) -- an illegal access once, fixed in
the kernels."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import test_xattn_epilogue_gpu as XA
from test_gemm_classes import CLASS_CASES, launch_class
from test_gemm_plan import (ALIGNED, BIAS, GLU_BWD, GLU_FWD, GN_BWD, GN_STATS, LN_BWD, LNF, RESIDUAL, ROWVEC, SILU, XATTN_DQ, XATTN_FWD,
                            named, plan, shipped_hooks)  # noqa: F401  (shipped_hooks: autouse, the shipped policy)
from layernorm_ref import glu_paired_index
from test_unet_kernels_gpu import DT, L, P, close, dev, nhwc, poisoned

pytestmark = pytest.mark.gpu

TOL = {torch.float16: 4e-3, torch.bfloat16: 2.5e-2}           # GEMM, convolution, LayerNorm backward (GEGLU y: twice)
LNF_TOL = {torch.float16: 6e-3, torch.bfloat16: 3e-2}         # test_gemm_layernorm_fold
GN_DX_TOL = {torch.float16: 3e-3, torch.bfloat16: 2e-2}       # test_gemm_groupnorm_backward_statistics_by_producer (of max |dx|)


def kind_of(flags):
    """the hook and the reference a query's flags ask for"""
    if flags & XATTN_DQ:
        return "xattn_dq"
    if flags & XATTN_FWD:
        return "xattn"
    if flags & GLU_BWD:
        return "glu_bwd"
    if flags & GLU_FWD:
        return "lnf_glu" if flags & LNF else "glu"
    if flags & LNF:
        return "lnf"
    if flags & LN_BWD:
        return "ln_bwd"
    if flags & GN_BWD:
        return "gn_bwd"
    return "gn" if flags & GN_STATS else "gemm"


def out_side(q):
    conv, hw, stride, up = q[3:7]
    return 2 * hw if conv == 2 else hw * (2 if up else 1) // stride


def images(q):
    M, conv, flags, gn_HW, xa_Nq = q[0], q[3], q[9], q[10], q[13]
    return M // (out_side(q) ** 2 if conv else (gn_HW if flags & GN_STATS else (xa_Nq if flags & (XATTN_FWD | XATTN_DQ) else M)))


def rng(q):
    return torch.Generator(device=dev()).manual_seed((q[0] * 31 + q[1] * 17 + q[2] * 7 + q[9]) % (1 << 31))


def randn(g, *shape):
    return torch.randn(*shape, generator=g, device=dev())


def operands(dtype, q, g):
    """A, lda, W [N][K], mode, geometry of dh_dbg_gemm, and the f32 reference of A W^T [M][N]: a dense product, F.conv2d (of the
    up-sampled input where the query up-samples), or autograd's input gradient of a stride-2 convolution (conv == 2)"""
    M, N, K, conv, hw, stride, up = q[:7]
    if conv == 0:
        A, W = randn(g, M, K).to(dtype), (randn(g, N, K) / K ** 0.5).to(dtype)
        return A, K, W, 0, (0, 0, 0, 0, 0, 1, 0), A.float() @ W.float().t()
    Cin, Ho, B = K // 9, out_side(q), images(q)
    x = randn(g, B, Cin, hw, hw).to(dtype)
    if conv == 1:
        w = (randn(g, N, Cin, 3, 3) / K ** 0.5).to(dtype)
        xin = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if up else x.float()
        Z = nhwc(F.conv2d(xin, w.float(), None, stride=stride, padding=1)).reshape(M, N)
        return nhwc(x), Cin, w.permute(0, 2, 3, 1).reshape(N, K).contiguous(), 1, (hw, hw, Cin, Ho, Ho, stride, up), Z
    # x is dy [B][Cin][hw][hw] of a stride-2 convolution N -> Cin channels; a quarter of the taps reach each input pixel
    w = (randn(g, Cin, N, 3, 3) / (K / 4) ** 0.5).to(dtype)
    xr = torch.zeros(B, N, Ho, Ho, device=dev(), requires_grad=True)
    Z, = torch.autograd.grad(F.conv2d(xr, w.float(), None, stride=2, padding=1), xr, x.float())
    return nhwc(x), Cin, w.flip(2, 3).permute(1, 2, 3, 0).reshape(N, K).contiguous(), 2, (hw, hw, Cin, Ho, Ho, 1, 0), nhwc(Z).reshape(M, N)


def plain_epilogue(dtype, q, g, Z, dc=1.0):
    """bias (scaled by dc), per-image vector, SiLU, residual as the query's flags say; returns them and the f32 reference"""
    M, N, flags, B = q[0], q[1], q[9], images(q)
    bias = dc * randn(g, N) if flags & BIAS else None
    rowvec = randn(g, B, N) if flags & ROWVEC else None
    R = randn(g, M, N).to(dtype) if flags & RESIDUAL else None
    ref = Z
    if bias is not None:
        ref = ref + bias
    if rowvec is not None:
        ref = ref + rowvec.repeat_interleave(M // B, dim=0)
    if flags & SILU:
        ref = F.silu(ref)
    if R is not None:
        ref = ref + R.float()
    return bias, rowvec, R, ref


def workspace(elems):
    return poisoned((elems,), torch.float32) if elems else None


def gemm(dtype, A, lda, W, M, N, K, mode, geo, part_elems, bias=None, rowvec=None, rpb=1, R=None, silu=0):
    """dh_dbg_gemm into a NaN-filled [M][N] output, with a NaN-filled workspace of exactly part_elems f32"""
    C, part = poisoned((M, N), dtype), workspace(part_elems)
    L().check(L().lib().dh_dbg_gemm(DT[dtype], P(A), lda, P(W), M, N, K, mode, *geo, P(bias), P(rowvec), N if rowvec is not None else 0, rpb,
                                    P(R), N, P(C), N, silu, P(part), part_elems, L().stream_ptr()), "dh_dbg_gemm")
    torch.cuda.synchronize()
    return C


def last_tile():
    rep = (ctypes.c_int * 9)()
    L().check(L().lib().dh_dbg_gemm_last_tile(rep), "dh_dbg_gemm_last_tile")
    return list(rep)


def check_arm(cls, q):
    """the launch that just ran is the one the query plans and the class names: tile, K groups, stages and waves as launch_tile wrote
    them from its own template arguments, splits, family and GroupNorm riders of the plan it was given"""
    rep, p = last_tile(), named(plan(*q))
    assert cls is None or launch_class(p) == cls, (q, p)
    assert rep == [p["bm"], p["bn"], p["kg"], p["stages"], p["mw"], p["splits"], p["pp"], p["gn_epi"], int(p["reduce"] in (2, 3))], (rep, p)
    return p


def gn_carried(p):
    return p["gn_S"] if p["gn_epi"] else int(p["reduce"] in (2, 3))


def run_gemm_case(dtype, cls, q, what):
    M, N, K, flags = q[0], q[1], q[2], q[9]
    g = rng(q)
    A, lda, W, mode, geo, Z = operands(dtype, q, g)
    bias, rowvec, R, ref = plain_epilogue(dtype, q, g, Z)
    C = gemm(dtype, A, lda, W, M, N, K, mode, geo, q[16], bias, rowvec, M // images(q), R, int(bool(flags & SILU)))
    check_arm(cls, q)
    close(C, ref, TOL[dtype], TOL[dtype], what)


def run_gn_case(dtype, cls, q, what):
    """GEMM -> GroupNorm + SiLU (dh_dbg_gemm_groupnorm_geo): the output, the (mean, rstd) of the ROUNDED output in f64, the normalised tensor"""
    M, N, K, HW, G = q[0], q[1], q[2], q[10], q[11]
    B, g = M // HW, rng(q)
    A, lda, W, mode, geo, Z = operands(dtype, q, g)
    bias, rowvec, R, ref = plain_epilogue(dtype, q, g, Z, dc=3.0)          # a DC offset per channel: the unshifted sums must survive it
    gamma, beta = randn(g, N), randn(g, N)
    C, Y, stats = poisoned((M, N), dtype), poisoned((M, N), dtype), poisoned((B * G, 2), torch.float32)
    scratch, part, have = torch.zeros(1 << 20, device=dev()), workspace(q[16]), ctypes.c_int(-1)
    L().check(L().lib().dh_dbg_gemm_groupnorm_geo(DT[dtype], P(A), lda, P(W), M, N, K, mode, *geo, P(bias), P(rowvec), N if rowvec is not None else 0,
                                                  HW, P(R), N, P(C), P(part), q[16], HW, G, P(gamma), P(beta), 1e-5, 1, P(Y), P(stats),
                                                  P(scratch), ctypes.byref(have), L().stream_ptr()), "dh_dbg_gemm_groupnorm_geo")
    torch.cuda.synchronize()
    p = check_arm(cls, q)
    assert have.value == gn_carried(p), (have.value, p)
    close(C, ref, TOL[dtype], TOL[dtype], what + " output")
    x = C.double().view(B, HW, G, N // G)
    mean, var = x.mean(dim=(1, 3)), x.var(dim=(1, 3), unbiased=False)
    rstd = (var + 1e-5).rsqrt()
    got = stats.double().view(B, G, 2)
    em, er = float(((got[..., 0] - mean).abs() / var.sqrt()).max()), float(((got[..., 1] - rstd).abs() / rstd).max())
    print(f"{what}: carried {have.value}, mean err / sigma {em:.2e}, rstd rel err {er:.2e}")
    assert em < 1e-5 and er < 1e-5, (em, er)
    yref = F.silu(F.group_norm(C.float().view(B, HW, N).permute(0, 2, 1), G, gamma, beta, 1e-5)).permute(0, 2, 1)
    close(Y.view(B, HW, N), yref, TOL[dtype], TOL[dtype], what + " GroupNorm of the output")


def run_gn_bwd_case(dtype, cls, q, what):
    """input-gradient GEMM -> GroupNorm + SiLU backward (dh_dbg_gemm_groupnorm_bwd_geo): dy, and dx against autograd on the ROUNDED dy"""
    M, N, K, HW, G = q[0], q[1], q[2], q[10], q[11]
    B, g = M // HW, rng(q)
    A, lda, W, mode, geo, Z = operands(dtype, q, g)
    _, _, R, ref = plain_epilogue(dtype, q, g, Z)
    x = (randn(g, M, N) * 1.5 + randn(g, N)).to(dtype)
    gamma, beta = randn(g, N), randn(g, N)
    xd = x.double().view(B, HW, G, N // G)
    stats = torch.stack([xd.mean(dim=(1, 3)), (xd.var(dim=(1, 3), unbiased=False) + 1e-5).rsqrt()], dim=-1).float().contiguous()
    C, dx = poisoned((M, N), dtype), poisoned((M, N), dtype)
    scratch, part, have = torch.full((1 << 20,), float("nan"), device=dev()), workspace(q[16]), ctypes.c_int(-1)
    L().check(L().lib().dh_dbg_gemm_groupnorm_bwd_geo(DT[dtype], P(A), lda, P(W), M, N, K, mode, *geo, P(R), N, P(C), P(part), q[16], HW, G, P(x),
                                                      P(gamma), P(beta), P(stats), 1, P(dx), P(scratch), ctypes.byref(have),
                                                      L().stream_ptr()), "dh_dbg_gemm_groupnorm_bwd_geo")
    torch.cuda.synchronize()
    p = check_arm(cls, q)
    assert have.value == gn_carried(p), (have.value, p)
    close(C, ref, TOL[dtype], TOL[dtype], what + " dy")
    xin = x.float().view(B, HW, N).permute(0, 2, 1).clone().requires_grad_(True)
    F.silu(F.group_norm(xin, G, gamma, beta, 1e-5)).backward(C.float().view(B, HW, N).permute(0, 2, 1))
    dref = xin.grad.permute(0, 2, 1).reshape(M, N)
    assert bool(torch.isfinite(dx).all()), what + ": non-finite dx"
    err = float((dx.float() - dref).abs().max()) / float(dref.abs().max())
    print(f"{what}: carried {have.value}, dx vs autograd {err:.2e} of max |dx|")
    assert err < GN_DX_TOL[dtype], err


def lnf_inputs(dtype, q, g, bias_scale):
    """x with row means three standard deviations from zero, gamma / beta, W0 and what k_fold_ln makes of them; the f32 reference"""
    M, N, K = q[:3]
    x = (randn(g, M, K) + 3.0 * randn(g, M, 1).sign()).to(dtype)
    gamma, beta = 1.0 + 0.1 * randn(g, K), 0.1 * randn(g, K)
    W0, bias = (randn(g, N, K) / K ** 0.5).to(dtype), bias_scale * randn(g, N)
    Wf = (W0.float() * gamma).to(dtype)
    s, t = Wf.float().sum(dim=1).contiguous(), (W0.float() @ beta + bias).contiguous()
    return x, Wf.contiguous(), s, t, F.layer_norm(x.float(), (K,), gamma, beta, 1e-5) @ W0.float().t() + bias


def check_ln_stats(x, stats):
    mean, rstd = x.float().mean(dim=1), (x.float().var(dim=1, unbiased=False) + 1e-5).rsqrt()
    assert torch.allclose(stats[:, 0], mean, rtol=1e-3, atol=1e-4) and torch.allclose(stats[:, 1], rstd, rtol=2e-3, atol=0)


def run_lnf_case(dtype, cls, q, what):
    M, N, K = q[:3]
    x, Wf, s, t, ref = lnf_inputs(dtype, q, rng(q), 1.0)
    C, stats = poisoned((M, N), dtype), poisoned((M, 2), torch.float32)
    L().check(L().lib().dh_dbg_gemm_lnfold(DT[dtype], P(x), K, P(Wf), M, N, K, P(s), P(t), P(stats), 1e-5, P(C), N, L().stream_ptr()),
              "dh_dbg_gemm_lnfold")
    torch.cuda.synchronize()
    check_arm(cls, q)
    check_ln_stats(x, stats)
    close(C, ref, LNF_TOL[dtype], LNF_TOL[dtype], what)


def run_lnf_glu_case(dtype, cls, q, what):
    """LayerNorm-folded GEMM with the GEGLU forward epilogue: the pre-activations against LayerNorm -> GEMM, y against the GEGLU of the
    ROUNDED pre-activations the launch stored (the saving form; the other form against the same y)"""
    M, N, K = q[:3]
    Fd = N // 2
    x, Wf, s, t, pre_ref = lnf_inputs(dtype, q, rng(q), 0.5)
    idx = glu_paired_index(Fd).to(dev())
    Wp, sp, tp = Wf[idx].contiguous(), s[idx].contiguous(), t[idx].contiguous()
    y_ref = None
    for save in (True, False):
        pre = poisoned((M, N), dtype) if save else None
        y, stats = poisoned((M, Fd), dtype), poisoned((M, 2), torch.float32)
        L().check(L().lib().dh_dbg_gemm_lnfold_glu(DT[dtype], P(x), K, P(Wp), M, N, K, P(sp), P(tp), P(stats), 1e-5, P(pre), P(y),
                                                   L().stream_ptr()), "dh_dbg_gemm_lnfold_glu")
        torch.cuda.synchronize()
        check_arm(cls, q)
        check_ln_stats(x, stats)
        if save:
            nat = torch.empty_like(pre)
            nat[:, idx] = pre
            close(nat, pre_ref, LNF_TOL[dtype], LNF_TOL[dtype], what + " pre-activations")
            y_ref = nat[:, :Fd].float() * F.gelu(nat[:, Fd:].float())
        close(y, y_ref, 2 * TOL[dtype], 2 * TOL[dtype], what + f" y save={save}")


def run_glu_case(dtype, cls, q, what):
    """GEGLU forward epilogue (test_gemm_geglu_epilogues): y against the GEGLU of the rounded reference pre-activations"""
    M, N, K, flags = q[0], q[1], q[2], q[9]
    Fd, g = N // 2, rng(q)
    A, W = randn(g, M, K).to(dtype), (randn(g, N, K) / K ** 0.5).to(dtype)
    bias = 0.5 * randn(g, N) if flags & BIAS else None
    idx = glu_paired_index(Fd).to(dev())
    pre_ref = A.float() @ W.float().t() + (bias if bias is not None else 0.0)
    pre16 = pre_ref.to(dtype).float()
    y_ref = pre16[:, :Fd] * F.gelu(pre16[:, Fd:])
    Wp, bp = W[idx].contiguous(), bias[idx].contiguous() if bias is not None else None
    for save in (True, False):
        pre, y = poisoned((M, N), dtype) if save else None, poisoned((M, Fd), dtype)
        L().check(L().lib().dh_dbg_gemm_glu(DT[dtype], 0, P(A), K, P(Wp), M, N, K, P(bp), P(pre), P(y), P(None), P(None), L().stream_ptr()),
                  "dh_dbg_gemm_glu")
        torch.cuda.synchronize()
        check_arm(cls, q)
        close(y, y_ref, 2 * TOL[dtype], 2 * TOL[dtype], what + f" y save={save}")
        if save:
            nat = torch.empty_like(pre)
            nat[:, idx] = pre
            close(nat, pre_ref, TOL[dtype], TOL[dtype], what + " pre-activations")


def run_glu_bwd_case(dtype, cls, q, what):
    """the column-split GEGLU backward (test_column_split_geglu_backward_epilogue): columns [0, F) are dy of a GEGLU, [F, N) a plain output"""
    M, N, K, ldc, flags, Fd = q[0], q[1], q[2], q[8], q[9], q[12]
    assert 0 < Fd < N and ldc == N - Fd, q
    g = rng(q)
    A, W = randn(g, M, K).to(dtype), (randn(g, N, K) / K ** 0.5).to(dtype)
    x = randn(g, M, 2 * Fd).to(dtype)
    idx = glu_paired_index(Fd).to(dev())
    xp = x[:, idx].contiguous()
    d = A.float() @ W.float().t()
    xr = x.float().requires_grad_(True)
    gref, = torch.autograd.grad(xr[:, :Fd] * F.gelu(xr[:, Fd:]), xr, d[:, :Fd])
    accumulate = int(bool(flags & RESIDUAL))
    prior = randn(g, M, N - Fd).to(dtype)
    plain, dxp = prior.clone() if accumulate else poisoned((M, N - Fd), dtype), poisoned(xp.shape, dtype)
    L().check(L().lib().dh_dbg_gemm_glub_split(DT[dtype], P(A), K, P(W), M, N, K, Fd, P(plain), ldc, accumulate, P(xp), P(dxp), None,
                                               L().stream_ptr()), "dh_dbg_gemm_glub_split")
    torch.cuda.synchronize()
    check_arm(cls, q)
    dx = torch.empty_like(dxp)
    dx[:, idx] = dxp
    close(dx, gref, TOL[dtype], TOL[dtype], what + " d_value | d_gate")
    close(plain, d[:, Fd:] + (prior.float() if accumulate else 0.0), TOL[dtype], TOL[dtype], what + " plain columns")


def run_xattn_case(dtype, cls, q, what):
    """q projection with the cross-attention in its epilogue (test_q_projection_with_cross_attention_epilogue's fp32 gates)"""
    K, flags, Nq, Nk, H = q[2], q[9], q[13], q[14], q[15]
    lnf = bool(flags & LNF)
    assert lnf != bool(flags & BIAS), q           # (the hook: a bias, or the folded form with the bias inside ln_t)
    c = XA.make_case(dtype, images(q), Nq, H, Nk, K, lnf, seed=q[0] + K + H)
    tol, qtol = XA.ATTN_TOL[dtype], LNF_TOL[dtype]
    for save in (1, 0):
        qo, o, lse, carried = XA.run_xattn(c, save, 1)
        p = check_arm(cls, q)
        assert carried == int(p["epi"] == 3), (carried, p)
        close(o, c["o_ref"], 2 * tol, 2 * tol, what + f" o save={save}")
        close(lse, c["lse_ref"], 2e-3, 4e-3 + c["lse_q_round"], what + f" lse save={save}")
        if carried and not save:
            assert bool(torch.isnan(qo).all()), what + ": the unsaved form must not write q"
        else:
            close(qo, c["q_ref"], qtol, qtol, what + " q")


def run_xattn_dq_case(dtype, cls, q, what):
    """to_out input-gradient GEMM with the cross-attention dQ in its epilogue (test_to_out_input_gradient_with_dq_epilogue's autograd gate)"""
    K, Nq, Nk, H = q[2], q[13], q[14], q[15]
    B = images(q)
    c = XA.make_case(dtype, B, Nq, H, Nk, K, False, seed=q[0] + K + H + 1)
    M, C = c["M"], c["C"]
    qs, _, _, _ = XA.run_xattn(c, 1, 1 | 16)
    g = rng(q)
    A, W = randn(g, M, K).to(dtype), (randn(g, C, K) / K ** 0.5).to(dtype)
    qr = qs.float().requires_grad_(True)
    sp = lambda t, n: t.float().reshape(B, n, H, 64).transpose(1, 2)
    s = (sp(qr, Nq) @ sp(c["k"], Nk).transpose(-1, -2)) * 0.125
    out = (torch.softmax(s, dim=-1) @ sp(c["v"], Nk)).transpose(1, 2).reshape(M, C)
    o, lse = out.detach().to(dtype), torch.logsumexp(s.detach(), dim=-1).contiguous()
    d_o, dq, carried = XA.run_xattn_dq(c, qs, o, lse, A, W, 1)
    p = check_arm(cls, q)
    assert carried == int(p["epi"] == 4), (carried, p)
    d_ref = A.float() @ W.float().t()
    if carried:
        assert bool(torch.isnan(d_o).all()), what + ": a launch that carried dQ must not write dO"
    else:
        close(d_o, d_ref, TOL[dtype], TOL[dtype], what + " dO")
    gq, = torch.autograd.grad(out, qr, d_ref)
    tol = XA.ATTN_TOL[dtype]
    close(dq, gq, 2 * tol, 2 * tol * max(1.0, gq.abs().max().item()) * 0.2, what + " dq")


def run_ln_bwd(dtype, cls, M, N, K, part_elems, with_add, wide, what, splits=None):
    """dy = A W^T -> LayerNorm backward through dh_dbg_gemm_layernorm_bwd (the reduce of a split GEMM applies it, dy is not written)
    against autograd on the reference dy ROUNDED to the storage type (+ add), and bit for bit against the two-launch path with the
    same inputs, workspace and saved statistics: dh_dbg_gemm writing dy, then dh_dbg_layernorm's backward.  wide: x is a column
    slice of a NaN-padded tensor (ldx > N); the two-launch side gets a contiguous copy."""
    lib = L().lib()
    q = (M, N, K, 0, 0, 1, 0, 0, 0, ALIGNED | LN_BWD, 0, 0, 0, 0, 0, 0, part_elems)
    g = rng(q)
    A, W = randn(g, M, K).to(dtype), (randn(g, N, K) / K ** 0.5).to(dtype)
    ldx = N + 128 if wide else N
    xw = poisoned((M, ldx), dtype)
    x = xw[:, ldx - N - 64:ldx - 64] if wide else xw
    x.copy_((randn(g, M, N) * 1.5 - 0.3).to(dtype))
    gamma, beta = 1 + 0.1 * randn(g, N), 0.1 * randn(g, N)
    add = randn(g, M, N).to(dtype) if with_add else None
    # two launches
    dy2 = gemm(dtype, A, K, W, M, N, K, 0, (0, 0, 0, 0, 0, 1, 0), part_elems)
    rep2 = last_tile()
    y2, dx2, stats = poisoned((M, N), dtype), poisoned((M, N), dtype), poisoned((M * 2,), torch.float32)
    L().check(lib.dh_dbg_layernorm(DT[dtype], P(x.contiguous()), P(gamma), P(beta), P(y2), P(stats), P(dy2), P(add), P(dx2), M, N, 1e-5,
                                   L().stream_ptr()), "dh_dbg_layernorm")
    torch.cuda.synchronize()
    # one
    dy1, dx1, part, done = poisoned((M, N), dtype), poisoned((M, N), dtype), workspace(part_elems), ctypes.c_int(-1)
    L().check(lib.dh_dbg_gemm_layernorm_bwd(DT[dtype], P(A), K, P(W), M, N, K, P(x), ldx, P(gamma), P(stats), P(add), P(dy1), P(dx1), P(part),
                                            part_elems, ctypes.byref(done), L().stream_ptr()), "dh_dbg_gemm_layernorm_bwd")
    torch.cuda.synchronize()
    p = check_arm(cls, q)
    assert done.value == int(p["reduce"] == 4), (done.value, p)
    assert splits is None or (p["splits"], p["reduce"]) == (splits, 4), p
    assert rep2[:7] == last_tile()[:7], "the two-launch GEMM ran another tile or split"
    if done.value:
        assert bool(torch.isnan(dy1).all()), what + ": the reduce that applies the LayerNorm backward must not write dy"
    else:
        assert torch.equal(dy1, dy2)
    xr = x.float().requires_grad_(True)
    gref, = torch.autograd.grad(F.layer_norm(xr, (N,), gamma, beta, 1e-5), xr, (A.float() @ W.float().t()).to(dtype).float())
    close(dx1, gref + (add.float() if with_add else 0.0), TOL[dtype], TOL[dtype], what)
    same = torch.equal(dx1, dx2)
    if not same:
        diff = (dx1.float() - dx2.float()).abs()
        print(f"{what}: {int((diff > 0).sum())} of {diff.numel()} elements differ from the two-launch path, max {diff.max().item():.3g}")
    assert same, what + ": differs from split GEMM + LayerNorm backward"


def run_ln_bwd_case(dtype, cls, q, what):
    assert q[3] == 0 and q[9] == ALIGNED | LN_BWD, q
    run_ln_bwd(dtype, cls, q[0], q[1], q[2], q[16], True, False, what)


RUN = {"gemm": run_gemm_case, "gn": run_gn_case, "gn_bwd": run_gn_bwd_case, "lnf": run_lnf_case, "lnf_glu": run_lnf_glu_case,
       "glu": run_glu_case, "glu_bwd": run_glu_bwd_case, "xattn": run_xattn_case, "xattn_dq": run_xattn_dq_case, "ln_bwd": run_ln_bwd_case}


def case_id(i):
    q = CLASS_CASES[i][1]
    return f"{i:02d}-{kind_of(q[9])}-{q[0]}x{q[1]}x{q[2]}"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("i", range(len(CLASS_CASES)), ids=case_id)
def test_launch_class_parity(dtype, i):
    """one launch of the class: the arm that ran, then parity with the torch reference of its op"""
    cls, q = CLASS_CASES[i]
    kind = kind_of(q[9])
    RUN[kind](dtype, cls, q, f"{kind} class {i} {q[0]}x{q[1]}x{q[2]} {dtype}")


# k_splitk_reduce_ln_bwd: (rows, N, K, splits, add, ldx > N).  N = 320 / 640 / 1280: one / two / three 8-element chunks per lane; rows <=
# 1024: one wave per block, 1100: four with a ragged last block; splits 3: the remainder loop alone, 4: the four-at-a-time body alone,
# 5 / 6 / 10: both, 12: three bodies, 2: the policy's own choice for 1100 x 1280.  The workspace holds exactly `splits` slabs: where the
# policy would cut K further the workspace is what limits it (the plan of the query, asserted), and a slab past it would be a fault.
LN_REDUCE_CASES = [
    (64, 320, 2048, 3, True, False),
    (64, 640, 2048, 4, False, True),
    (64, 1280, 2048, 6, True, True),
    (64, 1280, 3072, 12, False, False),
    (64, 320, 2560, 10, False, True),
    (1100, 320, 2048, 3, True, True),
    (1100, 640, 2048, 4, False, False),
    (1100, 640, 2048, 5, True, False),
    (1100, 320, 2048, 5, False, False),
    (1100, 1280, 2048, 2, False, True),
]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows,N,K,splits,with_add,wide", LN_REDUCE_CASES)
def test_splitk_reduce_layernorm_backward_paths(dtype, rows, N, K, splits, with_add, wide):
    run_ln_bwd(dtype, None, rows, N, K, splits * rows * N, with_add, wide,
               f"ln_bwd reduce {rows}x{N}x{K} splits={splits} add={with_add} wide={wide} {dtype}", splits=splits)
