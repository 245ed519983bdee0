"""The 77-key cross-attention in the epilogue of its q projection (gemm.hip EPI_XATTN, GemmArgs::xa_o): a dense, unsplit
64-column k_gemm_dma tile is q of one head for 64 / 128 queries of one image, and its epilogue runs that head's attention instead
of a k_attn_fwd launch behind it.  Through dh_dbg_gemm_xattn (the real dispatch; it reports whether the launch carried the
attention) against a torch fp32 reference of LayerNorm -> q -> softmax(q K^T / 8) V, against the same build with the form switched
off (dh_dbg_gemm_stage bit 4 = value 16: two launches), and through the engine with the form on and off.  The backward twin
(EPI_XATTN_DQ, GemmArgs::xa_dq; stage bit 5 = value 32) turns the dO tile of the attn2.to_out.0 input-gradient GEMM into dq the same
way when no text gradient is wanted."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = {torch.float16: 0, torch.bfloat16: 1}
ATTN_TOL = {torch.float16: 5e-3, torch.bfloat16: 3e-2}      # tests/test_unet_kernels_gpu.py::test_attention_forward_backward
XA_KEYS = 96                                                # gemm_k.h: the key rows the epilogue stages


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def L():
    from diffusionhandles_amd import _lib
    return _lib


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def poisoned(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev())


def close(got, ref, rtol, atol, what, frac=1e-4, ceiling=8.0):
    """The rule of tests/test_unet_kernels_gpu.py close(): every element finite, at most `frac` of them over atol + rtol |ref|,
    none over `ceiling` times that.  Returns the worst ratio."""
    g, r = got.float(), ref.float()
    assert tuple(g.shape) == tuple(r.shape), what
    assert bool(torch.isfinite(g).all()), f"{what}: {int((~torch.isfinite(g)).sum())} non-finite elements"
    ratio = (g - r).abs() / (atol + rtol * r.abs())
    worst = int(ratio.argmax())
    wr = ratio.reshape(-1)[worst].item()
    msg = (f"{what}: worst element {worst} got {g.reshape(-1)[worst].item():.6g} ref {r.reshape(-1)[worst].item():.6g} "
           f"({wr:.3g} x tolerance)")
    assert wr <= ceiling, msg
    assert (ratio > 1.0).float().mean().item() <= frac, msg
    return wr


def rel(got, ref):
    return ((got.float() - ref.float()).norm() / (ref.float().norm() + 1e-12)).item()


def make_case(dtype, B, Nq, H, Nk, K, lnf, seed):
    """Inputs of one q projection + cross-attention and its fp32 reference.  K | V sit in one tensor with a row stride larger
    than 2 C and a column offset, as the engine's hoisted text projection does."""
    g = torch.Generator(device=dev()).manual_seed(seed)
    M, C = B * Nq, 64 * H
    x = torch.randn(M, K, generator=g, device=dev()).to(dtype)
    W0 = (torch.randn(C, K, generator=g, device=dev()) / K ** 0.5).to(dtype)
    bias = 0.2 * torch.randn(C, generator=g, device=dev())
    col, ld = 64, 2 * C + 192
    kv = torch.randn(B * Nk, ld, generator=g, device=dev()).to(dtype)
    k, v = kv[:, col:col + C], kv[:, col + C:col + 2 * C]
    c = dict(dtype=dtype, B=B, Nq=Nq, H=H, Nk=Nk, K=K, M=M, C=C, x=x, kv=kv, k=k, v=v, ld=ld, bias=bias, lnf=lnf)
    if lnf:
        gamma = 1.0 + 0.1 * torch.randn(K, generator=g, device=dev())
        beta = 0.1 * torch.randn(K, generator=g, device=dev())
        Wf = (W0.float() * gamma).to(dtype).contiguous()
        c.update(W=Wf, s=Wf.float().sum(dim=1).contiguous(), t=(W0.float() @ beta + bias).contiguous())
        q = F.layer_norm(x.float(), (K,), gamma, beta, 1e-5) @ W0.float().t() + bias
    else:
        c.update(W=W0.contiguous())
        q = x.float() @ W0.float().t() + bias
    sp = lambda t, n: t.float().reshape(B, n, H, 64).transpose(1, 2)
    s = (sp(q, Nq) @ sp(k, Nk).transpose(-1, -2)) * 0.125
    c["q_ref"] = q
    # What rounding q to 16 bits (unit roundoff u = 2^-11 fp16 / 2^-8 bf16) can move a score, hence lse, by: |d s_k| <=
    # 0.125 u sum_d |q_d| |k_d|; the fp32 reference keeps q unrounded, the kernels (fused or not) store and multiply the rounded one
    u = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    c["lse_q_round"] = 0.125 * u * (sp(q, Nq).abs() @ sp(k, Nk).abs().transpose(-1, -2)).amax(dim=-1)
    c["o_ref"] = (torch.softmax(s, dim=-1) @ sp(v, Nk)).transpose(1, 2).reshape(M, C)
    c["lse_ref"] = torch.logsumexp(s, dim=-1)
    return c


def run_xattn(c, save, stage):
    """dh_dbg_gemm_xattn with dh_dbg_gemm_stage(stage); returns (q, o, lse, carried), every output pre-poisoned."""
    lib, dtype = L().lib(), c["dtype"]
    q, o = poisoned((c["M"], c["C"]), dtype), poisoned((c["M"], c["C"]), dtype)
    lse = poisoned((c["B"], c["H"], c["Nq"]), torch.float32)
    stats = poisoned((c["M"], 2), torch.float32)
    carried = ctypes.c_int(-1)
    try:
        L().check(lib.dh_dbg_gemm_stage(stage), "dh_dbg_gemm_stage")
        rc = lib.dh_dbg_gemm_xattn(DT[dtype], P(c["x"]), c["K"], P(c["W"]), c["M"], c["C"], c["K"], None if c["lnf"] else P(c["bias"]),
                                   P(c["s"]) if c["lnf"] else None, P(c["t"]) if c["lnf"] else None, P(stats) if c["lnf"] else None,
                                   1e-5, P(q), P(c["k"]), P(c["v"]), c["ld"], P(o), P(lse), c["B"], c["Nk"], save, ctypes.byref(carried),
                                   L().stream_ptr())
        L().check(rc, "dh_dbg_gemm_xattn")
        torch.cuda.synchronize()
    finally:
        lib.dh_dbg_gemm_stage(1)
    return q, o, lse, carried.value


# (B, Nq, heads, Nk, K, carried)
CASES = [
    (1, 64, 1, 77, 128, 1),            # one tile, one head
    (1, 200, 2, 77, 128, 1),           # one image, tail rows in the last tile
    (2, 128, 2, 77, 128, 1),           # two images with different text: every tile uses its own image's K / V
    (2, 80, 2, 77, 128, 0),            # a 64-row tile would span two images: not fused, still right
    (1, 64, 1, 1, 64, 1),              # a single key
    (1, 64, 1, XA_KEYS, 64, 1),        # the padded maximum
    (1, 64, 1, XA_KEYS + 1, 64, 0),    # one key more: the attention kernel runs
    # the 128x64 tiles (the dispatch takes them from 128 row tiles of a 64-column GEMM): five-stage ring, two K groups, and the
    # three-stage ring of grids of 257..512 workgroups; ragged last tile
    (1, 16384, 1, 77, 64, 1),
    (1, 16300, 1, 77, 256, 1),
    (1, 32900, 1, 77, 64, 1),
]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("lnf", [True, False])
@pytest.mark.parametrize("B,Nq,H,Nk,K,expect", CASES)
def test_q_projection_with_cross_attention_epilogue(dtype, lnf, B, Nq, H, Nk, K, expect):
    """Forward: o and lse of the fused launch against fp32 (twice the attention tolerance: q is rounded to 16 bits on the way, as
    it is between the two kernels of the unfused path; lse: twice test_attention_forward_backward's lse tolerance plus the bound
    on what that rounding of q moves a score by, make_case) and against the two-launch path of the same build (the single
    attention tolerance); q is written only in the saved form and is then the unfused GEMM's output bit for bit."""
    c = make_case(dtype, B, Nq, H, Nk, K, lnf, seed=B * 1000 + Nq + H + Nk + K)
    tol = ATTN_TOL[dtype]
    what = f"xattn {dtype} lnf={lnf} B={B} Nq={Nq} H={H} Nk={Nk} K={K}"
    q0, o0, lse0, carried0 = run_xattn(c, 1, 1 | 16)
    assert carried0 == 0, what + ": stage bit 16 must switch the form off"
    for save in (1, 0):
        q, o, lse, carried = run_xattn(c, save, 1)
        assert carried == expect, f"{what}: carried {carried}, expected {expect}"
        r_o = close(o, c["o_ref"], 2 * tol, 2 * tol, what + f" save={save} o vs fp32")
        r_l = close(lse, c["lse_ref"], 2e-3, 4e-3 + c["lse_q_round"], what + f" save={save} lse vs fp32")
        p_o = close(o, o0, tol, tol, what + f" save={save} o vs two launches")
        p_l = close(lse, lse0, 1e-3, 2e-3, what + f" save={save} lse vs two launches")
        print(f"{what} save={save} carried={carried}: worst ratio vs fp32 o {r_o:.3f} lse {r_l:.3f}; vs two launches o {p_o:.3f} lse {p_l:.3f}")
        if carried and not save:
            assert bool(torch.isnan(q).all()), what + ": the unsaved form must not write q"
        else:
            assert torch.equal(q, q0), what + ": q differs from the unfused GEMM's output"
    qtol = 6e-3 if dtype == torch.float16 else 3e-2      # (the LayerNorm-folded GEMM's tolerance, test_gemm_layernorm_fold)
    close(q0, c["q_ref"], qtol, qtol, what + " q vs fp32")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_unfused_backward_consumes_a_fused_forward(dtype):
    """o and lse of a fused forward fed to the attention backward kernels (dh_dbg_attention_bwd_pair: dQ + dK/dV) against torch
    autograd of the same q, K, V at the backward tolerance of test_attention_forward_backward."""
    B, Nq, H, Nk, K = 2, 128, 2, 77, 128
    c = make_case(dtype, B, Nq, H, Nk, K, True, seed=77)
    q, o, lse, carried = run_xattn(c, 1, 1)
    assert carried == 1
    C = c["C"]
    g = torch.Generator(device=dev()).manual_seed(5)
    do = torch.randn(B * Nq, C, generator=g, device=dev()).to(dtype)
    kk, vv = c["k"].contiguous(), c["v"].contiguous()
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, kk, vv))
    sp = lambda t, n: t.reshape(B, n, H, 64).transpose(1, 2)
    s = (sp(qr, Nq) @ sp(kr, Nk).transpose(-1, -2)) * 0.125
    ref = (torch.softmax(s, dim=-1) @ sp(vr, Nk)).transpose(1, 2).reshape(B * Nq, C)
    gq, gk, gv = torch.autograd.grad(ref, (qr, kr, vr), do.float())
    dq, dk, dv = poisoned(q.shape, dtype), poisoned(kk.shape, dtype), poisoned(vv.shape, dtype)
    delta = poisoned((B, H, Nq), torch.float32)
    lib = L().lib()
    L().check(lib.dh_dbg_attention_bwd_pair(DT[dtype], P(q), C, P(kk), P(vv), C, P(o), C, P(lse), P(do), P(delta), P(dq), P(dk), P(dv),
                                            B, H, Nq, Nk, L().stream_ptr(), None), "dh_dbg_attention_bwd_pair")
    torch.cuda.synchronize()
    tol = ATTN_TOL[dtype]
    for got, r, nm in ((dq, gq, "dq"), (dk, gk, "dk"), (dv, gv, "dv")):
        close(got, r, 2 * tol, 2 * tol * max(1.0, r.abs().max().item()) * 0.2, f"fused forward -> unfused backward {dtype} {nm}")


def run_xattn_dq(c, q, o, lse, A, W, stage):
    """dh_dbg_gemm_xattn_dq with dh_dbg_gemm_stage(stage): dO = A W^T and dq of the cross-attention; returns (d_o, dq, carried)."""
    lib, dtype = L().lib(), c["dtype"]
    d_o, dq = poisoned((c["M"], c["C"]), dtype), poisoned((c["M"], c["C"]), dtype)
    carried = ctypes.c_int(-1)
    try:
        L().check(lib.dh_dbg_gemm_stage(stage), "dh_dbg_gemm_stage")
        rc = lib.dh_dbg_gemm_xattn_dq(DT[dtype], P(A), A.shape[1], P(W), c["M"], c["C"], A.shape[1], P(d_o), P(q), P(c["k"]), P(c["v"]), c["ld"],
                                      P(o), P(lse), P(dq), c["B"], c["Nk"], ctypes.byref(carried), L().stream_ptr())
        L().check(rc, "dh_dbg_gemm_xattn_dq")
        torch.cuda.synchronize()
    finally:
        lib.dh_dbg_gemm_stage(1)
    return d_o, dq, carried.value


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,Nq,H,Nk,K,expect", CASES)
def test_to_out_input_gradient_with_dq_epilogue(dtype, B, Nq, H, Nk, K, expect):
    """Backward to q: dO = A W^T in the GEMM, dq from its epilogue, against torch autograd of the attention (twice the attention
    tolerance, gradients scaled as in test_attention_forward_backward) and against the two-launch path of the same build -- the
    unfused GEMM's dO fed to k_attn_bwd_dq (the single tolerance).  dO is not written by a launch that carried the attention.
    The saved q is the two-launch forward's; the saved o and lse are the fp32 attention of that stored q, o rounded to the storage
    type, so that the gradient under test and the autograd reference differentiate the same function at the same point.  (With
    the o of k_attn_fwd instead, the single-key case misses the autograd gate at fp16 -- worst element 1.85 x tolerance, 0.34 % of
    the elements over it, fused and unfused alike: that kernel then rounded P toward zero, so its o was V (1 - 2^-11) wherever
    exp2 returns a hair under one, delta = rowsum(dO o) no longer cancelled dP, and the exact gradient there is zero.  pack8 has
    rounded to nearest since DESIGN.md 8c; the saved o stays the reference's, which keeps this a test of the gradient alone.)"""
    c = make_case(dtype, B, Nq, H, Nk, K, False, seed=B * 1000 + Nq + H + Nk + K + 1)
    M, C = c["M"], c["C"]
    q, _, _, _ = run_xattn(c, 1, 1 | 16)
    g = torch.Generator(device=dev()).manual_seed(Nq + Nk)
    A = torch.randn(M, K, generator=g, device=dev()).to(dtype)
    W = (torch.randn(C, K, generator=g, device=dev()) / K ** 0.5).to(dtype)
    what = f"xattn dq {dtype} B={B} Nq={Nq} H={H} Nk={Nk} K={K}"
    qr = q.float().requires_grad_(True)
    sp = lambda t, n: t.float().reshape(B, n, H, 64).transpose(1, 2)
    s = (sp(qr, Nq) @ sp(c["k"], Nk).transpose(-1, -2)) * 0.125
    out = (torch.softmax(s, dim=-1) @ sp(c["v"], Nk)).transpose(1, 2).reshape(M, C)
    o, lse = out.detach().to(dtype), torch.logsumexp(s.detach(), dim=-1).contiguous()
    do0, dq0, carried0 = run_xattn_dq(c, q, o, lse, A, W, 1 | 32)
    assert carried0 == 0, what + ": stage bit 32 must switch the form off"
    do1, dq1, carried = run_xattn_dq(c, q, o, lse, A, W, 1)
    assert carried == expect, f"{what}: carried {carried}, expected {expect}"
    if carried:
        assert bool(torch.isnan(do1).all()), what + ": a launch that carried dQ must not write dO"
    else:
        assert torch.equal(do1, do0)
    gq, = torch.autograd.grad(out, qr, A.float() @ W.float().t())       # (the fp32 dO: the kernels round it to 16 bits)
    tol = ATTN_TOL[dtype]
    scale = max(1.0, gq.abs().max().item()) * 0.2
    r_a = close(dq1, gq, 2 * tol, 2 * tol * scale, what + " dq vs autograd")
    r_p = close(dq1, dq0, tol, tol * scale, what + " dq vs two launches")
    print(f"{what} carried={carried}: worst ratio dq vs autograd {r_a:.3f}, vs two launches {r_p:.3f}")



# engine against its oracle, tests/test_unet_engine_gpu.py: (forward, backward) rel-L2 gates of the TINY network
ENGINE_TOL = {torch.float16: (1e-2, 3e-2), torch.bfloat16: (5e-2, 1.5e-1)}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 2])
def test_engine_with_the_form_on_and_off(dtype, B):
    """TINY U-Net, forward + backward to the latent with both epilogue forms on (shipped) and off (stage bits 16 | 32): eps, the
    captured activations and the latent gradient agree within the engine's gates against its oracle, and so does the text gradient
    of a backward with need_text.  With only the forward form off (bit 16) that text gradient is bit-identical to the all-off run:
    a backward that wants the text gradient keeps the two attention kernels.  The dispatch reports carried launches while the
    forms are on and none while they are off."""
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd.unet import HipUNet
    from oracle import unet_torch as U
    cfg = U.TINY
    lib = _lib.lib()
    ref = U.init_synthetic_(U.UNetTorch(cfg), seed=3).to(dev()).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.to(dtype).float())
    g = torch.Generator(device=dev()).manual_seed(31)
    S = cfg["sample_size"]
    sample = torch.randn(B, S, S, cfg["in_channels"], generator=g, device=dev())
    text = torch.randn(B, 77, cfg["cross_attention_dim"], generator=g, device=dev())
    d_act = [None, None, (torch.randn(B, S, S, cfg["block_out_channels"][0], generator=g, device=dev()) * 0.05).to(dtype)]
    outs, carried = {}, {}
    total = ctypes.c_longlong(0)
    try:
        for name, stage in (("on", 1), ("fwd_off", 1 | 16), ("off", 1 | 16 | 32)):
            _lib.check(lib.dh_dbg_gemm_stage(stage), "dh_dbg_gemm_stage")
            hip = HipUNet(dict(cfg, text_len=77), dtype=dtype, max_batch=B)
            hip.load_state_dict(ref.state_dict())
            _lib.check(lib.dh_dbg_gemm_xattn_carried(None, ctypes.byref(total)), "dh_dbg_gemm_xattn_carried")
            before = total.value
            eps, acts = hip.forward(sample, 500.0, text, save_for_backward=True)
            d_sample, _ = hip.backward(d_act, None, True, False)
            res = [eps.clone(), *[a.clone() for a in acts], d_sample.clone()]
            hip.forward(sample, 500.0, text, save_for_backward=True)
            _, d_text = hip.backward(d_act, None, True, True)
            res.append(d_text.clone())
            torch.cuda.synchronize()
            _lib.check(lib.dh_dbg_gemm_xattn_carried(None, ctypes.byref(total)), "dh_dbg_gemm_xattn_carried")
            carried[name] = total.value - before
            outs[name] = res
            del hip
    finally:
        lib.dh_dbg_gemm_stage(1)
    assert carried["on"] >= 2 and carried["on"] > carried["fwd_off"] >= 1 and carried["off"] == 0, carried
    assert torch.equal(outs["fwd_off"][5], outs["off"][5]), "text gradient with the forward form off differs from the unfused path"
    tol_f, tol_b = ENGINE_TOL[dtype]
    names = ["eps", "act0", "act1", "act2", "d_sample", "d_text"]
    errs = {n: rel(a, b2) for n, a, b2 in zip(names, outs["on"], outs["off"])}
    print(f"engine {dtype} B={B}: carried launches {carried}, rel-L2 form on vs off {errs}")
    for n, e in errs.items():
        gate = tol_f if n in ("eps", "act0", "act1", "act2") else tol_b
        assert e < gate, f"{n}: rel-L2 {e:.3e} >= gate {gate:.1e} ({errs})"
