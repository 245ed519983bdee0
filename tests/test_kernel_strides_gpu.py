"""The kernels in the forms the engine calls them (csrc/unet_engine.cpp), not only with packed leading dimensions:

- GEMM output into a column slice of a wider tensor (g.C = gradient + in_col, ldc = the tensor's width), dense and 3x3 conv;
- GEMM A operand read from a column slice (g.A = activation + in_col, lda = the tensor's width);
- gradient accumulation in place (g.R = g.C, ldr = ldc), split K and not;
- self-attention on views of the fused q | k | v tensor (ldq = ldk = 3C, k = qkv + C, v = qkv + 2C) with dq | dk | dv written
  into the fused gradient at the same offsets, cross-attention on a k | v pair inside the wide text-KV tensor (ldk = its width);
- the sequential form of dh_dbg_attention_bwd_pair (stream2 = NULL).

Each case compares with a plain fp32 torch reference of the same op, and the written view lies inside a larger buffer of random
sentinel values (the view itself starts as NaN): every element outside the view -- columns left and right of it, rows after the
last -- must be bit-unchanged afterwards, and every input buffer too.  Families: 1 = k_gemm_dma, 2 = k_gemm_pp (where the
shape is one k_gemm_pp carries; otherwise the launch stays on k_gemm_dma)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_unet_kernels_gpu import DT, L, P, close, dev, poisoned, run_gemm

pytestmark = pytest.mark.gpu

PAD_ROWS = 256          # sentinel rows after the last written row: one tile of the tallest GEMM tile


@pytest.fixture()
def family():
    lib = L().lib()

    def set_family(f):
        L().check(lib.dh_dbg_gemm_family(f), "dh_dbg_gemm_family")
    yield set_family
    lib.dh_dbg_gemm_family(0)


def at(t, elems):
    """pointer `elems` elements past the start of t (a column offset into a fused tensor)"""
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size())


def framed(rows, width, col, ncols, dtype, g, pad_rows=PAD_ROWS):
    """[rows + pad_rows][width] of random sentinel values; the view [:rows, col:col + ncols] is NaN.  -> (buffer, view, mask of
    the view)"""
    buf = torch.randn(rows + pad_rows, width, generator=g, device=dev()).to(dtype)
    buf[:rows, col:col + ncols] = float("nan")
    mask = torch.zeros(buf.shape, dtype=torch.bool, device=dev())
    mask[:rows, col:col + ncols] = True
    return buf, buf[:rows, col:col + ncols], mask


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def unchanged_outside(buf, before, mask, what):
    diff = (bits(buf) != bits(before)) & ~mask
    n = int(diff.sum())
    if n:
        first = tuple(int(i) for i in diff.nonzero()[0])
        raise AssertionError(f"{what}: {n} elements outside the written view changed, first at {first} "
                             f"({before[first].item():.6g} -> {buf[first].item():.6g})")


def unchanged(t, before, what):
    unchanged_outside(t, before, torch.zeros(t.shape, dtype=torch.bool, device=dev()), what)


def gemm_tol(dtype):
    return 4e-3 if dtype == torch.float16 else 2.5e-2


def operands(dtype, M, N, K, seed):
    g = torch.Generator(device=dev()).manual_seed(seed)
    A = torch.randn(M, K, generator=g, device=dev()).to(dtype)
    W = (torch.randn(N, K, generator=g, device=dev()) / K ** 0.5).to(dtype)
    bias = torch.randn(N, generator=g, device=dev())
    return g, A, W, bias


# (M, N, K, width, col): the engine's widths (q | k | v = 960 at the 64x64-latent level, 1280 = two 640-channel tensors
# concatenated, 2560 = two 1280-channel ones); ragged M; K = 2560 / 4096 to reach split K on both families
SLICE_SHAPES = [(1, 320, 320, 960, 320), (63, 320, 320, 960, 320), (65, 640, 640, 1280, 640), (1100, 320, 320, 960, 320),
                (1100, 640, 2560, 1280, 640), (4096, 320, 320, 960, 320), (4096, 640, 640, 1280, 640), (2048, 1280, 4096, 2560, 1280)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("fam", [1, 2])
@pytest.mark.parametrize("M,N,K,width,col", SLICE_SHAPES)
def test_gemm_output_into_column_slice(family, fam, dtype, M, N, K, width, col):
    g, A, W, bias = operands(dtype, M, N, K, M + N + K)
    R = torch.randn(M, N, generator=g, device=dev()).to(dtype)
    ref = A.float() @ W.float().t() + bias + R.float()
    family(fam)
    for split in (True, False):
        buf, C, mask = framed(M, width, col, N, dtype, g)
        before = buf.clone()
        run_gemm(dtype, A, K, W, M, N, K, bias=bias, R=R, split=split, C=C, ldc=width)
        close(C, ref, gemm_tol(dtype), gemm_tol(dtype), f"gemm {M}x{N}x{K} into cols {col}:{col + N} of {width} split={split}")
        unchanged_outside(buf, before, mask, f"gemm {M}x{N}x{K} into cols {col}:{col + N} of {width} split={split}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("fam", [1, 2])
@pytest.mark.parametrize("M,N,K,width,col", [(63, 320, 320, 960, 320), (1100, 640, 640, 1280, 640), (4096, 320, 320, 960, 640),
                                             (1024, 1280, 2560, 3840, 1280)])
def test_gemm_a_from_column_slice(family, fam, dtype, M, N, K, width, col):
    g = torch.Generator(device=dev()).manual_seed(M + N + K + col)
    Abuf = torch.randn(M, width, generator=g, device=dev()).to(dtype)
    A = Abuf[:, col:col + K]
    W = (torch.randn(N, K, generator=g, device=dev()) / K ** 0.5).to(dtype)
    bias = torch.randn(N, generator=g, device=dev())
    ref = A.float() @ W.float().t() + bias
    a_before = Abuf.clone()
    family(fam)
    for split in (True, False):
        C = run_gemm(dtype, A, width, W, M, N, K, bias=bias, split=split)
        close(C, ref, gemm_tol(dtype), gemm_tol(dtype), f"gemm A = cols {col}:{col + K} of {width}, {M}x{N}x{K} split={split}")
    unchanged(Abuf, a_before, "A operand")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("fam", [1, 2])
@pytest.mark.parametrize("M,N,K,width,col", [(63, 320, 320, 960, 320), (1100, 640, 2560, 1280, 640), (4096, 320, 320, 960, 320),
                                             (2048, 1280, 4096, 2560, 1280)])
def test_gemm_accumulates_in_place(family, fam, dtype, M, N, K, width, col):
    """C += A W^T + bias with R = C, ldr = ldc inside a column slice: the engine's gradient accumulation (unet_engine.cpp, the
    input-gradient GEMMs when the gradient already holds a contribution)."""
    g, A, W, bias = operands(dtype, M, N, K, M + N + K + 1)
    family(fam)
    for split in (True, False):
        buf, C, mask = framed(M, width, col, N, dtype, g)
        C.copy_(torch.randn(M, N, generator=g, device=dev()).to(dtype))
        ref = A.float() @ W.float().t() + bias + C.float()
        before = buf.clone()
        run_gemm(dtype, A, K, W, M, N, K, bias=bias, R=C, ldr=width, split=split, C=C, ldc=width)
        close(C, ref, gemm_tol(dtype), gemm_tol(dtype), f"gemm in place {M}x{N}x{K} cols {col}:{col + N} of {width} split={split}")
        unchanged_outside(buf, before, mask, f"gemm in place {M}x{N}x{K} split={split}")


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("fam", [1, 2])
@pytest.mark.parametrize("B,Cin,Cout,H,stride,up", [(1, 320, 320, 64, 1, 0), (2, 640, 320, 32, 1, 0), (1, 320, 320, 64, 2, 0),
                                                     (1, 1280, 1280, 8, 1, 1), (2, 64, 128, 16, 1, 0), (8, 320, 640, 32, 1, 0)])
def test_conv3_output_into_column_slice(family, fam, dtype, B, Cin, Cout, H, stride, up):
    """3x3 convolution (stride 1, stride 2, nearest-2x source) written into the middle third of a [M][3 Cout] tensor."""
    g = torch.Generator(device=dev()).manual_seed(Cin + Cout + H + stride + up + 3)
    x = torch.randn(B, Cin, H, H, generator=g, device=dev()).to(dtype)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g, device=dev()) / (9 * Cin) ** 0.5).to(dtype)
    bias = torch.randn(Cout, generator=g, device=dev())
    xin = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if up else x.float()
    ref = F.conv2d(xin, w.float(), bias, stride=stride, padding=1)
    Ho = ref.shape[-1]
    M, width, col = B * Ho * Ho, 3 * Cout, Cout
    ref = nhwc(ref).reshape(M, Cout)
    wf = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous()
    xa = nhwc(x)
    x_before = xa.clone()
    family(fam)
    for split in (True, False):
        buf, C, mask = framed(M, width, col, Cout, dtype, g)
        before = buf.clone()
        run_gemm(dtype, xa, Cin, wf, M, Cout, 9 * Cin, mode=1, geo=(H, H, Cin, Ho, Ho, stride, up), bias=bias, split=split, C=C,
                 ldc=width)
        what = f"conv {B}x{Cin}->{Cout} {H}^2 s{stride} up{up} into cols {col}:{col + Cout} of {width} split={split}"
        close(C, ref, gemm_tol(dtype), gemm_tol(dtype), what)
        unchanged_outside(buf, before, mask, what)
    unchanged(xa, x_before, "conv source")


def attn_ref(q, k, v, do, H):
    """fp32 attention of [B][N][H*64] views (scale 1/8) -> o, lse [B][H][Nq], dq, dk, dv"""
    B, Nq, C = q.shape
    Nk = k.shape[1]
    qr, kr, vr = (t.float().contiguous().requires_grad_(True) for t in (q, k, v))
    sp = lambda t, n: t.view(B, n, H, 64).transpose(1, 2)
    s = (sp(qr, Nq) @ sp(kr, Nk).transpose(-1, -2)) * 0.125
    o = (torch.softmax(s, dim=-1) @ sp(vr, Nk)).transpose(1, 2).reshape(B, Nq, C)
    gq, gk, gv = torch.autograd.grad(o, (qr, kr, vr), do.float())
    return o.detach(), torch.logsumexp(s, dim=-1).detach(), gq, gk, gv


def attn_tol(dtype):
    return 5e-3 if dtype == torch.float16 else 3e-2


def check_grads(dtype, got, refs, what):
    tol = attn_tol(dtype)
    for gt, r, nm in zip(got, refs, ("dq", "dk", "dv")):
        close(gt, r, 2 * tol, 2 * tol * max(1.0, r.abs().max().item()) * 0.2, f"{what} {nm}")


def fused_qkv(dtype, B, H, N, g):
    """q | k | v in one [B * N + pad][3C] buffer (one spiked key forces a running-max jump); do packed [B][N][C]"""
    C = H * 64
    qkv = torch.randn(B * N + 64, 3 * C, generator=g, device=dev()).to(dtype)
    v3 = qkv[:B * N].view(B, N, 3 * C)
    v3[:, N // 2, C:2 * C] *= 6.0
    do = torch.randn(B, N, C, generator=g, device=dev()).to(dtype)
    return qkv, v3[..., :C], v3[..., C:2 * C], v3[..., 2 * C:], do


SELF_SHAPES = [(2, 5, 64), (1, 10, 1000), (1, 20, 1100), (1, 5, 4096)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,H,N", SELF_SHAPES)
def test_self_attention_on_fused_qkv(dtype, B, H, N):
    g = torch.Generator(device=dev()).manual_seed(N + H + 17)
    C = H * 64
    qkv, q, k, v, do = fused_qkv(dtype, B, H, N, g)
    o_ref, lse_ref, *grads = attn_ref(q, k, v, do, H)
    qkv_before = qkv.clone()
    dqkv, _, mask = framed(B * N, 3 * C, 0, 3 * C, dtype, g, pad_rows=64)
    before = dqkv.clone()
    o = poisoned((B, N, C), dtype); lse = poisoned((B, H, N), torch.float32); delta = poisoned((B, H, N), torch.float32)
    L().check(L().lib().dh_dbg_attention(DT[dtype], P(qkv), 3 * C, at(qkv, C), at(qkv, 2 * C), 3 * C, P(o), C, P(lse), P(do), P(delta),
                                         P(dqkv), at(dqkv, C), at(dqkv, 2 * C), B, H, N, N, L().stream_ptr()), "dh_dbg_attention")
    what = f"fused-qkv attention B={B} H={H} N={N}"
    tol = attn_tol(dtype)
    close(o, o_ref, tol, tol, what + " o")
    close(lse, lse_ref, 1e-3, 2e-3, what + " lse")
    d3 = dqkv[:B * N].view(B, N, 3 * C)
    check_grads(dtype, (d3[..., :C], d3[..., C:2 * C], d3[..., 2 * C:]), grads, what)
    unchanged_outside(dqkv, before, mask, what + " dqkv")
    unchanged(qkv, qkv_before, what + " qkv")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,H,Nq", [(2, 5, 1024), (1, 10, 1100), (1, 20, 64), (1, 5, 4096)])
def test_cross_attention_on_fused_kv(dtype, B, H, Nq):
    """k | v at column C of a [B * 77][4C] text-KV tensor (the engine keeps the k | v pairs of all cross-attention layers side
    by side in one tensor: kv = text_kv + kv_col, ldk = its width); dk | dv into the same place of its gradient."""
    g = torch.Generator(device=dev()).manual_seed(Nq + H + 29)
    C, Nk = H * 64, 77
    width, col = 4 * C, C
    kvbuf = torch.randn(B * Nk + 64, width, generator=g, device=dev()).to(dtype)
    kv3 = kvbuf[:B * Nk].view(B, Nk, width)
    kv3[:, Nk // 2, col:col + C] *= 6.0
    k, v = kv3[..., col:col + C], kv3[..., col + C:col + 2 * C]
    q = torch.randn(B, Nq, C, generator=g, device=dev()).to(dtype)
    do = torch.randn(B, Nq, C, generator=g, device=dev()).to(dtype)
    o_ref, lse_ref, *grads = attn_ref(q, k, v, do, H)
    kv_before = kvbuf.clone()
    dkv, _, mask = framed(B * Nk, width, col, 2 * C, dtype, g, pad_rows=64)
    before = dkv.clone()
    dq = poisoned((B, Nq, C), dtype)
    o = poisoned((B, Nq, C), dtype); lse = poisoned((B, H, Nq), torch.float32); delta = poisoned((B, H, Nq), torch.float32)
    L().check(L().lib().dh_dbg_attention(DT[dtype], P(q), C, at(kvbuf, col), at(kvbuf, col + C), width, P(o), C, P(lse), P(do), P(delta),
                                         P(dq), at(dkv, col), at(dkv, col + C), B, H, Nq, Nk, L().stream_ptr()), "dh_dbg_attention")
    what = f"fused-kv cross-attention B={B} H={H} Nq={Nq}"
    tol = attn_tol(dtype)
    close(o, o_ref, tol, tol, what + " o")
    close(lse, lse_ref, 1e-3, 2e-3, what + " lse")
    d3 = dkv[:B * Nk].view(B, Nk, width)
    check_grads(dtype, (dq, d3[..., col:col + C], d3[..., col + C:col + 2 * C]), grads, what)
    unchanged_outside(dkv, before, mask, what + " dkv")
    unchanged(kvbuf, kv_before, what + " kv")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,H,N", [(2, 5, 64), (1, 20, 1100), (1, 10, 4096)])
def test_attention_bwd_pair_sequential_on_fused_qkv(dtype, B, H, N):
    """dh_dbg_attention_bwd_pair with stream2 = NULL (dQ writes delta, dK / dV reads it, one stream) at the fused strides: the
    forward leaves o and lse through dh_dbg_attention, the pair writes dq | dk | dv into the fused gradient."""
    g = torch.Generator(device=dev()).manual_seed(N + H + 41)
    C = H * 64
    qkv, q, k, v, do = fused_qkv(dtype, B, H, N, g)
    _, _, *grads = attn_ref(q, k, v, do, H)
    qkv_before = qkv.clone()
    o = poisoned((B, N, C), dtype); lse = poisoned((B, H, N), torch.float32); delta = poisoned((B, H, N), torch.float32)
    lib = L().lib()
    L().check(lib.dh_dbg_attention(DT[dtype], P(qkv), 3 * C, at(qkv, C), at(qkv, 2 * C), 3 * C, P(o), C, P(lse), P(None), P(None),
                                   P(None), P(None), P(None), B, H, N, N, L().stream_ptr()), "dh_dbg_attention fwd")
    dqkv, _, mask = framed(B * N, 3 * C, 0, 3 * C, dtype, g, pad_rows=64)
    before = dqkv.clone()
    L().check(lib.dh_dbg_attention_bwd_pair(DT[dtype], P(qkv), 3 * C, at(qkv, C), at(qkv, 2 * C), 3 * C, P(o), C, P(lse), P(do),
                                            P(delta), P(dqkv), at(dqkv, C), at(dqkv, 2 * C), B, H, N, N, L().stream_ptr(), P(None)),
              "dh_dbg_attention_bwd_pair")
    what = f"attention bwd pair (sequential) B={B} H={H} N={N}"
    d3 = dqkv[:B * N].view(B, N, 3 * C)
    check_grads(dtype, (d3[..., :C], d3[..., C:2 * C], d3[..., 2 * C:]), grads, what)
    unchanged_outside(dqkv, before, mask, what + " dqkv")
    unchanged(qkv, qkv_before, what + " qkv")
