"""GPU parity, element by element, of the kernels that only an engine launches (U-Net conv_in / conv_out, the VAE's attention block
and down-sampling convolution, the text tower's causal attention and GELU, the GroupNorm apply kernels at multi-chunk sizes and in
their split form, the column / pool / convert copies, the timestep embedding).  The engine tests gate one relative L2 norm per
output tensor, which a wrong border row, an unwritten tail block, a stale accumulate buffer or an off-by-one mask passes; here every
output starts NaN-filled and is compared with a torch fp32 / fp64 reference of the same operation on the same 16-bit-rounded inputs.
Where a tolerance is "one 16-bit unit in the last place" it is the spacing of the storage format at the reference's magnitude
(ulp16): the kernels round an f32 result once, which is half of that."""
import math

import pytest
import torch
import torch.nn.functional as F

from per_element import EMIN, MANT, ulp16, within  # noqa: F401  (other test files import them from here)
from test_unet_kernels_gpu import DT, L, P, close, dev, poisoned

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]


def gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def all_poison(t):
    return bool(torch.isnan(t).all())


# ---------------------------------------------------------------------------------------------------------- causal attention
def causal_shapes():
    import test_attn_plan as T
    return T.CAUSAL_SHAPES


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,N", causal_shapes())
def test_attention_causal(dtype, B, H, N):
    """launch_attention_fwd(..., causal = 1), the text tower's launch: o = softmax(mask(q k^T / 8)) v with key j visible to query i
    for j <= i.  Row 0 sees key 0 only, so it equals v[0]; the launch is the one the host plan names for the causal query; with
    lse = NULL (what the text engine passes) o has the same bits."""
    import test_attn_plan as T
    g = gen(N + H + B)
    C = H * 64
    q = torch.randn(B, N, C, generator=g, device=dev()).to(dtype)
    k = torch.randn(B, N, C, generator=g, device=dev()).to(dtype)
    v = torch.randn(B, N, C, generator=g, device=dev()).to(dtype)
    k[:, N // 2, :] *= 6.0                               # a large running-max jump mid-stream, for the rows that see that key
    sp = lambda t: t.float().view(B, N, H, 64).transpose(1, 2)
    s = (sp(q) @ sp(k).transpose(-1, -2)) * 0.125
    hidden = torch.ones(N, N, dtype=torch.bool, device=dev()).triu(1)          # [i][j]: j > i
    s = s.masked_fill(hidden, float("-inf"))
    ref = (torch.softmax(s, dim=-1) @ sp(v)).transpose(1, 2).reshape(B, N, C)
    lse_ref = torch.logsumexp(s, dim=-1)
    lib = L().lib()

    def run(with_lse):
        o = poisoned(q.shape, dtype)
        lse = poisoned((B, H, N), torch.float32) if with_lse else None
        L().check(lib.dh_dbg_attention_causal(DT[dtype], P(q), C, P(k), P(v), C, P(o), C, P(lse), B, H, N, N, L().stream_ptr()),
                  "dh_dbg_attention_causal")
        torch.cuda.synchronize()
        return o, lse

    o, lse = run(True)
    planned = T.named(T.plan(T.FWD, B, H, N, N, 1))
    what = f"causal attn {dtype} B={B} H={H} N={N}"
    assert planned["launch"] == 1 and T.last_launch(T.FWD) == {f: planned[f] for f in T.LAST}, (what, planned, T.last_launch(T.FWD))
    tol = 5e-3 if dtype == torch.float16 else 3e-2
    close(o, ref, tol, tol, what + " fwd")
    close(lse, lse_ref, 1e-3, 2e-3, what + " lse")
    close(o[:, 0, :], v[:, 0, :].float(), tol, tol, what + " row 0 == v[0]")
    if (B, H, N) == (1, 16, 77):
        o2, _ = run(False)
        assert torch.equal(bits(o), bits(o2)), what + ": o differs between lse given and lse = NULL"


# ------------------------------------------------------------------------------------------------------- VAE attention block
def vae_attention(dtype, N, sigma, seed):
    """dh_dbg_vae_attention on qkv [N][3 C], C = 512, q scaled so that the logits q k^T have standard deviation sigma (the engine folds
    the 1 / sqrt(C) into the q projection); returns (out, fp32 reference softmax(q k^T) v)"""
    C = 512
    g = gen(seed)
    qkv = torch.randn(N, 3 * C, generator=g, device=dev())
    qkv[:, :C] *= sigma / math.sqrt(C)
    qkv = qkv.to(dtype)
    q, k, v = (qkv[:, i * C:(i + 1) * C].float() for i in range(3))
    ref = torch.softmax(q @ k.t(), dim=-1) @ v
    out = poisoned((N, C), dtype)
    tiled = poisoned((N * C,), dtype)
    scores = poisoned((N * N,), dtype)
    part = poisoned((16 << 20,), torch.float32)          # NaN-filled split-K slab: whatever the reduce reads, the K loop wrote
    L().check(L().lib().dh_dbg_vae_attention(DT[dtype], P(qkv), 3 * C, N, C, P(out), P(tiled), P(scores), P(part), part.numel(),
                                             L().stream_ptr()), "dh_dbg_vae_attention")
    torch.cuda.synchronize()
    return out, ref


@pytest.mark.parametrize("dtype,N,sigma", [(dt, n, s) for dt in DTYPES for n in (256, 1024) for s in (1.0, 2.0)]
                         + [(torch.float16, 4096, 2.0)])
def test_vae_attention_block(dtype, N, sigma):
    """the VAE mid block's single-head attention as the tape runs it (k_tile_rows, Q K^T GEMM into 16-bit scores, k_softmax_rows in
    place, transposed k_tile_rows, P V GEMM): logits and probabilities are each rounded to 16 bits once.  At logit standard deviations
    1 and 2 a CPU model of those two roundings stays at or below 0.47 of the flash-attention tolerance (N = 1024)."""
    out, ref = vae_attention(dtype, N, sigma, N + int(sigma))
    tol = 5e-3 if dtype == torch.float16 else 3e-2
    close(out, ref, tol, tol, f"vae attention {dtype} N={N} logit std {sigma}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [256, 1024])
def test_vae_attention_block_logit_std_4(dtype, N):
    """at logit standard deviation 4 the two 16-bit roundings alone reach the flash-attention tolerance (the CPU model: 1.0 tolerances
    at fp16, 1.6 at bf16, up to 3.4e-5 of the elements over it), so this case is gated like the VAE decoder test: finite, relative L2
    below 1e-2 (fp16) / 4e-2 (bf16).  The worst ratio is printed (DESIGN.md records it)."""
    out, ref = vae_attention(dtype, N, 4.0, N + 4)
    tol = 5e-3 if dtype == torch.float16 else 3e-2
    assert bool(torch.isfinite(out).all())
    ratio = (out.float() - ref).abs() / (tol + tol * ref.abs())
    err = ((out.float() - ref).norm() / ref.norm()).item()
    print(f"vae attention {dtype} N={N} logit std 4: worst {ratio.max().item():.3g} x the flash-attention tolerance, "
          f"frac over {(ratio > 1).float().mean().item():.3g}, rel L2 {err:.3e}")
    assert err < (1e-2 if dtype == torch.float16 else 4e-2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", [(5, 64), (4, 72), (7, 520), (256, 256), (33, 4096)])
def test_softmax_rows(dtype, rows, cols):
    """k_softmax_rows in place against an fp64 softmax of the 16-bit inputs: 3 randn rows, a row of equal values, a row far from zero
    (the maximum must be subtracted before the exponential) and a row with one large entry; a column count that is no multiple of
    the 512-element sweep, fewer rows than a workgroup's four"""
    g = gen(rows + cols)
    x = torch.randn(rows, cols, generator=g, device=dev()) * 3.0
    x[0, :] = 1.5
    x[1, :] += 30000.0 if dtype == torch.float16 else 1e30
    x[2, cols // 3] = 40.0
    s = x.to(dtype)
    ref = torch.softmax(s.double(), dim=-1)
    L().check(L().lib().dh_dbg_softmax_rows(DT[dtype], P(s), rows, cols, L().stream_ptr()), "dh_dbg_softmax_rows")
    torch.cuda.synchronize()
    within(s, ref, ulp16(ref, dtype) + 1e-6, f"softmax rows {dtype} {rows}x{cols}")


# -------------------------------------------------------------------------- 3x3 convolution, pad = 0, stride 2 (VAE down-sampler)
def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,Cin,Cout,Hin", [(1, 128, 128, 16), (2, 256, 256, 12), (1, 512, 512, 8), (1, 128, 128, 64)])
def test_conv3_stride2_pad_bottom_right(dtype, B, Cin, Cout, Hin):
    """the VAE encoder's down-sampler: stride 2 with the zero padding on the bottom and right only (GemmArgs::pad = 0).  The last output
    row and column, where that padding acts, are checked on their own as well."""
    g = gen(Cin + Cout + Hin)
    x = torch.randn(B, Cin, Hin, Hin, generator=g, device=dev()).to(dtype)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g, device=dev()) / (9 * Cin) ** 0.5).to(dtype)
    bias = torch.randn(Cout, generator=g, device=dev())
    ref = nhwc(F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), w.float(), bias, stride=2))
    Ho = ref.shape[1]
    assert Ho == Hin // 2
    wf = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous()                      # [Cout][tap][Cin]
    M, K = B * Ho * Ho, 9 * Cin
    C = poisoned((M, Cout), dtype)
    part = poisoned((16 << 20,), torch.float32)
    A = nhwc(x)
    L().check(L().lib().dh_dbg_gemm_pad(DT[dtype], P(A), Cin, P(wf), M, Cout, K, 1, Hin, Hin, Cin, Ho, Ho, 2, 0, 0, P(bias), P(None), 0, 1,
                                        P(None), Cout, P(C), Cout, 0, P(part), part.numel(), L().stream_ptr()), "dh_dbg_gemm_pad")
    torch.cuda.synchronize()
    tol = 4e-3 if dtype == torch.float16 else 2.5e-2
    y = C.view(B, Ho, Ho, Cout)
    what = f"conv pad=0 stride 2 {dtype} B={B} {Cin}->{Cout} H={Hin}"
    close(y, ref, tol, tol, what)
    close(y[:, -1], ref[:, -1], tol, tol, what + " last output row")
    close(y[:, :, -1], ref[:, :, -1], tol, tol, what + " last output column")


# ------------------------------------------------------------------------------------------------------- small convolutions
SH, SW = 7, 5          # neither the 4-pixel groups of k_conv_few_in nor k_conv_few_out's pixels per block divide 35 (or 70) pixels


def conv_ref64(x, w, bias):
    """x [B,H,W,Ci], w [Co,Ci,3,3], bias [Co] or None -> (fp64 conv [B,H,W,Co], A = conv(|x|, |w|) + |b|), on the CPU"""
    xd, wd = x.double().cpu().permute(0, 3, 1, 2), w.double().cpu()
    bd = bias.double().cpu() if bias is not None else None
    ref = F.conv2d(xd, wd, bd, padding=1)
    mag = F.conv2d(xd.abs(), wd.abs(), bd.abs() if bd is not None else None, padding=1)
    return ref.permute(0, 2, 3, 1).contiguous().to(dev()), mag.permute(0, 2, 3, 1).contiguous().to(dev())


def taps_last(w):
    """torch [Co][Ci][3][3] -> the kernels' f32 [Co][tap][Ci]"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).float().contiguous()


def grad_weights(w):
    """weights of the gradient convolution of conv(., w) (w [Co][Ci][3][3]): taps flipped, channel roles swapped -> [Ci][Co][3][3]"""
    return w.flip(2, 3).permute(1, 0, 2, 3).contiguous()


def conv_small(dtype, bwd, x, w, bias, y, accumulate, B, Cin, Cout):
    return L().lib().dh_dbg_conv_small(DT[dtype], bwd, P(x), int(x.dtype == torch.float32), P(w), P(bias), P(y),
                                       int(y.dtype == torch.float32), accumulate, B, SH, SW, Cin, Cout, L().stream_ptr())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("Ci,Co", [(5, 320), (4, 512), (3, 128), (8, 64)])
def test_conv_few_in(dtype, B, Ci, Co):
    """k_conv_few_in forward (U-Net conv_in, VAE conv_in): f32 input, f32 weights and bias, 16-bit output"""
    g = gen(Ci + Co + B)
    x = torch.randn(B, SH, SW, Ci, generator=g, device=dev())
    w = torch.randn(Co, Ci, 3, 3, generator=g, device=dev()) / (9 * Ci) ** 0.5
    bias = torch.randn(Co, generator=g, device=dev())
    ref, mag = conv_ref64(x, w, bias)
    y = poisoned((B, SH, SW, Co), dtype)
    L().check(conv_small(dtype, 0, x, taps_last(w), bias, y, 0, B, Ci, Co), "dh_dbg_conv_small few-in")
    torch.cuda.synchronize()
    within(y, ref, ulp16(ref, dtype) + 1e-5 * mag, f"conv few-in {dtype} B={B} {Ci}->{Co}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("Ci,Co", [(320, 4), (128, 3), (64, 8), (512, 8), (2048, 1)])
def test_conv_few_out(dtype, B, Ci, Co):
    """k_conv_few_out forward (U-Net conv_out, VAE conv_out): 16-bit input, f32 weights, bias and output.  320 channels are 40 chunks,
    which do not divide the 256 threads; (64, 8) has exactly 256 reducing threads.  1e-5 A is about 170 f32 epsilons of the summed
    magnitudes; a missing tap is of order 0.1 A."""
    g = gen(Ci + Co + B)
    x = torch.randn(B, SH, SW, Ci, generator=g, device=dev()).to(dtype)
    w = torch.randn(Co, Ci, 3, 3, generator=g, device=dev()) / (9 * Ci) ** 0.5
    bias = torch.randn(Co, generator=g, device=dev())
    ref, mag = conv_ref64(x, w, bias)
    y = poisoned((B, SH, SW, Co), torch.float32)
    L().check(conv_small(dtype, 0, x, taps_last(w), bias, y, 0, B, Ci, Co), "dh_dbg_conv_small few-out")
    torch.cuda.synchronize()
    within(y, ref, 1e-5 * mag, f"conv few-out {dtype} B={B} {Ci}->{Co}")


def conv_grad64(w, dy, Ci):
    """fp64 autograd gradient of conv(x, w) (x [B,H,W,Ci]) to x for the output gradient dy [B,H,W,Co]; NHWC, on the CPU"""
    B = dy.shape[0]
    xr = torch.zeros(B, Ci, SH, SW, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(xr, w.double().cpu(), None, padding=1)
    gref, = torch.autograd.grad(out, xr, dy.double().cpu().permute(0, 3, 1, 2))
    return gref.permute(0, 2, 3, 1).contiguous().to(dev())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 2])
def test_conv_few_in_gradient(dtype, B):
    """k_conv_few_in as the input gradient of a 320 -> 4 convolution (U-Net conv_out backward): dy f32 with 4 channels, dx 16-bit with
    320, the gradient convolution's weights built here; against torch.autograd.grad of the forward convolution"""
    Ci, Co = 320, 4
    g = gen(17 + B)
    w = torch.randn(Co, Ci, 3, 3, generator=g, device=dev()) / (9 * Ci) ** 0.5
    dy = torch.randn(B, SH, SW, Co, generator=g, device=dev())
    gref = conv_grad64(w, dy, Ci)
    wg = grad_weights(w)                                                  # [Ci][Co][3][3]: a Co -> Ci convolution
    ref, mag = conv_ref64(dy, wg, None)
    assert torch.allclose(ref, gref, rtol=0, atol=1e-12)                  # the gradient convolution IS the autograd gradient
    dx = poisoned((B, SH, SW, Ci), dtype)
    L().check(conv_small(dtype, 1, dy, taps_last(wg), None, dx, 0, B, Co, Ci), "dh_dbg_conv_small few-in gradient")
    torch.cuda.synchronize()
    within(dx, gref, ulp16(gref, dtype) + 1e-5 * mag, f"conv few-in gradient {dtype} B={B}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 2])
def test_conv_few_out_gradient_and_accumulate(dtype, B):
    """k_conv_few_out as the input gradient of a 5 -> 320 convolution (U-Net conv_in backward: the guidance gradient to the latent): dy
    16-bit with 320 channels, dx f32 with 5.  accumulate = 0 must not read dx (NaN-filled here); accumulate = 1 adds onto it."""
    Ci, Co = 5, 320
    g = gen(29 + B)
    w = torch.randn(Co, Ci, 3, 3, generator=g, device=dev()) / (9 * Ci) ** 0.5
    dy = torch.randn(B, SH, SW, Co, generator=g, device=dev()).to(dtype)
    gref = conv_grad64(w, dy, Ci)
    wg = grad_weights(w)                                                  # [5][320][3][3]
    _, mag = conv_ref64(dy, wg, None)
    dx = poisoned((B, SH, SW, Ci), torch.float32)
    L().check(conv_small(dtype, 1, dy, taps_last(wg), None, dx, 0, B, Co, Ci), "dh_dbg_conv_small few-out gradient")
    torch.cuda.synchronize()
    within(dx, gref, 1e-5 * mag, f"conv few-out gradient {dtype} B={B} accumulate=0")
    acc0 = torch.randn(B, SH, SW, Ci, generator=g, device=dev())
    dx = acc0.clone()
    L().check(conv_small(dtype, 1, dy, taps_last(wg), None, dx, 1, B, Co, Ci), "dh_dbg_conv_small few-out gradient")
    torch.cuda.synchronize()
    within(dx, gref + acc0.double(), 1e-5 * mag, f"conv few-out gradient {dtype} B={B} accumulate=1")


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_few_out_refuses_a_shape_outside_its_limits(dtype):
    """Ci = 32 is below conv_few_out_ok's 64 channels: the launcher refuses before any launch, the hook returns the error, the message is
    in dh_last_error and the output keeps its poison"""
    Ci, Co = 32, 4
    x = torch.zeros(1, SH, SW, Ci, dtype=dtype, device=dev())
    w = torch.zeros(Co, 9 * Ci, device=dev())
    bias = torch.zeros(Co, device=dev())
    for bwd in (0, 1):
        y = poisoned((1, SH, SW, Co), torch.float32)
        rc = conv_small(dtype, bwd, x, w, bias if not bwd else None, y, 0, 1, Ci, Co)
        torch.cuda.synchronize()
        assert rc != 0 and b"few-output convolution" in L().lib().dh_last_error(), (rc, L().lib().dh_last_error())
        assert all_poison(y)


# ------------------------------------------------------------------------------------------------------- GroupNorm envelope
def gn_reference(x, gamma, beta, dy, silu):
    xr = x.float().requires_grad_(True)
    ref = F.group_norm(xr.transpose(1, 2), 32, gamma, beta, eps=1e-5).transpose(1, 2)
    if silu:
        ref = F.silu(ref)
    gref, = torch.autograd.grad(ref, xr, dy.float())
    return ref.detach(), gref


def gn_inputs(dtype, B, HW, C, seed):
    g = gen(seed)
    x = (torch.randn(B, HW, C, generator=g, device=dev()) * 2 + 0.5).to(dtype)
    gamma = 1 + 0.1 * torch.randn(C, generator=g, device=dev())
    beta = 0.1 * torch.randn(C, generator=g, device=dev())
    dy = torch.randn(B, HW, C, generator=g, device=dev()).to(dtype)
    acc0 = torch.randn(B, HW, C, generator=g, device=dev()).to(dtype)
    return x, gamma, beta, dy, acc0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,HW,C,silu", [(2, 4096, 640, 1),        # 5.2 M elements: two chunks per thread of the apply kernels
                                          (1, 66000, 256, 1),       # 16.9 M: eight chunks per thread, a ragged last block
                                          (1, 16384, 128, 1),       # 4 channels per group (the VAE): the non-WIDE apply kernels
                                          (3, 700, 1280, 0)])
def test_groupnorm_apply_envelope(dtype, B, HW, C, silu):
    """GroupNorm forward and backward where the apply kernels loop over several chunks per thread (gn_apply_iters >= 2 from
    B HW C >= 4.19 M on: every batch-8 U-Net pass, every VAE layer from 256^2 on), at 4 channels per group, and with accumulate = 0
    into a NaN-filled dx (which must not be read) as well as accumulate = 1"""
    x, gamma, beta, dy, acc0 = gn_inputs(dtype, B, HW, C, C + HW)
    ref, gref = gn_reference(x, gamma, beta, dy, silu)
    tol = 4e-3 if dtype == torch.float16 else 2.5e-2
    for accumulate in (0, 1):
        y = poisoned(x.shape, dtype)
        dx = acc0.clone() if accumulate else poisoned(x.shape, dtype)
        stats = poisoned((B * 32 * 2,), torch.float32)
        scr = torch.empty(B * 32 * 32 * 3 + 64, dtype=torch.float32, device=dev())
        L().check(L().lib().dh_dbg_groupnorm(DT[dtype], P(x), P(gamma), P(beta), P(y), P(stats), P(dy), P(dx), P(scr), B, HW, C, 32,
                                             1e-5, silu, accumulate, L().stream_ptr()), "dh_dbg_groupnorm")
        torch.cuda.synchronize()
        what = f"gn {dtype} B={B} HW={HW} C={C} accumulate={accumulate}"
        close(y, ref, tol, tol, what + " fwd")
        close(dx, gref + acc0.float() if accumulate else gref, tol, tol * 2, what + " bwd")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("HW", [64, 1024])
@pytest.mark.parametrize("Ca,Cb", [(320, 320), (640, 320), (1280, 640)])
def test_groupnorm_backward_split(dtype, Ca, Cb, HW):
    """the GnBwdSplit form (engine: the GroupNorm behind a concatenation): the gradient goes straight to the two sources of the
    concatenation, columns [0, Ca) to out0 and the rest to out1; dx itself is not touched (accumulate = 0: it is not read either)"""
    B, C = 2, Ca + Cb
    x, gamma, beta, dy, _ = gn_inputs(dtype, B, HW, C, Ca + Cb + HW)
    ref, gref = gn_reference(x, gamma, beta, dy, 1)
    y = poisoned(x.shape, dtype); dx = poisoned(x.shape, dtype)
    out0 = poisoned((B, HW, Ca), dtype); out1 = poisoned((B, HW, Cb), dtype)
    stats = poisoned((B * 32 * 2,), torch.float32)
    scr = torch.empty(B * 32 * 32 * 3 + 64, dtype=torch.float32, device=dev())
    L().check(L().lib().dh_dbg_groupnorm_split(DT[dtype], P(x), P(gamma), P(beta), P(y), P(stats), P(dy), P(dx), P(scr), B, HW, C, 32,
                                               1e-5, 1, 0, P(out0), P(out1), Ca, L().stream_ptr()), "dh_dbg_groupnorm_split")
    torch.cuda.synchronize()
    tol = 4e-3 if dtype == torch.float16 else 2.5e-2
    what = f"gn split {dtype} {Ca}+{Cb} HW={HW}"
    close(y, ref, tol, tol, what + " fwd")
    close(out0, gref[..., :Ca], tol, tol * 2, what + " out0")
    close(out1, gref[..., Ca:], tol, tol * 2, what + " out1")
    assert all_poison(dx), what + ": dx was written"


# ---------------------------------------------------------------------------------------------------------- activation sweep
def finite_patterns(dtype, multiple):
    """every finite value of the 16-bit format (65536 bit patterns minus inf and NaN), zero-padded to a multiple of `multiple`"""
    allp = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)
    v = allp[torch.isfinite(allp)]
    assert v.numel() == 65536 - (2048 if dtype == torch.float16 else 256)
    pad = (-v.numel()) % multiple
    return torch.cat([v, torch.zeros(pad, dtype=dtype)]).to(dev())


def gelu64(g):
    g = g.double()
    return 0.5 * g * torch.erfc(-g / math.sqrt(2.0))                      # = 0.5 g (1 + erf(g / sqrt 2)), without its cancellation at g << 0


def gelu_grad64(g):
    g = g.double()
    return 0.5 * torch.erfc(-g / math.sqrt(2.0)) + g * torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gelu_every_finite_value(dtype):
    """k_gelu (text-tower MLP) on every finite 16-bit value.  gelu_parts states |error| <= 1.5e-7 for Phi; 1e-6 |g| leaves room for the
    f32 rcp and exp steps on top of it."""
    g = finite_patterns(dtype, 8)
    y = poisoned(g.shape, dtype)
    L().check(L().lib().dh_dbg_gelu(DT[dtype], P(g), P(y), g.numel(), L().stream_ptr()), "dh_dbg_gelu")
    torch.cuda.synchronize()
    ref = gelu64(g)
    within(y, ref, ulp16(ref, dtype) + 1e-6 * g.double().abs(), f"gelu {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gelu_grad_every_finite_value(dtype):
    """gelu_grad through the GEGLU backward: every finite 16-bit value as the gate, value 1 and dy 1, so that d_gate = gelu'(g) (and
    d_value = y = gelu(g))"""
    from layernorm_ref import glu_paired_index
    g = finite_patterns(dtype, 16)
    Fd = g.numel()
    idx = glu_paired_index(Fd).to(dev())
    x = torch.cat([torch.ones(Fd, dtype=dtype, device=dev()), g]).view(1, 2 * Fd)
    xp = x[:, idx].contiguous()
    dy = torch.ones(1, Fd, dtype=dtype, device=dev())
    y = poisoned((1, Fd), dtype); dxp = poisoned((1, 2 * Fd), dtype)
    L().check(L().lib().dh_dbg_geglu(DT[dtype], P(xp), P(y), P(dy), P(dxp), 1, Fd, L().stream_ptr()), "dh_dbg_geglu")
    torch.cuda.synchronize()
    dx = torch.empty_like(dxp); dx[:, idx] = dxp
    ref, gref = gelu64(g), gelu_grad64(g)
    tol = ulp16(ref, dtype) + 1e-6 * g.double().abs()
    within(y[0], ref, tol, f"geglu y = gelu(g) {dtype}")
    within(dx[0, :Fd], ref, tol, f"geglu d_value = gelu(g) {dtype}")
    within(dx[0, Fd:], gref, ulp16(gref, dtype) + 1e-6 * (1.0 + g.double().abs()), f"geglu d_gate = gelu'(g) {dtype}")


# ------------------------------------------------------------------------------------------- column, pool and convert kernels
def check_sum16(got, a, b, dtype, what):
    """got = a + b rounded to 16 bits from an f32 sum: within one unit in the last place of the fp64 sum"""
    ref = a.double() + b.double()
    within(got, ref, ulp16(ref, dtype), what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", [64, 320])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_copy_cols_strided(dtype, cols, accumulate):
    """k_copy_cols from a column slice of a [37][960] tensor into a column slice of a [37][1280] one"""
    rows, lds, ldd, c_src, c_dst = 37, 960, 1280, 128, 320
    g = gen(cols + accumulate)
    src = torch.randn(rows, lds, generator=g, device=dev()).to(dtype)
    dst = poisoned((rows, ldd), dtype)
    old = torch.randn(rows, cols, generator=g, device=dev()).to(dtype)
    if accumulate:
        dst[:, c_dst:c_dst + cols] = old
    L().check(L().lib().dh_dbg_copy_cols(DT[dtype], P(src[:, c_src:]), lds, P(dst[:, c_dst:]), ldd, rows, cols, accumulate,
                                         L().stream_ptr()), "dh_dbg_copy_cols")
    torch.cuda.synchronize()
    got, want = dst[:, c_dst:c_dst + cols], src[:, c_src:c_src + cols]
    if accumulate:
        check_sum16(got, want, old, dtype, f"copy_cols += {dtype} cols={cols}")
    else:
        assert torch.equal(bits(got), bits(want))
    assert all_poison(dst[:, :c_dst]) and all_poison(dst[:, c_dst + cols:])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("colsA,colsB", [(320, 320), (640, 320)])
@pytest.mark.parametrize("accA,accB", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_split_cols_strided(dtype, colsA, colsB, accA, accB):
    """k_split_cols (concat backward): a [37][colsA + colsB] slice of a wider tensor into column slices of two wider tensors, each
    half assigned or accumulated"""
    rows, lds, c_src, pad = 37, 1280, 64, 64
    g = gen(colsA + colsB + 2 * accA + accB)
    src = torch.randn(rows, lds, generator=g, device=dev()).to(dtype)
    dA = poisoned((rows, colsA + 2 * pad), dtype); dB = poisoned((rows, colsB + 2 * pad), dtype)
    oldA = torch.randn(rows, colsA, generator=g, device=dev()).to(dtype)
    oldB = torch.randn(rows, colsB, generator=g, device=dev()).to(dtype)
    if accA:
        dA[:, pad:pad + colsA] = oldA
    if accB:
        dB[:, pad:pad + colsB] = oldB
    L().check(L().lib().dh_dbg_split_cols(DT[dtype], P(src[:, c_src:]), lds, P(dA[:, pad:]), dA.shape[1], colsA, accA, P(dB[:, pad:]),
                                          dB.shape[1], colsB, accB, rows, L().stream_ptr()), "dh_dbg_split_cols")
    torch.cuda.synchronize()
    for nm, d, old, acc, want in (("A", dA, oldA, accA, src[:, c_src:c_src + colsA]),
                                  ("B", dB, oldB, accB, src[:, c_src + colsA:c_src + colsA + colsB])):
        n = want.shape[1]
        got = d[:, pad:pad + n]
        if acc:
            check_sum16(got, want, old, dtype, f"split_cols {nm} += {dtype} {colsA}|{colsB}")
        else:
            assert torch.equal(bits(got), bits(want)), nm
        assert all_poison(d[:, :pad]) and all_poison(d[:, pad + n:]), nm


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,h,w,C", [(2, 3, 5, 64), (1, 8, 8, 320)])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_pool2x2_accumulate(dtype, B, h, w, C, accumulate):
    """k_pool2x2: dst (=|+=) the sum of each 2x2 block.  The kernel adds the four values in f32 in the order (0,0), (0,1), (1,0), (1,1)
    and rounds once: accumulate = 0 equals that IEEE sum bit for bit, and both forms are within one 16-bit unit in the last place of the
    fp64 sum."""
    g = gen(B + h + w + C + accumulate)
    src = torch.randn(B, 2 * h, 2 * w, C, generator=g, device=dev()).to(dtype)
    old = torch.randn(B, h, w, C, generator=g, device=dev()).to(dtype)
    dst = old.clone() if accumulate else poisoned((B, h, w, C), dtype)
    L().check(L().lib().dh_dbg_pool2x2(DT[dtype], P(src), P(dst), B, h, w, C, accumulate, L().stream_ptr()), "dh_dbg_pool2x2")
    torch.cuda.synchronize()
    quad = [src[:, dy::2, dx::2].float() for dy in (0, 1) for dx in (0, 1)]
    s32 = ((quad[0] + quad[1]) + quad[2]) + quad[3]
    s64 = sum(t.double() for t in quad)
    if accumulate:
        ref = s64 + old.double()
        within(dst, ref, ulp16(ref, dtype), f"pool2x2 += {dtype}")
    else:
        assert torch.equal(bits(dst), bits(s32.to(dtype)))
        within(dst, s64, ulp16(s64, dtype), f"pool2x2 {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_convert_both_directions(dtype):
    """k_f32_to_t rounds to nearest even as torch does; k_t_to_f32 is exact, and with accumulate adds in f32"""
    n = 1000
    g = gen(n)
    lib = L().lib()
    f = torch.randn(n, generator=g, device=dev()) * 100.0
    f[:4] = torch.tensor([0.0, -0.0, 1e-6, 3e-8], device=dev())
    h = poisoned((n + 8,), dtype)
    L().check(lib.dh_dbg_convert(DT[dtype], 0, P(f), P(h), n, 0, L().stream_ptr()), "dh_dbg_convert f32 -> 16-bit")
    torch.cuda.synchronize()
    assert torch.equal(bits(h[:n]), bits(f.to(dtype))) and all_poison(h[n:])
    s = f.to(dtype)
    d = poisoned((n + 8,), torch.float32)
    L().check(lib.dh_dbg_convert(DT[dtype], 1, P(s), P(d), n, 0, L().stream_ptr()), "dh_dbg_convert 16-bit -> f32")
    torch.cuda.synchronize()
    assert torch.equal(bits(d[:n]), bits(s.float())) and all_poison(d[n:])
    old = torch.randn(n, generator=g, device=dev())
    d[:n] = old
    L().check(lib.dh_dbg_convert(DT[dtype], 1, P(s), P(d), n, 1, L().stream_ptr()), "dh_dbg_convert 16-bit -> f32 +=")
    torch.cuda.synchronize()
    assert torch.equal(bits(d[:n]), bits(old + s.float())) and all_poison(d[n:])
    ref = old.double() + s.double()
    within(d[:n], ref, ulp16(ref, dtype), f"t_to_f32 += {dtype}")


# --------------------------------------------------------------------------------------------------------- timestep embedding
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [320, 64])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("t", [0.0, 1.0, 20.5, 999.0])
def test_timestep_embedding(dtype, dim, B, t):
    """k_timestep: every row of out [B][dim] = [cos(t f_i) | sin(t f_i)], f_i = 10000^(-i / half).  2e-4 covers the f32 argument:
    |t f| <= 999 carries a few f32 epsilons of 999 (6e-5 each)."""
    half = dim // 2
    td = torch.tensor([t], dtype=torch.float32, device=dev())
    out = poisoned((B, dim), dtype)
    L().check(L().lib().dh_dbg_timestep(DT[dtype], P(td), dim, B, P(out), L().stream_ptr()), "dh_dbg_timestep")
    torch.cuda.synchronize()
    a = t * torch.pow(torch.tensor(10000.0, dtype=torch.float64), -torch.arange(half, dtype=torch.float64) / half)
    ref = torch.cat([torch.cos(a), torch.sin(a)]).to(dev()).expand(B, dim)
    within(out, ref, ulp16(ref, dtype) + 2e-4, f"timestep {dtype} dim={dim} B={B} t={t}")
