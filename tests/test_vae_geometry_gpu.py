"""GPU parity of the VAE engine's launches at the VAE's own geometry (tests/test_vae_geometry.py: GEOMETRY_CASES -- the image side of
the engine's launch, the fewest channels that keep its launch class, the engine's split-K workspace).  One image, shipped policy,
fp16 and bf16, the outputs and the workspace NaN-filled, the arm that ran asserted (dh_dbg_gemm_last_tile against the plan and the
class), element-wise close() against torch fp32: F.conv2d, on F.interpolate(nearest) for the up-sampled form and on
F.pad(0, 1, 0, 1) for pad 0.  Tolerances: those of test_conv3_forward_and_input_gradient (4e-3 / 2.5e-2), CLOSE_CEILING unchanged.

RAMP_CASES run once more on a coordinate ramp with a weight that copies one tap per output channel: every value is a small integer,
the output is exact in 16 bits and the assertion is equality, so a mis-decomposed row index shows as a wrong coordinate.

The VAE attention block runs at N = 4096, C = 512, the only size the product runs (reference and tolerances of
test_vae_attention_block), with the engine's workspace.

GroupNorm runs at the VAE's row counts (G = 32, eps 1e-6, SiLU, forward and backward, test_groupnorm's tolerances, float64 reference).
The last row of the image holds 4096 and x is a view into a larger buffer whose next row holds -4096: a slice edge one row short or
one row long moves the published mean by 4096 / HW and rstd by a factor (tests/test_vae_geometry.py models both), against gates of
4096 / (8 HW) and 1e-3.

DESIGN.md section 8b has the measured close() ratios and what each group caught on detuned builds."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gemm_classes_gpu import TOL, check_arm, workspace
from test_gemm_plan import BIAS, PASS_PART, RESIDUAL, shipped_hooks  # noqa: F401  (shipped_hooks: autouse, the shipped policy)
from test_unet_kernels_gpu import DT, L, P, close, dev, nhwc, poisoned
from test_vae_geometry import CLASS_OF, GEOMETRY_CASES, RAMP_CASES, SPLIT_CLASS, case_query

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]


def gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def launch(dtype, name, A, lda, W, bias, R):
    """dh_dbg_gemm_pad of the case into a NaN-filled output with a NaN-filled workspace of the engine's size; the arm is asserted"""
    q, pad = case_query(name), GEOMETRY_CASES[name][1]
    M, N, K, conv, side, stride, up = q[:7]
    out = side * (2 if up else 1) // stride
    geo = (side, side, K // 9, out, out, stride, up) if conv else (0, 0, 0, 0, 0, 1, 0)
    C, part = poisoned((M, N), dtype), workspace(q[16])
    L().check(L().lib().dh_dbg_gemm_pad(DT[dtype], P(A), lda, P(W), M, N, K, conv, *geo, pad, P(bias), P(None), 0, 1, P(R), N, P(C), N, 0,
                                        P(part), q[16], L().stream_ptr()), "dh_dbg_gemm_pad")
    torch.cuda.synchronize()
    check_arm(SPLIT_CLASS.get(name, CLASS_OF.get(name[0])), q)
    return C


def conv_reference(x, w, bias, stride, up, pad):
    """x [1][Cin][side][side], w [Cout][Cin][3][3] (16-bit values) -> f32 NHWC rows [M][Cout]"""
    xin = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if up else x.float()
    if pad == 0:
        ref = F.conv2d(F.pad(xin, (0, 1, 0, 1)), w.float(), bias, stride=stride)
    else:
        ref = F.conv2d(xin, w.float(), bias, stride=stride, padding=1)
    return nhwc(ref).reshape(-1, w.shape[0])


def tiled_rows(w):
    """[Cout][Cin][3][3] -> the hook's [Cout][tap][Cin]"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def check_borders(C, ref, side_out, tol, what):
    """the image's first / last row and column on their own: where the padding acts, and where the last tile ends"""
    N = C.shape[1]
    c, r = C.view(side_out, side_out, N), ref.view(side_out, side_out, N)
    for sel, edge in ((c[0], r[0]), (c[-1], r[-1]), (c[:, 0], r[:, 0]), (c[:, -1], r[:, -1])):
        close(sel, edge, tol, tol, what + " border")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(GEOMETRY_CASES))
def test_geometry_case(dtype, name):
    q, pad = case_query(name), GEOMETRY_CASES[name][1]
    M, N, K, conv, side, stride, up, flags = q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[9]
    g = gen(M + N + K + side + stride + up + pad)
    bias = torch.randn(N, generator=g, device=dev()) if flags & BIAS else None
    R = torch.randn(M, N, generator=g, device=dev()).to(dtype) if flags & RESIDUAL else None
    what = f"vae geometry {name} {dtype}"
    if conv:
        Cin = K // 9
        x = torch.randn(1, Cin, side, side, generator=g, device=dev()).to(dtype)
        w = (torch.randn(N, Cin, 3, 3, generator=g, device=dev()) / K ** 0.5).to(dtype)
        ref = conv_reference(x, w, bias, stride, up, pad)
        A, lda, W = nhwc(x), Cin, tiled_rows(w)
    else:
        A = torch.randn(M, K, generator=g, device=dev()).to(dtype)
        W = (torch.randn(N, K, generator=g, device=dev()) / K ** 0.5).to(dtype)
        ref = A.float() @ W.float().t() + (bias if bias is not None else 0.0)
        lda = K
    if R is not None:
        ref = ref + R.float()
    assert ref.shape == (M, N)
    C = launch(dtype, name, A, lda, W, bias, R)
    close(C, ref, TOL[dtype], TOL[dtype], what)
    if conv:
        check_borders(C, ref, math.isqrt(M), TOL[dtype], what)
    else:
        close(C[-256:], ref[-256:], TOL[dtype], TOL[dtype], what + " last tile")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", RAMP_CASES)
def test_geometry_case_on_a_coordinate_ramp(dtype, name):
    """input channels 0..3 hold 1 + (y >> 5, y & 31, x >> 5, x & 31) of their pixel (1 .. 32: zero is the padding alone; two channels
    cannot hold 768 coordinates exactly in bf16's eight bits), output channel n copies channel n % 4 of tap (n / 4) % 9 and adds the
    bias n % 8 (and the residual, 0 .. 3): integers below 64, exact in both formats"""
    q, pad = case_query(name), GEOMETRY_CASES[name][1]
    M, N, K, side, stride, up, flags = q[0], q[1], q[2], q[4], q[5], q[6], q[9]
    Cin = K // 9
    yy, xx = torch.meshgrid(torch.arange(side, device=dev()), torch.arange(side, device=dev()), indexing="ij")
    x = torch.zeros(1, Cin, side, side, device=dev())
    for c, v in enumerate((yy >> 5, yy & 31, xx >> 5, xx & 31)):
        x[0, c] = 1 + v
    n = torch.arange(N, device=dev())
    tap = (n // 4) % 9
    w = torch.zeros(N, Cin, 3, 3, device=dev())
    w[n, n % 4, tap // 3, tap % 3] = 1.0
    bias = (n % 8).float()
    m = torch.arange(M, device=dev())
    R = ((m[:, None] * 3 + n[None, :]) % 4).to(dtype) if flags & RESIDUAL else None
    x, w = x.to(dtype), w.to(dtype)
    ref = conv_reference(x, w, bias, stride, up, pad) + (R.float() if R is not None else 0.0)
    assert float(ref.max()) < 64 and bool((ref == ref.round()).all())
    C = launch(dtype, name, nhwc(x), Cin, tiled_rows(w), bias, R)
    wrong = C.float() != ref
    if bool(wrong.any()):
        i = int(wrong.reshape(-1).nonzero()[0])
        row, col = divmod(i, N)
        so = math.isqrt(M)
        raise AssertionError(f"ramp {name} {dtype}: {int(wrong.sum())} of {wrong.numel()} elements differ; first at row {row} = (y {row // so}, "
                             f"x {row % so}), channel {col} (input channel {col % 4}, tap {(col // 4) % 9}): got {C[row, col].item()}, "
                             f"want {ref[row, col].item()}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sigma", [1.0, 2.0])
def test_vae_attention_block_at_the_product_size(dtype, sigma):
    """dh_dbg_vae_attention at N = 4096, C = 512 with the decoder's workspace: the Q K^T GEMM on 256 x 128 tiles, the P V GEMM split four ways"""
    N, C, part_elems = 4096, 512, PASS_PART["vae_dec_lat64"]
    g = gen(N + int(sigma))
    qkv = torch.randn(N, 3 * C, generator=g, device=dev())
    qkv[:, :C] *= sigma / math.sqrt(C)
    qkv = qkv.to(dtype)
    q, k, v = (qkv[:, i * C:(i + 1) * C].float() for i in range(3))
    ref = torch.softmax(q @ k.t(), dim=-1) @ v
    out, tiled, scores = poisoned((N, C), dtype), poisoned((N * C,), dtype), poisoned((N * N,), dtype)
    part = workspace(part_elems)
    L().check(L().lib().dh_dbg_vae_attention(DT[dtype], P(qkv), 3 * C, N, C, P(out), P(tiled), P(scores), P(part), part_elems,
                                             L().stream_ptr()), "dh_dbg_vae_attention")
    torch.cuda.synchronize()
    check_arm(SPLIT_CLASS["e-split-pv"], case_query("e-split-pv"))          # (the last launch of the block: P V)
    tol = 5e-3 if dtype == torch.float16 else 3e-2
    close(out, ref, tol, tol, f"vae attention {dtype} N={N} logit std {sigma}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("HW,C", [(262144, 128), (262144, 256), (589824, 128), (65536, 512)])
def test_groupnorm_at_the_vae_row_counts(dtype, HW, C):
    G, eps = 32, 1e-6
    g = gen(HW + C)
    buf = (torch.randn(HW + 1, C, generator=g, device=dev()) * 2 + 0.5).to(dtype)
    buf[HW - 1] = 4096.0
    buf[HW] = -4096.0
    x = buf[:HW]
    gamma = 1 + 0.1 * torch.randn(C, generator=g, device=dev())
    beta = 0.1 * torch.randn(C, generator=g, device=dev())
    dy = torch.randn(HW, C, generator=g, device=dev()).to(dtype)
    acc0 = torch.randn(HW, C, generator=g, device=dev()).to(dtype)
    xr = x.double().requires_grad_(True)
    xg = xr.view(HW, G, C // G)
    mean, var = xg.mean(dim=(0, 2), keepdim=True), xg.var(dim=(0, 2), unbiased=False, keepdim=True)
    ref = F.silu(((xg - mean) * (var + eps).rsqrt()).view(HW, C) * gamma.double() + beta.double())
    gref, = torch.autograd.grad(ref, xr, dy.double())
    y, dx = poisoned((HW, C), dtype), acc0.clone()          # dx accumulates onto acc0 by design
    stats = poisoned((G * 2,), torch.float32)
    scr = torch.empty(G * 32 * 3 + 64, dtype=torch.float32, device=dev())
    L().check(L().lib().dh_dbg_groupnorm(DT[dtype], P(x), P(gamma), P(beta), P(y), P(stats), P(dy), P(dx), P(scr), 1, HW, C, G, eps, 1, 1,
                                         L().stream_ptr()), "dh_dbg_groupnorm")
    torch.cuda.synchronize()
    got = stats.double().view(G, 2)
    m64, r64 = mean.detach().reshape(G), (var.detach().reshape(G) + eps).rsqrt()
    em, er = float((got[:, 0] - m64).abs().max()), float((got[:, 1] / r64 - 1).abs().max())
    gate = 4096.0 / (8 * HW)
    print(f"groupnorm {dtype} HW={HW} C={C}: mean error {em:.2e} (gate {gate:.2e}), rstd relative error {er:.2e} (gate 1e-3)")
    assert em <= gate and er <= 1e-3, (em, gate, er)
    tol = TOL[dtype]
    what = f"groupnorm {dtype} HW={HW} C={C}"
    close(y, ref.detach(), tol, tol, what + " fwd")
    close(dx, gref + acc0.double(), tol, tol * 2, what + " bwd (accumulate)")
    close(y[-1], ref.detach()[-1], tol, tol, what + " fwd last row")
    assert float(buf[HW, 0]) == -4096.0
