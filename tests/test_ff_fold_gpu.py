"""A transformer's proj_out folded into its ff.net.2 (csrc/unet_engine.cpp FfFold): the folded weight and bias against the
f64 product of the unfolded parameters, and the column-split GEGLU-backward epilogue of the folded op's input-gradient GEMM
(gemm.hip, GemmArgs::glub_f) against torch.  The end-to-end parity of the folded blocks, forward and backward at every latent
level, is tests/test_unet_engine_gpu.py's."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from layernorm_ref import glu_paired_index

pytestmark = pytest.mark.gpu

DT = {torch.float16: 0, torch.bfloat16: 1}


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
    """Every element finite; at most `frac` of them over atol + rtol |ref| (16-bit rounding of near-ties), none over `ceiling`
    times that (the rule of tests/test_unet_kernels_gpu.py close())."""
    g, r = got.float(), ref.float()
    assert tuple(g.shape) == tuple(r.shape), what
    assert bool(torch.isfinite(g).all()), f"{what}: {int((~torch.isfinite(g)).sum())} non-finite elements"
    ratio = (g - r).abs() / (atol + rtol * r.abs())
    worst = int(ratio.argmax())
    msg = f"{what}: worst element {worst} got {g.reshape(-1)[worst].item():.6g} ref {r.reshape(-1)[worst].item():.6g}"
    assert ratio.reshape(-1)[worst].item() <= ceiling, msg
    assert (ratio > 1.0).float().mean().item() <= frac, msg


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_folded_weight_and_bias_match_the_f64_product(dtype):
    """Every transformer of the SD-2-depth U-Net (16 of them, C = 320 / 640 / 1280): forward weight [C][5C] =
    [W_po W_ffo | W_po] rounded once from the f32-accumulated product of the stored 16-bit weights, bias W_po b_ffo + b_po in f32."""
    from diffusionhandles_amd.unet import HipUNet
    from oracle import unet_torch as U
    ref = U.init_synthetic_(U.UNetTorch(U.SD2_DEPTH), seed=0).to(dev()).eval()
    sd = {k: v.to(dtype).float() if k.endswith(".weight") else v.float() for k, v in ref.state_dict().items()}
    hip = HipUNet(dict(U.SD2_DEPTH, text_len=77), dtype=dtype, max_batch=1)
    hip.load_state_dict(sd)
    lib = L().lib()
    n, C = ctypes.c_int(), ctypes.c_int()
    L().check(lib.dh_dbg_unet_ff_fold(hip._h, -1, ctypes.byref(n), ctypes.byref(C), None, None, L().stream_ptr()))
    # the folds in tape order: down blocks, mid block, up blocks
    prefixes = ([f"down_blocks.{i}.attentions.{j}" for i in range(3) for j in range(2)] + ["mid_block.attentions.0"] +
                [f"up_blocks.{i}.attentions.{j}" for i in range(1, 4) for j in range(3)])
    assert n.value == len(prefixes) == 16
    # (rounding once: half an ulp of the product; the f32 accumulation over C <= 1280 terms adds far less than that)
    ulp = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    for i, pre in enumerate(prefixes):
        wpo = sd[pre + ".proj_out.weight"].reshape(sd[pre + ".proj_out.weight"].shape[0], -1).double()
        wff = sd[pre + ".transformer_blocks.0.ff.net.2.weight"].double()
        bpo = sd[pre + ".proj_out.bias"].double()
        bff = sd[pre + ".transformer_blocks.0.ff.net.2.bias"].double()
        c = wpo.shape[0]
        w = torch.empty(c, 5 * c, dtype=dtype, device=dev())
        b = torch.empty(c, dtype=torch.float32, device=dev())
        L().check(lib.dh_dbg_unet_ff_fold(hip._h, i, ctypes.byref(n), ctypes.byref(C), P(w), P(b), L().stream_ptr()))
        torch.cuda.synchronize()
        assert C.value == c
        prod = wpo @ wff
        # (atol: the subnormal spacing of fp16 and the f32 accumulation error of a product near zero)
        close(w[:, : 4 * c].double(), prod, 1.01 * ulp, 2e-7 + 1e-6 * (wpo.abs() @ wff.abs()).max().item(), f"{pre} W_po W_ffo", frac=0.0, ceiling=1.0)
        assert torch.equal(w[:, 4 * c:].float(), wpo.float()), f"{pre}: the W_po block is not W_po"
        bref = wpo @ bff + bpo
        close(b.double(), bref, 1e-5, 1e-6 * (wpo.abs() @ bff.abs() + bpo.abs()).max().item(), f"{pre} folded bias", frac=0.0, ceiling=1.0)


# (rows, C) of the folded op's input-gradient GEMM: the 64x64 / 32x32 / 16x16 / 8x8 latent levels at B = 1, 2 and 8
SHAPES = [(b * hw, c) for b in (1, 2, 8) for hw, c in ((4096, 320), (1024, 640), (256, 1280), (64, 1280))]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,C", SHAPES)
def test_column_split_geglu_backward_epilogue(dtype, M, C):
    """dOut [M][C] x [W_po W_ffo | W_po] ([5C][C]): the column tiles of [0, 4C) apply the GEGLU backward to their dy and write
    d_value | d_gate (paired layout), those of [4C, 5C) write (or add to) the gradient of t2 -- NaN-poisoned outputs, every tile
    form the dispatch picks for the shape."""
    g = torch.Generator(device=dev()).manual_seed(M + C)
    lib = L().lib()
    Fd, N, K = 4 * C, 5 * C, C
    A = torch.randn(M, K, generator=g, device=dev()).to(dtype)
    W = (torch.randn(N, K, generator=g, device=dev()) / K ** 0.5).to(dtype)
    x = torch.randn(M, 2 * Fd, generator=g, device=dev()).to(dtype)
    idx = glu_paired_index(Fd).to(dev())
    xp = x[:, idx].contiguous()
    d = A.float() @ W.float().t()
    xr = x.float().requires_grad_(True)
    out = xr[:, :Fd] * F.gelu(xr[:, Fd:])
    gref, = torch.autograd.grad(out, xr, d[:, :Fd])
    tol = 4e-3 if dtype == torch.float16 else 2.5e-2
    tile = (ctypes.c_int * 9)()
    for accumulate in (0, 1):
        prior = torch.randn(M, C, generator=g, device=dev()).to(dtype)
        dt2 = prior.clone() if accumulate else poisoned((M, C), dtype)
        dxp = poisoned(xp.shape, dtype)
        L().check(lib.dh_dbg_gemm_glub_split(DT[dtype], P(A), K, P(W), M, N, K, Fd, P(dt2), C, accumulate, P(xp), P(dxp), tile,
                                             L().stream_ptr()), "dh_dbg_gemm_glub_split")
        torch.cuda.synchronize()
        bm, bn, kg, _, _, splits, pp = tile[0], tile[1], tile[2], tile[3], tile[4], tile[5], tile[6]
        assert pp == 0 and splits == 1 and kg == 1 and Fd % bn == 0, f"tile {list(tile)}"
        assert (bm, bn) in ((64, 64), (128, 128), (256, 128)), f"tile {list(tile)}"
        dx = torch.empty_like(dxp)
        dx[:, idx] = dxp
        close(dx, gref, tol, tol, f"d_value | d_gate {M}x{C} {bm}x{bn}")
        ref_t2 = d[:, Fd:] + (prior.float() if accumulate else 0.0)
        close(dt2, ref_t2, tol, tol, f"d t2 {M}x{C} {bm}x{bn} accumulate={accumulate}")
