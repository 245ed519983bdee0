"""Per-element comparison against an fp64 reference (pure torch, CPU or GPU tensors): the spacing of a 16-bit storage format at the
reference's magnitude (ulp16) and the assertion that every element lies within its own tolerance (within).  Shared by the GPU parity
tests and by the CPU tests of their references."""
import torch

MANT = {torch.float16: 10, torch.bfloat16: 7}               # stored mantissa bits
EMIN = {torch.float16: -14, torch.bfloat16: -126}           # exponent of the smallest normal number


def ulp16(ref, dtype):
    """spacing of `dtype` at the magnitude of every element of ref (fp64); the subnormal spacing below the smallest normal"""
    a = ref.double().abs()
    _, e = torch.frexp(a)                                   # |ref| = m 2^e, m in [0.5, 1)
    e = torch.where(a > 0, e - 1, torch.full_like(e, EMIN[dtype])).clamp(min=EMIN[dtype])
    return torch.ldexp(torch.ones_like(a), e - MANT[dtype])


def within(got, ref, tol, what):
    """every element of got finite and within tol (a tensor) of ref (fp64); the message names the worst element"""
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)} != reference {tuple(ref.shape)}"
    g, r = got.double(), ref.double()
    tol = torch.as_tensor(tol, dtype=torch.float64, device=r.device).expand_as(r)
    nonfin = ~torch.isfinite(g)
    ratio = torch.where(nonfin, torch.full_like(r, float("inf")), (g - r).abs() / tol)
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), ratio.shape))
    wr = ratio.reshape(-1)[worst].item()
    print(f"{what}: worst {wr:.3g} x tolerance")
    assert int(nonfin.sum()) == 0 and wr <= 1.0, (
        f"{what}: worst element {idx} got {g.reshape(-1)[worst].item():.9g} ref {r.reshape(-1)[worst].item():.9g} "
        f"({wr:.3g} x tolerance {tol.reshape(-1)[worst].item():.3g}), non-finite {int(nonfin.sum())}, "
        f"over tolerance {int((ratio > 1.0).sum())} of {ratio.numel()}")
