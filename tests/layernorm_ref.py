"""float64 references, input families, gates and the case table for the LayerNorm and GEGLU kernels (csrc/unet_kernels.hip: k_ln_fwd,
k_ln_bwd, k_geglu_fwd, k_geglu_bwd).  Pure torch on CPU or GPU tensors; nothing here calls the library.

Everything is computed in float64 from the ROUNDED operands the kernels read: the 16-bit x, dy, add and the f32 gamma, beta, eps.

Gates (derived, not fitted; they are stated here and nowhere else):

  16-bit outputs y, dx      ulp16(ref) + 2^-20 mag
      ulp16(ref): half a unit in the last place of the storage type for the one rounding of the f32 result, and half for an f32
      error that moves the result across a rounding boundary.  2^-20 mag: sixteen f32 roundings (2^-24 each) of the magnitudes of the
      terms the result is summed from -- the 8 NCH deep lane sum and the six-level wave tree average out far below their worst case,
      the products, the subtraction of the mean and the final multiply-adds are a handful.  mag is
          mag_y  = rstd |gamma| (|x| + |mean|) + |beta|
          mag_dx = rstd (|d| + mean|d| + |xhat| mean|d xhat|) + |add|,      d = dy gamma.
  mean                      2^-20 (|mean| + mean|x|)       the same sixteen roundings of an average of |x|
  rstd                      2^-18 relative                  the approximate rsqrtf (1 ulp of f32 and a bit) and the variance sum
  GEGLU y, d_value, d_gate  ulp16(ref) + 1e-6 (1 + |gate|) |factor|
      the form tests/test_engine_kernels_gpu.py holds gelu and gelu_grad to on every finite gate (gelu_parts: |error of Phi| <=
      1.5e-7, the f32 rcp and exp steps on top), multiplied by the factor the kernel multiplies gelu / gelu' with: |value| for y,
      |dy| for d_value, |dy value| for d_gate.

A plain f32 restatement of the kernels (tests/test_layernorm_ref.py) stays at about half of these gates in every family, which is the
16-bit rounding itself."""
import functools
import math
import types

import torch

from per_element import ulp16

EPS = 1e-5
LN_MAX_C = 4096                                   # csrc/unet_kernels.h LN_MAX_C
DTYPES = (torch.float16, torch.bfloat16)
FAMILIES = ("normal", "offset", "outlier", "dymean", "spike")
ADD_FORMS = ("separate", "none", "alias")         # the three ways the engine passes `add` to launch_layernorm_bwd

# (rows, C).  C: one lane active (8), a partly filled first slot (64), and for every instantiation NCH = 1, 2, 3, 8 the width that
# fills its last slot (512, 1024, 1536, 4096) and the width that puts exactly ONE lane into a slot (520, 1032, 1544).  rows >= C / 8
# (the spike family then hits every chunk of every lane slot once) and never a multiple of 4 (the forward's four-wave block has a
# ragged tail); one case per NCH has 1029 rows, above the 1024 at which the backward goes from one-wave to four-wave blocks.
SHAPES = ((3, 8), (77, 64), (1029, 64), (131, 512),
          (131, 520), (1029, 520), (131, 1024),
          (131, 1032), (1029, 1032), (515, 1536),
          (515, 1544), (1029, 1544), (515, 4096))
CASES = tuple((rows, C, family) for rows, C in SHAPES for family in FAMILIES)      # each runs in both DTYPES and all ADD_FORMS

GEGLU_F = (16, 48, 1280, 5120)                    # one 32-column block; not a multiple of 32; the SD-2 widths
GEGLU_ROWS = (1, 3, 257)
GEGLU_FAMILIES = ("normal", "wide")


def nch_of(C):
    """the NCH instantiation the launchers pick"""
    return 1 if C <= 512 else (2 if C <= 1024 else (3 if C <= 1536 else 8))


def last_slot_population(C):
    """lanes that hold a chunk in the last occupied chunk slot of a row"""
    nch = C // 8
    return nch - 64 * ((nch - 1) // 64)


def wpb_of(rows):
    """waves per block of launch_layernorm_bwd"""
    return 1 if rows <= 1024 else 4


def eps32(eps=EPS):
    return float(torch.tensor(eps, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=2)
def _draws(rows, C):
    """the unit draws every family of a shape is made from (CPU generator: the same numbers on every device)"""
    g = torch.Generator().manual_seed(1000003 * rows + C)
    n = [torch.randn(rows, C, generator=g) for _ in range(3)]
    u = torch.rand(rows, 1, generator=g)
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    return n[0], n[1], n[2], u, gamma, beta


def spike_columns(rows, C):
    r = torch.arange(rows)
    return (8 * r + r % 8) % C, (8 * (7 * r + 3) + r % 8) % C


def inputs(rows, C, family, dtype):
    """x, dy, add (16-bit), gamma, beta (f32) of one case, on the CPU"""
    n0, n1, n2, u, gamma, beta = _draws(rows, C)
    r = torch.arange(rows)
    x, dy = n0, n1
    if family == "offset":
        x = n0 + (60.0 * u - 30.0)
    elif family == "outlier":
        c1 = (13 * r + 5) % C
        c2 = (c1 + 1 + r % (C - 1)) % C
        x = n0.clone()
        x[r, c1] = 100.0
        x[r, c2] = -100.0
    elif family == "dymean":
        dy = 1.0 + 0.5 * n0 + 0.25 * n1
    elif family == "spike":
        cx, cd = spike_columns(rows, C)
        x = torch.zeros(rows, C)
        dy = torch.zeros(rows, C)
        x[r, cx] = 8.0
        dy[r, cd] = 4.0
    else:
        assert family == "normal", family
    return types.SimpleNamespace(x=x.to(dtype), dy=dy.to(dtype), add=n2.to(dtype), gamma=gamma.clone(), beta=beta.clone())


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
def reference(x, gamma, beta, eps, dy=None, add=None):
    """float64 LayerNorm over the last dimension of x [rows][C] and its input gradient.  y, mean [rows], rstd [rows], mag_y; with dy
    also dx0 = rstd (d - s1 - xhat s2), d = dy gamma, and dx = dx0 + add (= dx0 without add), each with its term magnitude."""
    X, g, b = x.double(), gamma.double(), beta.double()
    C = X.shape[1]
    mean = X.sum(dim=1, keepdim=True) / C
    xc = X - mean
    rstd = 1.0 / torch.sqrt((xc * xc).sum(dim=1, keepdim=True) / C + eps32(eps))
    xhat = xc * rstd
    o = types.SimpleNamespace(mean=mean[:, 0], rstd=rstd[:, 0], y=xhat * g + b,
                              mag_y=rstd * g.abs() * (X.abs() + mean.abs()) + b.abs(),
                              mean_abs_x=X.abs().sum(dim=1) / C)
    if dy is not None:
        d = dy.double() * g
        s1 = d.sum(dim=1, keepdim=True) / C
        s2 = (d * xhat).sum(dim=1, keepdim=True) / C
        o.dx0 = rstd * (d - s1 - xhat * s2)
        o.mag_dx0 = rstd * (d.abs() + d.abs().sum(dim=1, keepdim=True) / C + xhat.abs() * (d * xhat).abs().sum(dim=1, keepdim=True) / C)
        o.dx, o.mag_dx = o.dx0, o.mag_dx0
        if add is not None:
            o.dx, o.mag_dx = o.dx0 + add.double(), o.mag_dx0 + add.double().abs()
    return o


def gate16(ref, mag, dtype):
    return ulp16(ref, dtype) + 2.0 ** -20 * mag


def gate_mean(o):
    return 2.0 ** -20 * (o.mean.abs() + o.mean_abs_x)


def gate_rstd(o):
    return 2.0 ** -18 * o.rstd


# -------------------------------------------------------------------------------------------------------------------- GEGLU
def glu_paired_index(Fd):
    """Stored column n' of a GEGLU pre-activation tensor [rows][2F] -> column of the torch layout (value | gate): every 32-column
    block holds the 16 value columns of outputs 16b .. 16b+15, then their 16 gate columns (csrc/unet_kernels.h glu_src_row)."""
    n = torch.arange(2 * Fd)
    return ((n >> 4) & 1) * Fd + 16 * (n >> 5) + (n & 15)


def gelu64(g):
    g = g.double()
    return 0.5 * g * torch.erfc(-g / math.sqrt(2.0))                      # = 0.5 g (1 + erf(g / sqrt 2)), without its cancellation at g << 0


def gelu_grad64(g):
    g = g.double()
    return 0.5 * torch.erfc(-g / math.sqrt(2.0)) + g * torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)


def geglu_inputs(rows, Fd, family, dtype):
    """x [rows][2F] in the torch order (value | gate) and dy [rows][F], 16-bit, on the CPU"""
    g = torch.Generator().manual_seed(7919 * rows + Fd)
    x = torch.randn(rows, 2 * Fd, generator=g)
    dy = torch.randn(rows, Fd, generator=g)
    if family == "wide":                          # |value| up to 200, gate over [-12, 12]: both tails of Phi, large products
        u = torch.rand(rows, 2 * Fd, generator=g)
        x = torch.cat([400.0 * u[:, :Fd] - 200.0, 24.0 * u[:, Fd:] - 12.0], dim=1)
    else:
        assert family == "normal", family
    return x.to(dtype), dy.to(dtype)


def geglu_reference(x, dy, dtype):
    """float64 y = value gelu(gate), d_value = dy gelu(gate), d_gate = dy value gelu'(gate) in the torch column order, with their gates"""
    Fd = x.shape[1] // 2
    h, g, d = x[:, :Fd].double(), x[:, Fd:].double(), dy.double()
    o = types.SimpleNamespace(y=h * gelu64(g), d_value=d * gelu64(g), d_gate=d * h * gelu_grad64(g))
    room = 1e-6 * (1.0 + g.abs())
    o.gate_y = ulp16(o.y, dtype) + room * h.abs()
    o.gate_d_value = ulp16(o.d_value, dtype) + room * d.abs()
    o.gate_d_gate = ulp16(o.d_gate, dtype) + room * (d * h).abs()
    return o
