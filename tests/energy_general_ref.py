"""Float64 reference of ONE layer of the guidance energy as the general entry (dh_energy_fwd_bwd) computes it, and the cases
tests/test_energy_general_ref.py (CPU) and tests/test_energy_general_gpu.py (MI355X) share.  Plain torch, written for these
tests: nothing here calls into the product or into oracle/.

  resize      F.interpolate(mode="bilinear") of both maps to the cell grid
  A           avg_pool2d(w F) / (avg_pool2d(w) + 1e-10), w = indicator of the cells the index lists name
  pair term   mean_c mean_n | A1[c, o_n] - A2[c, t_n] |, duplicates kept (fg: the pairs; local_avg: identity pairs of bg_both)
  global_avg  mean_c | mean_{bg_orig} F1[c] - mean_{bg_trans} F2[c] |
  gradient    torch.autograd.grad of fg_w fg + bg_w bg with respect to the current map, at the INPUT size

An L1 gradient is a sum of signs.  `layer` therefore also returns, per gradient element, the smallest |d| over the
differences whose sign enters that element (inf where none does): for a pair term the pair differences of the target cells
that feed the element through the pooling window and the resize, for global_avg the channel's mean difference.  Where that
is below tau the f32 kernel may choose the other sign and the comparison leaves the element out.
"""
import zlib

import numpy as np
import scipy.ndimage
import torch
import torch.nn.functional as F

INF = float("inf")
CELL_PX = 8          # pixels per grid cell of every case: img_res = 8 grid (512 at grid 64, 768 at grid 96)


# ---- the reference ----------------------------------------------------------------------------------------------------
def cells_from_correspondences(corr, img_res, bg_erosion, grid):
    """[N,4] (ox, oy, tx, ty) pixel rows -> the ten int64 index arrays of process_correspondences, duplicates kept."""
    c = np.asarray(corr, dtype=np.int64).reshape(-1, 4)
    c = c[(c[:, 2] >= 0) & (c[:, 2] < img_res) & (c[:, 3] >= 0) & (c[:, 3] < img_res)] // (img_res // grid)
    bg_o, bg_t = np.ones((grid, grid), dtype=bool), np.ones((grid, grid), dtype=bool)
    bg_o[c[:, 1], c[:, 0]] = False
    bg_t[c[:, 3], c[:, 2]] = False
    if bg_erosion > 0:
        bg_o = scipy.ndimage.binary_erosion(bg_o, iterations=bg_erosion)
        bg_t = scipy.ndimage.binary_erosion(bg_t, iterations=bg_erosion)
    out = {"original_x": c[:, 0], "original_y": c[:, 1], "transformed_x": c[:, 2], "transformed_y": c[:, 3]}
    for key, m in (("", bg_o & bg_t), ("_orig", bg_o), ("_trans", bg_t)):
        out["background_y" + key], out["background_x" + key] = np.nonzero(m)
    return out


def resize_matrix(n_in, n_out):
    """[n_out, n_in] float64: row y holds the weights with which output y of the bilinear resize reads the inputs."""
    return F.interpolate(torch.eye(n_in, dtype=torch.float64)[None], n_out, mode="linear")[0].T.contiguous()


def _idx(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int64)


def _pair_term(f1, f2, y1, x1, y2, x2, patch):
    """-> (loss, min |d| per cell of f2 [C,g,g]: over the pairs whose target lies in the cell's pooling window)."""
    C, g, _ = f1.shape
    w1, w2 = torch.zeros((g, g), dtype=f1.dtype), torch.zeros((g, g), dtype=f1.dtype)
    w1[y1, x1] = 1
    w2[y2, x2] = 1
    pool = lambda t: F.avg_pool2d(t, patch, stride=1, padding=patch // 2)
    a1 = pool((w1 * f1)[None])[0] / (pool(w1[None, None])[0] + 1e-10)
    a2 = pool((w2 * f2)[None])[0] / (pool(w2[None, None])[0] + 1e-10)
    d = a1[:, y1, x1] - a2[:, y2, x2]
    mind = torch.full((C, g * g), INF, dtype=f1.dtype)
    mind.scatter_reduce_(1, (y2 * g + x2)[None].expand(C, -1), d.detach().abs(), "amin")
    mind = mind.view(C, g, g)
    if patch > 1:
        mind = -F.max_pool2d(-mind[None], patch, stride=1, padding=patch // 2)[0]
    return d.abs().mean(dim=-1).mean(), torch.where(w2.bool()[None], mind, torch.full_like(mind, INF))


def _min_over_readers(m, Wy, Wx):
    """[C,g,g] on the grid -> [C,h,w]: the minimum over the grid cells that read the input cell with a non-zero weight."""
    def fold(t, W, dim):
        cols = []
        for i in range(W.shape[1]):
            sel = t.index_select(dim, torch.nonzero(W[:, i] > 0)[:, 0])
            cols.append(sel.amin(dim) if sel.shape[dim] else torch.full_like(t.select(dim, 0), INF))
        return torch.stack(cols, dim)
    return fold(fold(m, Wy, 1), Wx, 2)


def layer(cur, org, cells, fg_w, bg_w, grid, fg_patch=1, bg_patch=1, bg_mode="global_avg"):
    """cur / org [h,w,C] (any dtype, read as float64) -> dict:
    loss [3] = (fg_w fg + bg_w bg, fg, bg); grad [h,w,C] = d loss[0] / d cur; grad_grid [grid,grid,C] the same with respect
    to the resized map; min_d [h,w,C]; global_d [C] = |mean difference| per channel (None without a global_avg term)."""
    a = cur.detach().double().permute(2, 0, 1).clone().requires_grad_(True)
    f2 = F.interpolate(a[None], (grid, grid), mode="bilinear")[0]
    f1 = F.interpolate(org.detach().double().permute(2, 0, 1)[None], (grid, grid), mode="bilinear")[0]
    C = a.shape[0]
    zero = (f2 * 0).sum()
    fg, bg, global_d = zero, zero, None
    mind = torch.full((C, grid, grid), INF, dtype=torch.float64)
    oy, ox, ty, tx = (_idx(cells[k]) for k in ("original_y", "original_x", "transformed_y", "transformed_x"))
    if oy.numel():
        fg, m = _pair_term(f1, f2, oy, ox, ty, tx, fg_patch)
        if fg_w != 0:
            mind = torch.minimum(mind, m)
    if bg_mode == "global_avg":
        byo, bxo, byt, bxt = (_idx(cells[k]) for k in ("background_y_orig", "background_x_orig", "background_y_trans",
                                                       "background_x_trans"))
        if byo.numel() and byt.numel():
            dm = f1[:, byo, bxo].mean(dim=-1) - f2[:, byt, bxt].mean(dim=-1)
            bg, global_d = dm.abs().mean(), dm.detach().abs()
            if bg_w != 0:
                m = torch.full((C, grid, grid), INF, dtype=torch.float64)
                m[:, byt, bxt] = global_d[:, None]
                mind = torch.minimum(mind, m)
    elif bg_mode == "local_avg":
        by, bx = _idx(cells["background_y"]), _idx(cells["background_x"])
        if by.numel():
            bg, m = _pair_term(f1, f2, by, bx, by, bx, bg_patch)
            if bg_w != 0:
                mind = torch.minimum(mind, m)
    else:
        raise ValueError(bg_mode)
    total = fg_w * fg + bg_w * bg
    g_in, g_grid = torch.autograd.grad(total, [a, f2], allow_unused=True)
    g_in = torch.zeros_like(a) if g_in is None else g_in
    g_grid = torch.zeros_like(f2) if g_grid is None else g_grid
    h, w = a.shape[1:]
    min_d = _min_over_readers(mind, resize_matrix(h, grid), resize_matrix(w, grid))
    return dict(loss=torch.stack([total, fg, bg]).detach(), grad=g_in.permute(1, 2, 0).contiguous(),
                grad_grid=g_grid.permute(1, 2, 0).contiguous(), min_d=min_d.permute(1, 2, 0).contiguous(),
                min_d_grid=mind.permute(1, 2, 0).contiguous(), global_d=global_d)


# ---- the comparison rule ------------------------------------------------------------------------------------------------
MAX_BELOW_TAU = 1e-4         # cap on the share of a call's sign-sum elements (the gradient on the cell grid) that may flip


def tau(cur, org):
    """2^-18 max|input|: about 15 f32 roundings of the largest operand (four taps, nine pooled cells, the subtraction)."""
    return 2.0 ** -18 * max(float(cur.abs().max()), float(org.abs().max()))


def excluded(case, ref, t):
    """The elements of the returned gradient the comparison leaves out: those a difference below tau enters.  None where
    the signs are certain: every resized value and every pair difference is exact in f32 there, so a tie is a tie on both
    sides (sign 0) and no other sign can flip."""
    return torch.zeros_like(ref["min_d"], dtype=torch.bool) if case.certain else ref["min_d"] < t


def check_caps(case, call, ref, t):
    """The conditions under which a call may be compared at all -> (share of the sign sums on the grid that a difference
    below tau enters, share of the returned gradient's elements that is left out).  The cap is on the first: that is where
    a sign is decided, one element per (cell, channel).  The resize adjoint then carries each such element to every input
    cell its grid cell reads -- 16 at the ratio 1/2, some 650 at 5 -> 64 -- so the second share is larger by about that
    count, whatever the inputs; it is reported, and it is what the GPU comparison skips."""
    on_grid = 0.0 if case.certain else float((ref["min_d_grid"] < t).double().mean())
    left_out = float(excluded(case, ref, t).double().mean())
    assert on_grid <= MAX_BELOW_TAU, f"{case.id} {call.name}: {on_grid:.3g} of the sign sums on the grid lie below tau"
    if call.bg_mode == "global_avg" and call.bg_w != 0 and ref["global_d"] is not None:
        low = float(ref["global_d"].min())      # (a mean is not exact in f32 in any case: this cap holds for all of them)
        assert low >= t, (f"{case.id} {call.name}: a channel's global_avg mean difference is {low:.3g}, below tau = {t:.3g}: "
                          f"one flipped channel moves every bg_trans cell, choose another seed")
    return on_grid, left_out


# ---- the cases ----------------------------------------------------------------------------------------------------------
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
TYPES = {"f16": (F16, F16), "bf16": (BF16, BF16), "bf16_f32": (BF16, F32), "f32": (F32, F32)}
GRAD_SCALE = 256.0           # keeps an fp16 gradient out of the subnormals
STORAGE_ULP = {F16: 2.0 ** -10, BF16: 2.0 ** -7, F32: 0.0}


# Another draw for the cases whose first one breaks a cap of check_caps (tests/test_energy_general_ref.py says which): a
# channel mean within tau with few channels or one input cell, or a share of the sign sums just above 1e-4.
SALT = {
    "terms-5x5to64-C320-f16-window-p1-e0": 1,              # a global_avg channel mean below tau
    "terms-8x8to64-C8-f16-window-p1-e0": 1,                # the same
    "terms-32x32to64-C72-f16-image-p1-e0": 1,              # the same
    "exact-1x1to64-C72-f16-image-p1-e0": 2,                # the same: one input cell, a channel of cur equal to org's
    "exact-1x1to64-C320-f32-image-p1-e0": 10,              # the same
    "terms-5x5to64-C320-bf16_f32-window-p1-e0": 1,         # local_avg: 1.17e-4 of the sign sums below tau
    "terms-8x8to64-C72-f32-image2k-p3-e0": 1,              # fg: 1.29e-4
}


class Call:
    def __init__(self, name, fg_w, bg_w, bg_mode="global_avg"):
        self.name, self.fg_w, self.bg_w, self.bg_mode = name, fg_w, bg_w, bg_mode


class Case:
    """One (shape, C, types, patch, correspondence set) and the calls made on it."""

    def __init__(self, kind, shape, C, types, pairs, patch=1, erosion=0, exact=False):
        self.kind, self.C, self.types, self.pairs, self.patch, self.erosion, self.exact = kind, C, types, pairs, patch, erosion, exact
        self.h, self.w, self.grid = shape
        self.in_dtype, self.grad_dtype = TYPES[types]
        self.img_res = CELL_PX * self.grid
        # signs that cannot flip: the exact cases, and maps already at the grid with patch 1 -- the kernel then subtracts the
        # inputs themselves, and the sign of a correctly rounded difference is the sign of the difference (16-bit inputs tie
        # in about 1e-4 of all pairs at fp16 and 8e-4 at bf16: exact ties, sign 0 on both sides)
        self.certain = exact or (self.h == self.w == self.grid and patch == 1)
        self.id = f"{'exact' if exact else kind}-{self.h}x{self.w}to{self.grid}-C{C}-{types}-{pairs}-p{patch}-e{erosion}"
        self.seed = zlib.crc32(self.id.encode()) + SALT.get(self.id, 0)

    def inputs(self):
        """(cur, org) [h,w,C] in the input dtype, on the CPU.  randn; the exact cases: multiples of 1/8 in [-4, 4]."""
        gen = torch.Generator().manual_seed(self.seed)
        if self.exact:
            draw = lambda: torch.randint(-32, 33, (self.h, self.w, self.C), generator=gen).double() / 8
        else:
            draw = lambda: torch.randn(self.h, self.w, self.C, generator=gen)
        return draw().to(self.in_dtype), draw().to(self.in_dtype)

    def correspondences(self):
        """The [N,4] int64 pixel rows of each call of the case: a list of (label, rows)."""
        gen = torch.Generator().manual_seed(self.seed ^ 0x5EED)
        res, g = self.img_res, self.grid
        if self.pairs == "window":          # 3000 pairs with duplicates inside a 40 x 40 pixel window
            return [("window", torch.stack([torch.randint(100, 140, (3000,), generator=gen) for _ in range(4)], dim=-1))]
        if self.pairs == "image":           # 3000 pairs over the whole image
            return [("image", torch.randint(0, res, (3000, 4), generator=gen))]
        if self.pairs == "image2k":         # 2000: patch 3 puts nine cells' differences into a sign sum, and 2000 pairs keep
            return [("image2k", torch.randint(0, res, (2000, 4), generator=gen))]      # both pooled terms near 5e-5 below tau
        if self.pairs == "none":
            return [("none", torch.zeros((0, 4), dtype=torch.int64))]
        if self.pairs == "single":          # one pair per call; the target cell at each border clamp and in the middle
            src = CELL_PX * torch.tensor([g // 3, g // 2]) + 3
            cells = [(0, 0), (0, g - 1), (g - 1, 0), (g - 1, g - 1), (far_reader(self.h, g), far_reader(self.w, g))]
            return [(f"target({y},{x})", torch.tensor([[int(src[0]), int(src[1]), CELL_PX * x + 5, CELL_PX * y + 2]]))
                    for y, x in cells]
        raise ValueError(self.pairs)

    def calls(self):
        if self.kind == "footprint":
            return [Call("fg", 1.0, 0.0)]
        if self.kind == "background":
            return [Call("bg_global", 0.0, 1.0), Call("bg_local", 0.0, 1.0, "local_avg")]
        if self.patch > 1:                  # patch 3 is a matter of the pooled terms: fg and local_avg
            return [Call("fg", 1.0, 0.0), Call("bg_local", 0.0, 1.0, "local_avg")]
        return [Call("fg", 1.0, 0.0), Call("bg_global", 0.0, 1.0), Call("bg_local", 0.0, 1.0, "local_avg"),
                Call("mixed", 3.0, 2.0)]


def far_reader(n_in, grid):
    """The last grid row that reads input row n_in // 2 - 1 (row 0 of a one-row input) with a non-zero weight: the reader
    farthest from its source row, where a gather window of the adjoint that is too narrow shows first."""
    W = resize_matrix(n_in, grid)
    return int(torch.nonzero(W[:, max(n_in // 2 - 1, 0)] > 0)[-1])


CONTROL, PRODUCT, PRODUCT96, EDGE = (64, 64, 64), (32, 32, 64), (48, 48, 96), (16, 16, 64)
BELOW = [(8, 8, 64), (16, 16, 96), (5, 5, 64)]              # ratios below 1/4
NONSQUARE, DOWN, ONE = (16, 32, 64), (128, 128, 64), (1, 1, 64)
SHAPES = [CONTROL, PRODUCT, PRODUCT96, EDGE] + BELOW + [NONSQUARE, DOWN, ONE]
DYADIC = [CONTROL, PRODUCT, PRODUCT96, EDGE, (8, 8, 64), NONSQUARE, DOWN, ONE]


def _cases():
    out = []
    # the three terms and the mix, patch 1, the 40 x 40 window: every shape at fp16 and at f32, every C at every type
    wide = {PRODUCT96: 72, DOWN: 72}
    for s in SHAPES:
        out.append(Case("terms", s, wide.get(s, 320), "f16", "window"))
        out.append(Case("terms", s, 72, "f32", "window"))
    out += [Case("terms", s, C, "f16", "window") for s in (PRODUCT, (8, 8, 64)) for C in (8, 72)]
    out += [Case("terms", PRODUCT96, 8, "f16", "window")]
    out += [Case("terms", s, C, "f32", "window") for s in (PRODUCT, (5, 5, 64)) for C in (8, 320)]
    out += [Case("terms", PRODUCT, C, t, "window") for t in ("bf16", "bf16_f32") for C in (8, 72, 320)]
    out += [Case("terms", (8, 8, 64), 320, "bf16", "window"), Case("terms", PRODUCT96, 72, "bf16", "window"),
            Case("terms", NONSQUARE, 8, "bf16", "window"), Case("terms", (16, 16, 96), 72, "bf16_f32", "window"),
            Case("terms", DOWN, 8, "bf16_f32", "window"), Case("terms", (5, 5, 64), 320, "bf16_f32", "window")]
    # pairs over the whole image
    for s in [PRODUCT, PRODUCT96, EDGE] + BELOW:
        out.append(Case("terms", s, 72, "f16", "image"))
        out.append(Case("terms", s, 8 if s == PRODUCT96 else 320, "f32", "image"))
    # patch 3, on the product's ratio and below the old window's edge
    for s in (PRODUCT, (8, 8, 64)):
        out += [Case("terms", s, C, t, "image2k", patch=3) for C, t in ((320, "f16"), (72, "f32"), (8, "bf16"), (72, "bf16_f32"))]
    # exact: dyadic ratio, patch 1, inputs on a 1/8 lattice; nothing may be left out
    for k, s in enumerate(DYADIC):
        for j, t in enumerate(("f16", "f32", "bf16", "bf16_f32")):
            C = (8, 72, 320)[(k + j) % 3]
            if j < 2 or s in (PRODUCT, (8, 8, 64), EDGE):
                out.append(Case("terms", s, 72 if (C == 320 and s in wide) else C, t, "image", exact=True))
    # one pair: the bare footprint of the resize adjoint at each border clamp and at the far end of a reader range
    for s in SHAPES:
        out.append(Case("footprint", s, 8, "f16", "single"))
        out.append(Case("footprint", s, 72, "f32", "single"))
    out += [Case("footprint", s, 320, "bf16", "single") for s in BELOW]
    # background alone: no pairs, and the window's pairs, under erosion 0 and 5
    for s, C, t in ((PRODUCT, 320, "f16"), ((8, 8, 64), 72, "f32"), ((16, 16, 96), 8, "bf16"), (PRODUCT96, 72, "bf16_f32")):
        out += [Case("background", s, C, t, "none", erosion=e) for e in (0, 5)]
        out.append(Case("background", s, C, t, "window", erosion=5))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), "duplicate case"
    return out


CASES = _cases()
