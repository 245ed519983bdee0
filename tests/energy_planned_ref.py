"""Float64 reference of ONE item of the planned guidance energy (dh_energy_fwd_bwd_planned, _objects, _donor and their batch
entries: k_colsum_q, then k_energy_grad or one of its _obj / _donor / _batch variants), and the cases that
tests/test_energy_planned_ref.py (CPU) and tests/test_energy_planned_gpu.py (MI355X) share.  Plain torch / NumPy, written for
these tests: nothing here calls into the product or into oracle/.

The planned path reads 16-bit maps that are already at the cell grid, with patch 1.  The sign of every pair difference is then
decided exactly (an IEEE subtraction of two 16-bit values has the right sign and is zero only on equality), so an element of
the gradient is an integer sign sum times a coefficient:

  grad[cell, c] = -(sum_m c_m S_m[cell, c]) - c_bg sgn_c [cell in bg_trans]
  S_m    integer sum of sign(src - cur) over the item's pairs of object m that target the cell; duplicates kept, sign(0) = 0
  c_m    fg_w omega_m / (C N_m); unweighted: one object with omega = 1
  omega  w_m / sum of the weights of the objects that have pairs
  src    a row of the donor map where the object's donor bit is set, of orig otherwise
  c_bg   bg_w / (C n_trans);  sgn_c = sign(mean_{bg_orig} orig - mean_{bg_trans} cur)

No element is left out of the comparison: the one sign that is not exact, sgn_c, is made certain by the inputs (every case
holds global_d.min() >= 2^-10, tests/test_energy_planned_ref.py).  DESIGN.md section 32.
"""
import functools
import zlib

import numpy as np
import torch

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
TYPES = {"f16": (F16, F16), "bf16": (BF16, BF16), "f16_f32": (F16, F32), "bf16_f32": (BF16, F32), "f16_bf16": (F16, BF16),
         "bf16_f16": (BF16, F16)}
COLSUM_S = 128               # slices of a background list in k_colsum_q
GLOBAL_D_MIN = 2.0 ** -10    # the condition on the inputs: every channel's |mean difference|
PAIR_KEYS = ("original_y", "original_x", "transformed_y", "transformed_x")


# ---- the reference ----------------------------------------------------------------------------------------------------
def entries(cells, grid):
    """The distinct (object, target cell, source cell) rows of an item's pairs in ascending order, and their multiplicities."""
    g = grid
    s = np.asarray(cells["original_y"], dtype=np.int64) * g + np.asarray(cells["original_x"], dtype=np.int64)
    t = np.asarray(cells["transformed_y"], dtype=np.int64) * g + np.asarray(cells["transformed_x"], dtype=np.int64)
    obj = np.asarray(cells["object"], dtype=np.int64) if "object" in cells else np.zeros_like(s)
    if s.size == 0:
        return np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.unique(np.stack([obj, t, s], axis=1), axis=0, return_counts=True)


def item(cur, org, cells, fg_w, bg_w, grid, weights=None, donor=None, donor_bits=0):
    """cur / org / donor [g,g,C] (any dtype, read as float64); cells: the index arrays of process_correspondences (plus "object"
    for a weighted item); weights: one per object, None for the unweighted item -> dict:
    grad [g,g,C]; mag [g,g,C] = sum of the magnitudes of the terms of each element; loss [3] = (fg_w fg + bg_w bg, fg, bg);
    global_d [C] = |mean difference| per channel (None without a background term); seg [g*g] = distinct (object, source)
    entries per target cell."""
    g, C = grid, cur.shape[-1]
    G2 = g * g
    a, o = cur.detach().double().reshape(G2, C), org.detach().double().reshape(G2, C)
    dn = None if donor is None else donor.detach().double().reshape(G2, C)
    keys, mult = entries(cells, g)
    n = int(mult.sum())
    w = np.asarray([1.0] if weights is None else weights, dtype=np.float64)
    counts = np.bincount(keys[:, 0], weights=mult, minlength=len(w)).astype(np.int64)
    assert len(counts) == len(w), "a pair of an object without a weight"
    live = counts > 0
    omega = np.where(live, w / w[live].sum(), 0.0) if n else np.zeros_like(w)
    grad, mag = torch.zeros((G2, C), dtype=torch.float64), torch.zeros((G2, C), dtype=torch.float64)
    fg = 0.0
    for m in np.nonzero(live)[0]:
        sel = keys[:, 0] == m
        tm, sm = torch.from_numpy(keys[sel, 1]), torch.from_numpy(keys[sel, 2])
        mu = torch.from_numpy(mult[sel]).double()[:, None]
        src = dn if (int(donor_bits) >> int(m)) & 1 else o
        d = src[sm] - a[tm]
        S = torch.zeros((G2, C), dtype=torch.float64).index_add_(0, tm, mu * torch.sign(d))      # integers: exact
        c_m = float(fg_w) * omega[m] / (C * counts[m])
        grad -= c_m * S
        mag += abs(c_m) * S.abs()
        fg += omega[m] / (C * counts[m]) * float((mu * d.abs()).sum())
    b1 = np.asarray(cells["background_y_orig"], dtype=np.int64) * g + np.asarray(cells["background_x_orig"], dtype=np.int64)
    b2 = np.asarray(cells["background_y_trans"], dtype=np.int64) * g + np.asarray(cells["background_x_trans"], dtype=np.int64)
    bg, global_d = 0.0, None
    if b1.size and b2.size:
        dm = o[torch.from_numpy(b1)].mean(dim=0) - a[torch.from_numpy(b2)].mean(dim=0)
        global_d = dm.abs()
        bg = float(global_d.mean())
        c_bg = float(bg_w) / (C * b2.size)
        flag = torch.zeros(G2, dtype=torch.float64)
        flag[torch.from_numpy(b2)] = 1.0
        grad -= c_bg * flag[:, None] * torch.sign(dm)[None]
        mag += abs(c_bg) * flag[:, None] * torch.sign(dm).abs()[None]
    seg = np.bincount(keys[:, 1], minlength=G2)
    loss = torch.tensor([float(fg_w) * fg + float(bg_w) * bg, fg, bg], dtype=torch.float64)
    return dict(grad=grad.view(g, g, C), mag=mag.view(g, g, C), loss=loss, global_d=global_d, seg=seg)


# ---- the cell lists of the cases ----------------------------------------------------------------------------------------
MULTS = (1, 2, 64, 300)                              # 300: a raw segment longer than k_dedupe_sources' 256 threads
DISTINCT = (1, 7, 8, 9, 15, 16, 17, 24, 41)          # distinct sources of the hand-made target cells (0: every other cell)
# the hand-made weighted layout: per target cell the (object, distinct sources) runs of its segment, in segment order
OBJECT_RUNS = (
    tuple((m, 1) for m in range(8)),                 # 8 entries of 8 different objects: a fold at every step of the 8-wide loop
    ((0, 8), (1, 3)),                                # the object changes between entries 7 and 8: at the first step of the tail
    ((0, 8), (1, 8), (2, 1)),                        # ... and at step 0 of a second 8-wide batch
    ((1, 3), (2, 7)),                                # the segment starts with an object other than 0; a change inside the batch
    ((0, 9), (3, 1), (4, 1)),                        # changes inside the tail
    ((7, 1),),                                       # one entry, of the last object
)
WEIGHTS = {"mix": (7.5, 1.5), "fg": (7.5, 0.0), "bg": (0.0, 1.5), "cancel": (6.4, 10.0)}
CANCEL_PAIRS, CANCEL_TRANS = 64, 100                 # fg_w / N = 6.4 / 64 = bg_w / n_trans = 10 / 100: the two terms cancel


def _spread(k, G2):
    """k distinct cells from 0 to G2 - 1, both included"""
    return [round(i * (G2 - 1) / max(k - 1, 1)) for i in range(k)]


def _with(cellset, special):
    if special not in cellset:
        cellset[0] = special
    return cellset


@functools.lru_cache(maxsize=None)
def cell_lists(grid, pairs, bg, M, dead=()):
    """The index arrays of one item: pair set `pairs`, background lists of bg = (n_orig, n_trans) distinct cells, the objects of
    the pairs among M (0: no "object" key); dead: objects that get no pair."""
    g, G2 = grid, grid * grid
    rng = np.random.default_rng(zlib.crc32(f"{grid}-{pairs}-{bg}-{M}-{dead}".encode()))
    s, t, ob = [], [], []
    objects = max(M, 1)

    def add(tc, sc, m, mult):
        m = m % objects
        if m in dead:
            return
        s.extend([sc] * mult), t.extend([tc] * mult), ob.extend([m] * mult)

    if pairs == "hand":
        counts = [d for d in DISTINCT if d <= G2 - 1]
        for i, (tc, d) in enumerate(zip(_spread(len(counts), G2), counts)):
            srcs = list(rng.permutation(G2)[:d])
            srcs = _with(srcs, G2 - 1) if i == 0 else _with(srcs, 0) if i == len(counts) - 1 else srcs
            for j, sc in enumerate(sorted(srcs)):
                add(tc, int(sc), j * objects // d, MULTS[(i + j) % 4])
    elif pairs == "objects":
        for i, (tc, runs) in enumerate(zip(_spread(len(OBJECT_RUNS), G2), OBJECT_RUNS)):
            srcs = iter(rng.permutation(G2)[:sum(k for _, k in runs)])
            for j, (m, k) in enumerate(runs):
                for q in range(k):
                    add(tc, int(next(srcs)), m, MULTS[(i + j + q) % 4] if q < 2 else 1)
        hand = set(_spread(len(OBJECT_RUNS), G2))
        free = np.array([c for c in range(G2) if c not in hand])
        for sc, tc, m in zip(rng.integers(0, G2, 500), free[rng.integers(0, free.size, 500)], rng.integers(0, objects, 500)):
            add(int(tc), int(sc), int(m), 1)
    elif pairs == "random":
        for sc, tc, m in zip(rng.integers(0, G2, 3000), rng.integers(0, G2, 3000), rng.integers(0, objects, 3000)):
            add(int(tc), int(sc), int(m), 1)
    elif pairs == "one":
        add(G2 // 3, G2 // 2, 0, 1)
    elif pairs == "cancel":                          # one pair into each of 64 cells that also lie in bg_trans
        for tc, sc in zip(rng.permutation(G2)[:CANCEL_PAIRS], rng.integers(0, G2, CANCEL_PAIRS)):
            add(int(tc), int(sc), 0, 1)
    elif pairs != "none":
        raise ValueError(pairs)
    order = rng.permutation(len(s))                  # the build sees the pairs in no particular order
    s, t, ob = (np.asarray(v, dtype=np.int64)[order] for v in (s, t, ob))
    n1, n2 = bg
    b1, b2 = rng.permutation(G2)[:n1].astype(np.int64), rng.permutation(G2)[:n2].astype(np.int64)
    if pairs == "cancel":
        rest = np.setdiff1d(np.arange(G2), t)
        b2 = rng.permutation(np.concatenate([np.unique(t), rng.permutation(rest)[:n2 - np.unique(t).size]]))
    both = np.intersect1d(b1, b2)
    out = {"original_y": s // g, "original_x": s % g, "transformed_y": t // g, "transformed_x": t % g,
           "background_y": both // g, "background_x": both % g, "background_y_orig": b1 // g, "background_x_orig": b1 % g,
           "background_y_trans": b2 // g, "background_x_trans": b2 % g}
    if M:
        out["object"] = ob
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------
# Another draw for a case whose first one breaks the global_d condition (tests/test_energy_planned_ref.py says which).
SALT = {
    "g5-C320-bf16-random-bg3x25-bg-s256": 7,
    "g16-C1280-f16-random-bg100x129-mix-s256": 2,
    "g16-C1280-bf16-hand-bg128x100-mix-s256": 3,
    "g8-C2048-f16-hand-bg64x33-mix-s256": 17,
    "g8-C2048-bf16-random-bg20x64-mix-s256": 82,
    "g32-C320-bf16_f16-hand-bg1000x128-mix-s256": 1,
    "g32-C320-bf16-none-bg1000x1-mix-s256": 1,
    "g16-C72-f16-objects-bg129x100-mix-s256-M8": 1,
    "g16-C72-f16-random-bg100x128-mix-s256-M1-donor_all": 1,
    "g16-C72-bf16_f16-hand-bg100x128-mix-s256-M2-donor_all": 1,
    "g32-C320-f16-random-bg1000x129-mix-s256-M2": 1,
    "g32-C320-bf16-objects-bg1000x129-mix-s256-M8": 1,
    "g32-C320-bf16-one-bg100x1-mix-s256-M2": 2,
    "g32-C320-f16_f32-objects-bg1000x129-mix-s1-M8": 1,
    "g32-C320-f16-none-bg100x128-mix-s256-item0": 4,
    "g32-C320-f16-one-bg1x128-bg-s256-item3": 1,
    "g32-C320-f16-none-bg100x128-mix-s256-item8": 2,
    "g32-C320-f16-hand-bg128x129-mix-s32-item12": 1,
    "g32-C320-f16-random-bg100x1-fg-s512-item14": 1,
    "g32-C320-f16-hand-bg129x128-bg-s1024-item15": 1,
    "g16-C72-bf16-random-bg129x100-mix-s128-M8-item2": 1,
    "g16-C72-bf16-cancel-bg128x100-cancel-s256-M1-item13": 1,
    "g32-C320-f16-random-bg129x100-mix-s128-M8-item2": 2,
    "g32-C320-f16-hand-bg128x129-mix-s32-M2-item4": 2,
    "g32-C320-f16-cancel-bg128x100-cancel-s256-M1-item5": 1,
    "g32-C320-f16-objects-bg100x129-mix-s16-M8-item7": 1,
    "g32-C320-f16-one-bg1x128-bg-s256-M1-item11": 1,
    "g32-C320-f16-hand-bg129x128-bg-s1024-M2-item15": 1,
    "g16-C72-bf16-random-bg129x100-mix-s128-M8-donor_all-item2": 1,
    "g32-C320-f16-none-bg100x128-mix-s256-M2-donor_none-item0": 1,
    "g32-C320-f16-random-bg129x100-mix-s128-M8-donor_all-item2": 1,
    "g32-C320-f16-one-bg1x128-bg-s256-M1-donor_none-item3": 1,
    "g32-C320-f16-hand-bg128x129-mix-s32-M2-donor_one-item4": 1,
    "g32-C320-f16-none-bg100x128-mix-s256-M2-donor_all-item8": 1,
}


class Item:
    """One evaluation: geometry, types, pair set, background list lengths, the weights of the two terms, the gradient scale and,
    for a weighted item, M objects with their weights and the donor bits ("none" / "one" / "all"; None: not a donor call)."""

    def __init__(self, grid, C, types, pairs, bg, fwbw="mix", scale=None, M=0, weights=None, dead=(), donor=None, tag=""):
        self.grid, self.C, self.types, self.pairs, self.bg, self.fwbw, self.M, self.dead, self.donor = (
            grid, C, types, pairs, tuple(bg), fwbw, M, tuple(dead), donor)
        self.in_dtype, self.grad_dtype = TYPES[types]
        self.fg_w, self.bg_w = WEIGHTS[fwbw]
        self.scale = float(256.0 if scale is None else scale)
        self.weights = None if not M else tuple(weights) if weights is not None else tuple(0.5 + 0.75 * m for m in range(M))
        assert donor is None or M, "donor bits need a weighted item"
        self.donor_bits = {None: 0, "none": 0, "one": 1 << (M - 1) if M else 0, "all": (1 << M) - 1}[donor]
        self.kind = "plain" if not M else "objects" if donor is None else "donor"
        self.id = (f"g{grid}-C{C}-{types}-{pairs}-bg{bg[0]}x{bg[1]}-{fwbw}-s{self.scale:g}" + (f"-M{M}" if M else "")
                   + ("-gap" if dead else "") + (f"-donor_{donor}" if donor else "") + tag)
        self.seed = zlib.crc32(self.id.encode()) + SALT.get(self.id, 0)

    def cells(self):
        return cell_lists(self.grid, self.pairs, self.bg, self.M, self.dead)

    def inputs(self):
        """(cur, org, donor) [g,g,C] in the activation type, on the CPU: randn, and + 0.25 (-1)^c on org's bg_orig rows -- every
        channel's mean difference is then near +-0.25, both signs present."""
        return _inputs(self)

    def ref(self):
        return _ref(self)


@functools.lru_cache(maxsize=None)
def _inputs(it):
    gen = torch.Generator().manual_seed(it.seed)
    g, C = it.grid, it.C
    cur, org, donor = (torch.randn(g, g, C, generator=gen) for _ in range(3))
    c = it.cells()
    rows = torch.from_numpy(c["background_y_orig"] * g + c["background_x_orig"])
    org.view(g * g, C)[rows] += 0.25 * (1.0 - 2.0 * (torch.arange(C) % 2))
    return cur.to(it.in_dtype), org.to(it.in_dtype), donor.to(it.in_dtype)


@functools.lru_cache(maxsize=None)
def _ref(it):
    cur, org, donor = it.inputs()
    return item(cur, org, it.cells(), it.fg_w, it.bg_w, it.grid, it.weights, donor if it.donor_bits else None, it.donor_bits)


GEOMETRY = [(16, 8), (16, 72), (5, 320), (16, 1280), (8, 2048), (32, 320), (64, 72), (64, 320), (96, 64)]
WEIGHTED_GEOMETRY = [(16, 72), (32, 320)]
GAP = dict(M=8, weights=(1.0, 0.5, 2.0, 0.25, 3.0, 1.5, 0.0, 0.75), dead=(5,))      # object 5: no pairs; object 6: weight 0


def _singles():
    out = []
    S = lambda *a, **k: out.append(Item(*a, **k))
    # every geometry at both activation types, gradient in the activation type; the pair sets and list lengths take turns
    S(16, 8, "f16", "hand", (100, 1));                 S(16, 8, "bf16", "random", (128, 129))
    S(16, 72, "f16", "hand", (129, 100));              S(16, 72, "bf16", "hand", (1, 128), "fg")
    S(5, 320, "f16", "hand", (24, 7));                 S(5, 320, "bf16", "random", (3, 25), "bg")
    S(16, 1280, "f16", "random", (100, 129));          S(16, 1280, "bf16", "hand", (128, 100))
    S(8, 2048, "f16", "hand", (64, 33));               S(8, 2048, "bf16", "random", (20, 64))
    S(32, 320, "f16", "hand", (1000, 129));            S(32, 320, "bf16", "random", (128, 1000))
    S(64, 72, "f16", "hand", (1100, 2100));            S(64, 72, "bf16", "random", (3100, 4000))
    S(64, 320, "f16", "random", (2100, 3100), "bg");   S(64, 320, "bf16", "hand", (4000, 1100))
    S(96, 64, "f16", "hand", (1000, 3100));            S(96, 64, "bf16", "random", (2100, 1000), "fg")
    # the f32 gradient (scale 1 and 256) and the other 16-bit gradient type
    for t in ("f16_f32", "bf16_f32", "f16_bf16", "bf16_f16"):
        f32 = TYPES[t][1] == F32
        S(16, 72, t, "hand", (100, 129), scale=1.0 if f32 else None)
        S(32, 320, t, "random" if t.startswith("f16") else "hand", (1000, 128))
    # no pairs, one pair, an empty list on either side, nothing at all, the cancelling terms
    S(16, 72, "f16", "none", (100, 128));              S(32, 320, "bf16", "none", (1000, 1))
    S(16, 72, "bf16", "one", (128, 100));              S(32, 320, "f16", "one", (1, 1000), "fg")
    S(16, 72, "f16", "hand", (0, 100));                S(16, 72, "bf16", "random", (100, 0))
    S(16, 72, "bf16_f32", "none", (0, 0), scale=1.0)
    S(64, 320, "f16", "one", (4000, 1000))                                  # slices of 32 and 8 rows: k_colsum_q's last loop idles
    S(16, 72, "f16", "cancel", (128, CANCEL_TRANS), "cancel")
    S(16, 72, "bf16_f32", "cancel", (129, CANCEL_TRANS), "cancel", scale=1.0)
    S(32, 320, "bf16", "cancel", (1000, CANCEL_TRANS), "cancel")
    # a weight per object, and donor objects
    for g, C in WEIGHTED_GEOMETRY:
        big = (1000, 129) if g == 32 else (129, 100)
        for t in ("f16", "bf16"):
            S(g, C, t, "objects", big, M=8);           S(g, C, t, "objects", big[::-1], "fg", **GAP)
            S(g, C, t, "hand", (100, 128), M=2);       S(g, C, t, "random", big, M=2, weights=(0.25, 2.0))
            S(g, C, t, "hand", (128, 100), M=1);       S(g, C, t, "one", (100, 1), M=2)
            S(g, C, t, "objects", big, M=8, donor="none")
            S(g, C, t, "objects", (100, 129), M=8, donor="one")
            S(g, C, t, "objects", big, donor="all", **GAP)
            S(g, C, t, "hand", (128, 129), "fg", M=2, donor="one")
            S(g, C, t, "random", (100, 128), M=1, donor="all")
        S(g, C, "f16_f32", "objects", big, M=8, scale=1.0)
        S(g, C, "bf16_f32", "objects", big, M=8, donor="one")
        S(g, C, "bf16_f16", "hand", (100, 128), M=2, donor="all")
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), "duplicate case"
    return out


SINGLES = _singles()


class Batch:
    """K items of one geometry and type pair through one batch entry: "plain", "objects", "mixed" (weighted and unweighted
    items alternate) or "donor".  The items have different plans, term weights and scales; item 0 has no pairs, item 1 no
    background term, and the last item is like no other."""
    VARIANTS = [("none", (100, 128), "mix", 256.0), ("hand", (0, 100), "fg", 64.0), ("random", (129, 100), "mix", 128.0),
                ("one", (1, 128), "bg", 256.0), ("hand", (128, 129), "mix", 32.0), ("cancel", (128, CANCEL_TRANS), "cancel", 256.0),
                ("random", (100, 1), "fg", 512.0), ("objects", (100, 129), "mix", 16.0)]
    LAST = ("hand", (129, 128), "bg", 1024.0)
    OBJECTS = {"none": 2, "hand": 2, "random": 8, "one": 1, "cancel": 1, "objects": 8}

    def __init__(self, entry, K, grid, C, types):
        self.entry, self.K, self.grid, self.C, self.types = entry, K, grid, C, types
        self.id = f"{entry}-K{K}-g{grid}-C{C}-{types}"
        self.items = []
        for e in range(K):
            pairs, bg, fwbw, scale = self.LAST if (e == K - 1 and K > 2) else self.VARIANTS[e % len(self.VARIANTS)]
            weighted = entry in ("objects", "donor") or (entry == "mixed" and e % 2 == 0)
            M = self.OBJECTS[pairs] if weighted else 0
            donor = ("none", "one", "all")[e % 3] if entry == "donor" else None
            self.items.append(Item(grid, C, types, pairs, bg, fwbw, scale, M=M, donor=donor, tag=f"-item{e}"))
        self.in_dtype, self.grad_dtype = TYPES[types]


BATCHES = [Batch(entry, K, g, C, t) for entry in ("plain", "objects", "mixed", "donor")
           for K, g, C, t in ((2, 16, 72, "f16"), (16, 16, 72, "bf16"), (16, 32, 320, "f16"))]


def all_items():
    return SINGLES + [it for b in BATCHES for it in b.items]


# ---- what the kernels branch on, from the case definitions alone -----------------------------------------------------------
def branches(it):
    """The quantities of one item that decide a path in k_dedupe_sources[_obj], k_colsum_q and k_energy_grad[_obj]."""
    g, C = it.grid, it.C
    G2, nch = g * g, C // 8
    cpb = 256 // nch
    c = it.cells()
    keys, mult = entries(c, g)
    seg = np.bincount(keys[:, 1], minlength=G2)                       # distinct entries per target cell
    raw = np.bincount(keys[:, 1], weights=mult, minlength=G2)         # pairs per target cell
    n1, n2 = c["background_y_orig"].size, c["background_y_trans"].size
    out = dict(cpb=cpb, idle_lanes=256 - cpb * nch, ragged_last_block=G2 % cpb != 0, colsum_live_chunks_last=(nch - 1) % 8 + 1,
               seg=set(seg.tolist()), mult=set(mult.tolist()), raw_max=int(raw.max()), use_bg=bool(n1 and n2), n=(n1, n2),
               per={-(-n // COLSUM_S) for n in (n1, n2) if n}, targets=set(keys[:, 1].tolist()), sources=set(keys[:, 2].tolist()),
               n_pairs=int(mult.sum()))
    # the steps of a segment at which the object changes: ("batch", j) in the 8-wide loop, "tail" behind it
    changes, first_objects, eight_of_eight = set(), set(), False
    trans = set((c["background_y_trans"] * g + c["background_x_trans"]).tolist())
    single, mult_in_batch = 0, False
    for tc in np.nonzero(seg)[0]:
        rows = keys[:, 1] == tc
        objs = keys[rows, 0]
        L = objs.size
        mult_in_batch |= bool((mult[rows][:L // 8 * 8] > 1).any())      # a multiplicity that the 8-wide loop applies
        first_objects.add(int(objs[0]))
        eight_of_eight |= L == 8 and len(set(objs.tolist())) == 8
        for p in range(1, L):
            if objs[p] != objs[p - 1]:
                changes.add(("batch", p % 8, p >= 8) if p < L // 8 * 8 else "tail")
        single += int(L == 1 and mult[rows][0] == 1 and int(tc) in trans)
    live = np.bincount(keys[:, 0], weights=mult, minlength=max(it.M, 1)) > 0
    # the rows that the last loop of k_colsum_q adds: slice length % 8 of every slice of both lists
    tail_rows = 0
    for n in (n1, n2):
        per = -(-n // COLSUM_S) if n else 0
        tail_rows += sum(max(min(per, n - sl * per), 0) % 8 for sl in range(COLSUM_S)) if n else 0
    out.update(changes=changes, first_objects=first_objects, eight_of_eight=eight_of_eight, live=live.tolist(),
               mult_in_batch=mult_in_batch, folds=bool(changes), colsum_tail_rows=tail_rows if n1 and n2 else 0,
               # elements where the foreground and the background term are equal in magnitude (one pair, one flag)
               cancelling_cells=single if (n2 and out["n_pairs"]
                                           and abs(it.fg_w / out["n_pairs"] - it.bg_w / n2) <= 2.0 ** -10 * it.fg_w / out["n_pairs"]
                                           and it.fg_w > 0) else 0)
    return out
