"""Test-side reference of the harmonic in-fill, shared by tests/test_infill_solvers_gpu.py (one system per dh_laplacian_blend
call), tests/test_infill_reproject_gpu.py (the K systems of a re-projection call) and tests/test_infill_ref.py (this file and the
cases below, on the CPU).  Built here and never taken from the library: the linear system in float64 (diagonal 4, -1 towards
every unknown 4-neighbour inside the image, right-hand side = the known neighbours, minus an optional Laplacian image), solved
by a sparse direct solve (x_ref) and by a plain classic CG with the kernels' stop rule (its_ref).

Also the cases whose in-fill sets are LARGE inside a re-projection: an object of multi_object_ref.two_spheres(512) scaled up in
point mode (the lattice of gaps between its points, which the mask CLOSE turns into in-fill pixels) and the background alone
un-projected with a longer lens (a frame of pixels without an owner, unknowns on the image's first and last rows and columns).
The n / class / classic-iteration columns are pinned by tests/test_infill_ref.py."""
import ctypes
import functools

import numpy as np

TOL2 = 1e-24           # the kernels' stop rule: iterate while (r, r) > TOL2 * (b, b)
CG_REPLACE = 50        # k_cg_fill_multi: iterations between two residual replacements (csrc/geometry.hip)
RES = 512

# multi_object_ref.two_spheres(512); every edit is [(0, Y, t, s, None), (0, Y, (0, 0, 0))]: object 0 scaled by s about its
# centroid and shifted by t, object 1 left alone.  (s, t, in-fill pixels, solver class, classic CG iterations)
SCALED = (
    (1.0, (0.0, 0.0, 0.0), 1036, "lds", 34),
    (1.5, (0.3, 0.0, 0.0), 22303, "multi", 43),
    (2.0, (0.5, 0.0, 0.0), 41889, "multi", 45),
    (2.6, (0.6, 0.0, 0.0), 63216, "multi", 62),           # > CG_REPLACE iterations: one residual replacement
    (2.8, (0.6, 0.0, 0.0), 71545, "single", 70),
)
# the same five edits with footprint splatting: the triangles close the lattice, the in-fill sets are small (all on chip)
FOOTPRINT_N = (1036, 1326, 1300, 1339, 1380)
# object_removal_ref.background_alone(bg, K_unproject = the intrinsics with both focal lengths times the factor).
# (lens factor, in-fill pixels, solver class, classic CG iterations)
BACKGROUND = (
    (1.12, 52380, "multi", 326),                          # six residual replacements
    (1.25, 94044, "single", 573),
)
# synthetic.make_scene(512) with synthetic.TRANSFORMS[0..5] in one call: (in-fill pixels, solver class)
MIXED = ((755, "lds"), (6123, "lds"), (11189, "multi"), (17503, "multi"), (1943, "lds"), (8454, "multi"))


def laplacian_f32(img):
    """5-point Laplacian with zero padding, an f64 sum rounded to f32, as k_laplacian defines it; returned in f64."""
    a = np.asarray(img).astype(np.float64)
    pad = np.pad(a, 1)
    return (pad[:-2, 1:-1] + pad[2:, 1:-1] + pad[1:-1, :-2] + pad[1:-1, 2:] - 4.0 * a).astype(np.float32).astype(np.float64)


def system(known, mask, lap=None):
    """A (csr, f64), b (f64) and the unknowns' pixel coordinates, row-major like the library's compaction.  known: the field
    whose values outside the mask enter the right-hand side; lap: None (the re-projection's rhs_extra = NULL) or an image that is
    subtracted from the right-hand side (laplacian_f32 of the background depth in dh_laplacian_blend)."""
    import scipy.sparse
    h, w = mask.shape
    ys, xs = np.nonzero(mask)
    n = ys.size
    idx = -np.ones((h, w), dtype=np.int64)
    idx[ys, xs] = np.arange(n)
    rows, cols = [np.arange(n)], [np.arange(n)]
    vals = [np.full(n, 4.0)]
    b = np.zeros(n)
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        yy, xx = ys + dy, xs + dx
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        yc, xc = np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)
        unk = inside & mask[yc, xc]
        kn = inside & ~mask[yc, xc]
        rows.append(np.nonzero(unk)[0])
        cols.append(idx[yc[unk], xc[unk]])
        vals.append(np.full(int(unk.sum()), -1.0))
        b[kn] += known[yc[kn], xc[kn]].astype(np.float64)
    if lap is not None:
        b -= lap[ys, xs]
    A = scipy.sparse.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    return A, b, ys, xs


def classic_cg_iterations(A, b, cap=50000):
    """textbook CG in numpy f64 from x = 0; the number of iterations taken while (r, r) > TOL2 * (b, b)"""
    x = np.zeros_like(b)
    r = b.copy()
    p = b.copy()
    rs = float(r @ r)
    bnorm = rs
    it = 0
    while it < cap and rs > TOL2 * bnorm:
        q = A @ p
        alpha = rs / float(p @ q)
        x += alpha * p
        r -= alpha * q
        rsn = float(r @ r)
        p = r + (rsn / rs) * p
        rs = rsn
        it += 1
    return it


def solve(known, mask, lap=None):
    """(x_ref as a full f64 image: `known` with the direct solution on the mask, its_ref); the direct solve checks itself."""
    import scipy.sparse.linalg
    A, b, ys, xs = system(known, mask, lap)
    x = scipy.sparse.linalg.spsolve(A.tocsc(), b)
    assert float(np.abs(A @ x - b).max()) <= 1e-11 * float(np.abs(b).max())      # the direct solve itself
    ref = known.astype(np.float64)
    ref[ys, xs] = x
    return ref, classic_cg_iterations(A, b)


@functools.lru_cache(maxsize=64)
def _reference(known_bytes, mask_bytes, h, w):
    known = np.frombuffer(known_bytes, dtype=np.float32).reshape(h, w)
    mask = np.unpackbits(np.frombuffer(mask_bytes, dtype=np.uint8), count=h * w).reshape(h, w).astype(bool)
    ref, its = solve(known, mask)
    ref.setflags(write=False)
    return ref, its


def reference(known_f32, inpaint_bool):
    """The re-projection's system (no Laplacian term): (x_ref as a full f64 image, its_ref), read-only and computed once per
    distinct input.  Only the values of known_f32 OUTSIDE inpaint_bool enter (the others are set to 0 before anything is formed),
    and x_ref holds 0 .. the known field there."""
    known = np.ascontiguousarray(known_f32)
    mask = np.ascontiguousarray(inpaint_bool)
    assert known.dtype == np.float32 and mask.dtype == np.bool_ and known.shape == mask.shape and known.ndim == 2
    known = np.where(mask, np.float32(0.0), known)
    assert np.isfinite(known).all()
    return _reference(known.tobytes(), np.packbits(mask).tobytes(), *mask.shape)


def bound(x_ref, mask):
    """f32 rounding of an f64 solution, the project's rule: 4 * 2^-24 * max |x_ref| over the unknowns"""
    return 4.0 * 2.0 ** -24 * float(np.abs(x_ref[mask]).max())


def limits():
    """(largest n solved on chip, largest n of the sixteen-workgroup kernel, its workgroups), from the library's constants
    (dh_dbg_cg_limits is host-only: no device call)"""
    from diffusionhandles_amd import _lib
    v = (ctypes.c_int * 3)()
    _lib.check(_lib.lib().dh_dbg_cg_limits(v), "dh_dbg_cg_limits")
    return int(v[0]), int(v[1]), int(v[2])


def solver_of(n):
    lds_max, multi_max, _ = limits()
    return "lds" if n <= lds_max else "multi" if n <= multi_max else "single"


# ---- the re-projection cases ------------------------------------------------------------------------------------------------
def scaled_edit(i):
    """The two transforms of row i of SCALED."""
    import multi_object_ref as R
    s, t = SCALED[i][:2]
    return [(0.0, R.Y, t, s, None), (0.0, R.Y, (0.0, 0.0, 0.0))]


def _explicit(make):
    """The oracle under the written-out dot order of the kernels (for a turn about Y it is the BLAS result too)."""
    from oracle import depth_ref as D
    D.DOT_ORDER = "explicit"
    try:
        return make()
    finally:
        D.DOT_ORDER = "blas"


@functools.lru_cache(maxsize=None)
def scaled_oracle(i):
    """similarity_ref.transform_objects of row i of SCALED on two_spheres(512): (disparity, correspondences, debug dict)"""
    import multi_object_ref as R
    import similarity_ref as S
    depth, bg, masks = R.two_spheres(RES)
    return _explicit(lambda: S.transform_objects(depth, bg, masks, scaled_edit(i)))


@functools.lru_cache(maxsize=None)
def footprint_oracle(i):
    """footprints_ref.transform_objects(footprints=True) of row i of SCALED on two_spheres(512)"""
    import footprints_ref as F
    import multi_object_ref as R
    depth, bg, masks = R.two_spheres(RES)
    return _explicit(lambda: F.transform_objects(depth, bg, masks, scaled_edit(i), footprints=True))


def longer_lens(factor):
    from oracle import depth_ref as D
    k = D.intrinsics_f32().clone()
    k[0, 0] *= factor
    k[1, 1] *= factor
    return k


@functools.lru_cache(maxsize=None)
def background_oracle(i):
    """object_removal_ref.background_alone of row i of BACKGROUND on the background of two_spheres(512): (disparity, debug dict)"""
    import multi_object_ref as R
    import object_removal_ref as RR
    _, bg, _ = R.two_spheres(RES)
    return RR.background_alone(bg, K_unproject=longer_lens(BACKGROUND[i][0]))
