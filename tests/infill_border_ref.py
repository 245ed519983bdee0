"""Test-side statement of the in-fill's image border ("In-fill border"), independent of the product and shared by
tests/test_infill_border_ref.py (CPU) and tests/test_infill_border_gpu.py.  The reference has no such mode; this file is the
yardstick.

    border   "zero": a neighbour beyond the frame is a known 0 -- the diagonal of every unknown is 4 (oracle.depth_ref).
             "reflect": the mirror ghost cell x_ghost = x_self, zero normal derivative at the frame -- the diagonal of an unknown
             is the number of its 4-neighbours inside the image (4, 3 on an edge, 2 in a corner).
    matrix   -1 towards every unknown neighbour inside the image; known neighbours inside the image on the right-hand side;
             nothing else depends on the border.
    blend    the same matrix; the background's 5-point Laplacian on the right-hand side with zero padding ("zero",
             scipy.ndimage.convolve(mode="constant")) or replicate padding ("reflect", mode="nearest": -(degree) * img + the sum of
             the in-image neighbours).
    whole    the one component without a known neighbour is the whole image: the right-hand side of the fill is 0 and the result
             is all zeros (the solvers never enter their loop: (b, b) = 0), under both borders.

Also the f64 model of the pipelined recurrence the sixteen-workgroup solver runs (Ghysels & Vanroose, with a residual replacement
every infill_ref.CG_REPLACE iterations), for the iteration-count gate."""
import numpy as np

from infill_ref import CG_REPLACE, TOL2, bound, classic_cg_iterations, solver_of  # noqa: F401  (re-exported for the tests)

BORDERS = ("zero", "reflect")
STENCIL = np.array([[0, 1, 0], [1, -4, 1], [0, 1, 0]])


def degree(h, w):
    """The number of 4-neighbours inside an h x w image, per pixel (f64)."""
    d = np.full((h, w), 4.0)
    d[0, :] -= 1.0
    d[-1, :] -= 1.0
    d[:, 0] -= 1.0
    d[:, -1] -= 1.0
    return d


def laplacian(img, border):
    """The blend's Laplacian of the background in the image's own precision (what oracle.depth_ref.laplacian_blend forms)."""
    import scipy.ndimage
    assert border in BORDERS
    return scipy.ndimage.convolve(np.asarray(img), STENCIL, mode="constant" if border == "zero" else "nearest")


def laplacian_f32(img, border):
    """The Laplacian as k_laplacian defines it: an f64 sum rounded to f32, returned in f64.  "reflect": replicate padding."""
    assert border in BORDERS
    a = np.asarray(img).astype(np.float64)
    pad = np.pad(a, 1, mode="constant" if border == "zero" else "edge")
    return (pad[:-2, 1:-1] + pad[2:, 1:-1] + pad[1:-1, :-2] + pad[1:-1, 2:] - 4.0 * a).astype(np.float32).astype(np.float64)


def system(known, mask, lap=None, border="zero"):
    """A (csr, f64), b (f64) and the unknowns' pixel coordinates (row-major).  known: the field whose values outside the mask
    enter the right-hand side; lap: None or an image that is subtracted from it."""
    import scipy.sparse
    assert border in BORDERS
    mk = np.asarray(mask).astype(bool)
    h, w = mk.shape
    ys, xs = np.nonzero(mk)
    n = ys.size
    idx = -np.ones((h, w), dtype=np.int64)
    idx[ys, xs] = np.arange(n)
    diag = np.full(n, 4.0) if border == "zero" else degree(h, w)[ys, xs]
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [diag]
    b = np.zeros(n)
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        yy, xx = ys + dy, xs + dx
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        yc, xc = np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)
        unk = inside & mk[yc, xc]
        kn = inside & ~mk[yc, xc]
        rows.append(np.nonzero(unk)[0])
        cols.append(idx[yc[unk], xc[unk]])
        vals.append(np.full(int(unk.sum()), -1.0))
        b[kn] += known[yc[kn], xc[kn]]
    if lap is not None:
        b -= lap[ys, xs]
    A = scipy.sparse.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    return A, b, ys, xs


def _solve(A, b):
    import scipy.sparse.linalg
    return scipy.sparse.linalg.spsolve(A, b)


def harmonic_fill(image, mask, border="zero"):
    """`image` with the pixels of `mask` in-filled (f64 direct solve, the result in the image's dtype)."""
    img = np.asarray(image)
    mk = np.asarray(mask).astype(bool)
    out = img.copy()
    if not mk.any():
        return out
    if mk.all():                      # no known neighbour: b = 0, the solvers leave before their first iteration
        out[...] = 0
        return out
    A, b, ys, xs = system(img, mk, None, border)
    out[ys, xs] = _solve(A, b)
    return out


def laplacian_blend(fg, bg, mask, border="zero"):
    """oracle.depth_ref.laplacian_blend with the border: `fg` outside the mask, inside the solution with the background's
    Laplacian on the right-hand side."""
    fg = np.asarray(fg)
    mk = np.asarray(mask).astype(bool)
    out = fg.copy()
    if not mk.any():
        return out
    A, b, ys, xs = system(fg, mk, laplacian(bg, border), border)
    out[ys, xs] = _solve(A, b)
    return out


def solve(known, mask, lap=None, border="zero"):
    """(x_ref as a full f64 image: `known` with the direct solution on the mask, classic CG's iteration count); the direct solve
    checks itself."""
    A, b, ys, xs = system(np.asarray(known).astype(np.float64), mask, lap, border)
    x = _solve(A.tocsc(), b)
    assert float(np.abs(A @ x - b).max()) <= 1e-11 * float(np.abs(b).max())
    ref = np.asarray(known).astype(np.float64)
    ref[ys, xs] = x
    return ref, classic_cg_iterations(A, b)


BREAKDOWN = -3


def pipelined_cg_iterations(A, b, replace=CG_REPLACE, cap=50000):
    """The recurrence of k_cg_fill_multi in numpy f64 from x = 0: w = A r carried along, both dot products from one state,
    q = A w; every `replace`-th iteration ends with r = b - A x, s = A p, w = A r, z = A s (replace = 0: never).  Returns the
    number of iterations taken while (r, r) > TOL2 * (b, b), BREAKDOWN for a step length that is not positive and finite, or
    None at the cap."""
    x = np.zeros_like(b)
    r = b.copy()
    w = A @ r
    z, s, p = np.zeros_like(b), np.zeros_like(b), np.zeros_like(b)
    bnorm = float(b @ b)
    gamma_old = alpha_old = 1.0
    it = 0
    while True:
        gamma, delta = float(r @ r), float(w @ r)
        if not gamma > TOL2 * bnorm:
            return it
        if it >= cap:
            return None
        beta = gamma / gamma_old if it else 0.0
        with np.errstate(all="ignore"):
            alpha = gamma / (delta - beta * gamma / alpha_old) if it else gamma / delta
        if not (alpha > 0.0 and np.isfinite(alpha)):
            return BREAKDOWN
        q = A @ w
        z = q + beta * z
        s = w + beta * s
        p = r + beta * p
        x = x + alpha * p
        r = r - alpha * s
        w = w - alpha * z
        if replace and (it + 1) % replace == 0:
            r = b - A @ x
            s = A @ p
            w = A @ r
            z = A @ s
        gamma_old, alpha_old = gamma, alpha
        it += 1


# ---- shapes -----------------------------------------------------------------------------------------------------------------
def corner(res, side):
    """a side x side hole in the top right corner: rows y = 0 and columns x = res - 1 are unknowns"""
    m = np.zeros((res, res), dtype=bool)
    m[:side, res - side:] = True
    return m


def strip_columns(res, width):
    """a full-height strip at the left edge: three borders"""
    m = np.zeros((res, res), dtype=bool)
    m[:, :width] = True
    return m


def strip_rows(res, height):
    """a full-width strip at the top edge: three borders"""
    m = np.zeros((res, res), dtype=bool)
    m[:height, :] = True
    return m


def frame(res, width):
    """a frame of `width` pixels around a known interior: all four borders"""
    m = np.ones((res, res), dtype=bool)
    m[width:res - width, width:res - width] = False
    return m


# name -> (res, mask builder, unknowns, solver class): the smallest shapes per class (tests/test_infill_border_gpu.py)
SOLVER_CASES = {
    "lds_corner_60": (64, lambda: corner(64, 60), 3600, "lds"),
    "lds_strip_8": (64, lambda: strip_columns(64, 8), 512, "lds"),
    "multi_corner_92": (96, lambda: corner(96, 92), 8464, "multi"),                # crosses eight replacements
    "multi_frame_20": (128, lambda: frame(128, 20), 8640, "multi"),               # all four borders
    "multi_corner_150": (256, lambda: corner(256, 150), 22500, "multi"),
    "single_corner_257": (261, lambda: corner(261, 257), 66049, "single"),
}
# further systems of the pipelined model (CPU only)
MODEL_CASES = {
    "strip_rows_40": (256, lambda: strip_rows(256, 40)),
    "frame_12": (256, lambda: frame(256, 12)),
}


def fields(res):
    """depth: the analytic scene (values 2 .. 5.5); bg = 3 + 0.05 sin(x / 9) + 0.3 y / res + 1e-3 Gaussian noise -- the fields of
    tests/test_infill_solvers_gpu.py at `res`."""
    from diffusionhandles_amd.synthetic import make_scene
    depth, _, _ = make_scene(res)
    yy, xx = np.meshgrid(np.arange(res, dtype=np.float64), np.arange(res, dtype=np.float64), indexing="ij")
    noise = np.random.default_rng(20).standard_normal((res, res))
    bg = (3.0 + 0.05 * np.sin(xx / 9.0) + 0.3 * yy / res + 1e-3 * noise).astype(np.float32)
    return depth[0, 0].numpy().copy(), bg


_SOLVER_REFERENCE = {}


def solver_reference(name, border="reflect"):
    """(depth, bg, mask, x_ref as a full f64 image, its_ref, A, b) of a solver case under `border`: computed once, read-only"""
    key = (name, border)
    if key not in _SOLVER_REFERENCE:
        res, make = (SOLVER_CASES.get(name) or MODEL_CASES[name])[:2]
        depth, bg = fields(res)
        mask = make()
        lap = laplacian_f32(bg, border)
        ref, its_ref = solve(depth, mask, lap, border)
        A, b, _, _ = system(depth.astype(np.float64), mask, lap, border)
        for a in (depth, bg, mask, ref, b):
            a.setflags(write=False)
        _SOLVER_REFERENCE[key] = (depth, bg, mask, ref, its_ref, A, b)
    return _SOLVER_REFERENCE[key]


# ---- the six-camera fixture -------------------------------------------------------------------------------------------------
def components(mask):
    """(label image, number of components) of a mask under 4-connectivity -- the connectivity of the stencil"""
    import scipy.ndimage
    return scipy.ndimage.label(np.asarray(mask).astype(bool))


def frame_edge(shape):
    e = np.zeros(shape, dtype=bool)
    e[0, :] = e[-1, :] = e[:, 0] = e[:, -1] = True
    return e


def touching(mask):
    """(the pixels of the components of `mask` that touch the frame, those of the others)"""
    lab, n = components(mask)
    ids = np.unique(lab[frame_edge(lab.shape) & (lab > 0)])
    touch = np.isin(lab, ids) & (lab > 0)
    return touch, (lab > 0) & ~touch


def bordering_known(mask_part, mask_all):
    """the known pixels that are 4-neighbours of `mask_part`"""
    import scipy.ndimage
    return scipy.ndimage.binary_dilation(mask_part) & ~np.asarray(mask_all).astype(bool)


def camera_fill(geo, border):
    """The filled disparity (f32 [res, res]) of one geometry of camera_moves_ref.fixture under `border`."""
    g = geo[2]
    return harmonic_fill(g["disparity"], g["inpaint"], border).astype(np.float32)


def camera_table_row(geo):
    """One row of the table of DESIGN.md "In-fill border": (in-fill pixels, those in components touching the frame, mean of the
    known pixels bordering those components, frame-edge mean under zero, under reflect, classic CG iterations under zero, under
    reflect)."""
    g = geo[2]
    disp, inpaint = g["disparity"], g["inpaint"]
    touch, _ = touching(inpaint)
    edge = touch & frame_edge(inpaint.shape)
    ring = bordering_known(touch, inpaint)
    out = [int(inpaint.sum()), int(touch.sum()), float(disp[ring].astype(np.float64).mean())]
    its = []
    for border in BORDERS:
        out.append(float(harmonic_fill(disp, inpaint, border)[edge].astype(np.float64).mean()))
        A, b, _, _ = system(disp, inpaint, None, border)
        its.append(classic_cg_iterations(A, b))
    return tuple(out + its)
