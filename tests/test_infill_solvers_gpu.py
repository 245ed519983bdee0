"""The three f64 conjugate-gradient kernels of the harmonic in-fill (set_foreground / laplacian_depth_blend and every
re-projection), driven through dh_laplacian_blend with dilate_iterations = 0 so that the number of unknowns is exactly the
mask's pixel count.

Reference, built here and never taken from the library: the same linear system on the CPU in float64 (diagonal 4, -1
towards every masked 4-neighbour inside the image, right-hand side = known neighbours - laplacian(bg), the Laplacian an
f64 sum rounded to f32 as k_laplacian defines it), solved by a sparse direct solve (x_ref) and by a plain classic CG with
the kernels' stop rule (its_ref).  The system, the classic CG and the solver-class rule live in tests/infill_ref.py, which the
re-projection's in-fill tests (tests/test_infill_reproject_gpu.py) share.

What an accuracy bound alone cannot see: a recurrence that has lost its orthogonality still reaches the fixed point, only
in several times the iterations (each one a grid-wide seam in the sixteen-workgroup kernel), or leaves at the cap with
an ordinary count.  So every case also gates the ITERATION COUNT against classic CG: <= 1.05 * its_ref + 5 (a healthy
pipelined recurrence stays within 2 % of classic in an f64 model, every degraded one is >= 9 % above it)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infill_ref as I  # noqa: E402
from infill_ref import limits as _limits, solver_of as _solver_of  # noqa: E402

from diffusionhandles_amd.synthetic import make_scene  # noqa: E402

pytestmark = pytest.mark.gpu

RES = 512


def _dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _rect(y0, x0, h, w):
    m = np.zeros((RES, RES), dtype=bool)
    m[y0:y0 + h, x0:x0 + w] = True
    return m


def _centred(h, w):
    return _rect((RES - h) // 2, (RES - w) // 2, h, w)


def _plus_pixel(m):
    """one more unknown, attached to the rectangle's top right corner from the right"""
    ys, xs = np.nonzero(m)
    m = m.copy()
    m[ys.min(), xs.max() + 1] = True
    return m


def _island(side, hole):
    m = _centred(side, side)
    m &= ~_centred(hole, hole)
    return m


# name -> (mask, number of unknowns, solver the dispatch must pick)
CASES = {
    "control_6000_on_chip": (lambda: _centred(75, 80), 6000, "lds"),
    "boundary_8192": (lambda: _centred(64, 128), 8192, "lds"),
    "boundary_8193": (lambda: _plus_pixel(_centred(64, 128)), 8193, "multi"),      # per = 513: the last workgroup is short
    "square_200": (lambda: _centred(200, 200), 40000, "multi"),
    "square_230": (lambda: _centred(230, 230), 52900, "multi"),
    "square_255": (lambda: _centred(255, 255), 65025, "multi"),
    "rect_120x420": (lambda: _centred(120, 420), 50400, "multi"),
    "square_240_island_60": (lambda: _island(240, 60), 54000, "multi"),
    "corner_230": (lambda: _rect(0, RES - 230, 230, 230), 52900, "multi"),         # rows y = 0 and columns x = res - 1 are unknowns
    "boundary_65536": (lambda: _centred(256, 256), 65536, "multi"),                # 4 unknowns per thread in every workgroup
    "boundary_65537": (lambda: _plus_pixel(_centred(256, 256)), 65537, "single"),
    "control_70225_single": (lambda: _centred(265, 265), 70225, "single"),
}


@functools.lru_cache(maxsize=None)
def _fields():
    """depth: the analytic scene (values 2 .. 5.5, so the rim carries O(1) values into the right-hand side);
    bg = 3 + 0.05 sin(x / 9) + 0.3 y / res + 1e-3 Gaussian noise (an interior right-hand side)."""
    depth, _, _ = make_scene(RES)
    yy, xx = np.meshgrid(np.arange(RES, dtype=np.float64), np.arange(RES, dtype=np.float64), indexing="ij")
    noise = np.random.default_rng(20).standard_normal((RES, RES))
    bg = (3.0 + 0.05 * np.sin(xx / 9.0) + 0.3 * yy / RES + 1e-3 * noise).astype(np.float32)
    return depth[0, 0].numpy().copy(), bg


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(mask, x_ref as a full f64 image, its_ref) of a case, computed once and shared"""
    depth, bg = _fields()
    mask = CASES[name][0]()
    ref, its_ref = I.solve(depth, mask, I.laplacian_f32(bg))
    ref.setflags(write=False)
    mask.setflags(write=False)
    return mask, ref, its_ref


def _blend(mask):
    from diffusionhandles_amd import depth_transform as DT
    depth, bg = _fields()
    t = lambda a: torch.from_numpy(np.array(a))[None, None].to(_dev())      # (a copy: the cached references are read-only)
    out, its = DT.laplacian_depth_blend(t(depth), t(bg), t(mask), dilate_iterations=0, return_iterations=True)
    return out[0, 0].cpu().numpy(), its


def test_dispatch_constants():
    lds_max, multi_max, wgs = _limits()
    assert (lds_max, multi_max, wgs) == (8192, 65536, 16)
    assert (8193 + wgs - 1) // wgs == 513 and 15 * 513 < 8193 < 16 * 513      # the last workgroup owns 498 of 513
    assert multi_max == wgs * 4 * 1024                                          # full: 4 unknowns per thread everywhere


@pytest.mark.parametrize("name", list(CASES))
def test_infill_solver_vs_f64_reference(name):
    _, n_expected, solver = CASES[name]
    mask, ref, its_ref = _reference(name)
    n = int(mask.sum())
    assert n == n_expected
    assert _solver_of(n) == solver, (n, _solver_of(n))
    depth, _ = _fields()
    out, its = _blend(mask)
    finite = bool(np.isfinite(out).all())
    err = float(np.abs(out.astype(np.float64) - ref).max()) if finite else float("nan")
    bound = 4.0 * 2.0 ** -24 * float(np.abs(ref[mask]).max())
    print(f"in-fill {name}: n {n} ({solver}), its_ref {its_ref}, iterations {its}, max abs err {err:.3e} (bound {bound:.3e})")
    assert its >= 0, its
    assert its <= 1.05 * its_ref + 5, (name, its, its_ref)
    assert finite
    assert err <= bound, (name, err, bound)
    assert np.array_equal(out[~mask].view(np.uint32), depth[~mask].view(np.uint32))      # outside the mask: the input's bits
    out2, its2 = _blend(mask)
    assert its2 == its
    assert np.array_equal(out2.view(np.uint32), out.view(np.uint32))


def test_iteration_cap_is_an_error_and_is_restored():
    """dh_dbg_cg_max_iter(10) on a 200 x 200 hole: the solver leaves at the cap far from converged, which must surface as
    the non-convergence error (not as a count of 10 beside an unconverged field); with the cap restored the same call
    succeeds."""
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd import depth_transform as DT
    mask, ref, its_ref = _reference("square_200")
    L = _lib.lib()
    _lib.check(L.dh_dbg_cg_max_iter(10), "dh_dbg_cg_max_iter")
    try:
        with pytest.raises(DT.InfillNotConverged):
            _blend(mask)
    finally:
        _lib.check(L.dh_dbg_cg_max_iter(0), "dh_dbg_cg_max_iter")
    out, its = _blend(mask)
    assert 10 < its <= 1.05 * its_ref + 5
    assert float(np.abs(out.astype(np.float64) - ref).max()) <= 4.0 * 2.0 ** -24 * float(np.abs(ref[mask]).max())
