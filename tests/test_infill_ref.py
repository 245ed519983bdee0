"""CPU: the inputs of tests/test_infill_reproject_gpu.py reach what they claim, by the references alone -- the in-fill sets of the
scaled-object and background-alone cases of tests/infill_ref.py have the pinned sizes, fall in the pinned solver class of the
library's dispatch constants (dh_dbg_cg_limits, host only), take the pinned classic-CG iteration counts (one multi case beyond a
residual replacement), and the oracle's own harmonic_fill lies within the f32-rounding bound of infill_ref.reference built from
the oracle's known pixels: the reference alone holds the gate the GPU tests apply."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infill_ref as I  # noqa: E402


def _check(what, inpaint, disparity, filled, n, solver, its):
    """inpaint: the oracle's in-fill set; disparity: its f32 field before the in-fill; filled: its harmonic_fill output (f32)"""
    assert inpaint.dtype == np.bool_ and disparity.dtype == np.float32 and filled.dtype == np.float32
    assert int(inpaint.sum()) == n, (what, int(inpaint.sum()))
    assert I.solver_of(n) == solver, (what, n, I.solver_of(n))
    x_ref, its_ref = I.reference(disparity, inpaint)
    bound = I.bound(x_ref, inpaint)
    err = float(np.abs(filled.astype(np.float64) - x_ref)[inpaint].max())
    print(f"{what}: n {n} ({solver}), its_ref {its_ref}, oracle harmonic_fill against the reference {err:.3e} (bound {bound:.3e})")
    assert np.array_equal(x_ref[~inpaint], disparity[~inpaint].astype(np.float64))       # outside: the known field itself
    assert err <= bound, (what, err, bound)
    assert abs(its_ref - its) <= 2, (what, its_ref, its)                                  # NumPy's summation order may move it by one
    return its_ref


def test_dispatch_constants_and_the_case_tables():
    assert I.limits() == (8192, 65536, 16)
    assert [I.solver_of(n) for n in (0, 8192, 8193, 65536, 65537)] == ["lds", "lds", "multi", "multi", "single"]
    for n, solver in [row[2:4] for row in I.SCALED] + [row[1:3] for row in I.BACKGROUND] + list(I.MIXED):
        assert I.solver_of(n) == solver, (n, solver)
    # every class inside one scaled-object call, single first and lds second; both large classes in the background cases
    assert {row[3] for row in I.SCALED} == {"lds", "multi", "single"} and [row[2] for row in I.BACKGROUND] == ["multi", "single"]
    # at least one multi case runs beyond a residual replacement
    assert max(row[4] for row in I.SCALED if row[3] == "multi") > I.CG_REPLACE
    assert [row[3] for row in I.BACKGROUND if row[2] == "multi"] == [326] and 326 // I.CG_REPLACE == 6


@pytest.mark.parametrize("i", range(len(I.SCALED)))
def test_scaled_object_case(i):
    s, t, n, solver, its = I.SCALED[i]
    disp, corr, dbg = I.scaled_oracle(i)
    its_ref = _check(f"two_spheres(512), object 0 scaled by {s}", dbg["inpaint"], dbg["disparity"], disp[0, 0].numpy(), n, solver, its)
    if solver == "multi" and its > I.CG_REPLACE:
        assert its_ref > I.CG_REPLACE
    assert len(corr) > 1000
    # the lattice of gaps: from 1.5 on, the in-fill set is more than a third of the cleaned mask
    if s >= 1.5:
        assert n > int((dbg["cleaned"] != 0).sum()) // 3


def test_footprint_cases_are_small_and_have_held_the_keep_flags():
    """With footprints the same edits leave in-fill sets of about 1 300 pixels (the on-chip solver), while the keep flags that
    the library parks in the in-fill's buffers before number tens of thousands: every correspondence row is one."""
    for i, n in enumerate(I.FOOTPRINT_N):
        _, corr, dbg = I.footprint_oracle(i)
        assert int(dbg["inpaint"].sum()) == n and I.solver_of(n) == "lds", (i, int(dbg["inpaint"].sum()))
        assert len(corr) > 20 * n and len(corr) > I.limits()[0]
        if i > 0:
            assert len(corr) > len(I.footprint_oracle(i - 1)[1])              # the enlarged object covers more pixels


@pytest.mark.parametrize("i", range(len(I.BACKGROUND)))
def test_background_alone_case(i):
    factor, n, solver, its = I.BACKGROUND[i]
    disp, dbg = I.background_oracle(i)
    un = dbg["unowned"]
    assert un[0].all() and un[-1].all() and un[:, 0].all() and un[:, -1].all() and not un[I.RES // 2, I.RES // 2]
    its_ref = _check(f"background alone, lens factor {factor}", un, dbg["disparity"], disp[0, 0].numpy(), n, solver, its)
    if solver == "multi":
        assert its_ref > I.CG_REPLACE


def test_reference_ignores_the_values_under_the_mask_and_is_shared():
    rng = np.random.default_rng(3)
    known = rng.uniform(0.0, 255.0, (24, 31)).astype(np.float32)
    mask = np.zeros((24, 31), dtype=bool)
    mask[0:9, 20:31] = True                              # touches the first row and the last column
    mask[12:20, 3:17] = True
    x0, its0 = I.reference(known, mask)
    poisoned = known.copy()
    poisoned[mask] = np.float32(1e30)
    x1, its1 = I.reference(poisoned, mask)
    assert x1 is x0 and its1 == its0 and not x0.flags.writeable
    # the solution is harmonic: 4 x - the four neighbours (0 beyond the border) vanishes on the mask
    pad = np.pad(x0, 1)
    lap = 4.0 * x0 - pad[:-2, 1:-1] - pad[2:, 1:-1] - pad[1:-1, :-2] - pad[1:-1, 2:]
    assert float(np.abs(lap[mask]).max()) < 1e-9 and 0 < its0 < 100
    # with a Laplacian term the dh_laplacian_blend system: subtracting lap moves the solution
    A, b, _, _ = I.system(known, mask)
    A2, b2, _, _ = I.system(known, mask, I.laplacian_f32(known))
    assert (A != A2).nnz == 0 and not np.array_equal(b, b2)
