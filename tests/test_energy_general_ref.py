"""The float64 reference of the general guidance-energy path (tests/energy_general_ref.py), held on the CPU: against the
oracle's energy on the golden layers, against the explicit matrix form of the resize adjoint, and -- for every case the GPU
module runs -- the caps on what the comparison may leave out, so that a seed that breaks one fails here, before any GPU run."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import energy_general_ref as R
from oracle import guidance_ref as G


def test_reference_equals_oracle_on_golden_layers(golden):
    """Every g5 layer, patch 1 / 3, erosion 0 / 5, the three terms: loss and autograd gradient to 1e-12 in float64."""
    g3, g5 = golden("g3_zbuffer.npz"), golden("g5_energy.npz")
    corr = g3["t2_corr"].astype(np.int64)
    for er in (0, 5):
        cells = G.cells_from_correspondences(corr, 512, er)
        mine = R.cells_from_correspondences(corr, 512, er, 64)
        assert all(np.array_equal(mine[k], cells[k]) for k in cells)
        for li in range(3):
            cur, org = torch.from_numpy(g5[f"l{li}_cur"]).double(), torch.from_numpy(g5[f"l{li}_org"]).double()
            for patch in (1, 3):
                for kind in ("fg", "bg_global_avg", "bg_local_avg"):
                    a = cur.clone().requires_grad_(True)
                    if kind == "fg":
                        want = G.foreground_energy(a, org, cells, patch, (64, 64))
                        ref = R.layer(cur.permute(1, 2, 0), org.permute(1, 2, 0), mine, 1.0, 0.0, 64, fg_patch=patch)
                        got = ref["loss"][1]
                    else:
                        want = G.background_energy(a, org, cells, patch, (64, 64), kind[3:])
                        ref = R.layer(cur.permute(1, 2, 0), org.permute(1, 2, 0), mine, 0.0, 1.0, 64, bg_patch=patch,
                                      bg_mode=kind[3:])
                        got = ref["loss"][2]
                    gr, = torch.autograd.grad(want, a)
                    key = (er, li, patch, kind)
                    assert abs(float(got) - float(want.detach())) <= 1e-12, key
                    assert float(ref["loss"][0]) == float(got), key
                    assert float((ref["grad"].permute(2, 0, 1) - gr).abs().max()) <= 1e-12, key


@pytest.mark.parametrize("shape", [(5, 7, 64), (16, 16, 96), (100, 32, 64)], ids=str)
def test_resized_gradient_is_the_matrix_adjoint(shape):
    """grad = Wy^T G Wx per channel, W from F.interpolate of an identity, G the gradient on the grid; and the resize itself
    is Wy X Wx^T.  Float64, mixed terms, patch 3 foreground."""
    h, w, grid = shape
    gen = torch.Generator().manual_seed(30)
    cur, org = (torch.randn(h, w, 6, generator=gen, dtype=torch.float64) for _ in range(2))
    cells = R.cells_from_correspondences(torch.randint(0, 8 * grid, (500, 4), generator=gen).numpy(), 8 * grid, 0, grid)
    ref = R.layer(cur, org, cells, 3.0, 2.0, grid, fg_patch=3)
    Wy, Wx = R.resize_matrix(h, grid), R.resize_matrix(w, grid)
    assert torch.equal((Wy > 0).sum(1).clamp(max=2), (Wy > 0).sum(1)) and float((Wy.sum(1) - 1).abs().max()) < 1e-15
    resized = F.interpolate(cur.permute(2, 0, 1)[None], (grid, grid), mode="bilinear")[0]
    assert float((torch.einsum("yi,ijc,xj->cyx", Wy, cur, Wx) - resized).abs().max()) < 1e-14
    want = torch.einsum("yi,yxc,xj->ijc", Wy, ref["grad_grid"], Wx)
    assert float(ref["grad_grid"].abs().max()) > 0
    assert float((ref["grad"] - want).abs().max()) <= 1e-15 * float(want.abs().max()) * grid


def test_min_d_names_the_differences_that_enter_an_element():
    """One pair, fg only, 8 -> 64: min_d is |d| of that pair on exactly the input cells the target cell reads, inf elsewhere;
    a gradient element is non-zero exactly where min_d is finite."""
    gen = torch.Generator().manual_seed(31)
    cur, org = (torch.randn(8, 8, 3, generator=gen, dtype=torch.float64) for _ in range(2))
    cells = R.cells_from_correspondences(np.array([[100, 200, 8 * 27 + 1, 8 * 11 + 1]]), 512, 0, 64)      # target cell (11, 27)
    ref = R.layer(cur, org, cells, 1.0, 0.0, 64)
    finite = torch.isfinite(ref["min_d"])
    assert torch.equal(finite, ref["grad"] != 0)
    assert finite.any(-1).nonzero().tolist() == [[0, 2], [0, 3], [1, 2], [1, 3]]      # s = 0.9375 in y, 2.9375 in x
    f = lambda t: F.interpolate(t.permute(2, 0, 1)[None], (64, 64), mode="bilinear")[0]
    d = (f(org)[:, 25, 12] - f(cur)[:, 11, 27]).abs()
    assert float((ref["min_d"][0, 2] - d).abs().max()) < 1e-9      # (the 1e-10 of the pooling denominator)


def test_far_reader_lies_beyond_the_old_window_below_a_quarter():
    """The centre target of the footprint cases: inside floor((yi - 1) / sy) - 1 .. ceil((yi + 1) / sy) + 1 at every ratio from
    1/4 up, outside it at the three smaller ratios -- a footprint there is what the old gather window dropped."""
    for h, _, grid in R.SHAPES:
        yi, sy = max(h // 2 - 1, 0), h / grid
        y = R.far_reader(h, grid)
        inside = np.floor((yi - 1) / sy) - 1 <= y <= np.ceil((yi + 1) / sy) + 1
        assert inside == ((h, h, grid) not in R.BELOW), (h, grid, y)


def test_case_table_covers_what_the_kernels_branch_on():
    by = lambda f: {f(c) for c in R.CASES}
    assert by(lambda c: (c.h, c.w, c.grid)) == set(R.SHAPES)
    for t in ("f16", "f32"):
        assert {(c.h, c.w, c.grid) for c in R.CASES if c.types == t and c.kind == "terms"} == set(R.SHAPES)
    assert by(lambda c: (c.C, c.types)) == {(C, t) for C in (8, 72, 320) for t in R.TYPES}
    assert {(c.h, c.w, c.grid) for c in R.CASES if c.patch == 3} == {R.PRODUCT, (8, 8, 64)}
    assert all(c.C in (8, 72) for c in R.CASES if (c.h, c.w, c.grid) == R.PRODUCT96)
    assert all((c.h, c.w, c.grid) in R.DYADIC and c.patch == 1 for c in R.CASES if c.exact)
    assert by(lambda c: c.pairs) == {"window", "image", "image2k", "single", "none"} and by(lambda c: c.erosion) == {0, 5}


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_caps_hold(case):
    """At most 1e-4 of a call's gradient elements below tau, no global_avg channel below tau, and in the exact cases the
    premise of leaving nothing out: the resized maps and all pair differences are the same numbers in f32 and in float64."""
    cur, org = case.inputs()
    t = R.tau(cur, org)
    for label, corr in case.correspondences():
        cells = R.cells_from_correspondences(corr.numpy(), case.img_res, case.erosion, case.grid)
        for call in case.calls():
            ref = R.layer(cur, org, cells, call.fg_w, call.bg_w, case.grid, case.patch, case.patch, call.bg_mode)
            on_grid, left_out = R.check_caps(case, call, ref, t)
            assert (on_grid == 0.0 and left_out == 0.0) or not case.certain
            assert torch.isfinite(ref["grad"]).all() and torch.isfinite(ref["loss"]).all()
            print(f"{case.id}\t{label}\t{call.name}\tbelow tau on the grid {on_grid:.3g}\tleft out {left_out:.3g}")
    if case.exact:
        size = (case.grid, case.grid)
        for m in (cur, org):
            lo = F.interpolate(m.float().permute(2, 0, 1)[None], size, mode="bilinear")
            hi = F.interpolate(m.double().permute(2, 0, 1)[None], size, mode="bilinear")
            assert torch.equal(lo.double(), hi)
            assert float(hi.abs().max()) <= 4 and torch.equal(hi * 2 ** 11, (hi * 2 ** 11).round())      # |d| <= 8 on a 2^-11 lattice
