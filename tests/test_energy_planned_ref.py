"""The float64 reference of the planned guidance-energy path (tests/energy_planned_ref.py), held on the CPU: against the
reference of the general path at h = w = grid, against the weighted statement of tests/object_weights_ref.py, the table of
what the cases make the kernels do, and -- for every item the GPU module runs -- the condition on the inputs under which no
gradient element is left out, so that a draw that breaks it fails here, before any GPU run."""
import numpy as np
import pytest
import torch

import energy_general_ref as G
import energy_planned_ref as R
import object_weights_ref as W
from oracle import guidance_ref as O

PLAIN = [it for it in R.SINGLES if it.kind == "plain" and it.C <= 320]
WEIGHTED = [it for it in R.SINGLES if it.kind != "plain"]


POOL = 1.0 + 1e-10


def _pooled(it):
    """(loss [3], grad) of the item's reference with its foreground term divided by POOL.  The oracle's energies and
    energy_general_ref.layer pool with the denominator avg_pool(w) + 1e-10, which at patch 1 is 1 + 1e-10 on every named cell:
    their foreground term, loss and gradient, is this reference's divided by exactly that, and is compared as such."""
    cur, org, donor = it.inputs()
    ref = it.ref()
    dn = donor if it.donor_bits else None
    fg = R.item(cur, org, it.cells(), it.fg_w, 0.0, it.grid, it.weights, dn, it.donor_bits)
    bg = R.item(cur, org, it.cells(), 0.0, it.bg_w, it.grid, it.weights, dn, it.donor_bits)
    assert float((fg["grad"] + bg["grad"] - ref["grad"]).abs().max()) <= 1e-15 and float(fg["loss"][1]) == float(ref["loss"][1])
    assert float((ref["mag"] - ref["grad"].abs()).min()) >= -1e-15          # the term magnitudes bound the element
    loss = torch.stack([it.fg_w * ref["loss"][1] / POOL + it.bg_w * ref["loss"][2], ref["loss"][1] / POOL, ref["loss"][2]])
    return loss, fg["grad"] / POOL + bg["grad"]


@pytest.mark.parametrize("it", PLAIN, ids=lambda c: c.id)
def test_reference_equals_the_general_reference_at_the_grid(it):
    """energy_general_ref.layer with maps at the grid, patch 1, global_avg: loss, gradient and global_d to 1e-12."""
    cur, org, _ = it.inputs()
    ref = it.ref()
    want = G.layer(cur, org, it.cells(), it.fg_w, it.bg_w, it.grid)
    loss, grad = _pooled(it)
    assert float((loss - want["loss"]).abs().max()) <= 1e-12
    assert float((grad - want["grad"]).abs().max()) <= 1e-12
    assert (ref["global_d"] is None) == (want["global_d"] is None)
    if ref["global_d"] is not None:
        assert float((ref["global_d"] - want["global_d"]).abs().max()) <= 1e-12


def _weighted_statement(it):
    """fw sum_m omega_m fg(a, src_m, cells_m) + bw bg(a, o, cells) from the oracle's two energies, src_m the donor map for the
    objects whose bit is set; autograd gradient.  Without donor bits this is object_weights_ref.energy."""
    cur, org, donor = it.inputs()
    cells, size = it.cells(), (it.grid, it.grid)
    a = cur.double().permute(2, 0, 1).contiguous().requires_grad_(True)
    o, dn = org.double().permute(2, 0, 1).contiguous(), donor.double().permute(2, 0, 1).contiguous()
    objects = cells["object"]
    if not it.donor_bits:
        tot, fg, bg = W.energy(a, o, cells, objects, it.weights, it.fg_w, it.bg_w, size=size)
    else:
        fg = bg = a.sum() * 0.0
        _, om = W.omegas(objects, it.weights)
        for m, w in enumerate(om):
            if w > 0.0:
                src = dn if (it.donor_bits >> m) & 1 else o
                fg = fg + w * O.foreground_energy(a, src, W.cells_of_object(cells, objects, m), 1, size)
        if cells["background_x_orig"].size and cells["background_x_trans"].size:
            bg = O.background_energy(a, o, cells, 1, size)
        tot = it.fg_w * fg + it.bg_w * bg
    grad, = torch.autograd.grad(tot, a, allow_unused=True)
    grad = torch.zeros_like(a) if grad is None else grad
    return torch.stack([tot, fg, bg]).detach(), grad.permute(1, 2, 0)


@pytest.mark.parametrize("it", WEIGHTED, ids=lambda c: c.id)
def test_weighted_reference_equals_the_weighted_statement(it):
    """object_weights_ref.energy (with donor bits: the same sum over the oracle's energies) and its autograd gradient: 1e-12"""
    want_loss, want_grad = _pooled(it)
    loss, grad = _weighted_statement(it)
    assert float((want_loss - loss).abs().max()) <= 1e-12
    assert float((want_grad - grad).abs().max()) <= 1e-12


def test_donor_bits_change_the_reference():
    """the donor map is drawn independently of orig: a set bit moves the gradient"""
    for it in WEIGHTED:
        if it.donor_bits:
            cur, org, _ = it.inputs()
            plain = R.item(cur, org, it.cells(), it.fg_w, it.bg_w, it.grid, it.weights)
            assert float((plain["grad"] - it.ref()["grad"]).abs().max()) > 0, it.id


def test_case_table_covers_what_the_kernels_branch_on():
    items = R.all_items()
    B = {it.id: R.branches(it) for it in items}
    plain = [it for it in R.SINGLES if it.kind == "plain"]
    weighted = [it for it in R.SINGLES if it.kind != "plain"]
    both = lambda its, f: {f(it) for it in its}
    union = lambda its, key: set().union(*(B[it.id][key] for it in its))
    # geometry and types
    for t in ("f16", "bf16"):
        assert {(it.grid, it.C) for it in plain if it.types == t} == set(R.GEOMETRY)
    for geo in R.WEIGHTED_GEOMETRY:
        assert {it.types for it in plain if (it.grid, it.C) == geo} == set(R.TYPES)
        for kind in ("objects", "donor"):
            got = {it.types for it in weighted if (it.grid, it.C) == geo and it.kind == kind}
            assert {"f16", "bf16"} <= got and any(R.TYPES[t][1] == R.F32 for t in got)
    assert both(weighted, lambda it: (it.grid, it.C)) == set(R.WEIGHTED_GEOMETRY)
    assert {256, 1} <= both(plain, lambda it: B[it.id]["cpb"])                                  # C = 8 and C >= 1280
    assert {True, False} == both(plain, lambda it: B[it.id]["ragged_last_block"])              # G2 % cpb
    assert {0, 4, 16, 96} <= both(plain, lambda it: B[it.id]["idle_lanes"])                     # 256 - cpb C/8
    assert {1, 8} <= both(plain, lambda it: B[it.id]["colsum_live_chunks_last"])                # k_colsum_q's last block
    assert any(B[it.id]["colsum_live_chunks_last"] < 8 and it.C > 64 for it in plain)           # ... behind full blocks
    # pair sets
    for its in (plain, weighted):
        assert {0, 1, 7, 8, 9, 15, 16, 17, 24, 41} <= union(its, "seg")
        assert {1, 2, 64, 300} <= union(its, "mult")
        assert max(B[it.id]["raw_max"] for it in its) > 256
        assert any(B[it.id]["n_pairs"] == 1 for it in its)
    for it in R.SINGLES:
        if it.pairs in ("hand", "objects"):
            G2 = it.grid ** 2
            assert {0, G2 - 1} <= B[it.id]["targets"], it.id
        if it.pairs == "hand":
            assert {0, it.grid ** 2 - 1} <= B[it.id]["sources"], it.id
    assert {"hand", "random", "none", "one", "cancel"} <= both(plain, lambda it: it.pairs)
    assert any(B[it.id]["n_pairs"] == 3000 for it in plain)
    # background lists: the slice lengths of k_colsum_q's three loops, the list lengths around one slice per row, unequal lists
    assert {1, 2, 8, 9, 17, 25, 32} <= union(plain, "per")
    lengths = set().union(*({n for n in it.bg} for it in plain))
    assert {0, 1, 100, 128, 129, 1000} <= lengths
    assert all(it.bg[0] != it.bg[1] or it.bg == (0, 0) for it in items)
    assert {(True, False), (False, True), (False, False)} <= both(plain, lambda it: (it.bg[0] > 0, it.bg[1] > 0))
    assert any(it.bg == (0, 0) and not B[it.id]["n_pairs"] for it in plain)
    assert any(B[it.id]["cancelling_cells"] >= 64 for it in plain) and any(B[it.id]["cancelling_cells"] >= 64 for it in weighted + items)
    assert {"mix", "fg", "bg", "cancel"} <= both(plain, lambda it: it.fwbw)
    assert {(R.F32, 1.0), (R.F32, 256.0), (R.F16, 256.0), (R.BF16, 256.0)} <= both(plain, lambda it: (it.grad_dtype, it.scale))
    # a weight per object
    for geo in R.WEIGHTED_GEOMETRY:
        its = [it for it in weighted if (it.grid, it.C) == geo]
        assert {1, 2, 8} <= both(its, lambda it: it.M)
        assert any(B[it.id]["eight_of_eight"] for it in its)
        ch = union(its, "changes")
        assert {("batch", 0, True), "tail"} <= ch and any(c != "tail" and 0 < c[1] < 8 for c in ch)
        assert all(("batch", j, False) in ch for j in range(1, 8))                              # a fold at every step of a batch
        assert any(f != 0 for f in union(its, "first_objects"))                                 # a segment that starts past object 0
        assert any(not all(B[it.id]["live"]) and all(w > 0 for w in it.weights) for it in its)   # no pairs, positive weight
        assert any(not all(B[it.id]["live"]) and 0.0 in it.weights for it in its)                # ... next to a weight 0
        assert any(len(set(it.weights)) == it.M > 1 for it in its)
        assert {"none", "one", "all"} <= both(its, lambda it: it.donor)
        assert any(it.donor_bits and it.donor_bits != (1 << it.M) - 1 for it in its)
    # what the three arithmetic mutants of DESIGN.md section 32 change is taken by some items and not by others
    for key in ("mult_in_batch", "folds"):
        assert {True, False} == both(R.SINGLES, lambda it: bool(B[it.id][key]))
    assert {True, False} == both([it for it in R.SINGLES if B[it.id]["use_bg"]], lambda it: B[it.id]["colsum_tail_rows"] > 0)
    # batches
    assert {(b.entry, b.K, b.grid, b.C) for b in R.BATCHES} == {(e, K, g, C) for e in ("plain", "objects", "mixed", "donor")
                                                               for K, g, C in ((2, 16, 72), (16, 16, 72), (16, 32, 320))}
    for b in R.BATCHES:
        assert len(b.items) == b.K
        assert any(B[it.id]["n_pairs"] == 0 for it in b.items) and any(not B[it.id]["use_bg"] for it in b.items)
        last = b.items[-1]
        sig = lambda it: (it.pairs, it.bg, it.fwbw, it.scale)
        assert all(sig(it) != sig(last) for it in b.items[:-1])
        assert len({sig(it) for it in b.items}) >= min(b.K, 8)
        kinds = {it.kind for it in b.items}
        assert kinds == {"plain": {"plain"}, "objects": {"objects"}, "mixed": {"plain", "objects"}, "donor": {"donor"}}[b.entry]
        if b.entry == "donor" and b.K > 2:
            assert {0} < {it.donor_bits for it in b.items}


@pytest.mark.parametrize("it", R.all_items(), ids=lambda c: c.id)
def test_global_d_condition_holds(it):
    """Every channel's background mean difference is at least 2^-10: sgn_c is certain, so no element of the item is left out.
    A draw that fails gets another seed in energy_planned_ref.SALT; the bound stays."""
    ref = it.ref()
    assert torch.isfinite(ref["grad"]).all() and torch.isfinite(ref["loss"]).all() and float(ref["mag"].min()) >= 0
    b = R.branches(it)
    assert (ref["global_d"] is not None) == b["use_bg"]
    if ref["global_d"] is not None:
        low = float(ref["global_d"].min())
        assert low >= R.GLOBAL_D_MIN, f"{it.id}: a channel's mean difference is {low:.3g}, choose another seed"
    assert np.array_equal(ref["seg"], np.bincount(R.entries(it.cells(), it.grid)[0][:, 1], minlength=it.grid ** 2))
