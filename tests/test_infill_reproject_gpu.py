"""GPU: the harmonic in-fill as the batched re-projection calls launch it -- k_cg_fill_multi on grid (16, K) and k_cg_fill on grid
(K) at the end of dh_reproject_instance_edits and dh_reproject_background: K systems of different solver classes in one launch,
each leaving one of the two kernels early; the scratch carved out of dead buffers (the z-buffer as the up / down neighbour list,
the key list as the left / right one with stride res^2 + n_pts, the owner map as the pixel -> unknown map); one CgSync per edit;
no Laplacian term; a cap of 20 000; with footprints, in-fill buffers that held the keep flags before.
tests/test_infill_solvers_gpu.py reaches the same three solvers one system per launch through dh_laplacian_blend only.

Every edit of every call goes through `_check`: the in-fill set from the call's OWN masks, its size in counts[e, 2], the solver
class of that size, then tests/infill_ref.reference (f64 direct solve + classic CG) built from the call's own disparity outside
the set -- k_normalize's output, which the in-fill never writes -- and

    max |out - x_ref| over the set  <=  4 * 2^-24 * max |x_ref|          (f32 rounding of an f64 solution; about 6e-5 of 255)
    0 <= counts[e, 3] <= 1.05 * its_ref + 5                               (the rule of tests/test_infill_solvers_gpu.py)

The cases are those of tests/infill_ref.py; tests/test_infill_ref.py pins their sizes, classes and classic counts on the CPU and
shows that the oracle's own in-fill holds the error gate with a factor of 8 to spare."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infill_ref as I  # noqa: E402
import multi_object_ref as R  # noqa: E402

from diffusionhandles_amd.synthetic import TRANSFORMS, make_scene  # noqa: E402

pytestmark = pytest.mark.gpu

# rows of infill_ref.SCALED in the order of the K = 5 call: s = 2.8, 1.0, 2.6, 1.5, 2.0 -- single first, lds second, so that the
# class does not rise with the edit index
ORDER = (4, 0, 3, 1, 2)


def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _t(tf):
    return (float(tf[0]), torch.tensor(tf[1], dtype=torch.float32), torch.tensor(tf[2], dtype=torch.float32)) + tuple(tf[3:])


def _K():
    from oracle import depth_ref as D
    return D.intrinsics_f32()


def _check(what, disp, inpaint, counts_row, solver, n=None, its_pinned=None):
    """The common check of one edit.  disp: [res, res] f32, the returned disparity; inpaint: [res, res] bool, from the call's own
    outputs; counts_row: the edit's four counts; n, its_pinned: the pinned size and classic count where the case has them."""
    n_call, its = int(counts_row[2]), int(counts_row[3])
    assert n_call == int(inpaint.sum()), (what, n_call, int(inpaint.sum()))
    if n is not None:
        assert n_call == n, (what, n_call, n)
    assert I.solver_of(n_call) == solver, (what, n_call, I.solver_of(n_call))
    assert disp.dtype == np.float32 and np.isfinite(disp[~inpaint]).all(), what      # the known pixels: k_normalize's output
    finite = bool(np.isfinite(disp).all())
    x_ref, its_ref = I.reference(disp, inpaint)
    bound = I.bound(x_ref, inpaint)
    err = float(np.abs(disp.astype(np.float64) - x_ref)[inpaint].max()) if finite else float("nan")
    print(f"in-fill {what}: n {n_call} ({solver}), its_ref {its_ref}, iterations {its}, max abs err {err:.3e} (bound {bound:.3e})")
    if its_pinned is not None:
        assert abs(its_ref - its_pinned) <= 2, (what, its_ref, its_pinned)
    assert finite, what
    assert err <= bound, (what, err, bound)
    assert 0 <= its <= 1.05 * its_ref + 5, (what, its, its_ref)


def _inpaint_of(dbg, e):
    return (dbg["clean_mask"][e].cpu().numpy() != 0) != (dbg["raw_mask"][e].cpu().numpy() != 0)


def _spheres_call(order, footprints=False):
    """One reproject_object_edits call on two_spheres(512) with the edits of SCALED in `order`; everything on the host."""
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, masks = R.two_spheres(I.RES)
    edits = [[_t(tf) for tf in I.scaled_edit(i)] for i in order]
    out, dbg = DT.reproject_object_edits(depth.to(dev()), bg.to(dev()), [m.to(dev()) for m in masks], _K(), edits,
                                         return_debug=True, footprints=footprints)
    assert len(out) == len(order) and tuple(dbg["counts"].shape) == (len(order), 4)
    return dict(disp=[o[0][0, 0].cpu().numpy() for o in out], corr=[o[1].numpy() for o in out], counts=dbg["counts"].numpy().copy(),
                inpaint=[_inpaint_of(dbg, e) for e in range(len(order))],
                raw=(dbg["raw_mask"].cpu().numpy() != 0), clean=(dbg["clean_mask"].cpu().numpy() != 0))


@functools.lru_cache(maxsize=None)
def _five(footprints=False):
    """The K = 5 call, shared by the tests that only read it."""
    return _spheres_call(ORDER, footprints)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- a. mixed classes in one launch, point mode -------------------------------------------------------------------------------
def test_mixed_classes_in_one_launch():
    """K = 5 on two_spheres(512): single (71 545 unknowns), lds (1 036), multi (63 216, one residual replacement), multi (22 303),
    multi (41 889) in ONE pair of launches.  The masks and correspondences are the oracle's bit for bit, so the in-fill sets are."""
    c = _five()
    assert [I.SCALED[i][3] for i in ORDER] == ["single", "lds", "multi", "multi", "multi"]
    assert c["counts"][:, 2].tolist() == [I.SCALED[i][2] for i in ORDER]
    for e, i in enumerate(ORDER):
        s, _, n, solver, its_pinned = I.SCALED[i]
        _, corr_r, dbg_r = I.scaled_oracle(i)
        assert np.array_equal(c["raw"][e], dbg_r["raw_mask"]), f"edit {e}: raw mask"
        assert np.array_equal(c["clean"][e], dbg_r["cleaned"] != 0), f"edit {e}: clean mask"
        assert np.array_equal(c["inpaint"][e], dbg_r["inpaint"]), f"edit {e}: in-fill set"
        assert np.array_equal(c["corr"][e], corr_r.numpy()), f"edit {e}: correspondences (order included)"
        assert int(c["counts"][e, 0]) == len(corr_r) and int(c["counts"][e, 1]) == int(dbg_r["vis"].sum())
        _check(f"K = 5 point mode, edit {e} (scale {s})", c["disp"][e], c["inpaint"][e], c["counts"][e], solver, n, its_pinned)


# ---- b. neighbours do not matter ------------------------------------------------------------------------------------------------
def test_an_edit_does_not_depend_on_its_neighbours_in_the_launch():
    """Each of the five edits alone (K = 1), the five in reversed order and the same call again: per edit the same disparity bits
    and the same in-fill size and iteration count as in the K = 5 call."""
    c = _five()
    again = _spheres_call(ORDER)
    assert np.array_equal(again["counts"], c["counts"])
    for e in range(5):
        assert np.array_equal(_bits(again["disp"][e]), _bits(c["disp"][e])), f"second call, edit {e}"
    rev = _spheres_call(ORDER[::-1])
    for e in range(5):
        assert np.array_equal(rev["counts"][4 - e], c["counts"][e]), f"reversed order, edit {e}: {rev['counts'][4 - e]} {c['counts'][e]}"
        assert np.array_equal(_bits(rev["disp"][4 - e]), _bits(c["disp"][e])), f"reversed order, edit {e}"
    for e, i in enumerate(ORDER):
        one = _spheres_call((i,))
        assert np.array_equal(one["counts"][0, 2:4], c["counts"][e, 2:4]), f"K = 1, edit {e}: {one['counts'][0]} {c['counts'][e]}"
        assert np.array_equal(_bits(one["disp"][0]), _bits(c["disp"][e])), f"K = 1, edit {e}"


# ---- c. footprint mode ------------------------------------------------------------------------------------------------------------
def test_footprint_mode_rewrites_the_buffers_that_held_the_keep_flags():
    """The same five edits with footprints: the triangles close the lattice, so the in-fill sets are about 1 300 pixels (on chip);
    but w.inpaint / w.unk have held the keep flags and their compacted list -- 35 000 .. 97 000 rows per edit -- before k_normalize
    and the second compaction rewrite them.  Masks and correspondences against tests/footprints_ref.py, bit for bit."""
    c = _five(True)
    assert c["counts"][:, 2].tolist() == [I.FOOTPRINT_N[i] for i in ORDER]
    for e, i in enumerate(ORDER):
        _, corr_r, dbg_r = I.footprint_oracle(i)
        assert np.array_equal(c["raw"][e], dbg_r["raw_mask"]), f"edit {e}: raw mask"
        assert np.array_equal(c["clean"][e], dbg_r["cleaned"] != 0), f"edit {e}: clean mask"
        assert int(c["counts"][e, 0]) == len(corr_r) > 20 * I.FOOTPRINT_N[i]
        assert np.array_equal(c["corr"][e], corr_r.numpy()), f"edit {e}: correspondences (order included)"
        _check(f"K = 5 footprints, edit {e} (scale {I.SCALED[i][0]})", c["disp"][e], c["inpaint"][e], c["counts"][e], "lds", I.FOOTPRINT_N[i])


# ---- d. the one-edit background carving ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(I.BACKGROUND)))
def test_background_alone_frame(i):
    """dh_reproject_background (the call of tests/test_object_removal_gpu.py) at 512 with a longer lens for the un-projection:
    a frame of 52 380 (multi, six residual replacements) / 94 044 (single) unknowns that reaches the image's first and last rows
    and columns, on the one-edit carving whose key list has stride res^2."""
    import test_object_removal_gpu as TR
    factor, n, solver, its_pinned = I.BACKGROUND[i]
    _, bg, _ = R.two_spheres(I.RES)
    _, dbg_r = I.background_oracle(i)
    o = TR._background_call(bg, I.RES, K_unproject=I.longer_lens(factor))
    assert o.rc == 0, o.err
    zmap = o.zmap.cpu().numpy()
    assert np.array_equal(zmap, dbg_r["zmap"]), "zmap"
    unowned = np.isinf(zmap)
    assert np.array_equal(unowned, dbg_r["unowned"]) and unowned[0].all() and unowned[:, -1].all()
    counts = o.counts.cpu().numpy()
    assert counts[:2].tolist() == [0, 0]
    _check(f"background alone, lens factor {factor}", o.disp.cpu().numpy(), unowned, counts, solver, n, its_pinned)


# ---- e. the existing mixed batch ----------------------------------------------------------------------------------------------
def test_six_transforms_of_the_synthetic_scene_over_every_infill_pixel():
    """make_scene(512), TRANSFORMS[0..5] in one reproject_edits call (the batch of tests/test_geometry_gpu.py, which compares
    [::5, ::7] slices to 2e-3): lds, lds, multi, multi, lds, multi, every in-fill pixel against the f64 solve."""
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, mask = make_scene(I.RES)
    tf = [(TRANSFORMS[i][0], torch.tensor([0.0, 1.0, 0.0]), torch.tensor(TRANSFORMS[i][1])) for i in range(6)]
    out, dbg = DT.reproject_edits(depth.to(dev()), bg.to(dev()), mask.to(dev()), _K(), tf, return_debug=True)
    counts = dbg["counts"].numpy()
    assert counts[:, 2].tolist() == [n for n, _ in I.MIXED]
    for e, (n, solver) in enumerate(I.MIXED):
        _check(f"make_scene(512), transform {e}", out[e][0][0, 0].cpu().numpy(), _inpaint_of(dbg, e), counts[e], solver, n)
