"""GPU: guard bands and stale workspaces for every entry that takes caller memory -- the re-projection, Laplacian blend, mesh,
cells, keep-map and energy calls, through their Python callers (where the sizes of the outputs and workspaces are decided).

Every case runs four times: once per fill of tests/guarded.py (0x00, 0xFF, seeded random bytes) with the caller's `torch`
replaced by a guarded frame, the arena gap (dh_dbg_arena_gap) at 4096 bytes and the take log on, and once plainly.  It asserts
  (a) every guard byte around every tensor the caller allocated is intact,
  (b) every byte of a workspace arena that no sub-buffer covers (alignment padding, the 4096-byte gaps, the slack at the end) is
      what it was before the call,
  (c) the output elements the interface documents as unwritten hold their pre-call bytes,
  (d) the documented results are bit-identical across the three fills and the plain call (nothing reads a word before this call
      wrote it, nothing depends on the layout).
No tolerance anywhere and no reference: the existing tests hold the plain call to its references."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_moves_ref as CM  # noqa: E402  (scene builders only)
import guarded as G  # noqa: E402
import infill_ref as IR  # noqa: E402  (the solver limits)
import multi_object_ref as R  # noqa: E402
import object_insertion_ref as OI  # noqa: E402

from diffusionhandles_amd import _lib  # noqa: E402
from diffusionhandles_amd import background_lock as BL  # noqa: E402
from diffusionhandles_amd import depth_transform as DT  # noqa: E402
from diffusionhandles_amd import losses as LS  # noqa: E402
from diffusionhandles_amd.synthetic import make_scene  # noqa: E402

pytestmark = pytest.mark.gpu
GAP = 4096
Y = R.Y
Z0 = (0.0, 0.0, 0.0)


@pytest.fixture
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def hooks_at_their_defaults():
    yield
    L = _lib.lib()
    G.arena_reset(L)
    L.dh_dbg_footprint_tier(0)
    LS._WS.clear()


def _bytes(v):
    t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
    t = t.detach().contiguous().cpu().reshape(-1)
    return t.view(torch.uint8) if t.numel() else torch.zeros(0, dtype=torch.uint8)


def guarded_runs(monkeypatch, dev, modules, call, digest, unwritten=None, arenas=1, prepare=None):
    """`call()` three times inside a frame (one per fill) and once plainly; (a), (b), `unwritten(frame, result)` for (c) on each
    framed run, and (d) over the four digests.  arenas: how many logged arenas at least must lie inside frame tensors (0 for an
    entry without an arena).  prepare: run before every call (clearing a cache of the module)."""
    L = _lib.lib()
    digests = []
    for fill in G.FILLS + (None,):
        if prepare:
            prepare()
        if fill is None:
            result = call()
            torch.cuda.synchronize()
            digests.append(("plain", {k: _bytes(v) for k, v in digest(result).items()}))
            continue
        frame = G.Frame(fill, dev)
        proxy = G.TorchProxy(frame)
        with monkeypatch.context() as m:
            for mod in modules:
                m.setattr(mod, "torch", proxy)
            assert G.arena_gap(L, GAP) == 0
            G.arena_log_start(L)
            try:
                result = call()
                torch.cuda.synchronize()
                takes = G.arena_log_read(L)
            finally:
                G.arena_reset(L)
        assert frame.recs, "the caller allocated nothing through the proxy"
        frame.check()                                                  # (a)
        judged = frame.check_arena_gaps(takes)                         # (b)
        assert judged >= arenas, f"{judged} logged arenas lie in frame tensors, expected at least {arenas} (fill {fill})"
        if unwritten:
            unwritten(frame, result)                                   # (c)
        digests.append((fill, {k: _bytes(v) for k, v in digest(result).items()}))
    name0, d0 = digests[-1]
    for name, d in digests[:-1]:                                       # (d)
        assert d.keys() == d0.keys(), (name, sorted(d.keys() ^ d0.keys()))
        for k in d0:
            assert d[k].shape == d0[k].shape and torch.equal(d[k], d0[k]), f"{k}: fill {name} differs from the {name0} call"
    return digests


# ---- re-projection ----------------------------------------------------------------------------------------------------------
def _K():
    from oracle import depth_ref as D
    return D.intrinsics_f32()


def _reproject_digest(result):
    out, dbg = result
    d = {}
    for e, tup in enumerate(out):
        for j, t in enumerate(tup):
            d[f"out{e}.{j}"] = t
    counts = dbg["counts"]
    for k in ("zmap", "raw_mask", "clean_mask", "vis", "target_xy", "counts", "fg_pix", "vacated", "bg_counts", "bg_valid", "obj_start",
              "inst_start"):
        if k in dbg:
            d[k] = dbg[k]
    bgc = dbg["bg_counts"].cpu().tolist() if "bg_counts" in dbg else None
    for e in range(len(out)):
        n = int(counts[e, 0])
        d[f"corr{e}"] = dbg["corr_dev"][e, :n]
        for k in ("corr_inst", "row_donor"):
            if k in dbg:
                d[f"{k}{e}"] = dbg[k][e, :n]
        if bgc is not None:
            d[f"bg_corr{e}"] = dbg["bg_corr"][e, :bgc[e]]
    return d


def _reproject_unwritten(frame, result):
    """corr / corr_inst past the count, the background rows past theirs, fg_pix past n_fg"""
    out, dbg = result
    counts = dbg["counts"]
    bgc = dbg["bg_counts"].cpu().tolist() if "bg_counts" in dbg else None
    for e in range(len(out)):
        n = int(counts[e, 0])
        frame.unchanged(dbg["corr_dev"][e, n:], f"corr[{e}, {n}:]")
        if "corr_inst" in dbg and frame.rec_of(dbg["corr_inst"].data_ptr()) is not None:
            frame.unchanged(dbg["corr_inst"][e, n:], f"corr_inst[{e}, {n}:]")
        if bgc is not None:
            frame.unchanged(dbg["bg_corr"][e, bgc[e]:], f"bg_corr[{e}, {bgc[e]}:]")
    if dbg["fg_pix"].numel():
        frame.tail_unchanged(dbg["fg_pix"], "fg_pix past n_fg")


def _reproject(monkeypatch, dev, depth, bg, masks, edits, check=None, **kw):
    to = lambda t: t.to(dev)
    for k in ("removed_masks", "donor_masks"):
        if kw.get(k) is not None:
            kw[k] = [to(m) for m in kw[k]]
    if kw.get("donor_depth") is not None:
        kw["donor_depth"] = to(kw["donor_depth"])
    d, b, ms, Kc = to(depth), to(bg), [to(m) for m in masks], _K()

    def call():
        return DT.reproject(d, b, ms, Kc, edits, return_debug=True, device_correspondences=True, **kw)

    runs = guarded_runs(monkeypatch, dev, [DT], call, _reproject_digest, _reproject_unwritten)
    counts = runs[-1][1]["counts"].view(torch.int32).reshape(-1, 4)
    assert (counts[:, 3] >= 0).all(), counts
    if check:
        check(counts)
    return counts


def _block_scene(res, mask):
    """make_scene's background with the pixels of `mask` (bool [res, res]) one unit nearer"""
    _, bg, _ = make_scene(res)
    m = torch.from_numpy(mask)[None, None]
    return torch.where(m, bg - 1.0, bg).contiguous(), bg, [m.to(torch.float32)]


THREE = [[(0.0, Y, (-0.8, 0.0, 0.0)), (-30.0, Y, Z0)],
         [(25.0, Y, (0.0, -0.9, 0.3)), (0.0, Y, Z0)],
         [(-15.0, (0.3, 0.9, -0.2), (0.1, 0.6, 0.2)), (10.0, Y, (0.3, 0.0, -0.2))]]


@pytest.mark.parametrize("res", [64, 60])
def test_reproject_two_objects(monkeypatch, dev, res):
    """res 64: R2 = 2 CP_TILE, bit-row morphology; res 60: byte morphology, ragged last compaction tile"""
    depth, bg, masks = R.two_spheres(res)
    _reproject(monkeypatch, dev, depth, bg, masks, THREE)


@pytest.mark.parametrize("what", ["one_pixel", "all_but_a_border"])
def test_reproject_extreme_masks(monkeypatch, dev, what):
    res = 64
    m = np.zeros((res, res), dtype=bool)
    if what == "one_pixel":
        m[31, 29] = True
    else:
        m[2:-2, 2:-2] = True
    depth, bg, masks = _block_scene(res, m)
    edits = [[(0.0, Y, (-0.2, 0.0, 0.0))], [(20.0, Y, Z0)], [(0.0, Y, (0.1, 0.1, -0.3))]]
    counts = _reproject(monkeypatch, dev, depth, bg, masks, edits)
    assert int(m.sum()) in (1, 3600)
    assert (counts[:, 0] <= int(m.sum())).all()


@pytest.mark.parametrize("what", ["plain", "max_ratio", "wave_tier"])
def test_reproject_footprints(monkeypatch, dev, what):
    """scale 2.5: more rows than points, the res * res capacity in use; the wave tier's big_list with the tier at 1"""
    res = 64
    depth, bg, masks = R.two_spheres(res)
    edits = [[(0.0, Y, (0.2, 0.0, 0.0), 2.5, None), (0.0, Y, Z0)],
             [(25.0, Y, (0.0, -0.3, 0.3), 2.5, None), (-30.0, Y, Z0, 1.5, None)],
             [(0.0, Y, Z0), (10.0, Y, (0.3, 0.0, -0.2), (2.5, 1.0, 2.5), None)]]
    if what == "wave_tier":
        assert _lib.lib().dh_dbg_footprint_tier(1) == 0
    n_fg = int(sum(int(m.sum()) for m in masks))
    counts = _reproject(monkeypatch, dev, depth, bg, masks, edits, footprints=True,
                        footprint_max_ratio=1.02 if what == "max_ratio" else None)
    assert int(counts[:, 0].max()) > n_fg, (counts, n_fg)


def test_reproject_instances_more_points_than_pixels(monkeypatch, dev):
    """one mask of 61 % of the image drawn twice: n_pts > R2 and P > 2 R2"""
    res = 64
    m = np.zeros((res, res), dtype=bool)
    m[8:56, 6:58] = True
    assert 2 * int(m.sum()) > res * res
    depth, bg, masks = _block_scene(res, m)
    edits = [[(0.0, Y, (-0.3, 0.0, 0.0)), (0.0, Y, (0.3, 0.0, 0.2))],
             [(10.0, Y, Z0), (-10.0, Y, (0.0, 0.2, -0.1))],
             [(0.0, Y, Z0), (0.0, Y, Z0)]]
    _reproject(monkeypatch, dev, depth, bg, masks, edits, instances=[0, 0], return_instances=True)


def test_reproject_donor(monkeypatch, dev):
    res = 64
    depth, bg, masks = R.two_spheres(res)
    ddepth, dmasks = OI.donor_scene(res, "overlap")
    pv = OI.donor_pivot(ddepth, "overlap")
    # the host image keeps sphere 1 as it is (it is part of `depth` and of `bg`): the one host mask is sphere 0
    host_bg = torch.where(masks[1] > 0, depth, bg)
    edits = [[(0.0, Y, (-0.3, 0.0, 0.0)), (20.0, Y, (0.45, 0.55, 0.2), 0.8, pv)],
             [(10.0, Y, (0.1, 0.0, 0.0)), (-15.0, (0.3, 0.9, -0.2), (-0.3, 0.5, 0.4), 1.2, pv)],
             [(0.0, Y, Z0), (0.0, Y, Z0)]]
    _reproject(monkeypatch, dev, depth, host_bg, [masks[0]], edits, donor_depth=ddepth, donor_masks=dmasks)


def _cams(depth):
    c = CM.cameras_for(depth)
    return [c["general"], None, c["orbit"]]


@pytest.mark.parametrize("what", ["views_and_none", "with_removed_masks"])
def test_reproject_camera(monkeypatch, dev, what):
    """one edit with a view, one without, one with another view -- and the same with a removed mask"""
    res = 64
    depth, bg, masks = R.two_spheres(res)
    if what == "views_and_none":
        _reproject(monkeypatch, dev, depth, bg, masks, THREE, cameras=_cams(depth))
    else:
        _reproject(monkeypatch, dev, depth, bg, [masks[0]], [tfs[:1] for tfs in THREE], removed_masks=[masks[1]], cameras=_cams(depth))


@pytest.mark.parametrize("what", ["with_foreground", "pure_removal", "pure_camera"])
def test_reproject_removal(monkeypatch, dev, what):
    res = 64
    depth, bg, masks = R.two_spheres(res)
    if what == "with_foreground":
        _reproject(monkeypatch, dev, depth, bg, [masks[0]], [tfs[:1] for tfs in THREE], removed_masks=[masks[1]])
    elif what == "pure_removal":
        _reproject(monkeypatch, dev, depth, bg, [], [[], [], []], removed_masks=masks)
    else:
        _reproject(monkeypatch, dev, depth, depth, [], [[], [], []], cameras=_cams(depth))


def _dolly(z):
    return (0.0, Y, (0.0, 0.0, z), None)


@pytest.mark.parametrize("solver,res,zs", [("lds", 64, (-0.5, -1.0, -2.0)), ("multi", 128, (-3.0, -4.0, -5.0)), ("single", 288, (-9.0,))])
def test_reproject_every_infill_class(monkeypatch, dev, solver, res, zs):
    """One call per in-fill class at the smallest size that reaches it: the camera backs away, the pixels no point reaches are
    in-filled.  The pipelined and the single-workgroup solver keep their neighbour tables in zbuf and key."""
    depth, bg, masks = R.two_spheres(res)
    edits = [[(0.0, Y, Z0), (0.0, Y, Z0)] for _ in zs]

    def check(counts):
        for e in range(len(zs)):
            assert IR.solver_of(int(counts[e, 2])) == solver and int(counts[e, 2]) > 0, (solver, counts)

    _reproject(monkeypatch, dev, depth, bg, masks, edits, cameras=[_dolly(z) for z in zs], check=check)


# ---- Laplacian blend --------------------------------------------------------------------------------------------------------
def _blend(monkeypatch, dev, depth, bg, mask, dilate):
    d, b, m = depth.to(dev), bg.to(dev), mask.to(dev)
    call = lambda: DT.laplacian_depth_blend(d, b, m, dilate_iterations=dilate, return_iterations=True)
    guarded_runs(monkeypatch, dev, [DT], call, lambda r: dict(out=r[0], iterations=np.int64(r[1])))


def _wavy(bg):
    res = bg.shape[-1]
    return bg + 0.05 * torch.sin(torch.arange(res, dtype=torch.float32) / 9.0)[None, None, None, :]


@pytest.mark.parametrize("res,dilate", [(64, 0), (64, 3), (100, 3)])
def test_laplacian_blend(monkeypatch, dev, res, dilate):
    depth, bg, mask = make_scene(res)
    _blend(monkeypatch, dev, depth, _wavy(bg), mask, dilate)


@pytest.mark.parametrize("solver,res,side", [("lds", 64, 60), ("multi", 96, 92), ("single", 261, 257)])
def test_laplacian_blend_every_cg_class(monkeypatch, dev, solver, res, side):
    """a square hole per CG kernel (test_laplacian_blend_every_cg_kernel_vs_oracle sizes them at res 512) at the smallest
    resolution that holds it with a border of two known pixels"""
    assert IR.solver_of(side * side) == solver
    depth, bg, _ = make_scene(res)
    mask = torch.zeros(1, 1, res, res, dtype=torch.bool)
    a = (res - side) // 2
    mask[0, 0, a:a + side, a:a + side] = True
    _blend(monkeypatch, dev, depth, _wavy(bg), mask, 0)


# ---- mesh -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [32, 47])
def test_mesh(monkeypatch, dev, res):
    """res 47: R2 = 2209, one past a compaction tile"""
    depth, bg, mask = make_scene(res)
    d, b, m, Kc = depth.to(dev), bg.to(dev), mask.to(dev), _K()

    def call():
        return DT.transform_depth_mesh(d, b, m, Kc, rot_angle=30.0, translation=torch.tensor([0.1, 0.0, -0.1]), return_debug=True)

    def unwritten(frame, r):
        corr, = frame.find((res * res, 4), torch.int64)
        frame.unchanged(corr[r[1].shape[0]:], "corr past counts[0]")

    guarded_runs(monkeypatch, dev, [DT], call, lambda r: dict(disp=r[0], corr=r[1], zmap=r[2]["zmap"], fg_flag=r[2]["fg_flag"]), unwritten)


# ---- cells ------------------------------------------------------------------------------------------------------------------
CELL_VARIANTS = ("plain", "vacated", "donor", "donor_vacated", "rows", "rows_vacated")


def _cell_rows(n, img_res, seed):
    g = torch.Generator().manual_seed(seed)
    corr = torch.randint(0, img_res, (n, 4), generator=g, dtype=torch.int64)
    if n >= 8:                                   # a few rows the validity test drops: the pair list is shorter than n
        corr[3, 2], corr[5, 3], corr[n - 1, 2] = -1, img_res, img_res + 7
    return corr, torch.randint(0, 2, (n,), generator=g, dtype=torch.uint8), torch.randint(0, 3, (n,), generator=g, dtype=torch.uint8)


@pytest.mark.parametrize("variant", CELL_VARIANTS)
@pytest.mark.parametrize("erosion", [0, 5])
@pytest.mark.parametrize("n", [0, 1, 2048, 2049])
def test_cells(monkeypatch, dev, n, erosion, variant):
    img_res, grid = 128, 64
    corr, flags, kinds = _cell_rows(n, img_res, 100 + n)
    kw = {}
    if "vacated" in variant:
        vac = torch.zeros(img_res, img_res, dtype=torch.uint8)
        vac[20:50, 70:110] = 1
        kw["vacated"] = vac
    if variant.startswith("donor"):
        kw["row_donor"] = flags
    if variant.startswith("rows"):
        kw["row_kind"] = kinds
    call = lambda: LS.process_correspondences(corr, img_res, erosion, grid=grid, device=dev, **kw)

    def digest(pc):
        d = {k: v for k, v in pc.items()}
        d.update({f"dl_{k}": v for k, v in pc.device_lists.items() if k != "grid"})
        return d

    def unwritten(frame, pc):
        pairs, = frame.find((max(n, 1), 2), torch.int32)
        lists, = frame.find((3, grid * grid), torch.int32)
        frame.unchanged(pairs[pc.device_lists["pairs"].shape[0]:], "pairs past counts[0]")
        for k, name in enumerate(("bg_both", "bg_orig", "bg_trans")):
            frame.unchanged(lists[k, pc.device_lists[name].shape[0]:], f"bg_lists[{k}] past its count")

    guarded_runs(monkeypatch, dev, [LS], call, digest, unwritten)


# ---- keep map ---------------------------------------------------------------------------------------------------------------
def test_keep_map(monkeypatch, dev):
    res, s = 128, 64
    corr, _, _ = _cell_rows(500, res, 7)
    corr = corr.clamp(0, res - 1).to(dev)
    _, _, masks = R.two_spheres(res)
    release = torch.zeros(1, 1, res, res)
    release[0, 0, 100:120, 10:40] = 1.0
    ms = [m.to(dev) for m in masks]
    call = lambda: BL.keep_map(corr, ms, release.to(dev), res, s, dilate=2, feather=3)
    guarded_runs(monkeypatch, dev, [BL], call, lambda keep: dict(keep=keep), arenas=0)


# ---- energy -----------------------------------------------------------------------------------------------------------------
GRID = 16
G2 = GRID * GRID


def _cells_dict(n_pairs, seed, background=True, n_objects=0):
    """The dict process_correspondences returns, written down: n_pairs random (source, target) cells and three background
    lists (none with background=False); n_objects > 0 adds the object of every pair."""
    rng = np.random.default_rng(seed)
    src, tgt = rng.integers(0, G2, n_pairs), rng.integers(0, G2, n_pairs)
    pick = (lambda k: np.sort(rng.choice(G2, k, replace=False))) if background else (lambda k: np.zeros(0, dtype=np.int64))
    both, orig, trans = pick(G2 // 3), pick(G2 // 2), pick(G2 // 2 + 5)
    pc = {"original_x": src % GRID, "original_y": src // GRID, "transformed_x": tgt % GRID, "transformed_y": tgt // GRID,
          "background_x": both % GRID, "background_y": both // GRID, "background_x_orig": orig % GRID,
          "background_y_orig": orig // GRID, "background_x_trans": trans % GRID, "background_y_trans": trans // GRID}
    if n_objects:
        pc["object"] = np.sort(rng.integers(0, n_objects, n_pairs)) if n_pairs > 1 else np.zeros(n_pairs, dtype=np.int64)
    return pc


def _maps(h, C, dtype, seed, dev, k=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(h, h, C, generator=g).to(dtype).to(dev) for _ in range(k)]


@pytest.mark.parametrize("n_pairs", [0, 1, G2 - 1, 3 * G2])
@pytest.mark.parametrize("h", [16, 32])
@pytest.mark.parametrize("C", [8, 320])
def test_general_energy(monkeypatch, dev, C, h, n_pairs):
    """inputs at the cell grid and at 32 x 32 (the resampling load), patch 1 and 3, both background types"""
    pc = _cells_dict(n_pairs, 11 + n_pairs)
    cur, org = _maps(h, C, torch.float16, 5, dev, 2)
    for patch in (1, 3):
        for bg_type in ("global_avg", "local_avg"):
            call = lambda: LS.energy_and_grad(cur, org, pc, 3.0, 2.0, patch, patch, (GRID, GRID), bg_type, grad_scale=64.0)
            guarded_runs(monkeypatch, dev, [LS], call, lambda r: dict(loss=r[0], grad=r[1]), prepare=LS._WS.clear)


PLANNED_VARIANTS = ("plain", "weighted", "donor", "batch_plain", "batch_objects", "batch_mixed", "batch_donor")
WEIGHTS = [1.0, 2.0, 0.5]


def _planned_call(variant, C, n_pairs, dev, want_loss, grad_dtype):
    """-> call(): builds the plans (their buffers are the caller's allocations too) and evaluates"""
    k = 3 if variant.startswith("batch") else 1
    acts, origs, donors = (_maps(GRID, C, torch.bfloat16, s, dev, k) for s in (1, 2, 3))
    weighted = {"plain": [0], "weighted": [1], "donor": [1], "batch_plain": [0, 0, 0], "batch_objects": [1, 1, 1],
                "batch_mixed": [0, 1, 0], "batch_donor": [1, 1, 1]}[variant]
    # the items of a batch differ in their pairs: item 0 has the case's count, the others fewer and more
    ns = [n_pairs, max(n_pairs // 2, 0), n_pairs + 3][:k]
    pcs = [_cells_dict(n, 40 + e, n_objects=3 if w else 0) for e, (n, w) in enumerate(zip(ns, weighted))]

    def call():
        plans = [LS.EnergyPlan(pc, GRID, dev, object_weights=WEIGHTS if w else None) for pc, w in zip(pcs, weighted)]
        fw, bw, sc = [3.0, 1.5, 2.0][:k], [2.0, 1.0, 0.5][:k], [64.0, 32.0, 1.0][:k]
        kw = dict(want_loss=want_loss, grad_dtype=grad_dtype)
        if variant in ("plain", "weighted"):
            loss, grad = LS.energy_and_grad_planned(acts[0], origs[0], plans[0], fw[0], bw[0], sc[0], **kw)
            return loss, [grad]
        if variant == "donor":
            loss, grad = LS.energy_and_grad_planned_donor(acts[0], origs[0], plans[0], fw[0], bw[0], donors[0], 0b010, sc[0], **kw)
            return loss, [grad]
        if variant == "batch_mixed":
            return LS.energy_and_grad_planned_mixed(acts, origs, plans, fw, bw, sc, **kw)
        if variant == "batch_donor":
            return LS.energy_and_grad_planned_donor_batch(acts, origs, plans, fw, bw, sc, [None, donors[1], donors[2]], [0, 0b010, 0b101], **kw)
        return LS.energy_and_grad_planned_batch(acts, origs, plans, fw, bw, sc, **kw)

    return call


def _energy_digest(r):
    loss, grads = r
    d = {f"grad{e}": g for e, g in enumerate(grads)}
    if loss is not None:
        d["loss"] = loss
    return d


@pytest.mark.parametrize("variant", PLANNED_VARIANTS)
@pytest.mark.parametrize("n_pairs", [0, 1, 5 * G2])
@pytest.mark.parametrize("C", [8, 320, 2048])
def test_planned_energy(monkeypatch, dev, C, n_pairs, variant):
    """C = 2048: one cell per workgroup of the gradient launch, as many loss partials as the array has doubles"""
    for want_loss in (True, False):
        for grad_dtype in (None, torch.float32):
            call = _planned_call(variant, C, n_pairs, dev, want_loss, grad_dtype)
            # the plan buffers (one arena each, carved by the build and again by every evaluation) and the workspace
            guarded_runs(monkeypatch, dev, [LS], call, _energy_digest, arenas=3 if variant.startswith("batch") else 2)


# ---- stale workspaces -------------------------------------------------------------------------------------------------------
def _fresh(monkeypatch, dev, call):
    """call() with every allocation of losses.py pre-filled, once with 0x00 and once with 0xFF -> the two digests"""
    out = []
    for fill in ("zeros", "ones"):
        frame = G.Frame(fill, dev)
        with monkeypatch.context() as m:
            m.setattr(LS, "torch", G.TorchProxy(frame))
            out.append({k: _bytes(v) for k, v in _energy_digest(call()).items()})
        frame.check()
    return out


def _same(got, refs, what):
    got = {k: _bytes(v) for k, v in _energy_digest(got).items()}
    for ref in refs:
        for k in ref:
            assert torch.equal(got[k], ref[k]), f"{what}: {k} depends on what the workspace held"


@pytest.mark.parametrize("weighted", [False, True])
def test_stale_plan_workspace(monkeypatch, dev, weighted):
    """The workspace an EnergyPlan caches, after an evaluation with many pairs and a background, under an evaluation without
    pairs and without a background: B's bits are B's bits on a fresh plan."""
    C, w = 320, (WEIGHTS if weighted else None)
    pc_a = _cells_dict(5 * G2, 71, n_objects=3 if weighted else 0)
    pc_b = _cells_dict(0, 72, background=False, n_objects=3 if weighted else 0)
    (cur_a, org_a), (cur_b, org_b) = _maps(GRID, C, torch.float16, 8, dev, 2), _maps(GRID, C, torch.float16, 9, dev, 2)
    eval_b = lambda plan: (lambda r: (r[0], [r[1]]))(LS.energy_and_grad_planned(cur_b, org_b, plan, 3.0, 2.0, 64.0, want_loss=True))
    refs = _fresh(monkeypatch, dev, lambda: eval_b(LS.EnergyPlan(pc_b, GRID, dev, object_weights=w)))
    plan_a = LS.EnergyPlan(pc_a, GRID, dev, object_weights=w)
    LS.energy_and_grad_planned(cur_a, org_a, plan_a, 3.0, 2.0, 64.0, want_loss=True)
    plan_b = LS.EnergyPlan(pc_b, GRID, dev, object_weights=w)
    plan_b._ws = plan_a._ws                                             # B runs on the workspace A left behind
    assert C in plan_b._ws
    _same(eval_b(plan_b), refs, "EnergyPlan workspace")


def test_stale_batch_workspace(monkeypatch, dev):
    """the same for the workspace _batch_state keeps for a batch of K = 3 plans"""
    C, K = 320, 3
    pcs_a = [_cells_dict(5 * G2, 80 + e) for e in range(K)]
    pcs_b = [_cells_dict(0, 90 + e, background=False) for e in range(K)]
    acts_a, origs_a = _maps(GRID, C, torch.float16, 8, dev, K), _maps(GRID, C, torch.float16, 9, dev, K)
    acts_b, origs_b = _maps(GRID, C, torch.float16, 10, dev, K), _maps(GRID, C, torch.float16, 11, dev, K)
    w = [3.0, 1.5, 2.0], [2.0, 1.0, 0.5], [64.0, 32.0, 1.0]
    eval_b = lambda plans: LS.energy_and_grad_planned_batch(acts_b, origs_b, plans, *w, want_loss=True)
    refs = _fresh(monkeypatch, dev, lambda: eval_b([LS.EnergyPlan(pc, GRID, dev) for pc in pcs_b]))
    plans_a = [LS.EnergyPlan(pc, GRID, dev) for pc in pcs_a]
    LS.energy_and_grad_planned_batch(acts_a, origs_a, plans_a, *w, want_loss=True)
    ws_a = LS._batch_state(plans_a, C)[1]
    plans_b = [LS.EnergyPlan(pc, GRID, dev) for pc in pcs_b]
    items, ws_b, nbytes = LS._batch_state(plans_b, C)                   # B's cache entry, with A's workspace in it
    assert ws_a.numel() == ws_b.numel() == nbytes
    cache = plans_b[0]._batch
    key, = cache.keys()
    cache[key] = (cache[key][0], ws_a) + cache[key][2:]
    assert LS._batch_state(plans_b, C)[1] is ws_a
    _same(eval_b(plans_b), refs, "batch workspace")
