"""GPU: copies of an object (dh_reproject_instance_edits, depth_transform.reproject_instance_edits,
losses.process_correspondences(pair_instances=...), DiffusionHandles.transform_foreground_objects / transform_foregrounds with
instances) against the test-side reference tests/object_copies_ref.py on the two-sphere scene at 128 and 256 pixels: the
smallest sizes at which the CLOSE element (res // 50 >= 2), the bit-row morphology and both footprint tiers are exercised.
tests/test_object_copies_ref.py asserts on the reference alone that every edit used here has at least 100 kept pairs per
instance and no equal-depth pixel between instances (set C excepted: it IS the tie rule).  The C entry writes into outputs
that are NaN / 0xFF / -1 before the call."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_object_ref as R  # noqa: E402
import footprints_ref as F  # noqa: E402
import object_copies_ref as O  # noqa: E402
import object_weights_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu
OUTPUTS = ("zmap", "raw", "clean", "vis", "txy", "corr", "counts", "disp")
INT_MAX = 2 ** 31 - 1
DH_ERR_ARG = -1          # include/diffhandles_hip.h
RATIO = 1.02          # drops the steepest triangles at the spheres' rims (test_object_copies_ref.py: it changes the rows)


def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _t(tf):
    return (float(tf[0]), torch.tensor(tf[1], dtype=torch.float32), torch.tensor(tf[2], dtype=torch.float32)) + tuple(tf[3:])


def _rows(edits):
    from diffusionhandles_amd import depth_transform as DT
    rows = DT._xform_rows([_t(tf) for tfs in edits for tf in tfs], similarity=True)
    assert rows.shape == (sum(len(tfs) for tfs in edits), 16) and rows.dtype == np.float64
    return rows


def _setup(depth, bg, masks):
    """Device inputs of the C entries: the pixel lists of the masks, concatenated."""
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    L, st = _lib.lib(), _lib.stream_ptr()
    res, M = depth.shape[-1], len(masks)
    d = depth.to(dev(), torch.float32).contiguous()
    b = bg.to(dev(), torch.float32).contiguous()
    gx, gy = DT._grids(res, res, dev())
    intr = D.intrinsics_f32()
    ifx, ify = DT._inv_focal(intr)
    fg_pix = torch.full((res * res,), -1, dtype=torch.int32, device=dev())
    n_dev = torch.full((M,), -1, dtype=torch.int32, device=dev())
    ws_small = torch.empty(4096, dtype=torch.uint8, device=dev())
    start = [0]
    for m, mask in enumerate(masks):
        m8 = (mask.to(dev()) != 0).to(torch.uint8).contiguous().view(-1)
        _lib.check(L.dh_fg_pixel_list(_lib.ptr(m8), res, _lib.ptr(fg_pix[start[-1]:]), _lib.ptr(n_dev[m:]), _lib.ptr(ws_small),
                                      ws_small.numel(), st), "dh_fg_pixel_list")
        start.append(start[-1] + int(m8.sum().item()))
    assert n_dev.tolist() == [start[m + 1] - start[m] for m in range(M)] and min(n_dev.tolist()) > 0
    return SimpleNamespace(L=L, st=st, res=res, M=M, d=d, b=b, gx=gx, gy=gy, ifx=ifx, ify=ify, fx=float(intr[0, 0]),
                           fy=float(intr[1, 1]), fg_pix=fg_pix, n_fg=start[-1], obj_start=np.asarray(start, dtype=np.int32))


def _call(s, rows, inst=None, footprints=0, ratio=0.0, cap=None, n_inst=None, ws_cut=0):
    """dh_reproject_instance_edits on poisoned outputs -- or, inst=None, dh_reproject_footprint_edits (the call without an
    instance table).  n_inst: the count passed (default len(inst)); a call that returned 0 is checked for having written
    everything the contract promises."""
    from diffusionhandles_amd import _lib
    L, res, M = s.L, s.res, s.M
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    table = list(range(M)) if inst is None else list(inst)
    N = len(table)
    assert rows.ndim == 2 and rows.shape[1] == 16 and rows.shape[0] % N == 0
    K = rows.shape[0] // N
    sizes = np.diff(s.obj_start)
    n_pts = int(sum(int(sizes[o]) for o in table if 0 <= o < M))
    need = res * res if footprints == 1 else n_pts
    cap = need if cap is None else cap
    nb = ctypes.c_size_t()
    if inst is None:
        _lib.check(L.dh_reproject_footprints_workspace_bytes(res, s.n_fg, K, M, 1 if footprints == 1 else 0, ctypes.byref(nb)))
    else:
        _lib.check(L.dh_reproject_instances_workspace_bytes(res, n_pts, K, M, max(1, min(N, 8)), 1 if footprints == 1 else 0,
                                                            ctypes.byref(nb)))
    ws = torch.full((nb.value,), 0xFF, dtype=torch.uint8, device=dev())
    nan = float("nan")
    o = SimpleNamespace(
        zmap=torch.full((K, res, res), nan, device=dev()), disp=torch.full((K, res, res), nan, device=dev()),
        raw=torch.full((K, res, res), 0xFF, dtype=torch.uint8, device=dev()),
        clean=torch.full((K, res, res), 0xFF, dtype=torch.uint8, device=dev()),
        vis=torch.full((K, max(n_pts, 1)), 0xFF, dtype=torch.uint8, device=dev()),
        txy=torch.full((K, max(n_pts, 1), 2), -1, dtype=torch.int32, device=dev()),
        corr=torch.full((K, max(cap, 1), 4), -1, dtype=torch.int64, device=dev()),
        inst=torch.full((K, max(cap, 1)), 0xFF, dtype=torch.uint8, device=dev()),
        counts=torch.full((K, 4), -1, dtype=torch.int32, device=dev()), n_pts=n_pts)
    args = (_lib.ptr(s.d), _lib.ptr(s.b), _lib.ptr(s.fg_pix), s.n_fg, M, s.obj_start.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            res, _lib.ptr(s.gx), _lib.ptr(s.gy), s.ifx, s.ify, s.fx, s.fy, K, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            None, _lib.ptr(o.zmap), _lib.ptr(o.raw), _lib.ptr(o.clean), _lib.ptr(o.disp), _lib.ptr(o.vis), _lib.ptr(o.txy),
            _lib.ptr(o.corr), _lib.ptr(o.counts), _lib.ptr(ws), nb.value - ws_cut, s.st, footprints, ratio, cap)
    if inst is None:
        o.rc = L.dh_reproject_footprint_edits(*args)
    else:
        tab = np.asarray(table, dtype=np.int32)
        o.rc = L.dh_reproject_instance_edits(*args, N if n_inst is None else n_inst, tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                             _lib.ptr(o.inst))
    o.err = L.dh_last_error().decode() if o.rc != 0 else ""
    torch.cuda.synchronize()
    o.counts_h = o.counts.cpu()
    if o.rc == 0:
        assert torch.isfinite(o.disp).all() and not torch.isnan(o.zmap).any()
        assert int(o.raw.max()) <= 1 and int(o.clean.max()) <= 1 and int(o.vis.max()) <= 1
        assert int(o.txy.min()) >= 0 and int(o.txy.max()) < res
        assert (o.counts_h[:, 3] >= 0).all()
        for e in range(K):
            n = int(o.counts_h[e, 0])
            assert 0 < n <= cap and 0 < int(o.counts_h[e, 1]) <= n_pts
            assert int(o.corr[e, :n].min()) >= 0 and int(o.corr[e, :n].max()) < res and bool((o.corr[e, n:] == -1).all())
            if inst is not None:
                assert int(o.inst[e, :n].max()) < N and bool((o.inst[e, n:] == 0xFF).all())
    return o


def _same_bytes(a, b, what):
    for k in OUTPUTS:
        x, y = getattr(a, k).contiguous().view(torch.uint8), getattr(b, k).contiguous().view(torch.uint8)
        assert torch.equal(x, y), f"{what}: {k}"


def _untouched(o):
    assert torch.isnan(o.zmap).all() and torch.isnan(o.disp).all()
    assert bool((o.raw == 0xFF).all()) and bool((o.clean == 0xFF).all()) and bool((o.vis == 0xFF).all())
    assert bool((o.txy == -1).all()) and bool((o.corr == -1).all()) and bool((o.counts == -1).all()) and bool((o.inst == 0xFF).all())


def _check_against_ref(o, e, ref, what):
    """Every integer output bit-exact, no pixel left out; the disparity within the 2e-3 (of 255) of the point-mode tests."""
    disp_r, corr_r, dbg_r = ref
    n = int(o.counts_h[e, 0])
    assert n == len(corr_r), f"{what}: {n} correspondences, the reference has {len(corr_r)}"
    assert np.array_equal(o.corr[e, :n].cpu().numpy(), corr_r.numpy()), f"{what}: correspondences (order included)"
    assert np.array_equal(o.inst[e, :n].cpu().numpy(), dbg_r["corr_inst"]), f"{what}: corr_inst"
    assert np.array_equal(o.zmap[e].cpu().numpy(), dbg_r["zmap"]), f"{what}: zmap"
    assert np.array_equal(o.raw[e].cpu().numpy() != 0, dbg_r["raw_mask"]), f"{what}: raw mask"
    assert np.array_equal(o.clean[e].cpu().numpy() != 0, dbg_r["cleaned"] != 0), f"{what}: clean mask"
    assert np.array_equal(o.vis[e].cpu().numpy() != 0, dbg_r["vis"]), f"{what}: vis"
    txy = o.txy[e].cpu().numpy()
    assert np.array_equal(txy[:, 0], dbg_r["tx"]) and np.array_equal(txy[:, 1], dbg_r["ty"]), f"{what}: target_xy"
    assert int(o.counts_h[e, 1]) == int(dbg_r["vis"].sum()), f"{what}: visible count"
    assert int(o.counts_h[e, 2]) == int(dbg_r["inpaint"].sum()), f"{what}: in-fill count"
    err = float((o.disp[e].cpu() - disp_r[0, 0]).abs().max())
    print(f"{what}: {n} correspondences {np.bincount(dbg_r['corr_inst']).tolist()}, {int(o.counts_h[e, 2])} in-fill pixels, "
          f"disparity max abs err {err:.2e}")
    assert err < 2e-3, f"{what}: disparity {err}"


_REFS = {}


def _refs(key, make):
    """A reference is computed once per session and never changed."""
    if key not in _REFS:
        from oracle import depth_ref as D
        D.DOT_ORDER = "explicit"
        try:
            _REFS[key] = make()
        finally:
            D.DOT_ORDER = "blas"
    return _REFS[key]


# ---- 1. the identity table is the call without copies ------------------------------------------------------------------------
@pytest.mark.parametrize("footprints", [0, 1])
def test_identity_table_is_the_footprint_entry(footprints):
    """two_spheres(128), the five edits of the footprint tests: dh_reproject_instance_edits with inst_obj = (0, 1) against
    dh_reproject_footprint_edits, every byte of every output (the poison beyond the valid rows included); corr_inst is the
    object of the row's source pixel.  The queries that existed before return what the identity carving needs."""
    depth, bg, masks = R.two_spheres(128)
    s = _setup(depth, bg, masks)
    rows = _rows(F.EDITS)
    old = _call(s, rows, footprints=footprints)
    new = _call(s, rows, inst=[0, 1], footprints=footprints)
    assert old.rc == 0 and new.rc == 0, old.err + new.err
    assert min(int(old.counts_h[e, 0]) for e in range(5)) > 500
    _same_bytes(new, old, f"identity table, footprints = {footprints}")
    label = W.label_image([m.numpy() for m in masks])
    for e in range(5):
        n = int(new.counts_h[e, 0])
        c = new.corr[e, :n].cpu().numpy()
        assert np.array_equal(new.inst[e, :n].cpu().numpy(), label[c[:, 1], c[:, 0]] - 1), f"edit {e}: corr_inst"
        assert len(np.unique(new.inst[e, :n].cpu().numpy())) == 2


# ---- 2. sets A, B, C against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [128, 256])
@pytest.mark.parametrize("name", ["A", "B"])
def test_copies_against_the_reference(name, res):
    """Set A (instances (0, 0, 1), K = 2: the edit-major rows e * N + n) and set B (instances (0, 0, 1, 1), K = 1)."""
    inst, edits = O.SET_A if name == "A" else O.SET_B
    depth, bg, masks = R.two_spheres(res)
    s = _setup(depth, bg, masks)
    o = _call(s, _rows(edits), inst=inst)
    assert o.rc == 0, o.err
    assert o.n_pts > s.n_fg
    refs = _refs((name, res), lambda: [O.transform_instances(depth, bg, masks, inst, tfs) for tfs in edits])
    for e, ref in enumerate(refs):
        _check_against_ref(o, e, ref, f"set {name}, res {res}, edit {e}")
    # the Python call gives the same bits, on the host and on the device, and the instances beside the rows
    from diffusionhandles_amd import depth_transform as DT
    from oracle import depth_ref as D
    args = (depth.to(dev()), bg.to(dev()), [m.to(dev()) for m in masks], D.intrinsics_f32(), [[_t(tf) for tf in tfs] for tfs in edits])
    out, dbg = DT.reproject_instance_edits(*args, return_debug=True, instances=inst)
    out_d = DT.reproject_instance_edits(*args, device_correspondences=True, instances=inst, return_instances=True)
    assert dbg["corr_dev"].shape == (len(edits), o.n_pts, 4) and dbg["corr_inst"].shape == (len(edits), o.n_pts)
    assert dbg["inst_start"].tolist() == refs[0][2]["inst_start"].tolist()
    for e in range(len(edits)):
        n = int(o.counts_h[e, 0])
        assert len(out[e]) == 2 and torch.equal(out[e][1], o.corr[e, :n].cpu()) and torch.equal(out[e][0][0, 0], o.disp[e])
        assert len(out_d[e]) == 3 and out_d[e][1].is_cuda and torch.equal(out_d[e][1], o.corr[e, :n])
        assert out_d[e][2].dtype == torch.uint8 and torch.equal(out_d[e][2], o.inst[e, :n])
        assert torch.equal(dbg["corr_inst"][e, :n], o.inst[e, :n])
    assert torch.equal(dbg["zmap"], o.zmap) and torch.equal(dbg["vis"], o.vis) and torch.equal(dbg["clean_mask"], o.clean)


@pytest.mark.parametrize("res", [128, 256])
def test_two_instances_with_one_transform_are_the_one_instance_call(res):
    """Set C: mask 0 twice under one transform.  Equal depths go to the earlier instance: every geometry output is the
    one-instance call's, the later instance's points are all hidden, corr_inst is all 0."""
    inst, edits = O.SET_C
    depth, bg, masks = R.two_spheres(res)
    s = _setup(depth, bg, masks[:1])
    two = _call(s, _rows(edits), inst=inst)
    one = _call(s, _rows([edits[0][:1]]), inst=[0])
    assert two.rc == 0 and one.rc == 0, two.err + one.err
    n = int(one.counts_h[0, 0])
    for k in ("zmap", "raw", "clean", "disp", "counts"):
        assert torch.equal(getattr(two, k), getattr(one, k)), k
    assert torch.equal(two.corr[0, :n], one.corr[0, :n]) and bool((two.corr[0, n:] == -1).all())
    assert torch.equal(two.vis[0, :s.n_fg], one.vis[0]) and not bool(two.vis[0, s.n_fg:].any())
    assert torch.equal(two.txy[0, :s.n_fg], one.txy[0]) and torch.equal(two.txy[0, s.n_fg:], one.txy[0])
    assert bool((two.inst[0, :n] == 0).all())
    ref = _refs(("C", res), lambda: O.transform_instances(depth, bg, masks[:1], inst, edits[0]))
    _check_against_ref(two, 0, ref, f"set C, res {res}")
    assert n == {128: 1095, 256: 4546}[res]


# ---- 3. footprints ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [None, RATIO])
def test_footprints_join_the_points_of_one_instance(ratio):
    """Set A's first edit with instance 1 at uniform scale 2, footprints on, at 128, without and with the depth-ratio guard:
    what tests/test_footprints_gpu.py compares, bit-exact, at the tiers 1 (wave tier), default and INT_MAX (thread tier)."""
    inst, edits = O.SET_A_FP
    depth, bg, masks = R.two_spheres(128)
    s = _setup(depth, bg, masks)
    ref = _refs(("A_FP", ratio), lambda: O.transform_instances(depth, bg, masks, inst, edits[0], footprints=True, max_ratio=ratio))
    outs = {}
    try:
        for tier in (1, 0, INT_MAX):
            assert s.L.dh_dbg_footprint_tier(tier) == 0
            outs[tier] = _call(s, _rows(edits), inst=inst, footprints=1, ratio=0.0 if ratio is None else ratio)
            assert outs[tier].rc == 0, outs[tier].err
    finally:
        assert s.L.dh_dbg_footprint_tier(0) == 0
    _check_against_ref(outs[1], 0, ref, f"footprints, ratio {ratio}, wave tier")
    _same_bytes(outs[0], outs[1], "default tier against the wave tier")
    _same_bytes(outs[INT_MAX], outs[1], "thread tier against the wave tier")
    assert torch.equal(outs[0].inst, outs[1].inst) and torch.equal(outs[INT_MAX].inst, outs[1].inst)
    # the enlarged copy: more rows of instance 1 than its mask has points
    n = int(outs[0].counts_h[0, 0])
    assert int((outs[0].inst[0, :n] == 1).sum()) > int(s.obj_start[1])


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst,n_inst,word", [
    ([0, 0, 1], 0, "instances"), ([0, 0, 1, 0, 1, 0, 1, 0, 1], None, "instances"), ([0, 2, 1], None, "outside"),
    ([0, -1, 1], None, "outside"), ([0, 0, 0], None, "without an instance"), ([1, 1], None, "without an instance")])
def test_library_refuses_bad_instance_tables_before_any_launch(inst, n_inst, word):
    depth, bg, masks = R.two_spheres(128)
    s = _setup(depth, bg, masks)
    tfs = [(0.0, R.Y, (0.0, 0.0, 0.0))] * len(inst)
    o = _call(s, _rows([tfs, tfs]), inst=inst, n_inst=n_inst)
    assert o.rc == DH_ERR_ARG and word in o.err, o.err
    _untouched(o)


@pytest.mark.parametrize("what,word", [("scale", "scale"), ("cap", "capacity"), ("ws", "workspace")])
def test_library_checks_every_row_and_the_sizes_of_an_instance_call(what, word):
    """The row checks reach row K * N - 1 (a zero scale on the last instance of the last edit); the capacity is n_pts, not n_fg."""
    inst, edits = O.SET_A
    depth, bg, masks = R.two_spheres(128)
    s = _setup(depth, bg, masks)
    rows = _rows(edits)
    kw = {}
    if what == "scale":
        rows[-1, 8] = 0.0
    elif what == "cap":
        kw["cap"] = s.n_fg
    else:
        kw["ws_cut"] = 4096
    o = _call(s, rows, inst=inst, **kw)
    assert o.rc == DH_ERR_ARG and word in o.err, o.err
    _untouched(o)


def test_library_refuses_a_point_list_beyond_the_int_owner_map():
    """res * res + n_pts must fit an int: a table whose slices sum past 2^31 is refused on its sizes alone (obj_start is a host
    array; nothing is read on the device before the refusal)."""
    depth, bg, masks = R.two_spheres(128)
    s = _setup(depth, bg, masks)
    big = SimpleNamespace(**vars(s))
    big.n_fg = 2 ** 30
    big.obj_start = np.asarray([0, 2 ** 30], dtype=np.int32)
    big.M = 1
    from diffusionhandles_amd import _lib
    rows = _rows([[(0.0, R.Y, (0.0, 0.0, 0.0))] * 2])
    nan = float("nan")
    zmap = torch.full((1, 128, 128), nan, device=dev())
    small = torch.full((16,), -1, dtype=torch.int64, device=dev())
    tab = np.asarray([0, 0], dtype=np.int32)
    rc = s.L.dh_reproject_instance_edits(
        _lib.ptr(s.d), _lib.ptr(s.b), _lib.ptr(s.fg_pix), big.n_fg, 1, big.obj_start.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
        128, _lib.ptr(s.gx), _lib.ptr(s.gy), s.ifx, s.ify, s.fx, s.fy, 1, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None,
        _lib.ptr(zmap), _lib.ptr(small), _lib.ptr(small), _lib.ptr(zmap), _lib.ptr(small), _lib.ptr(small), _lib.ptr(small),
        _lib.ptr(small), _lib.ptr(small), 128, s.st, 0, 0.0, INT_MAX, 2, tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None)
    err = s.L.dh_last_error().decode()
    torch.cuda.synchronize()
    assert rc == DH_ERR_ARG and "owner map" in err, err
    assert torch.isnan(zmap).all() and bool((small == -1).all())


# ---- 5. the energy per instance -----------------------------------------------------------------------------------------------
GRID = 32          # 256 pixels / 8
C_ENERGY = 64
SCALE = 64.0


@pytest.fixture(scope="module")
def energy():
    """Set A's first edit at 256 pixels: its correspondences and instances from the library, the cells and the per-pair objects
    of the reference (oracle.guidance_ref.cells_from_correspondences; corr_inst filtered as the rows are), f16 maps."""
    from diffusionhandles_amd import depth_transform as DT
    from diffusionhandles_amd.losses import process_correspondences
    from oracle import depth_ref as D
    from oracle import guidance_ref as G
    inst, edits = O.SET_A
    res = 256
    depth, bg, masks = R.two_spheres(res)
    ref = _refs(("A", res), lambda: [O.transform_instances(depth, bg, masks, inst, tfs) for tfs in edits])[0]
    (_, corr, rows), = DT.reproject_instance_edits(depth.to(dev()), bg.to(dev()), [m.to(dev()) for m in masks], D.intrinsics_f32(),
                                                 [[_t(tf) for tf in edits[0]]], instances=inst, return_instances=True)
    assert torch.equal(corr, ref[1]) and np.array_equal(rows.numpy(), ref[2]["corr_inst"])
    c = ref[1].numpy()
    ok = (c[:, 2] >= 0) & (c[:, 2] < res) & (c[:, 3] >= 0) & (c[:, 3] < res)
    cells = G.cells_from_correspondences(c, res, 0, grid=GRID)
    objects = ref[2]["corr_inst"][ok].astype(np.int64)
    assert objects.size == cells["original_x"].size
    # repeated source cells: a source cell of mask 0 feeds pairs of instance 0 AND of instance 1
    src = cells["original_y"] * GRID + cells["original_x"]
    assert len(set(src[objects == 0].tolist()) & set(src[objects == 1].tolist())) > 10
    pc = process_correspondences(corr, res, 0, grid=GRID, device=dev(), pair_instances=rows)
    assert np.array_equal(pc["object"], objects) and np.array_equal(pc["transformed_x"], cells["transformed_x"])
    assert torch.equal(pc.device_lists["pair_obj"].cpu(), torch.from_numpy(objects).to(torch.uint8))
    plain_pc = process_correspondences(corr, res, 0, grid=GRID, device=dev())
    g = torch.Generator().manual_seed(64)
    act = torch.randn(GRID, GRID, C_ENERGY, generator=g).to(torch.float16).to(dev())
    orig = torch.randn(GRID, GRID, C_ENERGY, generator=g).to(torch.float16).to(dev())
    with pytest.raises(ValueError, match="mutually exclusive"):
        process_correspondences(corr, res, 0, grid=GRID, device=dev(), pair_instances=rows,
                                object_labels=torch.zeros(res, res, dtype=torch.uint8))
    with pytest.raises(ValueError, match="pair_instances has"):
        process_correspondences(corr, res, 0, grid=GRID, device=dev(), pair_instances=rows[:-1])
    return SimpleNamespace(pc=pc, plain_pc=plain_pc, cells=cells, objects=objects, act=act, orig=orig)


def _planned(energy, plan, fw, bw):
    """One planned call, f16 activations, f32 gradient (the 1e-4 * max gate is below one f16 rounding of the gradient, 2^-11)."""
    from diffusionhandles_amd.losses import energy_and_grad_planned
    out = torch.full((GRID, GRID, C_ENERGY), float("nan"), dtype=torch.float32, device=dev())
    loss, grad = energy_and_grad_planned(energy.act, energy.orig, plan, fw, bw, grad_scale=SCALE, want_loss=True, out=out,
                                         grad_dtype=torch.float32)
    torch.cuda.synchronize()
    assert torch.isfinite(grad).all() and torch.isfinite(loss).all()
    return loss, grad


def _check_energy(loss, grad, ref_loss, ref_grad, what):
    """loss within 2e-5 relative, gradient within 1e-4 of its largest entry."""
    got = [float(v) for v in loss.cpu()]
    ref = ref_grad.double().cpu() * SCALE
    err, top = float((grad.double().cpu() - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: loss {got} / reference {list(ref_loss)}; gradient max abs err {err:.3e}, max |ref| {top:.3e}")
    for g, r in zip(got, ref_loss):
        assert abs(g - r) <= 2e-5 * abs(r), (what, got, ref_loss)
    assert top > 0 and err <= 1e-4 * top, what


@pytest.mark.parametrize("fw,bw", [(7.5, 1.5), (7.5, 0.0)])
def test_unweighted_energy_on_repeated_source_cells(energy, fw, bw):
    """The planned, unweighted energy on set A's correspondences against oracle.guidance_ref (float64 autograd): the mean over
    all pairs, a source cell entering once per pair."""
    from diffusionhandles_amd.losses import EnergyPlan
    from oracle import guidance_ref as G
    plan = EnergyPlan(energy.plain_pc, GRID, dev())
    assert not plan.weighted and plan.n_pairs == energy.objects.size
    a = energy.act.double().cpu().permute(2, 0, 1).contiguous().requires_grad_(True)
    o = energy.orig.double().cpu().permute(2, 0, 1).contiguous()
    fg = G.foreground_energy(a, o, energy.cells, 1, (GRID, GRID))
    bg = G.background_energy(a, o, energy.cells, 1, (GRID, GRID))
    tot = fw * fg + bw * bg
    gr, = torch.autograd.grad(tot, a)
    loss, grad = _planned(energy, plan, fw, bw)
    _check_energy(loss, grad, (float(tot.detach()), float(fg.detach()), float(bg.detach())), gr.permute(1, 2, 0), f"unweighted (fw, bw) = ({fw}, {bw})")
    # the instances beside the rows change nothing without weights
    same = EnergyPlan(energy.pc, GRID, dev())
    loss2, grad2 = _planned(energy, same, fw, bw)
    assert not same.weighted and torch.equal(grad2, grad) and torch.equal(loss2, loss)


@pytest.mark.parametrize("weights", ["equal", [0.25, 2.0, 1.0]])
def test_weighted_energy_per_instance(energy, weights):
    """'equal' and N explicit weights against tests/object_weights_ref.py with the instances as its objects."""
    from diffusionhandles_amd.losses import EnergyPlan
    plan = EnergyPlan(energy.pc, GRID, dev(), object_weights=weights)
    assert plan.weighted and plan.counts.tolist() == np.bincount(energy.objects).tolist() and len(plan.counts) == 3
    w = [1.0, 1.0, 1.0] if weights == "equal" else weights
    for fw, bw in ((7.5, 1.5), (7.5, 0.0)):
        ref_loss, ref_grad = W.energy_and_grad(energy.act, energy.orig, energy.cells, energy.objects, w, fw, bw)
        loss, grad = _planned(energy, plan, fw, bw)
        _check_energy(loss, grad, ref_loss, ref_grad, f"weights {weights}, (fw, bw) = ({fw}, {bw})")
    with pytest.raises(ValueError, match="object 2, there are 2 weights"):
        EnergyPlan(energy.pc, GRID, dev(), object_weights=[1.0, 1.0])          # one weight per INSTANCE: pairs of instance 2


def _ordered(t):
    i = t.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i + (1 << 31)), i)


def test_weights_one_zero_zero_are_the_unweighted_call_on_instance_0(energy):
    """Against the unweighted plan of instance 0's pairs with the union's background lists, under the gate of
    tests/test_object_weights_gpu.py for (1, 0): within one unit in the last place of the gradient type."""
    from diffusionhandles_amd.losses import EnergyPlan, ProcessedCorrespondences
    dl = dict(energy.pc.device_lists)
    dl["pairs"] = dl["pairs"][dl["pair_obj"] == 0].contiguous()
    del dl["pair_obj"]
    pc0 = ProcessedCorrespondences(energy.pc)
    pc0.device_lists = dl
    plan0 = EnergyPlan(pc0, GRID, dev())
    plan = EnergyPlan(energy.pc, GRID, dev(), object_weights=[1.0, 0.0, 0.0])
    assert not plan0.weighted and plan0.n_pairs == int((energy.objects == 0).sum()) and plan.weighted
    for fw, bw in ((7.5, 1.5), (7.5, 0.0), (0.0, 1.5)):
        _, g0 = _planned(energy, plan0, fw, bw)
        _, g1 = _planned(energy, plan, fw, bw)
        ulps = int((_ordered(g1) - _ordered(g0)).abs().max())
        print(f"(fw, bw) = ({fw}, {bw}): largest distance {ulps} ulp, max |g| {float(g0.abs().max()):.3e}")
        assert ulps <= 1
        assert fw == 0.0 or float(g0.abs().max()) > 0


# ---- 6. the loop level, on the TINY rig of tests/test_object_items_gpu.py ------------------------------------------------------
RES = 512
LOOP_INST = [0, 0, 1]


def _loop_tfs():
    return [_t(tf) for tf in O.SET_A[1][0]]


@pytest.fixture(scope="module")
def tiny():
    from diffusionhandles_amd import DiffusionHandles
    from diffusionhandles_amd import conf as C
    from diffusionhandles_amd.synthetic import make_scene
    from diffusionhandles_amd.unet import HipUNet
    from oracle import unet_torch as U
    ref = U.init_synthetic_(U.UNetTorch(U.TINY), seed=0).to(dev()).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.half().float())
    hip = HipUNet(dict(U.TINY, text_len=77), dtype=torch.float16, max_batch=4)
    hip.load_state_dict(ref.state_dict())
    dh = DiffusionHandles(C.load_default(), unet=hip, unet_config=dict(U.TINY, text_len=77)).to(dev())

    def identity(depth, prompt, seed):
        g = torch.Generator().manual_seed(seed)
        noise = torch.randn(1, 4, RES // 8, RES // 8, generator=g).to(dev())
        Dm = dh.diffuser.unet.cfg["cross_attention_dim"]
        unc = (dh.diffuser._encode([""])[None].expand(50, -1, -1, -1) + 0.05 * torch.randn(50, 1, 77, Dm, generator=g).to(dev())).contiguous()
        null_text, noise, acts, _ = dh.generate_input_image(depth, prompt, unc, noise)
        return dict(null_text=null_text, noise=noise, acts=acts, prompt=prompt)
    depth, bg, masks = R.two_spheres(RES)
    depth, bg, masks = depth.to(dev()), bg.to(dev()), [m.to(dev()) for m in masks]
    two = SimpleNamespace(depth=depth, bg_depth=dh.set_foreground(depth, masks, bg), masks=masks,
                          **identity(depth, "two spheres on a plane", 11))
    d1, b1, m1 = (t.to(dev()).flip(-1).contiguous() for t in make_scene(RES))
    one = SimpleNamespace(depth=d1, bg_depth=dh.set_foreground(d1, m1, b1), fg_mask=m1, **identity(d1, "a red ball on a wooden table", 12))
    return SimpleNamespace(dh=dh, gd=dh.diffuser, two=two, one=one)


def _common(im):
    return dict(depth=im.depth, prompt=im.prompt, bg_depth=im.bg_depth, null_text_emb=im.null_text, init_noise=im.noise,
                activations=im.acts)


def _reproject_copies(tiny, device_correspondences=False):
    from diffusionhandles_amd.depth_transform import reproject_instance_edits
    t = tiny.two
    (d, c, rows), = reproject_instance_edits(t.depth, t.bg_depth, t.masks, tiny.gd.get_depth_intrinsics(device=dev()), [_loop_tfs()],
                                           instances=LOOP_INST, return_instances=True, device_correspondences=device_correspondences)
    return d, c, rows


def test_transform_foreground_objects_with_instances_is_guided_inference_on_the_same_rows(tiny):
    """transform_foreground_objects(..., instances=[0, 0, 1]) with 'equal' weights = guided_inference fed the re-projection's
    correspondences and per-row instances, bit for bit; the weights reach the energy (three instances, all with pairs)."""
    dh, gd, t = tiny.dh, tiny.gd, tiny.two
    img, disp = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=_loop_tfs(), instances=LOOP_INST,
                                                object_weights="equal")
    img, lat = img.clone(), gd.last_latents.clone()
    assert img.shape == (1, 3, RES, RES) and torch.isfinite(img).all()
    d, c, rows = _reproject_copies(tiny)
    assert torch.equal(d, disp) and sorted(rows.unique().tolist()) == [0, 1, 2]
    ref = gd.guided_inference(t.noise, d, t.null_text, t.prompt, t.acts, c, pair_instances=rows, object_weights="equal")
    assert torch.equal(gd.last_latents, lat) and torch.equal(ref, img)
    plain, _ = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=_loop_tfs(), instances=LOOP_INST)
    assert torch.isfinite(plain).all() and not torch.equal(plain, img)
    # a label image cannot stand in for the instances, and both at once are refused
    from diffusionhandles_amd.losses import object_label_image
    with pytest.raises(ValueError, match="mutually exclusive"):
        gd.prepare_guidance(d, t.prompt, t.acts, c, pair_instances=rows, object_labels=object_label_image(t.masks),
                            object_weights="equal")


def test_copies_in_a_mixed_image_batch_equal_the_items_call(tiny):
    """The same edit inside a transform_foregrounds batch next to a one-object edit of another image: bit-identical to
    guided_inference_items on the re-projections (the gate of tests/test_object_items_gpu.py)."""
    from diffusionhandles_amd.depth_transform import reproject_edits
    from diffusionhandles_amd.synthetic import TRANSFORMS
    dh, gd, t, o = tiny.dh, tiny.gd, tiny.two, tiny.one
    Yt = torch.tensor(R.Y)
    single = (TRANSFORMS[5][0], Yt, torch.tensor(TRANSFORMS[5][1]))
    edits = [dict(_common(t), fg_masks=t.masks, transforms=_loop_tfs(), instances=LOOP_INST, object_weights=[1.0, 2.0, 0.5]),
             dict(_common(o), fg_mask=o.fg_mask, rot_angle=single[0], rot_axis=single[1], translation=single[2])]
    images, disps = dh.transform_foregrounds(edits)
    images, lat = images.clone(), gd.last_latents.clone()
    assert images.shape == (2, 3, RES, RES) and torch.isfinite(images).all()
    d, c, rows = _reproject_copies(tiny, device_correspondences=True)
    (d1, c1), = reproject_edits(o.depth, o.bg_depth, o.fg_mask, gd.get_depth_intrinsics(), [single], device_correspondences=True)
    assert torch.equal(d, disps[0]) and torch.equal(d1, disps[1])
    item = lambda im, dd, cc, **kw: dict(latents=im.noise, depth=dd, uncond_embeddings=im.null_text, prompt=im.prompt,
                                         activations_orig=im.acts, correspondences=cc, **kw)
    ref = gd.guided_inference_items([item(t, d, c, pair_instances=rows, object_weights=[1.0, 2.0, 0.5]), item(o, d1, c1)])
    assert torch.equal(gd.last_latents, lat) and torch.equal(ref, images)
    # malformed edits are refused before any device work, naming the edit and the instance
    bad = lambda **kw: [dict(edits[0], **kw), edits[1]]
    with pytest.raises(ValueError, match="edit 0.*instance 1"):
        dh.transform_foregrounds(bad(instances=[0, 2, 1]))
    with pytest.raises(ValueError, match="edit 0.*mask 1 has no instance"):
        dh.transform_foregrounds(bad(instances=[0, 0, 0]))
    with pytest.raises(ValueError, match="edit 0 has 3 transforms for 4 instances"):
        dh.transform_foregrounds(bad(instances=[0, 0, 1, 1]))
    with pytest.raises(ValueError, match="edit 0.*2 entries for 3"):
        dh.transform_foregrounds(bad(object_weights=[1.0, 1.0]))


def test_background_lock_sets_every_instance_free(tiny):
    """conf background_lock: the keep map is 0 on every cell that a source or a target pixel of any instance touches."""
    dh, gd, t = tiny.dh, tiny.gd, tiny.two
    dh.conf["background_lock"] = True
    try:
        img, _ = dh.transform_foreground_objects(**_common(t), fg_masks=t.masks, transforms=_loop_tfs(), instances=LOOP_INST)
        keep, = dh.last_keep_maps
    finally:
        dh.conf.pop("background_lock", None)
    assert torch.isfinite(img).all()
    _, c, rows = _reproject_copies(tiny)
    s = gd.unet.sample_size
    cell = RES // s
    keep = keep.float().cpu().reshape(s, s)
    c = c.numpy()
    for n in range(3):
        sel = rows.numpy() == n
        assert sel.sum() > 100
        for x, y in ((c[sel, 0], c[sel, 1]), (c[sel, 2], c[sel, 3])):
            assert float(keep[y // cell, x // cell].max()) == 0.0, f"instance {n}"
    assert float(keep.max()) == 1.0          # and the lock does hold somewhere


# ---- 7. the harness on a scene directory with copies ---------------------------------------------------------------------------
def _run_edit_module():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_edit_tool", os.path.join(root, "tools", "run_edit.py"))
    run_edit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run_edit)
    return run_edit


def test_run_edit_passes_the_instances_of_a_scene_directory(tiny, tmp_path):
    """A two-mask scene whose entry `copy` has a third member with "mask": 0: run_scene and the --edit-batch path hand the
    table to transform_foreground_objects / transform_foregrounds and write the same disparity, which is the re-projection's."""
    import argparse
    import json
    from diffusionhandles_amd.scene_io import read_png, write_png
    run_edit = _run_edit_module()
    inp = tmp_path / "set"
    scene = inp / "two_spheres"
    scene.mkdir(parents=True)
    depth, bg, masks = R.two_spheres(RES)
    np.save(scene / "depth.npy", depth[0, 0].numpy())
    np.save(scene / "bg_depth.npy", bg[0, 0].numpy())
    for m, mask in enumerate(masks):
        write_png(str(scene / f"mask_{m}.png"), mask[0, 0].numpy())
    write_png(str(scene / "input.png"), np.full((RES, RES, 3), 0.5, dtype=np.float32))
    (scene / "prompt.txt").write_text("two spheres on a plane\n")
    member = lambda tf, **kw: dict(rotation_angle=tf[0], rotation_axis=list(tf[1]), translation=list(tf[2]), **kw)
    a = O.SET_A[1][0]          # instances (0, 0, 1) there; here the copy is the LAST member: (0, 1, 0)
    (scene / "transforms.json").write_text(json.dumps({
        "plain": {"objects": [member(a[0]), member(a[2])]},
        "copy": {"objects": [member(a[0]), member(a[2]), member(a[1], mask=0)], "object_weights": "equal"}}))
    args = argparse.Namespace(res=RES, mode="pc", skip_inversion=True, no_identity_cache=True, identity_cache=None, skip_existing=False,
                              max_edits=0, identity_batch=1, edit_batch=1, edit_batch_images=0)
    seen = []
    dh = tiny.dh
    inner_one, inner_many = dh.transform_foreground_objects, dh.transform_foregrounds
    dh.transform_foreground_objects = lambda *a_, **kw: (seen.append(kw.get("instances")), inner_one(*a_, **kw))[1]
    dh.transform_foregrounds = lambda edits, **kw: (seen.extend(e.get("instances") for e in edits), inner_many(edits, **kw))[1]
    try:
        report = run_edit.run_scene(args, dh.conf, lambda res: dh, str(scene), str(tmp_path / "one"), None)
        assert [e["name"] for e in report["edits"]] == ["plain", "copy"] and seen == [None, [0, 1, 0]]
        del seen[:]
        args.edit_batch, args.out = 2, str(tmp_path / "batched")
        reports, _ = run_edit.run_test_set_batched(args, dh.conf, lambda res: dh, [("two_spheres", ["plain", "copy"])], str(inp))
        assert [e["name"] for e in reports[0]["edits"]] == ["plain", "copy"] and seen == [None, [0, 1, 0]]
    finally:
        del dh.transform_foreground_objects, dh.transform_foregrounds
    for name in ("plain", "copy"):
        one, many = read_png(str(tmp_path / "one" / f"{name}.png")), read_png(str(tmp_path / "batched" / "two_spheres" / f"{name}.png"))
        assert one.shape == (RES, RES, 3) and one.std() > 0 and many.std() > 0
        d_one = read_png(str(tmp_path / "one" / f"{name}_disparity.png"))
        assert np.array_equal(d_one, read_png(str(tmp_path / "batched" / "two_spheres" / f"{name}_disparity.png")))
    # the copy is in the picture: its disparity differs from the plain edit's where the lifted copy stands
    assert (read_png(str(tmp_path / "one" / "copy_disparity.png")) != read_png(str(tmp_path / "one" / "plain_disparity.png"))).any()
