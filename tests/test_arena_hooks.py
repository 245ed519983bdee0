"""The arena hooks of the workspace queries (dh_dbg_arena_gap, dh_dbg_arena_log; host only, no GPU): at gap 0 every
*_workspace_bytes / *_plan_bytes query answers what it answered before the hooks existed, a gap moves every sub-buffer by exactly
the gap, and the logged takes are the layout the entries carve (tests/test_workspace_guards_gpu.py relies on all three)."""
import ctypes

import pytest

from diffusionhandles_amd import _lib

# (arguments, bytes) per query, generated from the library of the commit BEFORE the hooks (each query called with the arguments,
# the answer written down).  The three queries in FORMULA were hand-written sums with 4096 bytes of slack there; they are carved
# like the others now, so their pinned value is an upper bound and the exact statement is "the end of the last take + 256".
PARENT_SIZES = {
    "dh_reproject_workspace_bytes": [
        ((64, 0, 1), 326016),
        ((64, 1, 3), 844160),
        ((60, 977, 3), 801152),
        ((512, 20000, 8), 134917632),
    ],
    "dh_reproject_objects_workspace_bytes": [
        ((64, 700, 3, 2), 879488),
        ((60, 3136, 3, 1), 910976),
        ((288, 1, 1, 1), 5293952),
        ((512, 30000, 4, 8), 68175616),
    ],
    "dh_reproject_footprints_workspace_bytes": [
        ((64, 700, 3, 2, 0), 879488),
        ((64, 700, 3, 2, 1), 1041932),
        ((61, 1, 1, 1, 1), 348932),
        ((512, 30000, 2, 3, 1), 40786952),
    ],
    "dh_reproject_instances_workspace_bytes": [
        ((64, 4916, 3, 1, 2, 0), 1094528),
        ((64, 4916, 3, 1, 2, 1), 1583116),
        ((60, 50, 1, 2, 3, 0), 297856),
        ((256, 70000, 2, 2, 8, 1), 15450376),
    ],
    "dh_reproject_donor_workspace_bytes": [
        ((64, 900, 3, 2, 2, 0), 889984),
        ((128, 20000, 2, 3, 4, 0), 2813440),
        ((64, 5000, 1, 1, 1, 0), 411264),
    ],
    "dh_reproject_camera_workspace_bytes": [
        ((64, 900, 3, 2, 2, 0), 890496),
        ((128, 20000, 2, 3, 4, 0), 2813696),
        ((60, 1, 1, 1, 1, 0), 297088),
    ],
    "dh_reproject_background_workspace_bytes": [
        ((2,), 71040),
        ((60,), 296832),
        ((64,), 326016),
        ((288,), 5293440),
        ((512,), 16583552),
    ],
    "dh_laplacian_blend_workspace_bytes": [
        ((2,), 7948),
        ((64,), 262928),
        ((100,), 636956),
        ((160,), 1617724),
        ((300,), 5676728),
        ((512,), 16520456),
    ],
    "dh_mesh_workspace_bytes": [
        ((2,), 5644),
        ((32,), 50188),
        ((47,), 104464),
        ((64,), 188432),
        ((512,), 11801096),
    ],
    "dh_cells_workspace_bytes": [
        ((0, 64), 12860),
        ((1, 64), 12860),
        ((2048, 64), 22588),
        ((2049, 64), 23112),
        ((100000, 64), 513148),
        ((7, 1), 4912),
        ((5000, 16), 30024),
    ],
    "dh_energy_workspace_bytes": [
        ((8, 16, 0), 71424),
        ((8, 16, 1), 71424),
        ((320, 16, 255), 2308864),
        ((320, 16, 768), 2310912),
        ((1280, 32, 5000), 32841472),
        ((1, 1, 0), 5640),
    ],
    "dh_energy_plan_bytes": [
        ((16, 0), 5376),
        ((16, 1), 5376),
        ((16, 1280), 15104),
        ((64, 7000), 118784),
        ((1, 0), 2049),
    ],
    "dh_energy_plan_objects_bytes": [
        ((16, 0), 5761),
        ((16, 1), 5761),
        ((16, 1280), 21632),
        ((64, 7000), 154072),
        ((1, 0), 2689),
    ],
    "dh_energy_planned_workspace_bytes": [
        ((8, 16), 2576),
        ((320, 16), 12560),
        ((2048, 16), 67856),
        ((1280, 64), 74000),
        ((1, 1), 784),
    ],
    "dh_energy_planned_batch_workspace_bytes": [
        ((8, 16, 1), 2576),
        ((320, 16, 3), 37648),
        ((2048, 16, 3), 203536),
        ((1280, 64, 16), 1183760),
    ],
    "dh_energy_planned_objects_batch_workspace_bytes": [
        ((8, 16, 1), 2576),
        ((320, 16, 3), 37648),
        ((2048, 16, 3), 203536),
        ((1280, 64, 16), 1183760),
    ],
}

FORMULA = ("dh_laplacian_blend_workspace_bytes", "dh_mesh_workspace_bytes", "dh_cells_workspace_bytes")
CASES = [(name, args, size) for name, rows in PARENT_SIZES.items() for args, size in rows]
GAPS = (256, 4096, 65536)


def _query(L, name, args):
    nb = ctypes.c_size_t()
    assert getattr(L, name)(*args, ctypes.byref(nb)) == 0, (name, args, L.dh_last_error())
    return nb.value


def _logged(L, name, args):
    """(size, takes) of one query, takes = [(base, offset, bytes)] from the log"""
    assert L.dh_dbg_arena_log(1) == 0
    size = _query(L, name, args)
    n = ctypes.c_int(0)
    assert L.dh_dbg_arena_log_read(None, 0, ctypes.byref(n)) == 0
    out = (ctypes.c_int64 * (3 * max(n.value, 1)))()
    assert L.dh_dbg_arena_log_read(out, n.value, ctypes.byref(n)) == 0
    assert L.dh_dbg_arena_log(0) == 0
    return size, [tuple(out[3 * i:3 * i + 3]) for i in range(n.value)]


@pytest.fixture
def L():
    lib = _lib.lib()
    assert lib.dh_dbg_arena_gap(0) == 0 and lib.dh_dbg_arena_log(0) == 0
    yield lib
    lib.dh_dbg_arena_log(0)
    lib.dh_dbg_arena_gap(0)


def test_every_query_is_in_the_table():
    """every size query of the C ABI that an Arena answers (the U-Net engine's is a handle's, with its own allocator)"""
    mine = {n for n in _lib.SIGNATURES if n.endswith(("_workspace_bytes", "_plan_bytes", "_plan_objects_bytes"))} - {"dh_unet_workspace_bytes"}
    assert mine == set(PARENT_SIZES), mine ^ set(PARENT_SIZES)


@pytest.mark.parametrize("name,args,parent", CASES, ids=[f"{n[3:]}{a}" for n, a, _ in CASES])
def test_sizes_gaps_and_takes(L, name, args, parent):
    size, takes = _logged(L, name, args)
    assert takes, "the query carved nothing"
    # gap 0: the parent's answer (the three former formulas: no more than it, and the carving's own end + 256)
    if name in FORMULA:
        assert size <= parent, (size, parent)
    else:
        assert size == parent, (size, parent)
    assert all(base == 0 for base, _, _ in takes), "a query's arena is null-based"
    end = 0
    for _, off, nbytes in takes:
        assert off % 256 == 0 and off >= end and nbytes >= 0, (off, nbytes, end)
        assert off - end < 256, "only alignment padding lies between two takes at gap 0"
        end = off + nbytes
    assert end == size - 256
    for gap in GAPS:
        assert L.dh_dbg_arena_gap(gap) == 0
        g_size, g_takes = _logged(L, name, args)
        assert g_size == size + gap * len(takes), (gap, g_size, size, len(takes))
        assert len(g_takes) == len(takes)
        end = -gap
        for k, ((_, off0, n0), (_, off, nbytes)) in enumerate(zip(takes, g_takes)):
            assert nbytes == n0 and off == off0 + gap * k, (gap, k, off, off0)
            assert off % 256 == 0 and off >= end + gap, (gap, k)
            end = off + nbytes
        assert end + gap == g_size - 256            # (the gap lies behind the last take too)
    assert L.dh_dbg_arena_gap(0) == 0
    assert _logged(L, name, args) == (size, takes), "gap 0 after a gap restores the first answer"


@pytest.mark.parametrize("bad", [-256, -1, 1, 255, 257, 4095, 65536 + 256, 1 << 20])
def test_bad_gaps_are_refused_and_change_nothing(L, bad):
    assert L.dh_dbg_arena_gap(4096) == 0
    want = _query(L, "dh_mesh_workspace_bytes", (32,))
    assert L.dh_dbg_arena_gap(bad) != 0
    assert b"dh_dbg_arena_gap" in L.dh_last_error()
    assert _query(L, "dh_mesh_workspace_bytes", (32,)) == want


def test_the_log_clears_on_enable_and_stops_on_disable(L):
    _, a = _logged(L, "dh_cells_workspace_bytes", (5, 16))
    _query(L, "dh_cells_workspace_bytes", (5, 16))          # (disabled: not recorded)
    _, b = _logged(L, "dh_mesh_workspace_bytes", (8,))
    assert len(a) == 4 and len(b) == 7
    n = ctypes.c_int(-1)
    out = (ctypes.c_int64 * 6)()
    assert L.dh_dbg_arena_log_read(out, 2, ctypes.byref(n)) == 0 and n.value == 7          # (a short buffer: the first rows, n = all)
    assert [tuple(out[0:3]), tuple(out[3:6])] == b[:2]
    assert L.dh_dbg_arena_log_read(out, 2, None) != 0


# ---- tests/guarded.py on the CPU: the frame sees what it is there to see ------------------------------------------------------
def _frame(fill):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import guarded as G
    import torch
    f = G.Frame(fill, "cpu")
    return G, torch, f, G.TorchProxy(f)


@pytest.mark.parametrize("fill", ["zeros", "ones", "random"])
def test_frame_hands_out_aligned_filled_tensors_and_forwards_the_rest(fill):
    G, torch, f, P = _frame(fill)
    a = P.empty((3, 5), dtype=torch.int32, device="cpu")
    z = P.zeros(7, dtype=torch.float32, device=torch.device("cpu"))
    b = P.full((4,), 9, dtype=torch.uint8, device="cpu")
    e = P.empty(0, dtype=torch.int64, device="cpu")
    like = P.zeros_like(a)
    host = P.zeros((2, 2), dtype=torch.int64)                     # no device named: torch's own
    assert [r.tensor is t for r, t in zip(f.recs, (a, z, b, e, like))] == [True] * 5 and len(f.recs) == 5
    assert f.rec_of(host.data_ptr()) is None and P.float32 is torch.float32 and P.cat is torch.cat
    assert all(r.addr % 256 == 0 and r.start >= G.GUARD and r.buf.numel() - r.start - r.nbytes >= G.GUARD for r in f.recs)
    want = {"zeros": [0] * 15, "ones": [-1] * 15}.get(fill)
    assert want is None or a.flatten().tolist() == want
    assert z.tolist() == [0.0] * 7 and b.tolist() == [9] * 4 and like.tolist() == [[0] * 5] * 3 and e.numel() == 0
    assert f.find((3, 5), torch.int32) == [a, like] or f.find((3, 5), torch.int32)[0] is a
    assert "test_arena_hooks.py" in f.recs[0].name and "empty@" in f.recs[0].name
    f.check()
    f.unchanged(a[1:], "a")
    f.tail_unchanged(a[:1], "a")


@pytest.mark.parametrize("fill", ["zeros", "ones", "random"])
def test_frame_names_a_stray_write(fill):
    G, torch, f, P = _frame(fill)
    a = P.empty((3, 5), dtype=torch.int32, device="cpu")
    r = f.recs[0]
    for at, word in ((r.start + r.nbytes, "rear guard changed, first at byte 0 past"), (r.start - 1, "front guard changed, first at byte 1 before"),
                     (r.buf.numel() - 1, f"rear guard changed, first at byte {r.buf.numel() - 1 - r.start - r.nbytes} past")):
        r.buf[at] ^= 1
        with pytest.raises(AssertionError, match=word):
            f.check()
        r.buf[at] ^= 1
    f.check()
    a[2, 4] += 1
    f.unchanged(a[:2], "head")
    with pytest.raises(AssertionError, match="first at byte 56"):
        f.unchanged(a[2:], "tail")
    with pytest.raises(AssertionError, match="behind its written part, first at byte 56"):
        f.tail_unchanged(a[:1], "tail")


@pytest.mark.parametrize("fill", ["zeros", "ones", "random"])
def test_frame_judges_the_gaps_of_a_logged_arena(fill):
    G, torch, f, P = _frame(fill)
    ws = P.empty(2048, dtype=torch.uint8, device="cpu")
    other = P.empty(512, dtype=torch.uint8, device="cpu")
    base, b2 = ws.data_ptr(), other.data_ptr()
    # two arenas carved in turns (a batch: the workspace, an item's plan, the workspace again), and a query's null-based arena
    takes = [(base, 0, 100), (b2, 0, 16), (base, 256, 10), (0, 0, 5), (b2, 256, 16), (base, 512, 1000)]
    ws[0:100] = 1
    ws[256:266] = 2
    ws[512:1512] = 3
    other[0:16] = 4
    other[256:272] = 5
    assert f.check_arena_gaps(takes) == 2
    assert f.check_arena_gaps(takes + takes) == 4                     # an offset that goes back starts a new arena on that base
    for at, word in ((100, "0 bytes past the end of take 0 of 3"), (255, "155 bytes past the end of take 0"), (266, "take 1 of 3"),
                     (1512, "0 bytes past the end of take 2"), (2047, "take 2 of 3")):
        ws[at] ^= 0x5A
        with pytest.raises(AssertionError, match=word):
            f.check_arena_gaps(takes)
        ws[at] ^= 0x5A
    with pytest.raises(AssertionError, match="leaves the tensor"):
        f.check_arena_gaps([(b2, 0, 16), (b2, 256, 257)])
