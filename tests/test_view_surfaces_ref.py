"""CPU: view surfaces ("View surfaces") -- the test-side reference tests/view_surfaces_ref.py against
tests/camera_moves_ref.py where the setting is off, its own geometry (the table of the DESIGN section, re-derived), a quad worked
by hand, and every host-side part of the product: the validator, the parameter lists, the header, the plan, the refusals of the
DiffusionHandles entries and of tools/run_edit.py before any device work."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reproject_calls as RC  # noqa: E402
import camera_moves_ref as CM  # noqa: E402
import test_arena_hooks as AH  # noqa: E402  (helpers only: the arena fixture, the pinned sizes, the size / gap / take checks)
import multi_object_ref as R  # noqa: E402
import similarity_ref as S  # noqa: E402
import view_surfaces_ref as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y = R.Y
Z3 = (0.0, 0.0, 0.0)
GEOMETRY = ("zmap", "raw_mask", "cleaned", "vis", "tx", "ty", "inpaint", "unowned", "disparity", "owner", "gone", "corr_inst", "row_kind")

# camera -> (unowned with points, unowned with surfaces, pixels whose owner goes from a background point to an instance), 128 x 128,
# two_spheres with edit 0 of similarity_ref.edits_for, no ratio: the table of the DESIGN section
TABLE = {
    "pan": (1630, 1404, 358), "orbit": (1493, 782, 260), "dolly_in": (1902, 0, 758), "dolly_out": (1806, 1806, 191),
    "truck": (916, 795, 390), "general": (1680, 533, 480), "dolly_in_1": (5545, 0, 1728), "orbit_20": (3215, 1675, 397),
}


def _same(a, b, what):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), what
    for k in GEOMETRY:
        assert np.array_equal(a[2][k], b[2][k]), (what, k)


# ---- 1. the setting off, and an edit without a camera ----------------------------------------------------------------------------
def test_off_and_without_a_camera_it_is_the_camera_reference():
    fx = CM.fixture(64)
    args = (fx["depth"], fx["bg_depth"], fx["masks"], [0, 1], fx["transforms"])
    for name in CM.CAMERA_NAMES + ("none",):
        cam = fx["cameras"].get(name)
        _same(V.transform_surfaces(*args, cam, view_surfaces=False), fx["geo"][name], f"off, {name}")
    _same(V.transform_surfaces(*args, None, view_surfaces=True), fx["geo"]["none"], "on, no camera")
    _same(V.transform_surfaces(*args, None, view_surfaces=True, max_ratio=1.5), fx["geo"]["none"], "on with a ratio, no camera")
    # on with a camera it is another result
    on = V.transform_surfaces(*args, fx["cameras"]["dolly_in"], view_surfaces=True)
    assert not np.array_equal(on[2]["owner"], fx["geo"]["dolly_in"][2]["owner"])


# ---- 2. the table ----------------------------------------------------------------------------------------------------------------
def test_the_table_of_the_design_section():
    res = 128
    R2 = res * res
    depth, bg, masks = R.two_spheres(res)
    tfs = S.edits_for(res, depth)[0]
    cams = dict(V.cameras_for(depth), orbit_20=(20.0, Y, Z3, CM.centre_pivot(depth)))
    assert set(cams) == set(TABLE)
    for name, cam in cams.items():
        p = CM.transform_camera(depth, bg, masks, [0, 1], tfs, cam, infill=False)[2]
        s = V.transform_surfaces(depth, bg, masks, [0, 1], tfs, cam, (), True, None, infill=False)[2]
        a, b = p["owner"], s["owner"]
        to_instance = int(((a >= 0) & (a < R2) & (b >= R2)).sum())
        got = (int(p["unowned"].sum()), int(s["unowned"].sum()), to_instance)
        print(name, got, "instance -> background", int(((a >= R2) & (b < R2)).sum()), "owned -> unowned", int(((a >= 0) & (b < 0)).sum()))
        assert got == TABLE[name], (name, got)
        assert got[1] <= got[0], name
        # between the two paths a pixel goes from a background point to an instance or from unowned to owned, never back: no
        # instance pixel becomes background or unowned, no owned pixel unowned (the index WITHIN a kind may change: a triangle
        # of the same surface in front of the point)
        assert not ((a >= R2) & (b < R2)).any() and not ((a >= 0) & (b < 0)).any(), name
        changed_kind = ((a >= R2) != (b >= R2)) | ((a < 0) != (b < 0))
        assert int(changed_kind.sum()) == to_instance + (got[0] - got[1]), name
    assert TABLE["dolly_out"][0] == TABLE["dolly_out"][1] and TABLE["dolly_in"][1] == 0 and TABLE["dolly_in_1"][1] == 0


# ---- 3. the stepped background ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,truck,dolly", [(64, (384, 320, 384), (0, 18)), (128, (1536, 1152, 1536), (0, 38))])
def test_the_step_fixture(res, truck, dolly):
    """(unowned with points, with surfaces, with surfaces and ratio 1.1) under the truck by 0.3; (surfaces, ratio 1.1) under the
    dolly in by 0.5: without a ratio the sheet across the step covers 64 (384 at 128) unowned pixels, with 1.1 none; the seam
    opens under the dolly."""
    bg = V.step_background(res)
    unowned = lambda r: int(r[2]["unowned"].sum())
    got = (unowned(CM.background_camera(bg, V.STEP_TRUCK, infill=False)), unowned(V.background_surfaces(bg, V.STEP_TRUCK, infill=False)),
           unowned(V.background_surfaces(bg, V.STEP_TRUCK, max_ratio=1.1, infill=False)))
    assert got == truck
    got = (unowned(V.background_surfaces(bg, V.STEP_DOLLY, infill=False)), unowned(V.background_surfaces(bg, V.STEP_DOLLY, max_ratio=1.1, infill=False)))
    assert got == dolly
    # the guard is on the SOURCE depths (4 against 3 across the step): 1.3 cuts the sheet, 1.4 does not
    assert unowned(V.background_surfaces(bg, V.STEP_TRUCK, max_ratio=1.3, infill=False)) == truck[2]
    assert unowned(V.background_surfaces(bg, V.STEP_TRUCK, max_ratio=1.4, infill=False)) == truck[1]


# ---- 4. the rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("removed", [False, True])
def test_background_and_instance_rows(removed):
    res = 64
    fx = V.fixture(res, (0, 1), removed, False)
    covered = np.zeros(res * res, dtype=bool)
    for m in list(fx["masks"]) + list(fx["removed"]):
        covered |= (m[0, 0].numpy() != 0).reshape(-1)
    for name, (_, corr, g) in fx["geo"].items():
        corr, n = corr.numpy(), g["n_instance_rows"]
        inst, back = corr[:n], corr[n:]
        if name == "none":
            assert len(back) == 0
            continue
        assert len(back) == g["n_background"] > 1000 and n > 100
        assert not covered[back[:, 1] * res + back[:, 0]].any(), f"{name}: a background row from under a mask"
        assert (g["cleaned"][back[:, 3], back[:, 2]] == 0).all(), f"{name}: a background row inside the cleaned mask"
        assert (g["cleaned"][inst[:, 3], inst[:, 2]] == 255).all() and g["raw_mask"][inst[:, 3], inst[:, 2]].all()
        for rows in (inst, back):
            t = rows[:, 3] * res + rows[:, 2]
            assert (np.diff(t) > 0).all(), f"{name}: rows not in row-major target order (or a pixel twice)"
        assert (g["row_kind"][:n] == 0).all() and (g["row_kind"][n:] == 2).all() and (g["corr_inst"][n:] == len(fx["instances"])).all()
        # the owner of a background row's pixel is its source pixel; vis = the point owns a pixel; the target of a point is its own
        assert np.array_equal(g["owner"][back[:, 3] * res + back[:, 2]], back[:, 1] * res + back[:, 0])
        own = g["owner"][g["owner"] >= res * res] - res * res
        assert np.array_equal(np.nonzero(g["vis"])[0], np.unique(own))
        assert ((g["tx"] == -1) == g["gone"][res * res:]).all() and ((g["ty"] == -1) == g["gone"][res * res:]).all()


# ---- 5. one quad of background, by hand ------------------------------------------------------------------------------------------
def test_one_background_sheet_by_hand():
    """A 3 x 3 background, a plane at depth 2 seen with fx = fy = 1: pixel (col, row) is the point (2 (1 - col), 2 (1 - row), 2).
    The camera moves one unit closer (a pure translation): Z = 1, u = 2 col - 1, v = 2 row - 1 -- a magnification by 2 about the
    centre pixel.  Eight of the nine vertices leave the frame (u or v = -1 or 3) and still span the triangles that cover it.

    In the coordinates of a source quad (a along the columns, b along the rows, the quad's v00 at (0, 0)) half 0 = (v10, v11,
    v01) covers a + b >= 1 with the weights (1 - a, a + b - 1, 1 - b) / 1, half 1 = (v10, v01, v00) covers a + b <= 1 with
    (b, a, 1 - a - b); target pixel (c, r) lies at the source position ((c + 1) / 2, (r + 1) / 2).  Every area is 4, every weight
    a multiple of 1, every z exactly 1: the winner of a pixel is the smallest bidder index.
      (0,0) inside quad 00 on its diagonal: both halves, weights (.5, 0, .5) and (.5, .5, 0) -> v10 = pixel 3 both times
      (1,0) on the edge of quads 00 and 01: half 0 of 00 (0, .5, .5) -> v11 = 4; half 1 of 01 (.5, 0, .5) -> v10 = 4
      (2,0) inside quad 01 on its diagonal -> v10 = 4          (0,1) half 0 of 00 (.5, .5, 0) -> 3; half 1 of 10 (0, .5, .5) -> v01 = 4
      (1,1) the centre vertex, 4 from all six triangles around it and from its own point
      (2,1) half 0 of 01 (.5, .5, 0) -> 4; half 1 of 11 -> v01 = 5          (0,2) quad 10's diagonal -> v10 = 6
      (1,2) half 0 of 10 (0, .5, .5) -> v11 = 7; half 1 of 11 (.5, 0, .5) -> v10 = 7          (2,2) quad 11's diagonal -> v10 = 7
    Boxes (clipped to the image) and inclusive edges: quad 00 bids 4 + 1 times, 01 and 10 3 + 3 times, 11 1 + 4 times: 22."""
    res, K = 3, torch.eye(3)
    col, row = np.meshgrid(np.arange(3.0), np.arange(3.0))
    before = np.stack([2.0 * (1.0 - col), 2.0 * (1.0 - row), np.full((3, 3), 2.0)], axis=-1).reshape(-1, 3)
    u0, v0 = CM.unclamped_uv(before, K, res)
    assert np.array_equal(u0, col.reshape(-1)) and np.array_equal(v0, row.reshape(-1))          # the source view
    pts = before - np.array([0.0, 0.0, 1.0])
    u, v = CM.unclamped_uv(pts, K, res)
    assert np.array_equal(u, 2.0 * col.reshape(-1) - 1.0) and np.array_equal(v, 2.0 * row.reshape(-1) - 1.0)
    gone = CM.discarded(pts, K, res)
    assert np.array_equal(np.nonzero(~gone)[0], [4])
    bg = torch.full((1, 1, 3, 3), 2.0)
    pix, z, idx = V.surface_bids(pts, np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64), bg, bg, res, K)
    assert len(pix) == 22 and (z == 1.0).all()
    per_pixel = {p: sorted(idx[pix == p].tolist()) for p in range(9)}
    assert per_pixel == {0: [3, 3], 1: [4, 4], 2: [4, 4], 3: [3, 4], 4: [4] * 6, 5: [4, 5], 6: [6, 6], 7: [7, 7], 8: [7, 7]}
    zmap, owner = V.winners(np.concatenate([[4], pix]), np.concatenate([[1.0], z]), np.concatenate([[4], idx]), 9)
    assert owner.tolist() == [3, 4, 4, 3, 4, 4, 6, 7, 7] and (zmap == 1.0).all()
    # the guard leaves nothing out here (one depth), and a sheet seen from behind bids for nothing (area <= 0)
    assert len(V.surface_bids(pts, np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64), bg, bg, res, K, 1.01)[0]) == 22
    flipped = pts * np.array([-1.0, 1.0, 1.0])
    assert len(V.surface_bids(flipped, np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64), bg, bg, res, K)[0]) == 0


# ---- 6. validator, parameter lists, header ---------------------------------------------------------------------------------------
def test_check_view_surfaces():
    from diffusionhandles_amd import depth_transform as DT
    assert list(inspect.signature(DT.check_view_surfaces).parameters) == ["view_surfaces", "view_surface_max_ratio", "what"]
    assert DT.check_view_surfaces(False, None) == (False, None) and DT.check_view_surfaces(1, None) == (True, None)
    assert DT.check_view_surfaces(True, 1.5) == (True, 1.5) and DT.check_view_surfaces(True, 1.1)[1] == float(np.float32(1.1))
    for bad in (1.0, 0.5, 0.0, -2.0, float("nan"), float("inf"), 1e39, 1.0 + 1e-9, "x", True, [1.5]):
        with pytest.raises(ValueError, match="my_call: view_surface_max_ratio"):
            DT.check_view_surfaces(True, bad, "my_call")
    with pytest.raises(ValueError, match="without view_surfaces"):
        DT.check_view_surfaces(False, 1.5)
    depth, bg, masks = R.two_spheres(64)
    K, tf, cam = torch.eye(3), (10.0, Y, Z3), (4.0, Y, Z3, None)
    for call in (lambda **kw: DT.reproject(depth, bg, masks, K, [[tf, tf]], cameras=[cam], **kw),
                 lambda **kw: DT.reproject_plan(depth, masks, [[tf, tf]], cameras=[cam], **kw),
                 lambda **kw: DT.reproject_surface_edits(depth, bg, masks, K, [[tf, tf]], cameras=[cam], **kw),
                 lambda **kw: DT.reproject_surface_edits(depth, bg, masks, K, [[tf, tf]], **kw)):
        with pytest.raises(ValueError, match="without view_surfaces"):
            call(view_surface_max_ratio=1.5)
        with pytest.raises(ValueError, match="view_surface_max_ratio"):
            call(view_surfaces=True, view_surface_max_ratio=1.0)
    # a donor, and footprints with a camera (as before), are refused on the host
    ddepth, dmask = depth.clone(), [masks[1]]
    with pytest.raises(NotImplementedError, match="depth_transform_view_surfaces"):
        DT.reproject_plan(depth, masks[:1], [[tf, tf]], donor_depth=ddepth, donor_masks=dmask, view_surfaces=True)
    with pytest.raises(NotImplementedError, match="footprints with a camera"):
        DT.reproject_plan(depth, masks, [[tf, tf]], cameras=[cam], footprints=True, view_surfaces=True)
    with pytest.raises(NotImplementedError, match="view surfaces"):
        DT.mesh_has_no_view_surfaces(True, None, "x")
    assert DT.mesh_has_no_view_surfaces(False, None, "x") is None


def test_parameter_lists_signatures_and_header():
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd import depth_transform as DT
    border = inspect.signature(DT.reproject_border_edits).parameters
    new = inspect.signature(DT.reproject_surface_edits).parameters
    assert list(new) == list(border) + ["view_surfaces", "view_surface_max_ratio"]
    assert new["view_surfaces"].default is False and new["view_surface_max_ratio"].default is None
    for f in (DT.reproject, DT.reproject_plan):
        ps = inspect.signature(f).parameters
        assert list(ps)[-2:] == ["view_surfaces", "view_surface_max_ratio"]
        assert all(ps[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(ps)[-2:])
        assert ps["view_surfaces"].default is False and ps["view_surface_max_ratio"].default is None
    for f in (DT.reproject_border_edits, DT.reproject_camera_edits, DT.reproject_donor_edits, DT.reproject_object_edits, DT.reproject_edits,
              DT.transform_depth, DT.transform_depth_pc, DT.transform_depth_mesh, DT.transform_depth_footprints):
        assert "view_surfaces" not in inspect.signature(f).parameters, f.__name__
    sig = _lib.SIGNATURES
    for new_name, old_name in (("dh_reproject_surface_edits", "dh_reproject_border_edits"),
                               ("dh_reproject_surface_background", "dh_reproject_border_background")):
        assert sig[new_name][1] == sig[old_name][1] + [_lib.c_i, _lib.c_f] and sig[new_name][0] == sig[old_name][0]
    assert sig["dh_reproject_surface_ws_bytes"] == sig["dh_reproject_camera_workspace_bytes"]
    assert len(sig["dh_reproject_surface_background_ws_bytes"][1]) == len(sig["dh_reproject_background_workspace_bytes"][1]) + 1
    header = open(os.path.join(ROOT, "include", "diffhandles_hip.h")).read()
    for name in ("dh_reproject_surface_edits", "dh_reproject_surface_background", "dh_reproject_surface_ws_bytes",
                 "dh_reproject_surface_background_ws_bytes"):
        assert f"int {name}(" in header
    assert "int view_surfaces, float surface_max_ratio);" in header and "that entry is this one's (0, 0.f) call" in header
    # the queries answer without a device; with 0 they are the queries they extend
    import ctypes
    L = _lib.lib()

    def q(name, *a):
        nb = ctypes.c_size_t()
        assert getattr(L, name)(*a, ctypes.byref(nb)) == 0, L.dh_last_error()
        return nb.value
    for a in ((64, 900, 3, 2, 2), (128, 20000, 8, 2, 3)):
        off, on = q("dh_reproject_surface_ws_bytes", *a, 0), q("dh_reproject_surface_ws_bytes", *a, 1)
        assert off == q("dh_reproject_camera_workspace_bytes", *a, 0)
        res, n_pts, K = a[:3]
        extra = K * (res * res + n_pts) * 24 + res * res * 4 + K * (2 * n_pts + 2 * (res - 1) ** 2) * 4 + K * 4
        assert extra <= on - off < extra + 4 * 256          # (the stored vertices, the inverse map, the list, its counters; alignment)
    assert q("dh_reproject_surface_background_ws_bytes", 64, 0) == q("dh_reproject_background_workspace_bytes", 64)
    assert q("dh_reproject_surface_background_ws_bytes", 64, 1) > q("dh_reproject_background_workspace_bytes", 64) + 64 * 64 * 24
    nb = ctypes.c_size_t(7)
    assert L.dh_reproject_surface_ws_bytes(64, 900, 3, 2, 2, 2, ctypes.byref(nb)) != 0 and nb.value == 7


# (arguments, bytes) of the two new size queries: with view_surfaces = 0 the numbers tests/test_arena_hooks.py pins for
# dh_reproject_camera_workspace_bytes / dh_reproject_background_workspace_bytes with the same arguments, with 1 the carving of the
# build that added them, written down once.  Checked as that file checks every other query: the size, the takes, the gaps.
SURFACE_SIZES = {
    "dh_reproject_surface_ws_bytes": [((64, 900, 3, 2, 2, 0), 890496), ((128, 20000, 2, 3, 4, 0), 2813696), ((60, 1, 1, 1, 1, 0), 297088),
                                      ((64, 900, 3, 2, 2, 1), 1383948), ((60, 1, 1, 1, 1, 1), 426244)],
    "dh_reproject_surface_background_ws_bytes": [((2, 0), 71040), ((60, 0), 296832), ((64, 0), 326016), ((2, 1), 71684), ((64, 1), 456452)],
}
SURFACE_CASES = [(name, args, size) for name, rows in SURFACE_SIZES.items() for args, size in rows]
L = AH.L          # (the fixture: the library with the arena hooks at rest before and after)


@pytest.mark.parametrize("name,args,size", SURFACE_CASES, ids=[f"{n[3:]}{a}" for n, a, _ in SURFACE_CASES])
def test_sizes_gaps_and_takes_of_the_surface_queries(L, name, args, size):
    if args[-1] == 0:
        old = "dh_reproject_camera_workspace_bytes" if len(args) > 2 else "dh_reproject_background_workspace_bytes"
        assert (args if len(args) > 2 else args[:1], size) in AH.PARENT_SIZES[old], "not a row of the query it extends"
    AH.test_sizes_gaps_and_takes(L, name, args, size)


# ---- 7. the plan -----------------------------------------------------------------------------------------------------------------
def test_the_plan_names_the_surface_entries_only_with_a_camera():
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, masks = R.two_spheres(64)
    tf, cam = (10.0, Y, Z3), (4.0, Y, Z3, None)
    for border, value in (("zero", 0), ("reflect", 1)):
        p = DT.reproject_plan(depth, masks, [[tf, tf], [tf, tf]], cameras=[cam, None], view_surfaces=True, view_surface_max_ratio=1.25,
                              infill_border=border)
        assert (p.kind, RC.fields(p)) == ("objects", dict(RC.SURFACE, border=value))          # views, the setting, no bones, the table
        assert p.cap == 64 * 64 and p.view_surfaces is True and p.surface_ratio == 1.25 and p.infill_border == value and p.with_table
        q = DT.reproject_plan(depth, masks, [[tf, tf], [tf, tf]], cameras=[cam, None], infill_border=border)
        assert q.view_surfaces is False and q.surface_ratio is None and q.cap == q.n_pts == p.n_pts
        assert RC.fields(q) == (RC.border(RC.CAMERA) if value else RC.CAMERA)
        assert DT.reproject_record(q, 2).view_surfaces == 0 and list(DT.reproject_record(q, 2).has_view[0:2]) == [1, 0]
        p = DT.reproject_plan(depth, [], [[]], cameras=[cam], view_surfaces=True, infill_border=border)
        assert (p.kind, RC.fields(p), p.view_surfaces) == ("pure_camera", dict(RC.SURFACE_BACKGROUND, border=value), True)
    # off, and on without a camera: every plan is the one it was, field for field
    for kw in (dict(), dict(instances=[0, 1, 0]), dict(footprints=True), dict(infill_border="reflect"), dict(cameras=[None]),
               dict(removed_masks=[])):
        n = 3 if "instances" in kw else 2
        a = DT.reproject_plan(depth, masks, [[tf] * n], **kw)
        for extra in (dict(view_surfaces=False), dict(view_surfaces=True), dict(view_surfaces=True, view_surface_max_ratio=1.5)):
            b = DT.reproject_plan(depth, masks, [[tf] * n], **kw, **extra)
            assert b.view_surfaces is False and b.surface_ratio is None
            for k, v in vars(a).items():
                w = getattr(b, k)
                same = torch.equal(v, w) if isinstance(v, torch.Tensor) else np.array_equal(v, w) if isinstance(v, np.ndarray) else \
                    v is w or v == w or k in ("edits", "inst")
                assert same, (kw, extra, k)
    a = DT.reproject_plan(depth, [], [[]], removed_masks=masks)
    b = DT.reproject_plan(depth, [], [[]], removed_masks=masks, view_surfaces=True)
    assert (a.kind, RC.fields(a)) == (b.kind, RC.fields(b)) == ("pure_removal", RC.BACKGROUND)


# ---- 8. the edit calls and the tool ----------------------------------------------------------------------------------------------
def _camera_calls(dh):
    """The entries of DiffusionHandles that read a camera, as thunks (name, call)."""
    depth, bg, masks = R.two_spheres(128)
    tf, cam = (10.0, Y, Z3), (4.0, Y, Z3)
    common = dict(depth=depth, prompt="two spheres", bg_depth=bg, null_text_emb=None, init_noise=None, activations=[depth])
    return [
        ("transform_foreground_objects", lambda: dh.transform_foreground_objects(depth, "two spheres", masks, bg, None, None, None, [tf, tf],
                                                                                 camera=cam)),
        ("transform_foreground_objects_batch",
         lambda: dh.transform_foreground_objects_batch(depth, "two spheres", masks, bg, None, None, None, [[tf, tf]], cameras=[cam])),
        ("transform_foregrounds", lambda: dh.transform_foregrounds([dict(common, fg_masks=masks, transforms=[tf, tf], camera=cam)])),
    ]


def test_the_conf_keys_reach_the_plan_of_every_camera_call(monkeypatch):
    from diffusionhandles_amd import conf as C
    from diffusionhandles_amd import depth_transform as DT
    import test_footprints_ref as FP

    class Reached(Exception):
        pass

    seen = []

    def run_plan(p, *a, **kw):
        seen.append((RC.fields(p), p.view_surfaces, p.surface_ratio, p.cap == p.res * p.res))
        raise Reached

    monkeypatch.setattr(DT, "_run_plan", run_plan)
    on = (RC.SURFACE, True)
    for keys, want in ((dict(), (RC.CAMERA, False, None, False)),
                       (dict(depth_transform_view_surfaces=False), (RC.CAMERA, False, None, False)),
                       (dict(depth_transform_view_surfaces=True), on + (None, True)),
                       (dict(depth_transform_view_surfaces=True, depth_transform_view_surface_max_ratio=1.5), on + (1.5, True))):
        dh = FP._handles("pc", **keys)
        for name, call in _camera_calls(dh):
            seen.clear()
            with pytest.raises(Reached):
                call()
            assert seen == [want], (name, keys, seen)
        # without a camera the key changes no plan
        for name, call in FP._every_edit_call(dh)[1:]:
            seen.clear()
            with pytest.raises(Reached):
                call()
            assert len(seen) == 1 and seen[0][1:3] == (False, None) and seen[0][0]["surfaces"] == 0, (name, keys, seen)
    assert "depth_transform_view_surfaces" not in C.load_default() and "depth_transform_view_surface_max_ratio" not in C.load_default()


def test_refusals_of_the_edit_calls_before_any_device_work():
    import test_footprints_ref as FP
    depth, bg, masks = R.two_spheres(128)
    # mesh mode refuses a true key in every edit call, with or without a camera; a false key is no error of this setting
    for calls in (FP._every_edit_call, _camera_calls):
        for name, call in calls(FP._handles("mesh", depth_transform_view_surfaces=True)):
            with pytest.raises(NotImplementedError, match="depth_transform_view_surfaces"):
                call()
    assert FP._handles("mesh", depth_transform_view_surfaces=False)._view_surfaces("x") == dict(view_surfaces=False, view_surface_max_ratio=None)
    # malformed keys: ValueError naming the call and the key
    for keys in (dict(depth_transform_view_surface_max_ratio=1.5), dict(depth_transform_view_surfaces=True, depth_transform_view_surface_max_ratio=1.0),
                 dict(depth_transform_view_surfaces=True, depth_transform_view_surface_max_ratio="x")):
        for calls in (FP._every_edit_call, _camera_calls):
            for name, call in calls(FP._handles("pc", **keys)):
                with pytest.raises(ValueError, match=f"{name}.*conf depth_transform_view_surfaces"):
                    call()
    # a donor refuses the setting, naming it, before any identity
    dh = FP._handles("pc", depth_transform_view_surfaces=True)
    donor = dict(depth=depth, masks=[masks[1]], activations=[depth])
    tf = (10.0, Y, Z3)
    with pytest.raises(NotImplementedError, match="depth_transform_view_surfaces: true has no object insertion"):
        dh.transform_foreground_objects(depth, "two spheres", masks[:1], bg, None, None, [depth], [tf, tf], donor=donor)
    # footprints with a camera stay refused as they are, the setting on or off
    for keys in (dict(depth_transform_footprints=True), dict(depth_transform_footprints=True, depth_transform_view_surfaces=True)):
        for name, call in _camera_calls(FP._handles("pc", **keys)):
            with pytest.raises(NotImplementedError, match="depth_transform_footprints: true has no camera moves"):
                call()
    # the helper's dicts: what every other caller of the footprint helper sees is what it was
    dh = FP._handles("pc", depth_transform_view_surfaces=True, depth_transform_view_surface_max_ratio=2.0)
    assert dh._footprints("x") == dict(footprints=False, footprint_max_ratio=None)
    assert dh._reproject_keywords("x") == dict(footprints=False, footprint_max_ratio=None, infill_border="zero")
    assert dh._reproject_keywords("x", cameras=True) == dict(footprints=False, footprint_max_ratio=None, infill_border="zero",
                                                             view_surfaces=True, view_surface_max_ratio=2.0)


def test_run_edit_view_surface_arguments():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import run_edit
    from diffusionhandles_amd import conf as C
    conf = C.load_default()
    assert run_edit.apply_view_surface_args(run_edit.parse(["--scene", "x"]), conf) == {}
    assert "depth_transform_view_surfaces" not in conf
    conf = C.load_default()
    args = run_edit.parse(["--scene", "x", "--view-surfaces"])
    assert run_edit.apply_view_surface_args(args, conf) == dict(view_surfaces=True, view_surface_max_ratio=None) == args.view_surface_report
    assert conf.depth_transform_view_surfaces is True
    conf = C.load_default()
    args = run_edit.parse(["--scene", "x", "--view-surfaces", "--view-surface-max-ratio", "1.5"])
    assert run_edit.apply_view_surface_args(args, conf) == dict(view_surfaces=True, view_surface_max_ratio=1.5)
    assert conf.depth_transform_view_surface_max_ratio == 1.5
    for bad in (["--view-surface-max-ratio", "1.5"], ["--view-surfaces", "--view-surface-max-ratio", "1.0"],
                ["--view-surfaces", "--view-surface-max-ratio", "nan"]):
        with pytest.raises(ValueError, match="--view-surfaces"):
            run_edit.apply_view_surface_args(run_edit.parse(["--scene", "x"] + bad), C.load_default())
    with pytest.raises(SystemExit):
        run_edit.parse(["--scene", "x", "--view-surface-max-ratio", "x"])
    conf = C.load_default()
    conf.depth_transform_mode = "mesh"
    with pytest.raises(NotImplementedError, match="--view-surfaces"):
        run_edit.apply_view_surface_args(run_edit.parse(["--scene", "x", "--view-surfaces"]), conf)
    conf = C.load_default()
    conf.depth_transform_mode = "mesh"
    assert run_edit.apply_view_surface_args(run_edit.parse(["--scene", "x"]), conf) == {}
    # a configuration file that carries the keys is honoured without the flags, and load_conf knows them
    conf = C.load_default()
    conf["depth_transform_view_surfaces"] = True
    conf["depth_transform_view_surface_max_ratio"] = 2.0
    assert run_edit.apply_view_surface_args(run_edit.parse(["--scene", "x"]), conf) == dict(view_surfaces=True, view_surface_max_ratio=2.0)
    src = open(os.path.join(ROOT, "tools", "run_edit.py")).read()
    assert '"depth_transform_view_surfaces", ' in src and "apply_view_surface_args(args, conf)" in src
    bench = open(os.path.join(ROOT, "tools", "bench_reproject.py")).read()
    assert "DH_VIEW_SURFACES" in bench and "DH_VIEW_SURFACE_RATIO" in bench
