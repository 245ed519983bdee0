"""CPU: depth_transform.reproject_plan, the host decisions of a re-projection call, on a 16 x 16 scene of CPU tensors: no GPU and
no library (the plan makes no `_lib` call, asks for no compute device and allocates nothing there).  The expected fields were read
off the code before the plan existed (DESIGN.md "One host path for the re-projection") and confirmed against it."""
import os
import sys

import numpy as np
import pytest
import torch

from diffusionhandles_amd import _lib
from diffusionhandles_amd import depth_transform as DT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reproject_calls as RC  # noqa: E402

RES = 16
Y = torch.tensor([0.0, 1.0, 0.0])
GOOD = (10.0, Y, torch.zeros(3))
CAM = (5.0, Y, torch.zeros(3))
FOOTPRINT, INSTANCE = RC.FOOTPRINT, RC.INSTANCE


def box(r0, r1, c0, c1):
    m = torch.zeros((1, 1, RES, RES))
    m[..., r0:r1 + 1, c0:c1 + 1] = 1.0
    return m


A, B, E, R, DN = box(2, 4, 2, 5), box(8, 9, 8, 12), torch.zeros((1, 1, RES, RES)), box(12, 13, 1, 3), box(0, 1, 0, 2)
DEPTH = torch.ones((1, 1, RES, RES))


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    """The plan is host arithmetic: the library and the compute device are out of reach for the whole module."""
    def refuse(*a, **k):
        raise AssertionError("reproject_plan reached for the library or the compute device")
    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "require_gpu", refuse)
    monkeypatch.setattr(DT, "_compute_device", refuse)


def plan(masks, n_edits=1, n_transforms=None, **kw):
    n = len(kw["instances"]) if kw.get("instances") is not None else len(masks) + len(kw.get("donor_masks") or [])
    n = n if n_transforms is None else n_transforms
    return DT.reproject_plan(DEPTH, masks, [[GOOD] * n for _ in range(n_edits)], **kw)


def ints(v):
    return [int(x) for x in v]


def test_one_object_two_edits():
    for p in (plan([A], 2), plan([A], 2, cameras=[None, None])):          # cases 1 and 15: cameras all None is the call without
        assert p.kind == "objects" and RC.fields(p) == FOOTPRINT
        assert p.kept == [0] and ints(p.obj_start) == [0, 12] and p.obj_start.dtype == np.int32
        assert (p.n_fg, p.n_pts, p.cap) == (12, 12, 12)
        assert not p.with_table and not p.return_instances and p.cams is None
        assert (p.M, p.D, p.N) == (1, 0, 1) and len(p.edits) == 2


def test_footprints_take_one_row_per_target_pixel():
    p = plan([A, B], footprints=True)                                      # case 2
    assert p.kind == "objects" and RC.fields(p) == FOOTPRINT
    assert (p.n_fg, p.cap) == (22, RES * RES)


def test_an_empty_mask_is_dropped_with_its_transform():
    p = plan([A, E, B])                                                    # case 3
    assert RC.fields(p) == FOOTPRINT and not p.with_table
    assert p.kept == [0, 2] and ints(p.obj_start) == [0, 12, 22]
    assert p.caller == [0, 2] and ints(p.inst_obj) == [0, 1]


def test_an_instance_table():
    p = plan([A, B], instances=[1, 0, 1])                                  # case 4
    assert p.kind == "objects" and RC.fields(p) == INSTANCE and p.with_table
    assert ints(p.inst_obj) == [1, 0, 1] and ints(p.inst_start) == [0, 10, 22, 32] and p.inst_start.dtype == np.int32
    assert (p.n_fg, p.n_pts, p.cap) == (22, 32, 32) and p.N == 3
    p = plan([A, E, B], instances=[2, 1, 0, 0])                            # case 5
    assert p.kept == [0, 2] and p.caller == [0, 2, 3]
    assert ints(p.inst_obj) == [1, 0, 0] and ints(p.inst_start) == [0, 10, 22, 34]


def test_removed_masks():
    p = plan([A], removed_masks=[R])                                       # case 6
    assert p.kind == "objects" and RC.fields(p) == FOOTPRINT
    assert int(p.vacated.sum()) == 6 and len(p.removed) == 1
    p = plan([], 3, removed_masks=[R])                                     # case 7
    assert p.kind == "pure_removal" and RC.fields(p) == RC.BACKGROUND
    assert DT.reproject_record(p, 3).n_edits == 1                          # (one call, its result for every edit)
    assert len(p.edits) == 3 and int(p.vacated.sum()) == 6 and (p.M, p.N, p.n_fg, p.n_pts) == (0, 0, 0, 0)
    p = plan([E], removed_masks=[R])                                       # case 8
    assert p.kind == "pure_removal" and RC.fields(p) == RC.BACKGROUND and p.M == 1


def test_every_mask_empty_is_the_empty_result():
    p = plan([E])                                                          # case 9
    assert p.kind == "empty" and p.n_fg == 0
    with pytest.raises(ValueError, match="launches nothing"):             # no call, so no record and no workspace
        DT.reproject_record(p, 1)


def test_a_donor():
    p = plan([A], donor_depth=DEPTH, donor_masks=[DN])                     # case 10
    assert p.kind == "objects" and RC.fields(p) == RC.DONOR
    assert p.kept == [0, 1] and ints(p.obj_start) == [0, 12, 18] and p.n_host_kept == 1
    assert p.return_instances and p.with_table and (p.M, p.D, p.N) == (1, 1, 2)
    assert p.donor[0] is DEPTH and len(p.donor[1]) == 1
    p = plan([], donor_depth=DEPTH, donor_masks=[DN])                      # case 11
    assert RC.fields(p) == RC.DONOR and p.kept == [0] and p.n_host_kept == 0 and (p.M, p.D, p.N) == (0, 1, 1)


def test_cameras():
    p = plan([A, B], 2, cameras=[CAM, None])                               # case 12
    assert p.kind == "objects" and RC.fields(p) == RC.CAMERA
    assert list(DT.reproject_record(p, 2).has_view[0:2]) == [1, 0]        # (the view rows are reserved because an edit has one)
    assert p.N == 2 and p.return_instances and p.with_table
    assert p.cams[0] is not None and p.cams[1] is None
    assert int(p.covered.sum()) == 22                                      # bg_valid is its complement
    p = plan([], cameras=[CAM])                                            # case 13
    assert p.kind == "pure_camera" and RC.fields(p) == RC.CAMERA_BACKGROUND and p.N == 0
    assert DT.reproject_record(p, 1).view_surfaces == 0                    # (the background's own carving, nothing for triangles)
    p = plan([E], cameras=[CAM])                                           # case 14
    assert p.kind == "pure_camera" and RC.fields(p) == RC.CAMERA_BACKGROUND and p.N == 1
    p = plan([], cameras=[CAM], removed_masks=[R])
    assert p.kind == "pure_camera" and int(p.covered.sum()) == 6


def test_the_plan_takes_a_shape_for_the_depth():
    p, q = plan([A, E, B]), DT.reproject_plan(tuple(DEPTH.shape), [A, E, B], [[GOOD] * 3])
    assert (q.kind, RC.fields(q), q.kept, q.caller, q.n_pts, q.cap) == (p.kind, RC.fields(p), p.kept, p.caller, p.n_pts, p.cap)


def test_the_refusals_come_from_the_plan_alone():
    with pytest.raises(NotImplementedError, match="reproject_camera_edits: footprints with a camera are not supported"):
        plan([A], cameras=[CAM], footprints=True)
    with pytest.raises(NotImplementedError, match="reproject_donor_edits: footprints with a donor are not supported"):
        plan([A], donor_depth=DEPTH, donor_masks=[DN], footprints=True)
    with pytest.raises(ValueError, match="The foreground masks overlap"):
        plan([A, box(4, 6, 5, 7)])
    with pytest.raises(ValueError, match="Expected 1 to 8 foreground masks, got 9"):
        plan([box(r, r, 0, 0) for r in range(9)])
    with pytest.raises(ValueError, match="Expected 1 to 8 foreground masks, got 0"):
        plan([])
    with pytest.raises(ValueError, match="reproject_removal_edits: edit 0 has 1 transforms, but there is no foreground mask"):
        plan([], n_transforms=1, removed_masks=[R])
    with pytest.raises(ValueError, match="transform_foreground_objects: edit 0 has 1 transforms, but there is no foreground mask"):
        plan([], n_transforms=1, removed_masks=[R], what="transform_foreground_objects")
    with pytest.raises(ValueError, match="reproject_removal_edits: removed_masks: removed mask 0 overlaps foreground mask 0"):
        plan([A], removed_masks=[box(4, 5, 5, 6)])
