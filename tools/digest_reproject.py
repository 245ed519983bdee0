#!/usr/bin/env python3
"""SHA-256 digests of what the re-projection calls return, one line per returned tensor: the A/B record of a change to the host
side of depth_transform.py (DESIGN.md "One host path for the re-projection"; profiles/reproject_host_path/).
DH_TREE=<checkout> (default: this one) names the tree whose diffusionhandles_amd is imported; DIFFHANDLES_LIB names the library.
The calls are the cases of tests/test_reproject_plan.py that launch, scaled to 128 x 128.  Debug buffers are not digested: past
their counts they are uninitialised."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("DH_TREE") or ROOT)
import numpy as np
import torch
from diffusionhandles_amd import depth_transform as DT

dev = torch.device("cuda:0")
RES = 128


def box(r0, r1, c0, c1):
    m = torch.zeros((1, 1, RES, RES), dtype=torch.float32)
    m[..., r0:r1 + 1, c0:c1 + 1] = 1.0
    return m.to(dev)


A, B, E = box(16, 39, 16, 47), box(64, 79, 64, 103), torch.zeros((1, 1, RES, RES), device=dev)
R, DN = box(96, 111, 8, 31), box(0, 15, 0, 23)
ramp = torch.linspace(0.0, 0.3, RES)[None, None, None, :].expand(1, 1, RES, RES)
bg = (2.0 + ramp).contiguous().to(dev)
depth = torch.where((A + B + R) > 0, bg - 0.6, bg).contiguous()
donor_depth = torch.where(DN > 0, bg - 0.8, bg).contiguous()
f = 1.0 / np.tan(0.5 * 55.0 * (np.pi / 180.0))
intr = torch.tensor([[f, 0, 0], [0, f, 0], [0, 0, 1]], dtype=torch.float32)
Y = torch.tensor([0.0, 1.0, 0.0])
T0, T1, T2 = (10.0, Y, torch.zeros(3)), (-15.0, Y, torch.tensor([0.1, 0.0, 0.05])), (5.0, Y, torch.tensor([0.0, 0.1, 0.0]))
CAM = (5.0, Y, torch.zeros(3))
kw = dict(device_correspondences=True, return_debug=True)
CASES = [
    ("01", lambda: DT.reproject_object_edits(depth, bg, [A], intr, [[T0], [T1]], **kw)),
    ("02", lambda: DT.reproject_object_edits(depth, bg, [A, B], intr, [[T0, T1]], footprints=True, **kw)),
    ("03", lambda: DT.reproject_object_edits(depth, bg, [A, E, B], intr, [[T0, T2, T1]], **kw)),
    ("04", lambda: DT.reproject_instance_edits(depth, bg, [A, B], intr, [[T0, T1, T2]], [1, 0, 1], **kw)),
    ("05", lambda: DT.reproject_instance_edits(depth, bg, [A, E, B], intr, [[T0, T1, T2, T1]], [2, 1, 0, 0], **kw)),
    ("06", lambda: DT.reproject_removal_edits(depth, bg, [A], intr, [[T0]], removed_masks=[R], **kw)),
    ("07", lambda: DT.reproject_removal_edits(depth, bg, [], intr, [[], [], []], removed_masks=[R], **kw)),
    ("08", lambda: DT.reproject_removal_edits(depth, bg, [E], intr, [[T0]], removed_masks=[R], **kw)),
    ("10", lambda: DT.reproject_donor_edits(depth, bg, [A], intr, [[T0, T1]], donor_depth=donor_depth, donor_masks=[DN], **kw)),
    ("11", lambda: DT.reproject_donor_edits(depth, bg, [], intr, [[T1]], donor_depth=donor_depth, donor_masks=[DN], **kw)),
    ("12", lambda: DT.reproject_camera_edits(depth, bg, [A, B], intr, [[T0, T1], [T1, T2]], cameras=[CAM, None], **kw)),
    ("13", lambda: DT.reproject_camera_edits(depth, bg, [], intr, [[]], cameras=[CAM], **kw)),
    ("14", lambda: DT.reproject_camera_edits(depth, bg, [E], intr, [[T0]], cameras=[CAM], **kw)),
]


def sha(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return f"{hashlib.sha256(a.tobytes()).hexdigest()} {a.dtype} {list(a.shape)}"


for name, call in CASES:
    out, dbg = call()
    for e, item in enumerate(out):
        for part, t in zip(("disparity", "correspondences", "instances"), item):
            print(f"case {name} edit {e} {part}: {sha(t)}")
    print(f"case {name} counts: {sha(dbg['counts'])}", flush=True)
