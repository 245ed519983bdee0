"""CPU: several objects per edit -- the test-side reference (tests/multi_object_ref.py) is the one-object oracle when there
is one object, its two-sphere scene exercises what the feature is for (objects that hide each other), the C ABI declares
and exports the two entries, and the argument errors come before any device work."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_object_ref as R  # noqa: E402

from diffusionhandles_amd.synthetic import TRANSFORMS, make_scene  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dh_reproject_objects_workspace_bytes", "dh_reproject_object_edits")


@pytest.mark.parametrize("ti", [2, 6])
def test_one_object_helper_is_the_oracle(ti):
    from oracle import depth_ref as D
    depth, bg, mask = make_scene(256)
    angle, trans = TRANSFORMS[ti]
    disp, corr, dbg = R.transform_objects(depth, bg, [mask], [(angle, R.Y, trans)])
    disp_o, corr_o, dbg_o = D.transform_depth_pc(depth, bg, mask, rot_angle=angle, rot_axis=R.Y, translation=trans,
                                                 return_debug=True)
    assert len(corr_o) > 1000
    assert np.array_equal(corr.numpy(), corr_o.numpy())
    assert np.array_equal(dbg["zmap"], dbg_o["zmap"])
    assert np.array_equal(dbg["cleaned"], dbg_o["cleaned"]) and np.array_equal(dbg["raw_mask"], dbg_o["raw_mask"])
    assert torch.equal(disp, disp_o)


def _visible(res, which, transforms):
    depth, bg, masks = R.two_spheres(res)
    _, corr, dbg = R.transform_objects(depth, bg, [masks[m] for m in which], [transforms[m] for m in which])
    s = dbg["obj_start"]
    return [int(dbg["vis"][s[j]:s[j + 1]].sum()) for j in range(len(which))], corr, dbg, masks


# foreground pixels and visible points measured with this helper when the scene was chosen (res: object 0, object 1,
# object 1 visible alone, object 1 visible behind object 0)
MEASURED = {128: (1252, 952, 722, 191), 256: (5013, 3841, 2855, 795)}


@pytest.mark.parametrize("res", [128, 256])
def test_two_spheres_scene_has_objects_that_hide_each_other(res):
    (v0, v1), corr, dbg, masks = _visible(res, (0, 1), R.OCCLUDING)
    (a0,), _, _, _ = _visible(res, (0,), R.OCCLUDING)
    (a1,), _, _, _ = _visible(res, (1,), R.OCCLUDING)
    m0, m1 = (m[0, 0].numpy() > 0.5 for m in masks)
    assert not (m0 & m1).any() and m0.sum() > 1000 * (res / 128) ** 2 * 0.9 and m1.sum() > 900 * (res / 128) ** 2 * 0.9
    print(f"res {res}: pixels {int(m0.sum())} / {int(m1.sum())}; object 1 visible alone {a1}, with object 0 {v1}; object 0 {a0} / {v0}")
    assert (int(m0.sum()), int(m1.sum()), a1, v1) == MEASURED[res]
    assert v0 == a0 and (res != 128 or a0 == 1043)       # object 0 is in front: it keeps what it shows alone
    assert v1 < a1 / 2                                   # object 1 loses more than half of its points behind object 0
    c = corr.numpy()
    src0, src1 = m0[c[:, 1], c[:, 0]], m1[c[:, 1], c[:, 0]]
    assert src0.sum() > 100 and src1.sum() > 100 and (src0 | src1).all()            # both objects contribute pairs
    n0 = int(src0.sum())
    assert src0[:n0].all() and src1[n0:].all()           # object order, then row-major within each object
    for blk in (c[:n0], c[n0:]):
        assert (np.diff(blk[:, 1] * res + blk[:, 0]) > 0).all()
    assert R.z_ties_between_objects(dbg, res=res) == 0


def test_header_table_and_library_have_the_two_entries():
    from diffusionhandles_amd import _lib
    txt = open(os.path.join(ROOT, "include", "diffhandles_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", txt), f"{name} not declared in the header"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.lib()
    for name in NEW:
        assert name not in lib.dh_missing_symbols and hasattr(lib, name), f"{name} not exported"
    # the argument count of the table is the header's
    decl = re.search(r"dh_reproject_object_edits\s*\((.*?)\)\s*;", txt, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["dh_reproject_object_edits"][1]) == 27


def test_argument_errors_come_before_any_device_work():
    from diffusionhandles_amd import DiffusionHandles
    from diffusionhandles_amd import depth_transform as DT
    depth, bg, masks = R.two_spheres(128)
    K = torch.eye(3)
    tf = (10.0, torch.tensor(R.Y), torch.zeros(3))
    overlapping = [masks[0], torch.roll(masks[0], 5, dims=-1)]
    with pytest.raises(ValueError, match="overlap"):
        DT.reproject_object_edits(depth, bg, overlapping, K, [[tf, tf]])
    nine = []
    for i in range(9):
        m = torch.zeros(1, 1, 128, 128)
        m[0, 0, 10 * i:10 * i + 5, 20:40] = 1.0
        nine.append(m)
    with pytest.raises(ValueError, match="8"):
        DT.reproject_object_edits(depth, bg, nine, K, [[tf] * 9])
    with pytest.raises(ValueError, match="transforms"):
        DT.reproject_object_edits(depth, bg, masks, K, [[tf, tf], [tf]])
    with pytest.raises(ValueError, match="transforms"):
        DT.reproject_object_edits(depth, bg, masks, K, [[tf, tf, tf]])
    with pytest.raises(ValueError):
        DT.reproject_object_edits(depth, bg, [], K, [[]])
    dh = object.__new__(DiffusionHandles)                # no engine: the mode check comes first
    dh.conf = SimpleNamespace(depth_transform_mode="mesh")
    with pytest.raises(NotImplementedError):
        dh.transform_foreground_objects(depth, "two spheres", masks, bg, None, None, None, [tf, tf])
    with pytest.raises(NotImplementedError):
        dh.transform_foreground_objects_batch(depth, "two spheres", masks, bg, None, None, None, [[tf, tf]])
    # and through the facade in 'pc' mode the same ValueErrors
    dh.conf = SimpleNamespace(depth_transform_mode="pc")
    dh.diffuser = SimpleNamespace(get_depth_intrinsics=lambda device=None: K)
    with pytest.raises(ValueError, match="overlap"):
        dh.transform_foreground_objects(depth, "two spheres", overlapping, bg, None, None, None, [tf, tf])
    with pytest.raises(ValueError, match="transforms"):
        dh.transform_foreground_objects_batch(depth, "two spheres", masks, bg, None, None, None, [[tf]])
