"""CPU: a weight per object for the guidance energy of multi-object edits -- the cotangent bound of guidance_scale with objects
against the autograd gradient of the test-side reference (tests/object_weights_ref.py), the host-side argument errors of the
facade and of prepare_guidance, the label image and the per-pair objects."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_object_ref as R  # noqa: E402
import object_weights_ref as W  # noqa: E402

from diffusionhandles_amd import guidance_scale as GS  # noqa: E402

FW, BW = 7.5, 1.5


def _bound(cells, C, objects=None, omega=None):
    uf, ub = GS.layer_unit_bounds(cells, W.GRID, W.GRID, W.GRID, C, objects=objects, omega=omega)
    return float(np.max(FW * uf + BW * ub)), uf, ub


# ---- 1. layer_unit_bounds / scale_table with objects ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["occluding", "apart"])
def test_unit_bounds_with_objects_bound_the_reference_gradient(name):
    from diffusionhandles_amd.losses import object_omegas
    _, _, cells, objects = W.scene(name)
    n0, n1 = np.bincount(objects, minlength=2)
    shared = W.target_cells(cells, objects, 0) & W.target_cells(cells, objects, 1)
    if name == "occluding":
        assert 0 < n1 < n0 / 4 and len(shared) >= 1
        assert (int(n0), int(n1), len(shared)) == (4155, 795, 35)
    else:
        assert n0 > 0 and n1 > 0 and not shared
    C = 64
    g = torch.Generator().manual_seed(5)
    act = torch.randn(W.GRID, W.GRID, C, generator=g, dtype=torch.float64)
    orig = torch.randn(W.GRID, W.GRID, C, generator=g, dtype=torch.float64)
    plain, uf_plain, _ = _bound(cells, C)
    for weights in ([1.0, 1.0], [1.0, 0.0], [0.0, 3.0], [0.25, 2.0], [float(n0), float(n1)]):
        counts, omega = object_omegas(objects, weights)
        assert counts.tolist() == [n0, n1] and abs(omega.sum() - 1.0) < 1e-15
        assert np.allclose(omega, W.omegas(objects, weights)[1], rtol=1e-15, atol=0)
        b, uf, ub = _bound(cells, C, objects, omega)
        _, grad = W.energy_and_grad(act, orig, cells, objects, weights, FW, BW)
        peak = float(grad.abs().max())
        print(f"{name} weights {weights}: bound {b:.6e}, largest |gradient| {peak:.6e}")
        assert peak > 0 and peak <= b * (1 + 1e-12)
        # and per element
        assert bool((grad.abs().amax(dim=-1).numpy() <= (FW * uf + BW * ub) * (1 + 1e-12) + 1e-300).all())
        if weights[0] == float(n0) and weights[1] == float(n1):
            assert abs(b - plain) <= 1e-13 * plain and np.allclose(uf, uf_plain, rtol=1e-13, atol=0)
        if weights == [1.0, 1.0] and name == "occluding":
            assert b > plain
            print(f"equal / area-weighted bound: {b / plain:.3f}")


def test_scale_table_with_objects():
    from diffusionhandles_amd.losses import object_omegas
    _, _, cells, objects = W.scene("occluding")
    n0, n1 = np.bincount(objects, minlength=2)
    shapes = [(16, 16, 128), (W.GRID, W.GRID, 64), (W.GRID, W.GRID, 32)]
    sched = lambda t, it: ([0.0, 5.0 * 60, 7.5 * 60], [0.0, 1.5 * 60, 1.5 * 60])
    args = (cells, W.GRID, shapes, sched, 3, 2, 2)
    S0, B0 = GS.scale_table(*args)
    Sn, Bn = GS.scale_table(*args, objects=objects, omega=object_omegas(objects, [float(n0), float(n1)])[1])
    Se, Be = GS.scale_table(*args, objects=objects, omega=object_omegas(objects, [1.0, 1.0])[1])
    assert np.allclose(Bn, B0, rtol=1e-13, atol=0) and np.array_equal(Sn, S0)
    assert (Be[:2, :, 1:] > B0[:2, :, 1:]).all() and (Se[:2] <= S0[:2]).all() and (Se[2] == 1).all()
    for S, B in ((S0, B0), (Se, Be)):
        amp = B[:2].max(axis=-1) * S[:2]
        assert (amp <= GS.TARGET_AMPLITUDE).all() and (amp > GS.TARGET_AMPLITUDE / 2).all()
    with pytest.raises(NotImplementedError):
        GS.layer_unit_bounds(cells, W.GRID, W.GRID, W.GRID, 64, fg_patch=3, objects=objects, omega=[0.5, 0.5])


# ---- 2. argument errors, no GPU --------------------------------------------------------------------------------------------
def _facade():
    from diffusionhandles_amd import DiffusionHandles
    dh = object.__new__(DiffusionHandles)                # no engine: the checks come first
    dh.conf = SimpleNamespace(depth_transform_mode="pc")
    dh.diffuser = SimpleNamespace(get_depth_intrinsics=lambda device=None: torch.eye(3))
    return dh


@pytest.mark.parametrize("bad,match", [([1.0], "entries"), ([1.0, 1.0, 1.0], "entries"), ([1.0, -0.5], "finite"),
                                       ([float("nan"), 1.0], "finite"), ([float("inf"), 1.0], "finite"), ([0.0, 0.0], "zero"),
                                       ("area", "equal"), (2.0, "sequence")])
def test_facade_rejects_bad_object_weights_before_any_device_work(bad, match):
    depth, bg, masks = R.two_spheres(128)
    tf = (10.0, torch.tensor(R.Y), torch.zeros(3))
    dh = _facade()
    with pytest.raises(ValueError, match=match):
        dh.transform_foreground_objects(depth, "two spheres", masks, bg, None, None, None, [tf, tf], object_weights=bad)
    with pytest.raises(ValueError, match=match):
        dh.transform_foreground_objects_batch(depth, "two spheres", masks, bg, None, None, None, [[tf, tf]], object_weights=bad)


def _diffuser(**conf):
    from diffusionhandles_amd.guided_stable_diffuser import GuidedStableDiffuser
    gd = object.__new__(GuidedStableDiffuser)
    gd.conf = SimpleNamespace(**dict(dict(fg_patch_size=1, bg_patch_size=1, bg_loss_type="global_avg", fg_weight=1.0,
                                          bg_weight=1.0), **conf))
    return gd


def test_prepare_guidance_rejects_before_any_device_work():
    acts = [torch.zeros(2, 8, 16, 16), torch.zeros(2, 8, 32, 32), torch.zeros(2, 4, 32, 32)]
    depth = torch.zeros(1, 1, 256, 256)
    corr = torch.zeros((0, 4), dtype=torch.int64)
    label = torch.zeros((256, 256), dtype=torch.uint8)
    call = lambda gd, a=acts, **kw: gd.prepare_guidance(depth, "p", a, corr, **kw)
    with pytest.raises(ValueError, match="object_labels"):
        call(_diffuser(), object_weights="equal")
    with pytest.raises(NotImplementedError, match="bg_loss_type"):
        call(_diffuser(bg_loss_type="local_avg"), object_labels=label, object_weights="equal")
    with pytest.raises(NotImplementedError, match="fg_patch_size"):
        call(_diffuser(fg_patch_size=3), object_labels=label, object_weights=[1.0, 2.0])
    off_grid = [acts[0], torch.zeros(2, 8, 16, 16), acts[2]]
    with pytest.raises(NotImplementedError, match="cell grid"):
        call(_diffuser(), a=off_grid, object_labels=label, object_weights="equal")
    for bad in ([1.0, -1.0], [float("nan"), 1.0], [0.0, 0.0], "area"):
        with pytest.raises(ValueError):
            call(_diffuser(), object_labels=label, object_weights=bad)


def test_omegas_drop_objects_without_pairs():
    from diffusionhandles_amd.losses import object_omegas
    objects = np.array([0, 0, 0, 2, 2], dtype=np.int64)
    counts, omega = object_omegas(objects, [1.0, 5.0, 3.0])
    assert counts.tolist() == [3, 0, 2] and np.allclose(omega, [0.25, 0.0, 0.75], rtol=1e-15)
    with pytest.raises(ValueError, match="positive"):
        object_omegas(objects, [0.0, 5.0, 0.0])
    with pytest.raises(ValueError):
        object_omegas(objects, [1.0, 1.0])                                   # a pair of object 2, two weights
    counts, omega = object_omegas(np.zeros(0, dtype=np.int64), [1.0, 1.0])     # no pairs at all: no foreground term
    assert counts.tolist() == [0, 0] and omega.tolist() == [0.0, 0.0]


# ---- 3. label image and the objects of the oracle's correspondences ------------------------------------------------------------
def test_label_image_and_pair_objects():
    from diffusionhandles_amd.losses import object_label_image
    _, _, masks = R.two_spheres(W.RES)
    label = object_label_image(masks)
    assert label.dtype == torch.uint8 and tuple(label.shape) == (W.RES, W.RES)
    m0, m1 = (m[0, 0] > 0.5 for m in masks)
    assert bool((label[m0] == 1).all()) and bool((label[m1] == 2).all()) and bool((label[~(m0 | m1)] == 0).all())
    assert np.array_equal(label.numpy(), W.label_image([m.numpy() for m in masks]))
    assert torch.equal(object_label_image([masks[1], torch.zeros_like(masks[0]), masks[0]]),
                       torch.where(label == 1, 3, torch.where(label == 2, 1, 0)).to(torch.uint8))
    with pytest.raises(ValueError, match="overlaps"):
        object_label_image([masks[0], torch.roll(masks[0], 5, dims=-1)])
    with pytest.raises(ValueError):
        object_label_image([masks[0]] * 0)
    corr, lab, cells, objects = W.scene("occluding")
    assert len(corr) == 4950 and (np.diff(objects) >= 0).all()               # object order, as reproject_object_edits emits it
    assert np.bincount(objects).tolist() == [4155, 795]
    c = corr.numpy()
    assert np.array_equal(objects, label.numpy()[c[:, 1], c[:, 0]].astype(np.int64) - 1)
