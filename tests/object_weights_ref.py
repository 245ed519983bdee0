"""Test-side statement of the guidance energy with a weight per object ("A weight per object"), composed from
oracle.guidance_ref functions alone:

    E = fw * sum_m omega_m * foreground_energy(a, o, cells_m, 1, size) + bw * background_energy(a, o, cells, 1, size)

cells_m is the union's dict with the four pair arrays restricted to object m, omega_m = w_m / (sum of w_j over the objects that
have pairs); the gradient comes from torch autograd.  Also the two edits of multi_object_ref.two_spheres(256) the tests use, at
grid 32, computed once per process."""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_object_ref as R  # noqa: E402

from oracle import guidance_ref as G  # noqa: E402

RES, GRID = 256, 32
PAIR_KEYS = ("original_x", "original_y", "transformed_x", "transformed_y")
# object 0 slides in front of object 1 (they share target cells) / the two move apart (they share none)
EDITS = {"occluding": R.OCCLUDING,
         "apart": [(10.0, R.Y, (-0.1, 0.0, 0.0)), (-30.0, R.Y, (0.15, 0.0, 0.0))]}


def label_image(masks):
    """[H, W] uint8: 0 outside every mask, m + 1 inside mask m (numpy statement of losses.object_label_image)."""
    lab = np.zeros(masks[0].shape[-2:], dtype=np.uint8)
    for m, mask in enumerate(masks):
        inside = np.asarray(mask).reshape(lab.shape) != 0
        assert not lab[inside].any(), "overlapping masks"
        lab[inside] = m + 1
    return lab


@functools.lru_cache(maxsize=None)
def scene(name):
    """corr [N,4] int64 torch, label [H,W] uint8 numpy, cells (the oracle's dict at grid 32), objects [n] int64 (0-based, per
    kept pair) of the edit EDITS[name] of the two-sphere scene at 256 pixels."""
    depth, bg, masks = R.two_spheres(RES)
    _, corr, _ = R.transform_objects(depth, bg, masks, EDITS[name])
    label = label_image([m.numpy() for m in masks])
    c = corr.numpy()
    ok = (c[:, 2] >= 0) & (c[:, 2] < RES) & (c[:, 3] >= 0) & (c[:, 3] < RES)
    cells = G.cells_from_correspondences(c, RES, 0, grid=GRID)
    objects = label[c[ok, 1], c[ok, 0]].astype(np.int64) - 1
    assert objects.size == cells["original_x"].size and objects.min() >= 0
    return corr, label, cells, objects


def target_cells(cells, objects, m, grid=GRID):
    sel = objects == m
    return set((cells["transformed_y"][sel] * grid + cells["transformed_x"][sel]).tolist())


def cells_of_object(cells, objects, m):
    out = dict(cells)
    for k in PAIR_KEYS:
        out[k] = cells[k][objects == m]
    return out


def omegas(objects, weights):
    counts = np.bincount(objects, minlength=len(weights))
    live = counts > 0
    total = sum(float(w) for w, l in zip(weights, live) if l)
    return counts, [float(w) / total if l else 0.0 for w, l in zip(weights, live)]


def energy(act, act_orig, cells, objects, weights, fw, bw, size=(GRID, GRID)):
    """(total, fg, bg) torch scalars; act / act_orig [C,h,w].  A term whose lists are empty is 0 (the product skips it)."""
    zero = act.sum() * 0.0
    fg = zero
    if objects.size:
        _, om = omegas(objects, weights)
        for m, o in enumerate(om):
            if o > 0.0:
                fg = fg + o * G.foreground_energy(act, act_orig, cells_of_object(cells, objects, m), 1, size)
    bg = zero
    if len(cells["background_x_orig"]) and len(cells["background_x_trans"]):
        bg = G.background_energy(act, act_orig, cells, 1, size)
    return fw * fg + bw * bg, fg, bg


def energy_and_grad(act, act_orig, cells, objects, weights, fw, bw):
    """float64 reference on [h,w,C] channels-last maps (any float dtype): ((total, fg, bg) floats, gradient [h,w,C] f64)."""
    a = act.detach().double().cpu().permute(2, 0, 1).contiguous().requires_grad_(True)
    o = act_orig.detach().double().cpu().permute(2, 0, 1).contiguous()
    tot, fg, bg = energy(a, o, cells, objects, weights, fw, bw)
    grad, = torch.autograd.grad(tot, a, allow_unused=True)
    grad = torch.zeros_like(a) if grad is None else grad
    return (float(tot.detach()), float(fg.detach()), float(bg.detach())), grad.permute(1, 2, 0).contiguous()
