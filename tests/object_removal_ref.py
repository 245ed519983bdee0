"""Test-side statement of object removal ("Object removal"): an edit deletes the objects of its removed masks.
Composed from oracle/depth_ref.py, oracle/guidance_ref.py and tests/object_copies_ref.py, the way that file is composed, and
nothing else.  The reference has no such mode; this file is the yardstick:

    geometry, M >= 1   a removed object contributes no point: object_copies_ref.transform_instances on the REMAINING masks
    geometry, M = 0    the background alone: oracle.depth_ref.zbuffer over the H * W points of bg_depth (no flag set),
                       normalize_depth of 1 / z with the optional bounds, harmonic_fill of the pixels no point owns
    vacated pixels     the union of the removed masks; a grid cell that holds one is a vacated cell
    cells              oracle.guidance_ref.cells_from_correspondences at erosion 0, the vacated cells cleared from its
                       ORIGINAL mask, then scipy.ndimage.binary_erosion of both masks, the lists rebuilt in its order
    energy             oracle.guidance_ref's two terms on those cells; without pairs the foreground term is absent
"""
import functools

import numpy as np
import scipy.ndimage
import torch

import multi_object_ref as R
import object_copies_ref as C
from oracle import depth_ref as D
from oracle import guidance_ref as G

Y = R.Y
GRID = 64
# two_spheres: sphere 1 (the right one) is removed, sphere 0 moves.  Set A: it moves up, clear of the vacated region;
# set B: it slides to the right, onto the vacated region.  One edit each; the GPU tests add a second edit for K = 2.
SET_A = [(25.0, Y, (0.0, -0.9, 0.3))]
SET_B = [(0.0, Y, (-0.95, 0.0, 0.0))]
SECOND_EDIT = [(-15.0, Y, (0.1, 0.6, 0.2))]
SETS = {"A": SET_A, "B": SET_B}


def vacated_pixels(removed_masks, res):
    """[res, res] bool union of the removed masks (empty masks add nothing)."""
    out = np.zeros((res, res), dtype=bool)
    for m in removed_masks:
        out |= np.asarray(m).reshape(res, res) != 0
    return out


def vacated_cells(vacated, grid=GRID):
    """[grid, grid] bool: the cell holds at least one vacated pixel."""
    res = vacated.shape[-1]
    cs = res // grid
    return vacated.reshape(grid, cs, grid, cs).any(axis=(1, 3))


def cells(corr, img_res, vacated=None, bg_erosion=0, grid=GRID):
    """oracle.guidance_ref.cells_from_correspondences with the vacated cells cleared from the original-background mask before
    the erosion.  vacated: None or [img_res, img_res] bool.  Returns its dict, plus the three masks under "masks"."""
    out = dict(G.cells_from_correspondences(corr, img_res, 0, grid))
    bg_o = np.zeros((grid, grid), dtype=bool)
    bg_t = np.zeros((grid, grid), dtype=bool)
    bg_o[out["background_y_orig"], out["background_x_orig"]] = True
    bg_t[out["background_y_trans"], out["background_x_trans"]] = True
    if vacated is not None:
        bg_o &= ~vacated_cells(np.asarray(vacated) != 0, grid)
    if bg_erosion > 0:
        bg_o = scipy.ndimage.binary_erosion(bg_o, iterations=bg_erosion)
        bg_t = scipy.ndimage.binary_erosion(bg_t, iterations=bg_erosion)
    by, bx = np.nonzero(bg_o & bg_t)
    byo, bxo = np.nonzero(bg_o)
    byt, bxt = np.nonzero(bg_t)
    out.update(background_x=bx, background_y=by, background_x_orig=bxo, background_y_orig=byo,
               background_x_trans=bxt, background_y_trans=byt)
    out["masks"] = np.stack([bg_o & bg_t, bg_o, bg_t]).astype(np.uint8)
    return out


CELL_KEYS = ("original_x", "original_y", "transformed_x", "transformed_y", "background_x", "background_y",
             "background_x_orig", "background_y_orig", "background_x_trans", "background_y_trans")


def remove_objects(depth, bg_depth, fg_masks, removed_masks, transforms, instances=None, **kw):
    """One edit with M >= 1: object_copies_ref.transform_instances on the remaining masks -- the removed masks only have to be
    disjoint from them and from each other."""
    res = depth.shape[-1]
    union = np.zeros((res, res), dtype=np.int64)
    for m in list(fg_masks) + list(removed_masks):
        union += (m[0, 0].numpy() != 0)
    assert union.max() <= 1, "overlapping masks"
    instances = list(range(len(fg_masks))) if instances is None else instances
    return C.transform_instances(depth, bg_depth, fg_masks, instances, transforms, **kw)


def background_alone(bg_depth, K=None, bounds=None, K_unproject=None):
    """The pure removal.  Returns (disparity [1,1,H,W] f32 torch, debug dict with zmap, unowned [H,W] bool and the disparity
    before the in-fill).  bounds: None or (lo, hi) as oracle.depth_ref.normalize_depth takes them.  K_unproject: other
    intrinsics for the un-projection than for the projection (a test's way to leave pixels without an owner; None = K)."""
    if K is None:
        K = D.intrinsics_f32()
    res = bg_depth.shape[-1]
    pts = D.unproject(bg_depth[0, 0].numpy(), K if K_unproject is None else K_unproject).reshape(-1, 3).astype(np.float64)
    zmap, raw_mask, _, _, vis = D.zbuffer(pts, np.zeros(res * res, dtype=np.uint8), K, (res, res))
    assert not raw_mask.any() and not vis.any()
    unowned = np.isinf(zmap)
    disparity = D.normalize_depth(1.0 / torch.from_numpy(zmap)[None, None], bounds)[0][0, 0].numpy()
    filled = D.harmonic_fill(disparity, unowned.astype(np.uint8))
    return torch.from_numpy(filled).to(torch.float32)[None, None], dict(zmap=zmap, unowned=unowned, disparity=disparity)


@functools.lru_cache(maxsize=None)
def fixture(res, which):
    """two_spheres at `res` with sphere 1 removed and sphere 0 moved by set `which` ("A" / "B"), computed once: the scene,
    the reference geometry of the edit (on sphere 0 alone), the vacated image and the reference cells with and without it at
    erosion 0 and 5."""
    depth, bg, masks = R.two_spheres(res)
    tf = SETS[which]
    disp, corr, dbg = remove_objects(depth, bg, [masks[0]], [masks[1]], tf)
    vac = vacated_pixels([masks[1][0, 0].numpy()], res)
    out = dict(depth=depth, bg_depth=bg, masks=masks, transforms=tf, disparity=disp, corr=corr, dbg=dbg, vacated=vac)
    for er in (0, 5):
        out[f"cells{er}"] = cells(corr.numpy(), res, vac, er)
        out[f"plain{er}"] = cells(corr.numpy(), res, None, er)
    return out


def border_blob(res=128):
    """A synthetic vacated blob that touches the image border, with a few correspondences elsewhere (the erosion's
    border_value 0 meets the cleared cells at the border)."""
    vac = np.zeros((res, res), dtype=bool)
    vac[: res // 4, : res // 8] = True                      # the top-left corner, both borders
    vac[res // 2: res // 2 + 3, res - 2:] = True            # a sliver on the right border
    ys, xs = np.meshgrid(np.arange(res // 2, res // 2 + 20), np.arange(res // 3, res // 3 + 20), indexing="ij")
    corr = np.stack([xs.ravel(), ys.ravel(), xs.ravel() + res // 4, ys.ravel() + res // 8], axis=-1).astype(np.int64)
    return vac, corr


def energy_and_grad(act, act_orig, cell_dict, fg_weight, bg_weight, loss_type="global_avg"):
    """float64 reference on [h,w,C] channels-last maps (any float dtype): ((total, fg, bg) floats, gradient [h,w,C] f64);
    the terms are oracle.guidance_ref's, the foreground term 0 without pairs."""
    a = act.detach().double().cpu().permute(2, 0, 1).contiguous().requires_grad_(True)
    o = act_orig.detach().double().cpu().permute(2, 0, 1).contiguous()
    size = tuple(a.shape[-2:])
    bg = G.background_energy(a, o, cell_dict, 1, size, loss_type)
    fg = G.foreground_energy(a, o, cell_dict, 1, size) if len(cell_dict["original_x"]) > 0 else a.sum() * 0.0
    tot = fg_weight * fg + bg_weight * bg
    grad, = torch.autograd.grad(tot, a)
    return (float(tot.detach()), float(fg.detach()), float(bg.detach())), grad.permute(1, 2, 0).contiguous()
