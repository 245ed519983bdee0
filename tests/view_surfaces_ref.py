"""Test-side statement of view surfaces ("View surfaces"): under a camera move the whole scene is splatted as
triangles.  NumPy float64, composed from tests/camera_moves_ref.py (point list, view, discard), tests/footprints_ref.py
(footprint_bids: the triangle arithmetic), tests/similarity_ref.py and oracle/depth_ref.py, and nothing of the product.  The
reference has no such mode; this file is the yardstick.

    scope      the setting acts only in an edit that has a camera; every other edit is camera_moves_ref.transform_camera
    points     bid as a camera move's points do: view row, discard out of frame, no clamp; index = list position
    vertices   (u, v, Z) of EVERY point of the list after the view, unclamped, unrounded (a discarded point is still a vertex)
    instances  footprints_ref.footprint_bids per instance: three source pixels of ONE instance, the ratio guard on the f32 values
               of `depth`, index = R^2 + point-list position of the vertex with the largest weight
    background footprints_ref.footprint_bids over the whole image as one object (src = arange(R^2)): both triangles of every
               source quad, vertices the background points (under the masks too, where bg_depth is in-painted), the ratio guard
               on the f32 values of `bg_depth`, index = the source pixel of the vertex with the largest weight
    winner     lexicographic minimum of (z, index) over all bids of a pixel
    outputs    zmap, masks, disparity, unowned rule and in-fill as a camera move's; vis[j] = point j owns a pixel; target_xy[j]
               the point's own pixel or (-1, -1); instance rows one per instance-owned target pixel inside the cleaned mask,
               background rows one per target pixel outside it whose owner o < R^2 has bg_valid[o]: (o % res, o / res, tx, ty);
               both in row-major target order"""
import functools

import numpy as np
import torch

import camera_moves_ref as CM
import footprints_ref as F
import multi_object_ref as R
import similarity_ref as S
from oracle import depth_ref as D

Y = R.Y
DOLLY_IN_1 = (0.0, Y, (0.0, 0.0, 1.0), None)          # not in camera_moves_ref's set: the camera a whole unit closer
STEP_TRUCK = (0.0, Y, (0.3, 0.0, 0.0), None)          # the cameras of the stepped background
STEP_DOLLY = (0.0, Y, (0.0, 0.0, 0.5), None)


def surface_bids(all_pts, src_all, start, depth, bg_depth, res, K, max_ratio=None):
    """All triangle bids of one view edit -> (pixel, z, list index).  all_pts: the list AFTER the view; start: the slices of the
    instances in its foreground part."""
    R2 = res * res
    u, v = CM.unclamped_uv(all_pts, K, res)
    z = np.asarray(all_pts, dtype=np.float64)[:, 2]
    pix, zz, idx = [], [], []
    with np.errstate(all="ignore"):
        for k in range(len(start) - 1):
            a, b = R2 + int(start[k]), R2 + int(start[k + 1])
            src = src_all[a - R2:b - R2]
            p, q, who = F.footprint_bids(u[a:b], v[a:b], z[a:b], src, np.zeros(len(src), dtype=np.int64),
                                         depth[0, 0].numpy().reshape(-1), res, max_ratio)
            pix.append(p), zz.append(q), idx.append(a + who)
        p, q, who = F.footprint_bids(u[:R2], v[:R2], z[:R2], np.arange(R2), np.zeros(R2, dtype=np.int64),
                                     bg_depth[0, 0].numpy().reshape(-1), res, max_ratio)
        pix.append(p), zz.append(q), idx.append(who)
    return np.concatenate(pix), np.concatenate(zz), np.concatenate(idx)


def winners(pix, z, idx, R2):
    """The z-buffer over all bids: per pixel the lexicographic minimum of (z, index) -> (z [R2] f64, inf where no bid; owner [R2]
    int64, -1 where no bid)."""
    order = np.lexsort((idx, z, pix))
    first = np.ones(len(order), dtype=bool)
    first[1:] = pix[order][1:] != pix[order][:-1]
    win = order[first]
    zmap = np.full(R2, np.inf)
    zmap[pix[win]] = z[win]
    owner = -np.ones(R2, dtype=np.int64)
    owner[pix[win]] = idx[win]
    return zmap, owner


def transform_surfaces(depth, bg_depth, fg_masks, instances, transforms, camera, removed_masks=(), view_surfaces=False,
                       max_ratio=None, bounds=None, K=None, infill=True):
    """One edit.  What camera_moves_ref.transform_camera returns (and, with the setting off or without a camera, its result)."""
    if not view_surfaces:
        assert max_ratio is None
    if not view_surfaces or camera is None:
        return CM.transform_camera(depth, bg_depth, fg_masks, instances, transforms, camera, removed_masks, None, bounds, K, infill)
    if K is None:
        K = D.intrinsics_f32()
    res = depth.shape[-1]
    R2 = res * res
    M, N = len(fg_masks), len(instances)
    all_pts, src_all, inst_of, start = CM.point_list(depth, bg_depth, fg_masks, instances, transforms, None, K)
    n_pts = len(src_all)
    all_pts = CM.view_apply(all_pts, camera)
    # the point bids: the points that stay in the frame, at their rounded pixel
    gone = CM.discarded(all_pts, K, res)
    idx_p = np.nonzero(~gone)[0]
    ui_s, vi_s = D.project_points(all_pts[idx_p], K, (res, res))
    ui, vi = -np.ones(R2 + n_pts, dtype=np.int64), -np.ones(R2 + n_pts, dtype=np.int64)
    ui[idx_p], vi[idx_p] = ui_s, vi_s
    pix_t, z_t, idx_t = surface_bids(all_pts, src_all, start, depth, bg_depth, res, K, max_ratio)
    pix = np.concatenate([vi_s * res + ui_s, pix_t])
    z = np.concatenate([all_pts[idx_p, 2], z_t])
    idx = np.concatenate([idx_p, idx_t])
    zmap, owner = winners(pix, z, idx, R2)
    zmap = zmap.reshape(res, res).astype(np.float32)
    raw_mask = (owner >= R2).reshape(res, res)
    unowned = (owner < 0).reshape(res, res)
    d = 1.0 / torch.from_numpy(zmap)[None, None]
    own = torch.from_numpy(~unowned)[None, None]
    lo_hi = bounds if bounds is not None else (d[own].min(), d[own].max())
    disparity = D.normalize_depth(d, lo_hi)[0][0, 0].numpy()
    cleaned = D.clean_mask(raw_mask, res)
    vis = np.zeros(n_pts, dtype=bool)
    vis[owner[owner >= R2] - R2] = True
    o2 = owner.reshape(res, res)
    # the instance rows: per instance-owned target pixel inside the cleaned mask, row-major
    ty, tx = np.nonzero(raw_mask & (cleaned == 255))
    j = o2[ty, tx] - R2
    won, winst = src_all[j], inst_of[j]
    corr_i = np.stack([won % res, won // res, tx, ty], axis=-1).astype(np.int64).reshape(-1, 4)
    # the background rows: per target pixel outside the cleaned mask whose owner shows the background, row-major
    valid = np.ones(R2, dtype=bool)
    for m in list(fg_masks) + list(removed_masks):
        valid &= ~(m[0, 0].numpy() != 0).reshape(-1)
    bg_owned = (o2 >= 0) & (o2 < R2)
    rows = bg_owned & (cleaned == 0)
    rows[rows] = valid[o2[rows]]
    by, bx = np.nonzero(rows)
    b = o2[by, bx]
    corr_b = np.stack([b % res, b // res, bx, by], axis=-1).astype(np.int64).reshape(-1, 4)
    corr = np.concatenate([corr_i, corr_b])
    corr_inst = np.concatenate([winst, np.full(len(corr_b), N, dtype=np.int64)]).astype(np.uint8)
    kind = np.concatenate([(np.asarray(instances, dtype=np.int64)[winst] >= M).astype(np.uint8) if len(winst) else np.zeros(0, np.uint8),
                           np.full(len(corr_b), 2, dtype=np.uint8)])
    inpaint = ((cleaned != 0) != raw_mask) | unowned
    filled = D.harmonic_fill(disparity, inpaint.astype(np.uint8)) if infill else disparity
    out = torch.from_numpy(filled).to(torch.float32)[None, None]
    dbg = dict(zmap=zmap, raw_mask=raw_mask, cleaned=cleaned, vis=vis, tx=ui[R2:], ty=vi[R2:], inpaint=inpaint, unowned=unowned,
               disparity=disparity, owner=owner, gone=gone, inst_start=start, corr_inst=corr_inst, row_kind=kind,
               n_instance_rows=len(corr_i), n_background=len(corr_b), points=all_pts, n_triangle_bids=len(pix_t))
    return out, torch.from_numpy(corr), dbg


def background_surfaces(bg_depth, camera, removed_masks=(), view_surfaces=True, max_ratio=None, bounds=None, K=None, infill=True):
    """The pure camera move with the setting: the background sheet alone; every row is a background row."""
    return transform_surfaces(bg_depth, bg_depth, [], [], [], camera, removed_masks, view_surfaces, max_ratio, bounds, K, infill)


def step_background(res):
    """The second fixture: a background alone, its left half at depth 4, its right half at depth 3 -- a depth step that the sheet
    bridges unless the ratio guard cuts it."""
    d = np.full((res, res), 4.0, dtype=np.float32)
    d[:, res // 2:] = 3.0
    return torch.from_numpy(d)[None, None].contiguous()


def cameras_for(depth):
    """camera_moves_ref's six cameras and the dolly in by 1.0, in the order of the K = 8 comparison (its last edit has no camera)."""
    cams = dict(CM.cameras_for(depth))
    cams["dolly_in_1"] = DOLLY_IN_1
    return cams


@functools.lru_cache(maxsize=None)
def fixture(res, instances=(0, 1), removed=False, infill=True):
    """two_spheres at `res` with edit 0 of similarity_ref.edits_for, computed once: per camera (and "none") the geometry with
    the setting.  instances: the instance table (the transform of a copy is its mask's); removed: sphere 1 is deleted (its
    mask becomes a removed mask, bg_depth has it removed already)."""
    depth, bg, masks = R.two_spheres(res)
    tfs = S.edits_for(res, depth)[0]
    cams = cameras_for(depth)
    rem = ()
    if removed:
        depth = torch.where(masks[1] != 0, bg, depth)
        masks, rem, tfs, instances = masks[:1], (masks[1],), tfs[:1], (0,)
    inst = list(instances)
    tf_n = [tfs[o] for o in inst]
    if len(inst) > len(set(inst)):          # a copy: the second instance of a mask moves a little further
        seen = set()
        for n, o in enumerate(inst):
            if o in seen:
                a, ax, t = tf_n[n][:3]
                tf_n[n] = (a, ax, (t[0] - 0.5, t[1] + 0.2, t[2])) + tuple(tf_n[n][3:])
            seen.add(o)
    geo = {name: transform_surfaces(depth, bg, masks, inst, tf_n, cam, rem, True, None, infill=infill) for name, cam in cams.items()}
    geo["none"] = transform_surfaces(depth, bg, masks, inst, tf_n, None, rem, True, None, infill=infill)
    return dict(depth=depth, bg_depth=bg, masks=masks, removed=rem, instances=inst, transforms=tf_n, cameras=cams, geo=geo)
