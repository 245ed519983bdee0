"""Test-side statement of the multi-object re-projection ("Several objects per edit"), composed from the
functions oracle/depth_ref.py exports and nothing else: unproject, rigid_transform per object, np.vstack, zbuffer,
clean_mask, normalize_depth, harmonic_fill.  The reference has no such mode; with one object this is
oracle.depth_ref.transform_depth_pc line by line.  Also the two-sphere scene the tests and tools/bench_reproject.py use."""
import numpy as np
import torch

from oracle import depth_ref as D

Y = (0.0, 1.0, 0.0)
# (cx, cy, rad, z0) at res 512; scaled by res / 512
SPHERES = ((170.0, 256.0, 80.0, 2.6), (350.0, 270.0, 70.0, 3.1))
# object 0 slides in front of object 1, which turns in place: object 0 hides most of object 1
OCCLUDING = [(0.0, Y, (-0.8, 0.0, 0.0)), (-30.0, Y, (0.0, 0.0, 0.0))]


def two_spheres(res=512):
    """depth, bg_depth [1,1,res,res] f32 and the two masks: the background of synthetic.make_scene with two spheres
    of depth z0 - 0.5 sqrt(1 - r^2) in front of it, masks r^2 < 1."""
    from diffusionhandles_amd.synthetic import make_scene
    _, bg, _ = make_scene(res)
    yy, xx = np.meshgrid(np.arange(res, dtype=np.float64), np.arange(res, dtype=np.float64), indexing="ij")
    depth = bg[0, 0].numpy().astype(np.float64)
    masks = []
    s = res / 512.0
    for cx, cy, rad, z0 in SPHERES:
        r2 = ((yy - cy * s) ** 2 + (xx - cx * s) ** 2) / ((rad * s) ** 2)
        m = r2 < 1.0
        depth = np.where(m, z0 - 0.5 * np.sqrt(np.clip(1.0 - r2, 0.0, None)), depth)
        masks.append(m)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.float32))[None, None].contiguous()
    return t(depth), bg, [t(m) for m in masks]


def transform_objects(depth, bg_depth, fg_masks, transforms, K=None, use_input_depth_normalization=False):
    """One edit: transforms[m] = (angle_deg, axis, translation) moves the points of fg_masks[m].
    Returns (disparity [1,1,H,W] f32 torch, correspondences [N,4] int64 torch, debug dict)."""
    if K is None:
        K = D.intrinsics_f32()
    assert len(transforms) == len(fg_masks)
    bounds = None
    if use_input_depth_normalization:
        _, bounds = D.normalize_depth(1.0 / depth)
    pairs = [(m[0, 0].numpy().astype(bool), tf) for m, tf in zip(fg_masks, transforms)]
    pairs = [(m, tf) for m, tf in pairs if m.any()]                      # empty masks are dropped
    if not pairs:
        return D.normalize_depth(1.0 / depth, bounds)[0], torch.zeros((0, 4), dtype=torch.int64), {}
    res = depth.shape[-1]
    total = np.zeros((res, res), dtype=np.int64)
    for m, _ in pairs:
        total += m
    assert total.max() <= 1, "overlapping masks"
    bg_pts = D.unproject(bg_depth[0, 0].numpy(), K)
    pts = D.unproject(depth[0, 0].numpy(), K)
    blocks, src = [bg_pts.reshape(-1, 3).astype(np.float64)], []
    for m, (angle, axis, trans) in pairs:
        trans = np.asarray(trans, dtype=np.float32)                      # float32 values, as transform_depth_pc takes them
        moved = D.rigid_transform(pts, np.asarray(axis, dtype=np.float32), float(angle), [float(t) for t in trans], m)
        blocks.append(moved.reshape(-1, 3)[m.reshape(-1)])
        src.append(np.nonzero(m.reshape(-1))[0])
    all_pts = np.vstack(blocks)
    obj_start = np.concatenate([[0], np.cumsum([len(s) for s in src])])
    src = np.concatenate(src)
    flags = np.zeros(all_pts.shape[0], dtype=np.uint8)
    flags[res * res:] = 1
    zmap, raw_mask, tx, ty, vis = D.zbuffer(all_pts, flags, K, (res, res))
    disparity = D.normalize_depth(1.0 / torch.from_numpy(zmap)[None, None], bounds)[0][0, 0].numpy()
    won = src[vis[res * res:]]
    oy, ox = won // res, won % res
    cleaned = D.clean_mask(raw_mask, res)
    keep = cleaned[ty, tx] == 255
    corr = np.stack([ox[keep], oy[keep], tx[keep], ty[keep]], axis=-1).astype(np.int64).reshape(-1, 4)
    inpaint = (cleaned != 0) != raw_mask
    filled = D.harmonic_fill(disparity, inpaint.astype(np.uint8))
    out = torch.from_numpy(filled).to(torch.float32)[None, None]
    dbg = dict(zmap=zmap, raw_mask=raw_mask, cleaned=cleaned, vis=vis[res * res:], obj_start=obj_start, tx=tx, ty=ty,
               inpaint=inpaint, disparity=disparity, points=all_pts[res * res:])
    return out, torch.from_numpy(corr), dbg


def z_ties_between_objects(dbg, K=None, res=None):
    """Number of pixels where points of two different objects project with exactly the same depth (where the result
    would depend on the object order)."""
    if K is None:
        K = D.intrinsics_f32()
    pts, start = dbg["points"], dbg["obj_start"]
    ui, vi = D.project_points(pts, K, (res, res))
    obj = np.searchsorted(start, np.arange(len(pts)), side="right") - 1
    order = np.lexsort((pts[:, 2], vi * res + ui))
    pix, z, o = (vi * res + ui)[order], pts[order, 2], obj[order]
    same = (pix[1:] == pix[:-1]) & (z[1:] == z[:-1]) & (o[1:] != o[:-1])
    return int(same.sum())
