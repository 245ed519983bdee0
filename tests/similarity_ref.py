"""Test-side statement of the similarity edits ("Scale and pivot"): scale per camera axis and pivot of an
object transform, the formulas of include/diffhandles_hip.h written out in NumPy --

    q  = fl32(P - c)            c = the pivot, or the sequential f32 centroid of the object's masked points
    q' = fl32(q * s)            one f32 multiply per component, before the rotation
    f32 cross products and the f32 dot (q'0 a0 + q'1 a1) + q'2 a2, f64 combination with cos / sin / (1 - cos),
    (r + (double)c) + t

-- and everything else from the functions oracle/depth_ref.py exports, composed as tests/multi_object_ref.py composes
them.  The dot product is ALWAYS the written-out order (oracle.depth_ref.DOT_ORDER = "explicit"): for the Y axis it is the
BLAS result too.  tests/test_similarity_ref.py ties this file to oracle.depth_ref.rigid_transform at scale 1."""
import numpy as np
import torch

from oracle import depth_ref as D


def full(tf):
    """(angle, axis, translation[, scale, pivot]) -> the 5-tuple with scale as f32[3] and pivot as None or f32[3]."""
    angle, axis, trans = tf[:3]
    scale, pivot = (tf[3], tf[4]) if len(tf) == 5 else (None, None)
    if scale is None:
        scale = 1.0
    s = np.asarray(scale, dtype=np.float32).reshape(-1)
    s = np.repeat(s, 3) if s.size == 1 else s
    assert s.shape == (3,)
    if pivot is not None:
        pivot = np.asarray(pivot, dtype=np.float32).reshape(3)
    return angle, axis, trans, s, pivot


def similarity_transform(points_hw3, axis, angle_deg, translation, mask_hw, scale=None, pivot=None):
    """oracle.depth_ref.rigid_transform with q scaled before the rotation and an optional pivot -> float64 [H,W,3]."""
    _, _, _, s, pivot = full((angle_deg, axis, translation, scale, pivot))
    p = np.asarray(points_hw3, dtype=np.float32)
    h, w, _ = p.shape
    ax = np.asarray(axis, dtype=np.float32)
    ax = ax / np.linalg.norm(ax)
    theta = np.radians(angle_deg)
    c, sn = np.cos(theta), np.sin(theta)
    cen = D.masked_centroid_f32(p, mask_hw) if pivot is None else pivot
    assert cen.dtype == np.float32
    q = (p - cen).reshape(-1, 3)                      # f32
    q = q * s[None, :]                                # f32 * f32 -> f32, one rounding per component
    assert q.dtype == np.float32
    t1 = q * c                                        # f64
    cr = np.empty_like(q)
    cr[:, 0] = ax[1] * q[:, 2] - ax[2] * q[:, 1]
    cr[:, 1] = ax[2] * q[:, 0] - ax[0] * q[:, 2]
    cr[:, 2] = ax[0] * q[:, 1] - ax[1] * q[:, 0]
    t2 = cr * sn                                      # f64
    d = (q[:, 0] * ax[0] + q[:, 1] * ax[1]) + q[:, 2] * ax[2]           # f32, the written-out order
    t3 = ax * d[:, None] * (1 - c)                    # f32 * f32 -> f32, then f64
    tr = np.array([translation[0], translation[1], translation[2]], dtype=np.float64)
    return (t1 + t2 + t3).reshape(h, w, 3) + cen + tr


def transform_objects(depth, bg_depth, fg_masks, transforms, K=None):
    """One edit: transforms[m], a 3- or 5-tuple, moves the points of fg_masks[m] (no mask empty).  What
    multi_object_ref.transform_objects returns, with similarity_transform in place of the rigid one."""
    if K is None:
        K = D.intrinsics_f32()
    assert len(transforms) == len(fg_masks)
    res = depth.shape[-1]
    ms = [m[0, 0].numpy().astype(bool) for m in fg_masks]
    assert all(m.any() for m in ms) and np.sum(ms, axis=0).max() <= 1
    bg_pts = D.unproject(bg_depth[0, 0].numpy(), K)
    pts = D.unproject(depth[0, 0].numpy(), K)
    blocks, src = [bg_pts.reshape(-1, 3).astype(np.float64)], []
    for m, tf in zip(ms, transforms):
        angle, axis, trans, s, pivot = full(tf)
        trans = np.asarray(trans, dtype=np.float32)                      # float32 values, as transform_depth_pc takes them
        moved = similarity_transform(pts, np.asarray(axis, dtype=np.float32), float(angle), [float(t) for t in trans], m, s, pivot)
        blocks.append(moved.reshape(-1, 3)[m.reshape(-1)])
        src.append(np.nonzero(m.reshape(-1))[0])
    all_pts = np.vstack(blocks)
    obj_start = np.concatenate([[0], np.cumsum([len(s) for s in src])])
    src = np.concatenate(src)
    flags = np.zeros(all_pts.shape[0], dtype=np.uint8)
    flags[res * res:] = 1
    zmap, raw_mask, tx, ty, vis = D.zbuffer(all_pts, flags, K, (res, res))
    disparity = D.normalize_depth(1.0 / torch.from_numpy(zmap)[None, None])[0][0, 0].numpy()
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


def pairs_per_object(corr, fg_masks):
    """How many of the correspondences start in each mask."""
    c = corr.numpy()
    return [int((m[0, 0].numpy() > 0.5)[c[:, 1], c[:, 0]].sum()) for m in fg_masks]


def lower_edge_pixel(res, sphere=1):
    """(x, y) of a pixel at the lower edge of sphere `sphere` of multi_object_ref.two_spheres(res), inside its mask."""
    import multi_object_ref as R
    cx, cy, rad, _ = R.SPHERES[sphere]
    s = res / 512.0
    return int(cx * s), int((cy + rad) * s) - 1


def edits_for(res, depth):
    """The K = 4 edits of the GPU comparison on two_spheres(res), two objects each: all scale 1; uniform 1.5 / 0.6; per-axis
    scale with a turn about a general axis on object 0; object 1 turning 40 degrees about a pivot at its lower edge."""
    import multi_object_ref as R
    x, y = lower_edge_pixel(res)
    pivot = D.unproject(depth[0, 0].numpy())[y, x]
    assert pivot.dtype == np.float32
    Y = R.Y
    return [
        [(15.0, Y, (0.1, 0.0, -0.05), None, None), (-20.0, Y, (-0.15, 0.05, 0.1))],
        [(0.0, Y, (-0.1, 0.0, 0.0), 1.5, None), (10.0, Y, (0.1, 0.0, 0.0), 0.6, None)],
        [(25.0, (0.3, 0.9, -0.2), (0.1, -0.05, 0.2), (1.3, 0.8, 1.0), None), (-20.0, Y, (-0.15, 0.05, 0.1), None, None)],
        [(0.0, Y, (0.0, 0.0, 0.0)), (40.0, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0), None, tuple(float(v) for v in pivot))],
    ]
