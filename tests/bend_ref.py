"""Test-side statement of bend edits ("Bend edits"): linear-blend skinning of the point transform.  NumPy float64,
with float32 where the rule says float32; composed from tests/similarity_ref.py (similarity_transform, full: the arithmetic of
ONE bone, unchanged), tests/camera_moves_ref.py (point list, view, discard, rows), tests/view_surfaces_ref.py (triangles under
a view, the z-buffer over all bids), tests/footprints_ref.py (footprint_bids, infill_share), tests/object_copies_ref.py /
tests/multi_object_ref.py (the rows per target pixel, the scene, the tie counters) and oracle/depth_ref.py, and nothing of the
product.  The reference has no such mode; this file is the yardstick:

    bones      an instance carries B <= 4 transforms, each a 3- or 5-tuple with its own scale and its own pivot (None = the
               centroid of the instance's mask), and a weight image [B, H, W] (f32)
    X_b        similarity_ref.similarity_transform of the f32 point under bone b -> f64
    blend      f64, over b ascending and only over the bones with w_b != 0: acc = w_b0 * X_b0, then acc = acc + w_b * X_b, per
               component; the weights are the f32 values widened.  All weights 0: bone 0 with weight 1
    after it   the view row, the projection, the clamp or the discard, the vertices of footprints and view surfaces and the z
               key act on acc as they act on the one transform's (X, Y, Z)

An instance that is an ordinary tuple is camera_moves_ref.point_list's instance word for word.  `chain_weights` restates the
weights of depth_transform.bend_chain."""
import contextlib

import numpy as np
import torch

import camera_moves_ref as CM
import footprints_ref as F
import multi_object_ref as R
import similarity_ref as S
import view_surfaces_ref as V
from oracle import depth_ref as D

Y = R.Y
MAX_BONES = 4


class Bend:
    """bones: 1 .. 4 transform tuples; weights: [B, H, W], kept as float32."""

    def __init__(self, bones, weights):
        self.bones = [tuple(b) for b in bones]
        self.weights = np.ascontiguousarray(np.asarray(weights, dtype=np.float32))
        assert 1 <= len(self.bones) <= MAX_BONES and self.weights.ndim == 3 and self.weights.shape[0] == len(self.bones)


def one_hot(bones, mask_hw, bone=0):
    """Every pixel's weight 1 on `bone`."""
    w = np.zeros((len(bones),) + tuple(mask_hw.shape), dtype=np.float32)
    w[bone] = 1.0
    return Bend(bones, w)


def bone_points(points_hw3, mask_hw, tf):
    """X_b: the points under one bone -> f64 [H, W, 3]."""
    angle, axis, trans, s, pivot = S.full(tf)
    trans = np.asarray(trans, dtype=np.float32)
    return S.similarity_transform(points_hw3, np.asarray(axis, dtype=np.float32), float(angle), [float(t) for t in trans], mask_hw, s,
                                  pivot)


def blend(points_hw3, mask_hw, bend):
    """The rule of the header for every pixel -> f64 [H, W, 3] (only the pixels of the mask are used)."""
    w = bend.weights.astype(np.float64)
    B = w.shape[0]
    none = np.all(bend.weights == 0, axis=0)
    w[0][none] = 1.0
    acc = np.zeros(points_hw3.shape, dtype=np.float64)
    opened = np.zeros(mask_hw.shape, dtype=bool)
    for b in range(B):
        use = w[b] != 0
        if not use.any():
            continue
        term = w[b][..., None] * bone_points(points_hw3, mask_hw, bend.bones[b])
        first = use & ~opened
        later = use & opened
        acc[first] = term[first]
        acc[later] = acc[later] + term[later]
        opened |= use
    assert opened.all()
    return acc


def point_list(depth, bg_depth, fg_masks, instances, transforms, donor=None, K=None):
    """camera_moves_ref.point_list in which an instance may be a `Bend`."""
    if K is None:
        K = D.intrinsics_f32()
    M = len(fg_masks)
    hs = [m[0, 0].numpy().astype(bool) for m in fg_masks]
    ds = [] if donor is None else [m[0, 0].numpy().astype(bool) for m in donor[1]]
    ms = hs + ds
    assert all(0 <= o < len(ms) for o in instances) and set(range(len(ms))) <= set(instances)
    kept = [n for n, o in enumerate(instances) if ms[o].any()]
    bg_pts = D.unproject(bg_depth[0, 0].numpy(), K)
    host_pts = D.unproject(depth[0, 0].numpy(), K)
    donor_pts = None if donor is None else D.unproject(donor[0][0, 0].numpy(), K)
    blocks, src = [bg_pts.reshape(-1, 3).astype(np.float64)], []
    for n in kept:
        o = instances[n]
        pts = donor_pts if o >= M else host_pts
        tf = transforms[n]
        moved = blend(pts, ms[o], tf) if isinstance(tf, Bend) else bone_points(pts, ms[o], tf)
        blocks.append(moved.reshape(-1, 3)[ms[o].reshape(-1)])
        src.append(np.nonzero(ms[o].reshape(-1))[0])
    start = np.concatenate([[0], np.cumsum([len(s) for s in src])]).astype(np.int64)
    inst_of = np.repeat(np.asarray(kept, dtype=np.int64), [len(s) for s in src])
    src_all = np.concatenate(src) if src else np.zeros(0, dtype=np.int64)
    return np.vstack(blocks), src_all, inst_of, start


@contextlib.contextmanager
def _bent_point_list():
    """camera_moves_ref.transform_camera and view_surfaces_ref.transform_surfaces take their point list from
    camera_moves_ref.point_list: inside this block it is the one above, so everything after the point transform is theirs."""
    before = CM.point_list
    CM.point_list = point_list
    try:
        yield
    finally:
        CM.point_list = before


def _footprint_edit(depth, bg_depth, fg_masks, instances, transforms, max_ratio, K, infill):
    """The footprint branch of object_copies_ref.transform_instances over the bent point list."""
    res = depth.shape[-1]
    R2 = res * res
    all_pts, src_all, inst_of, start = point_list(depth, bg_depth, fg_masks, instances, transforms, None, K)
    n_pts = len(src_all)
    ui, vi = D.project_points(all_pts, K, (res, res))
    u, v = CM.unclamped_uv(all_pts[R2:], K, res)
    fgp = all_pts[R2:]
    pix_f, z_f, who = [], [], []
    with np.errstate(all="ignore"):
        for i in range(len(start) - 1):
            a, b = int(start[i]), int(start[i + 1])
            p, z, w = F.footprint_bids(u[a:b], v[a:b], fgp[a:b, 2], src_all[a:b], np.zeros(b - a, dtype=np.int64),
                                       depth[0, 0].numpy().reshape(-1), res, max_ratio)
            pix_f.append(p), z_f.append(z), who.append(w + a)
    pix = np.concatenate([vi * res + ui] + pix_f)
    z = np.concatenate([all_pts[:, 2]] + z_f)
    idx = np.concatenate([np.arange(R2 + n_pts)] + [R2 + w for w in who])
    zmap, owner = V.winners(pix, z, idx, R2)
    zmap = zmap.reshape(res, res).astype(np.float32)
    raw_mask = (owner >= R2).reshape(res, res)
    vis = np.zeros(n_pts, dtype=bool)
    vis[owner[owner >= R2] - R2] = True
    disparity = D.normalize_depth(1.0 / torch.from_numpy(zmap)[None, None])[0][0, 0].numpy()
    cleaned = D.clean_mask(raw_mask, res)
    ty, tx = np.nonzero(raw_mask & (cleaned == 255))
    j = owner.reshape(res, res)[ty, tx] - R2
    won, winst = src_all[j], inst_of[j]
    corr = np.stack([won % res, won // res, tx, ty], axis=-1).astype(np.int64).reshape(-1, 4)
    inpaint = (cleaned != 0) != raw_mask
    filled = D.harmonic_fill(disparity, inpaint.astype(np.uint8)) if infill else disparity
    out = torch.from_numpy(filled).to(torch.float32)[None, None]
    dbg = dict(zmap=zmap, raw_mask=raw_mask, cleaned=cleaned, vis=vis, tx=ui[R2:], ty=vi[R2:], inpaint=inpaint,
               unowned=np.zeros((res, res), dtype=bool), disparity=disparity, owner=owner, gone=np.zeros(R2 + n_pts, dtype=bool),
               inst_start=start, obj_start=start, corr_inst=winst.astype(np.uint8), n_instance_rows=len(corr), n_background=0,
               points=all_pts)
    return out, torch.from_numpy(corr), dbg


def transform_bend(depth, bg_depth, fg_masks, instances, transforms, camera=None, footprints=False, max_ratio=None,
                   view_surfaces=False, donor=None, K=None, infill=True):
    """One edit; transforms[n] is a tuple or a `Bend`.  Returns what camera_moves_ref.transform_camera returns (dbg["points"]: the
    whole list, background first)."""
    if K is None:
        K = D.intrinsics_f32()
    if footprints:
        assert camera is None and donor is None and not view_surfaces
        return _footprint_edit(depth, bg_depth, fg_masks, list(instances), list(transforms), max_ratio, K, infill)
    with _bent_point_list():
        if view_surfaces and camera is not None:
            assert donor is None
            return V.transform_surfaces(depth, bg_depth, fg_masks, list(instances), list(transforms), camera, (), True, max_ratio,
                                        None, K, infill)
        return CM.transform_camera(depth, bg_depth, fg_masks, list(instances), list(transforms), camera, (), donor, None, K, infill)


def foreground_dbg(dbg, res):
    """The debug dict with "points" cut to the foreground points and obj_start beside them: what
    multi_object_ref.z_ties_between_objects / object_copies_ref.z_ties_between_instances read."""
    pts = dbg["points"][res * res:]
    return dict(dbg, points=pts, obj_start=np.asarray(dbg["inst_start"]))


# ---- depth_transform.bend_chain's weights, restated --------------------------------------------------------------------------
def signed_distance(shape_hw, p0, p1):
    """d of every pixel (x = column, y = row) from the line p0 -> p1: ((x - x0)(y1 - y0) - (y - y0)(x1 - x0)) / |p1 - p0|, f64."""
    h, w = shape_hw
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    (x0, y0), (x1, y1) = (float(p0[0]), float(p0[1])), (float(p1[0]), float(p1[1]))
    return ((xx - x0) * (y1 - y0) - (yy - y0) * (x1 - x0)) / np.hypot(x1 - x0, y1 - y0)


def chain_weights(shape_hw, p0, p1, width, bones):
    """s = clamp(d / width + 0.5, 0, 1) (B - 1); w_b = max(0, 1 - |s - b|) -> f32 [B, H, W]."""
    d = signed_distance(shape_hw, p0, p1)
    s = np.clip(d / float(width) + 0.5, 0.0, 1.0) * (bones - 1)
    return np.stack([np.maximum(0.0, 1.0 - np.abs(s - b)) for b in range(bones)]).astype(np.float32)


def chain(depth, mask, p0, p1, width, rot_angle, rot_axis, translation=(0.0, 0.0, 0.0), pivot=None, bones=2, K=None):
    """bend_chain restated: bone b turns by rot_angle b / (B - 1) about rot_axis through the pivot (default: the point of the
    pixel at the rounded midpoint of p0 p1) and moves by translation b / (B - 1)."""
    if K is None:
        K = D.intrinsics_f32()
    if pivot is None:
        mx, my = int(round((p0[0] + p1[0]) / 2.0)), int(round((p0[1] + p1[1]) / 2.0))
        pivot = tuple(float(v) for v in D.unproject(depth[0, 0].numpy(), K)[my, mx])
    tfs = []
    for b in range(bones):
        tfs.append((float(rot_angle) * b / (bones - 1), tuple(rot_axis), tuple(float(np.float32(t)) * b / (bones - 1) for t in translation),
                    None, tuple(pivot)))
    return Bend(tfs, chain_weights(mask.shape[-2:], p0, p1, width, bones))
