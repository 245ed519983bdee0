"""Test-side statement of object copies ("Object copies"): an edit places N instances, instance n = (mask o_n,
transform n).  Composed from the functions oracle/depth_ref.py exports and the pieces of tests/similarity_ref.py
(similarity_transform, full) and tests/footprints_ref.py (footprint_bids), the way tests/multi_object_ref.py is composed, and
nothing else.  The reference has no such mode; this file is the yardstick:

    point list   background, instance 0's points (row-major), instance 1's, ...; every foreground point flagged
    centroid     oracle.depth_ref.masked_centroid_f32 of the instance's MASK (similarity_transform computes it from the mask, so
                 two instances of one mask turn about the same f32 values)
    z-buffer     oracle.depth_ref.zbuffer: min (z, point index) -- equal depths go to the earlier instance
    rows         point-list order; with footprints per foreground-owned target pixel, row-major in the target
    footprints   footprint_bids once per INSTANCE (a triangle joins points of one instance), the bidder's position moved to the
                 instance's slice of the point list

With the identity table (o_n = n) this is multi_object_ref / similarity_ref / footprints_ref.transform_objects."""
import numpy as np
import torch

import footprints_ref as F
import multi_object_ref as R
import similarity_ref as S
from oracle import depth_ref as D

Y = R.Y
Z0 = (0.0, 0.0, 0.0)
# the sets of the GPU comparison on multi_object_ref.two_spheres: (instances, K edits of N transforms)
SET_A = ([0, 0, 1], [
    [(0.0, Y, Z0), (25.0, Y, (0.0, -0.9, 0.3)), (-30.0, Y, Z0)],
    # the second edit of the call (other transforms: the edit-major rows e * N + n): the copy moves up and is enlarged
    [(10.0, Y, (0.1, 0.0, 0.0)), (-15.0, Y, (0.1, 0.9, 0.2), 1.25, None), (20.0, Y, (0.0, 0.0, 0.1))],
])
SET_B = ([0, 0, 1, 1], [
    [(0.0, Y, Z0), (0.0, Y, (-0.35, 0.0, -0.2)), (0.0, Y, Z0), (40.0, (0.3, 0.9, -0.2), (0.0, 0.8, 0.0))],
])
SET_C = ([0, 0], [[(10.0, Y, Z0), (10.0, Y, Z0)]])          # the tie rule: the later instance gets no pair
# footprints: set A's first edit with instance 1 at uniform scale 2
SET_A_FP = ([0, 0, 1], [[(0.0, Y, Z0), (25.0, Y, (0.0, -0.9, 0.3), 2.0, None), (-30.0, Y, Z0)]])


def transform_instances(depth, bg_depth, fg_masks, instances, transforms, footprints=False, max_ratio=None, K=None, infill=True):
    """One edit.  instances: N mask indices; transforms: N 3- or 5-tuples.  Returns (disparity [1,1,H,W] f32 torch,
    correspondences [R,4] int64 torch, debug dict): what footprints_ref.transform_objects returns, the debug dict also with
    corr_inst [R] (the caller's instance index of every row), inst_start (= obj_start: the slices of the kept instances) and
    inst_kept (their caller's indices); vis / tx / ty have one entry per foreground POINT (tx / ty of every point)."""
    if K is None:
        K = D.intrinsics_f32()
    assert len(transforms) == len(instances)
    res = depth.shape[-1]
    R2 = res * res
    ms = [m[0, 0].numpy().astype(bool) for m in fg_masks]
    assert np.sum(ms, axis=0).max() <= 1, "overlapping masks"
    assert all(0 <= o < len(ms) for o in instances) and set(range(len(ms))) <= set(instances)
    kept = [n for n, o in enumerate(instances) if ms[o].any()]              # empty masks are dropped with all their instances
    assert kept, "all masks empty"
    bg_pts = D.unproject(bg_depth[0, 0].numpy(), K)
    pts = D.unproject(depth[0, 0].numpy(), K)
    blocks, src = [bg_pts.reshape(-1, 3).astype(np.float64)], []
    for n in kept:
        m = ms[instances[n]]
        angle, axis, trans, s, pivot = S.full(transforms[n])
        trans = np.asarray(trans, dtype=np.float32)                          # float32 values, as transform_depth_pc takes them
        moved = S.similarity_transform(pts, np.asarray(axis, dtype=np.float32), float(angle), [float(t) for t in trans], m, s, pivot)
        blocks.append(moved.reshape(-1, 3)[m.reshape(-1)])
        src.append(np.nonzero(m.reshape(-1))[0])
    all_pts = np.vstack(blocks)
    start = np.concatenate([[0], np.cumsum([len(s) for s in src])])
    inst_of = np.repeat(np.asarray(kept, dtype=np.int64), [len(s) for s in src])       # caller's index per point
    src_all = np.concatenate(src)
    n_pts = len(src_all)
    flags = np.zeros(all_pts.shape[0], dtype=np.uint8)
    flags[R2:] = 1
    ui, vi = D.project_points(all_pts, K, (res, res))
    if not footprints:
        assert max_ratio is None
        zmap, raw_mask, tx, ty, vis = D.zbuffer(all_pts, flags, K, (res, res))
        vis = vis[R2:]
        owner = None
    else:
        # the point bids as oracle.depth_ref.zbuffer forms them, the footprint bids per instance
        pix_p, z_p, idx_p = vi * res + ui, all_pts[:, 2], np.arange(R2 + n_pts)
        k = K.numpy().astype(np.float64)
        fgp = all_pts[R2:]
        pix_f, z_f, who = [], [], []
        with np.errstate(all="ignore"):
            u = (((k[0, 0] * -fgp[:, 0]) / fgp[:, 2]) * 0.5 + 0.5) * (res - 1)
            v = (((k[1, 1] * -fgp[:, 1]) / fgp[:, 2]) * 0.5 + 0.5) * (res - 1)
            for i in range(len(kept)):
                a, b = start[i], start[i + 1]
                p, z, w = F.footprint_bids(u[a:b], v[a:b], fgp[a:b, 2], src[i], np.zeros(b - a, dtype=np.int64),
                                           depth[0, 0].numpy().reshape(-1), res, max_ratio)
                pix_f.append(p), z_f.append(z), who.append(w + a)
        pix_f, z_f, who = np.concatenate(pix_f), np.concatenate(z_f), np.concatenate(who)
        pix, z, idx = np.concatenate([pix_p, pix_f]), np.concatenate([z_p, z_f]), np.concatenate([idx_p, R2 + who])
        order = np.lexsort((idx, z, pix))
        first = np.ones(len(order), dtype=bool)
        first[1:] = pix[order][1:] != pix[order][:-1]
        win = order[first]
        zmap = np.full(R2, np.inf)
        zmap[pix[win]] = z[win]
        owner = -np.ones(R2, dtype=np.int64)
        owner[pix[win]] = idx[win]
        zmap = zmap.reshape(res, res).astype(np.float32)
        raw_mask = (owner >= R2).reshape(res, res)
        vis = np.zeros(n_pts, dtype=bool)
        vis[owner[owner >= R2] - R2] = True
    disparity = D.normalize_depth(1.0 / torch.from_numpy(zmap)[None, None])[0][0, 0].numpy()
    cleaned = D.clean_mask(raw_mask, res)
    if not footprints:
        tx, ty = ui[R2:][vis], vi[R2:][vis]
        keep = cleaned[ty, tx] == 255
        won, winst = src_all[vis][keep], inst_of[vis][keep]
        tx, ty = tx[keep], ty[keep]
    else:
        ty, tx = np.nonzero(raw_mask & (cleaned == 255))                     # row-major target order
        j = owner.reshape(res, res)[ty, tx] - R2
        won, winst = src_all[j], inst_of[j]
    corr = np.stack([won % res, won // res, tx, ty], axis=-1).astype(np.int64).reshape(-1, 4)
    inpaint = (cleaned != 0) != raw_mask
    filled = D.harmonic_fill(disparity, inpaint.astype(np.uint8)) if infill else disparity
    out = torch.from_numpy(filled).to(torch.float32)[None, None]
    dbg = dict(zmap=zmap, raw_mask=raw_mask, cleaned=cleaned, vis=vis, obj_start=start, inst_start=start, inst_kept=kept,
               tx=ui[R2:], ty=vi[R2:], inpaint=inpaint, disparity=disparity, points=all_pts[R2:], corr_inst=winst.astype(np.uint8),
               owner=owner)
    return out, torch.from_numpy(corr), dbg


def pairs_per_instance(dbg, n_instances):
    """How many of the correspondences belong to each instance."""
    return np.bincount(dbg["corr_inst"].astype(np.int64), minlength=n_instances).tolist()


def z_ties_between_instances(dbg, res):
    """multi_object_ref.z_ties_between_objects over the instance slices (dbg["obj_start"] holds them)."""
    return R.z_ties_between_objects(dbg, res=res)
