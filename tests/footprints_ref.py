"""Test-side statement of footprint splatting ("Footprint splatting"), in vectorised NumPy float64 on top of
tests/similarity_ref.py and the functions oracle/depth_ref.py exports.  The reference has no such mode; this file is the
yardstick.  Every operation below is one IEEE double operation in the written order (NumPy does not contract):

    vertices   (u, v, Z) of the foreground points, u = ((fx (-X)) / Z * 0.5 + 0.5) (res - 1), unclamped, unrounded
    triangles  per source quad (v10, v11, v01) and (v10, v01, v00), v[row][col]; the three pixels in ONE object's mask;
               dropped for Z <= 0, non-finite u / v, the depth-ratio guard on the f32 source depths, area <= 0
    E(p; a, b) = (px - ax) (by - ay) - (py - ay) (bx - ax);  area = E(v0; v1, v2)
    box        ceil(min u) <= c <= floor(max u) clipped to the image, the same in v; covered = all three E >= 0
    bid        z = (b0 Z0 + b1 Z1) + b2 Z2, b_i = w_i / area;  index = R^2 + fg position of argmax(w0, w1, w2)
    winner     lexicographic minimum of (z, index) over the point bids and the footprint bids of a pixel

With footprints off this is similarity_ref.transform_objects."""
import numpy as np
import torch

import multi_object_ref as R
import similarity_ref as S
from oracle import depth_ref as D

Y = R.Y
# the K = 5 edits of the GPU comparison on multi_object_ref.two_spheres: identity; 1.5 / 0.6; scale 3 with a turn; object 0 towards
# the camera; the rigid occluding edit of the multi-object tests
SCALE3 = [(20.0, Y, (0.2, 0.0, 0.0), 3.0, None), (-30.0, Y, (0.0, 0.0, 0.0))]
IDENTITY = [(0.0, Y, (0.0, 0.0, 0.0)), (0.0, Y, (0.0, 0.0, 0.0))]
EDITS = [
    IDENTITY,
    [(0.0, Y, (0.0, 0.0, 0.0), 1.5, None), (0.0, Y, (0.0, 0.0, 0.0), 0.6, None)],
    SCALE3,
    [(0.0, Y, (0.0, 0.0, -1.6)), (0.0, Y, (0.0, 0.0, 0.0))],
    list(R.OCCLUDING),
]
STEP_TURN = [(40.0, Y, (0.0, 0.0, 0.0))]


def step_scene(res):
    """depth, bg_depth, [mask]: ONE mask over a square whose left half lies at depth 3.0 and whose right half at 2.0, in front
    of the background of synthetic.make_scene.  Turned 40 degrees about Y (STEP_TURN) the step faces the camera and the quads
    across it become long sheets (with the halves the other way round the sheets face away and are dropped: area <= 0)."""
    from diffusionhandles_amd.synthetic import make_scene
    _, bg, _ = make_scene(res)
    a, b, mid = (3 * res) // 10, (7 * res) // 10, res // 2
    m = np.zeros((res, res), dtype=bool)
    m[a:b, a:b] = True
    depth = bg[0, 0].numpy().copy()
    depth[a:b, a:mid] = 3.0
    depth[a:b, mid:b] = 2.0
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).astype(np.float32))[None, None].contiguous()
    return t(depth), bg, [t(m)]


def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def footprint_bids(u, v, z, src, obj, depth_flat, res, max_ratio=None):
    """All footprint bids of one edit.  u, v, z: float64 [n_fg] of the foreground points; src: their source pixels; obj: their
    object.  Returns (pixel, z, fg position of the bidding vertex), one entry per covered candidate."""
    n_fg = len(src)
    inv = -np.ones(res * res, dtype=np.int64)
    inv[src] = np.arange(n_fg)
    g = inv.reshape(res, res)
    v00, v01, v10, v11 = g[:-1, :-1], g[:-1, 1:], g[1:, :-1], g[1:, 1:]
    tri = np.concatenate([np.stack([a.reshape(-1) for a in (v10, v11, v01)], axis=-1),
                          np.stack([a.reshape(-1) for a in (v10, v01, v00)], axis=-1)])
    tri = tri[tri.min(axis=-1) >= 0]
    tri = tri[(obj[tri[:, 0]] == obj[tri[:, 1]]) & (obj[tri[:, 0]] == obj[tri[:, 2]])]
    if max_ratio is not None:
        d = depth_flat[src][tri]                                             # f32 [T, 3], the SOURCE depths
        assert d.dtype == np.float32
        tri = tri[~(d.max(axis=-1) > d.min(axis=-1) * np.float32(max_ratio))]
    U, V, Z = u[tri], v[tri], z[tri]
    ok = (Z > 0).all(axis=-1) & np.isfinite(U).all(axis=-1) & np.isfinite(V).all(axis=-1)
    tri, U, V, Z = tri[ok], U[ok], V[ok], Z[ok]
    area = _edge(U[:, 0], V[:, 0], U[:, 1], V[:, 1], U[:, 2], V[:, 2])
    ok = area > 0
    tri, U, V, Z, area = tri[ok], U[ok], V[ok], Z[ok], area[ok]
    lim = float(res - 1)
    c0, c1 = np.maximum(np.ceil(U.min(axis=-1)), 0.0), np.minimum(np.floor(U.max(axis=-1)), lim)
    r0, r1 = np.maximum(np.ceil(V.min(axis=-1)), 0.0), np.minimum(np.floor(V.max(axis=-1)), lim)
    ok = (c0 <= c1) & (r0 <= r1)
    tri, U, V, Z, area = tri[ok], U[ok], V[ok], Z[ok], area[ok]
    c0, c1, r0, r1 = (a[ok].astype(np.int64) for a in (c0, c1, r0, r1))
    W = c1 - c0 + 1
    n = W * (r1 - r0 + 1)
    t = np.repeat(np.arange(len(tri)), n)                                    # the triangle of every candidate
    k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    c, r = c0[t] + k % W[t], r0[t] + k // W[t]
    px, py = c.astype(np.float64), r.astype(np.float64)
    U, V, Z, area = U[t], V[t], Z[t], area[t]
    w0 = _edge(px, py, U[:, 1], V[:, 1], U[:, 2], V[:, 2])
    w1 = _edge(px, py, U[:, 2], V[:, 2], U[:, 0], V[:, 0])
    w2 = _edge(px, py, U[:, 0], V[:, 0], U[:, 1], V[:, 1])
    cov = (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
    b0, b1, b2 = w0 / area, w1 / area, w2 / area
    zz = (b0 * Z[:, 0] + b1 * Z[:, 1]) + b2 * Z[:, 2]
    who = tri[t, np.argmax(np.stack([w0, w1, w2]), axis=0)]
    return (r * res + c)[cov], zz[cov], who[cov]


def transform_objects(depth, bg_depth, fg_masks, transforms, footprints=False, max_ratio=None, K=None, infill=True):
    """One edit.  What similarity_ref.transform_objects returns (and, with footprints off, its result); with footprints on the
    correspondences are one row per foreground-owned target pixel inside the cleaned mask, row-major in the target, and the
    debug dict also has owner [res*res] (point index, -1 = empty), tx / ty of EVERY foreground point and n_footprint_bids.
    infill=False (footprints on) skips the harmonic in-fill: the disparity returned is the un-filled one."""
    if not footprints:
        assert max_ratio is None
        return S.transform_objects(depth, bg_depth, fg_masks, transforms, K)
    if K is None:
        K = D.intrinsics_f32()
    assert len(transforms) == len(fg_masks)
    res = depth.shape[-1]
    R2 = res * res
    ms = [m[0, 0].numpy().astype(bool) for m in fg_masks]
    assert all(m.any() for m in ms) and np.sum(ms, axis=0).max() <= 1
    bg_pts = D.unproject(bg_depth[0, 0].numpy(), K)
    pts = D.unproject(depth[0, 0].numpy(), K)
    blocks, src = [bg_pts.reshape(-1, 3).astype(np.float64)], []
    for m, tf in zip(ms, transforms):
        angle, axis, trans, s, pivot = S.full(tf)
        trans = np.asarray(trans, dtype=np.float32)
        moved = S.similarity_transform(pts, np.asarray(axis, dtype=np.float32), float(angle), [float(t) for t in trans], m, s, pivot)
        blocks.append(moved.reshape(-1, 3)[m.reshape(-1)])
        src.append(np.nonzero(m.reshape(-1))[0])
    all_pts = np.vstack(blocks)
    obj_start = np.concatenate([[0], np.cumsum([len(s) for s in src])])
    obj = np.repeat(np.arange(len(src)), [len(s) for s in src])
    src = np.concatenate(src)
    n_fg = len(src)
    # the point bids, as oracle.depth_ref.zbuffer forms them
    ui, vi = D.project_points(all_pts, K, (res, res))
    pix_p, z_p, idx_p = vi * res + ui, all_pts[:, 2], np.arange(R2 + n_fg)
    # the footprint bids: the projection of oracle.depth_ref.project_points up to its clip
    k = K.numpy().astype(np.float64)
    fgp = all_pts[R2:]
    with np.errstate(all="ignore"):
        u = (((k[0, 0] * -fgp[:, 0]) / fgp[:, 2]) * 0.5 + 0.5) * (res - 1)
        v = (((k[1, 1] * -fgp[:, 1]) / fgp[:, 2]) * 0.5 + 0.5) * (res - 1)
        pix_f, z_f, who = footprint_bids(u, v, fgp[:, 2], src, obj, depth[0, 0].numpy().reshape(-1), res, max_ratio)
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
    vis = np.zeros(n_fg, dtype=bool)
    vis[owner[owner >= R2] - R2] = True
    disparity = D.normalize_depth(1.0 / torch.from_numpy(zmap)[None, None])[0][0, 0].numpy()
    cleaned = D.clean_mask(raw_mask, res)
    ty, tx = np.nonzero(raw_mask & (cleaned == 255))                         # row-major target order
    won = src[owner.reshape(res, res)[ty, tx] - R2]
    corr = np.stack([won % res, won // res, tx, ty], axis=-1).astype(np.int64).reshape(-1, 4)
    inpaint = (cleaned != 0) != raw_mask
    filled = D.harmonic_fill(disparity, inpaint.astype(np.uint8)) if infill else disparity
    out = torch.from_numpy(filled).to(torch.float32)[None, None]
    dbg = dict(zmap=zmap, raw_mask=raw_mask, cleaned=cleaned, vis=vis, obj_start=obj_start, tx=ui[R2:], ty=vi[R2:], inpaint=inpaint,
               disparity=disparity, points=fgp, owner=owner, n_footprint_bids=len(pix_f))
    return out, torch.from_numpy(corr), dbg


def infill_share(dbg):
    """In-fill pixels as a fraction of the cleaned mask."""
    return float(dbg["inpaint"].sum()) / float((dbg["cleaned"] != 0).sum())
