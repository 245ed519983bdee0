"""Test-side statement of camera moves ("Camera moves"): an edit may move the viewpoint as well as the objects.
Composed from oracle/depth_ref.py and the pieces of tests/similarity_ref.py (similarity_transform, full),
tests/object_copies_ref.py / tests/object_insertion_ref.py (the point list, the rows, cells) and tests/object_removal_ref.py
(cells, the pure case), the way those files are composed, and nothing else.  The reference has no camera mode; this file is
the yardstick:

    camera       (rot_angle_deg, rot_axis, translation[, pivot]): the CAMERA is turned about rot_axis through pivot (None = the
                 origin, the camera centre), then translated, in the coordinates of depth_to_world_coords
    view row     the inverse motion as a similarity row: f32-normalised axis, cos / sin of -angle, scale 1, the pivot c (f32) or
                 zeros with the has-pivot flag 1, t' = -(t cos + (a x t) sin + a (a . t)(1 - cos)) in f64 from the widened f32
                 values, rounded to f32
    composition  the point list of object_insertion_ref.transform_donor (background, then instance after instance, f64), rounded
                 to f32, through similarity_ref.similarity_transform with the view's angle, axis, translation and pivot
    discard      a point whose rint(u) or rint(v) (half to even, before any clamp) leaves 0 .. res - 1, or whose Z is not > 0,
                 is taken out of the list: no bid, no row, vis 0, target (-1, -1)
    z-buffer     oracle.depth_ref.zbuffer over the remaining points in list order: min (z, list index)
    rows         the instance rows as before (list order, visible, target inside the cleaned mask); then the BACKGROUND rows:
                 background point i (source pixel i) with bg_valid[i], owning its target pixel, that pixel outside the cleaned
                 mask -- ascending i, instance index N, kind 2
    in-fill      (cleaned != raw) | unowned; the disparity is normalised with the min / max over the OWNED pixels
    cells        object_insertion_ref.cells on the rows of kind 0 / 1 for the masks; the pairs are all rows'

An edit without a camera is object_insertion_ref.transform_donor / object_copies_ref.transform_instances word for word (no
discard, the reference's clamp, no background rows)."""
import functools

import numpy as np
import torch

import multi_object_ref as R
import object_insertion_ref as IN
import object_removal_ref as RM
import similarity_ref as S
from oracle import depth_ref as D

Y = R.Y
GRID = 64
CAMERA_NAMES = ("pan", "orbit", "dolly_in", "dolly_out", "truck", "general")


def centre_pivot(depth, K=None):
    """The point of the centre pixel of `depth` [1,1,H,W]: three f32 values."""
    if K is None:
        K = D.intrinsics_f32()
    res = depth.shape[-1]
    p = D.unproject(depth[0, 0].numpy(), K)[res // 2, res // 2]
    return tuple(float(v) for v in np.asarray(p, dtype=np.float32))


def cameras_for(depth):
    """The camera set of the comparison on two_spheres: name -> (rot_angle_deg, rot_axis, translation, pivot)."""
    c = centre_pivot(depth)
    return {
        "pan": (4.0, Y, (0.0, 0.0, 0.0), None),
        "orbit": (8.0, Y, (0.0, 0.0, 0.0), c),
        "dolly_in": (0.0, Y, (0.0, 0.0, 0.3), None),
        "dolly_out": (0.0, Y, (0.0, 0.0, -0.3), None),
        "truck": (0.0, Y, (0.2, 0.05, 0.0), None),
        "general": (6.0, (0.3, 0.9, -0.2), (0.1, -0.05, 0.15), c),
    }


def view_row(camera):
    """Rule 2, stated independently of the product: the 16 doubles of the view row of `camera`."""
    angle, axis, trans = camera[:3]
    pivot = camera[3] if len(camera) == 4 else None
    a = np.asarray(axis, dtype=np.float32)
    a = (a / np.linalg.norm(a)).astype(np.float64)
    t = np.asarray(trans, dtype=np.float32).astype(np.float64)
    th = np.radians(-float(angle))
    c, s = np.cos(th), np.sin(th)
    tp = -(t * c + np.cross(a, t) * s + a * np.dot(a, t) * (1.0 - c))
    row = np.zeros(16, dtype=np.float64)
    row[0:3] = a
    row[3], row[4] = c, s
    row[5:8] = tp.astype(np.float32).astype(np.float64)
    row[8:11] = 1.0
    if pivot is not None:
        row[11:14] = np.asarray(pivot, dtype=np.float32).astype(np.float64)
    row[14] = 1.0
    return row


def camera_move(points_n3, camera):
    """The forward motion, plain f64: a point of the NEW camera's frame in the old frame, P = R (P' - c) + c + t."""
    angle, axis, trans = camera[:3]
    pivot = camera[3] if len(camera) == 4 else None
    a = np.asarray(axis, dtype=np.float32)
    a = (a / np.linalg.norm(a)).astype(np.float64)
    t = np.asarray(trans, dtype=np.float32).astype(np.float64)
    c = np.zeros(3) if pivot is None else np.asarray(pivot, dtype=np.float32).astype(np.float64)
    th = np.radians(float(angle))
    q = np.asarray(points_n3, dtype=np.float64) - c
    r = q * np.cos(th) + np.cross(a, q) * np.sin(th) + a * (q @ a)[:, None] * (1.0 - np.cos(th))
    return r + c + t


def view_apply(points_n3, camera):
    """Rule 3: the points, ROUNDED TO F32, through the view row with the instance row's arithmetic -> f64 [N, 3]."""
    angle, axis, _ = camera[:3]
    row = view_row(camera)
    p = np.asarray(points_n3).astype(np.float32).reshape(-1, 1, 3)
    pivot = row[11:14].astype(np.float32)
    out = S.similarity_transform(p, np.asarray(axis, dtype=np.float32), -float(angle), [float(v) for v in row[5:8]], None, None, pivot)
    return out.reshape(-1, 3)


def unclamped_uv(points_n3, K, res):
    """u, v of oracle.depth_ref.project_points before its clip and rounding (f64)."""
    p = np.asarray(points_n3, dtype=np.float64)
    k = K.numpy().astype(np.float64)
    with np.errstate(all="ignore"):
        u = (((k[0, 0] * -p[:, 0]) / p[:, 2]) * 0.5 + 0.5) * (res - 1)
        v = (((k[1, 1] * -p[:, 1]) / p[:, 2]) * 0.5 + 0.5) * (res - 1)
    return u, v


def discarded(points_n3, K, res):
    """Rule 4: bool [N], the points of a view edit that bid for no pixel."""
    u, v = unclamped_uv(points_n3, K, res)
    with np.errstate(all="ignore"):
        ru, rv = np.rint(u), np.rint(v)
        ok = (ru >= 0) & (ru <= res - 1) & (rv >= 0) & (rv <= res - 1) & (np.asarray(points_n3)[:, 2] > 0)
    return ~ok


def point_list(depth, bg_depth, fg_masks, instances, transforms, donor=None, K=None):
    """The f64 point list of object_insertion_ref.transform_donor before any view: (points [R2 + n_pts, 3], source pixel and
    caller's instance of every foreground point, the slices' starts)."""
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
        angle, axis, trans, s, pivot = S.full(transforms[n])
        trans = np.asarray(trans, dtype=np.float32)
        moved = S.similarity_transform(pts, np.asarray(axis, dtype=np.float32), float(angle), [float(t) for t in trans], ms[o], s, pivot)
        blocks.append(moved.reshape(-1, 3)[ms[o].reshape(-1)])
        src.append(np.nonzero(ms[o].reshape(-1))[0])
    start = np.concatenate([[0], np.cumsum([len(s) for s in src])]).astype(np.int64)
    inst_of = np.repeat(np.asarray(kept, dtype=np.int64), [len(s) for s in src])
    src_all = np.concatenate(src) if src else np.zeros(0, dtype=np.int64)
    return np.vstack(blocks), src_all, inst_of, start


def resolve(all_pts, R2, res, K, view):
    """Discard (view edits), z-buffer, owner map.  Returns a dict: gone [P] bool, ui / vi [P] (-1 where gone), owner [R2] int64
    (list index, -1 = unowned), zmap [res, res] f32 (inf where unowned), raw_mask [res, res] bool."""
    P = all_pts.shape[0]
    gone = discarded(all_pts, K, res) if view else np.zeros(P, dtype=bool)
    idx = np.nonzero(~gone)[0]
    sub = all_pts[idx]
    zmap, _, _, _, win = D.zbuffer(sub, np.ones(len(idx), dtype=np.uint8), K, (res, res))      # every point flagged: win = the winners
    ui_s, vi_s = D.project_points(sub, K, (res, res))
    ui, vi = -np.ones(P, dtype=np.int64), -np.ones(P, dtype=np.int64)
    ui[idx], vi[idx] = ui_s, vi_s
    owner = -np.ones(R2, dtype=np.int64)
    w = idx[win]
    owner[vi[w] * res + ui[w]] = w
    raw_mask = (owner >= R2).reshape(res, res)
    return dict(gone=gone, ui=ui, vi=vi, owner=owner, zmap=zmap, raw_mask=raw_mask)


def transform_camera(depth, bg_depth, fg_masks, instances, transforms, camera, removed_masks=(), donor=None, bounds=None, K=None,
                     infill=True, view_fn=None):
    """One edit with an optional camera (None = no view).  fg_masks: M >= 0 host masks; donor: None or (donor depth, donor masks);
    instances / transforms as object_insertion_ref.transform_donor takes them (empty for the pure case).  Returns (disparity
    [1,1,H,W] f32 torch, correspondences [R + Rb, 4] int64 torch, debug dict): the instance rows, then the background rows.
    view_fn: another statement of the view (the test's plain f64 composition) in place of view_apply."""
    if K is None:
        K = D.intrinsics_f32()
    res = depth.shape[-1]
    R2 = res * res
    M = len(fg_masks)
    N = len(instances)
    all_pts, src_all, inst_of, start = point_list(depth, bg_depth, fg_masks, instances, transforms, donor, K)
    n_pts = len(src_all)
    view = camera is not None
    if view:
        all_pts = view_apply(all_pts, camera) if view_fn is None else view_fn(all_pts, camera)
    r = resolve(all_pts, R2, res, K, view)
    owner, zmap, raw_mask, ui, vi = r["owner"], r["zmap"], r["raw_mask"], r["ui"], r["vi"]
    unowned = (owner < 0).reshape(res, res)
    if view:
        d = 1.0 / torch.from_numpy(zmap)[None, None]
        own = torch.from_numpy(~unowned)[None, None]
        lo_hi = bounds if bounds is not None else (d[own].min(), d[own].max())
        disparity = D.normalize_depth(d, lo_hi)[0][0, 0].numpy()
    else:
        disparity = D.normalize_depth(1.0 / torch.from_numpy(zmap)[None, None], bounds)[0][0, 0].numpy()
    cleaned = D.clean_mask(raw_mask, res)
    # the instance rows: list order, visible, target inside the cleaned mask
    fg_idx = np.arange(R2, R2 + n_pts)
    vis = np.zeros(n_pts, dtype=bool)
    ok = ~r["gone"][R2:]
    vis[ok] = owner[vi[R2:][ok] * res + ui[R2:][ok]] == fg_idx[ok]
    tx, ty = ui[R2:][vis], vi[R2:][vis]
    keep = cleaned[ty, tx] == 255
    won, winst = src_all[vis][keep], inst_of[vis][keep]
    corr_i = np.stack([won % res, won // res, tx[keep], ty[keep]], axis=-1).astype(np.int64).reshape(-1, 4)
    # the background rows (view edits only)
    corr_b = np.zeros((0, 4), dtype=np.int64)
    if view:
        valid = np.ones(R2, dtype=bool)
        for m in list(fg_masks) + list(removed_masks):
            valid &= ~(m[0, 0].numpy() != 0).reshape(-1)
        i = np.arange(R2)
        okb = ~r["gone"][:R2]
        rows = np.zeros(R2, dtype=bool)
        rows[okb] = valid[okb] & (owner[vi[:R2][okb] * res + ui[:R2][okb]] == i[okb]) & (cleaned[vi[:R2][okb], ui[:R2][okb]] == 0)
        b = np.nonzero(rows)[0]
        corr_b = np.stack([b % res, b // res, ui[b], vi[b]], axis=-1).astype(np.int64).reshape(-1, 4)
    corr = np.concatenate([corr_i, corr_b])
    corr_inst = np.concatenate([winst, np.full(len(corr_b), N, dtype=np.int64)]).astype(np.uint8)
    kind = np.concatenate([(np.asarray(instances, dtype=np.int64)[winst] >= M).astype(np.uint8) if len(winst) else np.zeros(0, np.uint8),
                           np.full(len(corr_b), 2, dtype=np.uint8)])
    inpaint = (cleaned != 0) != raw_mask
    if view:
        inpaint = inpaint | unowned
    filled = D.harmonic_fill(disparity, inpaint.astype(np.uint8)) if infill else disparity
    out = torch.from_numpy(filled).to(torch.float32)[None, None]
    dbg = dict(zmap=zmap, raw_mask=raw_mask, cleaned=cleaned, vis=vis, tx=ui[R2:], ty=vi[R2:], inpaint=inpaint, unowned=unowned,
               disparity=disparity, owner=owner, gone=r["gone"], inst_start=start, corr_inst=corr_inst, row_kind=kind,
               n_instance_rows=len(corr_i), n_background=len(corr_b), points=all_pts)
    return out, torch.from_numpy(corr), dbg


def background_camera(bg_depth, camera, removed_masks=(), bounds=None, K=None, infill=True):
    """The pure camera move (rule 9): the background alone under a view; every row is a background row."""
    return transform_camera(bg_depth, bg_depth, [], [], [], camera, removed_masks, None, bounds, K, infill)


def cells(corr, img_res, row_kind=None, vacated=None, bg_erosion=0, grid=GRID):
    """object_insertion_ref.cells in which the rows of kind 2 form their pairs and clear neither mask: the masks and lists are
    those of the rows of kind 0 / 1, the pairs all rows'."""
    corr = np.asarray(corr).reshape(-1, 4)
    if row_kind is None:
        return IN.cells(corr, img_res, None, vacated, bg_erosion, grid)
    kind = np.asarray(row_kind).reshape(-1)
    rest = kind != 2
    out = IN.cells(corr[rest], img_res, (kind[rest] == 1).astype(np.uint8), vacated, bg_erosion, grid)
    allrows = RM.cells(corr, img_res, None, 0, grid)
    for k in ("original_x", "original_y", "transformed_x", "transformed_y"):
        out[k] = allrows[k]
    return out


@functools.lru_cache(maxsize=None)
def fixture(res):
    """two_spheres at `res` with edit 0 of similarity_ref.edits_for, computed once: the scene, the cameras, and the reference
    geometry of every camera (in-fill included) plus the edit without a camera under "none"."""
    depth, bg, masks = R.two_spheres(res)
    tfs = S.edits_for(res, depth)[0]
    cams = cameras_for(depth)
    geo = {name: transform_camera(depth, bg, masks, [0, 1], tfs, cam) for name, cam in cams.items()}
    geo["none"] = transform_camera(depth, bg, masks, [0, 1], tfs, None)
    return dict(depth=depth, bg_depth=bg, masks=masks, transforms=tfs, cameras=cams, geo=geo)
