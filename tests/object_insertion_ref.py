"""Test-side statement of object insertion ("Object insertion"): an edit places objects of ANOTHER image, the donor.
Composed from oracle/depth_ref.py, oracle/guidance_ref.py, tests/object_copies_ref.py (through tests/similarity_ref.py's
similarity_transform, which it is built on), tests/object_removal_ref.py's cells and tests/object_weights_ref.py, the way
tests/object_removal_ref.py is composed, and nothing else.  The reference has no such mode; this file is the yardstick:

    object list  the host's M masks (0 .. M - 1), then the donor's D masks (M .. M + D - 1)
    points       mask m < M: oracle.depth_ref.unproject of the HOST depth at the mask's pixels; m >= M: of the DONOR depth
    centroid     oracle.depth_ref.masked_centroid_f32 of those points (similarity_transform computes it from points and mask)
    the rest     object_copies_ref.transform_instances' statements, word for word: the point list (background, instance after
                 instance), oracle.depth_ref.zbuffer (min (z, point index)), clean_mask, the kept rows in point-list order,
                 normalize_depth, harmonic_fill
    rows         a row of a donor instance carries its source pixel in the donor image; row_donor = instances[corr_inst] >= M
    cells        object_removal_ref.cells, in which a donor row does not clear its source cell from the ORIGINAL mask
    energy       object_weights_ref.energy with the source features of object m read from the donor's map when m is a donor's

With a donor mask that shares no pixel with a host mask this is object_copies_ref.transform_instances on the composite depth
where(donor_mask, donor_depth, depth) with the masks concatenated (tests/test_object_insertion_ref.py pins that)."""
import functools

import numpy as np
import scipy.ndimage
import torch

import multi_object_ref as R
import object_copies_ref as C
import object_removal_ref as RM
import object_weights_ref as W
import similarity_ref as S
from oracle import depth_ref as D
from oracle import guidance_ref as G

Y = R.Y
GRID = 64
# the donor scene: another background and one sphere of another radius and depth, (cx, cy, rad, z0) at res 512.  "overlap": its
# pixels overlap host sphere 0's (the composite depth cannot express that); "disjoint": they share no pixel with a host mask.
DONOR_SPHERES = {"overlap": (230.0, 200.0, 50.0, 2.2), "disjoint": (256.0, 110.0, 45.0, 2.2)}
# instances: host sphere 0, host sphere 1, the donor sphere.  The donor sphere is shrunk and turned about a pivot and set down
# at the lower left; the second edit of a K = 2 call moves everything differently and enlarges the donor.
INSTANCES = [0, 1, 2]


def donor_scene(res, which):
    """donor depth [1,1,res,res] f32 and its one mask."""
    cx, cy, rad, z0 = DONOR_SPHERES[which]
    s = res / 512.0
    yy, xx = np.meshgrid(np.arange(res, dtype=np.float64), np.arange(res, dtype=np.float64), indexing="ij")
    depth = 5.0 + 1.0 * xx / res
    r2 = ((yy - cy * s) ** 2 + (xx - cx * s) ** 2) / ((rad * s) ** 2)
    m = r2 < 1.0
    depth = np.where(m, z0 - 0.4 * np.sqrt(np.clip(1.0 - r2, 0.0, None)), depth)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.float32))[None, None].contiguous()
    return t(depth), [t(m)]


def donor_pivot(donor_depth, which, K=None):
    """A pivot in the shared camera coordinates: the donor's point at the centre pixel of its sphere (three f32 values)."""
    if K is None:
        K = D.intrinsics_f32()
    res = donor_depth.shape[-1]
    cx, cy, _, _ = DONOR_SPHERES[which]
    p = D.unproject(donor_depth[0, 0].numpy(), K)[int(cy * res / 512.0), int(cx * res / 512.0)]
    return tuple(float(v) for v in np.asarray(p, dtype=np.float32))


def edits_for(donor_depth, which):
    """The K = 2 edits of the GPU comparison (the first alone for K = 1): three transforms each, the donor's scaled and pivoted."""
    pv = donor_pivot(donor_depth, which)
    return [
        [(0.0, Y, (0.0, 0.0, 0.0)), (-30.0, Y, (0.0, 0.0, 0.0)), (20.0, Y, (0.45, 0.55, 0.2), 0.8, pv)],
        [(10.0, Y, (0.1, 0.0, 0.0)), (20.0, Y, (0.0, 0.0, 0.1)), (-15.0, (0.3, 0.9, -0.2), (-0.3, 0.5, 0.4), 1.2, pv)],
    ]


def transform_donor(depth, bg_depth, fg_masks, donor_depth, donor_masks, instances, transforms, K=None, infill=True):
    """One edit.  fg_masks: M >= 0 host masks; donor_masks: D >= 1 masks of the donor image; instances: N indices into the
    concatenated list; transforms: N 3- or 5-tuples.  Returns what object_copies_ref.transform_instances returns (no footprints),
    the debug dict also with row_donor [R] uint8."""
    if K is None:
        K = D.intrinsics_f32()
    assert len(transforms) == len(instances)
    res = depth.shape[-1]
    R2 = res * res
    M = len(fg_masks)
    hs = [m[0, 0].numpy().astype(bool) for m in fg_masks]
    ds = [m[0, 0].numpy().astype(bool) for m in donor_masks]
    assert not hs or np.sum(hs, axis=0).max() <= 1, "overlapping host masks"
    assert np.sum(ds, axis=0).max() <= 1, "overlapping donor masks"
    assert all(m.any() for m in ds), "empty donor mask"
    ms = hs + ds
    assert all(0 <= o < len(ms) for o in instances) and set(range(len(ms))) <= set(instances)
    kept = [n for n, o in enumerate(instances) if ms[o].any()]
    bg_pts = D.unproject(bg_depth[0, 0].numpy(), K)
    host_pts = D.unproject(depth[0, 0].numpy(), K)
    donor_pts = D.unproject(donor_depth[0, 0].numpy(), K)
    blocks, src = [bg_pts.reshape(-1, 3).astype(np.float64)], []
    for n in kept:
        o = instances[n]
        m = ms[o]
        pts = donor_pts if o >= M else host_pts
        angle, axis, trans, s, pivot = S.full(transforms[n])
        trans = np.asarray(trans, dtype=np.float32)
        moved = S.similarity_transform(pts, np.asarray(axis, dtype=np.float32), float(angle), [float(t) for t in trans], m, s, pivot)
        blocks.append(moved.reshape(-1, 3)[m.reshape(-1)])
        src.append(np.nonzero(m.reshape(-1))[0])
    all_pts = np.vstack(blocks)
    start = np.concatenate([[0], np.cumsum([len(s) for s in src])])
    inst_of = np.repeat(np.asarray(kept, dtype=np.int64), [len(s) for s in src])
    src_all = np.concatenate(src)
    flags = np.zeros(all_pts.shape[0], dtype=np.uint8)
    flags[R2:] = 1
    ui, vi = D.project_points(all_pts, K, (res, res))
    zmap, raw_mask, tx, ty, vis = D.zbuffer(all_pts, flags, K, (res, res))
    vis = vis[R2:]
    disparity = D.normalize_depth(1.0 / torch.from_numpy(zmap)[None, None])[0][0, 0].numpy()
    cleaned = D.clean_mask(raw_mask, res)
    tx, ty = ui[R2:][vis], vi[R2:][vis]
    keep = cleaned[ty, tx] == 255
    won, winst = src_all[vis][keep], inst_of[vis][keep]
    tx, ty = tx[keep], ty[keep]
    corr = np.stack([won % res, won // res, tx, ty], axis=-1).astype(np.int64).reshape(-1, 4)
    inpaint = (cleaned != 0) != raw_mask
    filled = D.harmonic_fill(disparity, inpaint.astype(np.uint8)) if infill else disparity
    out = torch.from_numpy(filled).to(torch.float32)[None, None]
    row_donor = (np.asarray(instances, dtype=np.int64)[winst] >= M).astype(np.uint8)
    dbg = dict(zmap=zmap, raw_mask=raw_mask, cleaned=cleaned, vis=vis, obj_start=start, inst_start=start, inst_kept=kept,
               tx=ui[R2:], ty=vi[R2:], inpaint=inpaint, disparity=disparity, points=all_pts[R2:], corr_inst=winst.astype(np.uint8),
               row_donor=row_donor)
    return out, torch.from_numpy(corr), dbg


def composite(depth, fg_masks, donor_depth, donor_masks):
    """The one-image statement of a donor whose masks share no pixel with a host mask: the donor's depth pasted into the host's
    under the donor masks, and the masks concatenated."""
    union = np.zeros(depth.shape[-2:], dtype=bool)
    for m in donor_masks:
        union |= m[0, 0].numpy() != 0
    for m in fg_masks:
        assert not (union & (m[0, 0].numpy() != 0)).any(), "a donor mask shares a pixel with a host mask"
    pasted = torch.where(torch.from_numpy(union)[None, None], donor_depth, depth)
    return pasted, list(fg_masks) + list(donor_masks)


def cells(corr, img_res, row_donor=None, vacated=None, bg_erosion=0, grid=GRID):
    """object_removal_ref.cells in which the rows flagged in row_donor do not clear their source cell from the
    original-background mask: the original mask is that of the UNFLAGGED rows, the pairs and the transformed mask are all rows'."""
    corr = np.asarray(corr).reshape(-1, 4)
    out = RM.cells(corr, img_res, vacated, 0, grid)
    if row_donor is not None and np.asarray(row_donor).any():
        host = RM.cells(corr[np.asarray(row_donor) == 0], img_res, vacated, 0, grid)
        bg_o = host["masks"][1].astype(bool)
        bg_t = out["masks"][2].astype(bool)
    else:
        bg_o, bg_t = out["masks"][1].astype(bool), out["masks"][2].astype(bool)
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


def kept_rows(corr, img_res):
    """The validity test of the cells (a target inside the image): which rows form a pair."""
    c = np.asarray(corr).reshape(-1, 4)
    return (c[:, 2] >= 0) & (c[:, 2] < img_res) & (c[:, 3] >= 0) & (c[:, 3] < img_res)


def energy_and_grad(act, act_orig, act_donor, cell_dict, objects, donor_objects, weights, fw, bw, size):
    """float64 reference on [h,w,C] channels-last maps: ((total, fg, bg) floats, gradient [h,w,C] f64).  The foreground term of
    object m is object_weights_ref's with omega_m, its source features read from act_donor when m is in donor_objects and from
    act_orig otherwise; the background term is oracle.guidance_ref's on act_orig.  weights None: w_m = N_m."""
    a = act.detach().double().cpu().permute(2, 0, 1).contiguous().requires_grad_(True)
    o = act_orig.detach().double().cpu().permute(2, 0, 1).contiguous()
    dn = act_donor.detach().double().cpu().permute(2, 0, 1).contiguous()
    objects = np.asarray(objects, dtype=np.int64)
    n_obj = int(objects.max()) + 1 if weights is None else len(weights)
    if weights is None:
        weights = [float(c) for c in np.bincount(objects, minlength=n_obj)]
    zero = a.sum() * 0.0
    fg = zero
    if objects.size:
        _, om = W.omegas(objects, weights)
        for m, w in enumerate(om):
            if w > 0.0:
                fg = fg + w * G.foreground_energy(a, dn if m in donor_objects else o, W.cells_of_object(cell_dict, objects, m), 1, size)
    bg = zero
    if len(cell_dict["background_x_orig"]) and len(cell_dict["background_x_trans"]):
        bg = G.background_energy(a, o, cell_dict, 1, size)
    tot = fw * fg + bw * bg
    grad, = torch.autograd.grad(tot, a, allow_unused=True)
    grad = torch.zeros_like(a) if grad is None else grad
    return (float(tot.detach()), float(fg.detach()), float(bg.detach())), grad.permute(1, 2, 0).contiguous()


@functools.lru_cache(maxsize=None)
def fixture(res, which, pure=False):
    """two_spheres at `res` as the host with the donor scene `which`, computed once: the scenes, the K = 2 edits, the reference
    geometry of both edits, and the reference cells of the first at erosion 0 and 5 with and without the donor flags.
    pure: the pure insertion (no host mask; bg_depth is the host depth, the donor's transforms alone)."""
    depth, bg, masks = R.two_spheres(res)
    ddepth, dmasks = donor_scene(res, which)
    edits = edits_for(ddepth, which)
    instances = INSTANCES
    if pure:
        masks, bg, instances = [], depth, [0]
        edits = [tfs[2:] for tfs in edits]
    geo = [transform_donor(depth, bg, masks, ddepth, dmasks, instances, tfs) for tfs in edits]
    out = dict(depth=depth, bg_depth=bg, masks=masks, donor_depth=ddepth, donor_masks=dmasks, instances=instances, edits=edits,
               geo=geo)
    corr, flags = geo[0][1].numpy(), geo[0][2]["row_donor"]
    for er in (0, 5):
        out[f"cells{er}"] = cells(corr, res, flags, None, er)
        out[f"plain{er}"] = cells(corr, res, None, None, er)
    return out
