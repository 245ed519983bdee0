"""NumPy float32 statements of the background lock's rules (test-side reference; the product's are dh_keep_map and
dh_ddim_cfg_step_locked, include/diffhandles_hip.h)."""
import numpy as np


def region_cells(corr, mask, release, res, s):
    """bool [s,s]: the cells an edit touches.  corr: [N,4] integers (ox, oy, tx, ty) or None; mask / release: [res,res] or None."""
    cs = res // s
    region = np.zeros((s, s), dtype=bool)
    for img in (mask, release):
        if img is not None:
            a = np.asarray(img).reshape(res, res) != 0
            region |= a.reshape(s, cs, s, cs).any(axis=(1, 3))
    if corr is not None:
        for ox, oy, tx, ty in np.asarray(corr, dtype=np.int64).reshape(-1, 4):
            region[oy // cs, ox // cs] = True              # the source pixel always lies in the image
            if 0 <= tx < res and 0 <= ty < res:            # a target outside the image marks nothing
                region[ty // cs, tx // cs] = True
    return region


def keep_from_region(region, dilate, feather):
    """float32 [s,s]: d = Chebyshev distance in cells to the nearest region cell within dilate + feather + 1 cells (the
    window clipped by the border); 0 for d <= dilate, min(1, float32(d - dilate) / float32(feather + 1)) beyond, 1 where the
    window holds no region cell."""
    s = region.shape[0]
    R = dilate + feather + 1
    keep = np.ones((s, s), dtype=np.float32)
    for y in range(s):
        for x in range(s):
            win = region[max(y - R, 0):y + R + 1, max(x - R, 0):x + R + 1]
            if not win.any():
                continue
            yy, xx = np.nonzero(win)
            d = int(np.maximum(np.abs(yy + max(y - R, 0) - y), np.abs(xx + max(x - R, 0) - x)).min())
            if d <= dilate:
                keep[y, x] = 0.0
            else:
                keep[y, x] = min(np.float32(1.0), np.float32(d - dilate) / np.float32(feather + 1))
    return keep


def keep_map(corr, mask, release, res, s, dilate, feather):
    return keep_from_region(region_cells(corr, mask, release, res, s), dilate, feather)


def ddim_cfg(x, eu, ec, scale, alpha_t, alpha_prev):
    """float32 statement of dh_ddim_cfg_step (for the fractional cells' bound only: the kernels are compared bitwise with
    each other, not with this)."""
    f = np.float32
    sa_t, s1a_t = np.sqrt(f(alpha_t)), np.sqrt(f(1.0) - f(alpha_t))
    sa_p, s1a_p = np.sqrt(f(alpha_prev)), np.sqrt(f(1.0) - f(alpha_prev))
    e = eu + f(scale) * (ec - eu)
    x0 = (x - s1a_t * e) / sa_t
    return (sa_p * x0 + s1a_p * e).astype(np.float32)


def blend(o, r, keep):
    """float32: o where keep == 0, r where keep == 1, o + keep (r - o) in between (unfused).  keep broadcasts over o."""
    o, r = np.asarray(o, dtype=np.float32), np.asarray(r, dtype=np.float32)
    k = np.broadcast_to(np.asarray(keep, dtype=np.float32), o.shape)
    with np.errstate(invalid="ignore"):
        mid = (o + k * (r - o)).astype(np.float32)
    return np.where(k <= 0, o, np.where(k >= 1, r, mid)).astype(np.float32)


def composite(edited, original, keep_up):
    """edited + keep (original - edited) with keep already at the images' resolution."""
    return (edited + keep_up * (original - edited)).astype(np.float32)
