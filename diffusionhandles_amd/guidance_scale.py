"""Power-of-two scale of the guided edit's 16-bit backward ('auto' mode of conf.guided_diffuser.grad_scale).

The guidance energy is L1 (csrc/energy.hip), so the cotangent it writes for a layer is, per activation element,
  -coef_fg * (signed multiplicity sum of the pairs that target the cell) - coef_bg * sign        (patch size 1)
with coef_fg = fg_w / (C n_pairs) (fg_w omega_m / (C N_m) for a pair of object m under object weights), coef_bg = bg_w / (C n_bg_trans) ('global_avg') or bg_w / (C n_bg_both) ('local_avg').
Its largest magnitude is bounded by the weights and the correspondence structure alone: the multiplicity of each target
cell, spread through the masked box filter of a patch size > 1 (k_spread: sum over the window of count / window-weight),
and, for a map smaller than the cell grid, through the adjoint of the bilinear resize (k_store_grad).  No activation value
enters, so the bound is computed on the host once per guidance state, for every (timestep, iteration) of the schedule.

The backward is linear and one pass serves the three layers, so one scale S = 2^e is common to them: e puts
max_k B_k * S into (T/2, T], T = TARGET_AMPLITUDE (tools/probe_guidance_grad.py).  Multiplying every weight by
2^j moves e by exactly -j.
"""
import math

import numpy as np

MODES = ("static", "auto")
# target amplitude of the largest cotangent element: inside the error plateau of the full-size backward, 2^4 and more below
# its overflow (tools/probe_guidance_grad.py, DESIGN.md "Automatic guidance scale")
TARGET_AMPLITUDE = 2.0 ** 4
# covers the f32 arithmetic of the coefficients and the 16-bit rounding of the stored cotangent
_SLACK = 1.0 + 2.0 ** -8
_EXP_LIMIT = 100


def resolve_mode(conf):
    """conf.guided_diffuser-like object -> 'static' | 'auto'; a configuration without the key means 'static'."""
    v = conf.get("grad_scale", None) if hasattr(conf, "get") else getattr(conf, "grad_scale", None)
    v = "static" if v is None else str(v)
    if v not in MODES:
        raise ValueError(f"guided_diffuser.grad_scale must be one of {MODES}, got {v!r}")
    return v


def scale_exponent(bound, target=TARGET_AMPLITUDE):
    """e with bound * 2^e in (target / 2, target] (target a power of two); 0 for bound 0."""
    if not bound > 0.0 or not math.isfinite(bound):
        return 0
    f, m = math.frexp(bound)                     # bound = f 2^m, f in [0.5, 1)
    _, t = math.frexp(target)                    # target = 2^(t - 1)
    e = (t - 1) - m + (1 if f == 0.5 else 0)
    return max(-_EXP_LIMIT, min(_EXP_LIMIT, e))


def _box_sum(a, p):
    """sum over the p x p window centred on every cell, zero outside the grid (avg_pool2d's padding p // 2, times p^2)."""
    if p <= 1:
        return a.copy()
    r = p // 2
    G = a.shape[0]
    pad = np.zeros((G + 2 * r, G + 2 * r), dtype=np.float64)
    pad[r:r + G, r:r + G] = a
    out = np.zeros_like(a, dtype=np.float64)
    for dy in range(p):
        for dx in range(p):
            out += pad[dy:dy + G, dx:dx + G]
    return out


def _pair_map(count, patch):
    """Per cell of the grid: bound of |sum of signs| / coef of one pair term (k_pair_term, with k_pool / k_spread for patch > 1);
    count[t] = number of pairs with target cell t."""
    count = count.astype(np.float64)
    if patch <= 1:
        return count
    w2 = count > 0
    den = _box_sum(w2.astype(np.float64), patch)
    ratio = np.where(w2, count / np.maximum(den, 1.0), 0.0)
    return np.where(w2, _box_sum(ratio, patch), 0.0)


def _bilinear_matrix(n_in, grid):
    """[grid, n_in] weights of k_load_map's 1-D bilinear resize (align_corners False)."""
    M = np.zeros((grid, n_in), dtype=np.float64)
    scale = n_in / grid
    for d in range(grid):
        s = max(scale * (d + 0.5) - 0.5, 0.0)
        i0 = min(int(s), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        l1 = s - i0
        M[d, i0] += 1.0 - l1
        M[d, i1] += l1
    return M


def _to_input(grid_map, h, w):
    """The adjoint of the resize applied to a non-negative grid map (k_store_grad): a bound on the input map."""
    G = grid_map.shape[0]
    if h == G and w == G:
        return grid_map
    return _bilinear_matrix(h, G).T @ grid_map @ _bilinear_matrix(w, G)


def layer_unit_bounds(pc, grid, h, w, C, fg_patch=1, bg_patch=1, bg_loss_type="global_avg", objects=None, omega=None):
    """(U_fg, U_bg): maps [h, w] with |cotangent| <= fg_w U_fg + bg_w U_bg (before the grad scale) for one layer whose
    activation is h x w x C, under the correspondences pc (the dict of process_correspondences).
    objects / omega (a weight per object, losses.object_omegas): the 0-based object of every pair and omega_m; the coefficient
    of a pair of object m is omega_m / (C N_m), so the foreground map is sum_m (omega_m / N_m) cnt_m / C with cnt_m the
    per-cell target counts of object m.  Patch size 1 only (the weighted energy has no pooled form)."""
    G = int(grid)
    tgt = np.asarray(pc["transformed_y"], dtype=np.int64) * G + np.asarray(pc["transformed_x"], dtype=np.int64)
    n_pairs = tgt.size
    zero = np.zeros((G, G))
    fg = zero
    if objects is not None:
        if fg_patch != 1:
            raise NotImplementedError("object weights: fg_patch_size must be 1")
        objects = np.asarray(objects, dtype=np.int64)
        omega = np.asarray(omega, dtype=np.float64)
        if objects.size != n_pairs:
            raise ValueError(f"{objects.size} objects for {n_pairs} pairs")
        acc = np.zeros(G * G, dtype=np.float64)
        for m in range(len(omega)):                      # ascending objects: the kernel's order
            sel = objects == m
            n_m = int(sel.sum())
            if n_m > 0:
                acc += (omega[m] / n_m) * np.bincount(tgt[sel], minlength=G * G)
        fg = acc.reshape(G, G) / C
    elif n_pairs > 0:
        cnt = np.bincount(tgt, minlength=G * G).reshape(G, G)
        fg = _pair_map(cnt, fg_patch) / (C * n_pairs)
    bg = zero
    if bg_loss_type == "global_avg":
        n_o, n_t = len(pc["background_x_orig"]), len(pc["background_x_trans"])
        if n_o > 0 and n_t > 0:
            bg = np.zeros(G * G)
            bg[np.asarray(pc["background_y_trans"], dtype=np.int64) * G + np.asarray(pc["background_x_trans"], dtype=np.int64)] = 1.0
            bg = bg.reshape(G, G) / (C * n_t)
    elif bg_loss_type == "local_avg":
        nb = len(pc["background_x"])
        if nb > 0:
            cb = np.zeros(G * G)
            np.add.at(cb, np.asarray(pc["background_y"], dtype=np.int64) * G + np.asarray(pc["background_x"], dtype=np.int64), 1.0)
            bg = _pair_map(cb.reshape(G, G), bg_patch) / (C * nb)
    else:
        raise ValueError(f"Unknown background loss type: {bg_loss_type}")
    return _to_input(fg, h, w), _to_input(bg, h, w)


def scale_table(pc, grid, shapes, schedule, n_steps, n_iters, max_step, fg_patch=1, bg_patch=1, bg_loss_type="global_avg",
                target=TARGET_AMPLITUDE, objects=None, omega=None):
    """[n_steps, n_iters] float64 table of S (powers of two) for one edit, and the [n_steps, n_iters, 3] bounds B_k behind it.
    shapes: (h, w, C) of the three guided activations; schedule(t_idx, iteration) -> (fg 3-list, bg 3-list).  Entries of
    steps past max_step (no guidance) are 1.  objects / omega: a weight per object (layer_unit_bounds)."""
    units = [layer_unit_bounds(pc, grid, h, w, C, fg_patch, bg_patch, bg_loss_type, objects, omega) for h, w, C in shapes]
    peaks = [(U_fg.ravel(), U_bg.ravel()) for U_fg, U_bg in units]      # fixed maps: only the two weights change per entry
    n_pairs = len(pc["transformed_x"])
    S = np.ones((n_steps, n_iters), dtype=np.float64)
    B = np.zeros((n_steps, n_iters, 3), dtype=np.float64)
    for t in range(min(n_steps, max_step)):
        for it in range(n_iters):
            fgw, bgw = schedule(t, it)
            for k in range(3):
                fw = abs(float(fgw[k])) if n_pairs > 0 else 0.0
                bw = abs(float(bgw[k]))
                if fw == 0.0 and bw == 0.0:
                    continue
                uf, ub = peaks[k]
                B[t, it, k] = float(np.max(fw * uf + bw * ub)) * _SLACK
            S[t, it] = math.ldexp(1.0, scale_exponent(float(B[t, it].max()), target))
    return S, B
