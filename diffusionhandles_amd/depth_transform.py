"""Depth re-projection behind the reference's `transform_depth` API.

Mirrors /root/reference/diffhandles/depth_transform.py:73-89 (`transform_depth`),
:198-363 (`transform_depth_pc`), :15-28 (`normalize_depth`), :589-641
(`depth_to_world_coords`).  All arithmetic runs in the HIP library
(csrc/geometry.hip) through the C ABI; PyTorch only owns the device buffers.
`reproject` is the batched form (K edits of one image in one launch sequence) that the
reference does not have: `reproject_plan` decides everything on the host, `reproject_record` turns
the plan into the one argument record of the C call (dh_reproject_args), `_run_plan` allocates and
launches (DESIGN.md "One host path for the re-projection", "One record for the re-projection");
`reproject_edits` .. `reproject_border_edits` are that call under the names and parameter lists they
grew up with.
"""
import ctypes
import types

import numpy as np
import torch

from . import _lib


def normalize_depth(depth, bounds=None, return_bounds=False):
    """255 * (d - min) / (max - min) per sample (depth_transform.py:15-28)."""
    if depth.dim() != 4:
        raise RuntimeError(f"Expected depth to have 4 dimensions, got {depth.dim()}")
    if bounds is None:
        flat = depth.reshape(depth.shape[0], -1)
        hi = flat.max(dim=-1).values[..., None, None, None]
        lo = flat.min(dim=-1).values[..., None, None, None]
    else:
        lo, hi = bounds
    out = 255 * (depth - lo) / (hi - lo)
    return (out, (lo, hi)) if return_bounds else out


_GRID_CACHE = {}


def _grids(h, w, device):
    key = (h, w, str(device))
    if key not in _GRID_CACHE:
        m = max(h, w) - 1
        gx = torch.linspace(-(w - 1) / m, (w - 1) / m, steps=w, dtype=torch.float32)   # host values, see DESIGN.md
        gy = torch.linspace(-(h - 1) / m, (h - 1) / m, steps=h, dtype=torch.float32)
        _GRID_CACHE[key] = (gx.to(device), gy.to(device))
    return _GRID_CACHE[key]


def _compute_device(t):
    if t.is_cuda:
        return t.device
    _lib.require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


def _inv_focal(intrinsics):
    kinv = torch.linalg.inv(intrinsics.detach().to("cpu", torch.float32))
    return float(kinv[0, 0]), float(kinv[1, 1])


def depth_to_world_coords(depth, intrinsics, extrinsics_R=None, extrinsics_t=None):
    """[1,1,H,W] depth -> [H,W,3] float32 points (depth_transform.py:589-641)."""
    if depth.shape[0] != 1:
        raise ValueError("Only batch size 1 is supported")
    if extrinsics_R is not None or extrinsics_t is not None:
        raise NotImplementedError("only identity extrinsics are on the hot path")
    h, w = depth.shape[-2:]
    if h < 2 or w < 2:
        raise RuntimeError(f"Expected depth to have at least 2 pixels in each dimension, got {h} x {w}.")
    if h != w:
        raise RuntimeError("square depth maps only")
    dev = _compute_device(depth)
    d = depth.detach().to(dev, torch.float32).contiguous()
    gx, gy = _grids(h, w, dev)
    ifx, ify = _inv_focal(intrinsics)
    pts = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    L = _lib.lib()
    _lib.check(L.dh_unproject(_lib.ptr(d), h, _lib.ptr(gx), _lib.ptr(gy), ifx, ify, _lib.ptr(pts), _lib.stream_ptr()),
               "dh_unproject")
    return pts.to(depth.device)


def _f32_list(v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().reshape(-1).tolist()
    elif isinstance(v, np.ndarray):
        v = v.reshape(-1).tolist()
    return [float(np.float32(x)) for x in v]


def check_transform(tf, what="transform"):
    """One object transform, (rot_angle_deg, rot_axis[3], translation[3]) or (rot_angle_deg, rot_axis[3], translation[3],
    scale, pivot) -> the 5-tuple with scale as three float32 values and pivot as None or three float32 values.
    scale: None (= 1), one positive number or three (sx, sy, sz) along the camera axes of `depth_to_world_coords`;
    pivot: None (= the centroid of the object's masked points) or a point in the coordinates `depth_to_world_coords`
    returns.  ValueError naming `what` for another tuple length, a scale that is not positive and finite as float32, a
    pivot that is not three finite numbers.  Host only: no device work."""
    try:
        n = len(tf)
    except TypeError:
        n = -1
    if n not in (3, 5):
        raise ValueError(f"{what}: expected (rot_angle, rot_axis, translation) or (rot_angle, rot_axis, translation, scale, "
                         f"pivot), got {n if n >= 0 else 'no'} members")
    angle, axis, trans = tf[0], tf[1], tf[2]
    scale, pivot = (tf[3], tf[4]) if n == 5 else (None, None)
    if scale is None and pivot is None:          # the rigid transform: nothing to check
        return angle, axis, trans, [1.0, 1.0, 1.0], None
    if scale is None:
        sc = [1.0, 1.0, 1.0]
    else:
        try:
            with np.errstate(over="ignore"):
                sc = _f32_list(scale) if isinstance(scale, (list, tuple, np.ndarray, torch.Tensor)) else [float(np.float32(scale))] * 3
        except (TypeError, ValueError):
            raise ValueError(f"{what}: scale must be one number or three, got {scale!r}") from None
        if len(sc) == 1:
            sc = sc * 3
        if len(sc) != 3:
            raise ValueError(f"{what}: scale must be one number or three, got {len(sc)}")
        if not all(np.isfinite(v) and v > 0.0 for v in sc):
            raise ValueError(f"{what}: scale must be positive and finite (as float32), got {sc}")
    pv = None
    if pivot is not None:
        try:
            with np.errstate(over="ignore"):
                pv = _f32_list(pivot)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: pivot must be three numbers, got {pivot!r}") from None
        if len(pv) != 3:
            raise ValueError(f"{what}: pivot must be three numbers, got {len(pv)}")
        if not all(np.isfinite(v) for v in pv):
            raise ValueError(f"{what}: pivot must be finite (as float32), got {pv}")
    return angle, axis, trans, sc, pv


MAX_BONES = 4                # DH_MAX_BONES (include/diffhandles_hip.h)


class Bend:
    """A bend edit of one instance (DESIGN.md "Bend edits"): it may stand wherever a transform tuple of an instance stands.
    bones: 1 .. 4 ordinary transforms, 3- or 5-tuples, each with its own scale and pivot; weights: an array or tensor
    [B, H, W], the weight of bone b at every pixel of the image.  A point of the instance goes to the weighted sum of where
    each bone puts it (linear-blend skinning).  Immutable; nothing is checked here (`check_bend`)."""
    __slots__ = ("bones", "weights")

    def __init__(self, bones, weights):
        object.__setattr__(self, "bones", tuple(tuple(b) if isinstance(b, (list, tuple)) else b for b in bones))
        object.__setattr__(self, "weights", weights)

    def __setattr__(self, name, value):
        raise AttributeError("Bend is immutable")

    def __delattr__(self, name):
        raise AttributeError("Bend is immutable")

    def __repr__(self):
        shape = tuple(getattr(self.weights, "shape", ()))
        return f"Bend({len(self.bones)} bones, weights {shape})"


def check_bend(bend, mask, what="bend"):
    """A `Bend` of the instance that draws `mask` ([1,1,H,W] or [H,W]) -> the `Bend` with every bone through `check_transform`
    and the weights as a float32 tensor [B, H, W] where they were.  ValueError naming `what` (the call, the edit and the
    instance) and the member: a bone that is no transform, B outside 1 .. 4, weights that are not [B, H, W] of the mask's
    size, that are not finite or negative, or that do not sum to 1 within 1e-5 on the mask's pixels.  Before any launch of the
    library (weights on a device are read there)."""
    checked, flags = _bend_checks(bend, mask, what)
    _raise_bend_flags(what, flags.tolist())
    return checked


def _bend_checks(bend, mask, what):
    """`check_bend` up to the values of the weights -> (the checked `Bend`, a float64 tensor where the weights are: [any weight
    not finite, any weight < 0, the largest |sum - 1| on the mask's pixels]).  Nothing here waits for the device, so a call with
    several Bends reads all their flags in one copy (`reproject_plan`)."""
    if not isinstance(bend, Bend):
        raise ValueError(f"{what}: expected a Bend, got {type(bend).__name__}")
    B = len(bend.bones)
    if not 1 <= B <= MAX_BONES:
        raise ValueError(f"{what}: a Bend has 1 to {MAX_BONES} bones, got {B}")
    bones = tuple(check_transform(b, f"{what}: bone {i}") for i, b in enumerate(bend.bones))
    w = bend.weights
    try:
        w = (w.detach() if isinstance(w, torch.Tensor) else torch.as_tensor(np.asarray(w))).to(torch.float32)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{what}: weights must be an array or tensor [B, H, W], got {type(bend.weights).__name__}") from None
    hw = tuple(mask.shape[-2:])
    if w.dim() != 3 or w.shape[0] != B or tuple(w.shape[1:]) != hw:
        raise ValueError(f"{what}: weights must be [{B}, {hw[0]}, {hw[1]}] ({B} bones, the mask's size), got {list(w.shape)}")
    on = (mask.detach() if isinstance(mask, torch.Tensor) else torch.as_tensor(np.asarray(mask))).reshape(hw) != 0
    on = on.to(w.device)
    off = (w.to(torch.float64).sum(dim=0) - 1.0).abs()
    off = torch.where(on & ~torch.isnan(off), off, torch.zeros_like(off)).max()          # (a NaN is the first flag's)
    flags = torch.stack([(~torch.isfinite(w)).any().to(torch.float64), (w < 0).any().to(torch.float64), off])
    return Bend(bones, w.contiguous()), flags


def _raise_bend_flags(what, flags):
    if flags[0]:
        raise ValueError(f"{what}: weights must be finite")
    if flags[1]:
        raise ValueError(f"{what}: weights must be >= 0")
    if flags[2] > 1e-5:
        raise ValueError(f"{what}: weights must sum to 1 on the mask's pixels (within 1e-5), off by up to {flags[2]:.3g}")


def check_body(tf, mask, what):
    """What stands for an instance in an edit: a transform tuple (`check_transform`) or a `Bend` (`check_bend` against the
    instance's mask)."""
    return check_bend(tf, mask, what) if isinstance(tf, Bend) else check_transform(tf, what)


def bend_chain(depth, intrinsics, mask, p0, p1, width, rot_angle, rot_axis, translation=(0.0, 0.0, 0.0), pivot=None, bones=2):
    """The `Bend` that bends the object of `mask` across the line p0 -> p1 (pixels, (x, y)): with d the signed pixel distance of
    a pixel from the line, d = ((x - x0)(y1 - y0) - (y - y0)(x1 - x0)) / |p1 - p0|, and s = clamp(d / width + 0.5, 0, 1) (B - 1),
    bone b has the hat weight max(0, 1 - |s - b|), turns by rot_angle b / (B - 1) about rot_axis through `pivot` and moves by
    translation b / (B - 1).  The side with d < -width / 2 stays put (bone 0), the side beyond +width / 2 takes the full
    motion, and the band between blends neighbouring bones.  pivot: a point in the coordinates of `depth_to_world_coords`;
    None = `pivot_at_pixel` of the midpoint of p0 p1.  More bones spread a large angle over smaller steps: linear-blend
    skinning pulls the band between two bones towards the chord.  ValueError: width <= 0, p0 == p1, bones outside 2 .. 4."""
    what = "bend_chain"
    try:
        (x0, y0), (x1, y1) = (float(p0[0]), float(p0[1])), (float(p1[0]), float(p1[1]))
    except (TypeError, ValueError, IndexError):
        raise ValueError(f"{what}: p0 and p1 must be pixels (x, y), got {p0!r}, {p1!r}") from None
    if not all(np.isfinite(v) for v in (x0, y0, x1, y1)):
        raise ValueError(f"{what}: p0 and p1 must be finite, got {p0!r}, {p1!r}")
    if (x0, y0) == (x1, y1):
        raise ValueError(f"{what}: p0 == p1 ({p0!r}) is no line")
    if not (isinstance(width, (int, float)) and np.isfinite(width) and width > 0):
        raise ValueError(f"{what}: width must be a positive number of pixels, got {width!r}")
    if not (isinstance(bones, int) and not isinstance(bones, bool) and 2 <= bones <= MAX_BONES):
        raise ValueError(f"{what}: bones must be 2 .. {MAX_BONES}, got {bones!r}")
    h, w = (int(v) for v in mask.shape[-2:])
    if pivot is None:
        pivot = pivot_at_pixel(depth, intrinsics, int(round((x0 + x1) / 2.0)), int(round((y0 + y1) / 2.0)))
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    d = ((xx - x0) * (y1 - y0) - (yy - y0) * (x1 - x0)) / float(np.hypot(x1 - x0, y1 - y0))
    s = (d / float(width) + 0.5).clamp(0.0, 1.0) * (bones - 1)
    weights = torch.stack([(1.0 - (s - b).abs()).clamp(min=0.0) for b in range(bones)]).to(torch.float32)
    tr = _f32_list(translation)
    tfs = [(float(rot_angle) * b / (bones - 1), rot_axis, tuple(t * b / (bones - 1) for t in tr), None, pivot) for b in range(bones)]
    return Bend(tfs, weights)


SIMILARITY_ROW = 16          # DH_SIMILARITY_ROW (include/diffhandles_hip.h)


def _xform_rows(transforms, similarity=False):
    """(angle_deg, axis, translation) -> 8 doubles per edit, with NumPy's own cos/sin: the rows of dh_reproject_edits /
    dh_reproject_object_edits.  similarity=True: 3- or 5-tuples (check_transform) -> the 16 doubles of
    dh_reproject_similarity_edits, the same 8 followed by scale[3], pivot[3], has-pivot flag, 0."""
    if similarity:
        return _similarity_rows([check_transform(tf) for tf in transforms])
    return _rigid_rows(transforms, np.zeros((len(transforms), 8), dtype=np.float64))


def _similarity_rows(checked):
    """The rows of dh_reproject_similarity_edits from transforms that went through check_transform."""
    rows = np.zeros((len(checked), SIMILARITY_ROW), dtype=np.float64)
    _rigid_rows([tf[:3] for tf in checked], rows)
    rows[:, 8:11] = 1.0
    for i, (_, _, _, sc, pv) in enumerate(checked):
        if sc != [1.0, 1.0, 1.0]:
            rows[i, 8:11] = sc
        if pv is not None:
            rows[i, 11:14] = pv
            rows[i, 14] = 1.0
    return rows


def _rigid_rows(transforms, rows):
    for i, (angle, axis, trans) in enumerate(transforms):
        ax = np.asarray(axis.detach().cpu().numpy() if isinstance(axis, torch.Tensor) else axis, dtype=np.float32)
        ax = ax / np.linalg.norm(ax)
        tr = trans.detach().cpu() if isinstance(trans, torch.Tensor) else torch.as_tensor(trans, dtype=torch.float32)
        theta = np.radians(float(angle) if not isinstance(angle, torch.Tensor) else angle.item())
        rows[i, 0:3] = ax.astype(np.float64)
        rows[i, 3], rows[i, 4] = np.cos(theta), np.sin(theta)
        rows[i, 5:8] = [tr[0].item(), tr[1].item(), tr[2].item()]
    return rows


MAX_OBJECTS = 8              # csrc/geometry.hip: the object table travels in the kernel arguments


def check_camera(camera, what="camera"):
    """One camera of an edit (camera moves, DESIGN.md "Camera moves"): None (no camera), or (rot_angle_deg, rot_axis[3],
    translation[3]) or (rot_angle_deg, rot_axis[3], translation[3], pivot) -> None, or (angle as a float, axis, translation
    and pivot as three float32 values each, the pivot None for the camera centre).  It is the motion of the CAMERA in the
    coordinates of `depth_to_world_coords`: turned about rot_axis through pivot (None = the origin: a pan or tilt;
    `pivot_at_pixel` gives an orbit centre), then translated.  The one validator: ValueError naming `what` (the call and the
    edit) for another tuple length, a member that is not finite (as float32), an axis or a translation or a pivot that is not
    three numbers, a zero axis.  Host only: no device work."""
    if camera is None:
        return None
    try:
        n = len(camera)
    except TypeError:
        n = -1
    if n not in (3, 4):
        raise ValueError(f"{what}: camera: expected (rot_angle, rot_axis, translation[, pivot]), got "
                         f"{n if n >= 0 else 'no'} members")
    angle, axis, trans = camera[0], camera[1], camera[2]
    pivot = camera[3] if n == 4 else None
    try:
        ang = float(angle.item() if isinstance(angle, torch.Tensor) else angle)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{what}: camera: rot_angle must be a number, got {angle!r}") from None
    if not np.isfinite(ang):
        raise ValueError(f"{what}: camera: rot_angle must be finite, got {angle!r}")
    out = []
    for name, v in (("rot_axis", axis), ("translation", trans), ("pivot", pivot)):
        if v is None and name == "pivot":
            out.append(None)
            continue
        try:
            with np.errstate(over="ignore"):
                f = _f32_list(v)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: camera: {name} must be three numbers, got {v!r}") from None
        if len(f) != 3:
            raise ValueError(f"{what}: camera: {name} must be three numbers, got {len(f)}")
        if not all(np.isfinite(x) for x in f):
            raise ValueError(f"{what}: camera: {name} must be finite (as float32), got {f}")
        out.append(f)
    ax = np.asarray(out[0], dtype=np.float32)
    with np.errstate(all="ignore"):
        unit = ax / np.linalg.norm(ax)
    if not float(np.linalg.norm(ax)) > 0.0 or not np.all(np.isfinite(unit)):
        raise ValueError(f"{what}: camera: rot_axis must not be zero, got {out[0]}")
    return ang, out[0], out[1], out[2]


def view_row(camera):
    """The one builder of a view row: a camera that went through `check_camera` -> the DH_SIMILARITY_ROW doubles of the INVERSE
    motion (include/diffhandles_hip.h, dh_reproject_camera_edits): the f32-normalised axis, cos / sin of -rot_angle as
    `_rigid_rows` computes them, scale 1, the pivot (f32) or zeros with the has-pivot flag 1, and the translation
    t' = -(t cos + (a x t) sin + a (a . t)(1 - cos)) computed in f64 from the f32 axis and translation and rounded to f32."""
    ang, axis, trans, pivot = camera
    row = np.zeros((1, SIMILARITY_ROW), dtype=np.float64)
    _rigid_rows([(-ang, axis, [0.0, 0.0, 0.0])], row)
    row = row[0]
    a, c, s = row[0:3].copy(), row[3], row[4]
    t = np.asarray(trans, dtype=np.float32).astype(np.float64)
    tp = -(t * c + np.cross(a, t) * s + a * np.dot(a, t) * (1.0 - c))
    row[5:8] = tp.astype(np.float32).astype(np.float64)
    row[8:11] = 1.0
    if pivot is not None:
        row[11:14] = np.asarray(pivot, dtype=np.float32).astype(np.float64)
    row[14] = 1.0
    return row


def orbit_cameras(depth, intrinsics, x, y, angles, axis=(0.0, 1.0, 0.0)):
    """Cameras that turn about the point of pixel (x, y) = (column, row) of `depth` by each of `angles` (degrees) about `axis`,
    without translation: a turntable of K views for `reproject_camera_edits` / `transform_foreground_objects_batch`."""
    pivot = [float(v) for v in pivot_at_pixel(depth, intrinsics, x, y)]
    axis = [float(v) for v in _f32_list(axis)]
    return [check_camera((float(a), axis, (0.0, 0.0, 0.0), pivot), f"orbit_cameras: angle {k}") for k, a in enumerate(angles)]


def check_footprints(footprints, footprint_max_ratio, what="footprints"):
    """The footprint settings of a point-mode call -> (bool, None or the ratio as a float32 value).  ValueError for a ratio that
    is not a finite float > 1 (as float32) and for a ratio without footprints.  Host only: no device work."""
    footprints = bool(footprints)
    if footprint_max_ratio is None:
        return footprints, None
    try:
        with np.errstate(over="ignore"):
            ratio = float(np.float32(footprint_max_ratio))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: footprint_max_ratio must be a number > 1 or None, got {footprint_max_ratio!r}") from None
    if not (np.isfinite(ratio) and ratio > 1.0):
        raise ValueError(f"{what}: footprint_max_ratio must be finite and > 1 (as float32), got {footprint_max_ratio!r}")
    if not footprints:
        raise ValueError(f"{what}: footprint_max_ratio={footprint_max_ratio!r} without footprints=True")
    return footprints, ratio


def mesh_has_no_footprints(footprints, footprint_max_ratio, what):
    """Mesh mode draws triangles already: the footprint settings are checked as the point mode checks them, then
    footprints=True is refused.  Host only."""
    footprints, _ = check_footprints(footprints, footprint_max_ratio, what)
    if footprints:
        raise NotImplementedError(f"{what}: depth_transform_mode 'mesh' has no footprints (got footprints=True); use 'pc'")


INFILL_BORDERS = ("zero", "reflect")          # the C value is the index (include/diffhandles_hip.h, "The image border of the in-fill")


def check_infill_border(value, what="infill_border"):
    """The image border of the in-fill -> 0 (None or "zero": a neighbour beyond the frame is a known 0) or 1 ("reflect": the
    mirror ghost cell, zero normal derivative at the frame).  ValueError naming the call for anything else.  Host only."""
    if value is None:
        return 0
    if isinstance(value, str) and value in INFILL_BORDERS:
        return INFILL_BORDERS.index(value)
    raise ValueError(f"{what}: infill_border must be 'zero' or 'reflect' (or None = 'zero'), got {value!r}")


def mesh_has_no_infill_border(value, what):
    """Mesh mode in-fills against zero only: the setting is checked as the point mode checks it, then "reflect" is refused.
    `transform_depth_mesh` and `transform_depth` keep the parameter lists they have and take no border, so the callers that
    read the setting (DiffusionHandles' conf key, tools/run_edit.py --infill-border) refuse it for them here.  Host only."""
    if check_infill_border(value, what):
        raise NotImplementedError(f"{what}: depth_transform_mode 'mesh' has no reflecting in-fill border (got "
                                  f"infill_border={value!r}); use 'pc'")


def check_view_surfaces(view_surfaces, view_surface_max_ratio, what="view_surfaces"):
    """The view-surface settings of a point-mode call (DESIGN.md "View surfaces") -> (bool, None or the ratio as a float32
    value).  ValueError for a ratio that is not a finite float > 1 (as float32) and for a ratio without the setting.  The one
    validator; host only: no device work."""
    view_surfaces = bool(view_surfaces)
    if view_surface_max_ratio is None:
        return view_surfaces, None
    try:
        if np.ndim(view_surface_max_ratio) != 0:
            raise TypeError("not a scalar")
        with np.errstate(over="ignore"):
            ratio = float(np.float32(view_surface_max_ratio))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: view_surface_max_ratio must be a number > 1 or None, got {view_surface_max_ratio!r}") from None
    if isinstance(view_surface_max_ratio, bool) or not (np.isfinite(ratio) and ratio > 1.0):
        raise ValueError(f"{what}: view_surface_max_ratio must be finite and > 1 (as float32), got {view_surface_max_ratio!r}")
    if not view_surfaces:
        raise ValueError(f"{what}: view_surface_max_ratio={view_surface_max_ratio!r} without view_surfaces=True")
    return view_surfaces, ratio


def mesh_has_no_view_surfaces(view_surfaces, view_surface_max_ratio, what):
    """Mesh mode draws triangles already and has no camera: the settings are checked as the point mode checks them, then
    view_surfaces=True is refused.  Host only."""
    view_surfaces, _ = check_view_surfaces(view_surfaces, view_surface_max_ratio, what)
    if view_surfaces:
        raise NotImplementedError(f"{what}: depth_transform_mode 'mesh' has no view surfaces (got depth_transform_view_surfaces=True); "
                                  f"use 'pc'")


def check_instances(instances, n_masks, what="instances"):
    """The instance table of an edit with copies -> list of N mask indices (None -> None: one instance per mask).
    ValueError naming `what` and the instance for more than 8 instances, an entry that is not an integer in 0 .. n_masks - 1,
    or a mask that no instance names (removing an object is not supported).  Host only: no device work."""
    if instances is None:
        return None
    try:
        inst = list(instances)
    except TypeError:
        raise ValueError(f"{what}: expected a list of mask indices, got {instances!r}") from None
    if not 1 <= len(inst) <= MAX_OBJECTS:
        raise ValueError(f"{what}: expected 1 to {MAX_OBJECTS} instances, got {len(inst)}")
    out = []
    for n, o in enumerate(inst):
        if isinstance(o, bool) or not isinstance(o, (int, np.integer)) or not 0 <= int(o) < n_masks:
            raise ValueError(f"{what}: instance {n} names mask {o!r}, expected an integer in 0..{n_masks - 1}")
        out.append(int(o))
    for m in range(n_masks):
        if m not in out:
            raise ValueError(f"{what}: mask {m} has no instance (removing an object is not supported; every mask needs at "
                             f"least one instance)")
    return out


def check_removed_masks(removed_masks, fg_masks, what="removed_masks"):
    """The removed masks of an edit (object removal, DESIGN.md "Object removal") -> list of R >= 0 masks (None -> []).
    ValueError naming `what` and the mask for something that is not a list of masks, or a mask that is not square or not of
    the size of the foreground masks (of the first removed mask when there is no foreground mask).  Host only: it reads shapes.
    Whether a removed mask overlaps a foreground mask or another removed mask is a question about pixels:
    `reproject_plan` answers it in the device-to-host copy that reads the pixel counts, `removed_overlap` on its own."""
    if removed_masks is None:
        return []
    if isinstance(removed_masks, (torch.Tensor, np.ndarray)) or not isinstance(removed_masks, (list, tuple)):
        raise ValueError(f"{what}: expected a list of masks, got {type(removed_masks).__name__}")
    out = []
    size = None if len(fg_masks) == 0 else tuple(fg_masks[0].shape[-2:])
    for r, mask in enumerate(removed_masks):
        if not isinstance(mask, torch.Tensor) or mask.dim() < 2:
            raise ValueError(f"{what}: removed mask {r} is not a [.., H, W] tensor")
        if mask.shape[-2] != mask.shape[-1] or mask.numel() != mask.shape[-1] * mask.shape[-1]:
            raise ValueError(f"{what}: removed mask {r} is not one square image, got shape {tuple(mask.shape)}")
        if size is None:
            size = tuple(mask.shape[-2:])
        if tuple(mask.shape[-2:]) != size:
            raise ValueError(f"{what}: removed mask {r} is {mask.shape[-1]} x {mask.shape[-2]}, the other masks are "
                             f"{size[1]} x {size[0]}")
        out.append(mask)
    return out


def removed_overlap(removed_masks, fg_masks, what="removed_masks"):
    """ValueError naming `what` and the masks when a removed mask shares a pixel with a foreground mask or with an earlier
    removed mask.  Host arithmetic on the masks where they are (one copy per mask pair tested: the error path and host callers;
    `reproject_plan` carries one flag per removed mask in its own copy and calls this only to name the pair)."""
    removed = check_removed_masks(removed_masks, fg_masks, what)
    flat = lambda m: (m.detach() != 0).reshape(-1)
    for r, mask in enumerate(removed):
        mr = flat(mask)
        for m, fg in enumerate(fg_masks):
            if bool((mr & flat(fg).to(mr.device)).any()):
                raise ValueError(f"{what}: removed mask {r} overlaps foreground mask {m}")
        for q in range(r):
            if bool((mr & flat(removed[q]).to(mr.device)).any()):
                raise ValueError(f"{what}: removed mask {r} overlaps removed mask {q}")


def vacated_image(removed_masks, device=None):
    """[H, W] uint8 union of the removed masks (1 = vacated) on `device` (default: where the first mask is); None for no mask.
    An all-zero image is the call without it, byte for byte, so nothing here reads a pixel back."""
    removed = check_removed_masks(removed_masks, [], "vacated_image")
    if not removed:
        return None
    dev = removed[0].device if device is None else device
    res = removed[0].shape[-1]
    out = torch.zeros((res, res), dtype=torch.bool, device=dev)
    for mask in removed:
        out |= (mask.detach().to(dev) != 0).reshape(res, res)
    return out.to(torch.uint8).contiguous()


def check_donor(donor_depth, donor_masks, res, n_host, what="donor"):
    """The donor of an edit (object insertion, DESIGN.md "Object insertion") -> None, or (donor depth, list of D >= 1 masks).
    The one validator of a donor: ValueError naming `what` and the member for a donor without depth or without masks, a depth
    or a mask that is not one res x res image (the donor has the host's resolution), an empty mask beside non-empty ones,
    overlapping donor masks, and n_host + D > 8.  None for no donor: both arguments None, or every mask empty -- that is the
    call without the keyword.  It reads the masks' pixel counts (one device-to-host copy), before any launch of the library."""
    if donor_depth is None and donor_masks is None:
        return None
    if donor_depth is None:
        raise ValueError(f"{what}: donor: masks without a depth")
    if donor_masks is None:
        raise ValueError(f"{what}: donor: a depth without masks")
    if isinstance(donor_masks, (torch.Tensor, np.ndarray)) or not isinstance(donor_masks, (list, tuple)):
        raise ValueError(f"{what}: donor: masks: expected a list of masks, got {type(donor_masks).__name__}")
    if len(donor_masks) == 0:
        raise ValueError(f"{what}: donor: masks: the list is empty (a donor brings at least one mask)")
    res = int(res)
    if not isinstance(donor_depth, torch.Tensor) or donor_depth.numel() != res * res or tuple(donor_depth.shape[-2:]) != (res, res):
        raise ValueError(f"{what}: donor: depth has shape {tuple(getattr(donor_depth, 'shape', ()))}, the host is {res} x {res} "
                         "(a donor of another resolution is not supported)")
    for d, mask in enumerate(donor_masks):
        if not isinstance(mask, torch.Tensor) or mask.numel() != res * res or tuple(mask.shape[-2:]) != (res, res):
            raise ValueError(f"{what}: donor: mask {d} has shape {tuple(getattr(mask, 'shape', ()))}, the host is {res} x {res} "
                             "(a donor of another resolution is not supported)")
    flat = torch.stack([(m.detach() != 0).reshape(-1) for m in donor_masks]).to(torch.uint8)
    stats = torch.cat([flat.sum(dim=1), (flat.sum(dim=0) > 1).any()[None].to(torch.int64)]).tolist()
    counts, overlap = stats[:-1], stats[-1]
    if not any(counts):
        return None
    for d, c in enumerate(counts):
        if c == 0:
            raise ValueError(f"{what}: donor: mask {d} is empty (drop it, and renumber what names the masks behind it)")
    if overlap:
        for d in range(len(donor_masks)):
            for q in range(d):
                if bool((flat[d] & flat[q]).any()):
                    raise ValueError(f"{what}: donor: mask {d} overlaps donor mask {q}")
    if int(n_host) + len(donor_masks) > MAX_OBJECTS:
        raise ValueError(f"{what}: donor: {n_host} host masks and {len(donor_masks)} donor masks, at most {MAX_OBJECTS} in all")
    return donor_depth, list(donor_masks)


def donor_rows(rows, instances, n_host):
    """One byte per correspondence row: 1 where the row's instance draws a donor mask (instances[rows[r]] >= n_host).  `rows`
    holds instance indices as uint8 (256 table entries: the rows past the counts are not written), the result lies beside it."""
    lut = torch.zeros(256, dtype=torch.uint8)
    lut[:len(instances)] = torch.tensor([1 if o >= n_host else 0 for o in instances], dtype=torch.uint8)
    return lut.to(rows.device)[rows.long()]


def _plan(kind, **fields):
    """The record `reproject_plan` returns: what it decided about one call, host values only, nothing of the compute device.

    kind              "objects", "pure_removal", "pure_camera" or "empty" ("empty" launches nothing; the others are one
                      dh_reproject call, or one per edit, on the record `reproject_record` makes of the plan)
    res               the side of the images
    M, D, N           host masks, donor masks and instances as the caller gave them
    kept              indices of the non-empty masks (host masks, then donor masks)
    obj_start         int32, len(kept) + 1 offsets of the kept masks' slices of the pixel list
    n_host_kept       how many kept masks are host masks
    caller            the caller's instance indices that survive (an empty mask is dropped with its instances)
    inst_obj          int32 index into kept, per surviving instance
    inst_start        int32 point-list offsets, per surviving instance
    n_fg, n_pts       foreground points, and points summed over the instances (equal without copies)
    cap               correspondence rows per edit
    with_table        the call carries the instance table, and the debug dict has corr_inst / inst_start
    return_instances  every result carries the instance array
    footprints, ratio the checked footprint settings (check_footprints)
    edits             K lists of transforms after check_transform (as given where nothing moves)
    cams              K cameras after check_camera / None, or None for a call without a camera
    removed           the removed masks (check_removed_masks); removed_given: removed_masks was not None, so the debug dict has vacated
    donor             (donor depth, donor masks) after check_donor, or None
    inst              the instance table over the M + D masks (one instance per mask where the caller gave none)
    masks_u8          [M + D, res * res] uint8, where the masks are
    vacated           [res * res] bool union of the removed masks, or None
    covered           camera calls: [res * res] bool, host masks and removed masks (bg_valid is its complement), or None
    infill_border     0 (zero) or 1 (reflect)
    view_surfaces     the setting is on AND an edit has a camera: one row per target pixel in the edits with a camera (False
                      otherwise: the setting acts only where there is a view); surface_ratio: None or the checked ratio
    bent, n_bones     an instance of an edit is a `Bend`: n_bones rows per instance and edit (the
                      largest bone count of the call; shorter instances pad with copies of their bone 0 at weight 0) and the
                      weights gathered at the instances' pixels.  False, 1: the call it was"""
    p = types.SimpleNamespace(kind=kind, N=0, kept=[], n_host_kept=0, caller=[],
                              obj_start=np.zeros(1, dtype=np.int32), inst_obj=np.zeros(0, dtype=np.int32),
                              inst_start=np.zeros(1, dtype=np.int32), n_fg=0, n_pts=0, cap=0, with_table=False, inst=None, masks_u8=None,
                              vacated=None, covered=None, infill_border=0, view_surfaces=False, surface_ratio=None, n_bones=1, bent=False)
    vars(p).update(fields)
    return p


def _removed_stats(removed, seen):
    """Per removed mask its pixel count and whether it meets the union before it (`seen`, which it joins) -> (the 2 R values as
    0-d int64 tensors for the caller's one device-to-host copy, `seen` with the removed masks in it)."""
    extra = []
    for mask in removed:
        mr = (mask.detach() != 0).reshape(-1).to(seen.device)
        extra += [mr.sum(), (mr & seen).any().to(torch.int64)]
        seen = seen | mr
    return extra, seen


def _check_single_image(shape):
    if len(shape) != 4 or shape[0] != 1:
        raise ValueError("Only batch size 1 is supported")


def _removed_fit_depth(removed, shape, what):
    """A call without a foreground point takes its size from the first removed mask: the depth has to have it."""
    res = removed[0].shape[-1]
    if shape[-1] != res or shape[-2] != res:
        raise ValueError(f"{what}: removed_masks: removed mask 0 is {res} x {res}, the depth {shape[-1]} x {shape[-2]}")
    return res


def _plan_pure_camera(shape, removed):
    """The checks of a camera call without a foreground point -> (res, the union of the removed masks or None)."""
    what = "reproject_camera_edits"
    _check_single_image(shape)
    res = int(shape[-1])
    if shape[-2] != res:
        raise RuntimeError("square depth maps only")
    for r, mask in enumerate(removed):
        if mask.shape[-1] != res:
            raise ValueError(f"{what}: removed_masks: removed mask {r} is {mask.shape[-1]} x {mask.shape[-2]}, the depth {res} x {res}")
    if not removed:
        return res, None
    removed_overlap(removed, [], f"{what}: removed_masks")
    return res, _removed_stats(removed, torch.zeros(res * res, dtype=torch.bool, device=removed[0].device))[1]


def reproject_plan(depth, fg_masks, edits, *, instances=None, removed_masks=None, donor_depth=None, donor_masks=None, cameras=None,
                   footprints=False, footprint_max_ratio=None, return_instances=False, what=None, infill_border="zero",
                   view_surfaces=False, view_surface_max_ratio=None):
    """Everything `reproject` decides before it touches the compute device -> the record of `_plan`.  depth: the depth or its shape; the
    other arguments are `reproject`'s.  Every host check of the call (ValueError / NotImplementedError / RuntimeError with the
    texts the named functions always had; `what` is the caller's name in the two refusals of a call without a foreground mask)
    and the ONE device-to-host copy of the masks' statistics (pixel counts, overlap flags; none for host masks; `check_donor`
    reads the donor's masks in a copy of its own).  No call of the library, no compute device, no allocation there: CPU masks
    on a machine without a GPU give the same plan."""
    shape = tuple(getattr(depth, "shape", depth))
    removal = "reproject_removal_edits"
    footprints, ratio = check_footprints(footprints, footprint_max_ratio, "reproject_object_edits")
    border = check_infill_border(infill_border, "reproject_border_edits")
    surfaces, surface_ratio = check_view_surfaces(view_surfaces, view_surface_max_ratio, "reproject_surface_edits")
    fg_masks = list(fg_masks)
    edits = [list(tfs) for tfs in edits]
    cams = None
    if cameras is not None:
        cameras = list(cameras)
        if len(cameras) != len(edits):
            raise ValueError(f"reproject_camera_edits: cameras has {len(cameras)} entries for {len(edits)} edits")
        cams = [check_camera(c, f"reproject_camera_edits: edit {e}") for e, c in enumerate(cameras)]
        if all(c is None for c in cams):
            cams = None
    if cams is not None:
        if footprints:
            raise NotImplementedError("reproject_camera_edits: footprints with a camera are not supported (depth_transform_footprints)")
        return_instances = True
    removed = check_removed_masks(removed_masks, fg_masks, f"{removal}: removed_masks")
    M = len(fg_masks)
    donor = None
    if donor_depth is not None or donor_masks is not None:
        donor = check_donor(donor_depth, donor_masks, shape[-1], M, "reproject_donor_edits")
    if donor is not None:
        if surfaces:
            raise NotImplementedError("reproject_surface_edits: view surfaces with a donor are not supported "
                                      "(depth_transform_view_surfaces; two images share pixel indices)")
        if footprints:
            raise NotImplementedError("reproject_donor_edits: footprints with a donor are not supported (depth_transform_footprints; "
                                      "two images share pixel indices)")
        if fg_masks and fg_masks[0].shape[-1] != shape[-1]:
            raise ValueError("reproject_donor_edits: donor: the foreground masks and the depth differ in size")
        return_instances = True
    donor_list = [] if donor is None else donor[1]
    D = len(donor_list)
    common = dict(M=M, D=D, return_instances=bool(return_instances), footprints=footprints, ratio=ratio, cams=cams, removed=removed,
                  removed_given=removed_masks is not None, donor=donor, infill_border=border,
                  view_surfaces=surfaces and cams is not None, surface_ratio=surface_ratio if cams is not None else None)
    surfaces = common["view_surfaces"]          # (without a camera the call is the call without the setting)
    if M == 0 and (removed or cams is not None) and donor is None:
        for e, tfs in enumerate(edits):
            if len(tfs) != 0:
                raise ValueError(f"{what or removal}: edit {e} has {len(tfs)} transforms, but there is no foreground mask (a pure "
                                 f"removal moves nothing)")
        if instances is not None and len(list(instances)) != 0:
            raise ValueError(f"{what or removal}: instances={instances!r} given without a foreground mask (a pure removal has no "
                             f"instance)")
        if cams is not None:
            res, covered = _plan_pure_camera(shape, removed)
            return _plan("pure_camera", res=res, edits=edits, covered=covered, **common)
        _check_single_image(shape)
        res = _removed_fit_depth(removed, shape, removal)
        extra, vacated = _removed_stats(removed, torch.zeros(res * res, dtype=torch.bool, device=removed[0].device))
        tail = torch.stack(extra).tolist()          # the one device-to-host copy of this call
        if any(tail[1::2]):
            removed_overlap(removed, [], f"{removal}: removed_masks")
        if sum(tail[0::2]) == 0:
            raise ValueError(f"Expected 1 to {MAX_OBJECTS} foreground masks, got 0")
        return _plan("pure_removal", res=res, edits=edits, with_table=instances is not None, vacated=vacated,
                             **common)
    if not 1 <= M <= MAX_OBJECTS and donor is None:
        raise ValueError(f"Expected 1 to {MAX_OBJECTS} foreground masks, got {M}")
    # (with a donor the table names every mask of the concatenated list: the host's M, then the donor's D)
    inst = check_instances(instances, M + D, "reproject_donor_edits: instances" if donor is not None else
                           "reproject_instance_edits: instances")
    with_table = inst is not None or bool(return_instances)
    if inst is None:
        inst = list(range(M + D))
    N = len(inst)
    for e, tfs in enumerate(edits):
        if len(tfs) != N:
            if instances is None:
                raise ValueError(f"Edit {e} has {len(tfs)} transforms for {M + D} foreground masks")
            raise ValueError(f"Edit {e} has {len(tfs)} transforms for {N} instances")
    # (a Bend is checked against the mask its instance draws, below, once the masks' sizes are known to agree)
    edits = [[tf if isinstance(tf, Bend) else check_transform(tf, f"edit {e}, {'object' if instances is None else 'instance'} {m}")
              for m, tf in enumerate(tfs)] for e, tfs in enumerate(edits)]
    for fg_mask in fg_masks:
        if fg_mask.shape[-2] != fg_mask.shape[-1]:
            raise RuntimeError(f"Expected fg_mask to be square, got shape {fg_mask.shape[-2]} x {fg_mask.shape[-1]}.")
        if fg_mask.shape[-1] != fg_masks[0].shape[-1]:
            raise ValueError("Expected all foreground masks to have one size")
    _check_single_image(shape)
    res = fg_masks[0].shape[-1] if M else int(shape[-1])
    n_bones, flags = 1, []
    for e, tfs in enumerate(edits):
        for m, tf in enumerate(tfs):
            if isinstance(tf, Bend):
                name = f"reproject_bend_edits: edit {e}, {'object' if instances is None else 'instance'} {m}"
                tfs[m], f = _bend_checks(tf, (fg_masks + list(donor_list))[inst[m]], name)
                flags.append((name, f))
                n_bones = max(n_bones, len(tfs[m].bones))
    bent = bool(flags)
    if bent:          # the weights' flags of every Bend of the call: ONE copy per device they lie on
        where = {}
        for name, f in flags:
            where.setdefault(f.device, []).append((name, f))
        for group in where.values():
            for (name, _), row in zip(group, torch.stack([f for _, f in group]).tolist()):
                _raise_bend_flags(name, row)
    common.update(n_bones=n_bones, bent=bent)
    # the M pixel counts and the overlap flag: ONE device-to-host copy (none for host masks), before any launch of the library
    flat = [(fg_mask.detach() != 0).reshape(-1) for fg_mask in fg_masks]
    if donor is not None:          # the donor's masks behind the host's (they were checked, and are on the first mask's device)
        flat += [(m.detach() != 0).reshape(-1).to(flat[0].device if flat else m.device) for m in donor_list]
    masks_u8 = (flat[0][None] if M + D == 1 else torch.stack(flat)).to(torch.uint8)
    stats = masks_u8.sum(dim=1)
    if M > 1:
        stats = torch.cat([stats, (masks_u8[:M].sum(dim=0) > 1).any()[None].to(stats.dtype)])
    vacated = None
    covered = masks_u8[:M].sum(dim=0) > 0 if removed or cams is not None else None
    if removed:
        # the removed masks ride in the same copy (they are disjoint from the foreground masks, or the call is refused below)
        extra, everything = _removed_stats(removed, covered)
        vacated, covered = everything & ~covered, everything
        stats = torch.cat([stats, torch.stack(extra)])
    stats = stats.tolist()
    if M > 1 and stats[M + D]:
        raise ValueError("The foreground masks overlap")
    n_vacated = 0
    if removed:
        tail = stats[len(stats) - 2 * len(removed):]
        if any(tail[1::2]):
            removed_overlap(removed, fg_masks, f"{removal}: removed_masks")
            raise ValueError(f"{removal}: removed_masks: removed mask {tail[1::2].index(1)} overlaps another mask")
        n_vacated = sum(tail[0::2])
    kept = [m for m in range(M + D) if stats[m] > 0]
    obj_start = np.zeros(len(kept) + 1, dtype=np.int32)
    obj_start[1:] = np.cumsum([stats[m] for m in kept])
    n_fg = int(obj_start[-1])
    common.update(N=N, edits=edits, inst=inst, with_table=with_table, vacated=vacated)
    if n_fg == 0 and cams is not None:
        # every mask is empty (dropped with its transforms): the pure camera move
        res, covered = _plan_pure_camera(shape, removed)
        return _plan("pure_camera", res=res, covered=covered, **common)
    if n_fg == 0 and n_vacated > 0:
        # every foreground mask is empty (dropped with its transforms) and an object is deleted: the pure removal
        _removed_fit_depth(removed, shape, removal)
        return _plan("pure_removal", res=res, **common)
    if n_fg == 0:
        return _plan("empty", res=res, **common)
    # the instances of the kept masks (empty masks are dropped with all of their instances); caller[n'] = the caller's index
    caller = [n for n in range(N) if inst[n] in kept]
    inst_obj = np.asarray([kept.index(inst[n]) for n in caller], dtype=np.int32)
    inst_start = np.zeros(len(caller) + 1, dtype=np.int32)
    inst_start[1:] = np.cumsum([int(obj_start[o + 1] - obj_start[o]) for o in inst_obj])
    n_pts = int(inst_start[-1])                # = n_fg without copies
    return _plan("objects", res=res, kept=kept, obj_start=obj_start, n_host_kept=sum(1 for m in kept if m < M),
                         caller=caller, inst_obj=inst_obj, inst_start=inst_start, n_fg=n_fg, n_pts=n_pts,
                         cap=res * res if footprints or surfaces else n_pts,          # one row per target pixel with footprints / view surfaces, per point without
                         masks_u8=masks_u8, covered=covered if cams is not None else None, **common)


def _run_plan(p, depth, bg_depth, intrinsics, use_input_depth_normalization, return_debug, device_correspondences):
    """The one place a re-projection allocates and launches: the geometry set-up every kind shares, then what the plan names."""
    g = types.SimpleNamespace(out_dev=depth.device, dev=_compute_device(depth), L=_lib.lib(), st=_lib.stream_ptr(), res=p.res,
                              K=len(p.edits), return_debug=return_debug, on_device=device_correspondences)
    d = depth.detach().to(g.dev, torch.float32).contiguous()
    g.d, g.bg = d, bg_depth.detach().to(g.dev, torch.float32).contiguous()
    g.bounds = None
    if use_input_depth_normalization:
        disp_in = 1.0 / d
        g.bounds = torch.stack([disp_in.min(), disp_in.max()]).to(torch.float32).contiguous()
    if p.kind == "empty":
        # empty foreground: the input disparity and no correspondences (depth_transform.py:203-216)
        lo_hi = None if g.bounds is None else (g.bounds[0], g.bounds[1])
        disp = normalize_depth(1.0 / d, bounds=lo_hi).to(g.out_dev)
        empty = torch.zeros((0, 4), dtype=torch.int64)
        res_list = [(disp, empty) + ((torch.zeros(0, dtype=torch.uint8),) if p.return_instances else ()) for _ in range(g.K)]
        return (res_list, dict(vacated=_vacated_u8(p, g)) if p.removed_given else {}) if return_debug else res_list
    g.gx, g.gy = _grids(g.res, g.res, g.dev)
    g.ifx, g.ify = _inv_focal(intrinsics)
    kcpu = intrinsics.detach().to("cpu", torch.float32)
    g.fx, g.fy = float(kcpu[0, 0]), float(kcpu[1, 1])
    return _run_objects(p, g) if p.kind == "objects" else _run_background(p, g)


def _host_ptr(arr, ctype):
    return arr.ctypes.data_as(ctypes.POINTER(ctype))


def reproject_record(p, K):
    """The size-and-settings part of the dh_reproject_args (include/diffhandles_hip.h) of the plan's call with K edits: sizes, the
    mask and instance tables, the donor count, has_view, border, surfaces and ratio, footprints and ratio, bones, capacity --
    everything dh_reproject_workspace reads.  Pure host; `_run_objects` / `_run_background` add the pointers and call
    dh_reproject.  Zero means off, so a member is set only where the plan has the feature:
      the table      with an instance table, a camera, a reflecting border or a `Bend` (without: the identity table on the
                     workspace layout of the call without copies)
      has_view       with a camera: one flag per edit
    A kind without a foreground point ("pure_removal", "pure_camera") is one call per edit: n_fg = 0, n_edits = 1, and
    has_view[0] says whether ANY edit has a camera (the one workspace serves them all; `_run_background` sets each edit's).
    ValueError for the kind "empty", which launches nothing."""
    if p.kind == "empty":
        raise ValueError("reproject_record: an empty plan launches nothing and has no record")
    a = _lib.ReprojectArgs(res=p.res, n_fg=p.n_fg, n_edits=K, infill_border=p.infill_border, view_surfaces=int(p.view_surfaces),
                           surface_max_ratio=0.0 if p.surface_ratio is None else p.surface_ratio)
    has_view = None if p.cams is None else np.asarray([c is not None for c in p.cams], dtype=np.uint8)
    if p.kind != "objects":
        a.n_edits = 1
        has_view = None if has_view is None else np.asarray([has_view.any()], dtype=np.uint8)
    else:
        a.n_objects, a.n_donor_objects, a.corr_capacity = len(p.kept), len(p.kept) - p.n_host_kept, p.cap
        a.footprints, a.max_ratio = int(p.footprints), 0.0 if p.ratio is None else p.ratio
        a.obj_start = _host_ptr(p.obj_start, ctypes.c_int32)
        if p.with_table or p.cams is not None or p.infill_border or p.bent:
            a.n_instances, a.inst_obj = len(p.caller), _host_ptr(p.inst_obj, ctypes.c_int32)
        if p.bent:
            a.n_bones = p.n_bones
    if has_view is not None:
        a.has_view = _host_ptr(has_view, ctypes.c_uint8)
    a.host_arrays = (p.obj_start, p.inst_obj, has_view)          # (the record points into them)
    return a


def _workspace(a, g):
    """The workspace of the record's call, sized by dh_reproject_workspace."""
    nbytes = ctypes.c_size_t()
    _lib.check(g.L.dh_reproject_workspace(ctypes.byref(a), ctypes.byref(nbytes)), "dh_reproject_workspace")
    a.workspace_tensor = torch.empty(nbytes.value, dtype=torch.uint8, device=g.dev)
    a.workspace, a.workspace_bytes, a.stream = _lib.ptr(a.workspace_tensor), nbytes.value, g.st


def _geometry(a, g):
    """The members every call shares: the background depth, the pixel grids, the intrinsics, the bounds."""
    a.bg_depth, a.grid_x, a.grid_y, a.bounds = _lib.ptr(g.bg), _lib.ptr(g.gx), _lib.ptr(g.gy), _lib.ptr(g.bounds)
    a.inv_fx, a.inv_fy, a.fx, a.fy = g.ifx, g.ify, g.fx, g.fy


def _vacated_u8(p, g):
    if p.vacated is None:
        return torch.zeros((g.res, g.res), dtype=torch.uint8, device=g.dev)
    return p.vacated.to(g.dev).reshape(g.res, g.res).to(torch.uint8)


def _empty_debug(g, table):
    """The debug tensors of a call without a foreground point (`table`: the instance members too)."""
    K, res, dev = g.K, g.res, g.dev
    zeros = torch.zeros((K, res, res), dtype=torch.uint8, device=dev)
    dbg = dict(raw_mask=zeros, clean_mask=zeros.clone(), vis=torch.zeros((K, 0), dtype=torch.uint8, device=dev),
               target_xy=torch.zeros((K, 0, 2), dtype=torch.int32, device=dev), fg_pix=torch.zeros(0, dtype=torch.int32, device=dev),
               corr_dev=torch.zeros((K, 0, 4), dtype=torch.int64, device=dev), obj_start=np.zeros(1, dtype=np.int32))
    if table:
        dbg.update(corr_inst=torch.zeros((K, 0), dtype=torch.uint8, device=dev), inst_start=np.zeros(1, dtype=np.int32))
    return dbg


def _run_background(p, g):
    """The kinds without a foreground point (dh_reproject with n_fg = 0).  "pure_removal": one call, its result K times.
    "pure_camera": one call per edit, with the edit's view (an edit without a camera: without a view, the pure removal's
    result); every row is a background row, instance index N."""
    camera = p.kind == "pure_camera"
    dev, res, K = g.dev, g.res, g.K
    views = [None if c is None else view_row(c) for c in p.cams] if camera else [None]
    n = len(views)
    a = reproject_record(p, K)
    _workspace(a, g)
    _geometry(a, g)
    zmap = torch.empty((n, res, res), dtype=torch.float32, device=dev)
    disp = torch.empty((n, res, res), dtype=torch.float32, device=dev)
    counts = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    if camera:
        covered = torch.zeros(res * res, dtype=torch.bool, device=dev) if p.covered is None else p.covered.to(dev)
        bg_valid = (~covered).to(torch.uint8).contiguous()
        bg_corr = torch.empty((K, res * res, 4), dtype=torch.int64, device=dev)
        bg_counts = torch.zeros(K, dtype=torch.int32, device=dev)
    for e, view in enumerate(views):
        a.zmap, a.disparity, a.counts = _lib.ptr(zmap[e]), _lib.ptr(disp[e]), _lib.ptr(counts[e])
        if camera:
            a.host_arrays[2][0] = view is not None
            a.views = None if view is None else _host_ptr(view, ctypes.c_double)
            a.bg_valid, a.bg_corr, a.bg_counts = _lib.ptr(bg_valid), _lib.ptr(bg_corr[e]), _lib.ptr(bg_counts[e:])
        _lib.check(g.L.dh_reproject(ctypes.byref(a)), "dh_reproject")
    counts_h = counts.cpu()
    _check_infill(counts_h[:, 3])
    placed = (lambda t: t) if g.on_device else (lambda t: t.cpu())
    if camera:
        bg_h = bg_counts.cpu().tolist()
        out = [(disp[e][None, None].to(g.out_dev), placed(bg_corr[e, :nb]), placed(torch.full((nb,), p.N, dtype=torch.uint8, device=dev)))
               for e, nb in enumerate(bg_h)]
    else:
        empty = torch.zeros((0, 4), dtype=torch.int64, device=dev if g.on_device else "cpu")
        no_inst = torch.zeros(0, dtype=torch.uint8, device=empty.device)
        out = [(disp[None].to(g.out_dev), empty) + ((no_inst,) if p.return_instances else ())] * K
    if not g.return_debug:
        return out
    dbg = _empty_debug(g, camera or p.with_table or p.return_instances)
    if camera:
        dbg.update(zmap=zmap, counts=counts_h, vacated=covered.reshape(res, res).to(torch.uint8),
                   row_background=[torch.ones(nb, dtype=torch.uint8, device=dev) for nb in bg_h], n_background=[int(v) for v in bg_h],
                   bg_corr=bg_corr, bg_counts=bg_counts, bg_valid=bg_valid)
    else:
        dbg.update(zmap=zmap.expand(K, -1, -1), counts=counts_h.expand(K, -1).contiguous(), vacated=_vacated_u8(p, g))
    return out, dbg


def _bone_rows(p, fg_pix, dev):
    """The rows and weights of a call with a `Bend`: rows [K][Nk][B][16] f64 (host) -- B = p.n_bones; an instance with fewer
    bones, or an ordinary transform, pads with copies of its bone 0 -- and bone_w [K][n_pts][B] f32 on the device: the weights of
    a `Bend` gathered at its instance's pixels (fg_pix holds the pixel list of every kept mask), 1 on bone 0 for an ordinary
    transform, 0 on the padding."""
    K, Nk, B = len(p.edits), len(p.caller), p.n_bones
    flat = []
    bone_w = torch.zeros((K, p.n_pts, B), dtype=torch.float32, device=dev)
    bone_w[:, :, 0] = 1.0          # (an ordinary transform: bone 0; a Bend overwrites its slice)
    pix_of = {}                    # the pixel indices of a kept mask, once per call
    for e, tfs in enumerate(p.edits):
        for j, n in enumerate(p.caller):
            tf = tfs[n]
            bones = list(tf.bones) if isinstance(tf, Bend) else [tf]
            flat += bones + [bones[0]] * (B - len(bones))
            if isinstance(tf, Bend):
                a, b, o = int(p.inst_start[j]), int(p.inst_start[j + 1]), int(p.inst_obj[j])
                if o not in pix_of:
                    pix_of[o] = fg_pix[int(p.obj_start[o]):int(p.obj_start[o + 1])].long()
                w = tf.weights.to(dev).reshape(len(bones), -1)
                bone_w[e, a:b, :len(bones)] = w[:, pix_of[o]].t()
    return _similarity_rows(flat), bone_w


def _run_objects(p, g):
    """The kind with foreground points: the pixel lists of the kept masks, the buffers, dh_reproject on the plan's record, then
    the results and the debug dict."""
    dev, res, K, L = g.dev, g.res, g.K, g.L
    R2, Mk, Nk, n_fg, n_pts, cap = res * res, len(p.kept), len(p.caller), p.n_fg, p.n_pts, p.cap
    camera, donor = p.cams is not None, p.donor is not None
    masks_u8 = p.masks_u8.to(dev).contiguous()
    obj_start, inst_start = p.obj_start, p.inst_start
    fg_pix = torch.empty(max(R2, n_fg), dtype=torch.int32, device=dev)      # (beyond R2 only with a donor: its pixels are another image's)
    n_dev = torch.zeros(Mk, dtype=torch.int32, device=dev)
    ws_small = torch.empty(4096, dtype=torch.uint8, device=dev)
    for j, m in enumerate(p.kept):              # disjoint masks: the slices fill fg_pix[0 .. n_fg), n_fg <= R2
        _lib.check(L.dh_fg_pixel_list(_lib.ptr(masks_u8[m]), res, _lib.ptr(fg_pix[int(obj_start[j]):]), _lib.ptr(n_dev[j:]),
                                      _lib.ptr(ws_small), ws_small.numel(), g.st), "dh_fg_pixel_list")
    a = reproject_record(p, K)
    _workspace(a, g)
    _geometry(a, g)
    zmap = torch.empty((K, res, res), dtype=torch.float32, device=dev)
    raw = torch.empty((K, res, res), dtype=torch.uint8, device=dev)
    clean = torch.empty((K, res, res), dtype=torch.uint8, device=dev)
    disp = torch.empty((K, res, res), dtype=torch.float32, device=dev)
    vis = torch.empty((K, n_pts), dtype=torch.uint8, device=dev)
    txy = torch.empty((K, n_pts, 2), dtype=torch.int32, device=dev)
    corr = torch.empty((K, cap, 4), dtype=torch.int64, device=dev)
    counts = torch.zeros((K, 4), dtype=torch.int32, device=dev)
    bone_w = None
    if p.bent:
        rows, bone_w = _bone_rows(p, fg_pix, dev)
    else:
        rows = _similarity_rows([tfs[n] for tfs in p.edits for n in p.caller])    # edit-major, K x Nk rows (C-contiguous)
    a.depth, a.fg_pix, a.xforms_host = _lib.ptr(g.d), _lib.ptr(fg_pix), _host_ptr(rows, ctypes.c_double)
    a.zmap, a.raw_mask, a.clean_mask, a.disparity = _lib.ptr(zmap), _lib.ptr(raw), _lib.ptr(clean), _lib.ptr(disp)
    a.vis, a.target_xy, a.corr, a.counts, a.bone_w = _lib.ptr(vis), _lib.ptr(txy), _lib.ptr(corr), _lib.ptr(counts), _lib.ptr(bone_w)
    corr_inst = None
    if p.with_table:
        corr_inst = torch.empty((K, cap), dtype=torch.uint8, device=dev)
        a.corr_inst = _lib.ptr(corr_inst)
    if donor:
        dd = p.donor[0].detach().to(dev, torch.float32).contiguous()
        a.donor_depth = _lib.ptr(dd)
    if camera:
        # the view rows (host), the pixels that show the background (the union of the host's masks and the removed masks is
        # in-painted in bg_depth), and the background rows' buffers
        views = np.zeros((K, SIMILARITY_ROW), dtype=np.float64)
        for e, c in enumerate(p.cams):
            if c is not None:
                views[e] = view_row(c)
        bg_valid = (~p.covered.to(dev)).to(torch.uint8).contiguous()
        bg_corr = torch.empty((K, R2, 4), dtype=torch.int64, device=dev)
        bg_counts = torch.zeros(K, dtype=torch.int32, device=dev)
        a.views, a.bg_valid, a.bg_corr, a.bg_counts = _host_ptr(views, ctypes.c_double), _lib.ptr(bg_valid), _lib.ptr(bg_corr), _lib.ptr(bg_counts)
    _lib.check(L.dh_reproject(ctypes.byref(a)), "dh_reproject")
    row_donor = donor_rows(corr_inst, [p.inst[n] for n in p.caller], p.M) if donor else None
    if p.with_table and p.caller != list(range(Nk)):         # instances of empty masks were dropped: the indices reported stay the caller's
        lut = torch.zeros(256, dtype=torch.uint8)          # (256 entries: the rows past the counts are not written)
        lut[:Nk] = torch.tensor(p.caller, dtype=torch.uint8)
        corr_inst = lut.to(dev)[corr_inst.long()]
    counts_h = counts.cpu()
    _check_infill(counts_h[:, 3])
    out = []
    bg_h = bg_counts.cpu().tolist() if camera else None
    row_background = []
    placed = (lambda t: t) if g.on_device else (lambda t: t.cpu())
    for e in range(K):
        n = int(counts_h[e, 0])
        rows_e, inst_e = corr[e, :n], (corr_inst[e, :n] if p.return_instances else None)
        if camera:
            # the background rows behind the instance rows, instance index N
            nb = int(bg_h[e])
            rows_e = torch.cat([rows_e, bg_corr[e, :nb]])
            inst_e = torch.cat([inst_e, torch.full((nb,), p.N, dtype=torch.uint8, device=dev)])
            row_background.append(torch.cat([torch.zeros(n, dtype=torch.uint8, device=dev), torch.ones(nb, dtype=torch.uint8, device=dev)]))
        out.append((disp[e][None, None].to(g.out_dev), placed(rows_e)) + ((placed(inst_e),) if p.return_instances else ()))
    if not g.return_debug:
        return out
    dbg = dict(zmap=zmap, raw_mask=raw, clean_mask=clean, vis=vis, target_xy=txy, counts=counts_h,
               fg_pix=fg_pix[:n_fg], corr_dev=corr, obj_start=obj_start)
    if p.with_table:
        dbg.update(corr_inst=corr_inst, inst_start=inst_start)
    if p.removed_given:
        dbg.update(vacated=_vacated_u8(p, g))
    if row_donor is not None:
        dbg.update(row_donor=row_donor)
    if camera:
        dbg.update(row_background=row_background, n_background=[int(v) for v in bg_h], bg_corr=bg_corr, bg_counts=bg_counts,
                   bg_valid=bg_valid)
    return out, dbg


def reproject(depth, bg_depth, fg_masks, intrinsics, edits, *, instances=None, removed_masks=None, donor_depth=None,
              donor_masks=None, cameras=None, use_input_depth_normalization=False, return_debug=False,
              device_correspondences=False, footprints=False, footprint_max_ratio=None, return_instances=False, what=None,
              infill_border="zero", view_surfaces=False, view_surface_max_ratio=None):
    """K edits of one image (not in the reference, which has the one-object, one-edit call): `reproject_plan` decides on the
    host, `_run_plan` allocates and launches.  The named functions below are this call with fewer keywords.

    Objects.  fg_masks: M pairwise disjoint [1,1,H,W] masks (1 <= M <= 8); bg_depth: the depth with ALL objects removed; edits: K
    lists of M (rot_angle_deg, rot_axis[3], translation[3]) or (rot_angle_deg, rot_axis[3], translation[3], scale, pivot), one
    per mask.  Object m turns about the centroid of its own masked points, then moves.  With a 5-tuple it is first scaled --
    scale: None (= 1), one positive float or three (sx, sy, sz) along the camera axes of `depth_to_world_coords`, applied to the
    offsets from the pivot BEFORE the rotation, so a non-uniform scale of a turned object stretches along the un-turned camera
    axes -- and pivot (None = the centroid; else a point in the coordinates `depth_to_world_coords` returns, see
    `pivot_at_pixel`) replaces the centroid for the scale and the turn.  Scale 1 with pivot None is the 3-tuple's result bit for
    bit.  A magnified object leaves gaps between its points; the mask CLOSE bridges them only up to its element, res // 50 (as
    when an object moves towards the camera).  The point list is the background pixels, then the points of object 0 in row-major
    order, then object 1, ...: one z-buffer over all of it, so the objects occlude the background and each other, and equal
    depths go to the earlier object.  Mask clean-up, correspondence filter, in-fill and normalisation see the union.  Empty masks
    are dropped (with their transforms); all empty = the empty-mask result, the normalised input disparity without
    correspondences.  ValueError for overlapping masks, M > 8, an edit that does not have M transforms, and, naming the edit and
    the object, for a malformed transform (check_transform).

    Returns a list of K (disparity [1,1,H,W] f32 on depth.device, correspondences [R,4] int64 (ox, oy, tx, ty) on the CPU, in
    point-list order), plus a dict of the intermediate device tensors when return_debug is set (obj_start: the M' + 1 offsets of
    the kept objects' slices in fg_pix / vis / target_xy).  The reference hands the correspondences over as a CPU tensor
    (depth_transform.py:339-343) and so does `transform_depth`; device_correspondences=True leaves them where the kernels wrote
    them, for callers that feed them straight back to the device (the batched edit path: `process_correspondences` accepts
    either) -- K device-to-host copies and K uploads less per call.

    Footprints (footprint splatting) -- footprints=True: the triangles between neighbouring points of ONE object (of
    one instance) bid in the z-buffer too, so an enlarged or approaching object has no gaps between its points.  The
    correspondences are then one row per foreground-owned target pixel inside the cleaned mask -- (ox, oy) of the owning point,
    (tx, ty) of the pixel -- in ROW-MAJOR TARGET order, and there may be more of them than foreground points (at most H * W).
    footprint_max_ratio: None or a finite float > 1; a triangle whose source depths differ by more than this factor is left out
    (no sheets across a depth step inside one mask).  ValueError for a bad ratio or a ratio without footprints.

    Copies (DESIGN.md "Object copies") -- instances: None, or a list of N mask indices, M <= N <= 8, naming every mask at least
    once.  Instance n draws the points of mask instances[n] with transform n of every edit (the edits are then K lists of N
    transforms), about the centroid of that mask (computed once per mask) or its pivot.  The point list is the background, then
    instance 0's points, instance 1's, ...: one z-buffer, equal depths to the earlier instance; a source pixel has one row per
    visible, kept instance.  One table serves all K edits.  ValueError naming the instance (or the edit) for a bad table or an
    edit that does not have N transforms.  The debug dict gains corr_inst [K, capacity] uint8 (the caller's instance index of
    every correspondence row) and inst_start (the offsets of the kept instances' slices in vis / target_xy); instances=None is
    the call without the table, byte for byte.  return_instances=True: every result is (disparity, correspondences [R,4],
    instances [R] uint8 beside them); without an instance table the instance of a row is the index of its mask.

    Removal (DESIGN.md "Object removal") -- removed_masks: None, or a list of R >= 0 [1,1,H,W] masks of the objects the edit
    deletes, pairwise disjoint from each other and from fg_masks; bg_depth has them removed as well (that is its definition).
    A removed object contributes no point, so with M >= 1 every output is byte for byte the output of the call without removed
    masks.  Empty removed masks are dropped; None, [] and all-empty masks are the call without the keyword.  Pure removal --
    fg_masks empty (M = 0) and at least one non-empty removed mask: the edits are K empty transform lists, and every one of the K
    results is the re-projection of the background ALONE (z-buffer over the H * W background points, in-fill of the pixels no
    point owns, normalisation with the optional input bounds; computed once), with no correspondences and zero masks.  That is
    not the empty-mask result (the normalised INPUT disparity, object included), which stays what it is.  ValueError naming the
    mask: a removed mask of another size, one that overlaps a foreground mask or another removed mask, M = 0 without a
    non-empty removed mask, transforms or instances given for M = 0 (`what`: the caller's name in these two).  The debug dict
    gains vacated ([H, W] uint8 on the device: the union of the removed masks).

    Insertion (DESIGN.md "Object insertion") -- donor_depth, donor_masks: the [1,1,H,W] depth of a SECOND image of the host's
    resolution and intrinsics, and D >= 1 pairwise disjoint masks of objects in it.  The edit's objects are then the host's M
    masks (0 .. M - 1) followed by the donor's D masks (M .. M + D - 1), M + D <= 8: transforms and instances speak about that
    list.  A donor object's points are the unprojection of donor_depth at its mask's pixels, its centroid the sequential-f32
    centroid of those points; a pivot is a point of the shared camera coordinates.  From there on everything is shared (one
    z-buffer, masks, visibility, in-fill, normalisation).  Donor masks may overlap host masks, removed masks and each other's
    image position freely -- they are pixels of another image.  M = 0 with a donor is the pure insertion (bg_depth: the host
    depth, or the depth with the removed masks removed).  A row of a donor instance carries its source pixel IN THE DONOR IMAGE;
    a donor call always returns the instance array (return_instances is implied), and "row r is a donor row" means
    instances[corr_inst[r]] >= M (`donor_rows`).  The debug dict gains row_donor [K, capacity] uint8 (device).  No relative depth
    scale is estimated: the caller brings `scale`.  ValueError (check_donor); NotImplementedError for footprints with a donor
    (the pixel -> list-position inverse of the triangles is ambiguous when two images share pixel indices).  No donor -- None,
    or donor masks that are all empty -- is the call without the keywords, byte for byte, with the same launches.

    Camera moves (DESIGN.md "Camera moves") -- cameras: None, or a list of K entries, one camera (`check_camera`) or None per
    edit.  In an edit with a camera every point of the list, background included, is seen from the moved viewpoint: the points
    that leave the frame are dropped (no clamp onto the border), the pixels no point reaches are in-filled (against zero beyond
    the image border unless infill_border="reflect", below), and the background yields correspondence rows of its own -- a
    background pixel outside the host's foreground and removed masks whose point owns a target pixel outside the cleaned mask.
    A camera call returns the instance array (return_instances is implied): the instance rows first, in the order they always
    had, then the background rows in ascending source pixel order with instance index N (the number of instances).  An edit
    without a camera in the same call is what it is in a call of its own, byte for byte, and has no background rows.  The pure
    camera move is fg_masks = [] with K empty transform lists (bg_depth: the depth, or the depth with the removed masks
    removed): every row is a background row.  The debug dict gains row_background (K uint8 tensors beside the returned rows: 1 =
    a background row) and n_background (K ints), bg_corr and bg_counts.  ValueError (`check_camera`) naming the call and the
    edit, NotImplementedError for footprints with a camera.  cameras=None, or all None, is the call without the keyword, byte
    for byte, with the same launches.

    In-fill border (DESIGN.md "In-fill border") -- infill_border: "zero" (or None; the default: a neighbour beyond the frame is a
    known 0, which pulls an in-fill region that touches the frame towards disparity 0 there) or "reflect" (the mirror ghost
    cell: zero normal derivative at the frame, the diagonal of an unknown is the number of its neighbours inside the image).
    One setting per call.  It changes the disparity inside in-fill components that touch the frame and nothing else: every
    integer output stays, and "zero" is the call without the keyword, byte for byte, through the same entries.  Composes with
    everything above.  ValueError (`check_infill_border`) for any other value.

    View surfaces (DESIGN.md "View surfaces") -- view_surfaces=True: in an edit WITH a camera the whole scene is splatted as
    triangles -- between neighbouring points of one instance (the footprint rules, vertices after the view) and over every
    source quad of the background -- beside the points, in the one z-buffer; so a camera that moves closer or orbits leaves
    unowned only what it really uncovers, and a magnified near surface does not let the far one show through.  Such an edit
    takes its rows per target pixel, row-major: the instance rows (the owning point's source pixel, the pixel), then the
    background rows (the owning background pixel, the pixel; the owner outside the host's and the removed masks, the pixel
    outside the cleaned mask).  vis = the point owns a pixel.  view_surface_max_ratio: None or a finite float > 1, the
    depth-ratio guard of the triangles (instances: on depth; background: on bg_depth).  The setting acts only where there is a
    view: an edit without a camera, and a call without any, is what it is without the setting, byte for byte.  ValueError
    (`check_view_surfaces`); NotImplementedError with a donor.  `footprints=True` with a camera stays refused.

    Bend edits (DESIGN.md "Bend edits") -- a `Bend` in place of an instance's transform tuple, in any edit, for a host or a donor
    instance: the instance carries up to 4 transforms (bones) and a weight per pixel and bone, and each of its points goes to
    the weighted sum of where the bones put it (linear-blend skinning; `bend_chain` builds one from a line across the object).
    Everything after the point transform sees points as before, so copies, removal, a donor, cameras, view surfaces, the
    in-fill border and footprints compose; with footprints the triangles between neighbouring points stretch over the outside
    of the bend.  Plain skinning is not volume preserving: two bones about one pivot pull the band between them towards the
    chord (more bones, smaller steps).  ValueError (`check_bend`) naming the edit and the instance.  A call without a `Bend`
    is the call it was: the same entry, the same bytes.

    Every refusal precedes the first launch of the library (they are `reproject_plan`'s)."""
    p = reproject_plan(depth, fg_masks, edits, instances=instances, removed_masks=removed_masks, donor_depth=donor_depth,
                       donor_masks=donor_masks, cameras=cameras, footprints=footprints, footprint_max_ratio=footprint_max_ratio,
                       return_instances=return_instances, what=what, infill_border=infill_border, view_surfaces=view_surfaces,
                       view_surface_max_ratio=view_surface_max_ratio)
    return _run_plan(p, depth, bg_depth, intrinsics, use_input_depth_normalization, return_debug, device_correspondences)


def reproject_edits(depth, bg_depth, fg_mask, intrinsics, transforms, use_input_depth_normalization=False,
                    return_debug=False, device_correspondences=False, footprints=False, footprint_max_ratio=None):
    """`reproject` for one object: one mask, and one transform (not a list of them) per edit."""
    return reproject(depth, bg_depth, [fg_mask], intrinsics, [[tf] for tf in transforms],
                     use_input_depth_normalization=use_input_depth_normalization, return_debug=return_debug,
                     device_correspondences=device_correspondences, footprints=footprints, footprint_max_ratio=footprint_max_ratio)


def reproject_object_edits(depth, bg_depth, fg_masks, intrinsics, edits, use_input_depth_normalization=False,
                           return_debug=False, device_correspondences=False, footprints=False, footprint_max_ratio=None):
    """`reproject` for M objects, with or without footprints."""
    return reproject(depth, bg_depth, fg_masks, intrinsics, edits, use_input_depth_normalization=use_input_depth_normalization,
                     return_debug=return_debug, device_correspondences=device_correspondences, footprints=footprints,
                     footprint_max_ratio=footprint_max_ratio)


def reproject_instance_edits(depth, bg_depth, fg_masks, intrinsics, edits, instances=None, use_input_depth_normalization=False,
                             return_debug=False, device_correspondences=False, footprints=False, footprint_max_ratio=None,
                             return_instances=False):
    """`reproject` with an instance table (copies of an object)."""
    return reproject(depth, bg_depth, fg_masks, intrinsics, edits, instances=instances,
                     use_input_depth_normalization=use_input_depth_normalization, return_debug=return_debug,
                     device_correspondences=device_correspondences, footprints=footprints, footprint_max_ratio=footprint_max_ratio,
                     return_instances=return_instances)


def reproject_removal_edits(depth, bg_depth, fg_masks, intrinsics, edits, instances=None, removed_masks=None,
                            use_input_depth_normalization=False, return_debug=False, device_correspondences=False,
                            footprints=False, footprint_max_ratio=None, return_instances=False):
    """`reproject` for an edit that also deletes the objects of removed_masks."""
    return reproject(depth, bg_depth, fg_masks, intrinsics, edits, instances=instances, removed_masks=removed_masks,
                     use_input_depth_normalization=use_input_depth_normalization, return_debug=return_debug,
                     device_correspondences=device_correspondences, footprints=footprints, footprint_max_ratio=footprint_max_ratio,
                     return_instances=return_instances)


def reproject_donor_edits(depth, bg_depth, fg_masks, intrinsics, edits, instances=None, removed_masks=None, donor_depth=None,
                          donor_masks=None, use_input_depth_normalization=False, return_debug=False,
                          device_correspondences=False, footprints=False, footprint_max_ratio=None, return_instances=False):
    """`reproject` for an edit that also places objects of a donor image."""
    return reproject(depth, bg_depth, fg_masks, intrinsics, edits, instances=instances, removed_masks=removed_masks,
                     donor_depth=donor_depth, donor_masks=donor_masks, use_input_depth_normalization=use_input_depth_normalization,
                     return_debug=return_debug, device_correspondences=device_correspondences, footprints=footprints,
                     footprint_max_ratio=footprint_max_ratio, return_instances=return_instances)


def reproject_camera_edits(depth, bg_depth, fg_masks, intrinsics, edits, instances=None, removed_masks=None, donor_depth=None,
                           donor_masks=None, use_input_depth_normalization=False, return_debug=False,
                           device_correspondences=False, footprints=False, footprint_max_ratio=None, return_instances=False,
                           cameras=None):
    """`reproject` for edits that may also move the viewpoint."""
    return reproject_border_edits(depth, bg_depth, fg_masks, intrinsics, edits, instances, removed_masks, donor_depth, donor_masks,
                                  use_input_depth_normalization, return_debug, device_correspondences, footprints,
                                  footprint_max_ratio, return_instances, cameras)


def reproject_border_edits(depth, bg_depth, fg_masks, intrinsics, edits, instances=None, removed_masks=None, donor_depth=None,
                           donor_masks=None, use_input_depth_normalization=False, return_debug=False,
                           device_correspondences=False, footprints=False, footprint_max_ratio=None, return_instances=False,
                           cameras=None, infill_border="zero"):
    """`reproject` with the image border of the in-fill ("zero" or "reflect"); `reproject_camera_edits` is its call without it."""
    return reproject_surface_edits(depth, bg_depth, fg_masks, intrinsics, edits, instances, removed_masks, donor_depth, donor_masks,
                                   use_input_depth_normalization, return_debug, device_correspondences, footprints,
                                   footprint_max_ratio, return_instances, cameras, infill_border)


def reproject_surface_edits(depth, bg_depth, fg_masks, intrinsics, edits, instances=None, removed_masks=None, donor_depth=None,
                            donor_masks=None, use_input_depth_normalization=False, return_debug=False,
                            device_correspondences=False, footprints=False, footprint_max_ratio=None, return_instances=False,
                            cameras=None, infill_border="zero", view_surfaces=False, view_surface_max_ratio=None):
    """`reproject` with view surfaces (the scene as triangles in the edits with a camera); `reproject_border_edits` is its call
    without them."""
    return reproject(depth, bg_depth, fg_masks, intrinsics, edits, instances=instances, removed_masks=removed_masks,
                     donor_depth=donor_depth, donor_masks=donor_masks, cameras=cameras,
                     use_input_depth_normalization=use_input_depth_normalization, return_debug=return_debug,
                     device_correspondences=device_correspondences, footprints=footprints, footprint_max_ratio=footprint_max_ratio,
                     return_instances=return_instances, infill_border=infill_border, view_surfaces=view_surfaces,
                     view_surface_max_ratio=view_surface_max_ratio)


INFILL_BARRIER_TIMEOUT, INFILL_NOT_CONVERGED, INFILL_BREAKDOWN = -1, -2, -3      # counts[..., 3] < 0 (geometry.hip)


def reproject_bend_edits(depth, bg_depth, fg_masks, intrinsics, edits, instances=None, removed_masks=None, donor_depth=None,
                         donor_masks=None, use_input_depth_normalization=False, return_debug=False,
                         device_correspondences=False, footprints=False, footprint_max_ratio=None, return_instances=False,
                         cameras=None, infill_border="zero", view_surfaces=False, view_surface_max_ratio=None):
    """`reproject` for edits in which an instance may be a `Bend`; `reproject_surface_edits` is its call without one."""
    return reproject(depth, bg_depth, fg_masks, intrinsics, edits, instances=instances, removed_masks=removed_masks,
                     donor_depth=donor_depth, donor_masks=donor_masks, cameras=cameras,
                     use_input_depth_normalization=use_input_depth_normalization, return_debug=return_debug,
                     device_correspondences=device_correspondences, footprints=footprints, footprint_max_ratio=footprint_max_ratio,
                     return_instances=return_instances, infill_border=infill_border, view_surfaces=view_surfaces,
                     view_surface_max_ratio=view_surface_max_ratio)


class InfillNotConverged(RuntimeError):
    """The harmonic in-fill's CG left without reaching its tolerance: at the iteration cap, or on a breakdown."""


def _check_infill(iterations):
    """counts[..., 3] = CG iterations of the harmonic in-fill.  Negative = the result is not valid, an error and never a hang
    or a silently unconverged field: -1 = the multi-workgroup solver's bounded grid barrier ran out (its workgroups were not
    co-resident: CU masks, another process holding the chip); -2 = a solver reached its iteration cap with the residual still
    above the tolerance; -3 = the pipelined recurrence broke down (a step length that is not positive and finite)."""
    if not bool((iterations < 0).any()):
        return
    if bool((iterations == INFILL_BARRIER_TIMEOUT).any()):
        raise RuntimeError("harmonic in-fill: the multi-workgroup CG's grid barrier timed out (workgroups not co-resident); "
                           "the result is not valid")
    if bool((iterations == INFILL_NOT_CONVERGED).any()):
        raise InfillNotConverged("harmonic in-fill: CG reached its iteration cap before the residual met the tolerance; "
                                 "the result is not valid")
    if bool((iterations == INFILL_BREAKDOWN).any()):
        raise InfillNotConverged("harmonic in-fill: the pipelined CG broke down (step length not positive and finite); "
                                 "the result is not valid")
    raise RuntimeError(f"harmonic in-fill: unknown failure code {int(iterations.min())}; the result is not valid")


def pivot_at_pixel(depth, intrinsics, x, y):
    """The point of pixel (x, y) = (column, row) of `depth` [1,1,H,W] in the coordinates `depth_to_world_coords` returns:
    three float32 values (a CPU tensor), to hand to a transform as `pivot` -- "turn about this pixel"."""
    h, w = depth.shape[-2:]
    x, y = int(x), int(y)
    if not (0 <= x < w and 0 <= y < h):
        raise ValueError(f"pivot_at_pixel: pixel ({x}, {y}) is outside the {w} x {h} depth map")
    return depth_to_world_coords(depth, intrinsics)[y, x].detach().to("cpu", torch.float32).clone()


def transform_depth_footprints(depth, bg_depth, fg_mask, intrinsics, rot_angle=None, rot_axis=None, translation=None,
                               use_input_depth_normalization=False, scale=None, pivot=None, footprints=False,
                               footprint_max_ratio=None):
    """`transform_depth_pc` with the footprint settings of `reproject` (point mode only).  `transform_depth` and
    `transform_depth_pc` keep the parameter lists they have; `transform_depth_pc` is the footprints-off call of this one."""
    if rot_angle is None:
        rot_angle = 0.0
    if rot_axis is None:
        rot_axis = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float32)
    if translation is None:
        translation = torch.tensor([0.0, 0.0, 0.0], dtype=torch.float32)
    (disp, corr), = reproject_edits(depth, bg_depth, fg_mask, intrinsics, [(rot_angle, rot_axis, translation, scale, pivot)],
                                    use_input_depth_normalization, footprints=footprints, footprint_max_ratio=footprint_max_ratio)
    return disp, corr


def transform_depth_pc(depth, bg_depth, fg_mask, intrinsics, rot_angle=None, rot_axis=None, translation=None,
                       use_input_depth_normalization=False, scale=None, pivot=None):
    """The reference's transform_depth_pc (its parameters are a prefix); scale / pivot: see `reproject`."""
    return transform_depth_footprints(depth, bg_depth, fg_mask, intrinsics, rot_angle, rot_axis, translation,
                                      use_input_depth_normalization, scale, pivot)


MESH_BLUR_RADIUS = 1e-5      # depth_transform.py:152


def _mesh_similarity(scale, pivot, what):
    """scale / pivot of a mesh-mode call: checked as the point mode checks them (ValueError), then a scale other than 1 is
    refused -- the mesh path has no scale.  Returns the pivot as None or three float32 values.  Host only."""
    _, _, _, sc, pv = check_transform((0.0, None, None, scale, pivot), what)
    if sc != [1.0, 1.0, 1.0]:
        raise NotImplementedError(f"{what}: depth_transform_mode 'mesh' has no scale (got scale={scale!r}); use 'pc'")
    return pv


def mesh_xform(depth, fg_mask, intrinsics, rot_angle, rot_axis, translation, pivot=None):
    """The 11 float32 numbers dh_mesh_reproject takes: unit axis, cos, sin, translation, centroid of the masked
    points (transform_points, depth_transform.py:438-458; the centroid is the sequential float32 mean the point
    path uses -- torch's own reduction order is not specified).  pivot (three float32 values) takes the centroid's place."""
    pivot = _mesh_similarity(None, pivot, "mesh_xform")
    dev = _compute_device(depth)
    res = depth.shape[-1]
    d = depth.detach().to(dev, torch.float32).contiguous()
    fg_pix = torch.nonzero((fg_mask.detach().to(dev)[0, 0] > 0.5).reshape(-1)).to(torch.int32).reshape(-1).contiguous()
    gx, gy = _grids(res, res, dev)
    ifx, ify = _inv_focal(intrinsics)
    cen = torch.empty(3, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dh_masked_centroid(_lib.ptr(d), _lib.ptr(fg_pix), fg_pix.numel(), res, _lib.ptr(gx), _lib.ptr(gy),
                                             ifx, ify, _lib.ptr(cen), _lib.stream_ptr()), "dh_masked_centroid")
    ax = np.asarray(rot_axis.detach().cpu().numpy() if isinstance(rot_axis, torch.Tensor) else rot_axis, dtype=np.float32)
    ax = (ax / np.float32(np.linalg.norm(ax))).astype(np.float32)
    ang = np.float32(rot_angle.item() if isinstance(rot_angle, torch.Tensor) else rot_angle)
    theta = np.float32(ang * np.float32(np.pi / 180.0))
    tr = translation.detach().cpu().numpy() if isinstance(translation, torch.Tensor) else np.asarray(translation)
    c = cen.cpu().numpy() if pivot is None else np.asarray(pivot, dtype=np.float32)
    return np.array([ax[0], ax[1], ax[2], np.cos(theta), np.sin(theta), tr[0], tr[1], tr[2], c[0], c[1], c[2]],
                    dtype=np.float32)


def transform_depth_mesh(depth, bg_depth, fg_mask, intrinsics, rot_angle=None, rot_axis=None, translation=None,
                         use_input_depth_normalization=False, return_debug=False, scale=None, pivot=None, footprints=False,
                         footprint_max_ratio=None):
    """depth_transform.py:91-195 with our own HIP triangle rasteriser in place of pytorch3d (parity unpinned).
    pivot: None or three floats, the point the object turns about in place of its centroid; a scale other than 1 raises
    NotImplementedError before any device work (the mesh path has no scale), and so does footprints=True (point mode only).
    The mesh path in-fills against zero beyond the image border and has no setting for it (`mesh_has_no_infill_border`)."""
    mesh_has_no_footprints(footprints, footprint_max_ratio, "transform_depth_mesh")
    pivot = _mesh_similarity(scale, pivot, "transform_depth_mesh")
    if depth.dim() != 4 or depth.shape[0] != 1:
        raise ValueError("Only batch size 1 is supported")
    res = depth.shape[-1]
    if depth.shape[-2] != res:
        raise RuntimeError("square depth maps only")
    out_dev = depth.device
    dev = _compute_device(depth)
    d = depth.detach().to(dev, torch.float32).contiguous()
    bounds = None
    if use_input_depth_normalization:
        disp_in = 1.0 / d
        bounds = torch.stack([disp_in.min(), disp_in.max()]).to(torch.float32).contiguous()
    mask = (fg_mask.detach().to(dev)[0, 0] > 0.5)
    if not bool(mask.any()):
        lo_hi = None if bounds is None else (bounds[0], bounds[1])
        return normalize_depth(1.0 / d, bounds=lo_hi).to(out_dev), torch.zeros((0, 4), dtype=torch.int64)
    if rot_angle is None:
        rot_angle = 0.0
    if rot_axis is None:
        rot_axis = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float32)
    if translation is None:
        translation = torch.tensor([0.0, 0.0, 0.0], dtype=torch.float32)
    xf = mesh_xform(depth, fg_mask, intrinsics, rot_angle, rot_axis, translation, pivot)
    L = _lib.lib()
    bg = bg_depth.detach().to(dev, torch.float32).contiguous()
    m8 = mask.to(torch.uint8).contiguous()
    gx, _ = _grids(res, res, dev)
    lin01 = torch.linspace(0, 1, res, dtype=torch.float32).to(dev)
    ifx, _ = _inv_focal(intrinsics)
    f = float(intrinsics.detach().to("cpu", torch.float32)[0, 0])
    R2 = res * res
    zmap = torch.empty(R2, dtype=torch.float32, device=dev)
    disp = torch.empty(R2, dtype=torch.float32, device=dev)
    flag = torch.empty(R2, dtype=torch.uint8, device=dev)
    corr = torch.empty((R2, 4), dtype=torch.int64, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    nb = ctypes.c_size_t()
    _lib.check(L.dh_mesh_workspace_bytes(res, ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    xf_c = (ctypes.c_float * 11)(*[float(v) for v in xf])
    _lib.check(L.dh_mesh_reproject(_lib.ptr(d), _lib.ptr(bg), _lib.ptr(m8), res, _lib.ptr(gx), _lib.ptr(lin01), ifx, f,
                                   ctypes.cast(xf_c, ctypes.c_void_p), _lib.ptr(bounds), float(MESH_BLUR_RADIUS),
                                   _lib.ptr(zmap), _lib.ptr(disp), _lib.ptr(flag), _lib.ptr(corr), _lib.ptr(counts),
                                   _lib.ptr(ws), nb.value, _lib.stream_ptr()), "dh_mesh_reproject")
    n = int(counts[0].item())
    out = disp.view(1, 1, res, res).to(out_dev), corr[:n].cpu()
    if return_debug:
        return out + (dict(zmap=zmap.view(res, res), fg_flag=flag.view(res, res), xform=xf),)
    return out


def transform_depth(depth, bg_depth, fg_mask, intrinsics, rot_angle=None, rot_axis=None, translation=None,
                    use_input_depth_normalization=False, depth_transform_mode="pc", scale=None, pivot=None):
    """The reference's transform_depth (depth_transform.py:73-89): its signature is a prefix and its return value unchanged.
    scale / pivot (not in the reference): see `reproject`; mesh mode takes a pivot and refuses a scale.
    (Footprint splatting: `transform_depth_footprints`, point mode only.)"""
    if depth_transform_mode == "pc":
        return transform_depth_pc(depth, bg_depth, fg_mask, intrinsics, rot_angle, rot_axis, translation,
                                  use_input_depth_normalization, scale, pivot)
    if depth_transform_mode == "mesh":
        return transform_depth_mesh(depth, bg_depth, fg_mask, intrinsics, rot_angle, rot_axis, translation,
                                    use_input_depth_normalization, scale=scale, pivot=pivot)
    raise ValueError(f"Unknown depth transform mode '{depth_transform_mode}'.")


def laplacian_depth_blend(depth, bg_depth, fg_mask, dilate_iterations=15, return_iterations=False, infill_border="zero"):
    """set_foreground's background-depth update (diffusion_handles.py:90-111): `depth` everywhere except
    inside the dilated foreground mask, where the background depth's Laplacian is integrated from the
    surrounding depth values.  [1,1,H,W] tensors in, [1,1,H,W] float32 out (on depth.device); with return_iterations also
    the CG iteration count of the solve.  infill_border: "zero" (or None; the reference's blend) or "reflect" -- the diagonal of
    an unknown is the number of its neighbours inside the image and the Laplacian of bg_depth uses replicate padding, so a
    mismatch depth - bg_depth around a mask that touches the frame is no longer forced to 0 there (`reproject`)."""
    border = check_infill_border(infill_border, "laplacian_depth_blend")
    res = depth.shape[-1]
    if depth.shape[-2] != res:
        raise RuntimeError("square depth maps only")
    out_dev = depth.device
    dev = _compute_device(depth)
    L = _lib.lib()
    d = depth.detach().to(dev, torch.float32).contiguous()
    bg = bg_depth.detach().to(dev, torch.float32).contiguous()
    m = (fg_mask.detach().to(dev) != 0).to(torch.uint8).contiguous()
    out = torch.empty((res, res), dtype=torch.float32, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    nbytes = ctypes.c_size_t()
    _lib.check(L.dh_laplacian_blend_workspace_bytes(res, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    args = (_lib.ptr(d), _lib.ptr(bg), _lib.ptr(m), res, int(dilate_iterations), _lib.ptr(out), _lib.ptr(counts), _lib.ptr(ws),
            nbytes.value, _lib.stream_ptr())
    if border:
        _lib.check(L.dh_laplacian_blend_border(*args, border), "dh_laplacian_blend_border")
    else:
        _lib.check(L.dh_laplacian_blend(*args), "dh_laplacian_blend")
    its = counts[3:4].cpu()
    _check_infill(its)
    if return_iterations:
        return out[None, None].to(out_dev), int(its[0])
    return out[None, None].to(out_dev)
