"""Background lock: hold the latents outside an edit's region to the reconstruction of the input image.

The initial inference walks the reconstruction trajectory of the input image (same noise, same null-text embeddings); it
rides on the identity as `activations.trajectory` (Activations below).  An edit with a lock blends, after every DDIM step, its
latents with the reconstruction's latents of the same step by a per-cell keep map (dh_ddim_cfg_step_locked): 0 inside the
region the edit touches (the edit is free), 1 far from it (the reconstruction, bit for bit), a ramp between.  This module has
the keep map (dh_keep_map), the checks of the configuration keys and arguments (host only), and `composite`, the pixel-level
helper.  DESIGN.md "Background lock" has the rules and the numerics.
"""
import torch

from . import _lib

DEFAULT_DILATE = 2          # cells; a design choice (one cell = 8 pixels, the point mode's mask CLOSE bridges res // 50 pixels):
DEFAULT_FEATHER = 2         # no image quality has been measured with these two
MAX_REACH = 31              # dilate + feather, the library's bound
MAX_ITEMS = 16              # LOCK_MAX_ITEMS of csrc/loop_ops.hip


class Activations(list):
    """The three activation tensors of an identity ([T,C,h,w] each), plus the reconstruction trajectory: float32
    [T,4,s,s], trajectory[t_idx] = the latent after the DDIM step of timestep index t_idx."""
    trajectory = None

    def __init__(self, items=(), trajectory=None):
        super().__init__(items)
        self.trajectory = trajectory


class Lock:
    """A lock as the step kernels read it: keep [s,s] f32 and ref [T,s,s,4] f32 channels-last, both contiguous on the device."""
    __slots__ = ("keep", "ref")

    def __init__(self, keep, ref):
        self.keep, self.ref = keep, ref


def check_reach(dilate, feather, what):
    """dilate / feather as the library takes them: integers >= 0 with dilate + feather <= 31 (ValueError naming `what`)."""
    for name, v in (("dilate", dilate), ("feather", feather)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"{what}: background lock {name} must be an integer >= 0 (cells), got {v!r}")
    if dilate + feather > MAX_REACH:
        raise ValueError(f"{what}: background lock dilate + feather must be <= {MAX_REACH} cells, got {dilate} + {feather}")
    return dilate, feather


def lock_conf(conf, what):
    """The optional top-level conf keys background_lock (absent = false), background_lock_dilate and background_lock_feather
    (cells, absent = 2 each) -> None (lock off) or (dilate, feather).  Host checks only (ValueError naming `what`)."""
    get = conf.get if hasattr(conf, "get") else lambda k, d=None: getattr(conf, k, d)
    on = get("background_lock", False)
    if on is None:
        on = False
    if not isinstance(on, bool):
        raise ValueError(f"{what}: conf background_lock must be true or false, got {on!r}")
    dilate, feather = get("background_lock_dilate", None), get("background_lock_feather", None)
    if not on:
        if dilate is not None or feather is not None:
            raise ValueError(f"{what}: conf background_lock_dilate / background_lock_feather without background_lock: true")
        return None
    dilate = DEFAULT_DILATE if dilate is None else dilate
    feather = DEFAULT_FEATHER if feather is None else feather
    return check_reach(dilate, feather, f"{what}: conf")


def require_trajectory(activations, what):
    """The reconstruction trajectory of an identity; ValueError (never a silent unlocked edit) for activations without one."""
    traj = getattr(activations, "trajectory", None)
    if traj is None:
        raise ValueError(f"{what}: the background lock needs the reconstruction trajectory, and these activations carry none "
                         "(a plain list, or an identity cached before the lock existed): recompute the identity with "
                         "generate_input_image / generate_input_images and pass its activations on unchanged")
    return traj


def check_release_mask(release_mask, res, what):
    """None, or an image of res x res values (leading dimensions of 1 allowed) -> None | [res,res] tensor (ValueError)."""
    if release_mask is None:
        return None
    m = torch.as_tensor(release_mask)
    if m.numel() != res * res or tuple(m.shape[-2:]) != (res, res):
        raise ValueError(f"{what}: release_mask must be one {res} x {res} image, got shape {tuple(m.shape)}")
    return m.reshape(res, res)


def _u8(img, res, device):
    return (torch.as_tensor(img).reshape(res, res).to(device) != 0).to(torch.uint8).contiguous()


def mask_union(fg_masks, res, device):
    """u8 [res,res]: where any of the masks (one tensor or a list) is non-zero; None for no mask."""
    if fg_masks is None:
        return None
    masks = list(fg_masks) if isinstance(fg_masks, (list, tuple)) else [fg_masks]
    if not masks:
        return None
    union = _u8(masks[0], res, device)
    for m in masks[1:]:
        union = union | _u8(m, res, device)
    return union


def keep_map(correspondences, fg_masks, release_mask, res, s, dilate=DEFAULT_DILATE, feather=DEFAULT_FEATHER):
    """The keep map of one edit, float32 [s,s] on the device (dh_keep_map; the rules are in include/diffhandles_hip.h).
    correspondences: [N,4] int64 (ox, oy, tx, ty), N may be 0, or None; fg_masks: None, one mask or a list of masks ([.., res,
    res], non-zero = object); release_mask: None or one more image of area to set free (the shadow an object leaves behind).
    Runs once per edit; nothing comes back to the host."""
    _lib.require_gpu()
    check_reach(dilate, feather, "keep_map")
    if s < 1 or res % s != 0:
        raise ValueError(f"keep_map: res {res} is no multiple of s {s}")
    device = torch.device("cuda", torch.cuda.current_device())
    corr = None if correspondences is None else torch.as_tensor(correspondences)
    if corr is not None:
        if corr.dim() != 2 or corr.shape[1] != 4:
            raise ValueError(f"keep_map: correspondences must be [N,4], got {tuple(corr.shape)}")
        device = corr.device if corr.is_cuda else device
        corr = corr.to(device, torch.int64).contiguous()
    n = 0 if corr is None else corr.shape[0]
    release_mask = check_release_mask(release_mask, res, "keep_map")
    mask = mask_union(fg_masks, res, device)
    release = None if release_mask is None else _u8(release_mask, res, device)
    keep = torch.empty((s, s), dtype=torch.float32, device=device)
    ws = torch.empty(s * s, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().dh_keep_map(_lib.ptr(corr) if n else None, n, _lib.ptr(mask), _lib.ptr(release), int(res), int(s),
                                          int(dilate), int(feather), _lib.ptr(keep), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "dh_keep_map")
    return keep


def prepare_locks(lock, K, device, s, T, what):
    """`lock` of a diffuser call -> a list of K Lock / None.  lock: None, one (keep, trajectory) for all K edits, or a list of K
    such pairs / None (prepared Lock objects pass through).  keep [s,s]; trajectory [T,4,s,s] (Activations.trajectory).  Edits
    that name the same trajectory tensor share one channels-last copy of it; a trajectory that is the view the initial
    inference returned is used in place."""
    if lock is None:
        return [None] * K
    locks = list(lock) if isinstance(lock, list) else [lock] * K
    if len(locks) != K:
        raise ValueError(f"{what}: {len(locks)} locks for {K} edits")
    refs, out = {}, []
    for i, lk in enumerate(locks):
        if lk is None or isinstance(lk, Lock):
            out.append(lk)
            continue
        if not isinstance(lk, (tuple, list)) or len(lk) != 2:
            raise ValueError(f"{what}: lock of edit {i} must be (keep, trajectory)")
        keep, traj = lk
        if tuple(keep.shape) != (s, s):
            raise ValueError(f"{what}: keep map of edit {i} is {tuple(keep.shape)}, the engine runs {(s, s)} latents")
        if traj.dim() != 4 or traj.shape[0] != T or tuple(traj.shape[2:]) != (s, s):
            raise ValueError(f"{what}: trajectory of edit {i} is {tuple(traj.shape)}, expected [{T}, C, {s}, {s}]")
        if id(traj) not in refs:
            refs[id(traj)] = traj.to(device, torch.float32).permute(0, 2, 3, 1).contiguous()
        out.append(Lock(keep.to(device, torch.float32).contiguous(), refs[id(traj)]))
    return out


def composite(edited, original, keep):
    """The input's own pixels outside the region: keep [s,s] up-sampled bilinearly (align_corners=False) to the images'
    resolution, then edited + keep (original - edited).  edited / original: [..,3,H,W] of one shape.  A host helper for
    callers who want identical PIXELS outside the region: the VAE decoder has a global attention block, so locked latents
    alone do not give them."""
    edited, original = torch.as_tensor(edited), torch.as_tensor(original)
    if edited.shape != original.shape or edited.dim() < 3:
        raise ValueError(f"composite: edited {tuple(edited.shape)} and original {tuple(original.shape)} must be images of one shape")
    keep = torch.as_tensor(keep)
    if keep.dim() != 2:
        raise ValueError(f"composite: keep must be [s,s], got {tuple(keep.shape)}")
    H, W = edited.shape[-2:]
    k = torch.nn.functional.interpolate(keep.to(edited.device, torch.float32)[None, None], size=(H, W), mode="bilinear",
                                        align_corners=False)[0, 0].clamp(0.0, 1.0)
    return (edited.float() + k * (original.float() - edited.float())).to(edited.dtype)
