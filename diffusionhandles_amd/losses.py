"""Guidance energy behind the reference's losses.py API, computed by the HIP library.

`process_correspondences` (guided_stable_diffuser.py:490-584) and the two loss functions
(losses.py:4-40) keep their names and argument meaning.  Activations may be given the
reference way ([C,h,w], any float dtype) or channels-last ([h,w,C], the engine's native
layout, `channels_last=True`); the return value of the loss functions is a scalar tensor.
`energy_and_grad` is the fused form the denoising loop uses: it returns the loss and
d(loss)/d(activations) from one call, with no autograd graph.
"""
import ctypes
import weakref

import numpy as np
import torch

from . import _lib

GRID = 64


class ProcessedCorrespondences(dict):
    """The reference's dict of int64 index arrays, plus the device-side lists the kernels use."""
    device_lists = None


MAX_OBJECTS = 8           # ENERGY_MAX_OBJECTS of csrc/energy.hip


def object_label_image(fg_masks):
    """[H, W] uint8 label image of M pairwise disjoint masks: 0 outside all of them, m + 1 inside mask m."""
    if len(fg_masks) < 1 or len(fg_masks) > MAX_OBJECTS:
        raise ValueError(f"object labels: {len(fg_masks)} masks, 1 to {MAX_OBJECTS} are supported")
    m0 = torch.as_tensor(fg_masks[0])
    H, W = m0.shape[-2:]
    label = torch.zeros((H, W), dtype=torch.uint8, device=m0.device)
    for m, mask in enumerate(fg_masks):
        inside = torch.as_tensor(mask).reshape(H, W) != 0
        if bool((label[inside] != 0).any()):
            raise ValueError(f"object labels: mask {m} overlaps an earlier mask")
        label[inside] = m + 1
    return label


def check_object_weights(object_weights, n_objects):
    """None | "equal" | a sequence of n_objects finite weights >= 0, not all zero -> None | list of floats (host checks only)."""
    if object_weights is None:
        return None
    if isinstance(object_weights, str):
        if object_weights != "equal":
            raise ValueError(f"object_weights must be None, 'equal' or a sequence of floats, got {object_weights!r}")
        return [1.0] * int(n_objects)
    try:
        w = [float(v) for v in object_weights]
    except TypeError:
        raise ValueError(f"object_weights must be None, 'equal' or a sequence of floats, got {object_weights!r}") from None
    if len(w) != int(n_objects):
        raise ValueError(f"object_weights has {len(w)} entries for {n_objects} objects")
    if any(not np.isfinite(v) or v < 0.0 for v in w):
        raise ValueError(f"object_weights must be finite and >= 0, got {w}")
    if not any(v > 0.0 for v in w):
        raise ValueError("object_weights are all zero")
    return w


def object_omegas(objects, weights):
    """(N_m, omega_m) float64 of per-pair objects (0-based ints) and weights w_m: omega_m = w_m / sum of w_j over the objects
    that have pairs, 0 for an object without pairs.  ValueError when no object that has pairs has a positive weight."""
    w = np.asarray(weights, dtype=np.float64)
    counts = np.bincount(np.asarray(objects, dtype=np.int64), minlength=len(w))
    if len(counts) > len(w):
        raise ValueError(f"a pair belongs to object {len(counts) - 1}, there are {len(w)} weights")
    live = counts > 0
    total = float(w[live].sum())
    if live.any() and not total > 0.0:
        raise ValueError("object_weights: no positive weight among the objects that have correspondences")
    omega = np.where(live, w / total, 0.0) if live.any() else np.zeros_like(w)
    return counts, omega


def check_vacated(vacated, img_res, what="process_correspondences"):
    """The vacated image of an edit that deletes objects -> None or an [img_res, img_res] tensor (non-zero = vacated).
    ValueError naming `what` for another shape.  Host only: it reads the shape."""
    if vacated is None:
        return None
    v = torch.as_tensor(vacated)
    if v.numel() != int(img_res) * int(img_res) or v.shape[-1] != int(img_res):
        raise ValueError(f"{what}: vacated has shape {tuple(v.shape)}, expected one {img_res} x {img_res} image")
    return v.reshape(int(img_res), int(img_res))


def check_row_donor(row_donor, n_rows, what="process_correspondences"):
    """The donor flags of an edit's correspondence rows -> None or a flat uint8 tensor of n_rows entries (non-zero = the row's
    source pixel lies in the donor image).  ValueError naming `what` for another length.  Host only: it reads the shape."""
    if row_donor is None:
        return None
    r = torch.as_tensor(row_donor).reshape(-1)
    if r.numel() != int(n_rows):
        raise ValueError(f"{what}: row_donor has {r.numel()} entries for {n_rows} correspondences")
    return r


def check_row_kind(row_kind, n_rows, what="process_correspondences"):
    """The kinds of an edit's correspondence rows (camera moves, DESIGN.md "Camera moves") -> None or a flat uint8 tensor of
    n_rows entries: 0 = a host row, 1 = a donor row, 2 = a background row.  ValueError naming `what` for another length.
    Host only: it reads the shape."""
    if row_kind is None:
        return None
    r = torch.as_tensor(row_kind).reshape(-1)
    if r.numel() != int(n_rows):
        raise ValueError(f"{what}: row_kind has {r.numel()} entries for {n_rows} correspondences")
    return r


def process_correspondences(correspondences, img_res, bg_erosion=0, grid=GRID, device=None, row_donor=None, row_kind=None,
                            vacated=None, object_labels=None, pair_instances=None):
    """[N,4] int64 (ox,oy,tx,ty) -> dict with original_x/y, transformed_x/y, background_x/y[_orig|_trans].
    object_labels ([H, W] uint8, object_label_image): adds "object", the 0-based object of every kept pair (int64, host), and
    `pair_obj` (uint8, device) to device_lists.
    pair_instances ([N] uint8, the instance of every correspondence row -- edits with copies of an object, where a source pixel
    belongs to several instances and a label image cannot say which): filtered with the validity test of the rows, it fills the
    same "object" / `pair_obj`; an "object" of the energy is then an instance.  ValueError when both are given or when it does
    not have N entries, before any device work.
    vacated ([img_res, img_res], non-zero on the pixels of the objects the edit DELETES; DESIGN.md "Object removal"): a cell that
    holds a vacated pixel leaves the original-background list as if a kept correspondence started in it, before the erosion;
    the transformed-background list and the pairs do not see it.  None is the call without it (an all-zero image gives the
    same lists); the correspondences may then be empty (the pure removal).  The keys of the dict do not change.
    row_donor ([N] uint8, non-zero = the row's source pixel lies in a DONOR image; DESIGN.md "Object insertion"): such a row
    forms its pair and clears its target cell like any row, and leaves the original-background list alone -- nothing of the
    host started there.  None is the call without it, with the launches it had (all zeros give the same lists).
    row_kind ([N] uint8: 0 = a host row, 1 = a donor row, 2 = a BACKGROUND row of a camera move; DESIGN.md "Camera moves"): a
    background row forms its pair and clears neither background list -- the background stays background at both of its ends.
    row_donor remains as the 0 / 1 form; ValueError when both are given.  Kinds 0 and 1 give the lists of row_donor."""
    vacated = check_vacated(vacated, img_res)
    row_donor = check_row_donor(row_donor, int(torch.as_tensor(correspondences).reshape(-1, 4).shape[0]))
    row_kind = check_row_kind(row_kind, int(torch.as_tensor(correspondences).reshape(-1, 4).shape[0]))
    if row_donor is not None and row_kind is not None:
        raise ValueError("process_correspondences: row_donor and row_kind are mutually exclusive (row_kind 1 is a donor row)")
    if object_labels is not None and pair_instances is not None:
        raise ValueError("process_correspondences: object_labels and pair_instances are mutually exclusive")
    if pair_instances is not None:
        n_rows = int(torch.as_tensor(correspondences).reshape(-1, 4).shape[0])
        pair_instances = torch.as_tensor(pair_instances).reshape(-1)
        if pair_instances.numel() != n_rows:
            raise ValueError(f"process_correspondences: pair_instances has {pair_instances.numel()} entries for {n_rows} "
                             f"correspondences")
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    L = _lib.lib()
    corr = torch.as_tensor(correspondences).reshape(-1, 4).to(dev, torch.int64).contiguous()
    n = corr.shape[0]
    G2 = grid * grid
    pairs = torch.empty((max(n, 1), 2), dtype=torch.int32, device=dev)
    bg_lists = torch.empty((3, G2), dtype=torch.int32, device=dev)
    bg_masks = torch.empty((3, G2), dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    nbytes = ctypes.c_size_t()
    _lib.check(L.dh_cells_workspace_bytes(n, grid, ctypes.byref(nbytes)), "dh_cells_workspace_bytes")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    args = (_lib.ptr(corr) if n else _lib.c_p(0), n, int(img_res), grid, int(bg_erosion), _lib.ptr(pairs), _lib.ptr(bg_lists),
            _lib.ptr(bg_masks), _lib.ptr(counts), _lib.ptr(ws), nbytes.value, _lib.stream_ptr())
    if row_kind is not None:
        vac = None if vacated is None else (vacated.to(dev) != 0).to(torch.uint8).contiguous()
        kinds = row_kind.to(dev, torch.uint8).contiguous()
        _lib.check(L.dh_cells_from_correspondences_rows(*args, _lib.ptr(vac), _lib.ptr(kinds) if n else _lib.c_p(0)),
                   "dh_cells_from_correspondences_rows")
    elif row_donor is not None:
        vac = None if vacated is None else (vacated.to(dev) != 0).to(torch.uint8).contiguous()
        flags = (row_donor.to(dev) != 0).to(torch.uint8).contiguous()
        _lib.check(L.dh_cells_from_correspondences_donor(*args, _lib.ptr(vac), _lib.ptr(flags) if n else _lib.c_p(0)),
                   "dh_cells_from_correspondences_donor")
    elif vacated is None:
        _lib.check(L.dh_cells_from_correspondences(*args), "dh_cells_from_correspondences")
    else:
        vac = (vacated.to(dev) != 0).to(torch.uint8).contiguous()
        _lib.check(L.dh_cells_from_correspondences_vacated(*args, _lib.ptr(vac)), "dh_cells_from_correspondences_vacated")
    c = counts.cpu().tolist()
    pairs = pairs[:c[0]].contiguous()
    lists = [bg_lists[k, :c[1 + k]].contiguous() for k in range(3)]
    ph = pairs.cpu().numpy().astype(np.int64).reshape(-1, 2)
    lh = [l.cpu().numpy().astype(np.int64) for l in lists]
    out = ProcessedCorrespondences({
        "original_x": ph[:, 0] % grid, "original_y": ph[:, 0] // grid,
        "transformed_x": ph[:, 1] % grid, "transformed_y": ph[:, 1] // grid,
        "background_x": lh[0] % grid, "background_y": lh[0] // grid,
        "background_x_orig": lh[1] % grid, "background_y_orig": lh[1] // grid,
        "background_x_trans": lh[2] % grid, "background_y_trans": lh[2] // grid,
    })
    out.device_lists = dict(pairs=pairs, bg_both=lists[0], bg_orig=lists[1], bg_trans=lists[2],
                            bg_masks=bg_masks.view(3, grid, grid), grid=grid)
    if object_labels is not None:
        lab = torch.as_tensor(object_labels).to(dev)
        ok = (corr[:, 2] >= 0) & (corr[:, 2] < img_res) & (corr[:, 3] >= 0) & (corr[:, 3] < img_res)      # k_valid's test
        kept = corr[ok]
        obj = lab[kept[:, 1], kept[:, 0]].to(torch.int64) - 1
        oh = obj.cpu().numpy()
        if oh.shape[0] != ph.shape[0]:
            raise RuntimeError("object labels: the kept correspondences do not match the cell pairs")
        if oh.size and oh.min() < 0:
            raise ValueError("object labels: a correspondence starts outside every object mask")
        out["object"] = oh
        out.device_lists["pair_obj"] = obj.to(torch.uint8).contiguous()
    if pair_instances is not None:
        ok = (corr[:, 2] >= 0) & (corr[:, 2] < img_res) & (corr[:, 3] >= 0) & (corr[:, 3] < img_res)      # k_valid's test
        obj = pair_instances.to(dev)[ok].to(torch.uint8).contiguous()
        if obj.shape[0] != ph.shape[0]:
            raise RuntimeError("pair instances: the kept correspondences do not match the cell pairs")
        out["object"] = obj.cpu().numpy().astype(np.int64)
        out.device_lists["pair_obj"] = obj
    return out


def _device_lists(pc, dev, grid):
    dl = getattr(pc, "device_lists", None)
    if dl is not None and dl["pairs"].device == dev:
        return dl
    g = grid
    mk = lambda y, x: torch.as_tensor(np.asarray(pc[y]) * g + np.asarray(pc[x]), dtype=torch.int32, device=dev)
    pairs = torch.stack([mk("original_y", "original_x"), mk("transformed_y", "transformed_x")], dim=-1).contiguous()
    dl = dict(pairs=pairs, bg_both=mk("background_y", "background_x"),
              bg_orig=mk("background_y_orig", "background_x_orig"),
              bg_trans=mk("background_y_trans", "background_x_trans"), grid=g)
    if "object" in pc:
        dl["pair_obj"] = torch.as_tensor(np.asarray(pc["object"]), dtype=torch.uint8, device=dev)
    return dl


_WS = {}


class EnergyPlan:
    """Per-edit constants of the guidance energy on one cell grid: device index lists, the
    target-cell -> source-cells CSR and the transformed-background flags (dh_energy_plan_build).
    object_weights ("equal" or one weight per object; the correspondences must carry "object", process_correspondences with
    object_labels): the weighted plan of dh_energy_plan_build_objects -- `weighted` is then True, `omega` / `counts` hold
    omega_m and N_m, and the planned calls route to the _objects entries.  None, or a single object: the plan above --
    unless force_weighted (donor edits, whose kernels read the object of every entry: a weighted plan even for one object;
    object_weights None then means w_m = N_m, which gives every pair the unweighted coefficient fg_w / (C N) up to rounding).
    `n_objects` is the object count a weighted plan was built for."""

    weighted = False
    n_objects = 0

    def __init__(self, processed_correspondences, grid, device, object_weights=None, force_weighted=False):
        L = _lib.lib()
        self.grid = int(grid)
        self.dl = _device_lists(processed_correspondences, device, self.grid)
        self.n_pairs = int(self.dl["pairs"].shape[0])
        self._ws = {}
        if force_weighted and object_weights is None:
            if "object" not in processed_correspondences:
                raise ValueError("EnergyPlan: a forced weighted plan needs correspondences processed with pair_instances")
            objects = np.asarray(processed_correspondences["object"], dtype=np.int64)
            object_weights = [float(c) for c in np.bincount(objects, minlength=1)] if objects.size else [1.0]
        if object_weights is not None:
            if "object" not in processed_correspondences:
                raise ValueError("EnergyPlan: object_weights need correspondences processed with object_labels")
            objects = np.asarray(processed_correspondences["object"], dtype=np.int64)
            M = (int(objects.max()) + 1 if objects.size else 1) if isinstance(object_weights, str) else len(object_weights)
            w = check_object_weights(object_weights, M)
            if not 1 <= M <= MAX_OBJECTS:
                raise ValueError(f"EnergyPlan: {M} objects, 1 to {MAX_OBJECTS} are supported")
            counts, omega = object_omegas(objects, w)
            if M > 1 or force_weighted:
                self._build_weighted(L, w, counts, omega, device)
                return
        nb = ctypes.c_size_t()
        _lib.check(L.dh_energy_plan_bytes(self.grid, self.n_pairs, ctypes.byref(nb)), "dh_energy_plan_bytes")
        self.nbytes = nb.value
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        _lib.check(L.dh_energy_plan_build(_lib.ptr(self.dl["pairs"]), self.n_pairs, _lib.ptr(self.dl["bg_trans"]),
                                          self.dl["bg_trans"].numel(), self.grid, _lib.ptr(self.buf), self.nbytes,
                                          _lib.stream_ptr()), "dh_energy_plan_build")

    def _build_weighted(self, L, w, counts, omega, device):
        M = len(w)
        if self.dl.get("pair_obj") is None or self.dl["pair_obj"].numel() != self.n_pairs:
            raise ValueError("EnergyPlan: the device lists carry no object per pair")
        self.weighted, self.counts, self.omega, self.n_objects = True, counts, omega, M
        nb = ctypes.c_size_t()
        _lib.check(L.dh_energy_plan_objects_bytes(self.grid, self.n_pairs, ctypes.byref(nb)), "dh_energy_plan_objects_bytes")
        self.nbytes = nb.value
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        _lib.check(L.dh_energy_plan_build_objects(
            _lib.ptr(self.dl["pairs"]), _lib.ptr(self.dl["pair_obj"]), self.n_pairs, _lib.ptr(self.dl["bg_trans"]),
            self.dl["bg_trans"].numel(), self.grid, M, (ctypes.c_float * M)(*w), (ctypes.c_int32 * M)(*[int(c) for c in counts]),
            _lib.ptr(self.buf), self.nbytes, _lib.stream_ptr()), "dh_energy_plan_build_objects")

    def workspace(self, C):
        if C not in self._ws:
            nb = ctypes.c_size_t()
            _lib.check(_lib.lib().dh_energy_planned_workspace_bytes(C, self.grid, ctypes.byref(nb)))
            self._ws[C] = (torch.empty(nb.value, dtype=torch.uint8, device=self.buf.device), nb.value)
        return self._ws[C]


def energy_and_grad_planned(act, act_orig, plan, fg_weight, bg_weight, grad_scale=1.0, want_loss=False, out=None,
                            grad_dtype=None):
    """Default-configuration evaluation through a prebuilt EnergyPlan: act / act_orig [grid,grid,C] channels-last,
    16-bit, contiguous.  Returns (loss[3] or None, grad like act); `out`: where the gradient is written (e.g. the engine's
    own cotangent buffer of that activation); grad_dtype: the gradient's dtype (default: the activation's).  A weighted plan
    (EnergyPlan with object_weights) goes through dh_energy_fwd_bwd_planned_objects."""
    _lib.require_gpu(act)
    h, w, C = act.shape
    if h != plan.grid or w != plan.grid or act.dtype not in (torch.float16, torch.bfloat16) or act_orig.dtype != act.dtype:
        raise ValueError("planned energy: maps must be 16-bit [grid, grid, C] of one dtype")
    a = act.detach().contiguous()
    o = act_orig.detach().contiguous()
    gdt = a.dtype if grad_dtype is None else grad_dtype
    if out is not None and (out.shape != a.shape or out.dtype != gdt or not out.is_contiguous()):
        raise ValueError("planned energy: `out` must be a contiguous tensor like the activation")
    grad = torch.empty(a.shape, dtype=gdt, device=a.device) if out is None else out
    loss = torch.zeros(3, dtype=torch.float32, device=a.device) if want_loss else None
    ws, wsb = plan.workspace(C)
    dl = plan.dl
    L = _lib.lib()
    entry = L.dh_energy_fwd_bwd_planned_objects if plan.weighted else L.dh_energy_fwd_bwd_planned
    _lib.check(entry(
        _lib.ptr(a), _lib.ptr(o), _lib.DTYPE_CODE[a.dtype], C, plan.grid, _lib.ptr(plan.buf), plan.nbytes, plan.n_pairs,
        _lib.ptr(dl["bg_orig"]), dl["bg_orig"].numel(), _lib.ptr(dl["bg_trans"]), dl["bg_trans"].numel(),
        float(fg_weight), float(bg_weight), float(grad_scale), _lib.ptr(loss), _lib.ptr(grad),
        _lib.DTYPE_CODE[grad.dtype], _lib.ptr(ws), wsb, _lib.stream_ptr()),
        "dh_energy_fwd_bwd_planned_objects" if plan.weighted else "dh_energy_fwd_bwd_planned")
    return loss, grad


def check_donor_objects(donor_objects, plan, what):
    """The donor bits of one evaluation against its plan (host only): a weighted plan, no bit at or above its object count."""
    bits = int(donor_objects)
    if bits < 0 or bits >> 32:
        raise ValueError(f"{what}: donor_objects={donor_objects!r} is not a 32-bit mask")
    if not plan.weighted:
        raise ValueError(f"{what}: donor objects need a weighted plan (EnergyPlan with object_weights or force_weighted)")
    if bits >> plan.n_objects:
        raise ValueError(f"{what}: donor_objects={bits:#x} names an object at or above the plan's {plan.n_objects}")
    return bits


def energy_and_grad_planned_donor(act, act_orig, plan, fg_weight, bg_weight, act_donor, donor_objects, grad_scale=1.0,
                                  want_loss=False, out=None, grad_dtype=None):
    """energy_and_grad_planned for an edit with objects of another image (dh_energy_fwd_bwd_planned_donor; DESIGN.md "Object
    insertion"): the foreground term of a pair of object m reads act_donor where bit m of donor_objects is set, act_orig
    otherwise; act_donor is laid out like act_orig (None only with donor_objects = 0).  The plan is a weighted EnergyPlan;
    with object_weights None (force_weighted) w_m = N_m, the unweighted coefficient up to rounding.  donor_objects = 0 gives the
    bytes of energy_and_grad_planned.  ValueError before any launch for a bit at or above the plan's object count."""
    what = "energy_and_grad_planned_donor"
    _lib.require_gpu(act)
    bits = check_donor_objects(donor_objects, plan, what)
    h, w, C = act.shape
    if h != plan.grid or w != plan.grid or act.dtype not in (torch.float16, torch.bfloat16) or act_orig.dtype != act.dtype:
        raise ValueError("planned energy: maps must be 16-bit [grid, grid, C] of one dtype")
    if bits and (act_donor is None or act_donor.dtype != act.dtype or tuple(act_donor.shape) != tuple(act.shape)):
        raise ValueError(f"{what}: act_donor must be a map like act_orig")
    a = act.detach().contiguous()
    o = act_orig.detach().contiguous()
    dn = None if act_donor is None else act_donor.detach().contiguous()
    gdt = a.dtype if grad_dtype is None else grad_dtype
    if out is not None and (out.shape != a.shape or out.dtype != gdt or not out.is_contiguous()):
        raise ValueError("planned energy: `out` must be a contiguous tensor like the activation")
    grad = torch.empty(a.shape, dtype=gdt, device=a.device) if out is None else out
    loss = torch.zeros(3, dtype=torch.float32, device=a.device) if want_loss else None
    ws, wsb = plan.workspace(C)
    dl = plan.dl
    _lib.check(_lib.lib().dh_energy_fwd_bwd_planned_donor(
        _lib.ptr(a), _lib.ptr(o), _lib.DTYPE_CODE[a.dtype], C, plan.grid, _lib.ptr(plan.buf), plan.nbytes, plan.n_pairs,
        _lib.ptr(dl["bg_orig"]), dl["bg_orig"].numel(), _lib.ptr(dl["bg_trans"]), dl["bg_trans"].numel(),
        float(fg_weight), float(bg_weight), float(grad_scale), _lib.ptr(loss), _lib.ptr(grad),
        _lib.DTYPE_CODE[grad.dtype], _lib.ptr(ws), wsb, _lib.stream_ptr(), _lib.ptr(dn), bits), "dh_energy_fwd_bwd_planned_donor")
    return loss, grad


MAX_BATCH_ITEMS = 16      # ENERGY_MAX_ITEMS of csrc/energy.hip: the item table travels in the kernel arguments


def _batch_state(plans, C):
    """The item table of a batch of plans with its constant fields filled in, and the batch's workspace; kept on the first
    plan (a batch's plans live as long as its guidance states; lanes own their plans, so nothing is shared across streams)."""
    key = (C,) + tuple(id(p) for p in plans)
    cache = plans[0].__dict__.setdefault("_batch", {})
    hit = cache.get(key)
    if hit is None or any(r() is not p for r, p in zip(hit[3], plans)):      # (an id may be reused after a plan has died)
        cache.clear()
        K = len(plans)
        nb = ctypes.c_size_t()
        _lib.check(_lib.lib().dh_energy_planned_batch_workspace_bytes(C, plans[0].grid, K, ctypes.byref(nb)),
                   "dh_energy_planned_batch_workspace_bytes")
        items = (_lib.EnergyItem * K)()
        for it, p in zip(items, plans):
            it.plan, it.plan_bytes, it.n_pairs = p.buf.data_ptr(), p.nbytes, p.n_pairs
            it.bg_orig, it.n_bg_orig = p.dl["bg_orig"].data_ptr(), p.dl["bg_orig"].numel()
            it.bg_trans, it.n_bg_trans = p.dl["bg_trans"].data_ptr(), p.dl["bg_trans"].numel()
        cache[key] = (items, torch.empty(nb.value, dtype=torch.uint8, device=plans[0].buf.device), nb.value, [weakref.ref(p) for p in plans])
    return cache[key][:3]


def _planned_batch_call(entry_name, flags, acts, acts_orig, plans, fg_weights, bg_weights, grad_scales, want_loss, outs, grad_dtype,
                        call=None):
    """The argument checks and the item table of the batched planned entries, then the call: `entry_name` with the per-item
    flags of the mixed entry (flags = True) or without them."""
    K = len(acts)
    if K < 1 or not (len(acts_orig) == len(plans) == len(fg_weights) == len(bg_weights) == len(grad_scales) == K):
        raise ValueError("planned energy batch: the per-item lists must be non-empty and of one length")
    if K > MAX_BATCH_ITEMS:
        raise ValueError(f"planned energy batch: {K} items, at most {MAX_BATCH_ITEMS} go into one call")
    _lib.require_gpu(acts[0])
    h, w, C = acts[0].shape
    dt, grid = acts[0].dtype, plans[0].grid
    gdt = dt if grad_dtype is None else grad_dtype
    if dt not in (torch.float16, torch.bfloat16):
        raise ValueError("planned energy: maps must be 16-bit [grid, grid, C] of one dtype")
    if outs is None:
        outs = [torch.empty((h, w, C), dtype=gdt, device=acts[0].device) for _ in range(K)]
    for a, o, p, g in zip(acts, acts_orig, plans, outs):
        if (tuple(a.shape) != (grid, grid, C) or p.grid != grid or a.dtype != dt or o.dtype != dt or tuple(o.shape) != tuple(a.shape)
                or not a.is_contiguous() or not o.is_contiguous()):
            raise ValueError("planned energy batch: maps must be contiguous 16-bit [grid, grid, C] of one dtype and shape")
        if tuple(g.shape) != (h, w, C) or g.dtype != gdt or not g.is_contiguous():
            raise ValueError("planned energy batch: `outs` must be contiguous tensors like the activations")
    loss = torch.zeros((K, 3), dtype=torch.float32, device=acts[0].device) if want_loss else None
    items, ws, wsb = _batch_state(plans, C)
    for e, it in enumerate(items):
        it.cur, it.orig, it.grad = acts[e].data_ptr(), acts_orig[e].data_ptr(), outs[e].data_ptr()
        it.loss_out = loss[e].data_ptr() if want_loss else None
        it.fg_w, it.bg_w, it.grad_scale = float(fg_weights[e]), float(bg_weights[e]), float(grad_scales[e])
    # the flags are host bytes: the entry reads them while it fills the kernels' by-value tables, no kernel does
    head = (items, (ctypes.c_uint8 * K)(*[1 if p.weighted else 0 for p in plans])) if flags else (items,)
    _lib.check((call or getattr(_lib.lib(), entry_name))(*head, K, _lib.DTYPE_CODE[dt], C, grid, _lib.DTYPE_CODE[gdt], _lib.ptr(ws), wsb,
                                               _lib.stream_ptr()), entry_name)
    return loss, outs


def energy_and_grad_planned_donor_batch(acts, acts_orig, plans, fg_weights, bg_weights, grad_scales, acts_donor, donor_objects,
                                        want_loss=False, outs=None, grad_dtype=None):
    """energy_and_grad_planned_donor for K <= 16 items in one launch pair (dh_energy_fwd_bwd_planned_donor_batch): the arguments
    of energy_and_grad_planned_batch, then per item the donor map (None with no bit set) and the donor bits.  Weighted plans
    only.  Item e is bit-identical to the single call."""
    what = "energy_and_grad_planned_donor_batch"
    K = len(acts)
    if len(acts_donor) != K or len(donor_objects) != K:
        raise ValueError("planned energy batch: the per-item lists must be non-empty and of one length")
    bits = [check_donor_objects(b, p, f"{what}: item {e}") for e, (b, p) in enumerate(zip(donor_objects, plans))]
    for e, (dn, a) in enumerate(zip(acts_donor, acts)):
        if bits[e] and (dn is None or dn.dtype != a.dtype or tuple(dn.shape) != tuple(a.shape) or not dn.is_contiguous()):
            raise ValueError(f"{what}: item {e}: the donor map must be a contiguous map like the activation")

    def call(items, *tail):
        donor_items = (_lib.EnergyDonorItem * K)()
        for e in range(K):
            donor_items[e].item = items[e]
            donor_items[e].donor = acts_donor[e].data_ptr() if acts_donor[e] is not None else None
            donor_items[e].donor_objects = bits[e]
        return _lib.lib().dh_energy_fwd_bwd_planned_donor_batch(donor_items, *tail)

    return _planned_batch_call("dh_energy_fwd_bwd_planned_donor_batch", False, acts, acts_orig, plans, fg_weights, bg_weights,
                               grad_scales, want_loss, outs, grad_dtype, call=call)


def energy_and_grad_planned_batch(acts, acts_orig, plans, fg_weights, bg_weights, grad_scales, want_loss=False, outs=None,
                                  grad_dtype=None):
    """energy_and_grad_planned for K <= 16 items in one launch pair (dh_energy_fwd_bwd_planned_batch): item e is (acts[e],
    acts_orig[e], plans[e], fg_weights[e], bg_weights[e], grad_scales[e]); the items share the map shape and dtype and
    nothing else (edits of one image or of different images).  Returns (loss [K,3] or None, [K gradients]); outs: where the
    gradients are written.  Bit-identical per item to the single call.  More than 16 items raise (never split).  The plans are
    all weighted (EnergyPlan with object_weights: dh_energy_fwd_bwd_planned_objects_batch) or all unweighted; a mix goes to
    energy_and_grad_planned_mixed."""
    if any(p.weighted != plans[0].weighted for p in plans):
        raise ValueError("planned energy batch: weighted and unweighted plans do not go into one call")
    entry = "dh_energy_fwd_bwd_planned_objects_batch" if plans and plans[0].weighted else "dh_energy_fwd_bwd_planned_batch"
    return _planned_batch_call(entry, False, acts, acts_orig, plans, fg_weights, bg_weights, grad_scales, want_loss, outs, grad_dtype)


def energy_and_grad_planned_mixed(acts, acts_orig, plans, fg_weights, bg_weights, grad_scales, want_loss=False, outs=None,
                                  grad_dtype=None):
    """energy_and_grad_planned_batch for ANY mix of weighted and unweighted plans in one launch pair
    (dh_energy_fwd_bwd_planned_mixed_batch); same arguments and return value.  Item e is bit-identical to
    energy_and_grad_planned on it alone, whichever kind its plan is; all-weighted and all-unweighted batches are accepted too
    (and equal energy_and_grad_planned_batch)."""
    return _planned_batch_call("dh_energy_fwd_bwd_planned_mixed_batch", True, acts, acts_orig, plans, fg_weights, bg_weights,
                               grad_scales, want_loss, outs, grad_dtype)


def energy_and_grad(act, act_orig, processed_correspondences, fg_weight, bg_weight, fg_patch_size=1,
                    bg_patch_size=1, activations_size=(GRID, GRID), bg_loss_type="global_avg", grad_scale=1.0,
                    grad_dtype=None, channels_last=True, out=None):
    """One activation layer: returns (loss[3] = {total, fg, bg} f32 device tensor, grad like `act`).

    act / act_orig: [h,w,C] (channels_last) or [C,h,w] device tensors of the same dtype.
    """
    _lib.require_gpu(act)
    if bg_loss_type not in ("global_avg", "local_avg"):
        raise ValueError(f"Unknown background loss type: {bg_loss_type}")
    grid = int(activations_size[0])
    if not channels_last:
        act = act.permute(1, 2, 0)
        act_orig = act_orig.permute(1, 2, 0)
    a = act.detach().contiguous()
    o = act_orig.detach().to(a.dtype).contiguous()
    h, w, C = a.shape
    dev = a.device
    dl = _device_lists(processed_correspondences, dev, grid)
    gdt = a.dtype if grad_dtype is None else grad_dtype
    if out is not None and (tuple(out.shape) != (h, w, C) or out.dtype != gdt or not out.is_contiguous() or not channels_last):
        raise ValueError("energy: `out` must be a contiguous channels-last tensor like the activation")
    grad = torch.empty((h, w, C), dtype=gdt, device=dev) if out is None else out
    loss = torch.zeros(3, dtype=torch.float32, device=dev)
    L = _lib.lib()
    n_pairs = dl["pairs"].shape[0]
    nbytes = ctypes.c_size_t()
    _lib.check(L.dh_energy_workspace_bytes(C, grid, n_pairs, ctypes.byref(nbytes)), "dh_energy_workspace_bytes")
    key = (str(dev), nbytes.value)
    if key not in _WS:
        _WS.clear()
        _WS[key] = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    ws = _WS[key]
    _lib.check(L.dh_energy_fwd_bwd(
        _lib.ptr(a), _lib.ptr(o), _lib.DTYPE_CODE[a.dtype], C, h, w, grid,
        _lib.ptr(dl["pairs"]), n_pairs, _lib.ptr(dl["bg_both"]), dl["bg_both"].numel(),
        _lib.ptr(dl["bg_orig"]), dl["bg_orig"].numel(), _lib.ptr(dl["bg_trans"]), dl["bg_trans"].numel(),
        float(fg_weight), float(bg_weight), int(fg_patch_size), int(bg_patch_size),
        0 if bg_loss_type == "global_avg" else 1, float(grad_scale), _lib.ptr(loss), _lib.ptr(grad),
        _lib.DTYPE_CODE[gdt], _lib.ptr(ws), nbytes.value, _lib.stream_ptr()), "dh_energy_fwd_bwd")
    if not channels_last:
        grad = grad.permute(2, 0, 1)
    return loss, grad


def compute_foreground_loss(activations, activations_orig, processed_correspondences, patch_size, activations_size):
    """losses.py:4-17 -- [C,h,w] activations, returns the scalar foreground term."""
    loss, _ = energy_and_grad(activations, activations_orig, processed_correspondences, 1.0, 0.0, patch_size, 1,
                              activations_size, channels_last=False)
    return loss[1]


def compute_background_loss(activations, activations_orig, processed_correspondences, patch_size, activations_size,
                            loss_type="global_avg"):
    """losses.py:19-40 -- returns the scalar background term."""
    if loss_type not in ("global_avg", "local_avg"):
        raise ValueError(f"Unknown background loss type: {loss_type}")
    loss, _ = energy_and_grad(activations, activations_orig, processed_correspondences, 0.0, 1.0, 1, patch_size,
                              activations_size, bg_loss_type=loss_type, channels_last=False)
    return loss[2]
