#!/usr/bin/env python3
"""Batched K=8 reprojection of the bench scene (run under rocprofv3 --stats for per-kernel times).
DH_OBJECTS=M (default 1): M = 1 is reproject_edits on the one-sphere scene; M = 2 is reproject_object_edits on the two-sphere
scene of tests/multi_object_ref.py (both objects move in every edit; edit 0 is the one where object 0 hides object 1).
DH_CALLS=n timed calls (default 5); the line reports their mean, median and minimum.
DH_SCALE=s (default unset): a second line times the same call with the uniform scale s on every object (5-tuples).
DH_FOOTPRINTS=1 (default unset; combinable with DH_SCALE / DH_OBJECTS): every timed call is followed by the same call with
footprint splatting on (profiles/footprints/).  DH_STEP=1: instead of the spheres, K copies of the step-scene edit of
tests/footprints_ref.py with footprints on, once per tier threshold of DH_TIERS (comma-separated; 0 = the default).
DH_COPIES=c (default unset; M * c <= 8): a further line times the call with c instances of every sphere (object copies: copy k
of an object takes another of the bench transforms and is lifted by 0.4 k, so the copies do not coincide).
DH_REMOVE=1 (default unset; the two-sphere scene whatever DH_OBJECTS says): two further lines time the K = 8 call with sphere 1
removed and sphere 0 moved (reproject_removal_edits), and the pure removal of both spheres (the background alone, computed
once for the K edits).
DH_DONOR=1 (default unset; the two-sphere scene whatever DH_OBJECTS says): two further lines time the K = 8 instance call on the
two spheres (reproject_instance_edits, instances [0, 1]: what the parent commit runs too) and the same call with one donor
sphere of tests/object_insertion_ref.py beside them (reproject_donor_edits: object insertion; profiles/object_insertion/).
DH_CAMERA=1 (default unset; the two-sphere scene whatever DH_OBJECTS says): two further lines time the K = 8 instance call on the
two spheres and the same call with eight orbit cameras about the centre pixel (depth_transform.orbit_cameras, -14 .. 14 degrees:
reproject_camera_edits, camera moves; profiles/camera_moves/); the second line also reports the background rows per edit.
DH_BORDER=reflect (default unset = zero): every call of the run in-fills with the reflecting image border (the named calls
timed here keep their parameter lists, so the setting is given to depth_transform.reproject, which they all are;
profiles/infill_border/); every line then says so.
DH_VIEW_SURFACES=1 [DH_VIEW_SURFACE_RATIO=R] (default unset), next to DH_CAMERA=1: the camera line runs with view surfaces
(reproject_surface_edits: the scene as triangles under the eight cameras; profiles/view_surfaces/) and says so.
DH_BEND=B (default unset; 2 .. 4; the two-sphere scene whatever DH_OBJECTS says): two further lines time the K = 8 call on the two
spheres unbent (reproject_object_edits) and the same call with sphere 0 a depth_transform.bend_chain of B bones across its
middle, the edit's own transform the full motion of its lower half (reproject_bend_edits; profiles/bend/).  The weights lie on
the device; the bent call's time includes the host's check of them and the gather at the objects' pixels.  With
DH_FOOTPRINTS=1 both lines are followed by their footprint runs."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from diffusionhandles_amd.guided_stable_diffuser import GuidedStableDiffuser
from diffusionhandles_amd.synthetic import TRANSFORMS, make_scene
dev = torch.device("cuda:0")
res = int(os.environ.get("DH_RES", "512"))
M = int(os.environ.get("DH_OBJECTS", "1"))
n = int(os.environ.get("DH_CALLS", "5"))
K = 8
Y = torch.tensor([0.0, 1.0, 0.0])
tfs = [(TRANSFORMS[i % 8][0], Y, torch.tensor(TRANSFORMS[i % 8][1])) for i in range(K)]
intr = GuidedStableDiffuser.get_depth_intrinsics(dev)
if M == 1:
    from diffusionhandles_amd.depth_transform import reproject_edits
    depth, bg_depth, mask = (t.to(dev) for t in make_scene(res))
    call = lambda **kw: reproject_edits(depth, bg_depth, mask, intr, tfs, **kw)
elif M == 2:
    from diffusionhandles_amd.depth_transform import reproject_object_edits
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import multi_object_ref as R
    depth, bg_depth, masks = R.two_spheres(res)
    depth, bg_depth, masks = depth.to(dev), bg_depth.to(dev), [m.to(dev) for m in masks]
    as_t = lambda tf: (tf[0], torch.tensor(tf[1]), torch.tensor(tf[2]))
    edits = [[as_t(tf) for tf in R.OCCLUDING]] + [[tfs[i], tfs[(i + 3) % 8]] for i in range(1, K)]
    call = lambda **kw: reproject_object_edits(depth, bg_depth, masks, intr, edits, **kw)
else:
    sys.exit("DH_OBJECTS: 1 or 2")
border = os.environ.get("DH_BORDER") or "zero"
if border != "zero":
    import diffusionhandles_amd.depth_transform as _DT
    _DT.check_infill_border(border, "DH_BORDER")
    _reproject = _DT.reproject
    _DT.reproject = lambda *a, **kw: _reproject(*a, **dict(kw, infill_border=border))
scale = float(os.environ["DH_SCALE"]) if os.environ.get("DH_SCALE") else None
footprints = os.environ.get("DH_FOOTPRINTS", "0") not in ("", "0")
CG_LDS, CG_MULTI = 8192, 65536          # dh_dbg_cg_limits: largest hole solved on chip / by the multi-workgroup CG


def solver(n):
    return "-" if n == 0 else "lds" if n <= CG_LDS else "multi" if n <= CG_MULTI else "single"


def report(call, label, **fp):
    if border != "zero":
        label += f" border={border}"
    if fp:
        label, inner = label + " footprints", call
        call = lambda **kw: inner(**kw, **fp)
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(n):
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    out, dbg = call(return_debug=True)
    cn = dbg["counts"]
    times.sort()
    print(f"K={K} M={M} res={res}{label}: {sum(times)/n:.2f} ms per call (median {times[n // 2]:.2f}, min {times[0]:.2f}, {n} calls); "
          f"foreground points {int(dbg['fg_pix'].numel())}; correspondences {[int(c.shape[0]) for _, c in out]}; "
          f"in-fill pixels {[int(v) for v in cn[:, 2]]}; CG iterations {[int(v) for v in cn[:, 3]]}; "
          f"solver {[solver(int(v)) for v in cn[:, 2]]}", flush=True)


if os.environ.get("DH_STEP", "0") not in ("", "0"):
    from diffusionhandles_amd import _lib
    from diffusionhandles_amd.depth_transform import reproject_object_edits
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import footprints_ref as F
    depth, bg_depth, masks = F.step_scene(res)
    depth, bg_depth, masks = depth.to(dev), bg_depth.to(dev), [m.to(dev) for m in masks]
    edits = [[(tf[0], torch.tensor(tf[1]), torch.tensor(tf[2])) for tf in F.STEP_TURN]] * K
    M = 1
    call = lambda **kw: reproject_object_edits(depth, bg_depth, masks, intr, edits, **kw)
    try:
        for tier in [int(t) for t in os.environ.get("DH_TIERS", "0").split(",")]:
            _lib.check(_lib.lib().dh_dbg_footprint_tier(tier), "dh_dbg_footprint_tier")
            report(call, f" step scene, tier {tier if tier else 'default'}", footprints=True)
    finally:
        _lib.lib().dh_dbg_footprint_tier(0)
    sys.exit(0)
report(call, "")
if footprints:
    report(call, "", footprints=True)
copies = int(os.environ.get("DH_COPIES", "0") or 0)
if copies:
    from diffusionhandles_amd.depth_transform import reproject_instance_edits
    if not 1 <= M * copies <= 8:
        sys.exit("DH_COPIES: objects * copies must be 1 to 8")
    inst = [m for m in range(M) for _ in range(copies)]
    lift = lambda tf, k: (tf[0], tf[1], tf[2] + torch.tensor([0.0, 0.4 * k, 0.0])) + tuple(tf[3:])
    inst_edits = [[lift(tfs[(i + 3 * m + 5 * k) % 8], k) for m in range(M) for k in range(copies)] for i in range(K)]
    inst_masks = [mask] if M == 1 else masks
    inst_call = lambda **kw: reproject_instance_edits(depth, bg_depth, inst_masks, intr, inst_edits, inst, **kw)
    report(inst_call, f" copies={copies} (instances {inst})")
    if footprints:
        report(inst_call, f" copies={copies} (instances {inst})", footprints=True)
if os.environ.get("DH_REMOVE", "0") not in ("", "0"):
    from diffusionhandles_amd.depth_transform import reproject_removal_edits
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import multi_object_ref as R
    r_depth, r_bg, r_masks = R.two_spheres(res)
    r_depth, r_bg, r_masks = r_depth.to(dev), r_bg.to(dev), [m.to(dev) for m in r_masks]
    M_shown, M = M, 1
    report(lambda **kw: reproject_removal_edits(r_depth, r_bg, r_masks[:1], intr, [[tf] for tf in tfs], removed_masks=r_masks[1:], **kw),
           " two spheres, sphere 1 removed")
    M = 0
    report(lambda **kw: reproject_removal_edits(r_depth, r_bg, [], intr, [[]] * K, removed_masks=r_masks, **kw),
           " two spheres, pure removal")
    M = M_shown
if os.environ.get("DH_DONOR", "0") not in ("", "0"):
    from diffusionhandles_amd.depth_transform import reproject_donor_edits, reproject_instance_edits
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import multi_object_ref as R
    import object_insertion_ref as I
    d_depth, d_bg, d_masks = R.two_spheres(res)
    d_depth, d_bg, d_masks = d_depth.to(dev), d_bg.to(dev), [m.to(dev) for m in d_masks]
    donor_depth, donor_masks = I.donor_scene(res, "disjoint")
    donor_depth, donor_masks = donor_depth.to(dev), [m.to(dev) for m in donor_masks]
    M_shown, M = M, 2
    two = [[tfs[i], tfs[(i + 3) % 8]] for i in range(K)]
    report(lambda **kw: reproject_instance_edits(d_depth, d_bg, d_masks, intr, two, [0, 1], **kw), " two spheres, instances [0, 1]")
    M = 3
    three = [e + [tfs[(i + 5) % 8] + (0.8, None)] for i, e in enumerate(two)]

    def donor_call(**kw):          # (a donor call returns the instance array beside every result: report() reads pairs)
        out = reproject_donor_edits(d_depth, d_bg, d_masks, intr, three, [0, 1, 2], donor_depth=donor_depth,
                                    donor_masks=donor_masks, **kw)
        return ([r[:2] for r in out[0]], out[1]) if kw.get("return_debug") else [r[:2] for r in out]
    report(donor_call, " two spheres and one donor sphere")
    M = M_shown
if os.environ.get("DH_CAMERA", "0") not in ("", "0"):
    from diffusionhandles_amd.depth_transform import orbit_cameras, reproject_camera_edits, reproject_instance_edits
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import multi_object_ref as R
    c_depth, c_bg, c_masks = R.two_spheres(res)
    c_depth, c_bg, c_masks = c_depth.to(dev), c_bg.to(dev), [m.to(dev) for m in c_masks]
    M_shown, M = M, 2
    two = [[tfs[i], tfs[(i + 3) % 8]] for i in range(K)]
    cams = orbit_cameras(c_depth, intr, res // 2, res // 2, [-14.0 + 4.0 * i for i in range(K)])
    report(lambda **kw: reproject_instance_edits(c_depth, c_bg, c_masks, intr, two, [0, 1], **kw), " two spheres, instances [0, 1]")
    n_bg = []
    surfaces = os.environ.get("DH_VIEW_SURFACES", "0") not in ("", "0")
    vs = {}
    if surfaces:
        from diffusionhandles_amd.depth_transform import reproject_surface_edits
        ratio = os.environ.get("DH_VIEW_SURFACE_RATIO")
        vs = dict(view_surfaces=True, view_surface_max_ratio=float(ratio) if ratio else None)

    def camera_call(**kw):          # (a camera call returns the instance array beside every result: report() reads pairs)
        if surfaces:
            out = reproject_surface_edits(c_depth, c_bg, c_masks, intr, two, [0, 1], cameras=cams, **vs, **kw)
        else:
            out = reproject_camera_edits(c_depth, c_bg, c_masks, intr, two, [0, 1], cameras=cams, **kw)
        if kw.get("return_debug"):
            n_bg[:] = out[1]["n_background"]
            return [r[:2] for r in out[0]], out[1]
        return [r[:2] for r in out]
    report(camera_call, " two spheres, eight orbit cameras" +
           (f" view surfaces (ratio {vs['view_surface_max_ratio']})" if surfaces else ""))
    print(f"  background rows per edit {n_bg}", flush=True)
    M = M_shown
bend = int(os.environ.get("DH_BEND", "0") or 0)
if bend:
    from diffusionhandles_amd.depth_transform import Bend, bend_chain, reproject_bend_edits, reproject_object_edits
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import multi_object_ref as R
    if not 2 <= bend <= 4:
        sys.exit("DH_BEND: 2 to 4 bones")
    b_depth, b_bg, b_masks = R.two_spheres(res)
    b_depth, b_bg, b_masks = b_depth.to(dev), b_bg.to(dev), [m.to(dev) for m in b_masks]
    M_shown, M = M, 2
    two = [[tfs[i], tfs[(i + 3) % 8]] for i in range(K)]
    cx, cy, rad, _ = R.SPHERES[0]
    k = res / 512.0
    p0, p1 = (int((cx - rad) * k), int(cy * k)), (int((cx + rad) * k), int(cy * k))

    def chain(tf):
        c = bend_chain(b_depth, intr, b_masks[0], p0, p1, res / 8.0, tf[0], tf[1], tf[2], bones=bend)
        return Bend(c.bones, c.weights.to(dev))
    bent = [[chain(e[0]), e[1]] for e in two]
    report(lambda **kw: reproject_object_edits(b_depth, b_bg, b_masks, intr, two, **kw), " two spheres, unbent")
    report(lambda **kw: reproject_bend_edits(b_depth, b_bg, b_masks, intr, bent, **kw), f" two spheres, sphere 0 a bend chain of {bend} bones")
    if footprints:
        report(lambda **kw: reproject_object_edits(b_depth, b_bg, b_masks, intr, two, **kw), " two spheres, unbent", footprints=True)
        report(lambda **kw: reproject_bend_edits(b_depth, b_bg, b_masks, intr, bent, **kw),
               f" two spheres, sphere 0 a bend chain of {bend} bones", footprints=True)
    M = M_shown
if scale is not None:
    if M == 1:
        tfs = [tf + (scale, None) for tf in tfs]
    else:
        edits = [[tf + (scale, None) for tf in e] for e in edits]
    report(call, f" scale={scale:g}")
    if footprints:
        report(call, f" scale={scale:g}", footprints=True)
