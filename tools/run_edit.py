#!/usr/bin/env python3
"""End-to-end edit harness: the build's counterpart of the reference's test/test_diffusion_handles.py
(invert -> reconstruct -> set_foreground -> transform_foreground per transform), on the synthetic scene or on a
scene directory, writing PNGs and the .npz identity cache with the reference's keys
(null_text_emb, init_noise, activations1..3, latent_image; test_diffusion_handles.py:106-113).

  python tools/run_edit.py --out /tmp/edit                       # synthetic sphere-on-plane scene
  python tools/run_edit.py --scene DIR --out /tmp/edit           # DIR laid out like the reference's test/data/<set>/<scene>:
                                                                 #   input.png, mask.png, depth.exr, bg_depth.exr (or .npy),
                                                                 #   prompt.txt, transforms.json {name: {translation,
                                                                 #   rotation_axis, rotation_angle}}; an entry may also have
                                                                 #   "scale" (a number or 3) and "pivot" (3 numbers): pc mode
                                                                 #   takes both, mesh mode a pivot only
                                                                 # several objects: mask_0.png .. mask_{M-1}.png and entries
                                                                 #   {name: {"objects": [M such entries], "object_weights":
                                                                 #   "equal" | [M floats]}} (scene_io.load_scene_geometry; pc mode)
  python tools/run_edit.py --scene tests/golden/scene_banana_fruits --out /tmp/edit   # a scene of the reference's test data
  python tools/run_edit.py --scene DIR --out /tmp/edit --background-lock [--lock-dilate D] [--lock-feather F]
                                                                 # hold the latents outside each edit's region to the
                                                                 #   reconstruction (conf key background_lock): an optional
                                                                 #   release.png in DIR sets extra area free, identity.npz
                                                                 #   also keeps the key `trajectory`, <edit>_keep.png is written
PNG / OpenEXR are read by diffusionhandles_amd.scene_io (no imaging library offline).
Real weights: DIFFHANDLES_UNET_SAFETENSORS / DIFFHANDLES_VAE_SAFETENSORS / DIFFHANDLES_TEXT_ENCODER_DIR /
DIFFHANDLES_TOKENIZER_DIR (otherwise seeded random U-Net weights and the synthetic side modules).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load_config(path):
    """--config PATH.yaml (test_diffusion_handles.py:47, --config_path): a configuration file of the reference's layout
    (test/config/*.yaml: the 13 guided_diffuser keys + depth_transform_mode).  Keys the file does not name keep the
    defaults of config/default.yaml; unknown keys are an error (a typo must not silently run the default edit)."""
    from diffusionhandles_amd import conf as C
    conf = C.load_default()
    if path is None:
        return conf
    over = C.load(path) or {}
    for k, v in over.items():
        if k == "guided_diffuser":
            for kk, vv in (v or {}).items():
                if kk not in conf.guided_diffuser and kk not in C.OPTIONAL_GUIDED_KEYS:
                    raise ValueError(f"{path}: unknown key guided_diffuser.{kk}")
                conf.guided_diffuser[kk] = vv
        elif k in conf or k in ("background_lock", "background_lock_dilate", "background_lock_feather",
                                "depth_transform_infill_border", "depth_transform_view_surfaces",
                                "depth_transform_view_surface_max_ratio"):
            conf[k] = v
        else:
            raise ValueError(f"{path}: unknown key {k}")
    return conf


def apply_footprint_args(args, conf):
    """--footprints / --footprint-max-ratio -> the optional conf keys depth_transform_footprints /
    depth_transform_footprint_max_ratio (DiffusionHandles reads them for --scene, --test-set and --edit-batch alike), checked
    as the library checks them (ValueError; NotImplementedError in mesh mode) before any engine is built.  Returns what the
    report carries: {footprints, footprint_max_ratio}."""
    from diffusionhandles_amd.depth_transform import check_footprints, mesh_has_no_footprints
    if args.footprints:
        conf["depth_transform_footprints"] = True
    if args.footprint_max_ratio is not None:
        conf["depth_transform_footprint_max_ratio"] = args.footprint_max_ratio
    fp, ratio = conf.get("depth_transform_footprints", False), conf.get("depth_transform_footprint_max_ratio")
    if conf.depth_transform_mode != "pc":
        mesh_has_no_footprints(fp, ratio, "--footprints")
    fp, ratio = check_footprints(fp, ratio, "--footprints")
    args.footprint_report = dict(footprints=fp, footprint_max_ratio=ratio)
    return args.footprint_report


def apply_border_args(args, conf):
    """--infill-border -> the optional conf key depth_transform_infill_border (DiffusionHandles reads it for --scene,
    --test-set and --edit-batch alike), checked as the library checks it (ValueError; NotImplementedError for reflect in mesh
    mode) before any engine is built and before any identity.  Returns what the report carries (nothing for the zero border:
    the reports of such runs stay what they were)."""
    from diffusionhandles_amd.depth_transform import INFILL_BORDERS, check_infill_border, mesh_has_no_infill_border
    if args.infill_border is not None:
        conf["depth_transform_infill_border"] = args.infill_border
    value = conf.get("depth_transform_infill_border")
    if conf.depth_transform_mode != "pc":
        mesh_has_no_infill_border(value, "--infill-border")
    border = check_infill_border(value, "--infill-border")
    args.border_report = dict(infill_border=INFILL_BORDERS[border]) if border else {}
    return args.border_report


def apply_view_surface_args(args, conf):
    """--view-surfaces / --view-surface-max-ratio -> the optional conf keys depth_transform_view_surfaces /
    depth_transform_view_surface_max_ratio (DiffusionHandles reads them wherever an edit carries a camera), checked as the
    library checks them (ValueError; NotImplementedError in mesh mode) before any engine is built and before any identity.
    Returns what the report carries (nothing with the setting off: the reports of such runs stay what they were)."""
    from diffusionhandles_amd.depth_transform import check_view_surfaces, mesh_has_no_view_surfaces
    if args.view_surfaces:
        conf["depth_transform_view_surfaces"] = True
    if args.view_surface_max_ratio is not None:
        conf["depth_transform_view_surface_max_ratio"] = args.view_surface_max_ratio
    vs, ratio = conf.get("depth_transform_view_surfaces", False), conf.get("depth_transform_view_surface_max_ratio")
    if conf.depth_transform_mode != "pc":
        mesh_has_no_view_surfaces(vs, ratio, "--view-surfaces")
    vs, ratio = check_view_surfaces(vs, ratio, "--view-surfaces")
    args.view_surface_report = dict(view_surfaces=True, view_surface_max_ratio=ratio) if vs else {}
    return args.view_surface_report


def apply_lock_args(args, conf):
    """--background-lock / --lock-dilate / --lock-feather -> the optional conf keys background_lock / background_lock_dilate /
    background_lock_feather (DiffusionHandles reads them for --scene, --test-set and --edit-batch alike), checked as the
    library checks them (ValueError) before any engine is built.  Sets args.background_lock (whether the lock is on, by the
    arguments or by the configuration file) and returns what the report carries."""
    from diffusionhandles_amd.background_lock import lock_conf
    if args.background_lock:
        conf["background_lock"] = True
    if args.lock_dilate is not None:
        conf["background_lock_dilate"] = args.lock_dilate
    if args.lock_feather is not None:
        conf["background_lock_feather"] = args.lock_feather
    reach = lock_conf(conf, "--background-lock")
    args.background_lock = reach is not None
    # (nothing with the lock off: the reports of unlocked runs stay what they were)
    args.lock_report = {} if reach is None else \
        dict(background_lock=True, background_lock_dilate=reach[0], background_lock_feather=reach[1])
    return args.lock_report


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=None)
    ap.add_argument("--out", default="edit_out")
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--mode", default=None, choices=["pc", "mesh"], help="depth_transform_mode (default: the configuration's)")
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--skip-inversion", action="store_true", help="generate the image from noise instead of inverting an input")
    ap.add_argument("--no-identity-cache", action="store_true",
                    help="neither read nor write the input-image identity cache (1 GB at 512x512)")
    ap.add_argument("--identity-cache", default=None,
                    help="path of the .npz identity cache (default <out>/identity.npz).  Like the reference's "
                         "--cache_input_image_identity (test_diffusion_handles.py:85-113): loaded when it exists, written otherwise")
    ap.add_argument("--skip-existing", action="store_true",
                    help="skip edits whose <name>.png exists, and the whole scene when all do (test_diffusion_handles.py:133-135, 216-225)")
    ap.add_argument("--max-edits", type=int, default=0, help="run only the first N transforms")
    # the reference harness's outer loop (test_diffusion_handles.py:302-323, 42-75)
    ap.add_argument("--test-set", default=None,
                    help="JSON {scene name: [transform names]} (the reference's data/photogen/photogen.json): every scene is read "
                         "from <input-dir>/<scene> and written to <out>/<scene>")
    ap.add_argument("--input-dir", default=None, help="directory of the scene directories of --test-set (default: the JSON's directory)")
    ap.add_argument("--config", default=None, help="configuration YAML (the reference's --config_path, test/config/*.yaml)")
    ap.add_argument("--max-scenes", type=int, default=0, help="--test-set: only the first N scenes")
    ap.add_argument("--identity-batch", type=int, default=1,
                    help="--scene with a donor/ directory: 2 takes the host's and the donor's identity in one pass.  "
                         "--test-set: the scenes that need an identity (not skipped, no cache file) are inverted and initially "
                         "inferred K at a time (DiffusionHandles.invert_input_images / generate_input_images; the engine is "
                         "built with max_batch >= 2K); 1 = one scene at a time")
    ap.add_argument("--edit-batch", type=int, default=1,
                    help="--test-set: the edits of ALL scenes are packed K at a time (parallel.pack_edit_batches) and every batch "
                         "runs as one DiffusionHandles.transform_foregrounds (the engine is built with max_batch >= 2K; 'pc' mode); "
                         "1 = one transform_foreground per edit")
    ap.add_argument("--edit-batch-images", type=int, default=0,
                    help="--edit-batch: at most N scenes in one batch (each keeps 0.53 GB of activations resident at 512x512); 0 = no bound")
    ap.add_argument("--footprints", action="store_true",
                    help="footprint splatting in 'pc' mode (conf key depth_transform_footprints): the triangles between "
                         "neighbouring points of an object are drawn too, so an enlarged or approaching object has no gaps")
    ap.add_argument("--footprint-max-ratio", type=float, default=None, metavar="R",
                    help="with --footprints: leave out triangles whose source depths differ by more than the factor R > 1 "
                         "(conf key depth_transform_footprint_max_ratio)")
    ap.add_argument("--infill-border", default=None, choices=["zero", "reflect"],
                    help="the image border of the depth in-fill in 'pc' mode (conf key depth_transform_infill_border): reflect = "
                         "zero normal derivative at the frame, so a region a camera move or a removal uncovers at the frame is "
                         "not pulled towards disparity 0 there; applies to the re-projection and to set_foreground")
    ap.add_argument("--view-surfaces", action="store_true",
                    help="--scene: under a camera move splat the whole scene as triangles in 'pc' mode (conf key "
                         "depth_transform_view_surfaces): the background and every object are surfaces, so a camera that moves "
                         "closer or orbits leaves unowned only what it uncovers and far surfaces do not show through near ones")
    ap.add_argument("--view-surface-max-ratio", type=float, default=None, metavar="R",
                    help="with --view-surfaces: leave out triangles whose source depths differ by more than the factor R > 1 "
                         "(conf key depth_transform_view_surface_max_ratio)")
    ap.add_argument("--background-lock", action="store_true",
                    help="hold every edit's latents to the reconstruction outside the region the edit touches (conf key "
                         "background_lock); the identity cache then also keeps the reconstruction trajectory, a release.png in "
                         "the scene directory sets extra area free, and every edit also writes <name>_keep.png")
    ap.add_argument("--lock-dilate", type=int, default=None, metavar="D",
                    help="with --background-lock: cells around the region that stay free (conf key background_lock_dilate, default 2)")
    ap.add_argument("--lock-feather", type=int, default=None, metavar="F",
                    help="with --background-lock: cells of the ramp from free to locked (conf key background_lock_feather, default 2)")
    args = ap.parse_args(argv)
    if args.edit_batch < 1 or (args.edit_batch > 1 and args.test_set is None):
        ap.error("--edit-batch K needs K >= 1, and K > 1 needs --test-set")
    if args.identity_batch < 1 or (args.identity_batch > 1 and args.test_set is None and args.scene is None):
        ap.error("--identity-batch K needs K >= 1, and K > 1 needs --test-set (or a --scene with a donor)")
    return args


def main():
    args = parse()
    conf = load_config(args.config)
    if args.mode is not None:
        conf.depth_transform_mode = args.mode
    args.mode = conf.depth_transform_mode
    apply_footprint_args(args, conf)
    apply_border_args(args, conf)
    apply_view_surface_args(args, conf)
    apply_lock_args(args, conf)
    state = {"dh": None}           # the engine is built on first use: a run that skips every scene never touches the GPU

    def handles(res):
        from diffusionhandles_amd import DiffusionHandles
        from diffusionhandles_amd.unet import SD2_DEPTH
        if state["dh"] is None:
            ucfg = dict(SD2_DEPTH, sample_size=res // 8)
            if not conf.guided_diffuser.use_depth:
                ucfg["in_channels"] = 4          # use_depth: false (test/config/no_depth.yaml): no depth channel beside the latent
            kmax = max(args.identity_batch, args.edit_batch)
            extra = {} if kmax == 1 else {"max_batch": 2 * kmax}
            state["dh"] = DiffusionHandles(conf, dtype=torch.float16 if args.dtype == "fp16" else torch.bfloat16,
                                           unet_config=ucfg, **extra).to(torch.device("cuda:0"))
        return state["dh"]

    if args.test_set is None:
        print(json.dumps(run_scene(args, conf, handles, args.scene, args.out, None)))
        return
    # ---- the test set: one output directory per scene, the configuration saved beside them, one summary page ----------------
    import yaml
    with open(args.test_set) as f:
        from collections import OrderedDict
        dataset = json.load(f, object_pairs_hook=OrderedDict)
    input_dir = args.input_dir or os.path.dirname(os.path.abspath(args.test_set))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "config.yaml"), "w") as f:            # (test_diffusion_handles.py:52-55)
        yaml.safe_dump(json.loads(json.dumps(conf)), f, sort_keys=False)
    names = list(dataset.items())
    if args.max_scenes > 0:
        names = names[:args.max_scenes]
    reports = []
    sub = argparse.Namespace(**vars(args))
    # the identity cache of a scene lives in its own output directory unless the caller disabled it
    sub.identity_cache = None
    identities = {}                 # --identity-batch > 1: the identities of the current chunk, by scene
    batch_seconds = None
    if args.edit_batch > 1:
        reports, batch_seconds = run_test_set_batched(sub, conf, handles, names, input_dir)
        names = []
    for idx, (scene, transform_names) in enumerate(names):
        sys.stderr.write(f"[{idx + 1}/{len(names)}] {scene}: {len(transform_names)} transforms\n")
        if args.identity_batch > 1 and scene not in identities:
            need = lambda i: needs_identity(sub, os.path.join(input_dir, names[i][0]), os.path.join(args.out, names[i][0]),
                                            list(names[i][1]))
            if need(idx):
                chunk = [idx]
                j = idx + 1
                while len(chunk) < args.identity_batch and j < len(names):
                    if need(j):
                        chunk.append(j)
                    j += 1
                identities = identity_chunk(sub, handles, [(os.path.join(input_dir, names[i][0]), names[i][0]) for i in chunk])
        rep = run_scene(sub, conf, handles, os.path.join(input_dir, scene), os.path.join(args.out, scene), list(transform_names),
                        identity=identities.pop(scene, None))
        rep["scene"] = scene
        reports.append(rep)
    set_name = os.path.splitext(os.path.basename(args.test_set))[0]
    rows = "".join(f'<tr><td><a href="{r["scene"]}/summary.html">{r["scene"]}</a></td><td>{len(r["edits"])}</td>'
                   f'<td>{"skipped" if r.get("skipped_scene") else r.get("identity_s", "")}</td></tr>' for r in reports)
    with open(os.path.join(args.out, f"{set_name}_summary.html"), "w") as f:
        f.write(f"<!doctype html><html><head><meta charset='utf-8'><title>{set_name}</title></head><body><h3>{set_name}: "
                f"{len(reports)} scenes</h3><table border='1' cellspacing='0' cellpadding='4'><tr><th>scene</th><th>edits</th>"
                f"<th>identity s</th></tr>{rows}</table></body></html>")
    total = dict(test_set=set_name, scenes=reports, config=args.config, depth_transform_mode=conf.depth_transform_mode,
                 **args.footprint_report, **args.border_report, **args.view_surface_report, **args.lock_report,
                 edits_run=sum(1 for r in reports for e in r["edits"] if not e.get("skipped")),
                 edits_skipped=sum(1 for r in reports for e in r["edits"] if e.get("skipped")))
    if batch_seconds is not None:
        total.update(edit_batch=args.edit_batch, batch_seconds=batch_seconds)
    json.dump(total, open(os.path.join(args.out, "report.json"), "w"), indent=1)
    print(json.dumps(total))


def needs_identity(args, scene, out, transform_names):
    """--identity-batch: whether run_scene would compute this scene's identity (not skipped, no cache file to load)."""
    p = prepare_scene(args, scene, out, transform_names, warn=False)
    if args.skip_existing and p["transforms"] and all(p["exists"].values()):
        return False
    return args.no_identity_cache or not cache_usable(args, os.path.join(out, "identity.npz"))


def cache_usable(args, cache):
    """Whether the identity cache file exists and serves this run: with --background-lock it must hold the reconstruction
    trajectory (a cache written without the lock is recomputed, never used unlocked)."""
    if not os.path.exists(cache):
        return False
    if not getattr(args, "background_lock", False):
        return True
    with np.load(cache) as z:
        return "trajectory" in z.files


def identity_chunk(args, handles, scenes):
    """The identities of K scenes of one resolution in batched passes: DiffusionHandles.invert_input_images (B = K) and
    generate_input_images (B = 2 K).  scenes: [(scene directory, name)].  Returns {name: (null_text, noise, acts, latent,
    seconds)}, seconds = the chunk's time divided by its number of scenes."""
    from diffusionhandles_amd.scene_io import load_scene
    dev = torch.device("cuda:0")
    scs = [load_scene(d, args.res) for d, _ in scenes]
    dh = handles(args.res)
    imgs = [sc["img"].to(dev) for sc in scs]
    depths = [sc["depth"].to(dev) for sc in scs]
    prompts = [sc["prompt"] for sc in scs]
    t0 = time.time()
    null_texts, noises = [None] * len(scs), [None] * len(scs)
    if not args.skip_inversion:
        null_texts, noises = map(list, zip(*dh.invert_input_images(imgs, depths, prompts)))
    res = dh.generate_input_images(depths, prompts, null_texts, noises)
    torch.cuda.synchronize()
    share = (time.time() - t0) / len(scs)
    return {name: r + (share,) for (_, name), r in zip(scenes, res)}


def prepare_scene(args, scene, out, transform_names, warn=True):
    """The inputs and the transform list of one scene, and which of its edits exist already."""
    from diffusionhandles_amd.scene_io import load_scene, object_transform_args, transform_args
    from diffusionhandles_amd.synthetic import TRANSFORMS, make_image, make_scene
    masks = None                    # a multi-object scene (mask_0.png ...): the list of its masks; `mask` is then their union
    release = None                  # --background-lock: the scene's optional release.png, [res,res] in {0,1}, read like a mask
    if scene and getattr(args, "background_lock", False) and os.path.exists(os.path.join(scene, "release.png")):
        from diffusionhandles_amd.scene_io import crop_and_resize, load_image
        release = load_image(os.path.join(scene, "release.png"))[None]
        release = (crop_and_resize(release.mean(dim=1, keepdim=True), args.res) > 0.5).to(torch.float32)[0, 0]
    if scene:
        sc = load_scene(scene, args.res)
        img, depth, bg_depth, mask, prompt, res = sc["img"], sc["depth"], sc["bg_depth"], sc["fg_mask"], sc["prompt"], args.res
        masks = sc.get("fg_masks")
        # object insertion: refused before any identity is computed where the re-projection has none
        for n, t in sc["transforms"].items():
            if isinstance(t, dict) and any(isinstance(o, dict) and "donor" in o for o in t.get("objects") or []):
                if args.mode != "pc":
                    raise NotImplementedError(f"{scene}: transform {n!r} inserts a donor object (\"donor\"); --mode {args.mode} has "
                                              "no object insertion, use --mode pc")
                if getattr(args, "footprint_report", {}).get("footprints"):
                    raise NotImplementedError(f"{scene}: transform {n!r} inserts a donor object (\"donor\"); --footprints "
                                              "(depth_transform_footprints) has no object insertion")
                if getattr(args, "view_surface_report", {}).get("view_surfaces"):
                    raise NotImplementedError(f"{scene}: transform {n!r} inserts a donor object (\"donor\"); --view-surfaces "
                                              "(depth_transform_view_surfaces) has no object insertion")
                if getattr(args, "edit_batch", 1) > 1:
                    raise NotImplementedError(f"{scene}: transform {n!r} inserts a donor object (\"donor\"); --edit-batch "
                                              "(mixed-image batches) has no object insertion")
        # camera moves: refused before any identity is computed where the re-projection or the loop has none
        for n, t in sc["transforms"].items():
            if isinstance(t, dict) and "camera" in t:
                if args.mode != "pc":
                    raise NotImplementedError(f"{scene}: transform {n!r} moves the camera (\"camera\"); --mode {args.mode} has no "
                                              "camera moves, use --mode pc")
                if getattr(args, "footprint_report", {}).get("footprints"):
                    raise NotImplementedError(f"{scene}: transform {n!r} moves the camera (\"camera\"); --footprints "
                                              "(depth_transform_footprints) has no camera moves")
                if getattr(args, "background_lock", False):
                    raise NotImplementedError(f"{scene}: transform {n!r} moves the camera (\"camera\"); --background-lock "
                                              "(background_lock) has no camera moves: the reconstruction's latents belong to "
                                              "another view")
                if any(isinstance(o, dict) and "donor" in o for o in t.get("objects") or []):
                    raise NotImplementedError(f"{scene}: transform {n!r} moves the camera (\"camera\") and inserts a donor object "
                                              "(\"donor\"): not supported together")
                if getattr(args, "edit_batch", 1) > 1:
                    raise NotImplementedError(f"{scene}: transform {n!r} moves the camera (\"camera\"); --edit-batch (mixed-image "
                                              "batches of scene directories) does not pass cameras, use --edit-batch 1")
        if args.mode != "pc":           # bend edits: before the identity is computed
            for n, t in sc["transforms"].items():
                objs = t.get("objects") if isinstance(t, dict) else None
                if (isinstance(t, dict) and "bend" in t) or any(isinstance(o, dict) and "bend" in o for o in objs or []):
                    raise NotImplementedError(f"{scene}: transform {n!r} bends an object (\"bend\"); --mode {args.mode} has no bend "
                                              "edits, use --mode pc")
        if args.mode != "pc":           # object removal: before the identity is computed
            for n, t in sc["transforms"].items():
                objs = t.get("objects") if isinstance(t, dict) else None
                if (isinstance(t, dict) and "remove" in t) or any(isinstance(o, dict) and "remove" in o for o in objs or []):
                    raise NotImplementedError(f"{scene}: transform {n!r} removes an object (\"remove\"); --mode {args.mode} has "
                                              "no object removal, use --mode pc")
        if masks is not None and args.mode != "pc":
            from diffusionhandles_amd.scene_io import entry_instances
            for n, t in sc["transforms"].items():          # (copies of an object: named for what they are)
                if entry_instances(t["objects"]) is not None:
                    raise NotImplementedError(f"{scene}: transform {n!r} places copies of an object (\"mask\" in its objects); "
                                              f"--mode {args.mode} has no copies, use --mode pc")
            raise NotImplementedError(f"{scene}: a multi-object scene ({len(masks)} masks) needs --mode pc; depth_transform_mode "
                                      f"{args.mode!r} has no multi-object re-projection")
        if masks is not None:       # entries {"objects": [...], "object_weights": ...}: transforms / object_weights per edit
            transforms = [dict(name=n, **object_transform_args(t)) for n, t in sc["transforms"].items()]
        else:
            transforms = [dict(name=n, **transform_args(t)) for n, t in sc["transforms"].items()]
    else:
        res = args.res
        depth, bg_depth, mask = make_scene(res)
        img = make_image(res)
        prompt = "a sphere on a plane"
        transforms = [dict(name=f"edit{i}", rot_angle=float(TRANSFORMS[i][0]), rot_axis=torch.tensor([0.0, 1.0, 0.0]),
                           translation=torch.tensor(TRANSFORMS[i][1], dtype=torch.float32)) for i in (2, 4)]
    if transform_names is not None:
        have = {tf["name"]: tf for tf in transforms}
        for n in transform_names:
            if warn and n not in have:
                sys.stderr.write(f"WARNING: transform {n} not found for scene {scene}; skipping\n")
        transforms = [have[n] for n in transform_names if n in have]
    if args.max_edits > 0:
        transforms = transforms[:args.max_edits]
    for i, tf in enumerate(transforms):
        tf.setdefault("name", f"edit{i}")
    if args.mode == "mesh":         # before the identity is computed: the mesh re-projection has no scale
        from diffusionhandles_amd.depth_transform import check_transform
        for tf in transforms:
            if check_transform((0.0, None, None, tf.get("scale"), None), f"{scene}: transform {tf['name']!r}")[3] != [1.0] * 3:
                raise NotImplementedError(f"{scene}: transform {tf['name']!r} has a scale ({tf['scale']!r}); --mode mesh has no "
                                          "scale, use --mode pc")
    exists = {tf["name"]: os.path.exists(os.path.join(out, tf["name"] + ".png")) for tf in transforms}
    donor = sc.get("donor") if scene and any(tf.get("donor") for tf in transforms) else None
    return dict(img=img, depth=depth, bg_depth=bg_depth, mask=mask, masks=masks, prompt=prompt, res=res, transforms=transforms,
                exists=exists, release=release, donor=donor)


def scene_identity(args, dh, p, out, identity=None):
    """The identity part of one scene: inversion + initial inference, the cache file, or `identity` from identity_chunk; then
    set_foreground and recon.png.  Returns the scene's device tensors and the head of its report."""
    from diffusionhandles_amd.scene_io import write_png
    dev = torch.device("cuda:0")
    img, depth, bg_depth, mask, prompt, res = p["img"], p["depth"], p["bg_depth"], p["mask"], p["prompt"], p["res"]
    depth, bg_depth, mask, img = depth.to(dev), bg_depth.to(dev), mask.to(dev), img.to(dev)
    t0 = time.time()
    cache = None if args.no_identity_cache else (args.identity_cache or os.path.join(out, "identity.npz"))
    lock = getattr(args, "background_lock", False)
    # (--background-lock: a cache without the reconstruction trajectory is recomputed and rewritten, never used unlocked)
    identity_from_cache = identity is None and cache is not None and cache_usable(args, cache)
    chunk_s = 0.0
    if identity is not None:
        null_text, noise, acts, latent, chunk_s = identity
    if identity_from_cache:
        # the input-image identity as the reference caches it (and as its web services pass it around,
        # webapp/webapps/diffhandles_webapp.py:82-94): float32 arrays under the reference's keys
        with np.load(cache) as z:
            null_text = torch.from_numpy(z["null_text_emb"]).to(dev)
            noise = torch.from_numpy(z["init_noise"]).to(dev)
            acts = [torch.from_numpy(z[f"activations{i + 1}"]).to(dev) for i in range(3)]
            latent = torch.from_numpy(z["latent_image"]).to(dev)
            if lock:
                from diffusionhandles_amd.background_lock import Activations
                acts = Activations(acts, trajectory=torch.from_numpy(z["trajectory"]).to(dev))
    else:
        if identity is None:
            null_text, noise = (None, None)
            if not args.skip_inversion:
                null_text, noise = dh.invert_input_image(img, depth, prompt)
            null_text, noise, acts, latent = dh.generate_input_image(depth, prompt, null_text, noise)
        if cache is not None:
            os.makedirs(os.path.dirname(os.path.abspath(cache)), exist_ok=True)
            # (the key `trajectory` only with the lock on: an unlocked run writes the reference's keys and nothing else)
            extra = dict(trajectory=acts.trajectory.float().cpu().numpy()) if lock else {}
            np.savez(cache, null_text_emb=null_text.float().cpu().numpy(),
                     init_noise=noise.float().cpu().numpy(), activations1=acts[0].float().cpu().numpy(),
                     activations2=acts[1].float().cpu().numpy(), activations3=acts[2].float().cpu().numpy(),
                     latent_image=latent.float().cpu().numpy(), **extra)
    if p.get("masks") is not None:          # several objects: the blend runs over the union of the list
        p["masks_dev"] = [m.to(dev) for m in p["masks"]]
        bg_depth = dh.set_foreground(depth, p["masks_dev"], bg_depth)
    else:
        bg_depth = dh.set_foreground(depth, mask, bg_depth)
    torch.cuda.synchronize()
    t_identity = time.time() - t0 + chunk_s
    recon = dh.diffuser.decode_latent_image(latent)
    write_png(os.path.join(out, "recon.png"), recon[0].permute(1, 2, 0).float().cpu().numpy())
    report = dict(resolution=res, mode=args.mode, identity_s=round(t_identity, 2), identity_from_cache=bool(identity_from_cache),
                  edits=[], **getattr(args, "footprint_report", {}), **getattr(args, "border_report", {}),
                  **getattr(args, "view_surface_report", {}),
                  **getattr(args, "lock_report", {}))
    if args.identity_batch > 1:
        report["identity_batch"] = args.identity_batch
    return depth, bg_depth, mask, img, null_text, noise, acts, report


def donor_identity(args, dh, p, out, host=None):
    """The identity of the scene's donor image (object insertion): its activations, from the cache donor_identity.npz beside the
    host's, or by inversion + initial inference -- with `host` = (img, depth, prompt) and --identity-batch >= 2 in ONE batched
    pass with the host's, whose identity tuple is then returned too.  Returns (donor dict for transform_foreground_objects,
    host identity or None)."""
    dev = torch.device("cuda:0")
    d = p["donor"]
    img, depth, prompt = d["img"].to(dev), d["depth"].to(dev), d["prompt"]
    host_cache = args.identity_cache or os.path.join(out, "identity.npz")
    cache = None if args.no_identity_cache else os.path.join(os.path.dirname(os.path.abspath(host_cache)), "donor_identity.npz")
    host_identity = None
    if cache is not None and os.path.exists(cache):
        with np.load(cache) as z:
            acts = [torch.from_numpy(z[f"activations{i + 1}"]).to(dev) for i in range(3)]
    else:
        t0 = time.time()
        if host is not None and args.identity_batch >= 2:
            imgs, depths, prompts = [host[0], img], [host[1], depth], [host[2], prompt]
            null_texts, noises = [None, None], [None, None]
            if not args.skip_inversion:
                null_texts, noises = map(list, zip(*dh.invert_input_images(imgs, depths, prompts)))
            both = dh.generate_input_images(depths, prompts, null_texts, noises)
            torch.cuda.synchronize()
            host_identity = both[0] + ((time.time() - t0) / 2,)
            acts = both[1][2]
        else:
            null_text, noise = (None, None)
            if not args.skip_inversion:
                null_text, noise = dh.invert_input_image(img, depth, prompt)
            acts = dh.generate_input_image(depth, prompt, null_text, noise)[2]
        if cache is not None:
            os.makedirs(os.path.dirname(cache), exist_ok=True)
            np.savez(cache, activations1=acts[0].float().cpu().numpy(), activations2=acts[1].float().cpu().numpy(),
                     activations3=acts[2].float().cpu().numpy())
    return dict(depth=depth, masks=[m.to(dev) for m in d["masks"]], activations=acts), host_identity


def write_scene_pages(args, out, img, mask, depth, bg_depth, prompt, res, report):
    """report.json, the input images and the results page of one scene."""
    from diffusionhandles_amd.scene_io import write_png
    json.dump(report, open(os.path.join(out, "report.json"), "w"), indent=1)
    # the results page of the reference's harness (test/generate_results_webpage.py: one row per edit with input, mask,
    # depth, background depth, reconstruction, edit, edited disparity), written without a template engine
    norm = lambda d: ((d - d.min()) / (d.max() - d.min() + 1e-12)).float().cpu().numpy()
    write_png(os.path.join(out, "input.png"), img[0].permute(1, 2, 0).float().cpu().numpy())
    write_png(os.path.join(out, "mask.png"), mask[0, 0].float().cpu().numpy())
    write_png(os.path.join(out, "depth.png"), norm(1.0 / depth[0, 0]))
    write_png(os.path.join(out, "bg_depth.png"), norm(1.0 / bg_depth[0, 0]))
    cols = ["input", "mask", "depth", "bg_depth", "recon"]
    rows = []
    for e in report["edits"]:
        e.setdefault("seconds", "skipped")
        cells = "".join(f'<td><img src="{c}.png" width="192"></td>' for c in cols)
        cells += f'<td><img src="{e["name"]}.png" width="192"></td><td><img src="{e["name"]}_disparity.png" width="192"></td>'
        rows.append(f'<tr><th>{e["name"]}<br>{e["seconds"]} s</th>{cells}</tr>')
    head = "".join(f"<th>{c}</th>" for c in ["edit"] + cols + ["edited image", "edited disparity"])
    with open(os.path.join(out, "summary.html"), "w") as f:
        f.write(f"<!doctype html><html><head><meta charset='utf-8'><title>{prompt}</title></head><body><h3>{prompt} "
                f"({res}x{res}, {args.mode})</h3><table border='1' cellspacing='0' cellpadding='4'><tr>{head}</tr>{''.join(rows)}</table></body></html>")


def resolve_camera(dh, depth, camera):
    """camera_args' dict -> the camera tuple of transform_foreground_objects (None -> None); "pivot_pixel" is resolved against
    the scene's depth with depth_transform.pivot_at_pixel."""
    if camera is None:
        return None
    pivot = camera.get("pivot")
    if "pivot_pixel" in camera:
        from diffusionhandles_amd.depth_transform import pivot_at_pixel
        x, y = camera["pivot_pixel"]
        pivot = tuple(float(v) for v in pivot_at_pixel(depth, dh.diffuser.get_depth_intrinsics(device=depth.device), x, y))
    return (camera["rot_angle"], camera["rot_axis"], camera["translation"], pivot)


def resolve_bends(dh, tf, depth, masks, donor=None):
    """The transforms of one entry with depth_transform.bend_chain in place of every member that carries "bend"
    (object_transform_args' `bends`; a single-mask scene's transform_args: `bend`).  masks: the masks the entry leaves, in
    order; donor: the scene's donor (depth, masks) when the entry has donor members.  A member's own angle, axis and
    translation are the chain's full motion; its "pivot", or the bend's "pivot_pixel" (resolved against the depth the member's
    mask belongs to), the chain's pivot."""
    from diffusionhandles_amd.depth_transform import bend_chain, pivot_at_pixel
    if "transforms" in tf:
        tfs, bends = list(tf["transforms"]), tf.get("bends")
    else:
        tfs, bends = [(tf["rot_angle"], tf["rot_axis"], tf["translation"], tf.get("scale"), tf.get("pivot"))], [tf.get("bend")]
    if not bends or all(b is None for b in bends):
        return tfs
    intr = dh.diffuser.get_depth_intrinsics(device=depth.device)
    every = [(depth, m) for m in masks]
    if donor is not None:
        every += [(donor["depth"].to(depth.device), m.to(depth.device)) for m in donor["masks"]]
    inst = tf.get("instances") or list(range(len(tfs)))
    for n, b in enumerate(bends):
        if b is None:
            continue
        d, m = every[inst[n]]
        t = tfs[n]
        pivot = t[4] if len(t) == 5 else None
        if "pivot_pixel" in b:
            pivot = pivot_at_pixel(d, intr, *b["pivot_pixel"])
        tfs[n] = bend_chain(d, intr, m, b["p0"], b["p1"], b["width"], t[0], t[1], t[2], pivot, b["bones"])
    return tfs


def split_removed(masks, remove):
    """The masks of a multi-object scene as the keywords of an edit call: fg_masks (what the entry leaves) and, for an entry
    with {"remove": true} members (object_transform_args' `remove`), removed_masks."""
    if not remove:
        return dict(fg_masks=masks)
    return dict(fg_masks=[m for i, m in enumerate(masks) if i not in remove], removed_masks=[masks[i] for i in remove])


def run_test_set_batched(args, conf, handles, names, input_dir):
    """--edit-batch K: the edits of every scene that are still to do (--skip-existing), packed K at a time over the scenes in
    test-set order; a batch's scenes keep their identities resident while it runs, a finished scene's identity is dropped.
    Writes the files run_scene writes.  Returns (scene reports, seconds per batch)."""
    from diffusionhandles_amd.parallel import pack_edit_batches
    from diffusionhandles_amd.scene_io import write_png
    if conf.depth_transform_mode != "pc":
        raise NotImplementedError("--edit-batch needs depth_transform_mode 'pc' (there is no batched mesh re-projection)")
    prep, reports, todo = {}, {}, []
    for scene, transform_names in names:
        out = os.path.join(args.out, scene)
        os.makedirs(out, exist_ok=True)
        p = prep[scene] = prepare_scene(args, os.path.join(input_dir, scene), out, list(transform_names))
        if args.skip_existing and p["transforms"] and all(p["exists"].values()):
            reports[scene] = dict(resolution=p["res"], mode=args.mode, skipped_scene=True, scene=scene,
                                  edits=[dict(name=n, skipped=True) for n in p["exists"]])
            continue
        todo.append((scene, [tf["name"] for tf in p["transforms"] if not (args.skip_existing and p["exists"][tf["name"]])]))
    batches = pack_edit_batches(todo, args.edit_batch, args.edit_batch_images or None)
    resident, seconds = {}, []
    for bi, batch in enumerate(batches):
        scenes = list(dict.fromkeys(s for s, _ in batch))
        sys.stderr.write(f"[batch {bi + 1}/{len(batches)}] {len(batch)} edits of {', '.join(scenes)}\n")
        for s in [s for s in resident if s not in scenes]:          # (a scene's edits are contiguous: it is finished)
            del resident[s]
        need = [s for s in scenes if s not in resident]
        ident = {}
        if args.identity_batch > 1:          # the batch's scenes without a cache file, --identity-batch at a time
            fresh = [s for s in need if needs_identity(args, os.path.join(input_dir, s), os.path.join(args.out, s),
                                                       [tf["name"] for tf in prep[s]["transforms"]])]
            for i in range(0, len(fresh), args.identity_batch):
                ident.update(identity_chunk(args, handles, [(os.path.join(input_dir, s), s)
                                                            for s in fresh[i:i + args.identity_batch]]))
        for s in need:
            p = prep[s]
            d, bg, m, img, null_text, noise, acts, rep = scene_identity(args, handles(p["res"]), p, os.path.join(args.out, s),
                                                                        ident.pop(s, None))
            resident[s] = dict(depth=d, bg_depth=bg, fg_mask=m, fg_masks=p.get("masks_dev"), img=img, null_text_emb=null_text,
                               init_noise=noise, activations=acts, prompt=p["prompt"])
            rep.update(scene=s, edit_batch=args.edit_batch,
                       edits=[dict(name=n, skipped=True) for n, ex in p["exists"].items() if args.skip_existing and ex])
            reports[s] = rep
        edits = []
        for s, name in batch:
            tf = next(t for t in prep[s]["transforms"] if t["name"] == name)
            r = resident[s]
            common = dict(depth=r["depth"], prompt=r["prompt"], bg_depth=r["bg_depth"], null_text_emb=r["null_text_emb"],
                          init_noise=r["init_noise"], activations=r["activations"])
            if prep[s].get("release") is not None:          # (--background-lock: the scene's release.png)
                common["release_mask"] = prep[s]["release"]
            if r["fg_masks"] is not None:
                sp = split_removed(r["fg_masks"], tf.get("remove"))
                edits.append(dict(common, **sp, transforms=resolve_bends(handles(prep[s]["res"]), tf, r["depth"], sp["fg_masks"]),
                                  object_weights=tf["object_weights"], instances=tf.get("instances")))
            elif tf.get("bend"):            # a single-mask scene's entry with "bend": the one-mask form of the multi-object edit
                edits.append(dict(common, fg_masks=[r["fg_mask"]],
                                  transforms=resolve_bends(handles(prep[s]["res"]), tf, r["depth"], [r["fg_mask"]])))
            elif tf.get("remove"):          # a single-mask scene's {"remove": true}: a pure removal
                edits.append(dict(common, fg_masks=[], transforms=[], removed_masks=[r["fg_mask"]]))
            else:
                edits.append(dict(common, fg_mask=r["fg_mask"], rot_angle=tf["rot_angle"], rot_axis=tf["rot_axis"],
                                  translation=tf["translation"], scale=tf.get("scale"), pivot=tf.get("pivot")))
        t0 = time.time()
        dh = handles(prep[scenes[0]]["res"])
        images, disparities = dh.transform_foregrounds(edits)
        torch.cuda.synchronize()
        dt = time.time() - t0
        seconds.append(round(dt, 3))
        for i, ((s, name), image, disparity) in enumerate(zip(batch, images, disparities)):
            out = os.path.join(args.out, s)
            if getattr(args, "background_lock", False):
                write_png(os.path.join(out, f"{name}_keep.png"), dh.last_keep_maps[i].float().cpu().numpy())
            write_png(os.path.join(out, f"{name}.png"), image.permute(1, 2, 0).float().cpu().numpy())
            write_png(os.path.join(out, f"{name}_disparity.png"), (disparity[0, 0] / disparity.max()).float().cpu().numpy())
            reports[s]["edits"].append(dict(name=name, seconds=round(dt / len(batch), 3), batch=bi))
        for s in scenes:             # a scene whose last edit ran in this batch is complete: its pages
            if not any(s == s2 for later in batches[bi + 1:] for s2, _ in later):
                r, p = resident[s], prep[s]
                order = {tf["name"]: i for i, tf in enumerate(p["transforms"])}
                reports[s]["edits"].sort(key=lambda e: order[e["name"]])
                write_scene_pages(args, os.path.join(args.out, s), r["img"], r["fg_mask"], r["depth"], r["bg_depth"], p["prompt"],
                                  p["res"], reports[s])
    return [reports[s] for s, _ in names if s in reports], seconds


def run_scene(args, conf, handles, scene, out, transform_names, identity=None):
    """One scene (the body of the reference's loop, test_diffusion_handles.py:66-175): identity (inversion + initial inference,
    or the cache), set_foreground, one transform_foreground per transform (a multi-object scene, mask_0.png ...:
    set_foreground on the list of masks and one transform_foreground_objects per entry).  transform_names: the subset / order the test set
    lists for this scene (names the scene's transforms.json does not have are skipped with a warning, :126-128).
    identity: (null_text, noise, acts, latent, seconds) computed by identity_chunk (--identity-batch), written to the cache."""
    from diffusionhandles_amd.scene_io import write_png
    os.makedirs(out, exist_ok=True)
    dev = torch.device("cuda:0")
    p = prepare_scene(args, scene, out, transform_names)
    img, depth, bg_depth, mask, prompt, res = p["img"], p["depth"], p["bg_depth"], p["mask"], p["prompt"], p["res"]
    transforms, exists = p["transforms"], p["exists"]
    if args.skip_existing and transforms and all(exists.values()):
        return dict(resolution=res, mode=args.mode, skipped_scene=True, edits=[dict(name=n, skipped=True) for n in exists])
    dh = handles(res)
    donor = None
    if p.get("donor") is not None:          # both identities; --identity-batch 2 takes them in one pass when neither is cached
        fresh = identity is None and (args.no_identity_cache or not cache_usable(args, args.identity_cache or os.path.join(out, "identity.npz")))
        donor, both = donor_identity(args, dh, p, out, (img.to(dev), depth.to(dev), prompt) if fresh else None)
        identity = both if both is not None else identity
    depth, bg_depth, mask, img, null_text, noise, acts, report = scene_identity(args, dh, p, out, identity)
    for tf in transforms:
        if args.skip_existing and exists[tf["name"]]:
            report["edits"].append(dict(name=tf["name"], skipped=True))
            continue
        t0 = time.time()
        cam = {} if tf.get("camera") is None else dict(camera=resolve_camera(dh, depth, tf["camera"]))
        if p.get("masks_dev") is not None:
            rel = {} if p.get("release") is None else dict(release_mask=p["release"])
            sp = split_removed(p["masks_dev"], tf.get("remove"))
            res_ = dh.transform_foreground_objects(depth, prompt, sp["fg_masks"], bg_depth, null_text, noise, acts,
                                                   transforms=resolve_bends(dh, tf, depth, sp["fg_masks"], p.get("donor")),
                                                   object_weights=tf["object_weights"],
                                                   removed_masks=sp.get("removed_masks"), instances=tf.get("instances"),
                                                   **(dict(donor=donor) if tf.get("donor") else {}), **rel, **cam)
        elif tf.get("bend"):            # a single-mask scene's entry with "bend": the one-mask form of transform_foreground_objects
            rel = {} if p.get("release") is None else dict(release_mask=p["release"])
            res_ = dh.transform_foreground_objects(depth, prompt, [mask], bg_depth, null_text, noise, acts,
                                                   transforms=resolve_bends(dh, tf, depth, [mask]), **rel, **cam)
        elif tf.get("camera_only"):     # a single-mask scene's entry with only "camera": the whole image from another viewpoint
            res_ = dh.transform_foreground_objects(depth, prompt, [], depth, null_text, noise, acts, transforms=[], **cam)
        elif cam:                       # the object moves and the camera moves: the one-mask form of transform_foreground_objects
            tf5 = (tf["rot_angle"], tf["rot_axis"], tf["translation"], tf.get("scale"), tf.get("pivot"))
            res_ = dh.transform_foreground_objects(depth, prompt, [mask], bg_depth, null_text, noise, acts, transforms=[tf5], **cam)
        elif tf.get("remove"):          # a single-mask scene's {"remove": true}: a pure removal
            rel = {} if p.get("release") is None else dict(release_mask=p["release"])
            res_ = dh.transform_foreground_objects(depth, prompt, [], bg_depth, null_text, noise, acts, transforms=[],
                                                   removed_masks=[mask], **rel)
        elif p.get("release") is not None:
            # (transform_foreground keeps the reference's parameter list: a release mask goes through the one-mask form of
            #  transform_foreground_objects, the same edit in 'pc' mode)
            if args.mode != "pc":
                raise NotImplementedError(f"{scene}: release.png needs --mode pc (the mesh mode's transform_foreground takes no "
                                          "release mask)")
            tf5 = (tf["rot_angle"], tf["rot_axis"], tf["translation"], tf.get("scale"), tf.get("pivot"))
            res_ = dh.transform_foreground_objects(depth, prompt, [mask], bg_depth, null_text, noise, acts, transforms=[tf5],
                                                   release_mask=p["release"])
        else:
            res_ = dh.transform_foreground(depth, prompt, mask, bg_depth, null_text, noise, acts, rot_angle=tf["rot_angle"],
                                          rot_axis=tf["rot_axis"], translation=tf["translation"], scale=tf.get("scale"),
                                          pivot=tf.get("pivot"))
        torch.cuda.synchronize()
        dt = time.time() - t0
        edited, disparity = res_[0], res_[1]
        name = tf["name"]
        write_png(os.path.join(out, f"{name}.png"), edited[0].permute(1, 2, 0).float().cpu().numpy())
        write_png(os.path.join(out, f"{name}_disparity.png"), (disparity[0, 0] / disparity.max()).float().cpu().numpy())
        if getattr(args, "background_lock", False):
            write_png(os.path.join(out, f"{name}_keep.png"), dh.last_keep_maps[0].float().cpu().numpy())
        report["edits"].append(dict(name=name, seconds=round(dt, 3)))
    write_scene_pages(args, out, img, mask, depth, bg_depth, prompt, res, report)
    return report


if __name__ == "__main__":
    main()
