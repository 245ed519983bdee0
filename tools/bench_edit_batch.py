#!/usr/bin/env python3
"""Guided edits of different images in one U-Net batch (DiffusionHandles.transform_foregrounds /
GuidedStableDiffuser.guided_inference_items) against the one-image batch and against single edits.

  python tools/bench_edit_batch.py steps  [--reps 2] [--energy batched,per-item] [--out FILE.json]
  python tools/bench_edit_batch.py corpus [--batch 8] [--max-images 0] [--out FILE.json]

Full SD-2-depth configuration at 512x512 with seeded U-Net weights and the synthetic VAE / text stand-ins, max_batch 16.

steps:  edit-steps/s (K x 50 timesteps / seconds of the whole guided_inference_* call: preparation, 50 steps, decode, one
        device synchronise) of K = 8 edits as  one-image: 8 transforms of one image (guided_inference_batch),  8x1: one
        transform of each of 8 images,  4x2: two transforms of each of 4 images (guided_inference_items).  The images are
        mirror images of the synthetic scene with different prompts and start noise, their identities come from
        generate_input_images (no inversion).  Every case runs once untimed, then --reps times, the cases alternating;
        with --energy batched,per-item every case is timed with the K-item energy launch pair and with K per-item
        launches (GuidedStableDiffuser._batch_energy).  A library without the batched entry (the parent's build through
        DIFFHANDLES_LIB, for a same-box A/B) runs with --energy per-item.
corpus: wall time of the 90 edits of tests/golden/photogen/photogen.json one at a time (transform_foreground) and packed
        --batch at a time over the scenes (parallel.pack_edit_batches -> transform_foregrounds).  The fixtures carry depth,
        background depth, mask and transforms but no image or prompt: the geometry is theirs, the identities come from
        generate_input_images with the scene name as prompt (no inversion) and are timed apart.
Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PROMPTS = ["a sphere on a plane", "a red ball in a bright room", "a wooden toy on a table", "a blue vase on a shelf",
           "a car in a street", "a chair in a garden", "a lamp on a desk", "a cup on a kitchen counter"]


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def steps(args, dh, dev):
    from diffusionhandles_amd.depth_transform import reproject_edits
    from diffusionhandles_amd.synthetic import TRANSFORMS, make_scene
    gd = dh.diffuser
    depth, bg, mask = (t.to(dev) for t in make_scene(512))
    flips = [(), (-1,), (-2,), (-1, -2)]
    geo = []
    for b in range(8):
        d, g, m = ((t.flip(*flips[b % 4]) if flips[b % 4] else t).contiguous() for t in (depth, bg, mask))
        geo.append((d * (1.0 + 0.05 * (b // 4)), dh.set_foreground(d, m, g) * (1.0 + 0.05 * (b // 4)), m))
    noises = [torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(100 + b)).to(dev) for b in range(8)]
    ids = []
    t_id = timed(lambda: ids.extend(dh.generate_input_images([d for d, _, _ in geo], PROMPTS, None, noises)), dev)
    Y = torch.tensor([0.0, 1.0, 0.0])
    tfs = [(TRANSFORMS[i][0], Y, torch.tensor(TRANSFORMS[i][1])) for i in range(8)]
    K_ = gd.get_depth_intrinsics()

    def items(n_img, per):
        out = []
        for b in range(n_img):
            d, g, m = geo[b]
            null_text, noise, acts, _ = ids[b]
            for dd, c in reproject_edits(d, g, m, K_, tfs[b * per:(b + 1) * per] if n_img > 1 else tfs, device_correspondences=True):
                out.append(dict(latents=noise, depth=dd, uncond_embeddings=null_text, prompt=PROMPTS[b], activations_orig=acts,
                                correspondences=c))
        return out
    one = items(1, 8)
    cases = OrderedDict([
        ("one_image_8", lambda: gd.guided_inference_batch(one[0]["latents"], [it["depth"] for it in one], one[0]["uncond_embeddings"],
                                                          PROMPTS[0], one[0]["activations_orig"], [it["correspondences"] for it in one])),
        ("items_8x1", (lambda its: lambda: gd.guided_inference_items(its))(items(8, 1))),
        ("items_4x2", (lambda its: lambda: gd.guided_inference_items(its))(items(4, 2))),
    ])
    T = int(gd.conf.num_timesteps)
    rows = {}
    energies = args.energy.split(",")
    for name, fn in cases.items():          # untimed: hipGraph capture per batch, allocator
        gd._batch_energy = energies[0] == "batched"
        fn()
    for rep in range(args.reps):
        for name, fn in cases.items():
            for en in energies:
                gd._batch_energy = en == "batched"
                s = timed(fn, dev)
                rows.setdefault(f"{name}/{en}", []).append(round(s, 4))
                sys.stderr.write(f"rep {rep} {name} energy {en}: {s:.4f} s, {8 * T / s:.2f} edit-steps/s\n")
    gd._batch_energy = True
    res = {k: dict(seconds=v, best_s=min(v), edit_steps_per_s=round(8 * T / min(v), 2), edits_per_s=round(8 / min(v), 3))
           for k, v in rows.items()}
    return dict(metric="edit_batch_steps", K=8, timesteps=T, identity_s_8_images=round(t_id, 3), cases=res)


def corpus(args, dh, dev):
    from diffusionhandles_amd.parallel import pack_edit_batches
    from diffusionhandles_amd.scene_io import load_scene_geometry, transform_args
    gold = os.path.join(ROOT, "tests", "golden", "photogen")
    with open(os.path.join(gold, "photogen.json")) as f:
        dataset = list(json.load(f, object_pairs_hook=OrderedDict).items())
    scenes, t_id = OrderedDict(), 0.0
    names = [s for s, _ in dataset]
    geos = {s: load_scene_geometry(os.path.join(gold, s), 512) for s in names}
    for i in range(0, len(names), 8):          # identities 8 scenes at a time
        chunk = names[i:i + 8]
        depths = [geos[s]["depth"].to(dev) for s in chunk]
        res = []
        t_id += timed(lambda: res.extend(dh.generate_input_images(depths, [s.replace("_", " ") for s in chunk])), dev)
        for s, d, (null_text, noise, acts, _) in zip(chunk, depths, res):
            m = geos[s]["fg_mask"].to(dev)
            scenes[s] = dict(depth=d, fg_mask=m, bg_depth=dh.set_foreground(d, m, geos[s]["bg_depth"].to(dev)), prompt=s.replace("_", " "),
                             null_text_emb=null_text, init_noise=noise, activations=acts)
    todo = [(s, [n for n in ns if n in geos[s]["transforms"]]) for s, ns in dataset]
    n_edits = sum(len(ns) for _, ns in todo)
    edit = lambda s, n: dict(scenes[s], **transform_args(geos[s]["transforms"][n]))

    def single():
        for s, ns in todo:
            for n in ns:
                e = edit(s, n)
                dh.transform_foreground(e["depth"], e["prompt"], e["fg_mask"], e["bg_depth"], e["null_text_emb"], e["init_noise"],
                                        e["activations"], rot_angle=e["rot_angle"], rot_axis=e["rot_axis"], translation=e["translation"])
    batches = pack_edit_batches(todo, args.batch, args.max_images or None)
    per_batch = []

    def packed():
        for b in batches:
            per_batch.append(round(timed(lambda: dh.transform_foregrounds([edit(s, n) for s, n in b]), dev), 3))
    # untimed: one single edit and one batch of every size that occurs (hipGraph capture per batch size)
    s0, n0 = todo[0][0], todo[0][1][0]
    e = edit(s0, n0)
    dh.transform_foreground(e["depth"], e["prompt"], e["fg_mask"], e["bg_depth"], e["null_text_emb"], e["init_noise"], e["activations"],
                            rot_angle=e["rot_angle"], rot_axis=e["rot_axis"], translation=e["translation"])
    for size in sorted({len(b) for b in batches}):
        dh.transform_foregrounds([edit(s, n) for s, n in next(b for b in batches if len(b) == size)])
    t1 = timed(single, dev)
    tk = timed(packed, dev)
    return dict(metric="edit_batch_corpus", edits=n_edits, scenes=len(todo), identity_s=round(t_id, 2), batch=args.batch,
                max_images=args.max_images, batches=[len(b) for b in batches], batch1_s=round(t1, 2), packed_s=round(tk, 2),
                speedup=round(t1 / tk, 3), batch1_s_per_edit=round(t1 / n_edits, 3), packed_s_per_edit=round(tk / n_edits, 3),
                batch_seconds=per_batch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["steps", "corpus"])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--energy", default="batched,per-item")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--max-images", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_edit_batch.py needs an MI355X (HIP device); there is no CPU fallback")
    from diffusionhandles_amd import DiffusionHandles, _lib
    dev = torch.device("cuda:0")
    if "batched" in args.energy.split(",") and "dh_energy_fwd_bwd_planned_batch" in _lib.lib().dh_missing_symbols:
        sys.exit("this library has no batched energy entry: run it with --energy per-item")
    dh = DiffusionHandles(max_batch=16).to(dev)
    if args.mode == "corpus":
        dh.diffuser._batch_energy = args.energy.split(",")[0] == "batched"
    out = (steps if args.mode == "steps" else corpus)(args, dh, dev)
    out.update(resolution=512, unet="sd2-depth seeded", dtype="fp16", device=torch.cuda.get_device_name(dev),
               library=os.path.basename(_lib.LIB_PATH))
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
