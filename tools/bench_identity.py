#!/usr/bin/env python3
"""Per-image cost of the image identity (null-text inversion + initial inference) computed K images at a time.

  python tools/bench_identity.py [--ks 1,2,4,8] [--out FILE.json] [--no-warmup]

Full SD-2-depth configuration at 512x512 with seeded U-Net weights (the synthetic VAE / text stand-ins unless the
DIFFHANDLES_* environment names checkpoints), one diffuser built with max_batch = 2 max(K), every K in the same process.
Per K: StableNullInverter.invert_batch (5 inner steps, the facade's setting) and GuidedStableDiffuser.initial_inference_batch
on K images (seeds, depth mirror images and prompts differ per image), each phase timed separately with a device synchronise
after one untimed warm-up of the same K (the engine captures its hipGraphs per batch).  Prints one JSON line: seconds per
batch and per image, inner steps run, and the per-image speedup against K = 1.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

PROMPTS = ["a sphere on a plane", "a red ball in a bright room", "a wooden toy on a table", "a blue vase on a shelf",
           "a car in a street", "a chair in a garden", "a lamp on a desk", "a cup on a kitchen counter"]


def inputs(K, dev):
    from diffusionhandles_amd.depth_transform import normalize_depth
    from diffusionhandles_amd.synthetic import make_image, make_scene
    depth = make_scene(512)[0]
    mirrors = [depth, depth.flip(-1), depth.flip(-2), depth.flip(-1).flip(-2)]
    imgs = [make_image(512, seed=3 + 8 * b).to(dev) for b in range(K)]
    disps = [normalize_depth(1.0 / mirrors[b % 4]).to(dev) for b in range(K)]
    return imgs, disps, [PROMPTS[b % len(PROMPTS)] for b in range(K)]


def run(inv, gd, K, dev, inversion_only=False):
    imgs, disps, prompts = inputs(K, dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    res = inv.invert_batch(imgs, disps, prompts, num_inner_steps=5)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    if inversion_only:
        return t1 - t0, 0.0, [sum(tk) for tk in inv.inner_steps_taken]
    gd.initial_inference_batch([r[1] for r in res], disps, [r[2] for r in res], prompts)
    torch.cuda.synchronize(dev)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, [sum(tk) for tk in inv.inner_steps_taken]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--no-warmup", action="store_true", help="time the first run of every K (for a kernel trace of one run)")
    ap.add_argument("--inversion-only", action="store_true", help="skip the initial inference (kernel trace of the inversion)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_identity.py needs an MI355X (HIP device); there is no CPU fallback")
    from diffusionhandles_amd import conf as C
    from diffusionhandles_amd.guided_stable_diffuser import GuidedStableDiffuser
    from diffusionhandles_amd.stable_null_inverter import StableNullInverter
    ks = [int(k) for k in args.ks.split(",")]
    dev = torch.device("cuda:0")
    gd = GuidedStableDiffuser(C.load_default().guided_diffuser, max_batch=2 * max(ks)).to(dev)
    inv = StableNullInverter(gd)
    rows = []
    for K in ks:
        if not args.no_warmup:
            run(inv, gd, K, dev, args.inversion_only)
        inv_s, ii_s, steps = run(inv, gd, K, dev, args.inversion_only)
        rows.append(dict(K=K, inversion_s_per_batch=round(inv_s, 3), inversion_s_per_image=round(inv_s / K, 4),
                         initial_inference_s_per_batch=round(ii_s, 3), initial_inference_s_per_image=round(ii_s / K, 4) if ii_s else None,
                         identity_s_per_image=round((inv_s + ii_s) / K, 4), inner_steps_per_image=steps))
        sys.stderr.write(f"K = {K}: {json.dumps(rows[-1])}\n")
    base = next((r for r in rows if r["K"] == 1), None)
    if base is not None:
        for r in rows:
            r["speedup_per_image"] = dict(inversion=round(base["inversion_s_per_image"] / r["inversion_s_per_image"], 3),
                                          identity=round(base["identity_s_per_image"] / r["identity_s_per_image"], 3))
            if not args.inversion_only:
                r["speedup_per_image"]["initial_inference"] = round(base["initial_inference_s_per_image"]
                                                                    / r["initial_inference_s_per_image"], 3)
    line = json.dumps(dict(metric="identity_batch", resolution=512, unet="sd2-depth seeded", dtype="fp16", num_inner_steps=5,
                           warmup=not args.no_warmup, device=torch.cuda.get_device_name(dev), rows=rows))
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
