#!/usr/bin/env python3
"""Guided edits with and without the background lock (conf background_lock; DESIGN.md "Background lock").

  python tools/bench_background_lock.py steps [--reps 3] [--out FILE.json]
  python tools/bench_background_lock.py edit --lock {0,1}

Full SD-2-depth configuration at 512x512 with seeded U-Net weights and the synthetic VAE / text stand-ins, max_batch 16; the
synthetic scene, its identity from generate_input_image (no inversion), the first 8 TRANSFORMS.

steps: edit-steps/s (K x 50 timesteps / seconds of the whole guided_inference[_batch] call: preparation, 50 steps, decode,
       one device synchronise) at B = 1 and at batch 8, unlocked and locked, in ONE process; every case runs once untimed,
       then --reps times, the cases alternating.  The keep maps are built before the timed window (once per edit, as the
       facade builds them).
edit:  one B = 1 edit, unlocked or locked, keep map included -- the program for a kernel-trace run of its own
       (rocprofv3 --kernel-trace --stats -- python tools/bench_background_lock.py edit --lock 1): the launches per step must be
       equal with and without the lock.
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


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["steps", "edit"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lock", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_background_lock.py needs an MI355X (HIP device); there is no CPU fallback")
    from diffusionhandles_amd import DiffusionHandles, _lib
    from diffusionhandles_amd.background_lock import keep_map
    from diffusionhandles_amd.depth_transform import reproject_edits
    from diffusionhandles_amd.synthetic import TRANSFORMS, make_scene
    dev = torch.device("cuda:0")
    dh = DiffusionHandles(max_batch=16 if args.mode == "steps" else 2).to(dev)
    gd = dh.diffuser
    depth, bg, mask = (t.to(dev) for t in make_scene(512))
    bg = dh.set_foreground(depth, mask, bg)
    noise = torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(100)).to(dev)
    prompt = "a sphere on a plane"
    null_text, noise, acts, _ = dh.generate_input_image(depth, prompt, None, noise)
    Y = torch.tensor([0.0, 1.0, 0.0])
    tfs = [(TRANSFORMS[i][0], Y, torch.tensor(TRANSFORMS[i][1])) for i in range(8)]
    rp = reproject_edits(depth, bg, mask, gd.get_depth_intrinsics(), tfs, device_correspondences=True)
    s = gd.unet.sample_size
    T = int(gd.conf.num_timesteps)
    one = lambda lock: gd.guided_inference(noise, rp[0][0], null_text, prompt, acts, rp[0][1], lock=lock)
    if args.mode == "edit":
        lock = (keep_map(rp[0][1], mask, None, 512, s), acts.trajectory) if args.lock else None
        sec = timed(lambda: one(lock), dev)
        out = dict(metric="background_lock_edit", lock=bool(args.lock), seconds=round(sec, 3))
    else:
        keeps = [keep_map(c, mask, None, 512, s) for _, c in rp]
        locks = [(k, acts.trajectory) for k in keeps]
        eight = lambda lock: gd.guided_inference_batch(noise, [d for d, _ in rp], null_text, prompt, acts, [c for _, c in rp], lock=lock)
        cases = OrderedDict([("b1_unlocked", (1, lambda: one(None))), ("b1_locked", (1, lambda: one(locks[0]))),
                             ("b8_unlocked", (8, lambda: eight(None))), ("b8_locked", (8, lambda: eight(locks)))])
        for _, fn in cases.values():          # untimed: hipGraph capture per batch, allocator
            fn()
        rows = {}
        for rep in range(args.reps):
            for name, (K, fn) in cases.items():
                sec = timed(fn, dev)
                rows.setdefault(name, []).append(round(sec, 4))
                sys.stderr.write(f"rep {rep} {name}: {sec:.4f} s, {K * T / sec:.2f} edit-steps/s\n")
        res = {k: dict(seconds=v, edit_steps_per_s=[round(cases[k][0] * T / x, 2) for x in v],
                       best_edit_steps_per_s=round(cases[k][0] * T / min(v), 2)) for k, v in rows.items()}
        out = dict(metric="background_lock_steps", timesteps=T, locked_fraction=[round(float((k == 1).float().mean()), 3) for k in keeps],
                   cases=res)
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
