#!/usr/bin/env python3
"""Same-box steps/s of the guided step with grad_scale 'static' and 'auto' (full SD-2-depth size, synthetic weights): one
process, the two modes alternating round by round, B = 1 (guided_step) and B = 8 (guided_step_batch).

  python tools/bench_guidance_scale.py [--steps 12] [--rounds 5] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from diffusionhandles_amd import conf as C
    from diffusionhandles_amd.depth_transform import reproject_edits, transform_depth
    from diffusionhandles_amd.guided_stable_diffuser import GuidedStableDiffuser
    from diffusionhandles_amd.synthetic import TRANSFORMS, make_scene
    from oracle import depth_ref as D
    dev = torch.device("cuda:0")
    conf = C.load_default().guided_diffuser
    K = args.batch
    gd = GuidedStableDiffuser(conf, max_batch=2 * K).to(dev)
    depth, bg, mask = make_scene(512)
    depth, bg, mask = depth.to(dev), bg.to(dev), mask.to(dev)
    disp = D.normalize_depth(1.0 / depth.cpu())[0].to(dev)
    prompt = "a sphere on a plane"
    unc = gd._encode([""])[None].expand(50, -1, -1, -1).contiguous()
    acts, _, _, noise = gd.initial_inference(None, disp, unc, prompt)
    Y = torch.tensor([0.0, 1.0, 0.0])
    ang, tr = TRANSFORMS[2]
    disp_e, corr = transform_depth(depth, bg, mask, gd.get_depth_intrinsics(), rot_angle=ang, rot_axis=Y, translation=torch.tensor(tr))
    tfs = [(TRANSFORMS[i % 8][0], Y, torch.tensor(TRANSFORMS[i % 8][1])) for i in range(K)]
    edits = reproject_edits(depth, bg, mask, gd.get_depth_intrinsics(), tfs, device_correspondences=True)
    gmax = conf.guidance_max_step
    x0 = noise.to(dev, torch.float32).permute(0, 2, 3, 1).contiguous()
    states = {}
    with torch.no_grad():
        for m in ("static", "auto"):
            gd.grad_scale_mode = m
            states[m] = (gd.prepare_guidance(disp_e, prompt, acts, corr), [gd.prepare_guidance(d, prompt, acts, c) for d, c in edits])
    gd.scheduler.set_timesteps(50)
    ts = gd.scheduler.timesteps

    def run(m, batched, n):
        st, sts = states[m]
        with torch.no_grad(), gd.on_stream():
            x = x0.expand(K, -1, -1, -1).contiguous() if batched else x0
            for i in range(n):
                t_idx = i % gmax
                x = gd.guided_step_batch(sts, x, t_idx, ts[t_idx], unc[t_idx]) if batched else \
                    gd.guided_step(st, x, t_idx, ts[t_idx], unc[t_idx])
        torch.cuda.synchronize()

    out = {}
    for batched in (False, True):
        B = K if batched else 1
        for m in ("static", "auto"):
            run(m, batched, 3)                       # warm: graphs captured, arenas touched
        times = {"static": [], "auto": []}
        for r in range(args.rounds):
            for m in (("static", "auto") if r % 2 == 0 else ("auto", "static")):
                t0 = time.perf_counter()
                run(m, batched, args.steps)
                times[m].append(args.steps / (time.perf_counter() - t0))
        med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
        out[f"B{B}"] = dict(steps_per_s=times, median=med, auto_over_static=med["auto"] / med["static"])
        print(f"B = {B}: steps/s median static {med['static']:.3f}  auto {med['auto']:.3f}  auto/static "
              f"{med['auto'] / med['static']:.4f}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
