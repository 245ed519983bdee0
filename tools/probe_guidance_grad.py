#!/usr/bin/env python3
"""Which amplitude should the guided edit's cotangent have?  (the target T of diffusionhandles_amd/guidance_scale.py)

One backward from the three guided activations to d(sample) at the full SD-2-depth size, fp16 and bf16 engines, against the
oracle's fp32 autograd (torch on the GPU), over log2(max |cotangent|) from -12 to +16.  The cotangent has the structure of
the L1 guidance energy's: a sign times an integer multiplicity (1..64) on a foreground block of cells, a sign on the
background cells, zero elsewhere, the same max-normalised pattern on all three maps.  The engine's backward is linear in its
cotangent, so the rows differ only by 16-bit range: subnormals at small amplitudes, overflow at large ones.

  python tools/probe_guidance_grad.py [--json OUT]        # one line per (dtype, log2 amplitude)
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-30)).item()


def cotangent(shape, g, dev):
    """[C, h, w] L1-like cotangent with max |.| = 1"""
    C, h, w = shape
    sign = torch.randint(0, 2, (C, h, w), generator=g, device=dev).float() * 2 - 1
    mult = torch.zeros(h, w, device=dev)
    y0, x0 = h // 4, w // 3
    mult[y0:y0 + h // 3, x0:x0 + w // 3] = torch.randint(1, 65, (h // 3, w // 3), generator=g, device=dev).float()
    bg = torch.ones(h, w, device=dev)
    bg[y0 - 2:y0 + h // 3 + 2, x0 - 2:x0 + w // 3 + 2] = 0.0
    d = sign * (mult + 0.5 * bg)[None]
    return d / d.abs().max()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from diffusionhandles_amd.unet import HipUNet
    from oracle import unet_torch as U
    dev = torch.device("cuda:0")
    ref = U.init_synthetic_(U.UNetTorch(U.SD2_DEPTH), seed=0).to(dev).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.half().float())
            p.requires_grad_(False)
    g = torch.Generator(device=dev).manual_seed(41)
    text = torch.randn(1, 77, 1024, generator=g, device=dev)
    x = torch.randn(1, 5, 64, 64, generator=g, device=dev)
    xq = x.clone().requires_grad_(True)
    out = ref(xq, torch.tensor(921, device=dev), encoder_hidden_states=text, return_dict=False)
    acts = [out[4 + k] for k in range(3)]
    d_acts = [cotangent(tuple(a.shape[1:]), g, dev)[None] for a in acts]
    (gx,) = torch.autograd.grad(acts, [xq], d_acts)
    gx = gx[:, :4]
    print(f"oracle: |d_sample| max {gx.abs().max().item():.3e} for max |cotangent| = 1", flush=True)
    rows = []
    sd = ref.state_dict()
    for dtype in (torch.float16, torch.bfloat16):
        hip = HipUNet(dict(U.SD2_DEPTH, text_len=77), dtype=dtype, max_batch=1)
        hip.load_state_dict(sd)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            xs = x.permute(0, 2, 3, 1).contiguous()
            for lg in range(-12, 17, 2):
                s = 2.0 ** lg
                hip.forward(xs, 921.0, text.contiguous(), save_for_backward=True, want_acts=[0, 1, 2], want_eps=False)
                d = [(a * s).permute(0, 2, 3, 1).to(dtype).contiguous() for a in d_acts]
                dx, _ = hip.backward(d, None, want_sample_grad=True, want_text_grad=False)
                torch.cuda.synchronize()
                dxs = dx.permute(0, 3, 1, 2)[:, :4].float()
                fin = bool(torch.isfinite(dxs).all())
                e = rel(dxs / s, gx) if fin else float("inf")
                rows.append(dict(dtype=str(dtype).split(".")[-1], log2_amplitude=lg, rel_err=e, finite=fin,
                                 max_d_sample=float(dxs.abs().max()) if fin else None))
                print(f"{str(dtype):16s} max|cotangent| = 2^{lg:+3d}: d_sample rel err {e:.3e}  finite {fin}", flush=True)
        hip.close()
        del hip
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(oracle_max_d_sample=float(gx.abs().max()), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
