#!/usr/bin/env python3
"""GPU, tuning build: the GEMMPLAN lines of the VAE and text engines, pass by pass -- the source of the vae_* and text_* passes of
tests/test_gemm_plan.py (profiles/gemm_plan_aux/).

    tools/lab.sh build-tuning
    DIFFHANDLES_LIB=tools/bin/libdiffhandles_hip_tuning.so DH_GEMM_LOG=2 python3 tools/trace_aux_gemm_plans.py run 2> gemmplan_aux.txt
    python3 tools/trace_aux_gemm_plans.py rows gemmplan_aux.txt          (CPU: the log as PASSES[...] rows, distinct lines in order)

`run` launches the real engines once each with zero weights (the plan depends on shapes, flags, pitches, alignment and workspace
only): the VAE decoder and encoder at latent 64 and 96, one image, and the SD-2 text tower at batch 1 and 2.  A `PASS name` line on
stderr precedes each pass.  `rows` turns the log into table rows: lda / ldc equal to the default pitch become 0, the workspace of a
pass (the same on every line of an engine that passes one; 0 where a launch has none) goes to PASS_PART."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PINNED = ("pp", "bm", "bn", "splits", "stages", "kg", "mw", "buf", "epi", "gn_epi", "reduce")
FIELDS = ("pp", "bm", "bn", "stages", "wg", "kg", "mw", "gm", "buf", "lnf", "epi", "splits", "k_per_split", "grid_x", "grid_y",
          "grid_z", "a_bytes", "w_bytes", "gn_epi", "gn_cpg", "gn_S", "xa", "reduce")


def run():
    import torch

    from diffusionhandles_amd import _lib
    from diffusionhandles_amd.vae import HipTextEncoder, HipVAEDecoder, HipVAEEncoder
    dev = torch.device("cuda:0")
    L = _lib.lib()

    def mark(name):
        torch.cuda.synchronize()
        sys.stderr.write(f"PASS {name}\n")
        sys.stderr.flush()

    for lat in (64, 96):
        dec = HipVAEDecoder(latent_size=lat)
        z, img = torch.zeros(1, lat, lat, 4, device=dev), torch.zeros(1, 8 * lat, 8 * lat, 3, device=dev)
        mark(f"vae_dec_lat{lat}")
        _lib.check(L.dh_vae_decoder_decode(dec._h, _lib.ptr(z), 1, _lib.ptr(img), _lib.stream_ptr()), "decode")
        torch.cuda.synchronize()
        del dec
        enc = HipVAEEncoder(latent_size=lat)
        mom = torch.zeros(1, lat, lat, 8, device=dev)
        mark(f"vae_enc_lat{lat}")
        _lib.check(L.dh_vae_encoder_encode(enc._h, _lib.ptr(img), 1, _lib.ptr(mom), _lib.stream_ptr()), "encode")
        torch.cuda.synchronize()
        del enc
    text = HipTextEncoder(max_batch=2)
    for B in (1, 2):
        emb = torch.zeros(B, 77, 1024, device=dev)
        out = torch.empty_like(emb)
        mark(f"text_b{B}")
        _lib.check(L.dh_text_encoder_encode(text._h, _lib.ptr(emb), B, 77, _lib.ptr(out), _lib.stream_ptr()), "text")
        torch.cuda.synchronize()
    mark("end")


def parse(path):
    """{pass: [(query 17 values as the table writes them, pinned plan values)]}, distinct lines in their first order, and the
    workspace of each pass"""
    passes, parts, name = {}, {}, None
    for line in open(path):
        if line.startswith("PASS "):
            name = line.split()[1]
            passes.setdefault(name, [])
            continue
        if not line.startswith("GEMMPLAN q ") or name is None:
            continue
        q, p = line[len("GEMMPLAN q "):].split("|")
        q, p = [int(v) for v in q.split()], dict(zip(FIELDS, (int(v) for v in p.split())))
        M, N, K, conv, hw, stride, up, lda, ldc, part, flags = q[:11]
        lda = 0 if lda == (K // 9 if conv else K) else lda
        ldc = 0 if ldc == N else ldc
        row = ((M, N, K, conv, hw, stride, up, lda, ldc, flags) + tuple(q[11:]) + (part,), tuple(p[f] for f in PINNED))
        if row not in passes[name]:
            passes[name].append(row)
        if part:
            assert parts.setdefault(name, part) == part, (name, part)
    passes.pop("end", None)
    return passes, parts


def render(passes, parts):
    out = []
    for name, rows in passes.items():
        part = parts.get(name, 0)
        out.append(f'PASS_PART["{name}"] = {part}')
        out.append(f'PASSES["{name}"] = [')
        for q, want in rows:
            q = q[:16] if q[16] == part else q
            while len(q) > 10 and len(q) <= 16 and q[-1] == 0:
                q = q[:-1]
            out.append(f"    ({q}, {want}),")
        out.append("]")
    return "\n".join(out)


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run()
    else:
        print(render(*parse(sys.argv[2])))
