#!/usr/bin/env python3
"""Planned guidance-energy evaluation on the bench scene's real correspondences (run under rocprofv3 --kernel-trace).

Prints one JSON line with what each kernel of an evaluation touches (bytes), so that tools/hbm_report.py can turn the
kernel trace into achieved GB/s per kernel:  DH_RES=512|768, C = 320 and 640 (act2 and act1 of the SD-2-depth U-Net).

DH_OBJECT_WEIGHTS=equal: instead, the weighted evaluation (a weight per object, dh_energy_fwd_bwd_planned_objects) next to the
unweighted one on the same correspondences -- the OCCLUDING edit of the two-sphere scene of tests/multi_object_ref.py, C = 640 and
1280 -- timed with device events over DH_CALLS evaluations (default 200), alternating the two in blocks; one JSON line, also
written to profiles/object_weights/bench_energy_res<res>.json (DH_OUT: another directory).

DH_MIXED=1: instead, a batch of K = 8 items of which 4 carry a weighted plan and 4 a plain one (the OCCLUDING edit and a second
edit of the two-sphere scene, interleaved), C = 320, 640 and 1280, three ways: the one launch pair of
dh_energy_fwd_bwd_planned_mixed_batch, the item-by-item route (8 single calls) and the all-unweighted batch of 8
(dh_energy_fwd_bwd_planned_batch) -- same timing scheme; one JSON line, also written to
profiles/mixed_objects/bench_energy_res<res>.json (DH_OUT: another directory).

DH_DONOR=1: instead, the weighted evaluation of DH_OBJECT_WEIGHTS=equal (what the parent commit runs too) next to the donor
evaluation on the same plan with object 1 read from a second map (dh_energy_fwd_bwd_planned_donor: object insertion) -- same
scene, sizes and timing scheme; one JSON line, also written to profiles/object_insertion/bench_energy_res<res>.json (DH_OUT:
another directory)."""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from diffusionhandles_amd import losses as LS
from diffusionhandles_amd.depth_transform import transform_depth
from diffusionhandles_amd.guided_stable_diffuser import GuidedStableDiffuser
from diffusionhandles_amd.synthetic import TRANSFORMS, make_scene
dev = torch.device("cuda:0")
res = int(os.environ.get("DH_RES", "512"))
grid = res // 8


def object_weights_bench(ow):
    from diffusionhandles_amd.depth_transform import reproject_object_edits
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import multi_object_ref as R
    depth, bg_depth, masks = R.two_spheres(res)
    depth, bg_depth, masks = depth.to(dev), bg_depth.to(dev), [m.to(dev) for m in masks]
    tfs = [(tf[0], torch.tensor(tf[1]), torch.tensor(tf[2])) for tf in R.OCCLUDING]
    (_, corr), = reproject_object_edits(depth, bg_depth, masks, GuidedStableDiffuser.get_depth_intrinsics(dev), [tfs])
    pc = LS.process_correspondences(corr, res, 0, grid=grid, device=dev, object_labels=LS.object_label_image(masks))
    plain, weighted = LS.EnergyPlan(pc, grid, dev), LS.EnergyPlan(pc, grid, dev, object_weights=ow)
    assert weighted.weighted and not plain.weighted
    G2 = grid * grid
    tgt = torch.as_tensor(pc["transformed_y"]) * grid + torch.as_tensor(pc["transformed_x"])
    src = torch.as_tensor(pc["original_y"]) * grid + torch.as_tensor(pc["original_x"])
    obj = torch.as_tensor(pc["object"])
    per_obj = [sorted(set(tgt[obj == m].tolist())) for m in range(len(weighted.counts))]
    shared = set(per_obj[0]).intersection(*per_obj[1:])
    info = dict(res=res, grid=grid, object_weights=ow, correspondences=int(corr.shape[0]), pairs_per_object=[int(c) for c in weighted.counts],
                omega=[float(o) for o in weighted.omega], target_cells_per_object=[len(c) for c in per_obj], target_cells_shared=len(shared),
                entries_unweighted=int(torch.unique(torch.stack([src, tgt], 1), dim=0).shape[0]),
                entries_weighted=int(torch.unique(torch.stack([obj, src, tgt], 1), dim=0).shape[0]), layers=[])
    n = int(os.environ.get("DH_CALLS", "200"))
    gen = torch.Generator().manual_seed(1)
    for C in (640, 1280):
        cur = torch.randn(grid, grid, C, generator=gen).half().to(dev)
        org = torch.randn(grid, grid, C, generator=gen).half().to(dev)
        out = torch.empty_like(cur)
        run = lambda p: LS.energy_and_grad_planned(cur, org, p, 3.0, 2.0, grad_scale=256.0, out=out)
        for p in (plain, weighted):
            for _ in range(20):
                run(p)
        torch.cuda.synchronize()
        best = {"unweighted": [], "weighted": []}
        for _ in range(5):                                   # alternating blocks of n calls
            for name, p in (("unweighted", plain), ("weighted", weighted)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    run(p)
                e1.record()
                torch.cuda.synchronize()
                best[name].append(e0.elapsed_time(e1) * 1e3 / n)
        med = {k: sorted(v)[len(v) // 2] for k, v in best.items()}
        info["layers"].append(dict(C=C, us_per_evaluation_median=med, us_per_evaluation_blocks=best,
                                   weighted_over_unweighted=med["weighted"] / med["unweighted"]))
    line = json.dumps(info)
    out_dir = os.environ.get("DH_OUT") or os.path.join(ROOT, "profiles", "object_weights")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"bench_energy_res{res}.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def donor_bench():
    from diffusionhandles_amd.depth_transform import reproject_object_edits
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import multi_object_ref as R
    depth, bg_depth, masks = R.two_spheres(res)
    depth, bg_depth, masks = depth.to(dev), bg_depth.to(dev), [m.to(dev) for m in masks]
    tfs = [(tf[0], torch.tensor(tf[1]), torch.tensor(tf[2])) for tf in R.OCCLUDING]
    (_, corr), = reproject_object_edits(depth, bg_depth, masks, GuidedStableDiffuser.get_depth_intrinsics(dev), [tfs])
    pc = LS.process_correspondences(corr, res, 0, grid=grid, device=dev, object_labels=LS.object_label_image(masks))
    plan = LS.EnergyPlan(pc, grid, dev, object_weights="equal")
    assert plan.weighted
    info = dict(res=res, grid=grid, correspondences=int(corr.shape[0]), pairs_per_object=[int(c) for c in plan.counts],
                donor_objects=2, layers=[])
    n = int(os.environ.get("DH_CALLS", "200"))
    gen = torch.Generator().manual_seed(1)
    for C in (640, 1280):
        cur, org, dnr = (torch.randn(grid, grid, C, generator=gen).half().to(dev) for _ in range(3))
        out = torch.empty_like(cur)
        runs = {"weighted": lambda: LS.energy_and_grad_planned(cur, org, plan, 3.0, 2.0, grad_scale=256.0, out=out),
                "donor": lambda: LS.energy_and_grad_planned_donor(cur, org, plan, 3.0, 2.0, dnr, 2, grad_scale=256.0, out=out)}
        for run in runs.values():
            for _ in range(20):
                run()
        torch.cuda.synchronize()
        best = {k: [] for k in runs}
        for _ in range(5):                                   # alternating blocks of n calls
            for name, run in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    run()
                e1.record()
                torch.cuda.synchronize()
                best[name].append(e0.elapsed_time(e1) * 1e3 / n)
        med = {k: sorted(v)[len(v) // 2] for k, v in best.items()}
        info["layers"].append(dict(C=C, us_per_evaluation_median=med, us_per_evaluation_blocks=best,
                                   donor_over_weighted=med["donor"] / med["weighted"]))
    line = json.dumps(info)
    out_dir = os.environ.get("DH_OUT") or os.path.join(ROOT, "profiles", "object_insertion")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"bench_energy_res{res}.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def mixed_bench():
    from diffusionhandles_amd.depth_transform import reproject_object_edits
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import multi_object_ref as R
    K = 8
    depth, bg_depth, masks = R.two_spheres(res)
    depth, bg_depth, masks = depth.to(dev), bg_depth.to(dev), [m.to(dev) for m in masks]
    apart = [(10.0, R.Y, (-0.1, 0.0, 0.0)), (-30.0, R.Y, (0.15, 0.0, 0.0))]
    edits = [[(tf[0], torch.tensor(tf[1]), torch.tensor(tf[2])) for tf in e] for e in (R.OCCLUDING, apart)]
    rp = reproject_object_edits(depth, bg_depth, masks, GuidedStableDiffuser.get_depth_intrinsics(dev), edits)
    labels = LS.object_label_image(masks)
    pcs = [LS.process_correspondences(corr, res, 0, grid=grid, device=dev, object_labels=labels) for _, corr in rp]
    # item e: edit e % 2 (per pair of items), weighted where e is even -- weighted and unweighted interleaved
    mixed = [LS.EnergyPlan(pcs[(e // 2) % 2], grid, dev, object_weights="equal" if e % 2 == 0 else None) for e in range(K)]
    plain = [LS.EnergyPlan(pcs[(e // 2) % 2], grid, dev) for e in range(K)]
    assert [p.weighted for p in mixed] == [e % 2 == 0 for e in range(K)] and not any(p.weighted for p in plain)
    info = dict(res=res, grid=grid, items=K, weighted_items=4, pairs_per_item=[p.n_pairs for p in mixed], layers=[])
    n = int(os.environ.get("DH_CALLS", "200"))
    gen = torch.Generator().manual_seed(1)
    fw, bw, sc = [3.0] * K, [2.0] * K, [256.0] * K
    for C in (320, 640, 1280):
        cur = list(torch.randn(K, grid, grid, C, generator=gen).half().to(dev))
        org = list(torch.randn(K, grid, grid, C, generator=gen).half().to(dev))
        outs = list(torch.empty(K, grid, grid, C, dtype=torch.float16, device=dev))

        def one_launch():
            LS.energy_and_grad_planned_mixed(cur, org, mixed, fw, bw, sc, outs=outs)

        def item_by_item():
            for e in range(K):
                LS.energy_and_grad_planned(cur[e], org[e], mixed[e], fw[e], bw[e], grad_scale=sc[e], out=outs[e])

        def unweighted_batch():
            LS.energy_and_grad_planned_batch(cur, org, plain, fw, bw, sc, outs=outs)
        ways = (("mixed_one_launch", one_launch), ("mixed_item_by_item", item_by_item), ("unweighted_batch", unweighted_batch))
        for _, run in ways:
            for _ in range(20):
                run()
        torch.cuda.synchronize()
        best = {name: [] for name, _ in ways}
        for _ in range(5):                                   # alternating blocks of n calls
            for name, run in ways:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    run()
                e1.record()
                torch.cuda.synchronize()
                best[name].append(e0.elapsed_time(e1) * 1e3 / n)
        med = {k: sorted(v)[len(v) // 2] for k, v in best.items()}
        info["layers"].append(dict(C=C, us_per_batch_median=med, us_per_batch_blocks=best,
                                   item_by_item_over_one_launch=med["mixed_item_by_item"] / med["mixed_one_launch"],
                                   one_launch_over_unweighted_batch=med["mixed_one_launch"] / med["unweighted_batch"]))
    line = json.dumps(info)
    out_dir = os.environ.get("DH_OUT") or os.path.join(ROOT, "profiles", "mixed_objects")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"bench_energy_res{res}.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if os.environ.get("DH_DONOR"):
    donor_bench()
    sys.exit(0)
if os.environ.get("DH_MIXED"):
    mixed_bench()
    sys.exit(0)
if os.environ.get("DH_OBJECT_WEIGHTS"):
    v = os.environ["DH_OBJECT_WEIGHTS"]
    object_weights_bench(v if v == "equal" else [float(x) for x in v.split(",")])
    sys.exit(0)
depth, bg, mask = (t.to(dev) for t in make_scene(res))
ang, tr = TRANSFORMS[2]
_, corr = transform_depth(depth, bg, mask, GuidedStableDiffuser.get_depth_intrinsics(), rot_angle=ang,
                          rot_axis=torch.tensor([0.0, 1.0, 0.0]), translation=torch.tensor(tr))
pc = LS.process_correspondences(corr, res, 0, grid=grid, device=dev)
plan = LS.EnergyPlan(pc, grid, dev)
n1, n2 = int(plan.dl["bg_orig"].numel()), int(plan.dl["bg_trans"].numel())
cells = torch.stack([torch.as_tensor(pc["original_y"]) * grid + torch.as_tensor(pc["original_x"]),
                     torch.as_tensor(pc["transformed_y"]) * grid + torch.as_tensor(pc["transformed_x"])], dim=1)
uniq = int(torch.unique(cells, dim=0).shape[0])
gen = torch.Generator().manual_seed(1)
info = dict(res=res, grid=grid, pairs=int(corr.shape[0]), unique_cell_pairs=uniq, n_bg_orig=n1, n_bg_trans=n2, layers=[])
for C in (320, 640):
    cur = torch.randn(grid, grid, C, generator=gen).half().to(dev)
    org = torch.randn(grid, grid, C, generator=gen).half().to(dev)
    for _ in range(50):
        LS.energy_and_grad_planned(cur, org, plan, 3.0, 2.0, grad_scale=256.0)
    G2 = grid * grid
    info["layers"].append(dict(C=C, algorithmic_bytes=3 * G2 * C * 2, kernels=dict(
        k_colsum_q=(n1 + n2) * C * 2 + (n1 + n2) * 4 * (C // 64) + 8 * C * 4,
        k_energy_grad=2 * G2 * C * 2 + uniq * C * 2 + uniq * 8 + G2 * 9)))
torch.cuda.synchronize()
print(json.dumps(info))
