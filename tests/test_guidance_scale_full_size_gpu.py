"""'static' and 'auto' guidance scale side by side at the full SD-2-depth size (fp16, seeded weights): the teacher-forced
first-iteration and three-iteration latent updates of GuidedStableDiffuser.guided_step against the fp32 oracle loop at t_idx 0,
12, 24 and 37 (all three layer phases of the weight schedule, early and late timesteps).  Every step starts from the ORACLE's
latent after the previous step."""
from types import SimpleNamespace

import pytest
import torch

from diffusionhandles_amd.synthetic import TRANSFORMS, make_scene

pytestmark = pytest.mark.gpu

CHECKED = (0, 12, 24, 37)
# 2x the worst 'auto' errors measured over CHECKED (first 1.145e-2, three 8.69e-3; 'static' 1.145e-2, 8.64e-3)
GATE_FIRST, GATE_THREE = 2.29e-2, 1.74e-2


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@pytest.fixture(scope="module")
def full():
    from diffusionhandles_amd import conf as C
    from diffusionhandles_amd.depth_transform import transform_depth
    from diffusionhandles_amd.guided_stable_diffuser import GuidedStableDiffuser
    from diffusionhandles_amd.unet import HipUNet
    from oracle import depth_ref as D
    from oracle import loop_ref as L
    from oracle import unet_torch as U
    ref = U.init_synthetic_(U.UNetTorch(U.SD2_DEPTH), seed=0).to(dev()).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.half().float())
            p.requires_grad_(False)
    hip = HipUNet(dict(U.SD2_DEPTH, text_len=77), dtype=torch.float16, max_batch=2)
    hip.load_state_dict(ref.state_dict())
    conf = C.load_default().guided_diffuser
    gd = GuidedStableDiffuser(conf, unet=hip, unet_config=dict(U.SD2_DEPTH, text_len=77)).to(dev())
    depth, bg, mask = make_scene(512)
    disp = D.normalize_depth(1.0 / depth)[0].to(dev())
    prompt = "a sphere on a plane"
    cond = gd._encode([prompt])
    unc = gd._encode([""])[None].expand(50, -1, -1, -1).contiguous()
    noise = torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(2773)).to(dev())
    n = max(CHECKED) + 1

    class First(L.DDIM):
        def set_timesteps(self, m):
            super().set_timesteps(m)
            self.timesteps = self.timesteps[:n]
    acts_o, _, _, _ = L.initial_inference(ref, First(), noise, disp, unc, cond)
    acts = []
    for a in acts_o:
        buf = torch.zeros((50,) + tuple(a.shape[1:]), dtype=torch.float32, device=dev())
        buf[:n] = a
        acts.append(buf)
    ang, tr = TRANSFORMS[2]
    disp_e, corr = transform_depth(depth.to(dev()), bg.to(dev()), mask.to(dev()), gd.get_depth_intrinsics(), rot_angle=ang,
                                   rot_axis=torch.tensor([0.0, 1.0, 0.0]), translation=torch.tensor(tr))
    return SimpleNamespace(ref=ref, gd=gd, conf=conf, prompt=prompt, cond=cond, unc=unc, noise=noise, acts=acts, disp_e=disp_e,
                           corr=corr)


def test_static_and_auto_updates_full_size_teacher_forced(full):
    from oracle import loop_ref as L
    r = full
    gd = r.gd
    states = {}
    with torch.no_grad(), gd.on_stream():
        for m in ("static", "auto"):
            gd.grad_scale_mode = m
            states[m] = gd.prepare_guidance(r.disp_e, r.prompt, r.acts, r.corr)
        gd.grad_scale_mode = "static"
    assert states["auto"].auto and not states["static"].auto
    worst = {m: [0.0, 0.0] for m in states}
    x_in = r.noise
    gd.scheduler.set_timesteps(50)
    ts = gd.scheduler.timesteps
    for i in range(max(CHECKED) + 1):
        rec_o = {}
        L.guided_inference(r.ref, L.DDIM(), x_in, r.disp_e, r.unc, r.cond, r.acts, r.corr.numpy(), r.conf, record=rec_o, steps=[i])
        if i in CHECKED:
            line = f"t_idx {i:2d}:"
            for m, st in states.items():
                rec = {}
                with torch.no_grad(), gd.on_stream():
                    gd.guided_step(st, x_in.permute(0, 2, 3, 1).contiguous(), i, ts[i], r.unc[i], record=rec)
                eu = rel(rec["opt"][0] - x_in, rec_o["opt"][0] - x_in)
                eu3 = rel(rec["opt"][2] - x_in, rec_o["opt"][2] - x_in)
                worst[m] = [max(worst[m][0], eu), max(worst[m][1], eu3)]
                line += f"  {m}: S {rec['scale'][0]:g} first {eu:.3e} three {eu3:.3e}"
            print(line)
        x_in = rec_o["step"][0]
    print(f"worst over t_idx {CHECKED}: static first {worst['static'][0]:.3e} three {worst['static'][1]:.3e}; "
          f"auto first {worst['auto'][0]:.3e} three {worst['auto'][1]:.3e}")
    assert worst["auto"][0] <= GATE_FIRST and worst["auto"][1] <= GATE_THREE, worst
