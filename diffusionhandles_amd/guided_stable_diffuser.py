"""GuidedStableDiffuser on the native MI355X engine.

Same public surface as the reference class (guided_stable_diffuser.py:22-610): `.unet .vae
.text_encoder .tokenizer .scheduler .conf .device`, `to`, `get_image_shape`,
`get_feature_shape`, `init_prompt`, `init_depth`, `get_depth_intrinsics`,
`initial_inference`, `guided_inference`, `decode_latent_image`, `encode_latent_image`,
`process_correspondences`, `get_timesteps`, `prepare_extra_step_kwargs`, and
`StepGuidanceWeightSchedule`.

What differs underneath: the U-Net forward, the guidance energy with its gradient, the
backward-to-latent, the latent update and the CFG/DDIM step are explicit calls into the HIP
library (no autograd graph, no per-iteration host sync), activations stay channels-last
16-bit, and zero-weight energy terms are skipped (exact: 0 * finite = 0).
N = 0 / N = 1 correspondences are defined (fg term skipped / handled) instead of NaN / TypeError.
"""
import inspect
import os

import numpy as np
import torch

from . import _lib
from . import background_lock as _bl
from . import guidance_scale as _gs
from . import losses as _losses
from .guided_diffuser import GuidedDiffuser
from .losses import (MAX_BATCH_ITEMS, EnergyPlan, check_object_weights as _check_object_weights, energy_and_grad,
                     energy_and_grad_planned, energy_and_grad_planned_batch, process_correspondences as _process_correspondences)
from .scheduler import DDIMScheduler
from .unet import HipUNet, SD2_DEPTH

CFG_SCALE = 7.5


class GuidanceWeightSchedule:
    def __call__(self, denoising_step: int, optimization_step: int):
        return [1.0] * 3, [1.0] * 3


class StepGuidanceWeightSchedule(GuidanceWeightSchedule):
    """Piecewise-constant lookup: last entry with step <= query, per-layer product
    (guided_stable_diffuser.py:622-665)."""

    def __init__(self, denoising_steps, optimization_steps):
        for steps in (denoising_steps, optimization_steps):
            if not all(len(f) == len(b) for _, f, b in steps):
                raise ValueError("Number of foreground and background weights do not match.")
        if len(denoising_steps[0][1]) != len(optimization_steps[0][1]):
            raise ValueError("Number of denoising and optimization weights do not match.")
        self.denoising_steps = sorted(denoising_steps, key=lambda s: s[0])
        self.optimization_steps = sorted(optimization_steps, key=lambda s: s[0])

    @staticmethod
    def _lookup(table, q):
        hit = None
        for step, f, b in table:
            if q >= step:
                hit = (f, b)
        return hit

    def __call__(self, denoising_step: int, optimization_step: int):
        d = self._lookup(self.denoising_steps, denoising_step)
        o = self._lookup(self.optimization_steps, optimization_step)
        if d is None or o is None:
            raise ValueError(f"Could not find weights for denoising step {denoising_step} and optimization step "
                             f"{optimization_step}.")
        return [x * y for x, y in zip(d[0], o[0])], [x * y for x, y in zip(d[1], o[1])]


def build_weight_schedule(fg_weight, bg_weight, max_step, kind):
    """fg/bg_weight are the user-facing values; the x30 happens here (guided_stable_diffuser.py:336-373)."""
    wf, wb = fg_weight * 30, bg_weight * 30
    if kind == "constant":
        ff, fb = np.linspace(wf, wf, max_step), np.linspace(wb, wb, max_step)
    elif kind == "linear":
        ff, fb = np.linspace(wf, 0.0, max_step), np.linspace(wb, 0.0, max_step)
    elif kind == "quadratic":
        ff, fb = np.linspace(np.sqrt(wf), 0.0, max_step) ** 2, np.linspace(np.sqrt(wb), 0.0, max_step) ** 2
    else:
        raise ValueError(f"Unknown guidance schedule type: {kind}")
    pattern = [([0.0, 0.0, 7.5], [0.0, 0.0, 1.5]), ([0.0, 5.0, 0.0], [0.0, 1.5, 0.0]), ([0.0, 5.0, 7.5], [0.0, 1.5, 1.5])]
    den = []
    for t in range(max_step):
        pf, pb = pattern[t % 3]
        den.append((t, (np.array(pf) * ff[t]).tolist(), (np.array(pb) * fb[t]).tolist()))
    den.append((max_step, [0.0] * 3, [0.0] * 3))
    opt = [(0, [2.5] * 3, [1.25] * 3), (1, [1.25] * 3, [2.5] * 3), (2, [1.25] * 3, [1.25] * 3), (3, [2.5] * 3, [2.5] * 3)]
    return StepGuidanceWeightSchedule(den, opt)


class DonorActivations(list):
    """The channels-last engine-dtype copies [T,h,w,C] of a donor image's activations, one per captured layer (prepare_guidance
    makes them; K edits of one image share one instance, as they share `orig`)."""


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


class GuidedStableDiffuser(GuidedDiffuser):
    _text_keys = 0

    def __init__(self, conf, unet=None, vae=None, text_encoder=None, tokenizer=None, dtype=torch.float16,
                 unet_config=None, max_batch=2, synthetic_seed=0):
        """max_batch sizes the engine this diffuser builds in .to(device) (ignored when `unet` is handed in): the largest batch of
        ANY U-Net pass.  Contract (since round 5): K batched edits need max_batch >= 2 K (their CFG pass runs [uncond | cond] for
        every edit; guided_step_batch / guided_inference_batch / guided_inference_streams raise RuntimeError otherwise, lanes are
        never silently re-sized), and a forward that is SAVED for a backward pass -- unet.forward(save_for_backward=True), i.e.
        the optimisation passes and null-text inversion -- may be at most max_batch // 2 wide (the engine's max_diff_batch:
        only those passes keep every activation, which is what halves the arenas); a wider saved forward fails with the
        engine's "exceeds max_diff_batch" error.  Build a HipUNet yourself (max_diff_batch=...) for any other split."""
        super().__init__(conf=conf)
        self.scheduler = DDIMScheduler()
        self.dtype = dtype
        self._unet_config = dict(SD2_DEPTH if unet_config is None else unet_config)
        self._max_batch = max(2, int(max_batch))
        self._synthetic_seed = synthetic_seed
        self.unet = unet            # built lazily in .to(device): the engine lives on a GPU
        self.vae = vae
        self.text_encoder = text_encoder
        self.tokenizer = tokenizer
        self.device = torch.device("cpu")
        # fp16 needs the guidance gradient scaled through the backward pass
        self.grad_scale = 256.0 if dtype == torch.float16 else 1.0
        # conf.grad_scale 'auto' (absent = 'static'): a power-of-two scale per edit and (timestep, iteration) from a host bound
        # of the cotangent (guidance_scale.py), the guarded latent update and the flagged DDIM step, FloatingPointError at the
        # end of a call when an edit met a non-finite value
        self.grad_scale_mode = _gs.resolve_mode(conf)
        # guided_step drives the engine through its own I/O buffers (no device copies / torch.cat around the passes); False
        # routes the same kernels through caller-owned tensors (bit-identical; kept for tools/ab_inplace.py)
        self._inplace_io = True
        # the batched loops evaluate the planned energy of their K items in one launch pair (dh_energy_fwd_bwd_planned_batch);
        # False: one call per item (bit-identical; kept for tools/bench_edit_batch.py)
        self._batch_energy = True

    # ---- plumbing -----------------------------------------------------------------------
    def to(self, device=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("GuidedStableDiffuser runs on an MI355X HIP device only (no CPU fallback)")
        _lib.require_gpu()
        with torch.cuda.device(device):
            if self.unet is None:
                # the optimisation passes (saved for their backward) run half the batch of the CFG pass: only they size the arenas
                self.unet = HipUNet(self._unet_config, dtype=self.dtype, max_batch=self._max_batch,
                                    max_diff_batch=max(1, self._max_batch // 2), device=device)
                wdir = os.environ.get("DIFFHANDLES_UNET_SAFETENSORS")
                if wdir:
                    from safetensors.torch import load_file
                    self.unet.load_state_dict(load_file(wdir))
                else:
                    self.unet.init_synthetic(self._synthetic_seed)     # no checkpoint offline: seeded weights
            from .synthetic import SyntheticTextEncoder, SyntheticTokenizer, SyntheticVAE
            from .vae import AutoencoderKL, build_text_encoder
            # Checkpoints named through the environment run on the ENGINE's kernels (csrc/vae_engine.cpp, csrc/text_engine.cpp):
            # the PyTorch-ROCm modules of vae.py only carry the parameters (and serve as the tests' oracles).  "sd" / "sd2"
            # name those torch modules with random weights (test oracles), "sd-native" / "sd2-native" the native engines with
            # random weights; with nothing given the cheap deterministic stand-ins of synthetic.py are used (no checkpoints offline).
            if self.tokenizer is None and os.environ.get("DIFFHANDLES_TOKENIZER_DIR"):
                from transformers import CLIPTokenizer
                self.tokenizer = CLIPTokenizer.from_pretrained(os.environ["DIFFHANDLES_TOKENIZER_DIR"])
            text_native = isinstance(self.text_encoder, str) and self.text_encoder.endswith("-native")
            if self.text_encoder is None and os.environ.get("DIFFHANDLES_TEXT_ENCODER_DIR"):
                self.text_encoder = build_text_encoder(os.environ["DIFFHANDLES_TEXT_ENCODER_DIR"])
                text_native = True
            elif isinstance(self.text_encoder, str):
                # (manual_seed also re-seeds every device generator, lazily: the fork must cover the current device as well, or a
                #  caller that draws noise on the device after building the diffuser gets a different stream)
                with torch.random.fork_rng(devices=[device]):      # random weights, but the SAME in every process (seeded like the U-Net's)
                    torch.manual_seed(1000 + self._synthetic_seed)
                    self.text_encoder = build_text_encoder()       # the SD-2 text configuration
            if text_native:
                from .vae import HipTextEncoder
                tc = self.text_encoder.config.to_dict()
                keys = ("hidden_size", "num_attention_heads", "num_hidden_layers", "intermediate_size", "max_position_embeddings",
                        "layer_norm_eps", "hidden_act", "vocab_size")
                self.text_encoder = HipTextEncoder({k: tc[k] for k in keys if k in tc}, self.dtype, max_batch=2,
                                                   device=device).load_state_dict(self.text_encoder.state_dict())
            from .vae import NativeDecodeVAE
            if self.vae is None and os.environ.get("DIFFHANDLES_VAE_SAFETENSORS"):
                self.vae = NativeDecodeVAE(AutoencoderKL.from_safetensors(os.environ["DIFFHANDLES_VAE_SAFETENSORS"]),
                                           self._unet_config["sample_size"], self.dtype)
            elif isinstance(self.vae, str):
                native = self.vae == "sd-native"
                with torch.random.fork_rng(devices=[device]):      # (two runs of a driver must decode with the same random VAE)
                    torch.manual_seed(2000 + self._synthetic_seed)
                    self.vae = AutoencoderKL()
                if native:
                    self.vae = NativeDecodeVAE(self.vae, self._unet_config["sample_size"], self.dtype)
            if self.tokenizer is None:
                self.tokenizer = SyntheticTokenizer()
            if self.text_encoder is None:
                self.text_encoder = SyntheticTextEncoder(dim=self._unet_config["cross_attention_dim"])
            if self.vae is None:
                self.vae = SyntheticVAE()
            self.text_encoder = self.text_encoder.to(device)
            self.vae = self.vae.to(device)
        self.device = device
        # a created (non-default) stream: the engine replays its passes as hipGraphs, which the legacy
        # default stream cannot capture
        self._stream = torch.cuda.Stream(device=device)
        return self

    class _on_stream:
        """Run a block on the diffuser's stream, ordered after / before the caller's current stream."""

        def __init__(self, gd):
            self.gd = gd

        def __enter__(self):
            self.outer = torch.cuda.current_stream(self.gd.device)
            self.gd._stream.wait_stream(self.outer)
            self.ctx = torch.cuda.stream(self.gd._stream)
            self.ctx.__enter__()

        def __exit__(self, *a):
            self.ctx.__exit__(*a)
            self.outer.wait_stream(self.gd._stream)

    def on_stream(self):
        return GuidedStableDiffuser._on_stream(self)

    def get_image_shape(self):
        f = self.get_feature_shape()
        s = 2 ** (len(self.vae.config.block_out_channels) - 1)
        return (f[0] * s, f[1] * s, 3)

    def get_feature_shape(self):
        hw = self.unet.sample_size
        hw = (hw, hw) if isinstance(hw, int) else hw
        return (hw[0], hw[1], self.unet.config.out_channels)

    def _encode(self, texts):
        ids = self.tokenizer(texts, padding="max_length", max_length=self.tokenizer.model_max_length, truncation=True,
                             return_tensors="pt")
        return self.text_encoder(ids.input_ids.to(self.device))[0].float()

    @torch.no_grad()
    def init_prompt(self, prompt: str):
        return torch.cat([self._encode([""]), self._encode([prompt])])

    @torch.no_grad()
    def init_depth(self, depth):
        h, w = self.get_feature_shape()[:2]
        depth = torch.nn.functional.interpolate(depth, size=(h, w), mode="bicubic", align_corners=False)
        lo = torch.amin(depth, dim=[1, 2, 3], keepdim=True)
        hi = torch.amax(depth, dim=[1, 2, 3], keepdim=True)
        return 2.0 * (depth - lo) / (hi - lo) - 1.0

    @staticmethod
    def get_depth_intrinsics(device=None):
        f = 1.0 / np.tan(0.5 * 55.0 * (np.pi / 180.0))
        return torch.tensor([[f, 0, 0], [0, f, 0], [0, 0, 1]], dtype=torch.float32, device=device)

    def encode_latent_image(self, image):
        raise NotImplementedError

    def decode_latent_image(self, latent_image):
        image = self.vae.decode(latent_image / self.vae.config.scaling_factor, return_dict=False)[0]
        return (image / 2 + 0.5).clamp(0, 1)

    def process_correspondences(self, correspondences, img_res, bg_erosion=0):
        return _process_correspondences(correspondences, img_res, bg_erosion, grid=self.unet.sample_size,
                                        device=self.device)

    def get_timesteps(self, num_inference_steps, strength):
        init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
        t_start = max(num_inference_steps - init_timestep, 0)
        return self.scheduler.timesteps[t_start * self.scheduler.order:], num_inference_steps - t_start

    def prepare_extra_step_kwargs(self, generator, eta):
        keys = set(inspect.signature(self.ddim_step).parameters.keys())
        kw = {}
        if "eta" in keys:
            kw["eta"] = eta
        if "generator" in keys:
            kw["generator"] = generator
        return kw

    # ---- native loop pieces --------------------------------------------------------------
    def ddim_step(self, x, eps_u, eps_c, t, scale=CFG_SCALE, eta=0.0, generator=None, out=None):
        """x, eps: [B,H,W,4] f32 channels-last.  CFG combine + DDIM step in one kernel.  out: where to write the result (a
        contiguous f32 tensor of x's shape, not x itself); None: a new tensor."""
        a_t, a_p = self.scheduler.step_alphas(t)
        if out is None:
            out = torch.empty_like(x)
        elif out.shape != x.shape or out.dtype != x.dtype or not out.is_contiguous() or out.data_ptr() == x.data_ptr():
            raise ValueError("ddim_step: out must be a contiguous tensor of x's shape and dtype, and not x")
        L = _lib.lib()
        _lib.check(L.dh_ddim_cfg_step(_lib.ptr(out), _lib.ptr(x), _lib.ptr(eps_u), _lib.ptr(eps_c), float(scale), a_t,
                                      a_p, x.numel(), _lib.stream_ptr()), "dh_ddim_cfg_step")
        return out

    def _ddim_step_flagged(self, x, eps_u, eps_c, t, status, t_idx, iteration, scale=CFG_SCALE):
        """ddim_step, plus the status bit of every edit (batch item) whose output has a non-finite element."""
        a_t, a_p = self.scheduler.step_alphas(t)
        out = torch.empty_like(x)
        _lib.check(_lib.lib().dh_ddim_cfg_step_flagged(_lib.ptr(out), _lib.ptr(x), _lib.ptr(eps_u), _lib.ptr(eps_c), float(scale),
                                                       a_t, a_p, x.numel(), x[0].numel(), _lib.ptr(status), int(t_idx),
                                                       int(iteration), _lib.stream_ptr()), "dh_ddim_cfg_step_flagged")
        return out

    def _ddim_step_locked(self, sts, x, eps_u, eps_c, t, status, t_idx, iteration, scale=CFG_SCALE):
        """The DDIM step of a batch in which some edit has a background lock (dh_ddim_cfg_step_locked, one launch in place
        of the step's one launch): edit e's output is blended with sts[e].lock.ref[t_idx] by sts[e].lock.keep; states without
        a lock get the plain step.  status: the [K, 4] status words ('auto'), or None ('static')."""
        K = x.shape[0]
        if K > _bl.MAX_ITEMS:
            raise RuntimeError(f"background lock: {K} edits in one step, at most {_bl.MAX_ITEMS}")
        a_t, a_p = self.scheduler.step_alphas(t)
        out = torch.empty_like(x)
        items = (_lib.LockItem * K)()
        for e, st in enumerate(sts):
            if st.lock is not None:
                items[e].keep, items[e].ref = st.lock.keep.data_ptr(), st.lock.ref[t_idx].data_ptr()
        _lib.check(_lib.lib().dh_ddim_cfg_step_locked(_lib.ptr(out), _lib.ptr(x), _lib.ptr(eps_u), _lib.ptr(eps_c), float(scale),
                                                      a_t, a_p, x.numel(), x[0].numel(), x.shape[-1], items, K,
                                                      _lib.ptr(status), int(t_idx), int(iteration), _lib.stream_ptr()),
                   "dh_ddim_cfg_step_locked")
        return out

    def _latent_update_guarded(self, x_new, x, d_sample, table, status, t_idx, iteration):
        """x_new = x - 0.1 d_sample / S per edit (batch item), held where the edit's d_sample has a non-finite element.
        table: [edits, T, I] device scales."""
        E, T, I = table.shape
        _lib.check(_lib.lib().dh_latent_update_guarded(_lib.ptr(x_new), _lib.ptr(x), _lib.ptr(d_sample), d_sample.shape[-1],
                                                       x.shape[-1], 0.1, x[0].numel() // x.shape[-1], E, _lib.ptr(table),
                                                       T * I, t_idx * I + iteration, _lib.ptr(status), None, int(t_idx),
                                                       int(iteration), _lib.stream_ptr()), "dh_latent_update_guarded")

    @staticmethod
    def raise_on_status(statuses):
        """statuses: list of (edit index, host int[4] status of dh_latent_update_guarded / dh_ddim_cfg_step_flagged).  Raises
        FloatingPointError naming every failing edit with its first (t_idx, iteration) and what failed; .edits = their indices."""
        bad = []
        for e, s in statuses:
            s = [int(v) for v in s]
            if s[0] == 0:
                continue
            code = s[2]
            t_idx, it, kind = (code >> 16) - 1, (code >> 8) & 0xff, code & 0xff
            what = "backward overflow, update held" if kind == 1 else "non-finite latent after the DDIM step"
            extra = f" ({s[1]} updates held)" if s[1] else ""
            bad.append((e, f"edit {e}: {what} at (t_idx={t_idx}, iteration={it}){extra}"))
        if bad:
            err = FloatingPointError("guided edit hit a non-finite value: " + "; ".join(m for _, m in bad))
            err.edits = [e for e, _ in bad]
            raise err

    def _unet_input(self, x, depth_nhwc, reps=1):
        """x [1,H,W,4], depth [1,H,W,1] -> [reps,H,W,5]"""
        s = torch.cat([x, depth_nhwc], dim=-1) if self.conf.use_depth else x
        return s.expand(reps, -1, -1, -1).contiguous() if reps > 1 else s.contiguous()

    def _cfg_eps(self, x, depth_nhwc, t, uncond, cond, want_acts=False, inplace=False):
        """(eps_uncond, eps_cond[, activations]) of the B=2 classifier-free-guidance pass.  inplace: the input is packed into
        the engine's buffer by one launch and eps comes back as views of the engine's output (valid until the next pass)."""
        text = torch.cat([uncond.reshape(1, *cond.shape[1:]).to(self.device, torch.float32), cond]).contiguous()
        if inplace and x.shape[0] == 1:
            sample = self.unet.stage_sample(x, depth_nhwc if self.conf.use_depth else None, 2)
        else:
            sample = self._unet_input(x, depth_nhwc, 2)
        eps, acts = self.unet.forward(sample, float(t), text, save_for_backward=False, want_acts=want_acts, inplace=inplace)
        return (eps[0:1], eps[1:2], acts) if want_acts else (eps[0:1], eps[1:2])

    # ---- reference API ----------------------------------------------------------------------
    @torch.no_grad()
    def initial_inference(self, init_latents, depth, uncond_embeddings, prompt):
        """Returns (activations [3 x [T,C,h,w]], latents [1,4,H,W], uncond_embeddings, init_latents).  activations is a list
        subclass (background_lock.Activations) whose .trajectory [T,4,H,W] f32 holds the latent after every DDIM step."""
        with self.on_stream():
            return self._initial_inference(init_latents, depth, uncond_embeddings, prompt)

    def _initial_inference(self, init_latents, depth, uncond_embeddings, prompt):
        torch.manual_seed(self.conf.seed)
        self.scheduler.set_timesteps(self.conf.num_timesteps, device=self.device)
        timesteps, _ = self.get_timesteps(self.conf.num_timesteps, 1.0)
        depth_nhwc = _nhwc(self.init_depth(depth.to(self.device, torch.float32))) if self.conf.use_depth else None
        cond = self._encode([prompt]).contiguous()
        if uncond_embeddings is None:
            uncond_embeddings = self._encode([""])[None].expand(len(timesteps), -1, -1, -1)
        s = self.unet.sample_size
        if init_latents is None:
            nlat = self.unet.config.in_channels - 1 if self.conf.use_depth else self.unet.config.in_channels
            noise = torch.randn([1, nlat, s, s], dtype=torch.float32).to(self.device)
            init_latents = self.scheduler.add_noise(torch.zeros_like(noise), noise, timesteps[0])
        x = _nhwc(init_latents.to(self.device, torch.float32))
        T = len(timesteps)
        store = [torch.empty((T,) + shp, dtype=self.dtype, device=self.device) for shp in self.unet.act_shapes]
        # the reconstruction trajectory (background lock): every step writes its latent into its slice, no extra launch
        traj = torch.empty((T,) + tuple(x.shape[1:]), dtype=torch.float32, device=self.device)
        for t_idx, t in enumerate(timesteps):
            # the reference runs a cond-only B=1 pass for the activations and then the B=2 CFG pass (guided_stable_diffuser.py
            # :222-257: three samples per step); the conditional half of the CFG pass has exactly the inputs of the B=1 pass, so
            # the activations are captured there (two samples per step).  Same values up to the engine's batch-dependent tile
            # selection (16-bit: < 1e-2 against the oracle's B=1 activations, tests/test_loops_gpu.py).
            eu, ec, acts = self._cfg_eps(x, depth_nhwc, t, uncond_embeddings[t_idx], cond, want_acts=True)
            for k in range(3):
                store[k][t_idx].copy_(acts[k][1])
            x = self.ddim_step(x, eu, ec, t, out=traj[t_idx:t_idx + 1])
        # [T,C,h,w] views of channels-last storage
        activations = _bl.Activations([a.permute(0, 3, 1, 2) for a in store], trajectory=traj.permute(0, 3, 1, 2))
        return activations, x.permute(0, 3, 1, 2), uncond_embeddings, init_latents

    @torch.no_grad()
    def initial_inference_batch(self, init_latents, depths, uncond_embeddings, prompts):
        """initial_inference for K images of the engine's resolution in B = 2K CFG passes (not in the reference).  Lists of K
        in (init_latents / uncond_embeddings entries may be None, or the lists themselves None), one (activations, latents,
        uncond_embeddings, init_latents) per image out.  Needs max_batch >= 2K.  Every image is seeded as its own
        initial_inference call would be (torch.manual_seed(conf.seed) per image, so images without init_latents share the
        noise), and its activations come from its conditional half, the capture rule of initial_inference; at K = 1 the
        result is bit-identical to initial_inference."""
        K = len(prompts)
        init_latents = [None] * K if init_latents is None else list(init_latents)
        uncond_embeddings = [None] * K if uncond_embeddings is None else list(uncond_embeddings)
        if K < 1 or not (len(depths) == len(init_latents) == len(uncond_embeddings) == K):
            raise ValueError("initial_inference_batch: init_latents, depths, uncond_embeddings and prompts must be non-empty "
                             "and of the same length")
        if self.unet.max_batch < 2 * K:
            raise RuntimeError(f"engine max_batch {self.unet.max_batch} < 2*K = {2 * K}: build the diffuser with "
                               f"max_batch >= {2 * K}")
        s = self.unet.sample_size
        for b, lat in enumerate(init_latents):
            if lat is not None and tuple(lat.shape[-2:]) != (s, s):
                raise ValueError(f"initial_inference_batch: init_latents {b} is {tuple(lat.shape[-2:])}, the engine runs "
                                 f"{(s, s)} latents")
        with self.on_stream():
            return self._initial_inference_batch(init_latents, depths, uncond_embeddings, prompts)

    def _initial_inference_batch(self, init_latents, depths, uncond_embeddings, prompts):
        K = len(prompts)
        self.scheduler.set_timesteps(self.conf.num_timesteps, device=self.device)
        timesteps, _ = self.get_timesteps(self.conf.num_timesteps, 1.0)
        T = len(timesteps)
        s = self.unet.sample_size
        inits, uncs = [], []
        for lat, unc in zip(init_latents, uncond_embeddings):
            torch.manual_seed(self.conf.seed)              # as K initial_inference calls, one after the other
            if lat is None:
                nlat = self.unet.config.in_channels - 1 if self.conf.use_depth else self.unet.config.in_channels
                noise = torch.randn([1, nlat, s, s], dtype=torch.float32).to(self.device)
                lat = self.scheduler.add_noise(torch.zeros_like(noise), noise, timesteps[0])
            inits.append(lat)
            uncs.append(self._encode([""])[None].expand(T, -1, -1, -1) if unc is None else unc)
        depth_nhwc = None
        if self.conf.use_depth:
            depth_nhwc = torch.cat([_nhwc(self.init_depth(d.to(self.device, torch.float32))) for d in depths])
        cond = torch.cat([self._encode([p]) for p in prompts]).contiguous()
        x = torch.cat([_nhwc(lat.to(self.device, torch.float32)) for lat in inits])
        store = [[torch.empty((T,) + shp, dtype=self.dtype, device=self.device) for shp in self.unet.act_shapes]
                 for _ in range(K)]
        traj = torch.empty((T,) + tuple(x.shape), dtype=torch.float32, device=self.device)      # [T,K,s,s,4]: initial_inference's, per image
        for t_idx, t in enumerate(timesteps):
            # [uncond_1 .. uncond_K | cond_1 .. cond_K]: image b's conditional half is batch item K + b
            unc = torch.cat([u[t_idx].reshape(1, *cond.shape[1:]).to(self.device, torch.float32) for u in uncs])
            text = torch.cat([unc, cond]).contiguous()
            sample = self._unet_input(x, depth_nhwc).repeat(2, 1, 1, 1)
            eps, acts = self.unet.forward(sample, float(t), text, save_for_backward=False, want_acts=True)
            for b in range(K):
                for k in range(3):
                    store[b][k][t_idx].copy_(acts[k][K + b])
            x = self.ddim_step(x, eps[:K], eps[K:], t, out=traj[t_idx])
        return [(_bl.Activations([a.permute(0, 3, 1, 2) for a in store[b]], trajectory=traj[:, b].permute(0, 3, 1, 2)),
                 x[b:b + 1].permute(0, 3, 1, 2), uncs[b], inits[b]) for b in range(K)]

    def _check_object_weights(self, object_labels, object_weights, activations_orig, pair_instances=None):
        """Host checks of prepare_guidance's object weights, before any device work: labels present, default configuration."""
        if object_labels is not None and pair_instances is not None:
            raise ValueError("object_labels and pair_instances are mutually exclusive")
        if object_labels is None and pair_instances is None:
            raise ValueError("object_weights need object_labels (the label image of the object masks)")
        if self.conf.fg_patch_size != 1:
            raise NotImplementedError(f"object_weights with fg_patch_size = {self.conf.fg_patch_size} (only 1: the weighted "
                                      "energy has no pooled form)")
        if self.conf.bg_loss_type != "global_avg":
            raise NotImplementedError(f"object_weights with bg_loss_type = {self.conf.bg_loss_type!r} (only 'global_avg')")
        size = tuple(activations_orig[2].shape[-2:])
        for k in (1, 2):                     # the layers build_weight_schedule guides
            if tuple(activations_orig[k].shape[-2:]) != size:
                raise NotImplementedError(f"object_weights with guided layer {k} off the cell grid "
                                          f"({tuple(activations_orig[k].shape[-2:])} / {size})")
        # (the number of objects is the label image's: the facade checks the length against its masks)
        n = len(object_weights) if hasattr(object_weights, "__len__") and not isinstance(object_weights, str) else 0
        _check_object_weights(object_weights, n)

    def prepare_guidance(self, depth, prompt, activations_orig, correspondences, fg_weight=None, bg_weight=None, orig=None,
                         cond=None, object_labels=None, object_weights=None, pair_instances=None, row_kind=None, donor=None, vacated=None,
                         lock=None):
        """Everything of guided_inference that is constant over the denoising loop.  `lock` (background lock): (keep [s,s],
        trajectory [T,4,s,s]) -- the keep map of this edit (background_lock.keep_map) and the reconstruction trajectory of its
        image (activations.trajectory) -- or a prepared background_lock.Lock (edits of one image share the channels-last copy
        of the trajectory, as they share `orig`); after every DDIM step the edit's latents are then blended with the
        reconstruction's (DESIGN.md "Background lock").  `orig`: the channels-last copies of
        the original activations of another guidance state of the SAME image (K edits of one image share them); `cond`: the
        prompt embedding when the caller already has it (lanes: the text tower is not run concurrently with itself).
        object_labels / object_weights (multi-object edits): the label image of the object masks (losses.object_label_image)
        and "equal" or one weight per object -- the foreground term then weighs the objects by omega_m instead of by their
        pair counts (DESIGN.md "A weight per object").  None: the area weighting, on the unchanged path.
        pair_instances (edits with copies of an object): the instance of every correspondence row, uint8 [N], IN PLACE OF the
        label image (giving both is a ValueError) -- an object of the energy is then an instance, object_weights has one entry
        per instance.
        vacated (edits that DELETE objects, DESIGN.md "Object removal"): the [H, W] image of the pixels the removed objects
        leave behind; their cells leave the original-background list of the energy (losses.process_correspondences).  The
        correspondences may then be empty (a pure removal: the background term runs alone).  None: the call without it.
        donor (edits that bring in objects of ANOTHER image, DESIGN.md "Object insertion"): (activations_donor, row_donor) -- the
        donor image's identity activations (as activations_orig, with its numbers of timesteps and layers; or the
        DonorActivations another guidance state of the same edit batch made of them) and one byte per correspondence row,
        non-zero where the row's source pixel lies in the donor image.  pair_instances is then required (an object of the
        energy is an instance, and a donor row's instance is a donor object).  A donor row's pair reads its source feature from
        the donor's activations, clears its target cell and leaves the original-background list alone.  Donor edits always run
        on the weighted plan: object_weights=None means w_m = N_m, which gives every pair the unweighted coefficient
        fg_w / (C N) up to rounding.  Default configuration only (planned path, fg_patch_size 1, global_avg; NotImplementedError
        naming the setting otherwise); grad_scale 'auto' takes its bound from the weighted plan, as it does for weights.
        None: the call without it.
        row_kind (edits that move the CAMERA, DESIGN.md "Camera moves"): one byte per correspondence row, 2 on the background
        rows of the re-projection (0 on an object's).  A background row forms its pair and clears neither background list
        (losses.process_correspondences).  Without object_weights the rows join the pairs of the unweighted plan; with them
        pair_instances is required and the background is its instance N (object_weights then has N + 1 entries).
        NotImplementedError together with donor.  None: the call without it."""
        from types import SimpleNamespace
        vacated = _losses.check_vacated(vacated, depth.shape[-1], "prepare_guidance")
        if row_kind is not None:
            if donor is not None:
                raise NotImplementedError("prepare_guidance: row_kind (a camera move) together with donor is not supported")
            row_kind = _losses.check_row_kind(row_kind, int(torch.as_tensor(correspondences).reshape(-1, 4).shape[0]),
                                              "prepare_guidance")
            if object_weights is not None and pair_instances is None:
                raise ValueError("prepare_guidance: row_kind with object_weights needs pair_instances (the background is "
                                 "instance N)")
        if donor is not None:
            donor = self._check_donor(donor, activations_orig, correspondences, pair_instances, object_labels)
        if object_labels is not None and pair_instances is not None:
            raise ValueError("object_labels and pair_instances are mutually exclusive")
        if object_weights is not None:
            self._check_object_weights(object_labels, object_weights, activations_orig, pair_instances)
        fg_weight = self.conf.fg_weight if fg_weight is None else fg_weight
        bg_weight = self.conf.bg_weight if bg_weight is None else bg_weight
        st = SimpleNamespace()
        if donor is not None:
            st.pc = _process_correspondences(correspondences, depth.shape[-1], self.conf.bg_erosion, grid=self.unet.sample_size,
                                             device=self.device, vacated=vacated, pair_instances=pair_instances,
                                             row_donor=donor[1])
        elif row_kind is not None:
            st.pc = _process_correspondences(correspondences, depth.shape[-1], self.conf.bg_erosion, grid=self.unet.sample_size,
                                             device=self.device, vacated=vacated, row_kind=row_kind,
                                             pair_instances=pair_instances if object_weights is not None else None)
        elif object_weights is None and vacated is None:
            st.pc = self.process_correspondences(correspondences, img_res=depth.shape[-1], bg_erosion=self.conf.bg_erosion)
        elif object_weights is None:
            st.pc = _process_correspondences(correspondences, depth.shape[-1], self.conf.bg_erosion, grid=self.unet.sample_size,
                                             device=self.device, vacated=vacated)
        else:
            st.pc = _process_correspondences(correspondences, depth.shape[-1], self.conf.bg_erosion, grid=self.unet.sample_size,
                                             device=self.device, vacated=vacated, object_labels=object_labels,
                                             pair_instances=pair_instances)
        st.depth_nhwc = _nhwc(self.init_depth(depth.to(self.device, torch.float32))) if self.conf.use_depth else None
        st.cond = self._encode([prompt]).contiguous() if cond is None else cond
        GuidedStableDiffuser._text_keys += 1
        st.cond_key = GuidedStableDiffuser._text_keys          # names st.cond for the engine's text K|V cache
        st.schedule = build_weight_schedule(fg_weight, bg_weight, self.conf.guidance_max_step,
                                            self.conf.guidance_schedule_type)
        # original activations as channels-last engine-dtype storage [T,h,w,C]
        st.orig = orig if orig is not None else \
            [a.to(self.device).permute(0, 2, 3, 1).to(self.dtype).contiguous() for a in activations_orig]
        st.size = (st.orig[2].shape[1], st.orig[2].shape[2])
        st.n_pairs = len(st.pc["original_x"])
        # default configuration: the energy runs through a per-edit plan (CSR + background flags built once)
        st.plan = None
        if (self.conf.fg_patch_size == 1 and self.conf.bg_loss_type == "global_avg"
                and all(o.shape[1] == st.size[0] and o.shape[2] == st.size[1] for o in st.orig[1:])):
            st.plan = EnergyPlan(st.pc, st.size[0], self.device, object_weights=object_weights, force_weighted=donor is not None)
        elif donor is not None:
            raise NotImplementedError("donor: guided layers off the cell grid (a donor edit needs the planned energy: default "
                                      "configuration, layers on the cell grid)")
        elif object_weights is not None:
            raise NotImplementedError("object_weights need the planned energy (default configuration, layers on the cell grid)")
        weighted = st.plan is not None and st.plan.weighted
        st.auto = self.grad_scale_mode == "auto"
        if st.auto:
            # S per (timestep, iteration): host copy for the energy calls, device copy for the guarded update
            st.scale_host, st.bounds = _gs.scale_table(
                st.pc, st.size[0], [tuple(o.shape[1:]) for o in st.orig], st.schedule, int(self.conf.num_timesteps),
                int(self.conf.num_optsteps), int(self.conf.guidance_max_step), self.conf.fg_patch_size,
                self.conf.bg_patch_size, self.conf.bg_loss_type, objects=st.pc["object"] if weighted else None,
                omega=st.plan.omega if weighted else None)
            st.scale_dev = torch.tensor(st.scale_host, dtype=torch.float32).to(self.device)[None].contiguous()
            st.status = torch.zeros((1, 4), dtype=torch.int32, device=self.device)
        st.lock = self._locks(lock, 1, "prepare_guidance")[0]
        st.donor, st.donor_bits = None, 0
        if donor is not None:
            # the donor objects of the energy: the instances of the flagged rows (one host read per edit, outside the loop)
            flagged = torch.as_tensor(pair_instances).reshape(-1).cpu()[torch.as_tensor(donor[1]).reshape(-1).cpu() != 0]
            for m in set(flagged.tolist()):
                st.donor_bits |= 1 << int(m)
            st.donor_bits &= (1 << st.plan.n_objects) - 1          # (an instance past the last one with kept pairs has none)
            acts = donor[0]
            st.donor = acts if isinstance(acts, DonorActivations) else DonorActivations(
                a.to(self.device).permute(0, 2, 3, 1).to(self.dtype).contiguous() for a in acts)
        return st

    def _check_donor(self, donor, activations_orig, correspondences, pair_instances, object_labels):
        """Host checks of prepare_guidance's donor, before any device work: the pair, the row flags' length, the instance
        column, the donor activations' layers and timesteps against the host's, the default configuration."""
        what = "prepare_guidance: donor"
        if not isinstance(donor, (tuple, list)) or len(donor) != 2:
            raise ValueError(f"{what}: expected (activations_donor, row_donor)")
        acts, row_donor = donor
        if acts is None or row_donor is None:
            raise ValueError(f"{what}: {'activations' if acts is None else 'row_donor'} missing")
        if pair_instances is None or object_labels is not None:
            raise ValueError(f"{what}: needs pair_instances (the instance of every correspondence row), not a label image")
        n_rows = int(torch.as_tensor(correspondences).reshape(-1, 4).shape[0])
        row_donor = _losses.check_row_donor(row_donor, n_rows, what)
        if len(acts) != len(activations_orig):
            raise ValueError(f"{what}: activations of {len(acts)} layers, the host's have {len(activations_orig)}")
        for k, (a, o) in enumerate(zip(acts, activations_orig)):
            if a.shape[0] != o.shape[0]:
                raise ValueError(f"{what}: activations of layer {k} hold {a.shape[0]} timesteps, the host's {o.shape[0]}")
            # (prepared copies are channels-last [T,h,w,C], identity activations [T,C,h,w])
            host_shape = (o.shape[2], o.shape[3], o.shape[1]) if isinstance(acts, DonorActivations) else tuple(o.shape[1:])
            if tuple(a.shape[1:]) != host_shape:
                raise ValueError(f"{what}: activations of layer {k} have shape {tuple(a.shape)}, the host's {tuple(o.shape)}")
        if self.conf.fg_patch_size != 1:
            raise NotImplementedError(f"donor with fg_patch_size = {self.conf.fg_patch_size} (only 1: the weighted energy has no "
                                      "pooled form)")
        if self.conf.bg_loss_type != "global_avg":
            raise NotImplementedError(f"donor with bg_loss_type = {self.conf.bg_loss_type!r} (only 'global_avg')")
        return acts, row_donor

    def _locks(self, lock, K, what):
        """`lock` of a loop call as K prepared background_lock.Lock / None (edits of one image share the trajectory's copy)."""
        return _bl.prepare_locks(lock, K, self.device, self.unet.sample_size, int(self.conf.num_timesteps), what)

    def _energy_grad(self, st, k, act, t_idx, fgw, bgw, out=None, scale=None):
        """d(energy of layer k)/d(act) * scale (default grad_scale), act [h,w,C] channels-last; `out`: where to write it."""
        scale = self.grad_scale if scale is None else scale
        if st.plan is not None and st.donor_bits:          # (prepare_guidance made sure the plan covers every guided layer)
            return _losses.energy_and_grad_planned_donor(act, st.orig[k][t_idx], st.plan, fgw, bgw, st.donor[k][t_idx],
                                                         st.donor_bits, grad_scale=scale, out=out)[1]
        if st.plan is not None and act.shape[0] == st.plan.grid and act.shape[1] == st.plan.grid:
            return energy_and_grad_planned(act, st.orig[k][t_idx], st.plan, fgw, bgw, grad_scale=scale, out=out)[1]
        return energy_and_grad(act, st.orig[k][t_idx], st.pc, fgw, bgw, self.conf.fg_patch_size, self.conf.bg_patch_size,
                               st.size, self.conf.bg_loss_type, grad_scale=scale, out=out)[1]

    @staticmethod
    def _latent_buffer(st, x, iteration):
        """The latent of optimisation iteration `iteration`: two buffers per guidance state, used alternately (the update reads
        the previous iteration's buffer or the caller's tensor and writes the other one; the DDIM step that follows allocates its
        own output, so nothing the caller holds is ever overwritten) -- no allocation inside the step loop."""
        bufs = st.__dict__.setdefault("_xbuf", [None, None])
        k = iteration & 1
        if bufs[k] is None or bufs[k].shape != x.shape or bufs[k].device != x.device:
            bufs[k] = torch.empty_like(x)
        return bufs[k]

    def guided_step(self, st, x, t_idx, t, uncond, record=None, images=None):
        """One guided-denoise step (guided_stable_diffuser.py:377-479): up to num_optsteps x
        {U-Net forward, energy + gradient, backward-to-latent, latent update}, then the CFG
        forward (B=2) and the DDIM step.  x: [1,H,W,4] f32 channels-last.  `images` (save_denoising_steps): this
        timestep's list, which receives the decoded image after the optimisation loop and after the DDIM step
        (reference :385-386, 446-448, 476-478)."""
        L = _lib.lib()
        iteration = 0
        while iteration < self.conf.num_optsteps and t_idx < self.conf.guidance_max_step:
            fgw, bgw = st.schedule(t_idx, iteration)
            active = [k for k in range(3) if (fgw[k] != 0.0 and st.n_pairs > 0) or bgw[k] != 0.0]
            if active:
                # no copies either side of the engine: the input is packed into the engine's buffer by one launch, the
                # energy kernels read the captured activations where the engine left them and write their cotangents where
                # its backward pass starts from, the latent update reads d(sample) in place (its first 4 of 5 channels)
                ip = self._inplace_io
                sample = self.unet.stage_sample(x, st.depth_nhwc if self.conf.use_depth else None, 1) if ip else \
                    self._unet_input(x, st.depth_nhwc)
                _, acts = self.unet.forward(sample, float(t), st.cond, save_for_backward=True, want_acts=active, want_eps=False,
                                            text_key=st.cond_key, inplace=ip)
                d_acts = [None, None, None]
                S = float(st.scale_host[t_idx, iteration]) if st.auto else self.grad_scale
                for k in active:
                    d_acts[k] = self.unet.io_view("act_grad", k)[:1] if ip else torch.empty_like(acts[k])
                    self._energy_grad(st, k, acts[k][0], t_idx, fgw[k], bgw[k], out=d_acts[k][0], scale=S)
                d_sample, _ = self.unet.backward(d_acts, None, want_sample_grad=True, want_text_grad=False, inplace=ip)
                x_new = self._latent_buffer(st, x, iteration)
                if st.auto:
                    self._latent_update_guarded(x_new, x, d_sample, st.scale_dev, st.status, t_idx, iteration)
                else:
                    _lib.check(L.dh_latent_update_strided(_lib.ptr(x_new), _lib.ptr(x), _lib.ptr(d_sample), d_sample.shape[-1],
                                                          x.shape[-1], 0.1, self.grad_scale, x.numel() // x.shape[-1],
                                                          _lib.stream_ptr()), "dh_latent_update_strided")
                if record is not None:
                    record.setdefault("scale", []).append(S)
                    record.setdefault("grad", []).append((d_sample[..., :x.shape[-1]].float() / S).permute(0, 3, 1, 2).clone())
                x = x_new
            if record is not None:
                record.setdefault("opt", []).append(x.permute(0, 3, 1, 2).clone())
            iteration += 1
        if images is not None:
            images.append(self.decode_latent_image(x.permute(0, 3, 1, 2)).cpu())
        eu, ec = self._cfg_eps(x, st.depth_nhwc, t, uncond, st.cond, inplace=self._inplace_io)      # (views: consumed by the step right here)
        if st.lock is not None:
            x = self._ddim_step_locked([st], x, eu, ec, t, st.status if st.auto else None, t_idx, iteration)
        elif st.auto:
            x = self._ddim_step_flagged(x, eu, ec, t, st.status, t_idx, iteration)
        else:
            x = self.ddim_step(x, eu, ec, t)
        if images is not None:
            images.append(self.decode_latent_image(x.permute(0, 3, 1, 2)).cpu())
        return x

    # ---- batched edits: K transforms of ONE image identity in one U-Net batch (BASELINE config 3) ------
    def guided_step_batch(self, sts, x, t_idx, t, uncond):
        """x: [K,H,W,4]; sts: K guidance states (same prompt / original activations, different edits)."""
        K = x.shape[0]
        cond = sts[0].cond.expand(K, -1, -1).contiguous()
        unc = uncond.reshape(1, *cond.shape[1:]).to(self.device, torch.float32).expand(K, -1, -1)
        return self._guided_step_rows(sts, x, t_idx, t, cond, sts[0].cond_key, unc)

    # ---- batched edits of DIFFERENT images: every item has its own prompt, depth, original activations and unconditional row ----
    def guided_step_items(self, sts, x, t_idx, t, unconds):
        """One guided-denoise step of K unrelated items in one U-Net batch.  x: [K,H,W,4]; sts: K guidance states
        (prepare_guidance), each with its own cond, depth, orig, plan, schedule and guard table; unconds: [K,77,D], this
        timestep's unconditional embedding of every item.  The passes of guided_step_batch: optimisation at B = K, CFG at
        B = 2K over [K unconds | K conds]."""
        K = x.shape[0]
        key = tuple(id(st) for st in sts)
        c = sts[0].__dict__.get("_items_cond")
        if c is None or c[0] != key:
            GuidedStableDiffuser._text_keys += 1          # the stacked prompts are a text of their own for the K|V cache
            c = sts[0]._items_cond = (key, torch.cat([st.cond for st in sts]).contiguous(), GuidedStableDiffuser._text_keys)
        unc = unconds.reshape(K, *c[1].shape[1:]).to(self.device, torch.float32)
        return self._guided_step_rows(sts, x, t_idx, t, c[1], c[2], unc)

    def _energy_grads(self, sts, k, acts_k, t_idx, iteration, ws, out):
        """Layer k's energy gradient of every item: acts_k / out [K,h,w,C].  Items whose plan is on this layer's grid go through
        the batched planned entry together, the others (resized layers, non-default configurations) one by one."""
        auto = sts[0].auto
        fw = [ws[e][0][k] if st.n_pairs > 0 else 0.0 for e, st in enumerate(sts)]
        bw = [ws[e][1][k] for e in range(len(sts))]
        S = [float(st.scale_host[t_idx, iteration]) if auto else self.grad_scale for st in sts]
        g = acts_k.shape[1]
        planned = [e for e, st in enumerate(sts) if st.plan is not None and g == st.plan.grid and acts_k.shape[2] == g]
        if not (self._batch_energy and 2 <= len(planned) <= MAX_BATCH_ITEMS):
            planned = []
        if planned and any(sts[e].donor_bits for e in planned):
            # donor edits: the donor batch takes weighted plans only; with an unweighted one among them, one by one
            if all(sts[e].plan.weighted for e in planned):
                _losses.energy_and_grad_planned_donor_batch(
                    [acts_k[e] for e in planned], [sts[e].orig[k][t_idx] for e in planned], [sts[e].plan for e in planned],
                    [fw[e] for e in planned], [bw[e] for e in planned], [S[e] for e in planned],
                    [sts[e].donor[k][t_idx] if sts[e].donor_bits else None for e in planned],
                    [sts[e].donor_bits for e in planned], outs=[out[e] for e in planned])
            else:
                planned = []
        elif planned:
            # weighted and unweighted plans together: the mixed entry, still one launch pair; a set of one kind keeps its entry
            mixed = len({sts[e].plan.weighted for e in planned}) > 1
            entry = _losses.energy_and_grad_planned_mixed if mixed else energy_and_grad_planned_batch
            entry([acts_k[e] for e in planned], [sts[e].orig[k][t_idx] for e in planned],
                  [sts[e].plan for e in planned], [fw[e] for e in planned], [bw[e] for e in planned],
                  [S[e] for e in planned], outs=[out[e] for e in planned])
        for e, st in enumerate(sts):
            if e not in planned:
                self._energy_grad(st, k, acts_k[e], t_idx, fw[e], bw[e], out=out[e], scale=S[e])

    def _guided_step_rows(self, sts, x, t_idx, t, cond, cond_key, unc):
        """The batched step on K text rows: cond / unc [K,77,D] (one image: K copies of one row)."""
        L = _lib.lib()
        K = x.shape[0]
        depth = torch.cat([st.depth_nhwc for st in sts], dim=0) if self.conf.use_depth else None
        auto = sts[0].auto
        if auto:
            table, status = self._batch_guard(sts)
        iteration = 0
        while iteration < self.conf.num_optsteps and t_idx < self.conf.guidance_max_step:
            ws = [st.schedule(t_idx, iteration) for st in sts]          # (edits may carry their own weights)
            active = [k for k in range(3) if any(fgw[k] != 0.0 or bgw[k] != 0.0 for fgw, bgw in ws)]
            if active:
                # the same in-place engine I/O as guided_step: one pack launch for the K inputs, every edit's energy gradient
                # written straight into its slice of the engine's cotangent buffer, d(sample) read in place
                sample = self.unet.stage_sample(x, depth, K)
                _, acts = self.unet.forward(sample, float(t), cond, save_for_backward=True, want_acts=active, want_eps=False,
                                            text_key=cond_key, inplace=True)
                d_acts = [None, None, None]
                for k in active:
                    d_acts[k] = self.unet.io_view("act_grad", k)[:K]
                    self._energy_grads(sts, k, acts[k], t_idx, iteration, ws, d_acts[k])
                d_sample, _ = self.unet.backward(d_acts, None, want_sample_grad=True, want_text_grad=False, inplace=True)
                x_new = self._latent_buffer(sts[0], x, iteration)
                if auto:
                    self._latent_update_guarded(x_new, x, d_sample, table, status, t_idx, iteration)
                else:
                    _lib.check(L.dh_latent_update_strided(_lib.ptr(x_new), _lib.ptr(x), _lib.ptr(d_sample), d_sample.shape[-1],
                                                          x.shape[-1], 0.1, self.grad_scale, x.numel() // x.shape[-1],
                                                          _lib.stream_ptr()), "dh_latent_update_strided")
                x = x_new
            iteration += 1
        sample2 = self.unet.stage_sample(x, depth, 2 * K)          # the K edits twice: unconditional and conditional halves
        text2 = torch.cat([unc, cond], dim=0).contiguous()
        eps, _ = self.unet.forward(sample2, float(t), text2, save_for_backward=False, want_acts=False, inplace=True)
        if any(st.lock is not None for st in sts):
            return self._ddim_step_locked(sts, x, eps[:K], eps[K:], t, status if auto else None, t_idx, iteration)
        if auto:
            return self._ddim_step_flagged(x, eps[:K], eps[K:], t, status, t_idx, iteration)
        return self.ddim_step(x, eps[:K], eps[K:], t)

    @staticmethod
    def _batch_guard(sts):
        """('auto') the [K, T, I] device scale table of a batch of guidance states and its [K, 4] status words, made at the
        batch's first step and kept on the first state."""
        key = tuple(id(st) for st in sts)
        g = sts[0].__dict__.get("_batch_guard")
        if g is None or g[0] != key:
            table = torch.cat([st.scale_dev for st in sts]).contiguous()
            status = torch.zeros((len(sts), 4), dtype=torch.int32, device=table.device)
            g = sts[0]._batch_guard = (key, table, status)
        return g[1], g[2]

    @staticmethod
    def _status_of(sts):
        """device [K, 4] status of a guidance state (list of one) or batch, None in 'static' mode"""
        if not sts[0].auto:
            return None
        if len(sts) == 1 and "_batch_guard" not in sts[0].__dict__:
            return sts[0].status
        return sts[0]._batch_guard[2]

    def _batch_edit_steps(self, latents, depths, uncond_embeddings, prompt, activations_orig, correspondences_list,
                          fg_weight=None, bg_weight=None, cond=None, orig=None, status_out=None, object_labels=None,
                          object_weights=None, pair_instances=None, row_kind=None, donor=None, vacated=None, lock=None):
        """The batched edit as a generator: yields after the preparation and after every denoising step (everything is only
        ENQUEUED on the current stream by then), returns the final latents [K,4,H,W] through StopIteration.  One body for the
        one-stream call below and for the lanes of guided_inference_batch_lanes.  fg_weight / bg_weight: one value, or one per
        edit.  status_out: a list that receives the device [K, 4] status ('auto') at the end.  object_labels / object_weights: one
        label image and one weight list for all K edits (prepare_guidance).  lock: one (keep, trajectory) for all K edits or a list
        of K (prepare_guidance; None entries are unlocked edits).  pair_instances: None or a list of K, the instances of every
        edit's correspondence rows (prepare_guidance).  vacated: None, one image for all K edits or a list of K (None entries: edits that
        delete nothing).  donor: None or (activations_donor, list of K row_donor) -- one donor image for all K edits, whose
        channels-last copy they share (prepare_guidance).  row_kind: None or a list of K (None entries: edits without a camera),
        the kinds of every edit's correspondence rows (prepare_guidance)."""
        K = len(depths)
        if row_kind is not None and len(row_kind) != K:
            raise ValueError(f"guided_inference_batch: row_kind has {len(row_kind)} entries for {K} edits")
        if donor is not None and (not isinstance(donor, (tuple, list)) or len(donor) != 2 or not isinstance(donor[1], (list, tuple))
                                  or len(donor[1]) != K):
            raise ValueError(f"guided_inference_batch: donor must be (activations_donor, a list of {K} row_donor arrays)")
        if pair_instances is not None and len(pair_instances) != K:
            raise ValueError(f"guided_inference_batch: pair_instances has {len(pair_instances)} entries for {K} edits")
        per = lambda w, i: w[i] if isinstance(w, (list, tuple)) else w
        if isinstance(vacated, (list, tuple)) and len(vacated) != K:
            raise ValueError(f"guided_inference_batch: vacated has {len(vacated)} entries for {K} edits")
        if self.unet.max_batch < 2 * K:
            raise RuntimeError(f"engine max_batch {self.unet.max_batch} < 2*K = {2 * K}")
        locks = self._locks(lock, K, "guided_inference_batch")
        torch.manual_seed(self.conf.seed)
        self.scheduler.set_timesteps(self.conf.num_timesteps, device=self.device)
        timesteps, _ = self.get_timesteps(self.conf.num_timesteps, 1.0)
        sts = []
        for i, (d, c) in enumerate(zip(depths, correspondences_list)):
            sts.append(self.prepare_guidance(d, prompt, activations_orig, c, per(fg_weight, i), per(bg_weight, i),
                                             orig=sts[0].orig if sts else orig, cond=sts[0].cond if sts else cond,
                                             object_labels=object_labels, object_weights=object_weights, lock=locks[i],
                                             pair_instances=None if pair_instances is None else pair_instances[i],
                                             row_kind=None if row_kind is None else row_kind[i],
                                             donor=None if donor is None else (sts[0].donor if sts else donor[0], donor[1][i]),
                                             vacated=per(vacated, i)))
        x = _nhwc(latents.to(self.device, torch.float32)).expand(K, -1, -1, -1).contiguous()
        yield None
        for t_idx, t in enumerate(timesteps):
            x = self.guided_step_batch(sts, x, t_idx, t, uncond_embeddings[t_idx])
            yield None
        if status_out is not None and sts[0].auto:
            status_out.append(self._status_of(sts))
        return x.permute(0, 3, 1, 2)

    def guided_inference_batch(self, latents, depths, uncond_embeddings, prompt, activations_orig, correspondences_list,
                               fg_weight=None, bg_weight=None, object_labels=None, object_weights=None,
                               pair_instances=None, row_kind=None, donor=None, vacated=None, lock=None):
        """K edits of one image at once.  depths: list of K edited disparities [1,1,H,W]; correspondences_list:
        K [N_k,4] tensors; fg_weight / bg_weight: one value or K.  Needs an engine built with max_batch >= 2K.  Returns images
        [K,3,H,W]; 'auto' grad_scale: FloatingPointError when an edit met a non-finite value.  object_labels / object_weights: one
        label image and one weight list for all K edits (prepare_guidance).  lock: the background lock, one (keep, trajectory)
        for all K edits or a list of K (prepare_guidance).  pair_instances: None or a list of K, the instances of every edit's
        correspondence rows, in place of the label image (prepare_guidance).  vacated: None, one vacated image for all K edits
        or a list of K with None for the edits that delete nothing (prepare_guidance; DESIGN.md "Object removal").  donor: None or
        (activations_donor, list of K row_donor), one donor image for all K edits (prepare_guidance; DESIGN.md "Object
        insertion").  row_kind: None or a list of K, the kinds of every edit's correspondence rows (prepare_guidance; DESIGN.md
        "Camera moves")."""
        status = []
        with torch.no_grad(), self.on_stream():
            gen = self._batch_edit_steps(latents, depths, uncond_embeddings, prompt, activations_orig, correspondences_list,
                                         fg_weight, bg_weight, status_out=status, object_labels=object_labels,
                                         object_weights=object_weights, lock=lock, pair_instances=pair_instances,
                                         row_kind=row_kind, donor=donor, vacated=vacated)
            try:
                while True:
                    next(gen)
            except StopIteration as done:
                self.last_latents = done.value
            image = self.decode_latent_image(self.last_latents)
        if status:
            self.raise_on_status(list(enumerate(status[0].cpu().tolist())))
        return image

    ITEM_FIELDS = ("latents", "depth", "uncond_embeddings", "prompt", "activations_orig", "correspondences")

    def guided_inference_items(self, items, fg_weight=None, bg_weight=None):
        """K edits of DIFFERENT images at once.  items: K records (dicts with the keys ITEM_FIELDS, or tuples in that order), the
        arguments of guided_inference per item, plus optional object_labels (or pair_instances: an edit with copies) /
        object_weights (prepare_guidance: a multi-object edit with a weight per object) and an optional lock ((keep,
        trajectory), prepare_guidance: locked and unlocked items may share a batch) and an optional vacated (the image of the pixels the
        item's removed objects leave behind, prepare_guidance: items with and without it share a batch) and an optional row_kind (the kinds of
        the item's correspondence rows, prepare_guidance: an edit that moves the camera); fg_weight / bg_weight: one value or K.  Items with the same activations_orig
        tensors share one channels-last copy of them, items with the same prompt one encoding.  One resolution (the
        engine's); needs max_batch >= 2K and max_diff_batch >= K, raises otherwise (never splits).  Returns images [K,3,H,W]
        in item order and sets last_latents; 'auto' grad_scale: FloatingPointError naming the items that met a non-finite
        value."""
        items = [it if isinstance(it, dict) else dict(zip(self.ITEM_FIELDS, it)) for it in items]
        K = len(items)
        if K < 1 or any(set(self.ITEM_FIELDS) - set(it) for it in items):
            raise ValueError(f"guided_inference_items: needs at least one item, each with {self.ITEM_FIELDS}")
        if self.unet.max_batch < 2 * K or self.unet.max_diff_batch < K:
            raise RuntimeError(f"engine max_batch {self.unet.max_batch} / max_diff_batch {self.unet.max_diff_batch} too small for "
                               f"{K} items: build the diffuser with max_batch >= {2 * K}")
        s = self.unet.sample_size
        for i, it in enumerate(items):
            if tuple(it["latents"].shape[-2:]) != (s, s):
                raise ValueError(f"guided_inference_items: latents of item {i} are {tuple(it['latents'].shape[-2:])}, the engine "
                                 f"runs {(s, s)} latents")
            if tuple(it["depth"].shape[-2:]) != tuple(items[0]["depth"].shape[-2:]):
                raise ValueError(f"guided_inference_items: item {i} has another resolution than item 0 "
                                 f"({tuple(it['depth'].shape[-2:])} / {tuple(items[0]['depth'].shape[-2:])})")
        per = lambda w, i: w[i] if isinstance(w, (list, tuple)) else w
        with torch.no_grad(), self.on_stream():
            torch.manual_seed(self.conf.seed)
            self.scheduler.set_timesteps(self.conf.num_timesteps, device=self.device)
            timesteps, _ = self.get_timesteps(self.conf.num_timesteps, 1.0)
            sts, origs, conds = [], {}, {}
            locks = self._locks([it.get("lock") for it in items], K, "guided_inference_items")
            for i, it in enumerate(items):
                okey = tuple(id(a) for a in it["activations_orig"])
                st = self.prepare_guidance(it["depth"], it["prompt"], it["activations_orig"], it["correspondences"],
                                           per(fg_weight, i), per(bg_weight, i), orig=origs.get(okey), cond=conds.get(it["prompt"]),
                                           object_labels=it.get("object_labels"), object_weights=it.get("object_weights"),
                                           lock=locks[i], pair_instances=it.get("pair_instances"), vacated=it.get("vacated"),
                                           row_kind=it.get("row_kind"))
                origs[okey], conds[it["prompt"]] = st.orig, st.cond
                sts.append(st)
            x = torch.cat([_nhwc(it["latents"].to(self.device, torch.float32)) for it in items]).contiguous()
            D = sts[0].cond.shape[1:]
            uncs = torch.stack([it["uncond_embeddings"].to(self.device, torch.float32).reshape(len(timesteps), *D)
                                for it in items], dim=1).contiguous()          # [T, K, 77, D]
            for t_idx, t in enumerate(timesteps):
                x = self.guided_step_items(sts, x, t_idx, t, uncs[t_idx])
            self.last_latents = x.permute(0, 3, 1, 2)
            image = self.decode_latent_image(self.last_latents)
        if sts[0].auto:
            self.raise_on_status(list(enumerate(self._status_of(sts).cpu().tolist())))
        return image

    # ---- lanes: concurrent edit streams on ONE copy of the weights --------------------------------------------------------
    def fork(self, max_batch=None):
        """A lane of this diffuser: the same configuration, VAE, text tower and U-Net WEIGHTS (HipUNet.share: resident once),
        with its own engine arenas, hipGraphs, stream and scheduler, so that a second edit can run next to the first one in the
        same process.  A single edit's passes are thousands of dependent launches of at most a few hundred workgroups: two
        independent edits interleave on the chip (two processes on one GPU measured 1.4x the steps/s of one,
        profiles/r03_bench_gloo2_one_gpu.json); lanes give that without a second copy of the weights."""
        import copy
        if self.unet is None:
            raise RuntimeError("fork() needs the diffuser on its device first (.to(device))")
        lane = copy.copy(self)
        lane.unet = self.unet.share(max_batch)
        lane._stream = torch.cuda.Stream(device=self.device)
        lane.scheduler = DDIMScheduler()
        lane._root = getattr(self, "_root", self)
        return lane

    def lanes(self, n, max_batch=None):
        """[self, fork, ...]: n lanes on this diffuser's weights.  ONE growing list of forks per max_batch: lanes(2) is a prefix
        of lanes(3), so a process that serves 8, 16 and 24 edits at streams = 3 holds two forks, not three sets (a fork owns a
        full engine arena: 28.4 GB at max_batch 16 in round 4, about half of it since the forward-only layout of round 5).  release_lanes() destroys them."""
        n = int(n)
        if n < 1:
            raise ValueError(f"lanes(n): n must be >= 1, got {n}")
        forks = self.__dict__.setdefault("_lane_forks", {}).setdefault(max_batch, [])
        while len(forks) < n - 1:
            forks.append(self.fork(max_batch))
        return [self] + forks[:n - 1]

    def lane_arena_bytes(self):
        """HBM held by the forks of this diffuser (all max_batch keys), for services that budget it."""
        return sum(f.unet.workspace_bytes() for forks in self.__dict__.get("_lane_forks", {}).values() for f in forks)

    def release_lanes(self):
        """Destroy every fork's engine (arenas, graphs) and forget them; the root diffuser and the shared weights stay."""
        for forks in self.__dict__.pop("_lane_forks", {}).values():
            for f in forks:
                f.unet.close()

    def _decode_serialized(self, latents):
        """VAE decode of a lane's result on the ROOT diffuser's decode stream: the decoder engine has one activation arena, so
        the lanes' decodes run one after the other (in host issue order) while the other lane keeps denoising."""
        root = getattr(self, "_root", self)
        if not hasattr(root, "_decode_stream"):
            root._decode_stream = torch.cuda.Stream(device=root.device)
        cur = torch.cuda.current_stream(self.device)
        root._decode_stream.wait_stream(cur)
        with torch.cuda.stream(root._decode_stream):
            img = root.decode_latent_image(latents)
        latents.record_stream(root._decode_stream)
        cur.wait_stream(root._decode_stream)
        return img

    @staticmethod
    def run_lanes(lanes, jobs):
        """Drive generator jobs on lanes from ONE host thread.  jobs: callables lane -> generator (a *_edit_steps body); job i
        runs on lanes[i % len(lanes)], a lane's jobs one after the other.  The host only enqueues: it advances every lane by one
        yield in turn, so the lanes' streams always hold work and the GPU interleaves them; nothing synchronises the lanes with
        each other.  Returns the generators' return values in job order (tensors produced on the lanes' streams; the caller's
        current stream is made to wait for every lane before this returns)."""
        import contextlib
        on_device = all(getattr(ln, "_stream", None) is not None for ln in lanes)      # (False: the scheduling alone, CPU tests)
        outer = torch.cuda.current_stream(lanes[0].device) if on_device else None
        for ln in lanes:
            if on_device:
                ln._stream.wait_stream(outer)
        queues = [[(i, job) for i, job in enumerate(jobs) if i % len(lanes) == li] for li in range(len(lanes))]
        running = [None] * len(lanes)
        results = [None] * len(jobs)
        with torch.no_grad():
            while any(q for q in queues) or any(r is not None for r in running):
                for li, ln in enumerate(lanes):
                    with (torch.cuda.stream(ln._stream) if on_device else contextlib.nullcontext()):
                        if running[li] is None and queues[li]:
                            i, job = queues[li].pop(0)
                            running[li] = (i, job(ln))
                        if running[li] is None:
                            continue
                        i, gen = running[li]
                        try:
                            next(gen)
                        except StopIteration as done:
                            results[i] = done.value
                            running[li] = None
        for ln in lanes:
            if on_device:
                outer.wait_stream(ln._stream)
        return results

    def guided_inference_batch_lanes(self, latents, chunks, uncond_embeddings, prompt, activations_orig, streams=2,
                                     fg_weight=None, bg_weight=None, object_labels=None, object_weights=None,
                                     pair_instances=None, donor=None, vacated=None, lock=None):
        """Batched edits of one image on `streams` concurrent lanes.  chunks: list of (depths, correspondences_list), each the
        argument pair of one guided_inference_batch call; chunk i runs on lane i % streams.  Every lane executes exactly the
        passes the one-stream call executes for its chunk (same batch, same kernels, private arenas), so the images are
        bit-identical to guided_inference_batch chunk by chunk.  Returns one image tensor [K_i,3,H,W] per chunk.
        object_labels / object_weights: one label image and one weight list for every edit (prepare_guidance).  lock: one
        (keep, trajectory) for every edit, or a list with one entry per edit over the chunks in order.  pair_instances: None or
        one list per chunk (guided_inference_batch).  vacated: None, one image for every edit, or one entry per chunk (each None, an
        image or a list, as guided_inference_batch takes it).  donor: None or (activations_donor, one list of row_donor per
        chunk); the lanes share the channels-last copy of the donor's activations."""
        if donor is not None and (len(donor) != 2 or len(donor[1]) != len(chunks)):
            raise ValueError(f"guided_inference_batch_lanes: donor must be (activations_donor, one row_donor list per chunk)")
        if pair_instances is not None and len(pair_instances) != len(chunks):
            raise ValueError(f"guided_inference_batch_lanes: pair_instances has {len(pair_instances)} entries for {len(chunks)} chunks")
        if isinstance(vacated, (list, tuple)) and len(vacated) != len(chunks):
            raise ValueError(f"guided_inference_batch_lanes: vacated has {len(vacated)} entries for {len(chunks)} chunks")
        kmax = max(len(d) for d, _ in chunks)
        if self.unet.max_batch < 2 * kmax:
            # lane 0 is THIS diffuser: it could not run its chunk, and forks sized 2 * kmax would be made for nothing
            raise RuntimeError(f"engine max_batch {self.unet.max_batch} < 2*K = {2 * kmax}: build the diffuser with max_batch >= {2 * kmax}")
        lanes = self.lanes(min(int(streams), len(chunks)))
        statuses = [[] for _ in chunks]
        with torch.no_grad(), self.on_stream():
            cond = self._encode([prompt]).contiguous()
            orig = [a.to(self.device).permute(0, 2, 3, 1).to(self.dtype).contiguous() for a in activations_orig]
            # (prepared here, on this stream, which every lane waits for: the lanes share the copies)
            offs = np.cumsum([0] + [len(d) for d, _ in chunks])
            locks = self._locks(lock, int(offs[-1]), "guided_inference_batch_lanes")
            dacts = None if donor is None else DonorActivations(
                a.to(self.device).permute(0, 2, 3, 1).to(self.dtype).contiguous() for a in donor[0])

            def make(depths, corrs, status, lk, inst, vac, dn):
                def job(lane):
                    def body():
                        lat = yield from lane._batch_edit_steps(latents, depths, uncond_embeddings, prompt, activations_orig,
                                                                corrs, fg_weight, bg_weight, cond=cond, orig=orig,
                                                                status_out=status, object_labels=object_labels,
                                                                object_weights=object_weights, lock=lk, pair_instances=inst,
                                                                donor=dn, vacated=vac)
                        return lane._decode_serialized(lat)
                    return body()
                return job
            vac_of = lambda i: vacated[i] if isinstance(vacated, (list, tuple)) else vacated
            images = GuidedStableDiffuser.run_lanes(lanes, [make(d, c, s, locks[int(offs[i]):int(offs[i + 1])],
                                                                 None if pair_instances is None else pair_instances[i], vac_of(i),
                                                                 None if donor is None else (dacts, donor[1][i]))
                                                            for i, ((d, c), s) in enumerate(zip(chunks, statuses))])
            if any(statuses):      # edits numbered over the chunks in order; read after every lane has finished
                self.raise_on_status([(int(offs[i]) + b, row) for i, s in enumerate(statuses)
                                      for b, row in enumerate(s[0].cpu().tolist())])
        return images

    def _edit_steps(self, latents, depth, uncond_embeddings, prompt, activations_orig, correspondences, fg_weight=None,
                    bg_weight=None, cond=None, orig=None, status_out=None, object_labels=None, object_weights=None,
                    pair_instances=None, donor=None, vacated=None, lock=None):
        """One edit as a generator (see _batch_edit_steps): yields after the preparation and after every denoising step,
        returns the final latents [1,4,H,W].  lock: the edit's background lock (prepare_guidance)."""
        torch.manual_seed(self.conf.seed)
        self.scheduler.set_timesteps(self.conf.num_timesteps, device=self.device)
        timesteps, _ = self.get_timesteps(self.conf.num_timesteps, 1.0)
        st = self.prepare_guidance(depth, prompt, activations_orig, correspondences, fg_weight, bg_weight, orig=orig, cond=cond,
                                   object_labels=object_labels, object_weights=object_weights, lock=lock,
                                   pair_instances=pair_instances, donor=donor, vacated=vacated)
        x = _nhwc(latents.to(self.device, torch.float32))
        yield None
        for t_idx, t in enumerate(timesteps):
            x = self.guided_step(st, x, t_idx, t, uncond_embeddings[t_idx])
            yield None
        if status_out is not None and st.auto:
            status_out.append(st.status)
        return x.permute(0, 3, 1, 2)

    def guided_inference_lanes(self, latents, edits, uncond_embeddings, prompt, activations_orig, streams=2, fg_weight=None,
                               bg_weight=None, object_labels=None, object_weights=None, pair_instances=None, donor=None,
                               vacated=None, lock=None):
        """Single (B = 1) edits of one image on `streams` concurrent lanes.  edits: list of (depth, correspondences), the
        argument pair of guided_inference; edit i runs on lane i % streams with exactly the passes guided_inference runs, so
        the images are bit-identical to the one-stream calls.  Returns a list of images [1,3,H,W].  object_labels /
        object_weights: one label image and one weight list for every edit (prepare_guidance).  lock: one (keep, trajectory)
        for every edit, or a list with one entry per edit.  pair_instances: None or a list with one entry per edit
        (prepare_guidance).  vacated: None, one image for every edit, or a list with one entry per edit (prepare_guidance).
        donor: None or (activations_donor, a list with one row_donor per edit); the lanes share the donor's channels-last copy."""
        if donor is not None and (len(donor) != 2 or len(donor[1]) != len(edits)):
            raise ValueError(f"guided_inference_lanes: donor must be (activations_donor, one row_donor per edit)")
        if pair_instances is not None and len(pair_instances) != len(edits):
            raise ValueError(f"guided_inference_lanes: pair_instances has {len(pair_instances)} entries for {len(edits)} edits")
        if isinstance(vacated, (list, tuple)) and len(vacated) != len(edits):
            raise ValueError(f"guided_inference_lanes: vacated has {len(vacated)} entries for {len(edits)} edits")
        lanes = self.lanes(min(int(streams), len(edits)))
        statuses = [[] for _ in edits]
        with torch.no_grad(), self.on_stream():
            cond = self._encode([prompt]).contiguous()
            orig = [a.to(self.device).permute(0, 2, 3, 1).to(self.dtype).contiguous() for a in activations_orig]
            locks = self._locks(lock, len(edits), "guided_inference_lanes")      # (on this stream, which every lane waits for)
            dacts = None if donor is None else DonorActivations(
                a.to(self.device).permute(0, 2, 3, 1).to(self.dtype).contiguous() for a in donor[0])

            def make(depth, corr, status, lk, inst, vac, dn):
                def job(lane):
                    def body():
                        lat = yield from lane._edit_steps(latents, depth, uncond_embeddings, prompt, activations_orig, corr,
                                                          fg_weight, bg_weight, cond=cond, orig=orig, status_out=status,
                                                          object_labels=object_labels, object_weights=object_weights, lock=lk,
                                                          pair_instances=inst, donor=dn, vacated=vac)
                        return lane._decode_serialized(lat)
                    return body()
                return job
            insts = [None] * len(edits) if pair_instances is None else pair_instances
            vacs = list(vacated) if isinstance(vacated, (list, tuple)) else [vacated] * len(edits)
            dns = [None] * len(edits) if donor is None else [(dacts, r) for r in donor[1]]
            images = GuidedStableDiffuser.run_lanes(lanes, [make(d, c, s, lk, n, v, dn)
                                                            for (d, c), s, lk, n, v, dn in zip(edits, statuses, locks, insts, vacs, dns)])
            if any(statuses):      # read after every lane has finished
                self.raise_on_status([(i, s[0][0].cpu().tolist()) for i, s in enumerate(statuses)])
        return images

    def guided_inference(self, latents, depth, uncond_embeddings, prompt, activations_orig, correspondences,
                         fg_weight=None, bg_weight=None, save_denoising_steps=False, record=None, object_labels=None,
                         object_weights=None, pair_instances=None, row_kind=None, donor=None, vacated=None, lock=None):
        """object_labels (or pair_instances, the instance of every correspondence row of an edit with copies) / object_weights:
        a weight per object for the foreground term (prepare_guidance).  lock: (keep,
        trajectory), the background lock -- after every DDIM step the latents are blended with the reconstruction's outside
        the edit's region (prepare_guidance; DESIGN.md "Background lock").  vacated: the image of the pixels the edit's removed
        objects leave behind (prepare_guidance; DESIGN.md "Object removal").  donor: (activations_donor, row_donor) of an edit
        that brings in objects of another image (prepare_guidance; DESIGN.md "Object insertion").  row_kind: the kinds of the
        correspondence rows of an edit that moves the camera (prepare_guidance; DESIGN.md "Camera moves")."""
        with torch.no_grad(), self.on_stream():
            torch.manual_seed(self.conf.seed)
            self.scheduler.set_timesteps(self.conf.num_timesteps, device=self.device)
            timesteps, _ = self.get_timesteps(self.conf.num_timesteps, 1.0)
            st = self.prepare_guidance(depth, prompt, activations_orig, correspondences, fg_weight, bg_weight,
                                       object_labels=object_labels, object_weights=object_weights, lock=lock,
                                       pair_instances=pair_instances, row_kind=row_kind, donor=donor, vacated=vacated)
            denoising_steps = {"opt": [], "post-opt": []} if save_denoising_steps else None
            x = _nhwc(latents.to(self.device, torch.float32))
            for t_idx, t in enumerate(timesteps):
                if save_denoising_steps:      # one list per timestep in 'opt': [after the optimisation, after the DDIM step];
                    denoising_steps["opt"].append([])         # 'post-opt' stays empty, as in the reference
                x = self.guided_step(st, x, t_idx, t, uncond_embeddings[t_idx], record,
                                     denoising_steps["opt"][-1] if save_denoising_steps else None)
                if record is not None:
                    record.setdefault("step", []).append(x.permute(0, 3, 1, 2).clone())
            self.last_latents = x.permute(0, 3, 1, 2)
            image = self.decode_latent_image(self.last_latents)
        if st.auto:      # the one read of the status, after the whole edit
            self.raise_on_status([(0, st.status[0].cpu().tolist())])
        return (image, denoising_steps) if save_denoising_steps else image
