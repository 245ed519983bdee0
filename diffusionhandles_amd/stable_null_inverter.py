"""Null-text inversion on the native engine (reference stable_null_inverter.py:12-181).

DDIM inversion (50 no-grad forwards) followed by the per-timestep Adam optimisation of the
unconditional embedding.  The gradient d mse / d uncond is obtained from ONE explicit
backward pass of the engine per inner step (eps -> text embedding, through the hoisted
K|V projection), seeded with the closed-form d mse / d eps_uncond.
"""
import torch

from . import _lib
from .null_inverter import NullInverter

VAE_SCALE = 0.18215


class StableNullInverter(NullInverter):
    def __init__(self, model, num_ddim_steps: int = 50, guidance_scale: float = 7.5):
        super().__init__(model=model)
        self.num_ddim_steps = num_ddim_steps
        self.guidance_scale = guidance_scale
        self.model.scheduler.set_timesteps(self.num_ddim_steps)
        # the eps cotangent is ~1e-6 and shrinks as the optimisation converges: every inner step scales it by the power of
        # two that brings its largest element to (8, 16] before the 16-bit backward pass and divides the text gradient
        # by the same factor (dh_mse_cotangent / dh_adam_step_scaled; the backward is linear, the factor cancels exactly).
        # Measured at the full SD-2-depth size (tools/probe_text_grad.py): fp16 text-gradient error 2.4e-3 for
        # max |cotangent| in [1, 4096], 1.9e-2 at 2^-4, 9e-2 at 2^-8 (fp16 subnormals); bf16 2.2e-2 at any amplitude.
        # 16 sits at the low end of that plateau: the accuracy of 256 with four more bits of fp16 overflow headroom for the
        # intermediate gradients (advisor, round 3); a gradient element that overflows anyway is skipped by the Adam kernel
        # (k_adam_scaled) instead of poisoning the embedding.
        self.cotangent_amp = 16.0

    def to(self, device):
        self.model.to(device)
        return self

    @property
    def scheduler(self):
        return self.model.scheduler

    def _step(self, x, eps_u, eps_c, scale, a_from, a_to):
        out = torch.empty_like(x)
        _lib.check(_lib.lib().dh_ddim_cfg_step(_lib.ptr(out), _lib.ptr(x), _lib.ptr(eps_u), _lib.ptr(eps_c), float(scale),
                                               a_from, a_to, x.numel(), _lib.stream_ptr()), "dh_ddim_cfg_step")
        return out

    def prev_step(self, model_output, timestep, sample):
        a_t, a_p = self.scheduler.step_alphas(timestep)
        return self._step(sample, None, model_output, 1.0, a_t, a_p)

    def next_step(self, model_output, timestep, sample):
        a_from, a_to = self.scheduler.inversion_alphas(timestep)
        return self._step(sample, None, model_output, 1.0, a_from, a_to)

    def get_noise_pred_single(self, latents, t, context, depth=None, save=False):
        sample = self.model._unet_input(latents, depth)
        eps, _ = self.model.unet.forward(sample, float(t), context.contiguous(), save_for_backward=save, want_acts=False)
        return eps

    @torch.no_grad()
    def get_noise_pred(self, latents, t, context, depth=None, is_forward=True):
        """One classifier-free-guidance DDIM move of `latents` (reference stable_null_inverter.py:55-70): a B = 2 engine pass
        over [uncond | cond] = `context`, eps = eps_u + w (eps_c - eps_u) with w = 1 on the way up (is_forward: next_step,
        the inversion direction) and w = guidance_scale on the way down (prev_step).  latents / depth are channels-last
        ([1,H,W,4] / [1,H,W,1]) like everywhere in this class; returns the moved latents [1,H,W,4]."""
        with self.model.on_stream():
            sample = self.model._unet_input(latents, depth, 2)
            text = context.to(self.model.device, torch.float32).contiguous()
            eps, _ = self.model.unet.forward(sample, float(t), text, save_for_backward=False, want_acts=False)
            eps_u, eps_c = eps[0:1].contiguous(), eps[1:2].contiguous()
            if is_forward:
                a_from, a_to = self.scheduler.inversion_alphas(t)
                return self._step(latents, eps_u, eps_c, 1.0, a_from, a_to)
            a_t, a_p = self.scheduler.step_alphas(t)
            return self._step(latents, eps_u, eps_c, self.guidance_scale, a_t, a_p)

    @torch.no_grad()
    def latent2image(self, latents_nchw):
        image = self.model.vae.decode(1 / VAE_SCALE * latents_nchw.detach())["sample"]
        return (image + 1) / 2

    @torch.no_grad()
    def image2latent(self, image):
        return self.model.vae.encode(image * 2 - 1)["latent_dist"].mean * VAE_SCALE

    @torch.no_grad()
    def ddim_loop(self, latent, context, depth):
        _, cond = context.chunk(2)
        all_latent = [latent]
        x = latent.clone()
        ts = self.scheduler.timesteps
        for i in range(self.num_ddim_steps):
            t = ts[len(ts) - i - 1]
            eps = self.get_noise_pred_single(x, t, cond, depth)
            x = self.next_step(eps, t, x)
            all_latent.append(x)
        return all_latent

    @torch.no_grad()
    def ddim_inversion(self, image, context, depth):
        latent = self.image2latent(image)
        image_rec = self.latent2image(latent)
        lat_nhwc = latent.permute(0, 2, 3, 1).contiguous()
        return image_rec, self.ddim_loop(lat_nhwc, context, depth)

    @torch.no_grad()
    def null_step(self, cur, uncond, cond, depth, i, target, num_inner_steps, epsilon, record=None):
        """The inner Adam loop of timestep index i (reference stable_null_inverter.py:141-158): up to num_inner_steps x
        {eps_u = unet(cur, uncond); loss = mse(prev_step(eps_u + w (eps_c - eps_u)), target); Adam step on uncond}, fresh
        optimiser state, lr = 1e-2 (1 - i/100), early stop at loss < epsilon + 2e-5 i.  Updates `uncond` in place and
        returns the number of inner steps taken.  d loss / d uncond comes from ONE explicit engine backward per inner
        step (eps -> text embedding), seeded with the closed-form d loss / d eps_u."""
        L = _lib.lib()
        n = cur.numel()
        loss_dev = torch.zeros(1, dtype=torch.float32, device=cur.device)
        scale_dev = torch.ones(1, dtype=torch.float32, device=cur.device)
        d_eps = torch.empty_like(cur)
        m = torch.zeros_like(uncond)
        v = torch.zeros_like(uncond)
        lr = 1e-2 * (1.0 - i / 100.0)
        t = self.scheduler.timesteps[i]
        a_t, a_p = self.scheduler.step_alphas(t)
        # d rec / d eps_u = (1 - w) * (sqrt(1-a_p) - sqrt(a_p) sqrt(1-a_t) / sqrt(a_t))
        k = (1.0 - self.guidance_scale) * ((1 - a_p) ** 0.5 - (a_p ** 0.5) * ((1 - a_t) ** 0.5) / (a_t ** 0.5))
        eps_c = self.get_noise_pred_single(cur, t, cond, depth)
        self._eps_c = eps_c                                     # the post-loop CFG step of this timestep reuses it
        taken = 0
        for j in range(num_inner_steps):
            eps_u = self.get_noise_pred_single(cur, t, uncond, depth, save=True)
            rec = self._step(cur, eps_u, eps_c, self.guidance_scale, a_t, a_p)
            _lib.check(L.dh_mse_cotangent(_lib.ptr(rec), _lib.ptr(target), n, k, self.cotangent_amp, _lib.ptr(loss_dev),
                                          _lib.ptr(d_eps), _lib.ptr(scale_dev), _lib.stream_ptr()), "dh_mse_cotangent")
            _, d_text = self.model.unet.backward(None, d_eps, want_sample_grad=False, want_text_grad=True)
            _lib.check(L.dh_adam_step_scaled(_lib.ptr(uncond), _lib.ptr(d_text), _lib.ptr(scale_dev), _lib.ptr(m), _lib.ptr(v),
                                             lr, 0.9, 0.999, 1e-8, j + 1, uncond.numel(), _lib.stream_ptr()),
                       "dh_adam_step_scaled")
            taken = j + 1
            # the reference's early stop: one host read per inner step.  It stalls the queue for ~50 us out of the ~9 ms of
            # an inner step; skipping the remaining passes when it fires is worth far more than the stall costs.
            loss = loss_dev.item()
            if record is not None:
                record.setdefault("loss", []).append(loss)
                record.setdefault("grad", []).append(d_text / scale_dev)
                record.setdefault("scale", []).append(float(scale_dev.item()))
                record.setdefault("d_eps", []).append(d_eps / scale_dev)
            if loss < epsilon + i * 2e-5:
                break
        return taken

    @torch.no_grad()
    def null_optimization(self, latents, context, depth, num_inner_steps, epsilon, max_timesteps=None):
        uncond, cond = context.chunk(2)
        uncond = uncond.clone().contiguous()
        cond = cond.contiguous()
        out = []
        cur = latents[-1]
        steps = self.num_ddim_steps if max_timesteps is None else max_timesteps
        self.inner_steps_taken = []
        for i in range(steps):
            target = latents[len(latents) - i - 2]
            t = self.scheduler.timesteps[i]
            a_t, a_p = self.scheduler.step_alphas(t)
            self.inner_steps_taken.append(self.null_step(cur, uncond, cond, depth, i, target, num_inner_steps, epsilon))
            out.append(uncond[:1].clone())
            # the CFG step with the optimised embedding (reference :162-165 runs a B=2 pass): its conditional half has the
            # inputs of the eps_c this timestep already computed (same latent, timestep, prompt), so only the
            # unconditional half is run, as a B=1 pass
            eu = self.get_noise_pred_single(cur, t, uncond, depth)
            cur = self._step(cur, eu, self._eps_c, self.guidance_scale, a_t, a_p)
        return torch.stack(out, dim=0)

    def invert(self, target_img, depth, prompt, num_inner_steps=10, early_stop_epsilon=1e-5, verbose=False,
               max_timesteps=None):
        with self.model.on_stream():
            return self._invert(target_img, depth, prompt, num_inner_steps, early_stop_epsilon, verbose, max_timesteps)

    def _invert(self, target_img, depth, prompt, num_inner_steps, early_stop_epsilon, verbose, max_timesteps):
        dev = self.model.device
        depth64 = self.model.init_depth(depth.to(dev, torch.float32))
        depth_nhwc = depth64.permute(0, 2, 3, 1).contiguous() if self.model.conf.use_depth else None
        context = self.model.init_prompt(prompt)
        if verbose:
            print("DDIM inversion...")
        recon_img, ddim_latents = self.ddim_inversion(target_img.to(dev, torch.float32), context, depth_nhwc)
        if verbose:
            print("Null-text optimization...")
        uncond = self.null_optimization(ddim_latents, context, depth_nhwc, num_inner_steps, early_stop_epsilon,
                                        max_timesteps)
        self.last_ddim_latents = ddim_latents
        return (target_img, recon_img), ddim_latents[-1].permute(0, 3, 1, 2), uncond

    # ---- K images of the same resolution inverted together (not in the reference: a batch-1 script) ---------------------
    @torch.no_grad()
    def null_step_batch(self, cur, uncond, cond, depth, i, target, num_inner_steps, epsilon, record=None):
        """null_step for K images at once: cur / target [K,H,W,4], uncond / cond [K,77,D] (uncond updated in place), depth
        [K,H,W,1] or None.  Every image keeps its own Adam state, cotangent scale and early stop (dh_mse_cotangent_batch /
        dh_adam_step_scaled_batch): an image that stopped rides along in the B = K passes with its embedding frozen.  One
        host read of the K active flags per inner step; the loop ends when no image is active.  Returns the inner steps
        taken per image."""
        L = _lib.lib()
        K = cur.shape[0]
        n = cur[0].numel()
        loss_dev = torch.zeros(K, dtype=torch.float32, device=cur.device)
        scale_dev = torch.ones(K, dtype=torch.float32, device=cur.device)
        active = torch.ones(K, dtype=torch.int32, device=cur.device)
        updated = torch.zeros(K, dtype=torch.int32, device=cur.device)
        d_eps = torch.empty_like(cur)
        m = torch.zeros_like(uncond)
        v = torch.zeros_like(uncond)
        lr = 1e-2 * (1.0 - i / 100.0)
        t = self.scheduler.timesteps[i]
        a_t, a_p = self.scheduler.step_alphas(t)
        k = (1.0 - self.guidance_scale) * ((1 - a_p) ** 0.5 - (a_p ** 0.5) * ((1 - a_t) ** 0.5) / (a_t ** 0.5))
        threshold = epsilon + i * 2e-5
        eps_c = self.get_noise_pred_single(cur, t, cond, depth)
        self._eps_c = eps_c
        taken = [0] * K
        on = [1] * K
        for j in range(num_inner_steps):
            eps_u = self.get_noise_pred_single(cur, t, uncond, depth, save=True)
            rec = self._step(cur, eps_u, eps_c, self.guidance_scale, a_t, a_p)
            _lib.check(L.dh_mse_cotangent_batch(_lib.ptr(rec), _lib.ptr(target), K, n, k, self.cotangent_amp, threshold,
                                                _lib.ptr(active), _lib.ptr(updated), _lib.ptr(loss_dev), _lib.ptr(d_eps),
                                                _lib.ptr(scale_dev), _lib.stream_ptr()), "dh_mse_cotangent_batch")
            _, d_text = self.model.unet.backward(None, d_eps, want_sample_grad=False, want_text_grad=True)
            _lib.check(L.dh_adam_step_scaled_batch(_lib.ptr(uncond), _lib.ptr(d_text), _lib.ptr(scale_dev), _lib.ptr(updated),
                                                   _lib.ptr(m), _lib.ptr(v), lr, 0.9, 0.999, 1e-8, j + 1, K, uncond[0].numel(),
                                                   _lib.stream_ptr()), "dh_adam_step_scaled_batch")
            taken = [n_ + o for n_, o in zip(taken, on)]
            if record is not None:
                record.setdefault("loss", []).append(loss_dev.tolist())
                record.setdefault("updated", []).append(list(on))
            on = active.tolist()                 # the one host read of the inner step (null_step reads the loss instead)
            if not any(on):
                break
        return taken

    def invert_batch(self, target_imgs, depths, prompts, num_inner_steps=10, early_stop_epsilon=1e-5, max_timesteps=None):
        """K images of the engine's resolution, each with its own depth and prompt, inverted in B = K engine passes: the DDIM
        inversion, then per timestep one B = K conditional forward, up to num_inner_steps x (saved B = K forward, backward to
        the K text embeddings, per-image Adam step and early stop) and the B = K unconditional forward of the CFG step.
        Returns one ((img, recon), init_noise [1,4,h,w], uncond [T,1,77,D]) per image, in input order; at K = 1 bit-identical
        to invert().  Needs an engine whose saved forwards may be K wide (max_diff_batch >= K)."""
        K = len(target_imgs)
        if K < 1 or not (len(depths) == len(prompts) == K):
            raise ValueError("invert_batch: target_imgs, depths and prompts must be non-empty and of the same length")
        unet = self.model.unet
        if unet.max_diff_batch < K:
            raise RuntimeError(f"engine max_diff_batch {unet.max_diff_batch} < K = {K}: inverting {K} images together needs "
                               f"max_diff_batch >= {K} (a diffuser built with max_batch >= {2 * K})")
        hw = tuple(self.model.get_image_shape()[:2])
        for b, img in enumerate(target_imgs):
            if tuple(img.shape[-2:]) != hw:
                raise ValueError(f"invert_batch: image {b} is {tuple(img.shape[-2:])}, the engine runs {hw} images")
        with self.model.on_stream():
            return self._invert_batch(target_imgs, depths, prompts, num_inner_steps, early_stop_epsilon, max_timesteps)

    @torch.no_grad()
    def _invert_batch(self, target_imgs, depths, prompts, num_inner_steps, epsilon, max_timesteps):
        dev = self.model.device
        K = len(target_imgs)
        depth_nhwc = None
        if self.model.conf.use_depth:
            depth_nhwc = torch.cat([self.model.init_depth(d.to(dev, torch.float32)).permute(0, 2, 3, 1) for d in depths])
            depth_nhwc = depth_nhwc.contiguous()
        contexts = [self.model.init_prompt(p) for p in prompts]
        uncond = torch.cat([c[0:1] for c in contexts]).contiguous()
        cond = torch.cat([c[1:2] for c in contexts]).contiguous()
        latent = self.image2latent(torch.cat([img.to(dev, torch.float32) for img in target_imgs]))
        recon = self.latent2image(latent)
        ddim_latents = self.ddim_loop(latent.permute(0, 2, 3, 1).contiguous(), torch.cat([uncond, cond]), depth_nhwc)
        out = []
        cur = ddim_latents[-1]
        steps = self.num_ddim_steps if max_timesteps is None else max_timesteps
        taken = []
        for i in range(steps):
            target = ddim_latents[len(ddim_latents) - i - 2]
            t = self.scheduler.timesteps[i]
            a_t, a_p = self.scheduler.step_alphas(t)
            taken.append(self.null_step_batch(cur, uncond, cond, depth_nhwc, i, target, num_inner_steps, epsilon))
            out.append(uncond.clone())
            # the CFG step with the optimised embeddings: the conditional half is this timestep's eps_c (null_optimization)
            eu = self.get_noise_pred_single(cur, t, uncond, depth_nhwc)
            cur = self._step(cur, eu, self._eps_c, self.guidance_scale, a_t, a_p)
        unconds = torch.stack(out, dim=0)                       # [T,K,77,D]
        self.inner_steps_taken = [[s[b] for s in taken] for b in range(K)]
        self.last_ddim_latents = ddim_latents
        init_noise = ddim_latents[-1].permute(0, 3, 1, 2)
        return [((target_imgs[b], recon[b:b + 1]), init_noise[b:b + 1], unconds[:, b:b + 1].contiguous()) for b in range(K)]
