"""DiffusionHandles facade (reference diffusion_handles.py:15-166) on the native MI355X path."""
import torch

from . import conf as _conf
from .depth_transform import laplacian_depth_blend, normalize_depth, transform_depth, transform_depth_footprints
from .guided_stable_diffuser import GuidedStableDiffuser
from .stable_null_inverter import StableNullInverter


class DiffusionHandles:
    def __init__(self, conf=None, **diffuser_kwargs):
        if conf is None:
            conf = _conf.load_default()
        self.conf = _conf.Conf.wrap(conf) if isinstance(conf, dict) else conf
        self.diffuser = GuidedStableDiffuser(conf=self.conf.guided_diffuser, **diffuser_kwargs)
        self.inverter = StableNullInverter(self.diffuser)
        self.device = torch.device("cpu")

    def to(self, device=None):
        self.diffuser.to(device=device)
        self.inverter.to(device=device)
        self.device = torch.device(device)
        return self

    def invert_input_image(self, img, depth, prompt):
        """-> (null_text_emb [T,1,77,D], init_noise [1,4,h,w])"""
        disparity = normalize_depth(1.0 / depth)
        _, init_noise, null_text_emb = self.inverter.invert(target_img=img, depth=disparity, prompt=prompt,
                                                            num_inner_steps=5, verbose=False)
        return null_text_emb, init_noise

    def generate_input_image(self, depth, prompt, null_text_emb=None, init_noise=None):
        """-> (null_text_emb, init_noise, activations [3], latent_image)"""
        disparity = normalize_depth(1.0 / depth)
        with torch.no_grad():
            activations, latent_image, null_text_emb, init_noise = self.diffuser.initial_inference(
                init_latents=init_noise, depth=disparity, uncond_embeddings=null_text_emb, prompt=prompt)
        return null_text_emb, init_noise, activations, latent_image

    def _require_identity_batch(self, K):
        unet = self.diffuser.unet
        if unet is not None and (unet.max_batch < 2 * K or unet.max_diff_batch < K):
            raise RuntimeError(f"engine max_batch {unet.max_batch} / max_diff_batch {unet.max_diff_batch} too small for {K} "
                               f"images: build the diffuser with max_batch >= {2 * K}")

    def invert_input_images(self, imgs, depths, prompts):
        """invert_input_image for K images of the same resolution in B = K passes (not in the reference).
        -> [(null_text_emb [T,1,77,D], init_noise [1,4,h,w])] per image.  Needs max_batch >= 2K."""
        self._require_identity_batch(len(imgs))
        disparities = [normalize_depth(1.0 / depth) for depth in depths]
        res = self.inverter.invert_batch(target_imgs=imgs, depths=disparities, prompts=prompts, num_inner_steps=5)
        return [(null_text_emb, init_noise) for _, init_noise, null_text_emb in res]

    def generate_input_images(self, depths, prompts, null_text_embs=None, init_noises=None):
        """generate_input_image for K images in B = 2K CFG passes (not in the reference).
        -> [(null_text_emb, init_noise, activations [3], latent_image)] per image.  Needs max_batch >= 2K."""
        self._require_identity_batch(len(depths))
        disparities = [normalize_depth(1.0 / depth) for depth in depths]
        with torch.no_grad():
            res = self.diffuser.initial_inference_batch(init_latents=init_noises, depths=disparities,
                                                        uncond_embeddings=null_text_embs, prompts=prompts)
        return [(null_text_emb, init_noise, activations, latent_image)
                for activations, latent_image, null_text_emb, init_noise in res]

    def set_foreground(self, depth, fg_mask, bg_depth):
        """Background depth = input depth with the hole of the (15x cross-dilated) foreground mask in-filled
        from the background depth's Laplacian (reference diffusion_handles.py:90-111).  fg_mask may be a list of masks
        (several objects, transform_foreground_objects): the blend runs over their union.  The masks of objects an edit DELETES
        (removed_masks of transform_foreground_objects) belong in that list too: bg_depth is the depth with all of them removed.
        With conf depth_transform_infill_border: reflect the blend treats the image frame as a mirror (_infill_border); the
        parameter list stays the reference's."""
        if isinstance(fg_mask, (list, tuple)):
            union = fg_mask[0] != 0
            for m in fg_mask[1:]:
                union = union | (m != 0)
            fg_mask = union.to(fg_mask[0].dtype)
        return laplacian_depth_blend(depth, bg_depth, fg_mask, dilate_iterations=15,
                                     infill_border=self._infill_border("set_foreground"))

    def _conf_get(self, key, default=None):
        conf = self.conf
        return conf.get(key, default) if hasattr(conf, "get") else getattr(conf, key, default)

    def _infill_border(self, what):
        """The optional top-level conf key depth_transform_infill_border (absent = zero) -> "zero" or "reflect", the keyword of
        the depth_transform calls (DESIGN.md "In-fill border").  ValueError for any other value; "reflect" under a mode other
        than 'pc' raises NotImplementedError naming the setting: the mesh mode in-fills against zero only.  No device work."""
        from .depth_transform import INFILL_BORDERS, check_infill_border, mesh_has_no_infill_border
        value = self._conf_get("depth_transform_infill_border", None)
        if self.conf.depth_transform_mode != "pc":
            mesh_has_no_infill_border(value, f"{what}: conf depth_transform_infill_border")
        return INFILL_BORDERS[check_infill_border(value, f"{what}: conf depth_transform_infill_border")]

    def _footprints(self, what):
        """The optional top-level conf keys depth_transform_footprints (absent = false) and
        depth_transform_footprint_max_ratio (absent = none) as the keywords of the depth_transform calls.  Checked on the host
        (ValueError); a true depth_transform_footprints under a mode other than 'pc' raises NotImplementedError: the mesh mode
        has no footprints.  The third key of the re-projection, depth_transform_infill_border, is read and checked here too
        (_infill_border: every edit call passes through this helper before any device work) and travels in
        _reproject_keywords.  No device work."""
        from .depth_transform import check_footprints, mesh_has_no_footprints
        fp, ratio = self._conf_get("depth_transform_footprints", False), self._conf_get("depth_transform_footprint_max_ratio", None)
        if self.conf.depth_transform_mode != "pc":
            mesh_has_no_footprints(fp, ratio, f"{what}: conf depth_transform_footprints")
        fp, _ = check_footprints(fp, ratio, f"{what}: conf depth_transform_footprints")
        self._infill_border(what)
        self._view_surfaces(what)
        return dict(footprints=fp, footprint_max_ratio=ratio)

    def _view_surfaces(self, what):
        """The optional top-level conf keys depth_transform_view_surfaces (absent = false) and
        depth_transform_view_surface_max_ratio (absent = none) as the keywords of depth_transform.reproject (DESIGN.md "View
        surfaces"): under a camera the scene is splatted as triangles.  Checked on the host (ValueError,
        depth_transform.check_view_surfaces); a true key under a mode other than 'pc' raises NotImplementedError naming the
        setting.  Read wherever an edit call reads its camera -- and, like the border, by every edit call through _footprints,
        before any device work.  Without a camera the setting changes nothing."""
        from .depth_transform import check_view_surfaces, mesh_has_no_view_surfaces
        vs = self._conf_get("depth_transform_view_surfaces", False)
        ratio = self._conf_get("depth_transform_view_surface_max_ratio", None)
        if self.conf.depth_transform_mode != "pc":
            mesh_has_no_view_surfaces(vs, ratio, f"{what}: conf depth_transform_view_surfaces")
        vs, _ = check_view_surfaces(vs, ratio, f"{what}: conf depth_transform_view_surfaces")
        return dict(view_surfaces=vs, view_surface_max_ratio=ratio)

    def _reproject_keywords(self, what, cameras=False):
        """_footprints and the in-fill border: the keywords of depth_transform.reproject that come from the conf; cameras: the
        call passes cameras on, so the view-surface keywords travel too."""
        kw = dict(self._footprints(what), infill_border=self._infill_border(what))
        return dict(kw, **self._view_surfaces(what)) if cameras else kw

    def _lock_setup(self, what, activations, depth, release_mask=None):
        """The optional top-level conf keys background_lock (absent = false), background_lock_dilate and
        background_lock_feather (cells, absent = 2 each) and what an edit call needs for its lock: None with the lock off (a
        release_mask is then an error), else (dilate, feather, trajectory, release_mask [res,res] or None).  Host checks only
        (ValueError naming `what`): malformed keys, a release mask that is no res x res image, activations without the
        reconstruction trajectory -- never a silent unlocked edit."""
        from . import background_lock as BL
        reach = BL.lock_conf(self.conf, what)
        if reach is None:
            if release_mask is not None:
                raise ValueError(f"{what}: release_mask needs conf background_lock: true")
            return None
        release = BL.check_release_mask(release_mask, depth.shape[-1], what)
        return reach + (BL.require_trajectory(activations, what), release)

    def _edit_lock(self, setup, fg_masks, correspondences, depth):
        """(keep, trajectory) of one edit -- its keep map from its mask(s), correspondences and release mask -- or None."""
        if setup is None:
            return None
        from . import background_lock as BL
        dilate, feather, trajectory, release = setup
        corr = torch.as_tensor(correspondences).to(self.device)
        keep = BL.keep_map(corr, fg_masks, release, depth.shape[-1], self.diffuser.unet.sample_size, dilate, feather)
        self.last_keep_maps.append(keep)
        return keep, trajectory

    last_keep_maps = ()          # the keep maps of the last edit call with the background lock on, in edit order

    def transform_foreground_batch(self, depth, prompt, fg_mask, bg_depth, null_text_emb, init_noise, activations,
                                   transforms, fg_weight=None, bg_weight=None, use_input_depth_normalization=False,
                                   streams=1, batch=None, release_mask=None):
        """K edits of one image in batched passes (not in the reference; BASELINE config 3).
        transforms: list of (rot_angle_deg, rot_axis[3], translation[3]) or (rot_angle_deg, rot_axis[3], translation[3], scale,
        pivot) (transform_foreground says what scale and pivot do).  Returns (images [K,3,H,W], [K disparities]).
        streams > 1: the K edits are cut into chunks of `batch` (default ceil(K / streams)) and the chunks run on `streams`
        concurrent lanes that share the U-Net weights (GuidedStableDiffuser.fork); batch = 1 runs single (B = 1) edits on the
        lanes.  Images are bit-identical to the one-stream result at the same batch.  release_mask (conf background_lock
        only): extra area every edit's lock sets free (transform_foreground_objects)."""
        from .depth_transform import reproject
        fp = self._reproject_keywords("transform_foreground_batch")
        lk = self._lock_setup("transform_foreground_batch", activations, depth, release_mask)
        with torch.no_grad():
            # (`reproject_edits` keeps its parameter list, which has no border: its body, with the border)
            edits = reproject(depth, bg_depth, [fg_mask], self.diffuser.get_depth_intrinsics(device=depth.device),
                              [[tf] for tf in transforms], use_input_depth_normalization=use_input_depth_normalization,
                              device_correspondences=True, **fp)
            self.last_keep_maps = []
            lock = {} if lk is None else dict(lock=[self._edit_lock(lk, fg_mask, c, depth) for _, c in edits])
            imgs = self._guided_batch(edits, streams, batch, (init_noise, null_text_emb, prompt, activations, fg_weight, bg_weight),
                                      {}, lock)
        return imgs, [d for d, _ in edits]

    def _guided_batch(self, edits, streams, batch, args, shared, per_edit, donor_acts=None):
        """The route of K re-projected edits (disparity, correspondences) of one image, chosen in one place: the whole batch in
        one loop (one stream, and a batch that holds all K), single edits on lanes (batch = 1), or chunks of `batch` edits (default
        ceil(K / streams)) on lanes.  args: (init_noise, null_text_emb, prompt, activations, fg_weight, bg_weight); shared: the
        guidance keywords all edits share; per_edit: those that are one entry per edit (_guidance_keywords) -- the chunked
        route takes "pair_instances" and "donor" as one list per chunk (the lock stays one entry per edit), and this is the one
        place where per-edit lists are cut; a "donor" entry travels as (donor_acts, its list).  -> images [K,3,H,W]."""
        init_noise, null_text_emb, prompt, activations, fg_weight, bg_weight = args
        K, lanes = len(edits), max(1, int(streams))
        per = K if batch is None and streams <= 1 else int(batch or -(-K // lanes))
        whole = streams <= 1 and per >= K
        cut = (lambda v: v) if whole or per <= 1 else (lambda v: [v[i:i + per] for i in range(0, K, per)])
        kw = dict(shared, **{k: cut(v) if k in ("pair_instances", "donor") else v for k, v in per_edit.items()})
        if "donor" in kw:
            kw["donor"] = (donor_acts, kw["donor"])
        if whole:
            return self.diffuser.guided_inference_batch(init_noise, [d for d, _ in edits], null_text_emb, prompt, activations,
                                                        [c for _, c in edits], fg_weight, bg_weight, **kw)
        if per <= 1:
            return torch.cat(self.diffuser.guided_inference_lanes(init_noise, edits, null_text_emb, prompt, activations, lanes,
                                                                  fg_weight, bg_weight, **kw))
        chunks = [([d for d, _ in chunk], [c for _, c in chunk]) for chunk in cut(edits)]
        return torch.cat(self.diffuser.guided_inference_batch_lanes(init_noise, chunks, null_text_emb, prompt, activations, lanes,
                                                                    fg_weight, bg_weight, **kw))

    def _camera_setup(self, what, cameras, donor):
        """The host checks of an edit call's cameras (camera moves; DESIGN.md "Camera moves"), before any identity or launch ->
        None (no camera: None, or every entry None: the call without the keyword) or the list of checked cameras / None.
        ValueError (depth_transform.check_camera) naming `what` and the edit; NotImplementedError naming the setting for mesh
        mode, footprints, conf background_lock: true (the reconstruction's latents belong to another view) and a donor."""
        if cameras is None:
            return None
        from .depth_transform import check_camera
        cams = [check_camera(c, f"{what}: edit {e}") for e, c in enumerate(cameras)]
        if all(c is None for c in cams):
            return None
        self._view_surfaces(what)          # (the keys that act on a camera edit: mesh mode names the setting when it is on)
        if self.conf.depth_transform_mode != "pc":
            raise NotImplementedError(f"{what}: depth_transform_mode {self.conf.depth_transform_mode!r} has no camera moves "
                                      "(camera; only 'pc')")
        if self._footprints(what)["footprints"]:
            raise NotImplementedError(f"{what}: depth_transform_footprints: true has no camera moves (camera)")
        from . import background_lock as BL
        if BL.lock_conf(self.conf, what) is not None:
            raise NotImplementedError(f"{what}: background_lock: true has no camera moves (camera; the reconstruction's latents "
                                      "belong to another view)")
        if donor is not None:
            raise NotImplementedError(f"{what}: donor together with a camera is not supported (camera)")
        return cams

    @staticmethod
    def _camera_weights(what, object_weights, n_instances):
        """object_weights of a camera edit: the background is instance N, so N + 1 entries, N + 1 <= 8 (ValueError)."""
        if object_weights is None:
            return None
        from .losses import MAX_OBJECTS, check_object_weights
        if n_instances + 1 > MAX_OBJECTS:
            raise ValueError(f"{what}: a camera edit with object_weights takes at most {MAX_OBJECTS - 1} instances (the background "
                             f"is instance N), got {n_instances}")
        try:
            return check_object_weights(object_weights, n_instances + 1)
        except ValueError as err:
            raise ValueError(f"{what}: {err} (one weight per instance and one for the background)") from None

    def _reproject_objects(self, what, depth, bg_depth, fg_masks, edits, use_input_depth_normalization, device_correspondences,
                           instances=None, removed_masks=None, donor=None, cameras=None):
        """instances given: every result is (disparity, correspondences, instance of every row).  removed_masks: the masks of the
        objects the edits delete (object removal); fg_masks may then be empty and the edits K empty lists.  donor: None or the
        checked donor (_donor_setup): its masks follow fg_masks in the object list, and an instance table is always given."""
        from .depth_transform import Bend, check_body, check_instances, reproject
        if cameras is not None and len(fg_masks) == 0 and removed_masks is None:
            removed_masks = []          # (checked by _camera_setup: no donor, no footprints, 'pc' mode)
        fp = self._reproject_keywords(what, cameras=True)
        if self.conf.depth_transform_mode != "pc":
            if any(isinstance(tf, Bend) for tfs in edits for tf in tfs):
                raise NotImplementedError(f"{what}: depth_transform_mode {self.conf.depth_transform_mode!r} has no bend edits "
                                          "(Bend; only 'pc')")
            if removed_masks is not None:
                raise NotImplementedError(f"{what}: depth_transform_mode {self.conf.depth_transform_mode!r} has no object removal "
                                          "(removed_masks; only 'pc')")
            if instances is not None:
                raise NotImplementedError(f"{what}: depth_transform_mode {self.conf.depth_transform_mode!r} has no copies of an "
                                          "object (instances; only 'pc')")
            raise NotImplementedError(f"{what}: depth_transform_mode {self.conf.depth_transform_mode!r} has no multi-object "
                                      "re-projection (only 'pc')")
        kw = dict(removed_masks=removed_masks, cameras=cameras, use_input_depth_normalization=use_input_depth_normalization,
                  device_correspondences=device_correspondences, what=what, **fp)
        n_donor = 0
        if donor is not None:
            kw.update(donor_depth=donor[0], donor_masks=donor[1])
            n_donor = len(donor[1])
        intrinsics = self.diffuser.get_depth_intrinsics(device=depth.device)
        if removed_masks is not None and len(fg_masks) == 0 and donor is None:
            # nothing moves: the re-projection refuses transforms and an instance table under this call's name
            return reproject(depth, bg_depth, [], intrinsics, edits, instances=instances, **kw)
        inst = check_instances(instances, len(fg_masks) + n_donor, f"{what}: instances")
        n_bodies, body = (len(fg_masks), "object") if inst is None else (len(inst), "instance")
        if all(len(tfs) == n_bodies for tfs in edits):          # (else the re-projection names the edit)
            every = list(fg_masks) + ([] if donor is None else list(donor[1]))
            mask_of = lambda m: every[m if inst is None else inst[m]]
            edits = [[self._fill_body(check_body(tf, mask_of(m), f"{what}: edit {e}, {body} {m}")) for m, tf in enumerate(tfs)]
                     for e, tfs in enumerate(edits)]
        return reproject(depth, bg_depth, fg_masks, intrinsics, edits, instances=inst, return_instances=inst is not None, **kw)

    @classmethod
    def _fill_body(cls, tf):
        """_fill_transform for what stands for an instance: a transform, or a Bend (every bone filled in)."""
        from .depth_transform import Bend
        if isinstance(tf, Bend):
            return Bend([cls._fill_transform(b) for b in tf.bones], tf.weights)
        return cls._fill_transform(tf)

    @staticmethod
    def _fill_transform(tf):
        """The None members of a transform's rotation angle, axis and translation filled in: no turn, about Y, no move."""
        angle, axis, translation, *rest = tf
        return (0.0 if angle is None else angle, torch.tensor([0.0, 1.0, 0.0], dtype=torch.float32) if axis is None else axis,
                torch.zeros(3) if translation is None else translation, *rest)

    def _donor_setup(self, what, donor, fg_masks, depth, activations):
        """The host checks of an edit call's donor, before any library launch -> None (no donor: None, or every donor mask empty)
        or (donor depth, donor masks, donor activations).  ValueError naming `what`, the edit's donor and the member: a donor
        that is no dict with depth, masks and activations, what depth_transform.check_donor refuses (another resolution,
        overlapping or empty masks, M + D > 8), activations with another number of layers or timesteps than the host's.
        NotImplementedError naming the setting for mesh mode and for footprints."""
        if donor is None:
            return None
        if not isinstance(donor, dict):
            raise ValueError(f"{what}: donor: expected a dict with depth, masks and activations, got {type(donor).__name__}")
        for member in ("depth", "masks", "activations"):
            if donor.get(member) is None:
                raise ValueError(f"{what}: donor: no {member}")
        extra = set(donor) - {"depth", "masks", "activations"}
        if extra:
            raise ValueError(f"{what}: donor: unknown members {sorted(extra)}")
        if self.conf.depth_transform_mode != "pc":
            raise NotImplementedError(f"{what}: depth_transform_mode {self.conf.depth_transform_mode!r} has no object insertion "
                                      "(donor; only 'pc')")
        if self._footprints(what)["footprints"]:
            raise NotImplementedError(f"{what}: depth_transform_footprints: true has no object insertion (donor; two images "
                                      "share pixel indices)")
        if self._view_surfaces(what)["view_surfaces"]:
            raise NotImplementedError(f"{what}: depth_transform_view_surfaces: true has no object insertion (donor; two images "
                                      "share pixel indices)")
        from .depth_transform import check_donor
        acts = donor["activations"]
        try:
            n_layers = len(acts)
        except TypeError:
            raise ValueError(f"{what}: donor: activations: expected the activations of an identity") from None
        if n_layers != len(activations):
            raise ValueError(f"{what}: donor: activations of {n_layers} layers, the host's have {len(activations)}")
        for k, (a, o) in enumerate(zip(acts, activations)):
            if a.shape[0] != o.shape[0]:
                raise ValueError(f"{what}: donor: activations of layer {k} hold {a.shape[0]} timesteps, the host's {o.shape[0]}")
        checked = check_donor(donor["depth"], donor["masks"], depth.shape[-1], len(fg_masks), what)
        return None if checked is None else checked + (acts,)

    @staticmethod
    def _lock_rows(correspondences, row_donor):
        """The correspondences the background lock sees: a donor row's source pixel lies in another image, so it is overwritten
        with the row's target pixel (where the tensor lives: on the device for the batched calls)."""
        corr = torch.as_tensor(correspondences).clone()
        flagged = row_donor.to(corr.device) != 0
        corr[:, 0:2] = torch.where(flagged[:, None], corr[:, 2:4], corr[:, 0:2])
        return corr

    @staticmethod
    def _vacated(removed_masks, what):
        """The guidance's keyword of an edit that deletes objects: {} for none, else dict(vacated=[res, res] uint8 union)."""
        if removed_masks is None:
            return {}
        from .depth_transform import vacated_image
        image = vacated_image(removed_masks)
        return {} if image is None else dict(vacated=image)

    def _check_removal(self, what, fg_masks, removed_masks):
        """The host checks of an edit call's removed_masks, before any device work: mesh mode has none (NotImplementedError naming
        the setting); a mask of another size raises ValueError naming `what` and the mask (check_removed_masks; an overlap is
        found by the re-projection, in the copy that reads the pixel counts, before its first launch)."""
        if removed_masks is None:
            return
        if self.conf.depth_transform_mode != "pc":
            raise NotImplementedError(f"{what}: depth_transform_mode {self.conf.depth_transform_mode!r} has no object removal "
                                      "(removed_masks; only 'pc')")
        from .depth_transform import check_removed_masks
        removed = check_removed_masks(removed_masks, fg_masks, f"{what}: removed_masks")
        if len(fg_masks) == 0 and not removed:
            raise ValueError(f"Expected 1 to 8 foreground masks, got 0 ({what}: no removed mask either)")

    @staticmethod
    def _object_labels(fg_masks, object_weights, instances=None, what="instances"):
        """Host checks of object_weights against the M masks -- with an instance table, against its N instances (and of the
        table itself) -- (ValueError, before any launch) and the label image the guidance needs; (None, None) for no weights:
        the unweighted path.  With an instance table there is no label image: the re-projection's per-row instances say which
        object of the energy a correspondence belongs to."""
        n = len(fg_masks)
        if n == 0:              # a pure removal (its refusals are _reproject_objects'): no object, so no weights
            if object_weights is not None:
                raise ValueError(f"{what.split(':')[0]}: object_weights={object_weights!r} given without a foreground mask")
            return None, None
        if instances is not None:
            from .depth_transform import check_instances
            n = len(check_instances(instances, len(fg_masks), what))
        if object_weights is None:
            return None, None
        from .losses import check_object_weights, object_label_image
        try:
            weights = check_object_weights(object_weights, n)
        except ValueError as err:
            if instances is None:
                raise
            raise ValueError(f"{what}: {err} (one weight per instance)") from None
        return (object_label_image(fg_masks) if instances is None else None), weights

    def transform_foreground_objects(self, depth, prompt, fg_masks, bg_depth, null_text_emb, init_noise, activations,
                                     transforms, fg_weight=None, bg_weight=None, use_input_depth_normalization=False,
                                     object_weights=None, camera=None, donor=None, removed_masks=None, instances=None,
                                     release_mask=None):
        """One edit that moves M objects of one image (not in the reference).  fg_masks: M pairwise disjoint masks (at most 8);
        bg_depth: the depth with all of them removed (set_foreground takes the list); transforms: M (rot_angle_deg,
        rot_axis[3], translation[3]) or (rot_angle_deg, rot_axis[3], translation[3], scale, pivot), one per mask.  Each object
        turns about its own centroid, or is scaled and turned about its pivot (transform_foreground); they occlude the background
        and each other (depth_transform.reproject).  The guidance sees the union of the correspondences: its
        foreground term is the mean over all pairs, so the objects weigh by covered area -- unless object_weights says
        otherwise: "equal" holds every object equally, a sequence of M floats (finite, >= 0, not all zero) sets each weight;
        objects without a visible correspondence drop out and the rest are renormalised (DESIGN.md "A weight per object";
        default configuration only).  Returns what transform_foreground returns.  'pc' re-projection only.  release_mask (conf
        background_lock only): a res x res image, non-zero = extra area the lock sets free beside the masks and the
        correspondences, such as the shadow an object leaves behind.
        instances (copies of an object; DESIGN.md "Object copies"): None, or N mask indices (M <= N <= 8, every mask named) --
        the edit places N instances, instance n the object of mask instances[n] under transforms[n] (N transforms); a mask
        named twice appears twice.  object_weights then has N entries and "equal" holds every instance equally.  ValueError
        naming the instance for a bad table, before any device work.
        removed_masks (object removal; DESIGN.md "Object removal"): None, or the masks of the objects the edit DELETES, disjoint
        from each other and from fg_masks; bg_depth has them removed too.  They contribute no point to the re-projection, their
        cells leave the guidance's original-background list, and the background lock sets them free (release_mask stays the
        tool for the shadow).  fg_masks may then be empty with transforms [] -- a pure removal: the disparity is the
        re-projection of the background alone.  Meant to run with conf background_lock: true.  ValueError naming the mask for
        an overlap or another size, for no mask at all, and for transforms without a foreground mask, before any device work.
        donor (object insertion; DESIGN.md "Object insertion"): None, or a dict {"depth", "masks", "activations"} -- the depth of
        a SECOND image of this image's resolution and intrinsics, D >= 1 pairwise disjoint masks of objects in it, and that
        image's identity activations (set_foreground / invert_input_image on the donor image).  The edit's objects are then the
        M masks of fg_masks (0 .. M - 1) followed by the donor's D masks (M .. M + D - 1), M + D <= 8: transforms, instances,
        object_weights and "equal" speak about that list.  fg_masks may be [] (a pure insertion; bg_depth is then the depth, or
        the depth with the removed masks removed).  The inserted object's features come from the donor's activations; it
        occludes and is occluded like any object.  No relative depth scale is estimated: two monocular depth estimates
        disagree by a factor, which the caller brings as the transform's `scale`.  Donor edits run on the weighted energy:
        object_weights=None weighs every instance by its pair count, which gives every pair the unweighted coefficient
        fg_w / (C N) up to rounding.  Default guidance configuration only; 'pc' mode without footprints
        (NotImplementedError naming the setting).  ValueError naming the call, the donor and the member before any launch
        (_donor_setup).  A donor whose masks are all empty is the call without the keyword.
        camera (camera moves; DESIGN.md "Camera moves"): None, or (rot_angle_deg, rot_axis, translation[, pivot]) -- the motion
        of the CAMERA in the coordinates of depth_to_world_coords: turned about rot_axis through pivot (None = the camera centre:
        a pan or tilt; depth_transform.pivot_at_pixel gives an orbit centre), then translated.  The whole image is then seen
        from the moved viewpoint, and the background yields correspondences of its own, which join the guidance's pairs.  With
        object_weights the background is instance N: the list has N + 1 entries (N + 1 <= 8) and "equal" includes the
        background; under the default area weighting the background's rows outnumber the objects' by roughly ten to one.
        fg_masks = [] with transforms = [] is the pure camera move.  ValueError (depth_transform.check_camera) before any
        launch; NotImplementedError naming the setting for mesh mode, footprints, background_lock: true and a donor.
        camera=None is the call without the keyword, byte for byte.
        Bend edits (DESIGN.md "Bend edits"): a member of transforms may be a depth_transform.Bend -- up to 4 transforms (bones)
        and a weight per pixel and bone; depth_transform.bend_chain builds one from a line across the object -- and the
        object then changes its shape: each of its points goes to the weighted sum of where the bones put it.  Everything
        else of the call (instances, removed_masks, donor, camera, object_weights, footprints, view surfaces, the in-fill
        border, the background lock) sees points, rows and masks as before.  ValueError (depth_transform.check_bend) naming the
        call, the edit and the instance before any launch; NotImplementedError naming Bend in mesh mode."""
        what = "transform_foreground_objects"
        fg_masks = list(fg_masks)
        cams = self._camera_setup(what, None if camera is None else [camera], donor)
        st = self._objects_setup(what, depth, fg_masks, activations, cams, donor, removed_masks, instances, object_weights,
                                 release_mask)
        with torch.no_grad():
            res = self._reproject_objects(what, depth, bg_depth, fg_masks, [transforms], use_input_depth_normalization, False,
                                          st.instances, removed_masks, st.donor, cams)
            shared, per_edit = self._guidance_keywords(what, st, res, depth, fg_masks, removed_masks)
            kw = dict(shared, **{k: v[0] for k, v in per_edit.items()})
            if st.donor is not None:
                kw["donor"] = (st.donor[2], kw["donor"])
            edited_disparity, correspondences = res[0][:2]
            results = self.diffuser.guided_inference(
                latents=init_noise, depth=edited_disparity, uncond_embeddings=null_text_emb, prompt=prompt,
                activations_orig=activations, correspondences=correspondences, fg_weight=fg_weight,
                bg_weight=bg_weight, save_denoising_steps=self.conf.guided_diffuser.save_denoising_steps, **kw)
        return self._edit_result(results, edited_disparity)

    def _edit_result(self, results, edited_disparity):
        """What a single edit returns: (image, disparity), with conf save_denoising_steps (image, disparity, denoising steps)."""
        if self.conf.guided_diffuser.save_denoising_steps:
            edited_img, denoising_steps = results
            return edited_img, edited_disparity, denoising_steps
        return results, edited_disparity

    def _objects_setup(self, what, depth, fg_masks, activations, cams, donor, removed_masks, instances, object_weights, release_mask):
        """The host checks an edit of several objects makes before its re-projection, for one edit and for K alike -> a record
        of: cams (the checked cameras, _camera_setup), donor (the checked donor or None, _donor_setup), instances (the table; with a
        donor the implied one over the host's and the donor's masks), labels and weights (_object_labels; with cameras the
        weights of _camera_weights: the background is instance N), N (with cameras: the instance index of the background's rows)
        and lock (_lock_setup; None with cameras, which the lock refuses)."""
        from types import SimpleNamespace
        if cams is not None:
            from .depth_transform import check_instances
            self._check_removal(what, fg_masks, removed_masks)
            inst = check_instances(instances, len(fg_masks), f"{what}: instances") if fg_masks else None
            N = len(fg_masks) if inst is None else len(inst)
            if not fg_masks and object_weights is not None:
                raise ValueError(f"{what}: object_weights={object_weights!r} given without a foreground mask")
            return SimpleNamespace(cams=cams, donor=None, instances=instances, labels=None, N=N, lock=None,
                                   weights=self._camera_weights(what, object_weights, N))
        dn = self._donor_setup(what, donor, fg_masks, depth, activations)
        bodies = fg_masks
        if dn is not None:
            if removed_masks is not None:
                self._check_removal(what, fg_masks or list(dn[1]), removed_masks)
            bodies = fg_masks + list(dn[1])
            instances = list(range(len(bodies))) if instances is None else instances
        else:
            self._check_removal(what, fg_masks, removed_masks)
        labels, weights = self._object_labels(bodies, object_weights, instances, f"{what}: instances")
        return SimpleNamespace(cams=None, donor=dn, instances=instances, labels=labels, weights=weights, N=None,
                               lock=self._lock_setup(what, activations, depth, release_mask))

    def _guidance_keywords(self, what, st, res, depth, fg_masks, removed_masks):
        """The guidance's keywords for the K re-projected edits `res` of one _objects_setup -> (those all edits share, those
        that are one entry per edit: K long lists).  A "donor" entry is the donor-row flags per edit; the loops take it as
        (the donor's activations, flags)."""
        self.last_keep_maps = []
        shared, per_edit = self._vacated(removed_masks, what), {}
        if st.cams is not None:
            # the rows are the instance rows, then the background's with instance index N; with weights the instance column is
            # the energy's object.  (An edit without a camera has no background row: its kinds are all zero, the call without.)
            per_edit["row_kind"] = [(r[2] == st.N).to(torch.uint8) * 2 for r in res]
            if st.weights is not None:
                per_edit["pair_instances"] = [r[2] for r in res]
                shared["object_weights"] = st.weights
            return shared, per_edit
        shared.update(object_labels=st.labels, object_weights=st.weights)
        lock_corrs = [r[1] for r in res]
        if st.donor is not None:
            from .depth_transform import donor_rows
            per_edit["donor"] = [donor_rows(r[2], st.instances, len(fg_masks)) for r in res]
            lock_corrs = [self._lock_rows(c, f) for c, f in zip(lock_corrs, per_edit["donor"])]
        if st.lock is not None:
            per_edit["lock"] = [self._edit_lock(st.lock, fg_masks + list(removed_masks or []), c, depth) for c in lock_corrs]
        if st.instances is not None:
            per_edit["pair_instances"] = [r[2] for r in res]
        return shared, per_edit

    def transform_foreground_objects_batch(self, depth, prompt, fg_masks, bg_depth, null_text_emb, init_noise, activations,
                                           edits, fg_weight=None, bg_weight=None, use_input_depth_normalization=False,
                                           object_weights=None, streams=1, batch=None, cameras=None, donor=None,
                                           removed_masks=None, instances=None, release_mask=None):
        """K edits of one image, each moving the M objects of fg_masks (transform_foreground_objects), in batched passes.
        edits: K lists of M (rot_angle_deg, rot_axis[3], translation[3]) or (rot_angle_deg, rot_axis[3], translation[3], scale,
        pivot).  Returns (images [K,3,H,W], [K disparities]) as
        transform_foreground_batch does.  object_weights: as in transform_foreground_objects, one list for all K edits.
        streams / batch: transform_foreground_batch's -- chunks of `batch` edits (default ceil(K / streams)) on `streams`
        lanes, batch = 1 runs single edits on the lanes; images are bit-identical to the one-stream result at the same batch.
        release_mask: transform_foreground_objects', one for all K edits.  instances: transform_foreground_objects', one table
        for all K edits (the edits are then K lists of N transforms).  removed_masks: transform_foreground_objects', one list for
        all K edits (with fg_masks empty the edits are K empty lists: K identical pure removals).  donor:
        transform_foreground_objects', one donor for all K edits (they share the channels-last copy of its activations).
        cameras (camera moves): None, or a list of K, one camera (transform_foreground_objects) or None per edit -- K views of
        one image are a turntable (depth_transform.orbit_cameras).  Edits with and without a camera share the call; the camera
        call runs as one batch on one stream (NotImplementedError for streams > 1 or a smaller batch)."""
        what = "transform_foreground_objects_batch"
        fg_masks = list(fg_masks)
        if cameras is not None and len(cameras) != len(edits):
            raise ValueError(f"{what}: cameras has {len(cameras)} entries for {len(edits)} edits")
        cams = self._camera_setup(what, cameras, donor)
        if cams is not None:
            if streams > 1 or (batch is not None and int(batch) < len(edits)):
                raise NotImplementedError(f"{what}: cameras run as one batch on one stream (streams={streams}, batch={batch})")
            if release_mask is not None:
                raise ValueError(f"{what}: release_mask needs conf background_lock: true")
        st = self._objects_setup(what, depth, fg_masks, activations, cams, donor, removed_masks, instances, object_weights,
                                 release_mask)
        with torch.no_grad():
            res = self._reproject_objects(what, depth, bg_depth, fg_masks, edits, use_input_depth_normalization, True, st.instances,
                                          removed_masks, st.donor, cams)
            shared, per_edit = self._guidance_keywords(what, st, res, depth, fg_masks, removed_masks)
            res = [r[:2] for r in res]
            imgs = self._guided_batch(res, streams, batch, (init_noise, null_text_emb, prompt, activations, fg_weight, bg_weight),
                                      shared, per_edit, None if st.donor is None else st.donor[2])
        return imgs, [d for d, _ in res]

    EDIT_FIELDS = ("depth", "prompt", "fg_mask", "bg_depth", "null_text_emb", "init_noise", "activations")

    def transform_foregrounds(self, edits, use_input_depth_normalization=False):
        """K edits of DIFFERENT images in batched passes (not in the reference).  edits: K dicts with the arguments of
        transform_foreground (EDIT_FIELDS, rot_angle / rot_axis / translation / scale / pivot, optional fg_weight / bg_weight)
        -- or, for an edit that moves several objects (transform_foreground_objects), `fg_masks` (M masks) in place of fg_mask,
        `transforms` (M triples (rot_angle, rot_axis, translation) or 5-tuples (.., scale, pivot), None members defaulted) in
        place of rot_angle / rot_axis / translation / scale / pivot, and optionally `object_weights` and `instances` (copies of an
        object, transform_foreground_objects: N mask indices; `transforms` and the weights are then N long).  An edit with both forms
        or with neither, with a `transforms` list that is not M long, or with a malformed transform (check_transform) raises
        ValueError naming the edit, before any device work.  Edits that name the same image (the same depth, mask,
        background-depth and activation tensors) are re-projected together, once per image (multi-object edits: one label
        image per image); then one GuidedStableDiffuser.guided_inference_items for single- and multi-object edits alike.
        Returns (images [K,3,H,W], [K disparities]) in input order.  'pc' re-projection only; one resolution; needs an engine
        with max_batch >= 2K.  With conf background_lock every edit is locked to its own image's reconstruction; an edit may
        carry a `release_mask` (transform_foreground_objects).  A multi-object edit may carry `removed_masks` (object removal,
        transform_foreground_objects; fg_masks may then be [] with no transforms): edits of one image that differ in it are
        re-projected in separate calls, and edits with and without it share the batch.  A multi-object edit may carry `camera`
        (camera moves, transform_foreground_objects; fg_masks may then be [] with no transforms: a pure camera move): edits with
        and without a camera share the batch, and edits of one image share its re-projection call."""
        from .depth_transform import check_body, check_instances, check_removed_masks, check_transform, reproject
        fp = self._reproject_keywords("transform_foregrounds")
        if self.conf.depth_transform_mode != "pc":
            raise NotImplementedError(f"transform_foregrounds: depth_transform_mode {self.conf.depth_transform_mode!r} has no "
                                      "batched re-projection (only 'pc')")
        K = len(edits)
        for i, e in enumerate(edits):
            if isinstance(e, dict) and "donor" in e:
                raise NotImplementedError(f"transform_foregrounds: edit {i}: donor (object insertion is not supported in "
                                          "mixed-image batches; transform_foreground_objects[_batch])")
        common = tuple(f for f in self.EDIT_FIELDS if f != "fg_mask")
        if K < 1 or any(set(common) - set(e) for e in edits):
            raise ValueError(f"transform_foregrounds: needs at least one edit, each with {self.EDIT_FIELDS}")
        single_keys = ("fg_mask", "rot_angle", "rot_axis", "translation", "scale", "pivot")
        multi_keys = ("fg_masks", "transforms", "object_weights", "instances", "removed_masks", "camera")
        weights = [None] * K
        cams = [None] * K
        for i, e in enumerate(edits):
            if isinstance(e, dict) and e.get("camera") is not None:
                cams[i] = self._camera_setup(f"transform_foregrounds: edit {i}", [e["camera"]], None)
                cams[i] = None if cams[i] is None else cams[i][0]
        for i, e in enumerate(edits):
            single = any(e.get(k) is not None for k in single_keys)
            multi = any(e.get(k) is not None for k in multi_keys)
            if single and multi:
                raise ValueError(f"transform_foregrounds: edit {i} mixes the one-object form {single_keys} with the multi-object "
                                 f"form {multi_keys}")
            if e.get("fg_mask") is None and e.get("fg_masks") is None:
                raise ValueError(f"transform_foregrounds: edit {i} has neither fg_mask nor fg_masks")
            if multi:
                masks, tfs = e.get("fg_masks"), e.get("transforms")
                removed = e.get("removed_masks")
                if removed is not None:
                    removed = check_removed_masks(removed, list(masks) if isinstance(masks, (list, tuple)) else [],
                                                  f"transform_foregrounds: edit {i}: removed_masks")
                if not isinstance(masks, (list, tuple)) or (len(masks) < 1 and not removed and cams[i] is None):
                    raise ValueError(f"transform_foregrounds: edit {i}: fg_masks must be a non-empty list of masks")
                if len(masks) == 0:          # a pure removal or a pure camera move: no transform, no table, no weights
                    if tfs or e.get("instances") or e.get("object_weights") is not None:
                        raise ValueError(f"transform_foregrounds: edit {i} has no foreground mask (a pure removal), but gives "
                                         "transforms, instances or object_weights")
                    continue
                inst = check_instances(e.get("instances"), len(masks), f"transform_foregrounds: edit {i}: instances")
                n_bodies, body = (len(masks), "masks") if inst is None else (len(inst), "instances")
                if tfs is None or len(tfs) != n_bodies:
                    raise ValueError(f"transform_foregrounds: edit {i} has {0 if tfs is None else len(tfs)} transforms for "
                                     f"{n_bodies} {body}")
                for m, tf in enumerate(tfs):
                    check_body(tf, masks[m if inst is None else inst[m]],
                               f"transform_foregrounds: edit {i}, {'object' if inst is None else 'instance'} {m}")
                if e.get("object_weights") is not None and cams[i] is not None:
                    weights[i] = self._camera_weights(f"transform_foregrounds: edit {i}", e["object_weights"], n_bodies)
                elif e.get("object_weights") is not None:
                    from .losses import check_object_weights
                    try:
                        weights[i] = check_object_weights(e["object_weights"], n_bodies)
                    except ValueError as err:
                        raise ValueError(f"transform_foregrounds: edit {i}: {err}") from None
            else:
                check_transform((0.0, None, None, e.get("scale"), e.get("pivot")), f"transform_foregrounds: edit {i}")
        lks = [self._lock_setup(f"transform_foregrounds: edit {i}", e["activations"], e["depth"], e.get("release_mask"))
               for i, e in enumerate(edits)]
        for i, e in enumerate(edits):
            if tuple(e["depth"].shape[-2:]) != tuple(edits[0]["depth"].shape[-2:]):
                raise ValueError(f"transform_foregrounds: edit {i} has another resolution than edit 0 "
                                 f"({tuple(e['depth'].shape[-2:])} / {tuple(edits[0]['depth'].shape[-2:])})")
        unet = self.diffuser.unet
        if unet is not None and (unet.max_batch < 2 * K or unet.max_diff_batch < K):
            raise RuntimeError(f"engine max_batch {unet.max_batch} / max_diff_batch {unet.max_diff_batch} too small for {K} edits: "
                               f"build the diffuser with max_batch >= {2 * K}")
        groups = {}                  # image (and its mask tensors) -> indices of its edits, in input order
        for i, e in enumerate(edits):
            masks = tuple(id(m) for m in e["fg_masks"]) if e.get("fg_masks") is not None else (id(e["fg_mask"]),)
            key = (id(e["depth"]), e.get("fg_masks") is not None) + masks + (id(e["bg_depth"]),) + tuple(id(a) for a in e["activations"])
            if e.get("instances") is not None:          # one instance table per re-projection call
                key += ("instances",) + tuple(int(o) for o in e["instances"])
            if e.get("removed_masks") is not None:      # one list of removed masks per re-projection call
                key += ("removed",) + tuple(id(m) for m in e["removed_masks"])
            groups.setdefault(key, []).append(i)
        reproj, labels, rows, kinds = [None] * K, [None] * K, [None] * K, [None] * K
        with torch.no_grad():
            for idx in groups.values():
                e0 = edits[idx[0]]
                if e0.get("fg_masks") is not None:
                    res = self._reproject_objects("transform_foregrounds", e0["depth"], e0["bg_depth"], list(e0["fg_masks"]),
                                                  [list(edits[i].get("transforms") or []) for i in idx],
                                                  use_input_depth_normalization, True, e0.get("instances"), e0.get("removed_masks"),
                                                  None, [cams[i] for i in idx] if any(cams[i] is not None for i in idx) else None)
                    if any(cams[i] is not None for i in idx):
                        # a camera call: the instance column always; the background's rows carry N.  The weighted edits of the
                        # group read their objects from it (a label image cannot name the background).
                        n_inst = len(e0["instances"]) if e0.get("instances") is not None else len(e0["fg_masks"])
                        for i, r in zip(idx, res):
                            kinds[i] = (r[2] == n_inst).to(torch.uint8) * 2 if cams[i] is not None else None
                            rows[i] = r[2] if weights[i] is not None or e0.get("instances") is not None else None
                            if cams[i] is None and weights[i] is not None and len(weights[i]) != n_inst:
                                raise ValueError(f"transform_foregrounds: edit {i}: object_weights has {len(weights[i])} entries "
                                                 f"for {n_inst} instances")
                        res = [r[:2] for r in res]
                    elif e0.get("instances") is not None:          # the rows' instances stand in for the label image
                        for i, r in zip(idx, res):
                            rows[i] = r[2]
                        res = [r[:2] for r in res]
                    elif any(weights[i] is not None for i in idx):
                        from .losses import object_label_image
                        label = object_label_image(list(e0["fg_masks"]))          # once per group
                        for i in idx:
                            labels[i] = label if weights[i] is not None else None
                else:
                    tfs = [self._fill_transform([edits[i].get(k) for k in ("rot_angle", "rot_axis", "translation", "scale", "pivot")])
                           for i in idx]
                    res = reproject(e0["depth"], e0["bg_depth"], [e0["fg_mask"]],
                                    self.diffuser.get_depth_intrinsics(device=e0["depth"].device), [[tf] for tf in tfs],
                                    use_input_depth_normalization=use_input_depth_normalization, device_correspondences=True, **fp)
                for i, r in zip(idx, res):
                    reproj[i] = r
            self.last_keep_maps = []
            items = [dict(latents=e["init_noise"], depth=d, uncond_embeddings=e["null_text_emb"], prompt=e["prompt"],
                          activations_orig=e["activations"], correspondences=c, object_labels=labels[i], object_weights=weights[i],
                          pair_instances=rows[i], row_kind=kinds[i], **self._vacated(e.get("removed_masks"), "transform_foregrounds"),
                          lock=self._edit_lock(lks[i], list(e["fg_masks"]) + list(e.get("removed_masks") or [])
                                               if e.get("fg_masks") is not None else e["fg_mask"], c, e["depth"]))
                     for i, (e, (d, c)) in enumerate(zip(edits, reproj))]
            imgs = self.diffuser.guided_inference_items(items, [e.get("fg_weight") for e in edits],
                                                        [e.get("bg_weight") for e in edits])
        return imgs, [d for d, _ in reproj]

    def transform_foreground(self, depth, prompt, fg_mask, bg_depth, null_text_emb, init_noise, activations,
                             rot_angle=None, rot_axis=None, translation=None, fg_weight=None, bg_weight=None,
                             use_input_depth_normalization=False, scale=None, pivot=None):
        """The reference's transform_foreground (diffusion_handles.py:113-166), its parameters a prefix.  scale / pivot (not in the
        reference) make the edit a similarity: scale -- None (= 1), one positive float or three (sx, sy, sz) along the camera
        axes of depth_to_world_coords -- multiplies the offsets of the object's points from the pivot BEFORE the rotation (a
        non-uniform scale of a turned object stretches along the un-turned camera axes); pivot -- None (= the centroid of the
        masked points) or a point in those coordinates (depth_transform.pivot_at_pixel) -- is what the object is scaled and
        turned about.  In 'pc' mode a magnified object leaves gaps between its points, bridged only up to the mask CLOSE's
        element (res // 50) -- unless the conf has depth_transform_footprints: true (footprint splatting, point mode only;
        depth_transform_footprint_max_ratio is its optional depth-ratio guard; depth_transform.reproject);
        'mesh' mode takes a pivot and refuses a scale, footprints and a reflecting in-fill border (NotImplementedError; conf
        depth_transform_infill_border: reflect, depth_transform.reproject: both then apply to every edit call and to
        set_foreground).  With conf background_lock: true
        the edit's latents are held to the reconstruction outside its region (DESIGN.md "Background lock"; both modes)."""
        fp = self._reproject_keywords("transform_foreground")
        lk = self._lock_setup("transform_foreground", activations, depth)
        with torch.no_grad():
            geo = dict(depth=depth, bg_depth=bg_depth, fg_mask=fg_mask,
                       intrinsics=self.diffuser.get_depth_intrinsics(device=depth.device),
                       rot_angle=rot_angle, rot_axis=rot_axis, translation=translation,
                       use_input_depth_normalization=use_input_depth_normalization, scale=scale, pivot=pivot)
            border = fp.pop("infill_border")
            if border != "zero":          # ('pc' mode: _footprints refused the others; the named calls keep their lists)
                from .depth_transform import reproject
                tf = self._fill_transform((rot_angle, rot_axis, translation, scale, pivot))
                (edited_disparity, correspondences), = reproject(
                    depth, bg_depth, [fg_mask], geo["intrinsics"], [[tf]],
                    use_input_depth_normalization=use_input_depth_normalization, infill_border=border, **fp)
            elif fp["footprints"]:
                edited_disparity, correspondences = transform_depth_footprints(**geo, **fp)
            else:
                edited_disparity, correspondences = transform_depth(**geo, depth_transform_mode=self.conf.depth_transform_mode)
            self.last_keep_maps = []
            lock = {} if lk is None else dict(lock=self._edit_lock(lk, fg_mask, correspondences, depth))
            results = self.diffuser.guided_inference(
                latents=init_noise, depth=edited_disparity, uncond_embeddings=null_text_emb, prompt=prompt,
                activations_orig=activations, correspondences=correspondences, fg_weight=fg_weight,
                bg_weight=bg_weight, save_denoising_steps=self.conf.guided_diffuser.save_denoising_steps, **lock)
        return self._edit_result(results, edited_disparity)
