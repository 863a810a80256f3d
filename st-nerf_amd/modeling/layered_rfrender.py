"""The layered model with the reference's constructor, attributes and forward signature
(modeling/layered_rfrender.py:19-741).

Everything numeric runs in the HIP library through ``stnerf_amd.ops`` (ONE call into the C ABI per launch
sequence, ``stnerf_render_rays``); this file only does what the reference does on the host: config, per-frame box
interpolation/edit on l x 8 x 3 numbers, chunk bookkeeping and output packing.
"""
from __future__ import annotations

import hashlib
import math
from typing import Optional

import torch
from torch import nn

from stnerf_amd import ops
from stnerf_amd.modeling.motion_net import MotionNet
from stnerf_amd.modeling.spacenet import SpaceNet

Tensor = torch.Tensor


def _alpha_acts(model):
    """``alpha`` acts on layer 2 of the fine composite: there is such a layer and the factor is not 1."""
    return model.total_layers > 2 and float(model.alpha) != 1.0


class LayeredRFRender(nn.Module):
    """modeling/layered_rfrender.py:19-741 -- same constructor, attributes and forward signature."""

    def __init__(self, cfg, camera_num, scale=None, shift=None):
        super().__init__()
        M = cfg.MODEL
        if M.SAMPLE_METHOD != "BBOX":
            raise NotImplementedError("only SAMPLE_METHOD 'BBOX' is on the render path (both shipped ymls)")
        unsupported = dict(POSE_REFINEMENT=M.POSE_REFINEMENT, USE_DEFORM_VIEW=M.USE_DEFORM_VIEW)
        bad = [k for k, v in unsupported.items() if v]
        if bad:
            raise NotImplementedError(f"config flags outside the MI355X hot path (training-time features): {bad}")
        if M.BKGD_USE_SPACE_TIME and not M.USE_SPACE_TIME:
            raise ValueError("BKGD_USE_SPACE_TIME needs USE_SPACE_TIME: the reference hands the background SpaceNet "
                             "its frame id only then (layered_rfrender.py:382-390) and fails on the missing input")
        if not (M.USE_DEFORM_TIME or M.USE_SPACE_TIME):
            raise ValueError("one of USE_DEFORM_TIME / USE_SPACE_TIME must be on (the reference dereferences a "
                             "missing frame id otherwise, layered_rfrender.py:193)")
        layer_num = cfg.DATASETS.LAYER_NUM
        self.coarse_ray_sample, self.fine_ray_sample = M.COARSE_RAY_SAMPLING, M.FINE_RAY_SAMPLING
        self.sample_method = M.SAMPLE_METHOD
        self.boarder_weight = M.BOARDER_WEIGHT
        self.scale, self.shift = scale, shift
        self.rotation = None               # per layer None | angle | R (3,3) | (angle | R, centre): layer_ray_transforms (not in the
                                           # reference, whose renderer stores `rotation` and never reads it)
        self.near, self.alpha = 0, 1
        self.layer_alpha = None            # None: `alpha` on layer 2, as the reference; else one density factor per layer of
                                           # total_layers (None = 1.0) for the fine composite (stnerf_render_rays_opacity) --
                                           # what lets a layer instance be a ghost.  Needs alpha == 1 (not in the reference)
        self._instances = []               # add_instance: the source performer (1..layer_num) of layer layer_num + 1 + j
        self.pose_refinement = False
        self.layer_num, self.camera_num = layer_num, camera_num
        self.use_deform_view, self.bkgd_use_deform_time = False, bool(M.BKGD_USE_DEFORM_TIME)
        self.use_deform_time, self.use_space_time = M.USE_DEFORM_TIME, M.USE_SPACE_TIME
        self.bkgd_use_space_time = bool(M.BKGD_USE_SPACE_TIME)

        self.deep_rgb = deep = bool(M.DEEP_RGB and M.USE_SPACE_TIME)      # :35
        inc, use_dir = bool(M.TKERNEL_INC_RAW), bool(M.USE_DIR)          # :27-29
        common = dict(include_input=inc, use_dir=use_dir, deep_rgb=deep)
        self.bkgd_spacenet = SpaceNet(use_time=self.bkgd_use_space_time, **common)
        self.bkgd_spacenet_fine = SpaceNet(use_time=self.bkgd_use_space_time, **common)
        self.spacenets, self.spacenets_fine = nn.ModuleList([]), nn.ModuleList([])
        for i in range(layer_num):
            self.spacenets.append(SpaceNet(use_time=self.use_space_time, **common))
            self.spacenets_fine.append(self.spacenets[i] if M.SAME_SPACENET
                                       else SpaceNet(use_time=self.use_space_time, **common))
        self.time_deform_nets = nn.ModuleList([])
        if self.use_deform_time:
            for i in range(layer_num):
                self.time_deform_nets.append(MotionNet(c_input=4, include_input=inc, input_time=True))
        if self.bkgd_use_deform_time:                                  # :92-93 (input_time stays False)
            self.bkgd_time_deform_net = MotionNet(c_input=4, include_input=inc)
        # the reference initialises the fine / other-layer nets as deep copies (:63-74); keep that for a
        # freshly built model (a loaded checkpoint overwrites everything anyway)
        self.bkgd_spacenet_fine.load_state_dict(self.bkgd_spacenet.state_dict())
        for i in range(layer_num):
            self.spacenets[i].load_state_dict(self.spacenets[0].state_dict())
            self.spacenets_fine[i].load_state_dict(self.spacenets[i].state_dict())
        self.maxs = self.mins = None
        self.display_layers = {i: 1 for i in range(layer_num + 1)}
        self.bkgd_bbox = None
        self.bboxes = None
        # MI355X-side knobs (not in the reference)
        self.seed = 0                      # Philox seed of the on-device jitter / resampling draws
        self.fresh_draws_per_call = type(self).FRESH_DRAWS_DEFAULT  # True: every forward() advances `seed` (the reference draws fresh torch.rand
                                           # numbers per call, layers/RaySamplePoint.py:98, utils/sample_pdf.py:31);
                                           # False: a call is a pure function of (rays, weights, seed) -- what the
                                           # sharded / chunked renders and the tests rely on.  dropin.patch_reference
                                           # switches it on for models built through the reference's own code
        self.max_rays_per_launch = 1 << 19 # rays per kernel sequence (workspace bound ~20 KB/ray, not a semantic chunk)
        self.replay = None                 # {"jitter": (l,N,N1), "u": (l,N,N2)} to replay recorded uniforms (parity tests); the training path
                                           # also takes "z" (l,N,N2) / "xyz_c" / "xyz_f": the reference's own fine depths and deformed
                                           # points (teacher forcing, stnerf_amd.modeling.training.render_rays_train)
        self.mlp_schedule = "stage"        # "stage": one persistent MLP launch per stage (stnerf_mlp_stage); "per_net":
                                           # one launch per (layer, network) through the op-level entries (A/B measurements)
        self.ray_window = (0, 0, 0)        # (first, stripe, period): which rays of the view `rays` are (include/stnerf.h);
                                           # keeps the RNG stream of a view under multi-GPU sharding
        self.shard_views = type(self).SHARD_VIEWS_DEFAULT
                                           # OPT-IN (default False): with an initialised torch.distributed group of > 1 ranks,
                                           # layered_batchify_ray / render_pose cut the view into interleaved stripes over the ranks
                                           # and all-gather the outputs -- a COLLECTIVE call every rank must make with the same
                                           # rays (stnerf_amd.parallel).  The `python -m stnerf_amd.dropin` launcher under
                                           # torch.distributed.run and bench.py switch it on
        self.gather = "all"                # what a sharded call all-gathers: "all" (the whole 5-tuple), "fine" (what render_pose
                                           # consumes: mixed + per-layer fine images, masks), "final" (the two mixed images);
                                           # entries that are not gathered come back as None
        self.shard_group = None            # the process group to shard over (None: the default group)
        self._bkgd_cache = None            # stnerf_amd.BackgroundCache or None (set_background_cache)
        self._layer_cache = None           # stnerf_amd.LayerCache or None (set_layer_cache)
        self._occupancy = None             # stnerf_amd.OccupancyGrids or None (set_occupancy)
        self._termination = None           # stnerf_amd.termination.Termination or None (set_termination)
        self._proposal = None              # stnerf_amd.ProposalGrids or None (set_proposal)
        self.view_key = None               # (view identity, background frame id) of the rays in flight (stnerf_amd.bkgd_cache.view_key),
                                           # set and restored around a call by whoever generated the rays from a camera
                                           # (stnerf_amd.parallel.render_view / render_view_share); None: rays of unknown origin,
                                           # never cached
        self.view_frame_ids = None         # the host frame ids those rays were generated with (a tuple of floats, one per frame-id
                                           # column), set and restored beside view_key: where the layer cache reads a layer's
                                           # frame id from (stnerf_amd.bkgd_cache.view_frame_ids)

    FRESH_DRAWS_DEFAULT = False   # what a new model's fresh_draws_per_call starts as (dropin.patch_reference: True)
    SHARD_VIEWS_DEFAULT = False   # what a new model's shard_views starts as (the dropin launcher under torch.distributed.run: True)

    # ---- layer instances (not in the reference: its advertised "duplication" edit) ---------------------
    @property
    def instances(self):
        """The source performer of every instance, in layer order: layer ``layer_num + 1 + j`` borrows the networks and the
        box column of performer ``instances[j]``."""
        return tuple(self._instances)

    @property
    def total_layers(self):
        """l: the background, the performers and the instances -- what the render path counts layers with."""
        return self.layer_num + 1 + len(self._instances)

    def add_instance(self, src):
        """Show performer ``src`` (1..layer_num) a second time -> the new layer's id.  The instance borrows the source's networks
        (the packed blobs themselves: no parameter, no second pack, no device copy) and its box column, and owns everything
        else a layer has: its frame-id column of the rays, its ``scale`` / ``shift`` / ``rotation`` / ``layer_alpha`` entry and its
        shown flag.  The model then renders what the WIDE model renders (LAYER_NUM + 1, the modules and
        the box column copied), bit for bit; the RNG is keyed by the layer index, so the instance draws its own jitter.
        Inference only."""
        from stnerf_amd import hip
        if isinstance(src, bool) or not isinstance(src, int) or not 1 <= src <= self.layer_num:
            raise ValueError(f"add_instance: the source must be a performer 1..{self.layer_num} (not the background, not an "
                             f"instance), got {src!r}")
        if self.total_layers + 1 > hip.MAX_LAYERS:
            raise ValueError(f"add_instance: {self.total_layers + 1} layers exceed STNERF_MAX_LAYERS = {hip.MAX_LAYERS}")
        self._instances.append(src)
        layer_id = self.total_layers - 1
        self.display_layers[layer_id] = 1
        return layer_id

    def clear_instances(self):
        """Drop every instance (the per-layer lists -- scale, shift, rotation, layer_alpha -- are the caller's to shorten)."""
        for i in range(self.layer_num + 1, self.total_layers):
            self.display_layers.pop(i, None)
        self._instances = []

    def _module_index(self, layer_id):
        """Index into spacenets / spacenets_fine / time_deform_nets of layer ``layer_id`` >= 1: its own, or its source's."""
        return (layer_id if layer_id <= self.layer_num else self._instances[layer_id - self.layer_num - 1]) - 1

    def _box_table(self):
        """``bboxes`` (frames, l - 1, 8, 3) with the instances' columns appended, each a copy of its source's: everything
        downstream of it (the pivot, the edits, retiming, the rotations' default centres) sees l layers."""
        if not self._instances:
            return self.bboxes
        return torch.cat([self.bboxes, self.bboxes[:, [s - 1 for s in self._instances]]], 1)

    def _box_table_host(self):
        """``_box_table()`` as fp32 on the host, copied once per state of ``bboxes`` and of the instances: ``layer_box_at`` runs
        per culled layer and launch piece, and a copy from the device there would make the host wait for the piece before."""
        bb = self.bboxes
        key = (bb.data_ptr(), bb._version, bb.device, tuple(bb.shape), tuple(self._instances))
        held = getattr(self, "_box_host", None)
        if held is None or held[0] != key:
            held = self._box_host = (key, self._box_table().detach().to("cpu", torch.float32).clone())
        return held[1]

    def _layer_alpha_table(self):
        """None (``layer_alpha`` unset: ``alpha`` acts, on layer 2) or l floats for stnerf_render_rays_opacity."""
        if self.layer_alpha is None:
            return None
        l = self.total_layers
        if len(self.layer_alpha) != l:
            raise ValueError(f"layer_alpha must have one entry per layer ({l}, layer 0 = the background), got {len(self.layer_alpha)}")
        if float(self.alpha) != 1.0:
            raise ValueError(f"layer_alpha together with alpha = {self.alpha}: alpha is layer 2's entry of the table -- set it there "
                             "and leave model.alpha at 1")
        return [1.0 if a is None else float(a) for a in self.layer_alpha]

    def _inference_only_edits(self):
        """What the op-by-op path (training, mixed background frame ids) does not implement, or None."""
        if self._instances:
            return "layer instances (add_instance)"
        if self.layer_alpha is not None:
            return "layer_alpha"
        if getattr(self, "_occupancy", None) is not None:
            return "occupancy grids (set_occupancy)"
        if getattr(self, "_termination", None) is not None:
            return "early ray termination (set_termination)"
        if getattr(self, "_proposal", None) is not None:
            return "grid proposals (set_proposal)"
        return None

    def set_precision(self, precision: str):
        """"bf16x3" (the default: three bf16 pieces per fp32 operand, six MFMAs per product, two accumulators: fp32's
        significand and range, closer to an fp64 evaluation than an fp32 fma chain, 1.5 x the speed) or "fp32" (exact f32
        MFMA, v_mfma_f32_32x32x2_f32)."""
        if precision not in ops.PRECISIONS:
            raise ValueError(f"precision must be one of {ops.PRECISIONS}")
        for m in self.modules():
            if isinstance(m, (SpaceNet, MotionNet)):
                m.precision = precision
        return self

    def set_background_cache(self, cache):
        """Attach a ``stnerf_amd.BackgroundCache`` (None: detach).  While one is attached, frames of a view whose camera the
        caller names (``view_key``: ``stnerf_amd.parallel.render_view`` / ``render_view_share``, so ``render_pose`` and the
        renderer's ``render_path``) evaluate the background networks once and later take their raw outputs from the cache as long
        as ``background_cache_key`` stays the same -- bit-identical frames, about half the network work on a two-performer scene.
        Calls with caller-made rays (``forward``, ``render_rays``), ``replay``, the training path and the per-sample background
        time path are never cached.

        While a cache is attached ``advance_seed()`` is a no-op: a cached run uses ONE jitter pattern for all its frames, also
        with ``fresh_draws_per_call`` (what ``dropin.patch_reference`` switches on) -- fresh draws per frame would change every
        background sample and nothing could be reused.  Detaching restores the per-call advance."""
        self._bkgd_cache = cache
        return self

    def set_layer_cache(self, cache):
        """Attach a ``stnerf_amd.LayerCache`` (None: detach).  While one is attached, frames of a view whose camera the caller
        names (``view_key`` / ``view_frame_ids``: ``stnerf_amd.parallel.render_view`` / ``render_view_share``, tagged rays) keep
        every shown performer's and instance's raw network outputs on the device, compact over the layer's hit rays, and copy
        them in instead of evaluating the layer for as long as ``layer_cache_key`` of that layer stays the same: nudging,
        retiming, rotating, fading or hiding ANOTHER layer, any ``layer_alpha``, ``bkgd_density_threshold``.  (With retiming
        ``density_threshold`` is an input of a performer's fine samples and so part of its key: a sweep over it re-evaluates the
        performers.)  Bit-identical frames.
        A key is captured at its second sighting and reused from its third, so a performer that moves every frame costs nothing.
        A cached performer is not terminated (``set_termination``): its outputs would depend on the other layers.  Calls with
        caller-made rays, ``replay``, the training path and the per-sample background time path are never cached.  Both caches may
        be attached at once.  While either is attached ``advance_seed()`` is a no-op (one jitter pattern for a cached run).
        While a layer cache is attached and the view is known, NO shown performer is terminated -- also one that moves every frame
        and is never captured --, so that all frames of a run agree; the background's termination stays."""
        self._layer_cache = cache
        return self

    def _edited_layer_key(self, i, box, pivot):
        """What the two cache keys hold of layer ``i``'s edits, as hashable host values: its EDITED box (``box``: the unedited one, a
        host copy this may change), its coarse and its fine point un-edit, the pivot they use and its (m, c) ray transform with the
        default centre it would get (the edited box's) -> (box bytes, coarse edit, fine edit, pivot tuple | None, rot | None)."""
        if self.scale is not None and pivot is None:
            pivot = self._pivot()
        if self.scale is not None and i < len(self.scale):
            box = (box - pivot) * self.scale[i] + pivot
        if self.shift is not None and i < len(self.shift) and self.shift[i] is not None:
            box = box + torch.tensor(self.shift[i], dtype=torch.float32)
        rot = None
        if self.rotation is not None:
            sp = self._rotation_specs()
            if sp is not None and sp[i] is not None:
                m = sp[i][0].T.contiguous()
                c = sp[i][1] if sp[i][1] is not None else torch.mean(box, 0)
                rot = (m.numpy().tobytes(), c.numpy().tobytes())
        def edit(fine):
            e = self._point_edits(self.total_layers, fine)
            if e is None:
                return None
            sh, sc = e[i]
            return (None if sh is None else tuple(float(x) for x in sh), None if sc is None else float(sc))
        return box.numpy().tobytes(), edit(False), edit(True), None if pivot is None else tuple(float(x) for x in pivot.tolist()), rot

    def layer_cache_key(self, i, view_key, piece, window, retiming, only_coarse, pivot=None, frame_ids=None, density_threshold=None):
        """(group, piece): the key of performer / instance ``i``'s raw outputs of a launch piece -- host arithmetic only (the box
        table's host copy is made once per tensor version, ``_box_table_host``).  The group reads every item of
        ``background_cache_key`` for layer i: the layer, the view (camera, h, w), the seed, n1 / n2 / only_coarse, the arithmetic
        and its schedule, the retiming flag and the ray width, the layer's EDITED box at its frame id, its coarse and fine point
        un-edit with the pivot they use, its (m, c) ray transform with the default centre it would get, near and border, the
        performer model flags, the parameter versions of spacenets / spacenets_fine / time_deform_nets at ``_module_index(i)``,
        the layer's frame id (always: its networks take it) and, while occupancy grids are attached, the layer's grid identity
        and the sample flag.  ``frame_ids``: the host values the view was generated with (default ``view_frame_ids``).
        ``density_threshold``: the render call's, in the group -- and required -- only with retiming and a fine stage: there the
        COARSE composite zeroes a performer's densities below it before it writes the layer's weights (layered_rfrender.py:416-418),
        the resampler draws the layer's fine depths from those weights, so the layer's fine points and fine raw outputs follow the
        threshold (the coarse ones do not; width-7 rays apply no threshold).  Deliberately absent: everything about other layers,
        ``display_layers``, ``alpha`` / ``layer_alpha``, ``bkgd_density_threshold`` (they act on other layers or in the fine
        composite, after the networks) and the termination settings (a cached layer is not terminated)."""
        from stnerf_amd.modeling._packed import _params_fingerprint
        l = self.total_layers
        if isinstance(i, bool) or not isinstance(i, int) or not 1 <= i < l:
            raise ValueError(f"layer_cache_key: layer {i!r} is not a performer or an instance (1..{l - 1}); the background has its own cache")
        frame_ids = self.view_frame_ids if frame_ids is None else frame_ids
        want = l if retiming else 1
        if frame_ids is None or len(frame_ids) != want:
            raise ValueError(f"layer_cache_key: the view's frame ids must be {want} host values, got {frame_ids!r}")
        fid = float(frame_ids[i] if retiming else frame_ids[0])
        thr = None
        if retiming and not only_coarse:
            if density_threshold is None:
                raise ValueError("layer_cache_key: with retiming and a fine stage the layer's fine samples depend on density_threshold; pass it")
            thr = float(density_threshold)
        view = view_key[0]
        box, edit_c, edit_f, pivot, rot = self._edited_layer_key(i, self.layer_box_at(i, fid, retiming).clone(), pivot)
        j = self._module_index(i)
        nets = [self.spacenets[j], self.spacenets_fine[j]] + ([self.time_deform_nets[j]] if self.use_deform_time else [])
        prec = self.bkgd_spacenet.precision
        grid = None
        grids = getattr(self, "_occupancy", None)
        if grids is not None:
            # a built grid: what it is made of beyond this key (res / threshold / dilate; box, frame id, flags and parameter
            # versions are above); a manual one: the digest of its words and bounds
            if i in grids._manual:
                words, res, lo, hi = grids._manual[i][:4]
                grid = ("manual", res, lo.tobytes(), hi.tobytes(), hashlib.sha256(words.tobytes()).digest()[:8])
            elif grids.auto:
                grid = ("built", grids.res, grids.threshold, grids.dilate)
            grid = None if grid is None else grid + (bool(grids.samples),)
        group = ("layer", int(i), view, int(self.seed) & 0xFFFFFFFFFFFFFFFF, int(self.coarse_ray_sample), int(self.fine_ray_sample),
                 bool(only_coarse), prec, self.mlp_schedule if prec != "bf16x3" else "stage", bool(retiming), 6 + want,
                 box, edit_c, edit_f, pivot,
                 float(self.near), float(self.boarder_weight), (bool(self.use_deform_time), bool(self.use_space_time), bool(self.deep_rgb)),
                 j, tuple(_params_fingerprint(m) for m in nets), fid, rot, grid, thr)
        return group, (int(piece[0]), int(piece[1]), tuple(int(x) for x in window))

    # ---- occupancy grids (not in the reference beyond utils/vis_density.py) ---------------------------------
    def set_occupancy(self, grids):
        """Attach a ``stnerf_amd.OccupancyGrids`` (None: detach).  While one is attached every launch culls the (ray, performer)
        pairs none of whose coarse sample points lies in an occupied cell of the performer's grid, before
        any network runs; the grids are built from the networks' own densities on first use (``density_grid``) or given by the
        caller (``OccupancyGrids.set_manual``).  A culled layer needs ONE frame id per chunk group.  Inference only; the
        background cache's key is unchanged, since grids act on performers.  ``OccupancyGrids(samples=True)`` also skips the
        samples of a kept ray whose point lies in an empty cell, in both network stages (their outputs are exact zeros).
        ``OccupancyGrids(background=True)`` (or a manual background grid) sample-culls the background too, on every ray, with a
        grid over the unedited ``bkgd_bbox``; then -- and only then -- the background cache's key gains the grid's identity, so a
        cache never serves un-culled outputs to a culled render or the reverse.  Under BKGD_USE_DEFORM_TIME / BKGD_USE_SPACE_TIME a
        culled background needs ONE background frame id per chunk group."""
        self._occupancy = grids
        return self

    # ---- grid proposals (not in the reference) ------------------------------------------------------------------
    def set_proposal(self, grids):
        """Attach a ``stnerf_amd.ProposalGrids`` (None: detach).  While one is attached a flagged layer's COARSE densities are a
        trilinear lookup in a grid of the layer's own fine densities (include/stnerf.h states the rule): its
        coarse SpaceNet and MotionNet do not run, and everything downstream -- the coarse composite, termination, the resampler,
        the fine stage -- is fed with those densities.  The grids are built on first use (``density_grid(..., fine=True)``) or given
        by the caller (``ProposalGrids.set_manual``).  A flagged layer needs ONE frame id per chunk group.  An approximation: the
        fine depths are drawn from other weights, so the frame differs from the exact one as a frame of another seed does;
        ``layer_coarse`` / ``mixed_coarse`` of a flagged layer carry zero colour and the grid's depth and alpha.  Inference only, one
        rank, the "stage" schedule; not beside a layer cache (performers flagged) or a background cache (the background flagged),
        and the background is not flagged beside a background grid or a per-ray background mask."""
        self._proposal = grids
        return self

    @property
    def proposal(self):
        """The attached ``stnerf_amd.ProposalGrids`` or None."""
        return getattr(self, "_proposal", None)

    def _check_proposal(self, flagged, background_rays):
        """The refusals of a render with grid proposals on the layers ``flagged``, before anything is launched."""
        from stnerf_amd import parallel
        window, self.ray_window = self.ray_window, (0, 0, 0)   # (inside a sharded call the rank's window is set: ask without it)
        try:
            sharded = parallel.active_group(self) is not None
        finally:
            self.ray_window = window
        if sharded:
            raise RuntimeError("grid proposals under shard_views with more than one rank: the cross-rank check does not cover the grids; "
                               "render on one rank (model.shard_views = False) or set_proposal(None)")
        if self.mlp_schedule != "stage" and self.bkgd_spacenet.precision != "bf16x3":
            raise ValueError("grid proposals with mlp_schedule = 'per_net' (one launch per network): that schedule does not store activated "
                             "colours; use mlp_schedule = 'stage' or set_proposal(None)")
        if any(i > 0 for i in flagged) and getattr(self, "_layer_cache", None) is not None:
            raise ValueError("grid proposals on a performer beside a layer cache: a cached layer's coarse slice would be the grid's; "
                             "set_layer_cache(None) or set_proposal(None)")
        if 0 in flagged:
            if getattr(self, "_bkgd_cache", None) is not None:
                raise ValueError("a grid proposal on the background beside a background cache: the cached coarse slice would be the grid's; "
                                 "set_background_cache(None) or ProposalGrids(background=False)")
            occ = getattr(self, "_occupancy", None)
            if occ is not None and occ.has_background():
                raise ValueError("a grid proposal on the background beside a background occupancy grid: the coarse rows launch that stores "
                                 "the grid's zeros is gone (out of scope); drop one of the two")
            if background_rays is not None:
                raise ValueError("a grid proposal on the background beside a per-ray background mask: the coarse rows launch that stores "
                                 "the mask's zeros is gone (out of scope); drop one of the two")

    def _proposal_frame_ids(self, rays, groups, retiming, flagged):
        """Per chunk group the frame id of every layer (l floats), after checking that each FLAGGED layer's frame-id column is constant
        within the group (the background's only where its flags make the id an input of its density): the rule of
        ``_occupancy_frame_ids``.  A grid made at row 0's id applied to rays of another id would propose wrongly and silently."""
        l = self.total_layers
        cols = (lambda a, b: rays[a:b, 6:6 + l]) if retiming else (lambda a, b: rays[a:b, 6:7].expand(b - a, l))
        mm, mixed = self._frame_id_ranges(groups, cols)
        out = []
        for k, g in enumerate(groups):
            for i in flagged:
                if i == 0 and not self._proposal.background_timed(self):
                    continue
                if mixed(mm[k, 0, i], mm[k, 1, i]):
                    raise ValueError(f"proposal: layer {i} has frame ids {float(mm[k, 0, i])} .. {float(mm[k, 1, i])} among rays {g[0]}..{g[1]} of "
                                     "one chunk group; a flagged layer needs one frame id per group (its grid is made at that id) -- "
                                     "render one frame id per chunk group, or detach the grids (set_proposal(None))")
            out.append([float(x) for x in mm[k, 0]])
        return out

    # ---- early ray termination (not in the reference) ---------------------------------------------------------
    def set_termination(self, tau=1e-4, layers=None, background=True):
        """Skip the fine samples the coarse pass shows are hidden (``stnerf_amd.termination``): once the
        coarse composite's merged transmittance along a ray has fallen to ``tau`` (fp32 in [0, 1)), the fine samples behind
        that depth get exact zero outputs and no network evaluation.  ``layers``: the performer / instance layers to terminate
        (None: every shown one); ``background``: layer 0 too (left alone while a background cache captures or serves it).
        ``tau=None``, or a ``Termination`` in its place, detaches / attaches one.  The fine stage only; inference only; needs
        ``alpha == 1`` and no ``layer_alpha`` entry other than 1 (the coarse pass ignores both) and the "stage" schedule."""
        from stnerf_amd.termination import Termination
        if tau is None or isinstance(tau, Termination):
            self._termination = tau
        else:
            self._termination = Termination(tau, layers, background)
        return self

    @property
    def termination(self):
        """The attached ``stnerf_amd.termination.Termination`` (tau, layers, background, ``stats()``) or None."""
        return getattr(self, "_termination", None)

    def layer_box_at(self, layer_id, frame_id, retiming=True):
        """The UNEDITED box (8,3), fp32 on the host, of layer ``layer_id`` >= 1 at ``frame_id``: the box table's column of the
        layer (an instance: its source's), lerped for a fractional id exactly as ``_retimed_boxes`` lerps it; ``retiming=False``:
        the row rays 7 wide select (``int(frame_id) - 1``)."""
        if not 1 <= layer_id < self.total_layers:
            raise ValueError(f"layer_box_at: layer {layer_id!r} is not a performer or an instance (1..{self.total_layers - 1})")
        bb = self._box_table_host()
        if not retiming:
            return bb[int(torch.tensor(float(frame_id), dtype=torch.float32).to(torch.int64)) - 1, layer_id - 1].clone()
        f = torch.tensor(float(frame_id), dtype=torch.float32) - 1
        return torch.lerp(bb[math.floor(f), layer_id - 1], bb[math.ceil(f), layer_id - 1], f - math.floor(f))

    def density_grid(self, layer_id, frame_id, res=64, fine=True, direction=(0.0, 0.0, 1.0), retiming=True):
        """-> (sigma (Rz+1, Ry+1, Rx+1) on the device, lo, hi): the density of layer ``layer_id``'s coarse (``fine=False``) or fine
        SpaceNet at the vertices of a grid of ``res`` cells (a number or (Rx, Ry, Rz)) over the axis-aligned bounds of the layer's
        unedited box at ``frame_id`` (``layer_box_at``).  Vertex j of axis a lies at lo_a + j ((hi_a - lo_a) / R_a) in fp32, vertex
        R_a at hi_a.  The points go through the layer's MotionNet at the frame id under USE_DEFORM_TIME and the time goes to the
        SpaceNet under USE_SPACE_TIME: what a render does to a sample point at that place, through the op-level entries on the
        "fp32" packs, so the grid does not depend on the render's arithmetic.  One grid row along x is a "ray" of Rx + 1
        samples; ``direction`` is any unit vector -- the density head does not see it.  The layered, time-aware counterpart of
        the reference's utils/vis_density.py.  Layer 0 (the background over ``bkgd_bbox``) is for inspection only."""
        from stnerf_amd import occupancy as occ
        rx, ry, rz = occ.normalise_res(res)
        if not 0 <= layer_id < self.total_layers:
            raise ValueError(f"density_grid: no layer {layer_id!r} (0..{self.total_layers - 1})")
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("density_grid evaluates the networks on the GPU: call .cuda() first (no CPU fallback)")
        lo, hi = occ.box_bounds(self.bkgd_bbox if layer_id == 0 else self.layer_box_at(layer_id, frame_id, retiming))
        vx, vy, vz = (torch.from_numpy(v) for v in occ.vertex_coordinates((rx, ry, rz), lo, hi))
        pts = torch.stack([vx.view(1, 1, -1).expand(rz + 1, ry + 1, rx + 1), vy.view(1, -1, 1).expand(rz + 1, ry + 1, rx + 1),
                           vz.view(-1, 1, 1).expand(rz + 1, ry + 1, rx + 1)], -1)
        rows = (rz + 1) * (ry + 1)
        xyz = pts.reshape(rows, rx + 1, 3).contiguous().to(dev)
        times = torch.full((rows,), float(frame_id), dtype=torch.float32, device=dev)
        dirs = torch.tensor([float(x) for x in direction], dtype=torch.float32, device=dev).reshape(1, 3).repeat(rows, 1)
        raw = torch.empty(rows, rx + 1, 4, dtype=torch.float32, device=dev)
        bk, nets = self._nets(fine)
        if layer_id == 0:
            if self.bkgd_use_deform_time:
                ops.motionnet_fwd(self.bkgd_time_deform_net._packed("fp32"), xyz, times, add_to_xyz=True, plain_time=True)
            ops.spacenet_fwd(bk._packed("fp32"), xyz, dirs, times if (self.bkgd_use_space_time and self.use_space_time) else None, raw)
        else:
            j = self._module_index(layer_id)
            if self.use_deform_time:
                ops.motionnet_fwd(self.time_deform_nets[j]._packed("fp32"), xyz, times, add_to_xyz=True)
            ops.spacenet_fwd(nets[j]._packed("fp32"), xyz, dirs, times if self.use_space_time else None, raw)
        return raw[..., 3].reshape(rz + 1, ry + 1, rx + 1).contiguous(), lo, hi

    @staticmethod
    def _frame_id_ranges(groups, cols):
        """(min, max) of the frame-id columns ``cols(start, end)`` within every chunk group, on the host (a min / max on the device
        and one device-to-host copy), and the test both callers apply to a pair: the ids differ, or are NaN."""
        mm = torch.stack([torch.stack([cols(g[0], g[1]).amin(0), cols(g[0], g[1]).amax(0)]) for g in groups]).cpu()
        return mm, lambda lo, hi: float(lo) != float(hi) or lo != lo

    def _occupancy_frame_ids(self, rays, groups, retiming):
        """Per chunk group the frame id of every layer (l floats), after checking that each CULLED layer's frame-id column is
        constant within the group: a min / max on the device and one device-to-host copy.  A grid at row 0's id applied to rays
        of another id would cull wrongly and silently."""
        l = self.total_layers
        culled = self._occupancy.culled_layers(self)
        cols = (lambda a, b: rays[a:b, 6:6 + l]) if retiming else (lambda a, b: rays[a:b, 6:7].expand(b - a, l))
        mm, mixed = self._frame_id_ranges(groups, cols)
        out = []
        for k, g in enumerate(groups):
            for i in culled:
                if mixed(mm[k, 0, i], mm[k, 1, i]):
                    raise ValueError(f"occupancy: layer {i} has frame ids {float(mm[k, 0, i])} .. {float(mm[k, 1, i])} among rays {g[0]}..{g[1]} of "
                                     "one chunk group; a culled layer needs one frame id per group (its grid is made at that id) -- "
                                     "render one frame id per chunk group, or detach the grids (set_occupancy(None))")
            out.append([float(x) for x in mm[k, 0]])
        return out

    def _background_frame_ids(self, rays, groups):
        """Per chunk group the background's frame id (column 6), for its occupancy grid; where the background flags make the id an
        input of the density it must be constant within the group (the min / max check of ``_occupancy_frame_ids``): a grid made
        at row 0's id applied to rays of another id would cull wrongly and silently."""
        mm, mixed = self._frame_id_ranges(groups, lambda a, b: rays[a:b, 6])
        if self._occupancy.background_timed(self):
            for k, g in enumerate(groups):
                if mixed(mm[k, 0], mm[k, 1]):
                    raise ValueError(f"occupancy: the background has frame ids {float(mm[k, 0])} .. {float(mm[k, 1])} among rays {g[0]}..{g[1]} of "
                                     "one chunk group; under BKGD_USE_DEFORM_TIME / BKGD_USE_SPACE_TIME its grid is made at one id -- "
                                     "render one background frame id per chunk group, or drop the background's grid")
        return [float(mm[k, 0]) for k in range(len(groups))]

    def background_cache_key(self, view_key, piece, window, retiming, only_coarse, pivot=None):
        """(group, piece): the key of a launch piece's background outputs -- host arithmetic only.  The group covers every input
        of layer 0's raw outputs: the view (camera, h, w), the seed, n1 / n2 / only_coarse, the arithmetic and its schedule, the
        ray format, the EDITED background box and layer 0's point un-edit (coarse and fine, with the pivot they use), near and
        border, the background model flags, the parameter versions of the background networks and -- only where
        BKGD_USE_DEFORM_TIME / BKGD_USE_SPACE_TIME make it an input -- the background's frame id.  The piece part is the ray
        range and its ray window.  Deliberately absent: performer frame ids, boxes, edits and shown flags, alpha and the two
        density thresholds -- they act on other layers or after the networks, and a sweep over them must hit.  Of ``rotation`` the
        group holds layer 0's (m, c) alone: a sweep over the performers' rotations hits.  While the attached occupancy grids cull
        the background (and only then) the group ends with the grid's identity: res / threshold / dilate of a built grid, the
        digest of a manual one -- the cached outputs are the culled ones."""
        from stnerf_amd.modeling._packed import _params_fingerprint
        view, bkgd_frame = view_key
        timed = self.bkgd_use_deform_time or (self.bkgd_use_space_time and self.use_space_time)
        bk = self.bkgd_bbox
        host = getattr(self, "_bkgd_bbox_host", None)          # (one D2H per box version, not per frame)
        if host is None or host[0] is not bk or host[1] != bk._version:
            host = self._bkgd_bbox_host = (bk, bk._version, bk.detach().cpu().float().clone())
        box0, edit_c, edit_f, pivot, rot0 = self._edited_layer_key(0, host[2].clone(), pivot)
        nets = [self.bkgd_spacenet, self.bkgd_spacenet_fine] + ([self.bkgd_time_deform_net] if self.bkgd_use_deform_time else [])
        prec = self.bkgd_spacenet.precision
        group = (view, int(self.seed) & 0xFFFFFFFFFFFFFFFF, int(self.coarse_ray_sample), int(self.fine_ray_sample), bool(only_coarse),
                 prec, self.mlp_schedule if prec != "bf16x3" else "stage", bool(retiming), box0, edit_c, edit_f,
                 pivot, float(self.near), float(self.boarder_weight),
                 (bool(self.bkgd_use_deform_time), bool(self.bkgd_use_space_time), bool(self.use_space_time), bool(self.deep_rgb)),
                 tuple(_params_fingerprint(m) for m in nets), bkgd_frame if timed else None, rot0)
        grids = getattr(self, "_occupancy", None)
        ident = grids.background_identity() if grids is not None else None
        if ident is not None:
            group = group + (ident,)
        return group, (int(piece[0]), int(piece[1]), tuple(int(x) for x in window))

    # ---- reference API -----------------------------------------------------------------------
    def hide_layer(self, layer_id):
        self.display_layers[layer_id] = 0

    def show_layer(self, layer_id):
        self.display_layers[layer_id] = 1

    def is_shown_layer(self, layer_id):
        return self.display_layers[layer_id] == 1

    def set_bkgd_bbox(self, bbox):
        self.bkgd_bbox = bbox

    def set_bboxes(self, bboxes):
        self.bboxes = bboxes

    def set_bkgd_near_far(self, near_far):
        self.bkgd_near_torchfar = near_far

    def set_max_min(self, maxs, mins):
        self.maxs, self.mins = maxs, mins

    def bbox_interpolation(self, float_frame_id, layer_id):
        start = self.bboxes[math.floor(float_frame_id), layer_id]
        end = self.bboxes[math.ceil(float_frame_id), layer_id]
        return torch.lerp(start, end, float_frame_id - math.floor(float_frame_id))

    # ---- host-side scene maths (l x 8 x 3 numbers, same torch ops as the reference) -------------
    def _pivot(self):
        """Edit pivot, layered_rfrender.py:216-232: mean of the frame-0 centres of layers 1 and 2, with each
        centre's z replaced by corner-1's z."""
        first = torch.cat([self.bkgd_bbox.detach().cpu().float(), self._box_table()[0].detach().cpu().float()], 0)
        centre = torch.mean(first, 1)
        centre[:, 2] = first[:, 1, 2]
        return (centre[2] + centre[1]) / 2

    def _edit_boxes(self, boxes):
        """boxes (..., l, 8, 3) on any device; returns edited boxes and the pivot (:230-242)."""
        pivot = None
        if self.scale is not None:
            pivot = self._pivot()
            pv = pivot.to(boxes.device)
            for i in range(len(self.scale)):
                boxes[..., i, :, :] = (boxes[..., i, :, :] - pv) * self.scale[i] + pv
        if self.shift is not None:
            for i in range(len(self.shift)):
                if self.shift[i] is None:
                    continue
                boxes[..., i, :, :] += torch.tensor(self.shift[i], dtype=torch.float32, device=boxes.device)
        return boxes, pivot

    @staticmethod
    def _parse_rotation(entry):
        """One entry of ``rotation`` -> None | (R (3,3) fp32, centre (3,) fp32 | None).  A float is radians about +z (the up axis
        of these scenes: the slab test's bottom / up faces, ``_pivot``), counter-clockwise seen from +z, its matrix built in
        fp64 and rounded to fp32; a (3,3) matrix must be a rotation; a pair adds the centre."""
        if entry is None:
            return None
        spec, centre = entry, None
        if isinstance(entry, (tuple, list)) and len(entry) == 2:
            spec, centre = entry
            centre = torch.as_tensor(centre, dtype=torch.float32).reshape(-1)
            if centre.numel() != 3:
                raise ValueError(f"rotation: a centre has 3 coordinates, got {centre.numel()}")
        a = torch.as_tensor(spec, dtype=torch.float64)
        if a.dim() == 0:
            c, s = math.cos(float(a)), math.sin(float(a))
            R = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64).to(torch.float32)
        elif tuple(a.shape) == (3, 3):
            R = a.to(torch.float32)
            r64 = R.to(torch.float64)
            # a non-rigid map would change the depths along a ray, which the depth merge of the layers relies on
            if float((r64.T @ r64 - torch.eye(3, dtype=torch.float64)).abs().max()) > 1e-5 or float(torch.linalg.det(r64)) < 0:
                raise ValueError("rotation: the 3x3 matrix is not a rotation (max |R^T R - I| > 1e-5 or det < 0)")
        else:
            raise ValueError(f"rotation: an entry is an angle, a 3x3 matrix or a (angle | matrix, centre) pair, got shape {tuple(a.shape)}")
        return R, centre

    def _rotation_specs(self):
        """None (no layer is rotated) or one parsed entry per layer (``_parse_rotation``)."""
        if self.rotation is None:
            return None
        l = self.total_layers
        if len(self.rotation) != l:
            raise ValueError(f"rotation must have one entry per layer ({l}, layer 0 = the background), got {len(self.rotation)}")
        specs = [self._parse_rotation(r) for r in self.rotation]
        return specs if any(sp is not None for sp in specs) else None

    def layer_ray_transforms(self, boxes):
        """Per layer None | (m (3,3) fp32, c (3,) fp32): the numbers the library gets for ``rotation`` (host arithmetic only).
        Layer i's content is turned by R_i about c_i after its scale and shift; rendering it, the layer sees the ray in its own
        frame, q = o - c:
            o'[r] = ((m[r,0] q[0] + m[r,1] q[1]) + m[r,2] q[2]) + c[r],   d'[r] = (m[r,0] d[0] + m[r,1] d[1]) + m[r,2] d[2]
        with m = R_i^T, every operation a separate fp32 one in this order (include/stnerf.h: stnerf_layer_rotation).
        boxes: the EDITED boxes (l,8,3) of the chunk group (any device), or None when every rotated layer names its centre.  A
        rotated layer without a centre turns about the fp32 mean of its box's 8 corners."""
        specs = self._rotation_specs()
        l = self.total_layers
        if specs is None:
            return [None] * l
        out = []
        for i, sp in enumerate(specs):
            if sp is None:
                out.append(None)
                continue
            R, c = sp
            if c is None:
                if boxes is None:
                    raise ValueError(f"rotation of layer {i} has no centre and no box to take one from: give (rotation, centre)")
                c = torch.mean(boxes[i].detach().to("cpu", torch.float32), 0)
            out.append((R.T.contiguous(), c.clone()))
        return out

    def _per_ray_box_transforms(self, rays, boxes):
        """``layer_ray_transforms`` for width-7 rays, whose edited boxes (n,l,8,3) are per ray: a default centre is row 0's box's,
        which is every ray's only if the call has ONE frame id (one device-to-host check, paid only for a rotation without a
        centre)."""
        need_box = any(sp is not None and sp[1] is None for sp in self._rotation_specs())
        if need_box and not bool((rays[:, 6] == rays[0, 6]).all()):
            raise ValueError("rotation without a centre on rays that mix frame ids: the layer's box differs from ray to ray, "
                             "give (rotation, centre)")
        return self.layer_ray_transforms(boxes[0] if need_box else None)

    def _point_edits(self, l, fine):
        """Per-layer inverse edit for sample points: coarse :293-303; fine :467-475 (where a None shift
        skips that layer's scale step as well)."""
        if self.shift is None and self.scale is None:
            return None
        out = []
        for i in range(l):
            sh = sc = None
            if self.shift is not None:
                if fine:
                    if self.shift[i] is None:
                        out.append((None, None))
                        continue
                    sh = self.shift[i]
                elif i < len(self.shift):
                    sh = self.shift[i]
            if self.scale is not None and (fine or i < len(self.scale)):
                sc = self.scale[i]
            out.append((sh, sc))
        return out

    def _retimed_boxes(self, row0_frame_ids):
        """One box per layer for a (reference) chunk from ROW 0's frame ids (:195-208), edited.
        row0_frame_ids: CPU fp32 tensor (l,) = rays[0, 6:]."""
        L = self.total_layers - 1
        bb = self._box_table().detach().cpu().float()
        per = torch.zeros(L, 8, 3)
        for i in range(L):
            f = row0_frame_ids[i + 1] - 1                        # fp32 0-dim tensor, as in the reference
            per[i] = torch.lerp(bb[math.floor(f), i], bb[math.ceil(f), i], f - math.floor(f))
        boxes = torch.cat([self.bkgd_bbox.detach().cpu().float(), per], 0)
        return self._edit_boxes(boxes)

    # ---- the chunk pipeline ------------------------------------------------------------------------
    def _nets(self, fine):
        return (self.bkgd_spacenet_fine, self.spacenets_fine) if fine else (self.bkgd_spacenet, self.spacenets)

    def _stage(self, rays, xyz, raw, lst, cnt, times_col, fine):
        """Deform + evaluate every layer's network on its (masked) rays through the op-level entry points
        (:340-418 / :495-576).  The render path itself runs this inside stnerf_render_rays; this op-level
        composition is kept for stage-by-stage debugging (tools/debug_stages.py)."""
        l = self.total_layers
        bk, nets = self._nets(fine)
        if self.use_deform_time:
            for i in range(1, l):
                if not self.is_shown_layer(i):
                    continue  # a hidden layer's points are never consumed
                ops.motionnet_fwd(self.time_deform_nets[self._module_index(i)]._packed("fp32"), xyz[:, i], rays[:, times_col(i)],
                                  add_to_xyz=True, ray_list=lst[i], ray_count=cnt[i:i + 1])
        ops.spacenet_fwd(bk._packed("fp32"), xyz[:, 0], rays[:, 3:6], None, raw[:, 0])
        for i in range(1, l):
            if not self.is_shown_layer(i):
                continue
            tm = rays[:, times_col(i)] if self.use_space_time else None
            ops.spacenet_fwd(nets[self._module_index(i)]._packed("fp32"), xyz[:, i], rays[:, 3:6], tm, raw[:, i], ray_list=lst[i],
                             ray_count=cnt[i:i + 1])

    def _render_launch(self, rays, boxes, pivot, retiming, only_coarse, thr, bthr, window, replay, piece=None, rotations=None,
                       scene=False, occupancy_ids=None, background_id=None, occluder=None, occluder_stops=False, background_rays=None,
                       deep=None, proposal_ids=None):
        """One kernel sequence over `rays` (n <= max_rays_per_launch) = ONE call into the C ABI
        (stnerf_render_rays, csrc/pipeline.hip).  boxes: (l,8,3) shared or (n,l,8,3).  piece: the (start, end) of `rays` in
        the call's ray tensor when the background cache or the layer cache may serve it (a view key is set), else None.  rotations: ``layer_ray_transforms`` of the
        chunk group, passed only when a layer is rotated.  scene: the in-scene layer passes come back as a sixth tensor (passed
        only by ``render_rays_scene``).  occupancy_ids: the chunk group's frame id per layer, passed only while occupancy grids
        are attached: one grid per shown performer layer is looked up or built and the table travels with the call.
        background_id: the chunk group's background frame id, passed only while the attached grids cull the background: its grid
        is looked up or built and travels with the call as an argument of its own.  occluder: the piece's rows (n,5) of
        ``render_rays_occluded`` (with scene): three more tensors come back; occluder_stops: its opaque rows lower the stop depth of
        the piece's terminated layers (dropped where the piece terminates nothing: only_coarse, every flagged layer cached).
        background_rays: the piece's entries (n,) of the per-ray background mask; such a call neither captures into nor reuses the
        background cache (the cached raw would hold the zeros of one mask); the layer cache is unaffected.  deep: the ``deep=`` dict of
        ``ops.render_rays`` (with scene): offsets, samples and total come back last.  proposal_ids: the chunk group's frame id per
        layer, passed only while grid proposals flag a layer: one density grid per flagged layer is looked up or built and the table
        travels with the call."""
        from stnerf_amd import hip
        n, l, dev = rays.shape[0], self.total_layers, rays.device
        p = self._render_params(rays.shape[1], pivot, retiming, only_coarse, thr, bthr, window)
        keep = []                                                    # packed blobs and grids must outlive the enqueue
        nets = self._net_pointers(keep)
        # the culls come before the workspace: their row lists and stop depths are part of it
        kw = self._occupancy_keywords(rays, retiming, occupancy_ids, background_id, keep)
        lcache = self._layer_cache if piece is not None else None
        lkeys = self._layer_cache_keys(lcache, piece, window, retiming, only_coarse, pivot, thr)
        kw.update(self._termination_keywords(dev, only_coarse, lkeys))
        need = ops.render_workspace_bytes(n, l, p.n1, p.n2, only_coarse, occupancy_samples=kw.get("occupancy_samples"),
                                          **(dict(terminate=kw["terminate"]) if "terminate" in kw else {}),
                                          **(dict(background=True) if "background_grid" in kw else {}),
                                          **(dict(background_rays=True) if background_rays is not None else {}))
        ws = getattr(self, "_workspace", None)
        if ws is None or ws.numel() < need or ws.device != dev:
            self._workspace = ws = torch.empty(need, dtype=torch.uint8, device=dev)
        cache = self._bkgd_cache if piece is not None and background_rays is None else None
        key, cache_arg = self._plan_background_cache(cache, piece, window, retiming, only_coarse, pivot, n, dev)
        lc_kw, wanted, capturing = self._plan_layer_caches(lcache, lkeys, only_coarse, dev)
        kw.update(lc_kw)
        # (a keyword travels only while its feature is on: an uncached, unedited call is the plain one it always was)
        if scene:
            kw.update(scene=True)
        if occluder is not None:
            kw.update(occluder=occluder, occluder_stops=bool(occluder_stops) and "terminate" in kw)
        if background_rays is not None:
            kw.update(background_rays=background_rays)
        if deep is not None:
            kw.update(deep=deep)
        if proposal_ids is not None:
            prop_table, held = self._proposal.table(self, proposal_ids, dev, retiming)
            keep.append(held)
            kw.update(proposal=prop_table)
        table = self._layer_alpha_table()
        if table is not None:
            kw.update(layer_alpha=table)
        try:
            out = ops.render_rays(rays, boxes, nets, p, ws, jitter=replay["jitter"] if replay else None,
                                  u=(replay.get("u") if replay else None), cache=cache_arg, rotations=rotations, **kw)
        except Exception:
            if cache_arg is not None and cache_arg[2] == hip.BKGD_CACHE_CAPTURE:
                cache.discard(key)             # (never filled)
            for k in capturing:
                lcache.discard(k)
            raise
        for i in wanted:                       # first sighting: the layer's hit count stays on the device (no sync)
            lcache.sighted(lkeys[i], out[4][:, i].sum(dtype=torch.int32))
        return out

    def _render_params(self, ray_width, pivot, retiming, only_coarse, thr, bthr, window):
        """The stnerf_render_params of one launch piece."""
        from stnerf_amd import hip
        l = self.total_layers
        p = hip.RenderParams()
        p.l, p.n1, p.n2, p.ray_stride = l, self.coarse_ray_sample, self.fine_ray_sample, ray_width
        p.retiming, p.only_coarse = int(retiming), int(only_coarse)
        p.use_deform_time, p.use_space_time = int(self.use_deform_time), int(self.use_space_time)
        p.bkgd_use_deform_time, p.bkgd_use_space_time = int(self.bkgd_use_deform_time), int(self.bkgd_use_space_time)
        p.deep_rgb = int(self.deep_rgb)
        # 3: bf16x3 (the default); 0: exact f32, one persistent launch per network stage; 2: exact f32, one launch per network
        p.precision = 3 if self.bkgd_spacenet.precision == "bf16x3" else (0 if self.mlp_schedule == "stage" else 2)
        for i in range(l):
            p.shown[i] = int(self.is_shown_layer(i))
        p.border, p.near, p.alpha = float(self.boarder_weight), float(self.near), float(self.alpha)
        p.density_threshold, p.bkgd_density_threshold = float(thr), float(bthr)
        p.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        p.ray_index_base, p.ray_index_stripe, p.ray_index_period = (int(x) for x in window)
        ec, ef = self._point_edits(l, False), self._point_edits(l, True)
        p.has_edits = int(ec is not None)
        ops.fill_edits(p.edits_coarse, ec, l)
        ops.fill_edits(p.edits_fine, ef, l)
        if pivot is not None:
            p.pivot[0], p.pivot[1], p.pivot[2] = pivot.tolist()
        return p

    def _net_pointers(self, keep):
        """The stnerf_nets of the shown layers in the model's arithmetic; the packed blobs go to ``keep``."""
        from stnerf_amd import hip
        prec = self.bkgd_spacenet.precision
        nets = hip.Nets()
        def ptr(module):
            pk = module._packed(prec)
            keep.append(pk)
            return pk.blob.data_ptr()
        nets.bkgd, nets.bkgd_fine = ptr(self.bkgd_spacenet), ptr(self.bkgd_spacenet_fine)
        if self.bkgd_use_deform_time:
            nets.motion[0] = ptr(self.bkgd_time_deform_net)
        for i in range(1, self.total_layers):
            if not self.is_shown_layer(i):
                continue
            j = self._module_index(i)                                # (an instance: its source's blobs, the same pointers)
            nets.space[i], nets.space_fine[i] = ptr(self.spacenets[j]), ptr(self.spacenets_fine[j])
            if self.use_deform_time:
                nets.motion[i] = ptr(self.time_deform_nets[j])
        return nets

    def _occupancy_keywords(self, rays, retiming, occupancy_ids, background_id, keep):
        """``ops.render_rays``'s keywords of the attached grids: the performers' table (looked up or built at ``occupancy_ids``) with
        its counters, the sample flags where the grids cull samples, and the background's grid at ``background_id``.  Nothing
        without grids; the grids in use go to ``keep``."""
        l, kw = self.total_layers, {}
        if occupancy_ids is not None:
            grids = self._occupancy
            occ_table, held = grids.table(self, occupancy_ids, rays.device, retiming)
            keep.append(held)
            if any(e is not None for e in occ_table):
                kw = dict(occupancy=occ_table, occupancy_counts=grids.counts(rays.device)[:l])
                if grids.samples:      # every ray-culled layer is sample-culled too
                    kw.update(occupancy_samples=[e is not None for e in occ_table], sample_counts=grids.sample_counts(rays.device)[:l])
        if background_id is not None:
            bg = self._occupancy.background_grid(self, background_id, rays.device)
            keep.append(bg)
            kw.update(background_grid=bg.entry(), background_counts=self._occupancy.background_counts(rays.device))
        return kw

    def _layer_cache_keys(self, lcache, piece, window, retiming, only_coarse, pivot, thr):
        """{layer: its ``layer_cache_key``} of every shown performer / instance of a piece whose view is known on the host."""
        l = self.total_layers
        if lcache is None or self.view_frame_ids is None or len(self.view_frame_ids) != (l if retiming else 1):
            return {}
        return {i: self.layer_cache_key(i, self.view_key, piece, window, retiming, only_coarse, pivot, density_threshold=thr)
                for i in range(1, l) if self.is_shown_layer(i)}

    def _termination_keywords(self, device, only_coarse, lkeys):
        """``ops.render_rays``'s keywords of the attached termination, or nothing: no fine stage, no flag left (a cached performer,
        one of ``lkeys``, is not terminated)."""
        term = getattr(self, "_termination", None)
        if term is None or only_coarse:
            return {}
        flags = [0 if i in lkeys else f for i, f in enumerate(term.flags(self))]
        if not any(flags):
            return {}
        return dict(terminate=flags, tau=term.tau, visibility_counts=term.counts(device)[:self.total_layers])

    def _plan_background_cache(self, cache, piece, window, retiming, only_coarse, pivot, n, device):
        """-> (key, ``ops.render_rays``'s cache argument): the background's raw outputs of this piece come from the cache (hit), go
        into it (miss with room), or neither (no cache, over budget)."""
        from stnerf_amd import hip
        if cache is None:
            return None, None
        key = self.background_cache_key(self.view_key, piece, window, retiming, only_coarse, pivot)
        entry, mode = cache.lookup(key), hip.BKGD_CACHE_REUSE
        if entry is None:
            entry, mode = cache.reserve(key, n, self.coarse_ray_sample, self.fine_ray_sample, only_coarse, device), hip.BKGD_CACHE_CAPTURE
        return key, (None if entry is None else (entry[0], entry[1], mode))

    def _plan_layer_caches(self, lcache, lkeys, only_coarse, device):
        """-> (``ops.render_rays``'s layer-cache keywords, the layers whose hit count is wanted, the keys being captured).  Per cached
        layer: from its entry (third sighting on), into a fresh one (second sighting, room in the budget), or neither."""
        from stnerf_amd import hip
        if not lkeys:
            return {}, [], []
        l = self.total_layers
        plans = {i: lcache.plan(k, self.coarse_ray_sample, self.fine_ray_sample, only_coarse, device) for i, k in lkeys.items()}
        wanted = [i for i, k in lkeys.items() if plans[i][1] is None and lcache.wants_count(k)]
        capturing = [lkeys[i] for i, (mode, _) in plans.items() if mode == hip.LAYER_CACHE_CAPTURE]
        kw = {}
        if any(e is not None for _, e in plans.values()):
            kw = dict(layer_caches=[plans[i][1].arg(plans[i][0]) if i in plans and plans[i][1] is not None else None for i in range(l)],
                      layer_mismatch=lcache.mismatch_counter(device))
        return kw, wanted, capturing

    def render_rays(self, rays, only_coarse=False, density_threshold=0.0001, bkgd_density_threshold=0.0,
                    ref_chunk: Optional[int] = None):
        """Render all `rays`; ``ref_chunk`` reproduces the reference's chunk semantics (boxes are taken
        from row 0 of every ``ref_chunk``-ray piece) while launching kernels over far larger pieces."""
        return self.as_reference_tuple(self.render_rays_raw(rays, only_coarse, density_threshold, bkgd_density_threshold,
                                                            ref_chunk))

    def _refuse_scene_call(self, name, what_has, how):
        """The two refusals of the calls that return scene passes: in training mode (no backward) and on more than one rank."""
        if torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError(f"{name} in training mode: {what_has} no backward; call model.eval() or wrap the render in torch.no_grad()")
        from stnerf_amd import parallel
        if parallel.active_group(self) is not None:
            raise RuntimeError(f"{name} under shard_views with more than one rank: the all-gather's modes (stnerf_amd.parallel) "
                               f"have fixed widths and a \"scene\" gather mode is out of scope; {how} (model.shard_views = False)")

    def render_rays_scene(self, rays, only_coarse=False, density_threshold=0.0001, bkgd_density_threshold=0.0,
                          ref_chunk: Optional[int] = None, background_rays=None):
        """``render_rays`` plus the in-scene layer passes of the final stage -> (the reference 5-tuple, scene).  ``scene`` is a
        list of l (colour (n,3), depth (n,1), alpha (n,1)) triples: layer i's share of the MIXED image -- premultiplied colour,
        weighted depth and alpha with the other layers occluding it and being occluded by it (fine_layer[i] is layer i alone).
        Their sum over the layers is the mixed triple up to fp32 summation order; a hidden layer's is exact zeros.  The five
        standard outputs are the bits of ``render_rays``.  Inference only: no backward is defined for the pass.
        ``background_rays``: the per-ray background mask of ``render_rays_raw``."""
        self._refuse_scene_call("render_rays_scene", "the in-scene layer passes have", "render the passes on one rank")
        raw = self._render_rays_raw(rays, only_coarse, density_threshold, bkgd_density_threshold, ref_chunk, scene=True,
                                    background_rays=background_rays)
        sc = raw[5]
        scene = [(sc[:, i, 0:3], sc[:, i, 3:4], sc[:, i, 4:5]) for i in range(self.total_layers)]
        return self.as_reference_tuple(raw[:5]), scene

    def render_rays_occluded(self, rays, occluder, only_coarse=False, density_threshold=0.0001, bkgd_density_threshold=0.0,
                             ref_chunk: Optional[int] = None, stops=False, background_rays=None):
        """``render_rays_scene`` with a depth-tested occluder in the scene -> (the reference 5-tuple, scene, occluded).
        ``occluder`` (n,5) fp32 on the device: one row {r, g, b, a, z} per ray -- a CG prop, a title card, a plate with a z-buffer;
        z is a RAY PARAMETER, in the units of the depth outputs (``ops.ray_parameter`` turns a camera-space z-buffer into it); a row
        with a <= 0 (or NaN) or a z that is not finite is absent.  It is sliced by launch piece and chunk group exactly as the rays
        are.  ``occluded`` = dict(mixed=triple, scene=[l triples], share=triple): the mixed image with the occluder in the scene
        (it hides the samples at or behind z in proportion to a, and is hidden by the samples in front of it), every layer's share
        of that image, and the occluder's own premultiplied share; mixed = sum of the shares up to fp32 summation order.  Samples
        are not clipped at z: one that starts in front keeps its whole weight.  include/stnerf.h states the arithmetic.
        ``stops=True``: an opaque row (a >= 1) also lowers early ray termination's stop depth to z, so the fine samples behind it
        are not evaluated; it needs an attached termination (``set_termination``; ValueError otherwise).  The occluded outputs keep
        their bits; the 5-tuple and ``scene`` become those of the terminated scene.  Without it they are the bits of
        ``render_rays_scene``.  ``background_rays``: the per-ray background mask of ``render_rays_raw``, sliced as the occluder rows
        are -- with it a frame takes its background from the occluder where a row is present and from the networks where it is not
        (``stnerf_amd.reproject``).  Inference only, one rank, the fused pipeline only."""
        self._refuse_scene_call("render_rays_occluded", "the occluder composite has", "render on one rank")
        if stops and getattr(self, "_termination", None) is None:
            raise ValueError("render_rays_occluded(stops=True) without early ray termination: the occluder lowers the stop depth the "
                             "terminated layers' row lists test; call set_termination(...) first or pass stops=False")
        if not torch.is_tensor(occluder) or occluder.dim() != 2 or tuple(occluder.shape) != (rays.shape[0], 5):
            raise ValueError(f"render_rays_occluded: the occluder must be a ({rays.shape[0]},5) tensor of (r, g, b, a, z) rows, got "
                             f"{tuple(occluder.shape) if torch.is_tensor(occluder) else type(occluder).__name__}")
        raw = self._render_rays_raw(rays, only_coarse, density_threshold, bkgd_density_threshold, ref_chunk, scene=True,
                                    occluder=occluder, occluder_stops=stops, background_rays=background_rays)
        l = self.total_layers
        trip = lambda x: (x[..., 0:3], x[..., 3:4], x[..., 4:5])
        scene = [trip(raw[5][:, i]) for i in range(l)]
        occluded = dict(mixed=trip(raw[6]), scene=[trip(raw[7][:, i]) for i in range(l)], share=trip(raw[8]))
        return self.as_reference_tuple(raw[:5]), scene, occluded

    def render_rays_deep(self, rays, spec=None, only_coarse=False, density_threshold=0.0001, bkgd_density_threshold=0.0,
                         ref_chunk: Optional[int] = None, occluder=None, capacity: Optional[int] = None):
        """``render_rays_scene`` with deep output -> (the reference 5-tuple, scene, DeepFrame) -- or, with ``occluder`` (n,5),
        (5-tuple, scene, occluded, DeepFrame) as ``render_rays_occluded`` returns them; the deep frame is of the scene WITHOUT the
        occluder.  ``spec``: a ``stnerf_amd.DeepSpec`` (None: the default, every sample of nonzero weight its own record).  The
        frame is a piece of H = 1, W = n pixels: per ray the kept samples of the final stage with their premultiplied colour, alpha
        and depths (include/stnerf.h states the rules), on which ``DeepFrame.composite`` puts depth-tested elements with no network.
        The five outputs and ``scene`` are the bits of ``render_rays_scene``.  The call never re-renders and never drops: every launch
        piece's record buffer has the worst case n l S records, and the piece is shrunk so that the buffer stays under
        ``stnerf_amd.deep.PIECE_BUFFER_BYTES``; the piece's total is read back (one host sync per piece) and that many records join
        the frame's list.  ``capacity``: records per launch piece instead of the worst case; a piece that needs more raises
        RuntimeError with the total it needs.  Inference only, one rank, the fused pipeline only."""
        from stnerf_amd import deep as D
        self._refuse_scene_call("render_rays_deep", "deep output has", "render on one rank")
        spec = D.as_spec(spec) or D.DeepSpec()
        if occluder is not None and (not torch.is_tensor(occluder) or tuple(occluder.shape) != (rays.shape[0], 5)):
            raise ValueError(f"render_rays_deep: the occluder must be a ({rays.shape[0]},5) tensor of (r, g, b, a, z) rows")
        raw, pieces = self._render_rays_raw(rays, only_coarse, density_threshold, bkgd_density_threshold, ref_chunk, scene=True,
                                            occluder=occluder, deep=spec.options(capacity))
        l = self.total_layers
        trip = lambda x: (x[..., 0:3], x[..., 3:4], x[..., 4:5])
        scene = [trip(raw[5][:, i]) for i in range(l)]
        frame = D.DeepFrame.from_pieces(pieces, 1, rays.shape[0], l, device=rays.device)
        if occluder is None:
            return self.as_reference_tuple(raw[:5]), scene, frame
        occluded = dict(mixed=trip(raw[6]), scene=[trip(raw[7][:, i]) for i in range(l)], share=trip(raw[8]))
        return self.as_reference_tuple(raw[:5]), scene, occluded, frame

    def as_reference_tuple(self, raw):
        """(mixed_fine (n,5), mixed_coarse (n,5), layer_fine (n,l,5), layer_coarse (n,l,5), mask (n,l)) -> the
        reference's 5-tuple of (color (n,3), depth (n,1), acc (n,1)) triples and bool masks (layered_rfrender.py:725-734)."""
        mix_f, mix_c, lo_f, lo_c, mask = raw
        l = self.total_layers
        trip = lambda x: None if x is None else (x[:, 0:3], x[:, 3:4], x[:, 4:5])
        fine_layer = None if lo_f is None else [trip(lo_f[:, i]) for i in range(l)]
        coarse_layer = None if lo_c is None else [trip(lo_c[:, i]) for i in range(l)]
        ray_mask = None if mask is None else [mask[:, i].bool() for i in range(l)]
        return trip(mix_f), trip(mix_c), fine_layer, coarse_layer, ray_mask

    def _warn_if_eval_with_grad(self):
        """the reference builds an autograd graph in eval() mode too; here training is gated on train() (the inference
        kernels save nothing), so a fine-tuning script that never calls model.train() would get outputs without history.  Say so once."""
        if (torch.is_grad_enabled() and not self.training and not getattr(self, "_warned_eval_grad", False)
                and any(p.requires_grad for p in self.parameters())):
            import warnings
            self._warned_eval_grad = True
            warnings.warn("LayeredRFRender.forward in eval() mode with autograd enabled and trainable parameters: the MI355X inference "
                          "kernels run and the outputs carry NO autograd history (the reference would build a graph here).  Call "
                          "model.train() to train, or wrap rendering in torch.no_grad() to silence this.", RuntimeWarning, stacklevel=3)

    def advance_seed(self):
        """What a finished call does to ``seed`` (``fresh_draws_per_call``; a rank that owns no ray of a sharded view
        calls this too, so that every rank's stream stays the same).  A no-op while a background cache is attached
        or a layer cache is attached (``set_background_cache`` / ``set_layer_cache``: one jitter pattern for all the frames of a
        cached run)."""
        if self.fresh_draws_per_call and self.replay is None and getattr(self, "_bkgd_cache", None) is None \
                and getattr(self, "_layer_cache", None) is None:
            self.seed = (int(self.seed) + 1) & 0xFFFFFFFFFFFFFFFF   # the next call draws new jitter / resampling numbers

    def render_rays_raw(self, rays, only_coarse=False, density_threshold=0.0001, bkgd_density_threshold=0.0,
                        ref_chunk: Optional[int] = None, background_rays=None):
        """``render_rays`` before the outputs are cut into the reference's triples: the five tensors the library
        wrote (what stnerf_amd.parallel packs into its one all-gather).
        ``background_rays``: None | an (n,) uint8 or bool device tensor, the per-ray background mask (include/stnerf.h states the
        rule): the background is evaluated only on the rays whose entry is nonzero; on the others every sample of layer 0 has zero
        network outputs in both stages -- what the background's sample cull does in an empty cell -- and costs no network row.  It
        is sliced by launch piece and chunk group exactly as an occluder's rows are, and composes with a background grid and with
        early ray termination.  Such a call neither captures into nor reuses the background cache; the layer cache is unaffected.
        Inference only, one rank, the fused pipeline only."""
        if background_rays is not None:
            self._refuse_scene_call("render_rays_raw(background_rays=)", "the per-ray background mask has", "render on one rank")
        return self._render_rays_raw(rays, only_coarse, density_threshold, bkgd_density_threshold, ref_chunk,
                                     background_rays=background_rays)

    def _render_rays_raw(self, rays, only_coarse, density_threshold, bkgd_density_threshold, ref_chunk, scene=False, occluder=None,
                         occluder_stops=False, background_rays=None, deep=None):
        """``render_rays_raw``; scene: a sixth tensor, the in-scene layer passes (n,l,5) of ``render_rays_scene``; occluder (with
        scene): the rows (N,5) of ``render_rays_occluded``, three more tensors (occluded mixed, scene, share); background_rays: the
        (N,) per-ray background mask of ``render_rays_raw``; deep (with scene): the ``deep=`` dict of ``ops.render_rays`` -- the
        result is then (the tuple, [(offsets, samples) per launch piece])."""
        if not rays.is_cuda:
            raise RuntimeError("rays must live on the GPU: the MI355X render path has no CPU fallback")
        rays = rays.contiguous().float()
        N, L = rays.shape[0], self.total_layers - 1      # (performers and instances: one frame-id column each with retiming)
        width = rays.shape[1]
        if width == 7:
            retiming = False
        elif width == 7 + L:
            retiming = True
        else:
            raise ValueError(f"undefined ray format in LayeredRFRender, ray dimension is {width}")
        if self.bkgd_bbox is None or self.bboxes is None:
            raise RuntimeError("set_bkgd_bbox / set_bboxes must be called before rendering")
        if N == 0:  # the reference dereferences row 0 (rays_frame_id[0, i+1], layered_rfrender.py:200)
            raise IndexError("empty ray batch: LayeredRFRender needs at least one ray")
        # BKGD_USE_SPACE_TIME on a batch that MIXES background frame ids (training rays; off in both shipped ymls): the reference tiles
        # the ids over the samples (modeling/spacenet.py:117-118 with the 1-D tensor of layered_rfrender.py:380,385), so every sample of
        # layer 0 has its own time.  The fused pipeline keeps one time per ray; such a call takes the op-by-op path below, which
        # evaluates the background per sample (stnerf_amd.modeling.training._stage).  One id per call -- every rendered frame -- is the
        # identity and stays on the fused pipeline.
        per_sample_bkgd_time = False
        if self.bkgd_use_space_time and self.use_space_time:
            from stnerf_amd.modeling import training as _training
            per_sample_bkgd_time = _training.mixed_bkgd_ids(rays)
        if occluder is not None and per_sample_bkgd_time:
            raise NotImplementedError("an occluder on rays that mix background frame ids (BKGD_USE_SPACE_TIME): that call takes the "
                                      "op-by-op path, which has no occluder composite -- a render-time edit, as rotation is; render one "
                                      "background frame id per call")
        if background_rays is not None:
            if (not torch.is_tensor(background_rays) or tuple(background_rays.shape) != (N,)
                    or background_rays.dtype not in (torch.uint8, torch.bool)):
                raise ValueError(f"background_rays must be a ({N},) uint8 or bool tensor, one entry per ray, got "
                                 f"{(tuple(background_rays.shape), background_rays.dtype) if torch.is_tensor(background_rays) else type(background_rays).__name__}")
            if per_sample_bkgd_time:
                raise NotImplementedError("a per-ray background mask on rays that mix background frame ids (BKGD_USE_SPACE_TIME): that call "
                                          "takes the op-by-op path, which has no row lists -- a render-time edit, as rotation is; render one "
                                          "background frame id per call")
            if self.mlp_schedule != "stage" and self.bkgd_spacenet.precision != "bf16x3":
                raise ValueError("a per-ray background mask with mlp_schedule = 'per_net' (one launch per network): the mask walks row "
                                 "lists in the persistent stage kernels; use mlp_schedule = 'stage' or drop background_rays")
        if deep is not None and torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("deep output in training mode: it has no backward; call model.eval() or wrap the render in torch.no_grad()")
        if scene and per_sample_bkgd_time:
            raise RuntimeError("render_rays_scene on rays that mix background frame ids (BKGD_USE_SPACE_TIME): that call takes the "
                               "op-by-op path, which has no in-scene layer passes; render one background frame id per call")
        # Training: model.train() + autograd enabled + trainable parameters = what engine/layered_trainer.py:186-194
        # sets up -> the same stages launched op by op with autograd history (stnerf_amd.modeling.training).  In eval() mode the
        # inference kernels run and the outputs carry no history, as under torch.no_grad() (render/layered_neural_renderer.py:377).
        train = torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.parameters())
        if train or per_sample_bkgd_time:
            what = self._inference_only_edits()
            if what is not None:
                raise NotImplementedError(f"{what} on the op-by-op path (training, and batches that mix background frame ids under "
                                          "BKGD_USE_SPACE_TIME): a render-time edit, as rotation is -- call model.eval() or wrap the "
                                          "render in torch.no_grad(), and clear_instances() / layer_alpha = None / set_termination(None) to train")
        self._layer_alpha_table()          # (its ValueErrors before anything is launched)
        culling = getattr(self, "_occupancy", None) is not None
        if culling and self.replay is not None and any(k in self.replay for k in ("xyz_c", "xyz_f")):
            raise ValueError("occupancy grids with replayed deformed points (replay[\"xyz_c\"] / [\"xyz_f\"]): those lists are per hit "
                             "ray, and the cull changes which rays hit; replay jitter / u only, or detach the grids")
        if culling and self._occupancy.samples and self.mlp_schedule != "stage" and self.bkgd_spacenet.precision != "bf16x3":
            raise ValueError("occupancy grids with samples=True and mlp_schedule = 'per_net' (one launch per network): the sample cull "
                             "walks row lists in the persistent stage kernels; use mlp_schedule = 'stage' or OccupancyGrids(samples=False)")
        bg_culling = culling and self._occupancy.has_background()
        if bg_culling and self.mlp_schedule != "stage" and self.bkgd_spacenet.precision != "bf16x3":
            raise ValueError("occupancy grids with a background grid and mlp_schedule = 'per_net' (one launch per network): the cull "
                             "walks row lists in the persistent stage kernels; use mlp_schedule = 'stage' or drop the background's grid")
        term = getattr(self, "_termination", None)
        if term is not None and not only_coarse and any(term.flags(self)):     # (what the library refuses too, before the first piece)
            if self.mlp_schedule != "stage" and self.bkgd_spacenet.precision != "bf16x3":
                raise ValueError("early ray termination with mlp_schedule = 'per_net' (one launch per network): the fine stage walks row "
                                 "lists in the persistent stage kernels; use mlp_schedule = 'stage' or set_termination(None)")
            table = self._layer_alpha_table()
            if (table is None and _alpha_acts(self)) or (table is not None and any(a != 1.0 for a in table)):
                raise ValueError(f"early ray termination with alpha = {self.alpha} / layer_alpha = {self.layer_alpha}: the coarse composite "
                                 "ignores both opacities, so its stop depth would be wrong for a layer made transparent in the fine "
                                 "composite; leave them at 1 or set_termination(None)")
        flagged = self._proposal.flagged_layers(self) if getattr(self, "_proposal", None) is not None else []
        if flagged:
            self._check_proposal(flagged, background_rays)
        self._warn_if_eval_with_grad()
        if occluder is not None:
            occluder = occluder.to(rays.device, torch.float32).contiguous()
        if background_rays is not None:
            background_rays = background_rays.to(rays.device).contiguous()
        groups = self._chunk_groups(rays, retiming, ref_chunk)
        occ_ids = self._occupancy_frame_ids(rays, groups, retiming) if culling and self._occupancy.culled_layers(self) else None
        bg_ids = self._background_frame_ids(rays, groups) if bg_culling else None
        prop_ids = self._proposal_frame_ids(rays, groups, retiming, flagged) if flagged else None
        outs, deep_pieces = [], []
        cap = self.max_rays_per_launch
        if deep is not None:   # the piece's worst-case record buffer stays under the budget
            from stnerf_amd import deep as _deep
            cap = min(cap, _deep.piece_rays(self.total_layers, self.coarse_ray_sample if only_coarse else self.coarse_ray_sample + self.fine_ray_sample))
        first, stripe, period = self.ray_window
        if stripe > 0:                     # launch pieces must start on a stripe boundary
            cap = max(stripe, cap // stripe * stripe)
            if any(g[0] % stripe for g in groups):
                raise ValueError("a striped ray window needs chunk groups that start on a stripe boundary "
                                 "(frame ids that change inside the view: render it unstriped)")
        window_at = (lambda s: (first + s, 0, 0)) if stripe <= 0 else (lambda s: (first + s // stripe * period, stripe, period))
        # the background cache serves calls whose view is known on the host (view_key) and whose draws are the device RNG's
        cacheable = ((getattr(self, "_bkgd_cache", None) is not None or getattr(self, "_layer_cache", None) is not None)
                     and getattr(self, "view_key", None) is not None
                     and self.replay is None and not train and not per_sample_bkgd_time)
        for gi, (g0, g1, boxes, pivot, *rot) in enumerate(groups):
            for s in range(g0, g1, cap):
                e = min(s + cap, g1)
                bx = boxes if boxes.dim() == 3 else boxes[s:e].contiguous()
                rp = None
                if self.replay is not None:
                    # jitter / u / z: (l, N, *) per-ray draws, cut with the rays; xyz_c / xyz_f (teacher forcing, parity tests only): per
                    # performer the deformed points of its hit rays -- whole-batch lists, one launch piece only
                    rp = {k: (v[:, s:e].contiguous() if torch.is_tensor(v) else v) for k, v in self.replay.items()}
                    if any(not torch.is_tensor(v) for v in rp.values()) and (s, e) != (0, N):
                        raise ValueError("replayed deformed points (xyz_c / xyz_f) need the whole batch in one launch piece")
                if train or per_sample_bkgd_time:
                    from stnerf_amd.modeling.training import render_rays_train
                    outs.append(render_rays_train(self, rays[s:e], bx, pivot, retiming, only_coarse, density_threshold,
                                                  bkgd_density_threshold, window_at(s), rp))
                else:
                    # (the piece travels only when the cache may serve it: uncached, the call is the nine-argument one it always was)
                    outs.append(self._render_launch(rays[s:e], bx, pivot, retiming, only_coarse, density_threshold,
                                                    bkgd_density_threshold, window_at(s), rp, *(((s, e),) if cacheable else ()),
                                                    **(dict(rotations=rot[0]) if rot else {}), **(dict(scene=True) if scene else {}),
                                                    **(dict(occupancy_ids=occ_ids[gi]) if occ_ids is not None else {}),
                                                    **(dict(background_id=bg_ids[gi]) if bg_ids is not None else {}),
                                                    **(dict(occluder=occluder[s:e], occluder_stops=occluder_stops)
                                                       if occluder is not None else {}),
                                                    **(dict(background_rays=background_rays[s:e]) if background_rays is not None else {}),
                                                    **(dict(deep=deep) if deep is not None else {}),
                                                    **(dict(proposal_ids=prop_ids[gi]) if prop_ids is not None else {})))
                    if deep is not None:
                        offsets, samples, total = outs[-1][-3:]
                        need = int(total)           # (the one host sync of a deep piece)
                        if need > samples.shape[0]:
                            raise RuntimeError(f"render_rays_deep: the launch piece of rays {s}..{e} needs {need} deep records, the "
                                               f"capacity is {samples.shape[0]}")
                        deep_pieces.append((offsets, samples[:need].clone()))
                        del samples, total
                        outs[-1] = outs[-1][:-3]    # (the worst-case buffer goes back to the allocator: the next piece reuses it)
        cat = (lambda j: outs[0][j]) if len(outs) == 1 else (lambda j: torch.cat([o[j] for o in outs], 0))
        raw = tuple(cat(j) for j in range((9 if occluder is not None else 6) if scene else 5))
        self.advance_seed()
        return raw if deep is None else (raw, deep_pieces)

    def _chunk_groups(self, rays, retiming, ref_chunk):
        """The chunk groups of a call's rays (contiguous float32, on the device): (start, end, edited boxes, pivot[, rotations]) per
        run of reference chunks that share their boxes -- one group of per-ray boxes for width-7 rays."""
        N = rays.shape[0]
        step = N if ref_chunk is None else ref_chunk
        rotated = self._rotation_specs() is not None
        groups = []  # (start, end, boxes, pivot[, rotations])
        if retiming:
            row0 = rays[0::step, 6:].cpu()  # one D2H: row-0 frame ids of every reference chunk
            n_chunks, c0 = row0.shape[0], 0
            for c in range(1, n_chunks + 1):  # merge runs of reference chunks that share their boxes
                if c == n_chunks or not torch.equal(row0[c], row0[c0]):
                    boxes, pivot = self._retimed_boxes(row0[c0])
                    groups.append((c0 * step, min(c * step, N), boxes.to(rays.device), pivot)
                                  + ((self.layer_ray_transforms(boxes),) if rotated else ()))
                    c0 = c
        else:
            fid = rays[:, 6].to(torch.int64) - 1
            bb = self._box_table().to(rays.device).float().index_select(0, fid)                    # :193
            bk = self.bkgd_bbox.to(rays.device).float().unsqueeze(0).expand(N, 1, 8, 3)
            boxes, pivot = self._edit_boxes(torch.cat([bk, bb], 1).contiguous())
            groups.append((0, N, boxes, pivot) + ((self._per_ray_box_transforms(rays, boxes),) if rotated else ()))
        return groups

    def ray_masks(self, rays, ref_chunk: Optional[int] = None):
        """The pipeline's own ray mask of ``rays`` without rendering them -> (n, l) uint8, 1 where the ray meets layer i's edited (and
        rotated) box: the coarse sampler's call of ``render_rays_raw`` on the same chunk groups -- the same boxes, edits, pivots and
        rotations, no points -- before any occupancy cull (which only clears bits).  It draws nothing that matters (a mask does not
        depend on the jitter) and leaves the seed alone."""
        if not rays.is_cuda:
            raise RuntimeError("rays must live on the GPU: the MI355X render path has no CPU fallback")
        rays = rays.contiguous().float()
        N, l = rays.shape[0], self.total_layers
        if rays.shape[1] not in (7, 6 + l):
            raise ValueError(f"undefined ray format in LayeredRFRender, ray dimension is {rays.shape[1]}")
        if self.bkgd_bbox is None or self.bboxes is None:
            raise RuntimeError("set_bkgd_bbox / set_bboxes must be called before rendering")
        if N == 0:
            raise IndexError("empty ray batch: LayeredRFRender needs at least one ray")
        edits = self._point_edits(l, False)
        masks = []
        for g0, g1, boxes, pivot, *rot in self._chunk_groups(rays, rays.shape[1] != 7, ref_chunk):
            bx = boxes if boxes.dim() == 3 else boxes[g0:g1].contiguous()
            masks.append(ops.sample_coarse(rays[g0:g1], bx, self.coarse_ray_sample, seed=int(self.seed) & 0xFFFFFFFFFFFFFFFF, edits=edits,
                                           pivot=pivot, want_xyz=False, **(dict(rotations=rot[0]) if rot else {}))[2])
        return masks[0] if len(masks) == 1 else torch.cat(masks, 0)

    def forward(self, rays, labels=None, bboxes=None, only_coarse=False, near_far=None, near_far_points=[],
                density_threshold=0.0001, bkgd_density_threshold=0):
        """(fine_mixed, coarse_mixed, fine_layer[l], coarse_layer[l], ray_mask[l]); every entry a
        (color (N,3), depth (N,1), acc (N,1)) triple.  layered_rfrender.py:141-734.
        labels / bboxes / near_far / near_far_points are accepted and ignored, as in the BBOX path."""
        return self.render_rays(rays, only_coarse, density_threshold, bkgd_density_threshold, ref_chunk=None)
