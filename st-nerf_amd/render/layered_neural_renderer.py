"""User-facing layered renderer: camera paths, retiming, per-frame edit schedule, per-pose rendering.

Mirror of ``LayeredNeuralRenderer`` (render/layered_neural_renderer.py:17-741) for the methods the shipped
demos use (demo/taekwondo_demo.py:46-53): same method names, argument meaning and bookkeeping
(``poses`` / ``Ks`` / ``layer_frame_pairs`` / ``s_*_frame`` lists), same scipy calls for the pose path
(Slerp of the rotations + ``splprep``/``splev`` of the camera centres).  Differences:

* the reference constructor reads a dataset and a checkpoint from ``cfg.OUTPUT_DIR``
  (:96-121, needs open3d / torchvision and the absent data); here the model, the camera poses and the
  intrinsics are passed in (``model=``, ``gt_poses=``, ``gt_Ks=``).  ``from_checkpoint`` covers the
  checkpoint half (reference key names);
* rays are generated on the device and images stay there until the caller asks for them
  (``render_path`` returns them; writing jpg/png/mp4 is left to ``on_frame`` -- imageio is absent here);
* per-frame rendering is ``stnerf_amd.render.render_pose.render_pose`` (HIP kernels).

The host logic below is pinned against fixtures produced by the reference's own methods
(tests/golden/make_golden.py: ``g_path``).
"""
from __future__ import annotations

from typing import Callable, List, Optional

import numpy as np
import torch
from scipy.interpolate import splev, splprep
from scipy.spatial.transform import Rotation as R
from scipy.spatial.transform import Slerp

from stnerf_amd.render.render_pose import render_pose as _render_pose


class LayeredNeuralRenderer:

    def __init__(self, cfg, scale=None, shift=None, rotation=None, s_shift=None, s_scale=None, s_alpha=None, *,
                 model=None, gt_poses=None, gt_Ks=None, cache_background=False, s_rotation=None, scene_passes=False,
                 layer_alpha=None, s_layer_alpha=None, occupancy=False, terminate=False, cache_layers=False,
                 occluder=None, occluder_stops=False, accumulate=None, lens=None, reproject=None, lattice=None, deep=None,
                 proposal=False):
        if model is None or gt_poses is None or gt_Ks is None:
            raise NotImplementedError(
                "dataset / checkpoint discovery from cfg.OUTPUT_DIR (render/layered_neural_renderer.py:96-121) is "
                "outside the MI355X hot path: pass model=, gt_poses= (C,4,4) and gt_Ks= (C x (3,3)) explicitly")
        self.alpha = None
        self.cfg = cfg
        self.scale, self.shift, self.rotation = scale, shift, rotation
        self.s_shift, self.s_scale, self.s_alpha = s_shift, s_scale, s_alpha
        # s_rotation = (start, end): per-layer angles about +z (radians; None = that layer is not rotated), interpolated per
        # frame like s_shift.  `rotation` itself goes to the model as scale / shift do (LayeredRFRender.rotation: angle, matrix
        # or (angle | matrix, centre) per layer); the reference stores it and never reads it (:19-24).
        self.s_rotation = s_rotation
        if s_rotation is not None:
            if len(s_rotation) != 2 or len(s_rotation[0]) != len(s_rotation[1]) or \
                    any((a is None) != (b is None) for a, b in zip(s_rotation[0], s_rotation[1])):
                raise ValueError("s_rotation is (start, end): two per-layer angle lists with None in the same places")
            self.rotation = list(s_rotation[0])
        # layer_alpha: one opacity per layer (None = 1.0; LayeredRFRender.layer_alpha: every layer's density factor in the fine
        # composite, where `alpha` reaches layer 2 alone); s_layer_alpha = (start, end), interpolated per frame like s_rotation.
        # Not in the reference (keyword-only)
        self.layer_alpha, self.s_layer_alpha = layer_alpha, s_layer_alpha
        if s_layer_alpha is not None:
            if len(s_layer_alpha) != 2 or len(s_layer_alpha[0]) != len(s_layer_alpha[1]) or \
                    any((a is None) != (b is None) for a, b in zip(s_layer_alpha[0], s_layer_alpha[1])):
                raise ValueError("s_layer_alpha is (start, end): two per-layer opacity lists with None in the same places")
            self.layer_alpha = list(s_layer_alpha[0])
        if s_shift is not None:
            self.shift = self.s_shift[0]
        if s_scale is not None:
            self.scale = self.s_scale[0]
        if s_alpha is not None:
            self.alpha = self.s_alpha[0]
        self.model = model
        self.model.scale, self.model.shift = self.scale, self.shift
        self.model.rotation = self.rotation
        self.model.layer_alpha = self.layer_alpha
        self.cache_background = cache_background
        self.cache_layers = cache_layers
        self.occupancy = occupancy
        self.terminate = terminate
        self.proposal = proposal
        # scene_passes: render_path / render_path_walking also keep every layer's share of the mixed image (its premultiplied
        # colour and alpha with the other layers' occlusion: render_pose's `scene_passes`) in images_scene / alphas_scene and
        # hand the frame's dict to on_frame as the keyword `scene`; not in the reference (keyword-only, off by default)
        self.scene_passes = bool(scene_passes)
        # occluder: callable(frame_index, pose, K) -> (rgba (H,W,4), depth (H,W) in ray-parameter units) | None, an element that is
        # not a radiance field put into every frame it returns one for (render_pose's `occluder`); the frame's occluded results are
        # kept in images_occluded and handed to on_frame as the keyword `occluded`.  occluder_stops: its opaque pixels also stop
        # early ray termination (it needs `terminate`).  Not in the reference (keyword-only, off by default)
        if occluder is not None and not callable(occluder):
            raise TypeError(f"occluder is a callable (frame_index, pose, K) -> (rgba, depth) | None, got {type(occluder).__name__}")
        self.occluder, self.occluder_stops = occluder, bool(occluder_stops)
        self.images_occluded = []
        # accumulate: an stnerf_amd.accumulate.AccumulateSpec or the dict of its arguments -- every frame of render_path /
        # render_path_walking is the per-pixel mean of several passes (anti-aliasing, motion blur, adaptive samples per pixel:
        # render_pose's `accumulate`); the frame's stats go to on_frame as the keyword `accumulated` and its samples-per-pixel map
        # is kept in spp_maps.  It does not combine with scene_passes or an occluder.  Not in the reference (keyword-only, off by
        # default)
        self.accumulate = None
        if accumulate is not None:
            from stnerf_amd.accumulate import as_spec
            self.accumulate = as_spec(accumulate)
        self.spp_maps = []
        self._frame_stats = None
        # lens: an stnerf_amd.lens.Lens or the dict of its arguments -- the camera's lens for every frame of the path (render_pose's
        # `lens`): its distortion bends the rays, its aperture (with accumulate) gives depth of field.  on_frame and the stats are
        # unchanged.  Not in the reference (keyword-only, off by default)
        from stnerf_amd.lens import as_lens
        self.lens = as_lens(lens)
        # reproject: an stnerf_amd.reproject.ReprojectSpec or the dict of its arguments -- the background of every frame of
        # render_path / render_path_walking is warped from key plates at path indices 0, N, 2N, ... (N = key_every), rendered
        # lazily and dropped once passed; only the holes of the warp are rendered, and the finished plate is composited into the
        # scene with layer 0 hidden (render_pose's `reproject`).  Every frame goes through the plate path, the
        # keys included (at a key's own camera the warp is the identity), so the look does not pop between keys and in-betweens.
        # The frame's stats go to on_frame as the keyword `reprojected` and are kept in reproject_stats.  Approximate; it does not
        # combine with accumulate, an occluder or an enabled lens.  Not in the reference (keyword-only, off by default).
        # exclusive=True in the spec: no hole is rendered separately; one render call per frame evaluates the background only on the
        # rays whose plate row is absent (the per-ray background mask) -- one source of background per ray
        self.reproject = None
        if reproject is not None:
            from stnerf_amd.reproject import as_spec as as_reproject_spec
            self.reproject = as_reproject_spec(reproject)
            if self.accumulate is not None:
                raise ValueError("reproject= with accumulate=: plates for the passes of a progressive frame are out of scope")
            if self.occluder is not None:
                raise ValueError("reproject= with occluder=: the warped background is the frame's occluder plate and a call composites one")
            if self.lens is not None and self.lens.enabled:
                raise ValueError("reproject= with an enabled lens: the warp is a pinhole's")
            if self.scene_passes:
                raise ValueError("reproject= with scene_passes: layer 0 is hidden in a reprojected frame; its passes are in the stats")
        self.reproject_stats = []
        self._plates = {}
        # lattice: an stnerf_amd.lattice.LatticeSpec or the dict of its arguments -- every frame of render_path /
        # render_path_walking is rendered on a sparse lattice of pixels, refined where the corners of a cell disagree and
        # interpolated where they agree (render_pose's `lattice`).  The frame's stats go to on_frame as the
        # keyword `lattice` and are kept in lattice_stats (without the status map).  Approximate; it does not combine with
        # accumulate, reproject, scene_passes or an occluder.  Not in the reference (keyword-only, off by default)
        self.lattice = None
        if lattice is not None:
            from stnerf_amd.lattice import as_spec as as_lattice_spec
            self.lattice = as_lattice_spec(lattice)
            if self.accumulate is not None or self.reproject is not None:
                raise ValueError("lattice= with accumulate= or reproject=: a sparse frame of progressive passes or of warped plates is "
                                 "out of scope")
            if self.scene_passes or self.occluder is not None:
                raise ValueError("lattice= with scene_passes or occluder=: interpolating those passes is out of scope")
        self.lattice_stats = []
        # deep: an stnerf_amd.DeepSpec (or True): every frame also keeps its deep frame -- the per-pixel list of the final stage's
        # weighted samples, on which any number of depth-tested elements are composited after the render (render_pose's `deep`;
        # DESIGN.md section 7).  The frames are kept in deep_frames (on the device, in the render's own row order: inverse_y_axis does
        # not reorder a list) and handed to on_frame as the keyword `deep`.  It does not combine with accumulate, lattice, reproject
        # or occluder_stops.  Not in the reference (keyword-only, off by default)
        self.deep = None
        if deep is not None:
            from stnerf_amd.deep import as_spec as as_deep_spec
            self.deep = as_deep_spec(deep)
            for name, value in (("accumulate", self.accumulate), ("lattice", self.lattice), ("reproject", self.reproject)):
                if value is not None:
                    raise ValueError(f"deep= with {name}=: such a frame is not one sample list per pixel")
            if self.occluder_stops:
                raise ValueError("deep= with occluder_stops: the deep frame is of the scene without the occluder")
        self.deep_frames = []
        self.layer_num = cfg.DATASETS.LAYER_NUM
        self.frame_num = cfg.DATASETS.FRAME_NUM
        self.display_layers = {i: 1 for i in range(self.total_layers)}
        self.gt_poses = torch.as_tensor(gt_poses, dtype=torch.float32)
        self.gt_Ks = [torch.as_tensor(k, dtype=torch.float32) for k in gt_Ks]
        self.far = 20.0
        off = cfg.DATASETS.FRAME_OFFSET
        self.min_frame = [1 + off for _ in range(self.total_layers)]
        self.max_frame = [self.frame_num + off for _ in range(self.total_layers)]
        self.images, self.depths = [], []
        self.image_num = 0
        self.camera_num = self.gt_poses.shape[0]
        self.min_camera_id, self.max_camera_id = 0, self.camera_num - 1
        self.fps = 25
        self.height, self.width = cfg.INPUT.SIZE_TEST[1], cfg.INPUT.SIZE_TEST[0]
        self.save_count = 0
        self.poses: List = []
        self.Ks: List = []
        self.layer_frame_pairs: List = []
        self.trace_layer = -1
        self.dir_name = ''

    @property
    def total_layers(self):
        """l: the background, the cfg's performers and the model's layer instances (``duplicate_layer``)."""
        return int(getattr(self.model, "total_layers", self.layer_num + 1))

    def duplicate_layer(self, src, *, shift=None, scale=None, rotation=None, alpha=None):
        """Show performer ``src`` a second time -> the copy's layer id (``LayeredRFRender.add_instance``: the source's networks,
        no second copy of them).  The copy is a layer like any other: it starts with the source's frame span, and
        ``set_frame_duration(..., layer_id)`` / ``retime_by_key_frames(layer_id, ...)`` retime it on its own; ``shift``, ``scale``,
        ``rotation`` and ``alpha`` are its entries of the per-layer edit lists, which grow by one (a list that was None is created
        with neutral entries -- zero shift, scale 1, no rotation, opaque -- when the copy needs it; a list that already has an
        entry for the new layer, such as the start of an ``s_*`` schedule given with the final layer count, keeps it unless
        the argument names another).  Call it before any path setter: the (layer, frame) pairs of a path are laid out for
        the layers that exist then.  Not in the reference."""
        if self.layer_frame_pairs:
            raise RuntimeError("duplicate_layer after a path setter: the path's (layer, frame) pairs are already laid out -- "
                               "duplicate the layers first, then set the path")
        layer_id = self.model.add_instance(src)
        self.display_layers[layer_id] = 1
        self.min_frame = list(self.min_frame[:layer_id]) + [self.min_frame[src]]
        self.max_frame = list(self.max_frame[:layer_id]) + [self.max_frame[src]]

        def grown(cur, value, neutral):
            if cur is None and value is None:
                return None
            out = list(cur) if cur is not None else []
            out += [neutral() for _ in range(layer_id + 1 - len(out))]
            if value is not None:
                out[layer_id] = value
            return out
        self.shift = self.model.shift = grown(self.shift, shift, lambda: [0.0, 0.0, 0.0])
        self.scale = self.model.scale = grown(self.scale, scale, lambda: 1.0)
        self.rotation = self.model.rotation = grown(self.rotation, rotation, lambda: None)
        self.layer_alpha = self.model.layer_alpha = grown(self.layer_alpha, alpha, lambda: None)
        return layer_id

    @property
    def cache_background(self):
        """True while the model keeps the background's network outputs of a fixed view across frames
        (``LayeredRFRender.set_background_cache``: a time sweep from one camera -- ``set_path_fixed_gt_poses`` + retiming / the
        edit schedule -- then evaluates the background once; the frames are bit-identical to uncached ones and share one
        jitter pattern).  Setting it attaches a fresh ``stnerf_amd.BackgroundCache`` to the model or detaches it; not in the
        reference (keyword-only, off by default)."""
        return getattr(self.model, "_bkgd_cache", None) is not None

    @cache_background.setter
    def cache_background(self, on):
        if bool(on) != self.cache_background:
            from stnerf_amd.bkgd_cache import BackgroundCache
            self.model.set_background_cache(BackgroundCache() if on else None)

    @property
    def cache_layers(self):
        """True while the model keeps the performers' network outputs of a fixed view across frames
        (``LayeredRFRender.set_layer_cache``: from one camera, a performer whose own inputs did not change since its last two
        frames is copied in instead of evaluated -- nudging, retiming, fading or hiding ANOTHER layer, any ``layer_alpha``,
        ``bkgd_density_threshold`` (with retiming ``density_threshold`` is an input of a performer's fine samples: a sweep over it
        re-evaluates the performers); no performer is terminated while it is attached; the frames are bit-identical to uncached ones and share one jitter pattern).  Setting it attaches a
        fresh ``stnerf_amd.LayerCache`` to the model or detaches it; not in the reference (keyword-only, off by default)."""
        return getattr(self.model, "_layer_cache", None) is not None

    @cache_layers.setter
    def cache_layers(self, on):
        if bool(on) != self.cache_layers:
            from stnerf_amd.layer_cache import LayerCache
            self.model.set_layer_cache(LayerCache() if on else None)

    @property
    def occupancy(self):
        """The ``stnerf_amd.OccupancyGrids`` attached to the model, or None: while one is attached the performer rays that cross
        only empty cells of their performer's grid are culled before the networks run (``LayeredRFRender.set_occupancy``).
        Setting True attaches fresh grids with the defaults, ``"samples"`` fresh grids with ``samples=True`` (kept rays skip the
        samples in empty cells too), ``"background"`` fresh grids with ``background=True`` (the background skips its samples in
        empty cells of a grid over ``bkgd_bbox``), ``"samples+background"`` both, an ``OccupancyGrids`` attaches that one,
        False / None detaches; not in the reference (keyword-only, off by default)."""
        return getattr(self.model, "_occupancy", None)

    @occupancy.setter
    def occupancy(self, value):
        from stnerf_amd.occupancy import OccupancyGrids
        if isinstance(value, OccupancyGrids):
            self.model.set_occupancy(value)
        elif value is None or isinstance(value, bool):
            if bool(value) != (self.occupancy is not None):
                self.model.set_occupancy(OccupancyGrids() if value else None)
        elif isinstance(value, str) and value == "samples":
            if self.occupancy is None or not self.occupancy.samples:
                self.model.set_occupancy(OccupancyGrids(samples=True))
        elif isinstance(value, str) and value in ("background", "samples+background"):
            want = value == "samples+background"
            if self.occupancy is None or not self.occupancy.background or self.occupancy.samples != want:
                self.model.set_occupancy(OccupancyGrids(samples=want, background=True))
        else:
            raise TypeError("occupancy is False, True, \"samples\", \"background\", \"samples+background\" or an OccupancyGrids, "
                            f"got {value!r}")

    @property
    def proposal(self):
        """The ``stnerf_amd.ProposalGrids`` attached to the model, or None: while one is attached the flagged layers' coarse densities
        come from a grid of their own fine densities and their coarse networks do not run (``LayeredRFRender.set_proposal``).
        Setting True attaches fresh grids with the defaults (every shown performer, 128 cells a side), a ``ProposalGrids`` attaches
        that one, False / None detaches; not in the reference (keyword-only, off by default)."""
        return getattr(self.model, "_proposal", None)

    @proposal.setter
    def proposal(self, value):
        from stnerf_amd.proposal import ProposalGrids
        if isinstance(value, ProposalGrids):
            self.model.set_proposal(value)
        elif value is None or isinstance(value, bool):
            if bool(value) != (self.proposal is not None):
                self.model.set_proposal(ProposalGrids() if value else None)
        else:
            raise TypeError(f"proposal is False, True or a ProposalGrids, got {type(value).__name__}")

    @property
    def terminate(self):
        """The ``stnerf_amd.termination.Termination`` attached to the model, or None: while one is attached the fine samples that
        the coarse pass shows to lie behind an opaque stretch of the ray get zero outputs instead of a network evaluation
        (``LayeredRFRender.set_termination``).  Setting True attaches one with the defaults (tau 1e-4, every layer, the background
        too), a number one with that tau, a ``Termination`` attaches that one, False / None detaches; not in the reference
        (keyword-only, off by default)."""
        return getattr(self.model, "_termination", None)

    @terminate.setter
    def terminate(self, value):
        from stnerf_amd.termination import Termination
        if isinstance(value, Termination):
            self.model.set_termination(value)
        elif value is None or isinstance(value, bool):
            if bool(value) != (self.terminate is not None):
                self.model.set_termination(1e-4 if value else None)
        elif isinstance(value, float):
            self.model.set_termination(value)
        else:
            raise TypeError(f"terminate is False, True, a tau or a Termination, got {type(value).__name__}")

    # ---- layer display / knobs (:643-686, :740-741) ----------------------------------------------------
    def hide_layer(self, layer_id):
        self.model.hide_layer(layer_id)
        self.display_layers[layer_id] = 0

    def show_layer(self, layer_id):
        self.model.show_layer(layer_id)
        self.display_layers[layer_id] = 1

    def is_shown_layer(self, layer_id):
        return self.display_layers[layer_id] == 1

    def set_save_dir(self, dir_name):
        self.dir_name = dir_name

    def set_fps(self, fps):
        self.fps = fps

    def set_near(self, near):
        self.model.near = near

    def set_frame_duration(self, min_frame, max_frame, layer_id=-1):
        if layer_id == -1:
            self.min_frame = [min_frame for _ in range(self.total_layers)]
            self.max_frame = [max_frame for _ in range(self.total_layers)]
        else:
            self.min_frame[layer_id], self.max_frame[layer_id] = min_frame, max_frame

    def set_pose_duration(self, min_camera_id, max_camera_id):
        self.min_camera_id, self.max_camera_id = min_camera_id, max_camera_id

    def invert_poses(self):
        self.poses.reverse()
        self.Ks.reverse()

    def save_poses(self, path):
        np.save(path, self.poses)

    # ---- (layer, frame) bookkeeping shared by every path setter (:161-168, :180-186, ...) ----------------
    def _append_layer_frame_pairs(self, n_poses, smooth_time=False):
        for idx in range(n_poses + 1):
            pair = []
            for layer_id in range(self.total_layers):
                if self.is_shown_layer(layer_id):
                    span = (self.max_frame[layer_id] - self.min_frame[layer_id]) / n_poses * idx
                    frame_id = (span if smooth_time else int(span)) + self.min_frame[layer_id]
                    pair.append((layer_id, frame_id))
            self.layer_frame_pairs.append(pair)

    def _edit_schedule(self, n):
        """Linear per-frame schedules of the editing knobs (:232-243, :279-301).  A per-layer schedule has one entry per layer
        of ``total_layers`` (the layer instances included), else ValueError."""
        l = self.total_layers
        for name in ("s_shift", "s_scale", "s_rotation", "s_layer_alpha"):
            sched = getattr(self, name)
            if sched is not None and (len(sched[0]) != l or len(sched[1]) != l):
                raise ValueError(f"{name} must have one entry per layer ({l}, layer 0 = the background, layer instances included), "
                                 f"got {len(sched[0])} and {len(sched[1])}")
        if self.s_shift is not None:
            a, b = np.array(self.s_shift[0]), np.array(self.s_shift[1])
            step = (b - a) / (n - 1)
            self.s_shift_frame = [(a + i * step).tolist() for i in range(n)]
        if self.s_scale is not None:
            a, b = np.array(self.s_scale[0]), np.array(self.s_scale[1])
            step = (b - a) / (n - 1)
            self.s_scale_frame = [(a + i * step).tolist() for i in range(n)]
        if self.s_alpha is not None:
            a, b = self.s_alpha[0], self.s_alpha[1]
            step = (b - a) / (n - 1)
            self.s_alpha_frame = [(a + i * step) for i in range(n)]
        if self.s_rotation is not None:
            lerp = lambda a, b, i: None if a is None else a + i * ((b - a) / (n - 1))
            self.s_rotation_frame = [[lerp(a, b, i) for a, b in zip(*self.s_rotation)] for i in range(n)]
        if self.s_layer_alpha is not None:
            lerp = lambda a, b, i: None if a is None else a + i * ((b - a) / (n - 1))
            self.s_layer_alpha_frame = [[lerp(a, b, i) for a, b in zip(*self.s_layer_alpha)] for i in range(n)]

    # ---- camera paths ---------------------------------------------------------------------------------------
    def set_smooth_path_poses(self, step_num, around=False, smooth_time=False):
        """Slerp of the key rotations + cubic B-spline through the key camera centres, linear intrinsics
        (:230-319).  ``around=False`` keeps only the first and last rotation (:254-257)."""
        self._edit_schedule(step_num)
        lo, hi = self.min_camera_id, self.max_camera_id
        Rs = self.gt_poses[lo:hi + 1, :3, :3].cpu().numpy()
        Ts = self.gt_poses[lo:hi + 1, :3, 3].cpu().numpy()
        key_frames = [i for i in range(lo, hi + 1)]
        if not around:
            Rs = np.array([Rs[0], Rs[-1]])
            key_frames = [lo, hi]
        interp_frames = [(i * (hi - lo) / (step_num - 1) + lo) for i in range(step_num)]
        interp_Rs = Slerp(key_frames, R.from_matrix(Rs))(interp_frames).as_matrix()
        tck, _ = splprep([Ts[:, 0], Ts[:, 1], Ts[:, 2]])
        new_points = np.stack(splev([i / (step_num - 1) for i in range(step_num)], tck), axis=1)
        K0, K1 = self.gt_Ks[lo], self.gt_Ks[hi]
        poses = []
        for i in range(step_num):
            pose = np.zeros((4, 4))
            pose[:3, :3] = interp_Rs[i]
            pose[:3, 3] = new_points[i]
            pose[3, 3] = 1
            poses.append(pose)
            self.Ks.append((K1 - K0) * i / (step_num - 1) + K0)
        self.poses = self.poses + poses
        self._append_layer_frame_pairs(len(poses), smooth_time)

    def set_path_gt_poses(self):
        """One frame per ground-truth camera (:171-186)."""
        poses = [self.gt_poses[i] for i in range(self.gt_poses.shape[0])]
        self.poses = self.poses + poses
        self.Ks = self.Ks + self.gt_Ks
        self._append_layer_frame_pairs(len(poses))

    def set_path_fixed_gt_poses(self, id, num=None):
        """``num`` frames from ground-truth camera ``id`` (a time sweep from a fixed view, :188-228)."""
        self._edit_schedule(num)
        self.poses = self.poses + [self.gt_poses[id] for _ in range(num)]
        self.Ks = self.Ks + [self.gt_Ks[id] for _ in range(num)]
        self._append_layer_frame_pairs(num)

    def load_path_poses(self, poses):
        """Externally supplied poses, intrinsics lerped between the first and last-but-one camera (:321-337)."""
        self.poses = poses
        n = len(poses)
        K0, K1 = self.gt_Ks[self.min_camera_id], self.gt_Ks[self.max_camera_id - 1]
        for i in range(n):
            self.Ks.append((K1 - K0) * i / (n - 1) + K0)
        self._append_layer_frame_pairs(n)

    # ---- retiming (:495-545) ------------------------------------------------------------------------------
    def retime_by_key_frames(self, layer_id, key_frames_layer, key_frames):
        """Piecewise-linear remap of one layer's frame ids: global key frame key_frames[i] shows the layer's
        frame key_frames_layer[i]."""
        assert len(key_frames_layer) == len(key_frames)
        for i in range(len(self.layer_frame_pairs)):
            for j in range(len(self.layer_frame_pairs[i])):
                layer, frame = self.layer_frame_pairs[i][j]
                if layer != layer_id:
                    continue
                idx_start, idx_end, weight = -1, -1, 0
                for idx in range(len(key_frames)):
                    if frame <= key_frames[idx]:
                        idx_end, idx_start = idx, idx - 1
                        end = key_frames[idx]
                        start = self.min_frame[layer] if idx == 0 else key_frames[idx - 1]
                        weight = (frame - start) / (end - start)
                        break
                if idx_start == -1 and idx_end == 0:
                    weight = (frame - self.min_frame[layer]) / (key_frames[0] - self.min_frame[layer])
                    new_start, new_end = self.min_frame[layer], key_frames_layer[0]
                elif idx_start >= -1 and idx_end != -1:
                    new_start, new_end = key_frames_layer[idx_start], key_frames_layer[idx_start + 1]
                elif idx_start == -1 and idx_end == -1:
                    weight = (frame - key_frames[-1]) / (self.max_frame[layer] - key_frames[-1])
                    new_start, new_end = key_frames_layer[-1], self.max_frame[layer]
                else:
                    raise RuntimeError(f"Undefined branch: start idx {idx_start}, end idx {idx_end}")  # exit(-1), :537-539
                self.layer_frame_pairs[i][j] = (layer, round(weight * (new_end - new_start) + new_start))

    # ---- rendering -------------------------------------------------------------------------------------------
    def render_pose(self, pose, K, layer_frame_pair, density_threshold=0, bkgd_density_threshold=0, scene_passes=False, occluder=None,
                    accumulate=None, lens=None, reproject=None, lattice=None, deep=None):
        """-> color (H,W,3), depth (H,W,1), color_layer, depth_layer on the device (:364-391); with ``scene_passes`` a fifth
        element, the dict of in-scene layer passes (stnerf_amd.render.render_pose); with ``occluder`` = (rgba, depth) that dict
        also holds the occluded results; with ``accumulate`` = a spec the frame is a progressive multi-sample one and the fifth
        element is its ``stats``.  ``lens``: the camera's lens for this frame (default: the renderer's ``lens``).
        ``reproject`` = (spec, plates): the background is warped from those key plates (stnerf_amd.render.render_pose); the fifth
        element is the frame's ``stats``.  ``lattice`` = a spec: the frame is an adaptive lattice one and the fifth element is its
        ``stats``.  ``deep`` = a ``DeepSpec``: the fifth element is the passes dict with ``deep``, the frame's ``DeepFrame``."""
        lens = self.lens if lens is None else lens
        return _render_pose(self.model, pose, K, self.height, self.width, layer_frame_pair, self.far, density_threshold,
                            bkgd_density_threshold, **(dict(scene_passes=True) if scene_passes else {}),
                            **(dict(occluder=occluder, occluder_stops=self.occluder_stops) if occluder is not None else {}),
                            **(dict(accumulate=accumulate) if accumulate is not None else {}),
                            **(dict(lens=lens) if lens is not None else {}),
                            **(dict(reproject=reproject) if reproject is not None else {}),
                            **(dict(lattice=lattice) if lattice is not None else {}),
                            **(dict(deep=deep) if deep is not None else {}))

    def _key_plates(self, idx, density_threshold, bkgd_density_threshold):
        """The key plates frame ``idx`` uses (``ReprojectSpec.keys_of``) -> (plates, how many were rendered for this frame).  A
        key is rendered on first use, at its own pose, under the model's state and frame ids of the frame that needs it; one whose
        identity differs from this frame's (a time-dependent background, an edit of layer 0) is rendered again -- re-keyed; keys
        the path has passed are dropped."""
        from stnerf_amd.reproject import BackgroundPlate, background_identity
        keys = self.reproject.keys_of(idx, len(self.poses))
        for k in [k for k in self._plates if k < keys[0]]:
            del self._plates[k]
        frame_ids = [0.0] * self.total_layers
        for layer_id, frame_id in self.layer_frame_pairs[idx]:
            frame_ids[layer_id] = float(frame_id)
        ident = background_identity(self.model, frame_ids, self.height, self.width, 512 * 7, density_threshold, bkgd_density_threshold)
        rendered = 0
        for k in keys:
            plate = self._plates.get(k)
            if plate is None or plate.identity != ident:
                self._plates[k] = BackgroundPlate.render(self.model, self.Ks[k], self.poses[k], self.height, self.width, frame_ids,
                                                         self.reproject, density_threshold, bkgd_density_threshold, index=k)
                rendered += 1
        return [self._plates[k] for k in keys], rendered

    def _render_frame(self, idx, density_threshold, bkgd_density_threshold, inverse_y_axis):
        """Frame ``idx`` of the path -> (color, depth, color_layer, depth_layer, passes): ``render_pose``, flipped on request;
        ``passes`` is None unless ``scene_passes`` is on or the frame has an occluder (then ``render_pose``'s dict, flipped
        alike)."""
        passes = None
        self._frame_stats = None
        occ = self.occluder(idx, self.poses[idx], self.Ks[idx]) if self.occluder is not None else None
        if self.reproject is not None:
            plates, rendered = self._key_plates(idx, density_threshold, bkgd_density_threshold)
            color, depth, color_layer, depth_layer, stats = self.render_pose(self.poses[idx], self.Ks[idx], self.layer_frame_pairs[idx],
                                                                            density_threshold, bkgd_density_threshold,
                                                                            reproject=(self.reproject, plates))
            stats = dict(stats, keys_rendered=rendered, rays_keys=rendered * self.height * self.width)
            if inverse_y_axis:
                flip = lambda v: torch.flip(v, [0]) if torch.is_tensor(v) else type(v)(flip(i) for i in v)
                stats["passes"] = {k: flip(v) for k, v in stats["passes"].items()}
            self._frame_stats = stats
            self.reproject_stats.append({k: v for k, v in stats.items() if k != "passes"})
        elif self.accumulate is not None:
            color, depth, color_layer, depth_layer, stats = self.render_pose(self.poses[idx], self.Ks[idx], self.layer_frame_pairs[idx],
                                                                            density_threshold, bkgd_density_threshold,
                                                                            scene_passes=self.scene_passes, occluder=occ,
                                                                            accumulate=self.accumulate)
            if inverse_y_axis:
                stats = dict(stats, spp=torch.flip(stats["spp"], [0]), variance=torch.flip(stats["variance"], [0]))
            self._frame_stats = stats
        elif self.lattice is not None:
            color, depth, color_layer, depth_layer, stats = self.render_pose(self.poses[idx], self.Ks[idx], self.layer_frame_pairs[idx],
                                                                            density_threshold, bkgd_density_threshold,
                                                                            lattice=self.lattice)
            if inverse_y_axis:
                stats = dict(stats, status=torch.flip(stats["status"], [0]))
            self._frame_stats = stats
            self.lattice_stats.append({k: v for k, v in stats.items() if k != "status"})
        elif self.scene_passes or occ is not None or self.deep is not None:
            color, depth, color_layer, depth_layer, passes = self.render_pose(self.poses[idx], self.Ks[idx],
                                                                             self.layer_frame_pairs[idx], density_threshold,
                                                                             bkgd_density_threshold, scene_passes=True,
                                                                             **(dict(occluder=occ) if occ is not None else {}),
                                                                             **(dict(deep=self.deep) if self.deep is not None else {}))
            self._deep_frame = passes.pop("deep", None)
            if self._deep_frame is not None:
                self.deep_frames.append(self._deep_frame)
        else:
            color, depth, color_layer, depth_layer = self.render_pose(self.poses[idx], self.Ks[idx],
                                                                     self.layer_frame_pairs[idx], density_threshold,
                                                                     bkgd_density_threshold)
        if inverse_y_axis:
            color, depth = torch.flip(color, [0]), torch.flip(depth, [0])
            color_layer = [torch.flip(i, [0]) for i in color_layer]
            depth_layer = [torch.flip(i, [0]) for i in depth_layer]
            if passes is not None:
                flip = lambda v: torch.flip(v, [0]) if torch.is_tensor(v) else type(v)(flip(i) for i in v)
                passes = {k: flip(v) for k, v in passes.items()}
        return color, depth, color_layer, depth_layer, passes

    def _frame_keywords(self, passes):
        """on_frame's keywords beyond the reference's five arguments: ``scene`` with ``scene_passes``, ``occluded`` with an
        ``occluder`` (the frame's occluded entries of the dict, or None where the callable gave none)."""
        kw = dict(scene=passes) if self.scene_passes else {}
        if self.accumulate is not None:
            kw["accumulated"] = self._frame_stats
        if self.reproject is not None:
            kw["reprojected"] = self._frame_stats
        if self.lattice is not None:
            kw["lattice"] = self._frame_stats
        if self.deep is not None:
            kw["deep"] = self._deep_frame
        if self.occluder is not None:
            has = passes is not None and "color_occluded" in passes
            kw["occluded"] = {k: v for k, v in passes.items() if "occlude" in k} if has else None
        return kw

    def _keep_occluded(self, passes):
        if passes is not None and "color_occluded" in passes:
            self.images_occluded.append(passes["color_occluded"].cpu())

    def _keep_spp(self):
        if self._frame_stats is not None and "spp" in self._frame_stats:
            self.spp_maps.append(self._frame_stats["spp"].cpu())

    def _keep_scene(self, passes, layer_id):
        self.images_scene[layer_id].append(passes["color_scene"][layer_id].cpu())
        self.alphas_scene[layer_id].append(passes["alpha_scene"][layer_id].cpu())

    def render_path(self, inverse_y_axis=False, density_threshold=0, bkgd_density_threshold=0, auto_save=True,
                    on_frame: Optional[Callable] = None):
        """Render every pose of the path with its (layer, frame) pairs and edit schedule (:401-488).  With
        ``auto_save`` the frames are kept in ``self.images`` / ``self.depths`` (CPU tensors, as the reference
        keeps them for ``save_video``); ``on_frame(idx, color, depth, color_layer, depth_layer)`` is called with
        the device tensors (write files there); with ``scene_passes`` it also gets ``scene=`` the frame's dict of in-scene layer
        passes, which are kept in ``self.images_scene`` / ``self.alphas_scene`` next to ``images_layer``; with ``accumulate`` every
        frame is a progressive multi-sample one, ``on_frame`` gets ``accumulated=`` its stats (spp and variance maps flipped with
        the images) and the samples-per-pixel maps are kept in ``self.spp_maps``."""
        self.images, self.depths = [], []
        self.images_layer = [[] for _ in range(self.total_layers)]
        self.depths_layer = [[] for _ in range(self.total_layers)]
        self.images_scene = [[] for _ in range(self.total_layers)]
        self.alphas_scene = [[] for _ in range(self.total_layers)]
        self.images_occluded = []
        self.spp_maps = []
        self.reproject_stats, self._plates = [], {}
        self.lattice_stats = []
        self.image_num = 0
        for idx in range(len(self.poses)):
            if self.s_shift is not None:
                self.model.shift = self.s_shift_frame[idx]
            if self.s_scale is not None:
                self.model.scale = self.s_scale_frame[idx]
            if self.s_alpha is not None:
                self.model.alpha = self.s_alpha_frame[idx]
            if self.s_rotation is not None:
                self.model.rotation = self.s_rotation_frame[idx]
            if self.s_layer_alpha is not None:
                self.model.layer_alpha = self.s_layer_alpha_frame[idx]
            color, depth, color_layer, depth_layer, passes = self._render_frame(idx, density_threshold, bkgd_density_threshold,
                                                                                inverse_y_axis)
            if on_frame is not None:
                on_frame(idx, color, depth, color_layer, depth_layer, **self._frame_keywords(passes))
            if auto_save:
                self.images.append(color.cpu())
                self.depths.append(depth.cpu())
                self._keep_occluded(passes)
                self._keep_spp()
                for layer_id in range(self.total_layers):
                    if self.is_shown_layer(layer_id):
                        self.images_layer[layer_id].append(color_layer[layer_id].cpu())
                        self.depths_layer[layer_id].append(depth_layer[layer_id].cpu())
                        if passes is not None and self.scene_passes:
                            self._keep_scene(passes, layer_id)
            self.image_num += 1
        return self.images, self.depths

    def render_path_walking(self, inverse_y_axis=False, density_threshold=0, bkgd_density_threshold=0, auto_save=True,
                            on_frame: Optional[Callable] = None):
        """``render_path`` without the per-frame edit schedule plus the occlusion composite of the walking demo
        (:550-618): layer 2 is pasted over the background image wherever it is in front of it
        (``depth_layer[2] < depth_layer[0]``) and has colour.  The composites are kept in ``self.images_hide``.  That paste is a
        per-pixel depth test on images composited alone; with ``scene_passes`` the layers' shares of the mixed image, with the
        compositor's own occlusion, are kept in ``self.images_scene`` / ``self.alphas_scene`` and given to ``on_frame`` as ``scene=``
        (``color_hide`` stays the reference's computation)."""
        self.images, self.depths, self.images_hide = [], [], []
        self.images_layer = [[] for _ in range(self.total_layers)]
        self.depths_layer = [[] for _ in range(self.total_layers)]
        self.images_scene = [[] for _ in range(self.total_layers)]
        self.alphas_scene = [[] for _ in range(self.total_layers)]
        self.images_occluded = []
        self.spp_maps = []
        self.reproject_stats, self._plates = [], {}
        self.lattice_stats = []
        self.image_num = 0
        for idx in range(len(self.poses)):
            color, depth, color_layer, depth_layer, passes = self._render_frame(idx, density_threshold, bkgd_density_threshold,
                                                                                inverse_y_axis)
            color_hide = None
            if self.layer_num >= 2:
                color_hide = color_layer[0].clone()                                   # :606-611
                index = depth_layer[2] < depth_layer[0]
                index = torch.cat([index, index, index], dim=2)
                index = torch.logical_and(index, color_layer[2] != 0)
                color_hide[index] = color_layer[2][index]
            if on_frame is not None:
                on_frame(idx, color, depth, color_layer, depth_layer, **self._frame_keywords(passes))
            if auto_save:
                self.images.append(color.cpu())
                self.depths.append(depth.cpu())
                if color_hide is not None:
                    self.images_hide.append(color_hide.cpu())
                self._keep_occluded(passes)
                self._keep_spp()
                for layer_id in range(self.total_layers):
                    self.images_layer[layer_id].append(color_layer[layer_id].cpu())
                    self.depths_layer[layer_id].append(depth_layer[layer_id].cpu())
                    if passes is not None and self.scene_passes:
                        self._keep_scene(passes, layer_id)
            self.image_num += 1
        return self.images, self.depths

    def save_video(self, writer: Optional[Callable] = None):
        """The reference writes ``color_<n>.mp4`` / ``depth_<n>.mp4`` with imageio (:624-637); imageio is not a
        dependency here, so the frames are handed to ``writer(kind, index, frames, fps)`` (``kind`` in
        {"color", "depth"}), e.g. ``lambda kind, i, frames, fps: imageio.mimwrite(f"{kind}_{i}.mp4", frames, fps=fps,
        quality=8)``.  As in the reference an empty renderer only warns."""
        if len(self.images) == 0:
            print("Warning: Cannot generate video for all rendered images, data is empty.")
            return False
        if writer is None:
            raise NotImplementedError("pass writer=...: video encoding (imageio) is outside the MI355X hot path")
        writer("color", self.save_count, self.images, self.fps)
        writer("depth", self.save_count, self.depths, self.fps)
        self.save_count += 1
        return True
