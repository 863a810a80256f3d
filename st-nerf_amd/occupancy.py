"""Occupancy grids: cull the performer rays that cross only empty space.

Every ray that hits a performer's box pays ``2 n1 + n2`` network evaluations for that performer although most of a box is air.
A grid holds one bit per cell of the box (include/stnerf.h: stnerf_occupancy; DESIGN.md section 7 states the format and the
rules); between the coarse sampler and the ray compaction the library clears the hit bit of every (ray, performer) pair none of
whose coarse sample points lies in an occupied cell (csrc/occupancy.hip).  Such a pair costs nothing in either network stage and
is treated like a ray that grazes the box.  A kept pair is untouched.

``LayeredRFRender.density_grid`` evaluates the networks' own densities at the grid's vertices; this module owns the bit tables,
as ``BackgroundCache`` owns its tensors.  Attach with ``model.set_occupancy(OccupancyGrids())`` or
``LayeredNeuralRenderer(..., occupancy=True)``.  Inference only.
"""
from __future__ import annotations

import hashlib
from collections import OrderedDict
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

MAX_RES, MAX_DILATE = 256, 4


class Grid(NamedTuple):
    bits: torch.Tensor          # int32 words holding the uint32 bits, on the device
    res: Tuple[int, int, int]   # (Rx, Ry, Rz)
    lo: np.ndarray              # fp32 (3,)
    hi: np.ndarray
    inv_cell: np.ndarray        # fp32 (3,): (float)R / (hi - lo)

    def entry(self):
        """The layer's entry of the table ``ops.occupancy_cull`` / ``ops.render_rays`` take."""
        return self.bits, self.res, self.lo.tolist(), self.inv_cell.tolist()


def normalise_res(res) -> Tuple[int, int, int]:
    """An int or (Rx, Ry, Rz) -> (Rx, Ry, Rz), each 1..256."""
    r = (int(res),) * 3 if isinstance(res, int) else tuple(int(x) for x in res)
    if len(r) != 3 or min(r) < 1 or max(r) > MAX_RES:
        raise ValueError(f"occupancy grid res must be 1..{MAX_RES} cells per axis, one number or (Rx, Ry, Rz), got {res!r}")
    return r


def box_bounds(box) -> Tuple[np.ndarray, np.ndarray]:
    """lo, hi (fp32): the axis-aligned bounds of a box's 8 corners."""
    b = torch.as_tensor(box).detach().to("cpu", torch.float32).reshape(-1, 3).numpy()
    return b.min(0), b.max(0)


def inv_cell(res, lo, hi) -> np.ndarray:
    """(float)R_a / (hi_a - lo_a), fp32 -- computed once on the host."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise ValueError(f"occupancy grid bounds must be finite with lo < hi on every axis, got lo {lo.tolist()}, hi {hi.tolist()}")
    return (np.asarray(res, np.float32) / (hi - lo)).astype(np.float32)


def vertex_coordinates(res, lo, hi):
    """Per axis the fp32 coordinates of the R_a + 1 vertices: lo_a + j ((hi_a - lo_a) / R_a), vertex R_a = hi_a itself."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    out = []
    for a in range(3):
        step = np.float32((hi[a] - lo[a]) / np.float32(res[a]))
        v = (lo[a] + np.arange(res[a] + 1, dtype=np.float32) * step).astype(np.float32)
        v[-1] = hi[a]
        out.append(v)
    return out


def pack_bits(occupied) -> np.ndarray:
    """A bool array [Rz][Ry][Rx] -> the uint32 words of the table: cell c = (z Ry + y) Rx + x at bit c & 31 of word c >> 5."""
    flat = np.ascontiguousarray(np.asarray(occupied, dtype=bool)).reshape(-1)
    pad = (-flat.size) % 32
    b = np.packbits(np.concatenate([flat, np.zeros(pad, bool)]), bitorder="little")
    return b.view("<u4").astype(np.uint32)


class OccupancyGrids:
    """The bit tables of a model's performer layers.

    ``res``, ``threshold``, ``dilate``: the grid a layer gets from the model's own networks -- ``res`` cells per axis (a number
    or (Rx, Ry, Rz)), a vertex dense when ``!(sigma <= threshold)`` in the coarse or the fine SpaceNet, the occupied set grown by
    ``dilate`` cells.  ``threshold`` defaults to ``render_rays``'s own default ``density_threshold``: with retiming the render
    zeroes such densities anyway.  profiles/occupancy_ab.md has the sweep behind ``res`` and ``dilate``.
    Built grids are keyed by the module index, the frame id, the bytes of lo / hi, res, threshold, dilate, the parameter versions
    of the layer's three networks and the model flags; at most ``max_grids`` are kept, least recently used first out.
    ``auto=False``: only layers given a manual grid (``set_manual``) are culled.
    ``samples=True``: every layer that is ray-culled is sample-culled too -- on a kept ray only the samples whose point lies in
    an occupied cell reach the networks, in both stages; the others get exact zero outputs (the sample
    cull).  Off by default: a grid that is right for whole rays (one occupied sample keeps the ray) can still be too tight for
    single samples, see profiles/sample_cull_ab.md.
    ``background=True``: the background (layer 0) gets a grid of its own over the unedited ``bkgd_bbox`` and is SAMPLE-culled with
    it in every stage it is evaluated in (the background's grid): on every ray, mask or not, only the samples
    whose point lies in an occupied cell reach ``bkgd_net`` / ``bkgd_net_fine``; the others get exact zero outputs.  The grid is
    built like a performer's, at ``background_res`` cells per axis (None: ``res``), or given with ``set_background_manual``, which
    switches the cull on by itself.  Never ray-culled: ``set_manual(0, ...)`` keeps raising.  Off by default: it changes the picture
    wherever the grid calls a cell empty that holds density, see profiles/background_grid_ab.md."""

    def __init__(self, res=64, threshold: float = 1e-4, dilate: int = 0, max_grids: int = 64, auto: bool = True, samples: bool = False,
                 background: bool = False, background_res=None):
        self.res = normalise_res(res)
        self.threshold = float(threshold)
        if self.threshold != self.threshold:
            raise ValueError("occupancy threshold is NaN")
        if isinstance(dilate, bool) or int(dilate) != dilate or not 0 <= int(dilate) <= MAX_DILATE:
            raise ValueError(f"occupancy dilate must be an integer 0..{MAX_DILATE}, got {dilate!r}")
        self.dilate = int(dilate)
        if int(max_grids) < 1:
            raise ValueError(f"max_grids must be at least 1, got {max_grids!r}")
        self.max_grids = int(max_grids)
        self.auto = bool(auto)
        if not isinstance(samples, bool):
            raise TypeError(f"samples is False or True, got {samples!r}")
        self.samples = samples
        if not isinstance(background, bool):
            raise TypeError(f"background is False or True, got {background!r}")
        self.background = background
        self.background_res = None if background_res is None else normalise_res(background_res)
        self._bkgd_manual = None     # (uint32 words (host), res, lo, hi, inv_cell, {device: Grid}) or None
        self._bkgd_counts = None     # int64 (2,) on the device: (background samples tested, not listed), by the background's rows kernel
        self._bkgd = [0, 0]          # what stats() has taken off them so far
        self._sample_counts = None   # int64 (MAX_LAYERS, 2) on the device: (samples tested, samples skipped), by the rows kernel
        self._samples = {}           # layer id -> [tested, skipped]: what stats() has taken off them so far
        self._built: "OrderedDict[tuple, Grid]" = OrderedDict()
        self._manual = {}            # layer id -> (uint32 words (host), res, lo, hi, inv_cell, {device: Grid})
        self._counts = None          # int32 (MAX_LAYERS, 2) on the device: (pairs tested, pairs culled), accumulated by the cull
        self._pairs = {}             # layer id -> [tested, culled]: what stats() has taken off the device counters so far
        self.built = self.reused = 0

    # ---- manual grids ---------------------------------------------------------------------------------
    def set_manual(self, layer_id: int, occupied, lo=None, hi=None) -> None:
        """Use ``occupied`` (bool [Rz][Ry][Rx]) over the bounds lo, hi for layer ``layer_id`` at every frame id, as given (no
        threshold, no dilation); ``None`` clears it.  For a caller with a mask of their own."""
        if isinstance(layer_id, bool) or int(layer_id) != layer_id or int(layer_id) < 1:
            raise ValueError(f"layer {layer_id!r} cannot carry an occupancy grid: the background (layer 0) runs on every ray whatever "
                             "its mask; grids belong to layers >= 1")
        if occupied is None:
            self._manual.pop(int(layer_id), None)
            return
        occ = torch.as_tensor(occupied)
        if occ.dtype != torch.bool or occ.dim() != 3:
            raise ValueError(f"a manual occupancy grid is a bool tensor [Rz][Ry][Rx], got {occ.dtype} of shape {tuple(occ.shape)}")
        res = normalise_res((occ.shape[2], occ.shape[1], occ.shape[0]))
        if lo is None or hi is None:
            raise ValueError("a manual occupancy grid needs its bounds lo, hi")
        lo, hi = np.asarray(lo, np.float32).reshape(-1), np.asarray(hi, np.float32).reshape(-1)
        inv = inv_cell(res, lo, hi)
        self._manual[int(layer_id)] = (pack_bits(occ.detach().cpu().numpy()), res, lo.copy(), hi.copy(), inv, {})

    def set_background_manual(self, occupied, lo=None, hi=None) -> None:
        """Use ``occupied`` (bool [Rz][Ry][Rx]) over the bounds lo, hi as the background's grid at every frame id, as given (no
        threshold, no dilation); ``None`` clears it.  A manual grid sample-culls the background whatever ``background`` says."""
        if occupied is None:
            self._bkgd_manual = None
            return
        occ = torch.as_tensor(occupied)
        if occ.dtype != torch.bool or occ.dim() != 3:
            raise ValueError(f"a manual occupancy grid is a bool tensor [Rz][Ry][Rx], got {occ.dtype} of shape {tuple(occ.shape)}")
        res = normalise_res((occ.shape[2], occ.shape[1], occ.shape[0]))
        if lo is None or hi is None:
            raise ValueError("a manual occupancy grid needs its bounds lo, hi")
        lo, hi = np.asarray(lo, np.float32).reshape(-1), np.asarray(hi, np.float32).reshape(-1)
        inv = inv_cell(res, lo, hi)
        self._bkgd_manual = (pack_bits(occ.detach().cpu().numpy()), res, lo.copy(), hi.copy(), inv, {})

    def has_background(self) -> bool:
        """The background is sample-culled: ``background=True`` or a manual background grid."""
        return self.background or self._bkgd_manual is not None

    @staticmethod
    def background_timed(model) -> bool:
        """The background's frame id is an input of its density: BKGD_USE_DEFORM_TIME, or BKGD_USE_SPACE_TIME under USE_SPACE_TIME."""
        return bool(model.bkgd_use_deform_time or (model.bkgd_use_space_time and model.use_space_time))

    def background_key(self, model, frame_id, lo, hi):
        """The key of a built background grid: lo / hi bytes, res, threshold, dilate, the parameter versions of the background
        networks (``bkgd_time_deform_net`` when it is used), the background model flags, and the frame id only where the flags make
        it an input."""
        from stnerf_amd.modeling._packed import _params_fingerprint
        nets = [model.bkgd_spacenet, model.bkgd_spacenet_fine] + ([model.bkgd_time_deform_net] if model.bkgd_use_deform_time else [])
        return ("bkgd", float(frame_id) if self.background_timed(model) else None, np.asarray(lo, np.float32).tobytes(),
                np.asarray(hi, np.float32).tobytes(), self.background_res or self.res, self.threshold, self.dilate,
                tuple(_params_fingerprint(m) for m in nets),
                (bool(model.bkgd_use_deform_time), bool(model.bkgd_use_space_time), bool(model.use_space_time), bool(model.deep_rgb)))

    def background_grid(self, model, frame_id, device) -> Grid:
        """The background's grid at ``frame_id``: its manual grid, a built one from the store, or a fresh build over the unedited
        ``bkgd_bbox`` (``model.density_grid(0, ...)`` of both background networks -> ``ops.occupancy_build``)."""
        from stnerf_amd import ops
        if self._bkgd_manual is not None:
            words, res, lo, hi, inv, per_device = self._bkgd_manual
            g = per_device.get(str(device))
            if g is None:
                g = per_device[str(device)] = Grid(torch.from_numpy(words.view(np.int32).copy()).to(device), res, lo, hi, inv)
            return g
        res = self.background_res or self.res
        lo, hi = box_bounds(model.bkgd_bbox)
        key = self.background_key(model, frame_id, lo, hi) + (str(device),)
        g = self._built.get(key)
        if g is not None:
            self._built.move_to_end(key)
            self.reused += 1
            return g
        sig_c, _, _ = model.density_grid(0, frame_id, res, fine=False)
        sig_f = None
        if model.bkgd_spacenet_fine is not model.bkgd_spacenet:
            sig_f, _, _ = model.density_grid(0, frame_id, res, fine=True)
        bits = ops.occupancy_build(sig_c, sig_f, self.threshold, self.dilate)
        g = self._built[key] = Grid(bits, res, lo, hi, inv_cell(res, lo, hi))
        self.built += 1
        while len(self._built) > self.max_grids:
            self._built.popitem(last=False)
        return g

    def _bkgd_digest(self) -> int:
        words, res, lo, hi, _, _ = self._bkgd_manual
        h = hashlib.sha256(repr(("bkgd", res)).encode() + lo.tobytes() + hi.tobytes() + words.tobytes())
        return int.from_bytes(h.digest()[:6], "little")

    def background_identity(self):
        """What ``background_cache_key`` gains while the background is culled (None otherwise): a built grid's res / threshold /
        dilate -- everything else it is made of is in that key already -- or a manual grid's digest."""
        if self._bkgd_manual is not None:
            return ("background grid", "manual", self._bkgd_digest())
        if self.background:
            return ("background grid", "built", self.background_res or self.res, self.threshold, self.dilate)
        return None

    def background_counts(self, device) -> torch.Tensor:
        """The device counters the background's rows kernel accumulates into: int64 (2,)."""
        if self._bkgd_counts is None or self._bkgd_counts.device != torch.device(device):
            self._bkgd_counts = torch.zeros(2, dtype=torch.int64, device=device)
        return self._bkgd_counts

    def manual_layers(self):
        return sorted(self._manual)

    def _manual_grid(self, layer_id, device) -> Grid:
        words, res, lo, hi, inv, per_device = self._manual[layer_id]
        g = per_device.get(str(device))
        if g is None:
            bits = torch.from_numpy(words.view(np.int32).copy()).to(device)
            g = per_device[str(device)] = Grid(bits, res, lo, hi, inv)
        return g

    # ---- the table of a launch ------------------------------------------------------------------------
    def culled_layers(self, model):
        """The layers a render of ``model`` culls: shown performers (and instances) with a manual grid, or all of them."""
        return [i for i in range(1, model.total_layers) if model.is_shown_layer(i) and (self.auto or i in self._manual)]

    def key(self, model, layer_id, frame_id, lo, hi):
        from stnerf_amd.modeling._packed import _params_fingerprint
        j = model._module_index(layer_id)
        nets = [model.spacenets[j], model.spacenets_fine[j]] + ([model.time_deform_nets[j]] if model.use_deform_time else [])
        return (j, float(frame_id), np.asarray(lo, np.float32).tobytes(), np.asarray(hi, np.float32).tobytes(), self.res, self.threshold,
                self.dilate, tuple(_params_fingerprint(m) for m in nets),
                (bool(model.use_deform_time), bool(model.use_space_time), bool(model.deep_rgb)))

    def grid(self, model, layer_id, frame_id, device, retiming=True) -> Grid:
        """Layer ``layer_id``'s grid at ``frame_id``: its manual grid, a built one from the store, or a fresh build."""
        from stnerf_amd import ops
        if layer_id in self._manual:
            return self._manual_grid(layer_id, device)
        lo, hi = box_bounds(model.layer_box_at(layer_id, frame_id, retiming))
        key = self.key(model, layer_id, frame_id, lo, hi) + (str(device),)
        g = self._built.get(key)
        if g is not None:
            self._built.move_to_end(key)
            self.reused += 1
            return g
        sig_c, _, _ = model.density_grid(layer_id, frame_id, self.res, fine=False, retiming=retiming)
        j = model._module_index(layer_id)
        sig_f = None
        if model.spacenets_fine[j] is not model.spacenets[j]:
            sig_f, _, _ = model.density_grid(layer_id, frame_id, self.res, fine=True, retiming=retiming)
        bits = ops.occupancy_build(sig_c, sig_f, self.threshold, self.dilate)
        g = self._built[key] = Grid(bits, self.res, lo, hi, inv_cell(self.res, lo, hi))
        self.built += 1
        while len(self._built) > self.max_grids:
            self._built.popitem(last=False)
        return g

    def table(self, model, frame_ids, device, retiming=True):
        """-> (per layer None | table entry, the Grids in use): one grid per culled layer, at that layer's frame id."""
        l = model.total_layers
        grids = [None] * l
        for i in self.culled_layers(model):
            grids[i] = self.grid(model, i, frame_ids[i], device, retiming)
        return [None if g is None else g.entry() for g in grids], grids

    def counts(self, device) -> torch.Tensor:
        """The device counters the cull accumulates into: int32 (MAX_LAYERS, 2)."""
        from stnerf_amd import hip
        if self._counts is None or self._counts.device != torch.device(device):
            self._counts = torch.zeros(hip.MAX_LAYERS, 2, dtype=torch.int32, device=device)
        return self._counts

    def sample_counts(self, device) -> torch.Tensor:
        """The device counters the sample cull accumulates into: int64 (MAX_LAYERS, 2)."""
        from stnerf_amd import hip
        if self._sample_counts is None or self._sample_counts.device != torch.device(device):
            self._sample_counts = torch.zeros(hip.MAX_LAYERS, 2, dtype=torch.int64, device=device)
        return self._sample_counts

    # ---- bookkeeping ----------------------------------------------------------------------------------
    def __len__(self):
        return len(self._built)

    def clear(self) -> None:
        """Drop every built grid (manual grids and the statistics stay)."""
        self._built.clear()

    def reset_stats(self) -> None:
        self.built = self.reused = 0
        self._pairs = {}
        self._samples = {}
        self._bkgd = [0, 0]
        if self._bkgd_counts is not None:
            self._bkgd_counts.zero_()
        if self._counts is not None:
            self._counts.zero_()
        if self._sample_counts is not None:
            self._sample_counts.zero_()

    def stats(self) -> dict:
        """built / reused grid counts and, per layer that was tested, (pairs tested, pairs culled) since the last
        ``reset_stats()``: one device-to-host copy, made only here.  The device counters are 32 bits wide and only the
        statistics depend on them: ``stats()`` moves them into Python integers and zeroes them, so ask (or ``reset_stats()``)
        before a layer has been tested 2^31 times -- about a thousand 1080p frames of a performer that fills the picture.
        ``samples``: per layer that was sample-culled, (samples tested, samples skipped) over both stages (64-bit counters).
        ``background``: (background samples tested, skipped) over both stages (64-bit counters)."""
        if self._counts is not None:
            for i, (t, c) in enumerate(self._counts.cpu().tolist()):
                if t:
                    held = self._pairs.setdefault(i, [0, 0])
                    held[0] += int(t)
                    held[1] += int(c)
            self._counts.zero_()
        if self._sample_counts is not None:
            for i, (t, c) in enumerate(self._sample_counts.cpu().tolist()):
                if t:
                    held = self._samples.setdefault(i, [0, 0])
                    held[0] += int(t)
                    held[1] += int(c)
            self._sample_counts.zero_()
        if self._bkgd_counts is not None:
            t, c = self._bkgd_counts.cpu().tolist()
            self._bkgd[0] += int(t)
            self._bkgd[1] += int(c)
            self._bkgd_counts.zero_()
        return dict(built=self.built, reused=self.reused, pairs={i: tuple(v) for i, v in sorted(self._pairs.items())},
                    samples={i: tuple(v) for i, v in sorted(self._samples.items())}, background=tuple(self._bkgd))

    def fingerprint(self):
        """A fixed number of floats for the cross-rank check of a sharded render (``stnerf_amd.parallel``): res, threshold,
        dilate, auto | samples << 1 | background << 2 | (background_res code) << 3, the number of manual grids, and a digest of the
        manual grids, the background's among them.  Eight floats, as before the background's grid: its fields ride in the flags and
        the digest, and without it both are what they were.  background_res code: 0 for None, else 1 + (Rx-1) + 256 (Ry-1) +
        65536 (Rz-1) < 2^25, so the flags stay exact in fp64."""
        h = hashlib.sha256()
        for i in sorted(self._manual):
            words, res, lo, hi, _, _ = self._manual[i]
            h.update(repr((i, res)).encode() + lo.tobytes() + hi.tobytes() + words.tobytes())
        if self._bkgd_manual is not None:
            h.update(self._bkgd_digest().to_bytes(6, "little"))
        digest = int.from_bytes(h.digest()[:6], "little") if (self._manual or self._bkgd_manual is not None) else 0      # (48 bits: exact in fp64)
        br = self.background_res
        code = 0 if br is None else 1 + (br[0] - 1) + 256 * (br[1] - 1) + 65536 * (br[2] - 1)
        flags = int(self.auto) | int(self.samples) << 1 | int(self.background) << 2 | code << 3
        return [float(x) for x in self.res] + [self.threshold, float(self.dilate), float(flags), float(len(self._manual)), float(digest)]
