"""Grid proposals: a layer's coarse densities from a density grid, no coarse network.

The only thing the final frame takes from the coarse pass is the weights the resampler turns into ``n2`` new depths; the fine
networks are evaluated at all ``n1 + n2`` sorted depths anyway.  A flagged layer's coarse pass is a trilinear lookup in a grid of
the layer's own densities (include/stnerf.h: stnerf_density_grid; DESIGN.md section 7 states the rule): its coarse SpaceNet and
MotionNet do not run, everything downstream is what it is, fed with those densities (csrc/proposal.hip).

``LayeredRFRender.density_grid(..., fine=True)`` evaluates the densities at the grid's vertices -- the object ``OccupancyGrids``
thresholds to bits; this module keeps them.  Attach with ``model.set_proposal(ProposalGrids())`` or
``LayeredNeuralRenderer(..., proposal=True)``.  Approximate, inference only, off by default.
"""
from __future__ import annotations

import hashlib
from collections import OrderedDict
from typing import NamedTuple, Tuple

import numpy as np
import torch

from stnerf_amd.occupancy import box_bounds, inv_cell, normalise_res


class DensityGrid(NamedTuple):
    sigma: torch.Tensor         # fp32 (Rz+1, Ry+1, Rx+1) vertex densities, on the device
    res: Tuple[int, int, int]   # (Rx, Ry, Rz)
    lo: np.ndarray              # fp32 (3,)
    hi: np.ndarray
    inv_cell: np.ndarray        # fp32 (3,): (float)R / (hi - lo)

    def entry(self):
        """The layer's entry of the table ``ops.proposal_density`` / ``ops.render_rays(proposal=)`` take."""
        return self.sigma, self.lo.tolist(), self.inv_cell.tolist()

    def nbytes(self) -> int:
        return int(self.sigma.numel()) * 4


class ProposalGrids:
    """The density grids of a model's flagged layers.

    ``res``: cells per axis (a number or (Rx, Ry, Rz), 1..256) of the grid a layer gets from the model's own FINE networks
    (``model.density_grid(layer, frame_id, res, fine=True)``: the fine stage is what the proposal has to predict).
    ``layers``: the performer / instance layers to flag (None: every shown one).  ``background=True`` flags layer 0 too, with a grid
    of ``background_res`` cells per axis (None: ``res``) over the unedited ``bkgd_bbox``.
    Built grids are keyed by the module index, the frame id, the bytes of lo / hi, res, the parameter versions of the layer's fine
    SpaceNet and MotionNet and the model flags; at most ``max_grids`` are kept, least recently used first out (a 128^3 grid holds
    8.6 MB).  ``set_manual`` gives a layer a grid of the caller's at every frame id.
    Not with: training, more than one rank, the op-by-op and per-net schedules, a layer or background cache on a flagged layer,
    the background flagged beside a background grid or a per-ray background mask (``LayeredRFRender.set_proposal``)."""

    def __init__(self, res=128, layers=None, background: bool = False, background_res=None, max_grids: int = 16):
        self.res = normalise_res(res)
        if layers is not None:
            layers = [l for l in layers]
            if any(isinstance(l, bool) or not isinstance(l, int) or l < 1 for l in layers):
                raise ValueError(f"proposal layers are performer / instance layers (integers >= 1; background=True flags layer 0), got {layers!r}")
            layers = sorted(set(layers))
        self.layers = layers
        if not isinstance(background, bool):
            raise TypeError(f"background is False or True, got {background!r}")
        self.background = background
        self.background_res = None if background_res is None else normalise_res(background_res)
        if isinstance(max_grids, bool) or int(max_grids) != max_grids or int(max_grids) < 1:
            raise ValueError(f"max_grids must be an integer of at least 1, got {max_grids!r}")
        self.max_grids = int(max_grids)
        self._built: "OrderedDict[tuple, DensityGrid]" = OrderedDict()
        self._manual = {}            # layer id -> (sigma fp32 (host), res, lo, hi, inv_cell, {device: DensityGrid})
        self.built = self.reused = 0

    # ---- manual grids ---------------------------------------------------------------------------------
    def set_manual(self, layer_id: int, sigma, lo=None, hi=None) -> None:
        """Use ``sigma`` (fp32 [Rz+1][Ry+1][Rx+1], the densities at the vertices) over the bounds lo, hi for layer ``layer_id`` at
        every frame id, as given; ``None`` clears it.  Layer 0 is the background.  A manual grid flags its layer whatever ``layers``
        / ``background`` say."""
        if isinstance(layer_id, bool) or int(layer_id) != layer_id or int(layer_id) < 0:
            raise ValueError(f"set_manual: layer {layer_id!r} is not a layer (0: the background, >= 1: performers and instances)")
        if sigma is None:
            self._manual.pop(int(layer_id), None)
            return
        s = torch.as_tensor(sigma)
        if not s.dtype.is_floating_point or s.dim() != 3 or min(s.shape) < 2:
            raise ValueError(f"a manual density grid is a float tensor [Rz+1][Ry+1][Rx+1] with at least one cell per axis, got {s.dtype} of "
                             f"shape {tuple(s.shape)}")
        res = normalise_res((s.shape[2] - 1, s.shape[1] - 1, s.shape[0] - 1))
        if lo is None or hi is None:
            raise ValueError("a manual density grid needs its bounds lo, hi")
        lo, hi = np.asarray(lo, np.float32).reshape(-1), np.asarray(hi, np.float32).reshape(-1)
        inv = inv_cell(res, lo, hi)
        host = s.detach().to("cpu", torch.float32).contiguous().clone()
        self._manual[int(layer_id)] = (host, res, lo.copy(), hi.copy(), inv, {})

    def manual_layers(self):
        return sorted(self._manual)

    def _manual_grid(self, layer_id, device) -> DensityGrid:
        host, res, lo, hi, inv, per_device = self._manual[layer_id]
        g = per_device.get(str(device))
        if g is None:
            g = per_device[str(device)] = DensityGrid(host.to(device), res, lo, hi, inv)
        return g

    # ---- the table of a launch ------------------------------------------------------------------------
    def has_background(self) -> bool:
        """Layer 0 is flagged: ``background=True`` or a manual grid on layer 0."""
        return self.background or 0 in self._manual

    @staticmethod
    def background_timed(model) -> bool:
        """The background's frame id is an input of its density: BKGD_USE_DEFORM_TIME, or BKGD_USE_SPACE_TIME under USE_SPACE_TIME."""
        return bool(model.bkgd_use_deform_time or (model.bkgd_use_space_time and model.use_space_time))

    def flagged_layers(self, model):
        """The layers a render of ``model`` flags, ascending: layer 0 with ``has_background()``, and the shown performers / instances
        among ``layers`` (None: all of them) or with a manual grid."""
        l = model.total_layers
        if self.layers is not None and any(i >= l for i in self.layers):
            raise ValueError(f"proposal layers {self.layers} name a layer the model does not have (1..{l - 1})")
        out = [0] if self.has_background() else []
        return out + [i for i in range(1, l) if model.is_shown_layer(i) and (i in self._manual or self.layers is None or i in self.layers)]

    def key(self, model, layer_id, frame_id, lo, hi):
        """The key of a built grid: module index (-1: the background), frame id (the background's only where its flags make it an
        input), lo / hi bytes, res, the parameter versions of the fine SpaceNet and the MotionNet, the model flags."""
        from stnerf_amd.modeling._packed import _params_fingerprint
        lo_b, hi_b = np.asarray(lo, np.float32).tobytes(), np.asarray(hi, np.float32).tobytes()
        if layer_id == 0:
            nets = [model.bkgd_spacenet_fine] + ([model.bkgd_time_deform_net] if model.bkgd_use_deform_time else [])
            return (-1, float(frame_id) if self.background_timed(model) else None, lo_b, hi_b, self.background_res or self.res,
                    tuple(_params_fingerprint(m) for m in nets),
                    (bool(model.bkgd_use_deform_time), bool(model.bkgd_use_space_time), bool(model.use_space_time), bool(model.deep_rgb)))
        j = model._module_index(layer_id)
        nets = [model.spacenets_fine[j]] + ([model.time_deform_nets[j]] if model.use_deform_time else [])
        return (j, float(frame_id), lo_b, hi_b, self.res, tuple(_params_fingerprint(m) for m in nets),
                (bool(model.use_deform_time), bool(model.use_space_time), bool(model.deep_rgb)))

    def grid(self, model, layer_id, frame_id, device, retiming=True) -> DensityGrid:
        """Layer ``layer_id``'s grid at ``frame_id``: its manual grid, a built one from the store, or a fresh build."""
        if layer_id in self._manual:
            return self._manual_grid(layer_id, device)
        res = (self.background_res or self.res) if layer_id == 0 else self.res
        lo, hi = box_bounds(model.bkgd_bbox if layer_id == 0 else model.layer_box_at(layer_id, frame_id, retiming))
        key = self.key(model, layer_id, frame_id, lo, hi) + (str(device),)
        g = self._built.get(key)
        if g is not None:
            self._built.move_to_end(key)
            self.reused += 1
            return g
        sigma, _, _ = model.density_grid(layer_id, frame_id, res, fine=True, retiming=retiming)
        g = self._built[key] = DensityGrid(sigma, res, lo, hi, inv_cell(res, lo, hi))
        self.built += 1
        while len(self._built) > self.max_grids:
            self._built.popitem(last=False)
        return g

    def table(self, model, frame_ids, device, retiming=True):
        """-> (per layer None | table entry, the DensityGrids in use): one grid per flagged layer, at that layer's frame id."""
        grids = [None] * model.total_layers
        for i in self.flagged_layers(model):
            grids[i] = self.grid(model, i, frame_ids[i], device, retiming)
        return [None if g is None else g.entry() for g in grids], grids

    # ---- bookkeeping ----------------------------------------------------------------------------------
    def __len__(self):
        return len(self._built)

    def clear(self) -> None:
        """Drop every built grid (manual grids and the statistics stay)."""
        self._built.clear()

    def reset_stats(self) -> None:
        self.built = self.reused = 0

    def stats(self) -> dict:
        """built / reused grid counts since the last ``reset_stats()``, the grids held and the device bytes they take (manual grids
        that have reached a device included)."""
        held = list(self._built.values()) + [g for m in self._manual.values() for g in m[5].values()]
        return dict(built=self.built, reused=self.reused, grids=len(held), bytes=sum(g.nbytes() for g in held))

    def identity(self):
        """A hashable summary of the settings and the manual grids (what a cache key or a cross-rank check would read)."""
        h = hashlib.sha256()
        for i in sorted(self._manual):
            host, res, lo, hi, _, _ = self._manual[i]
            h.update(repr((i, res)).encode() + lo.tobytes() + hi.tobytes() + host.numpy().tobytes())
        return ("proposal", self.res, None if self.layers is None else tuple(self.layers), self.background, self.background_res,
                h.hexdigest()[:16] if self._manual else None)
