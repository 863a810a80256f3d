"""Early ray termination: skip the fine samples the coarse pass shows are hidden.

The coarse composite knows the merged transmittance along every ray.  Where it has fallen to ``tau`` the ray is opaque, and a
fine sample behind that depth -- inside or behind an opaque performer, or of the background behind one -- cannot be seen; it gets
exact zero outputs instead of a network evaluation (include/stnerf.h and DESIGN.md section 7 state the rule; csrc/termination.hip).
The fine stage only, inference only, off by default.  Attach with ``model.set_termination()`` or
``LayeredNeuralRenderer(..., terminate=True)``.
"""
from __future__ import annotations

import numpy as np
import torch


class Termination:
    """``tau``: the transmittance at which a ray counts as opaque, fp32 in [0, 1) (instant-ngp and nerfacc use 1e-4).
    ``layers``: the performer (and instance) layers to terminate, or None = every shown one.  ``background``: terminate layer 0
    too (it is left alone while a background cache captures or serves it: its outputs would depend on the performers)."""

    def __init__(self, tau: float = 1e-4, layers=None, background: bool = True):
        tau32 = float(np.float32(tau))
        if not 0.0 <= tau32 < 1.0:          # (a NaN fails both)
            raise ValueError(f"termination: tau must lie in [0, 1) as fp32, got {tau!r}")
        self.tau = tau32
        if layers is not None:
            layers = tuple(sorted({int(i) for i in layers}))
            if any(i < 1 for i in layers):
                raise ValueError(f"termination: layers are performers and instances (>= 1; the background has its own flag), got {layers}")
        self.layers = layers
        if not isinstance(background, bool):
            raise TypeError(f"background is False or True, got {background!r}")
        self.background = background
        self._counts = None     # int64 (MAX_LAYERS, 2) on the device: (fine samples tested, not listed), by the rows kernel
        self._rows = {}         # layer id -> [tested, skipped]: what stats() has taken off them so far

    def flags(self, model):
        """One flag per layer of ``model``: the layers a render terminates."""
        l = model.total_layers
        if self.layers is not None and any(i >= l for i in self.layers):
            raise ValueError(f"termination: layers {self.layers} of a model with layers 0..{l - 1}")
        return [self.background] + [model.is_shown_layer(i) and (self.layers is None or i in self.layers) for i in range(1, l)]

    def counts(self, device) -> torch.Tensor:
        """The device counters the rows kernel accumulates into: int64 (MAX_LAYERS, 2)."""
        from stnerf_amd import hip
        if self._counts is None or self._counts.device != torch.device(device):
            self._counts = torch.zeros(hip.MAX_LAYERS, 2, dtype=torch.int64, device=device)
        return self._counts

    def reset_stats(self) -> None:
        self._rows = {}
        if self._counts is not None:
            self._counts.zero_()

    def stats(self) -> dict:
        """``rows``: per terminated layer (fine samples tested, samples not listed -- hidden, or with a sample-culling grid in an
        empty cell) since the last ``reset_stats()``: one device-to-host copy, made only here."""
        if self._counts is not None:
            for i, (t, c) in enumerate(self._counts.cpu().tolist()):
                if t:
                    held = self._rows.setdefault(i, [0, 0])
                    held[0] += int(t)
                    held[1] += int(c)
            self._counts.zero_()
        return dict(rows={i: tuple(v) for i, v in sorted(self._rows.items())})

    def fingerprint(self):
        """A fixed number of floats for the cross-rank check of a sharded render (``stnerf_amd.parallel``): tau, the background
        flag, and the layer set as a bit mask (-1: every shown layer)."""
        mask = -1.0 if self.layers is None else float(sum(1 << i for i in self.layers))
        return [self.tau, float(self.background), mask]
