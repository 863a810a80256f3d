"""Adaptive lattice frames: the user's spec and the host arithmetic of the lattice.

A frame is rendered on a sparse lattice of pixels (stride S = 2^levels), the cells whose four corners disagree are refined at
half the stride, and the pixels of the cells whose corners agree are interpolated from them.  The per-pixel state lives on the
device (``ops.lattice_begin`` / ``lattice_classify`` / ``lattice_select`` / ``lattice_scatter``, csrc/lattice.hip; the rule is
stated in include/stnerf.h); ``parallel.render_view_lattice`` is the loop.  This module is its host side, which needs no GPU.
An approximation, opt-in, inference only.
"""
from __future__ import annotations

import math
from typing import List, Tuple

MAX_LEVELS = 4      # (the library's bound: a top stride of 16 pixels)
EXACT_COLUMNS = 1   # the last column of pack_outputs(raw, "fine"), the hit-mask bits, is compared with ==


class LatticeSpec:
    """How a frame is rendered on a lattice.

    levels     K in 0..4: the top stride is 2^K pixels (0: every pixel is rendered, the plain frame).
    tol_rgb    a cell is flat only if every colour channel of its four corners -- of the mixed image and of every layer --
               spreads by at most tol_rgb (>= 0).  Required: no default has been measured.
    tol_depth  the same bound on the depth channels (default +inf: depth is only required to be finite).
    tol_alpha  the same bound on the alpha channels (default +inf).
    force      the pixels that are rendered whatever their cells say: "performers" (default: every pixel where a shown
               performer layer is hit, so that the approximation is confined to pixels only the background reaches), None, or an
               (h, w) uint8 tensor (nonzero = rendered).
    """

    def __init__(self, levels: int, tol_rgb: float, tol_depth: float = math.inf, tol_alpha: float = math.inf, force="performers"):
        if isinstance(levels, bool) or int(levels) != levels:
            raise ValueError(f"LatticeSpec: levels is a whole number, got {levels!r}")
        self.levels = int(levels)
        if not 0 <= self.levels <= MAX_LEVELS:
            raise ValueError(f"LatticeSpec: need 0 <= levels <= {MAX_LEVELS}, got {self.levels}")
        self.tol_rgb, self.tol_depth, self.tol_alpha = float(tol_rgb), float(tol_depth), float(tol_alpha)
        for name, t in (("tol_rgb", self.tol_rgb), ("tol_depth", self.tol_depth), ("tol_alpha", self.tol_alpha)):
            if not t >= 0.0:
                raise ValueError(f"LatticeSpec: {name} must be >= 0, got {t!r}")
        if isinstance(force, str):
            if force != "performers":
                raise ValueError(f"LatticeSpec: force is \"performers\", None or an (h, w) uint8 tensor, got {force!r}")
        elif force is not None:
            import torch
            if not torch.is_tensor(force) or force.dim() != 2 or force.dtype != torch.uint8:
                raise ValueError("LatticeSpec: force is \"performers\", None or an (h, w) uint8 tensor, got "
                                 f"{(tuple(force.shape), force.dtype) if torch.is_tensor(force) else type(force).__name__}")
        self.force = force

    def __repr__(self):
        force = self.force if self.force is None or isinstance(self.force, str) else f"<{tuple(self.force.shape)} uint8>"
        return (f"LatticeSpec(levels={self.levels}, tol_rgb={self.tol_rgb}, tol_depth={self.tol_depth}, tol_alpha={self.tol_alpha}, "
                f"force={force!r})")

    @property
    def stride(self) -> int:
        return 1 << self.levels

    def strides(self) -> List[int]:
        """The strides the loop classifies at: S, S / 2, .., 2."""
        return [1 << k for k in range(self.levels, 0, -1)]

    def tolerances(self, l: int) -> List[float]:
        """The C - E = 5 + 5 l bounds of the tested columns of ``pack_outputs(raw, "fine")``: [tol_rgb x 3, tol_depth, tol_alpha],
        tiled over the mixed five floats and each layer's five."""
        return [self.tol_rgb] * 3 + [self.tol_depth, self.tol_alpha] + ([self.tol_rgb] * 3 + [self.tol_depth, self.tol_alpha]) * l


def covered(h: int, w: int, levels: int) -> Tuple[int, int]:
    """(Wc, Hc) of include/stnerf.h: the pixels with x <= Wc and y <= Hc are covered by cells -- none if either is 0."""
    S = 1 << levels
    return (w - 1) // S * S, (h - 1) // S * S


def as_spec(spec) -> LatticeSpec:
    """A ``LatticeSpec`` from one or from the dict of its arguments."""
    if isinstance(spec, LatticeSpec):
        return spec
    if isinstance(spec, dict):
        return LatticeSpec(**spec)
    raise TypeError(f"lattice is a LatticeSpec or the dict of its arguments, got {type(spec).__name__}")
