"""Progressive multi-sample frames: the pass schedule and the user's spec.

A frame is the per-pixel mean of several passes.  Pass p moves every ray by a sub-pixel offset, plays every layer at a
shutter time and draws with its own seed; the means, second moments and counts live on the device
(``ops.accumulate`` / ``ops.accumulate_select``, csrc/accumulate.hip) and a pixel stops being sampled once the standard
error of its mean is below ``tol``.  ``parallel.render_view_accumulated`` is the loop; this module is its host arithmetic,
which is exact and needs no GPU.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

MAX_SPP = 32768     # (the library's bound: count * (count - 1) is an int32 product)


def radical_inverse(p: int, base: int) -> float:
    """phi_base(p) in fp64: the digits of p in ``base``, mirrored about the point.  f starts at 1 / base; every digit adds
    digit * f, then f = f / base."""
    if p < 0 or base < 2:
        raise ValueError(f"radical_inverse: need p >= 0 and base >= 2, got {p}, {base}")
    r = 0.0
    f = 1.0 / base
    while p:
        p, digit = divmod(p, base)
        r = r + digit * f
        f = f / base
    return r


def pass_schedule(p: int) -> Tuple[float, float, float]:
    """(du, dv, dt) of pass p >= 0: ((phi_b(p) + 0.5) mod 1) - 0.5 in fp64 with b = 2, 3, 5, rounded to fp32 -- a Halton
    sequence re-centred so that pass 0 is (0, 0, 0), the plain render.  All three lie in [-0.5, 0.5); every prefix of the
    sequence is well spread, which matters because pixels stop at different counts.  du, dv: pixels (before
    ``pixel_filter``); dt: shutter intervals (before ``shutter``)."""
    out = []
    for base in (2, 3, 5):
        x = radical_inverse(int(p), base) + 0.5
        x = x - np.floor(x)
        out.append(float(np.float32(x - 0.5)))
    return tuple(out)


class AccumulateSpec:
    """How a frame is accumulated.

    max_spp       passes a pixel gets at most (>= 1).
    min_spp       passes every pixel gets (default max_spp: fixed spp); 1 <= min_spp <= max_spp.
    tol           a pixel with min_spp <= count < max_spp goes on while the standard error of the mean of any colour channel
                  exceeds tol (>= 0; tol = 0 with min_spp < max_spp never converges and runs to max_spp).
    pixel_filter  width of the box the sub-pixel offsets cover, in pixels (default 1.0: the pixel; 0: no anti-aliasing).
    shutter       exposure per layer in frames: a list of l entries, or one number for the performers (the background stays
                  still); default None = 0: no motion blur.
    frame_range   (lo, hi): every layer's frame id of a pass is clamped to it; default None.
    """

    def __init__(self, max_spp: int, min_spp: Optional[int] = None, tol: float = 0.0, pixel_filter: float = 1.0, shutter=None,
                 frame_range: Optional[Sequence[float]] = None):
        if int(max_spp) != max_spp or (min_spp is not None and int(min_spp) != min_spp):
            raise ValueError(f"AccumulateSpec: max_spp and min_spp are whole numbers, got {max_spp!r}, {min_spp!r}")
        self.max_spp = int(max_spp)
        self.min_spp = self.max_spp if min_spp is None else int(min_spp)
        if not (1 <= self.min_spp <= self.max_spp <= MAX_SPP):
            raise ValueError(f"AccumulateSpec: need 1 <= min_spp <= max_spp <= {MAX_SPP}, got min_spp={self.min_spp}, max_spp={self.max_spp}")
        self.tol = float(tol)
        if not self.tol >= 0.0 or self.tol * self.tol > float(np.finfo(np.float32).max):
            raise ValueError(f"AccumulateSpec: tol must be >= 0 (and its square finite in fp32), got {tol!r}")
        self.pixel_filter = float(pixel_filter)
        if not (self.pixel_filter >= 0.0 and np.isfinite(self.pixel_filter)):
            raise ValueError(f"AccumulateSpec: pixel_filter must be >= 0, got {pixel_filter!r}")
        if shutter is None or isinstance(shutter, (int, float)):
            self.shutter = None if shutter is None else float(shutter)
            values = [] if shutter is None else [self.shutter]
        else:
            self.shutter = [float(s) for s in shutter]
            values = self.shutter
        if not all(np.isfinite(s) for s in values):
            raise ValueError(f"AccumulateSpec: shutter must be finite, got {shutter!r}")
        self.frame_range = None
        if frame_range is not None:
            if len(frame_range) != 2 or not float(frame_range[0]) <= float(frame_range[1]):
                raise ValueError(f"AccumulateSpec: frame_range is (lo, hi) with lo <= hi, got {frame_range!r}")
            self.frame_range = (float(frame_range[0]), float(frame_range[1]))

    def __repr__(self):
        return (f"AccumulateSpec(max_spp={self.max_spp}, min_spp={self.min_spp}, tol={self.tol}, pixel_filter={self.pixel_filter}, "
                f"shutter={self.shutter}, frame_range={self.frame_range})")

    @property
    def adaptive(self) -> bool:
        return self.min_spp < self.max_spp

    def shutters(self, l: int) -> List[float]:
        """One exposure per layer of an l-layer view: a scalar reaches the performers only."""
        if self.shutter is None:
            return [0.0] * l
        if isinstance(self.shutter, float):
            return [0.0] + [self.shutter] * (l - 1)
        if len(self.shutter) != l:
            raise ValueError(f"AccumulateSpec: shutter must have one entry per layer ({l}, layer 0 = the background) or be one number "
                             f"for the performers, got {len(self.shutter)}")
        return list(self.shutter)

    def has_shutter(self, l: int) -> bool:
        return any(s != 0.0 for s in self.shutters(l))

    def offset(self, p: int) -> Tuple[float, float]:
        """The sub-pixel offset of pass p: pixel_filter * (du, dv), each product rounded to fp32 once."""
        du, dv, _ = pass_schedule(p)
        return float(np.float32(self.pixel_filter * du)), float(np.float32(self.pixel_filter * dv))

    def frame_ids(self, p: int, frame_ids: Sequence[float]) -> List[float]:
        """Layer i's frame id of pass p: f_i + shutter[i] * dt_p in fp64, clamped to ``frame_range`` when given, rounded to fp32
        (what the ray tensor holds)."""
        _, _, dt = pass_schedule(p)
        out = []
        for f, s in zip(frame_ids, self.shutters(len(frame_ids))):
            f = float(f) + s * dt
            if self.frame_range is not None:
                f = min(max(f, self.frame_range[0]), self.frame_range[1])
            out.append(float(np.float32(f)))
        return out


def as_spec(spec) -> AccumulateSpec:
    """An ``AccumulateSpec`` from one or from the dict of its arguments."""
    if isinstance(spec, AccumulateSpec):
        return spec
    if isinstance(spec, dict):
        return AccumulateSpec(**spec)
    raise TypeError(f"accumulate is an AccumulateSpec or the dict of its arguments, got {type(spec).__name__}")
