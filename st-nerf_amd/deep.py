"""Deep frames (include/stnerf.h): the final stage's merged weights kept as a per-pixel list of deep samples,
so that any number of depth-tested elements -- props, title cards, z-buffered plates -- are composited AFTER the render, with no
network.  ``DeepSpec`` says which samples are kept and how they are merged; ``DeepFrame`` is the list in CSR form with the
compositing calls on it (``ops.deep_composite``: HIP, no PyTorch fallback)."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

# The wrapper sizes every launch piece's record buffer at the worst case (n l S records of 32 bytes) and shrinks the piece so that the
# buffer stays under this many bytes: it never re-renders and never drops a record.
PIECE_BUFFER_BYTES = 1 << 30
RECORD_BYTES = 32
WORDS = ("r", "g", "b", "a", "zw", "zf", "zb", "meta")


@dataclass(frozen=True)
class DeepSpec:
    """w_min >= 0: sample k of a layer is kept iff not (merged weight <= w_min).  merge_dz >= 0: 0 keeps every kept sample as its own
    record; > 0 merges a layer's consecutive kept samples that fall into the same depth bin of that width (in ray-parameter units)."""
    w_min: float = 0.0
    merge_dz: float = 0.0

    def __post_init__(self):
        for name in ("w_min", "merge_dz"):
            v = float(getattr(self, name))
            if not v >= 0.0 or v == float("inf"):
                raise ValueError(f"DeepSpec: {name} = {v} must be finite and >= 0")

    def options(self, capacity=None):
        """The ``deep=`` dict of ``ops.render_rays``."""
        return dict(w_min=float(self.w_min), merge_dz=float(self.merge_dz), capacity=capacity)


def as_spec(deep) -> Optional[DeepSpec]:
    if deep is None or isinstance(deep, DeepSpec):
        return deep
    if deep is True:
        return DeepSpec()
    raise TypeError(f"deep must be a DeepSpec, True or None, got {type(deep).__name__}")


def piece_rays(l: int, S: int, budget: int = PIECE_BUFFER_BYTES) -> int:
    """The most rays of a launch piece whose worst-case record buffer stays under ``budget`` bytes."""
    return max(1, budget // (RECORD_BYTES * l * S))


class DeepFrame:
    """offsets (H W + 1,) int64, samples (total, 8) fp32 words {r, g, b, a, zw, zf, zb, meta}, row-major pixels; ``layers`` the
    layer count, ``far`` the depth the depth outputs are divided by for display (None: unknown).  ``meta`` is a uint32 word:
    layer | first_k << 8 | count << 16."""

    def __init__(self, offsets, samples, H, W, layers, far=None):
        if offsets.dim() != 1 or offsets.shape[0] != H * W + 1 or samples.dim() != 2 or samples.shape[1] != 8:
            raise ValueError(f"DeepFrame: offsets must be ({H * W + 1},) and samples (total,8), got {tuple(offsets.shape)} and {tuple(samples.shape)}")
        self.offsets, self.samples, self.H, self.W, self.layers, self.far = offsets, samples, int(H), int(W), int(layers), far

    @classmethod
    def from_pieces(cls, pieces, H, W, layers, far=None, device="cpu"):
        """pieces: (offsets (n_i + 1,), samples (total_i, 8)) in pixel order -> one frame, the offsets rebased.  No piece: the empty
        frame on ``device``, offsets [0] and samples (0, 8)."""
        if not pieces:
            return cls(torch.zeros(1, dtype=torch.int64, device=device), torch.zeros(0, 8, dtype=torch.float32, device=device), H, W, layers, far)
        offs, base = [], 0
        for o, s in pieces:
            offs.append(o[:-1] + base)
            base += int(s.shape[0])
        dev = pieces[0][0].device
        offs.append(torch.tensor([base], dtype=torch.int64, device=dev))
        return cls(torch.cat(offs), torch.cat([s for _, s in pieces], 0), H, W, layers, far)

    @property
    def n_pixels(self):
        return self.H * self.W

    def meta(self):
        """-> (layer, first_k, count), int32 tensors (total,)."""
        m = self.samples[:, 7].contiguous().view(torch.int32)
        return m & 0xFF, (m >> 8) & 0xFF, (m >> 16) & 0xFFFF

    def composite(self, elements=None, want_scene=True, want_shares=True):
        """elements (H W, E, 5) or (H, W, E, 5) rows {r, g, b, a, z}, z a ray parameter, 0 <= E <= 8; None = the flatten.
        -> (mixed (H W, 5), scene (H W, l, 5) | None, shares (H W, E, 5) | None) (``ops.deep_composite``)."""
        from stnerf_amd import ops
        if elements is not None:
            if elements.dim() == 4:
                elements = elements.reshape(self.n_pixels, elements.shape[2], 5)
            elements = elements.to(self.samples.device, torch.float32).contiguous()
        return ops.deep_composite(self.offsets, self.samples, self.layers, elements, want_scene=want_scene, want_shares=want_shares)

    def flatten(self):
        """-> (mixed (H W, 5), scene (H W, l, 5)): the frame with no element in it."""
        mixed, scene, _ = self.composite(None)
        return mixed, scene

    def stats(self):
        """Samples per pixel (mean, max, histogram by count) and the bytes of the list."""
        per = (self.offsets[1:] - self.offsets[:-1]).cpu().numpy()
        hist = np.bincount(per) if per.size else np.zeros(1, np.int64)
        return dict(pixels=int(per.size), samples=int(per.sum()), mean=float(per.mean()) if per.size else 0.0,
                    max=int(per.max()) if per.size else 0, histogram=hist.tolist(),
                    bytes=int(self.samples.shape[0]) * RECORD_BYTES + int(self.offsets.numel()) * 8)

    def save(self, path):
        """An .npz with offsets, samples (as uint32 words: every bit kept, NaNs included), H, W, layers and far."""
        np.savez(path, offsets=self.offsets.cpu().numpy(), samples=self.samples.cpu().contiguous().view(torch.int32).numpy().view(np.uint32),
                 H=self.H, W=self.W, layers=self.layers, far=np.float64(np.nan if self.far is None else self.far))

    @classmethod
    def load(cls, path, device="cpu"):
        with np.load(path) as z:
            far = float(z["far"])
            samples = torch.from_numpy(z["samples"].view(np.int32).copy()).view(torch.float32)
            return cls(torch.from_numpy(z["offsets"].copy()).to(device), samples.to(device), int(z["H"]), int(z["W"]), int(z["layers"]),
                       None if far != far else far)
