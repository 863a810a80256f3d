"""The background cache: layer 0's raw network outputs of a fixed view, kept on the device across frames.

A time sweep from one camera (``LayeredNeuralRenderer.set_path_fixed_gt_poses`` + retiming / the edit schedule) renders many
frames in which nothing that feeds the background networks changes: the rays, the background box, the draws (the device RNG is
keyed by seed, global ray index, layer and sample) and -- the resampler working per layer -- the background's fine depths.  The
first such frame CAPTURES the background's slices of the two network stages, ``raw_c (n, n1, 4)`` and ``raw_f (n, n1 + n2, 4)``
(dense fp32, what the stage kernels stored: 16 (2 n1 + n2) bytes per ray); later frames leave the background out of both stages
and copy the slices in (stnerf_render_rays_cached, csrc/pipeline.hip).  Sampler, compaction, compositor and resampler still run
for every layer, so a frame rendered from the cache is bit-identical to the frame rendered without it.

``LayeredRFRender.background_cache_key`` says when "nothing changed" holds (a host function over everything the background's
outputs depend on); this module owns the tensors.  Attach with ``model.set_background_cache(BackgroundCache())`` or
``LayeredNeuralRenderer(..., cache_background=True)``.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Optional, Tuple

import torch

DEFAULT_MAX_BYTES = 8 << 30


def piece_bytes(n: int, n1: int, n2: int, only_coarse: bool) -> int:
    """Bytes the cache holds for a launch piece of n rays: 16 (2 n1 + n2) per ray (16 n1 with only_coarse)."""
    return 16 * n * (n1 if only_coarse else 2 * n1 + n2)


class BackgroundCache:
    """Device tensors of the cached launch pieces, keyed by ``(group, piece)`` (``LayeredRFRender.background_cache_key``): the
    group is everything but the piece's place in the view, so the pieces of one view under one set of inputs share it.

    ``max_bytes``: the budget (default 8 GiB, or ``STNERF_BKGD_CACHE_GB``).  A piece that does not fit is first given the room
    of OTHER groups' entries (a camera, seed or weight version left behind), oldest first; if it still does not fit it is
    rendered without the cache and counted in ``stats["skipped_over_budget"]`` -- never an error.
    ``stats``: hits, misses (lookups that found nothing), captures, skipped_over_budget.

    Entries are filled and read by kernels enqueued on the stream current at the call: use one stream per cache."""

    def __init__(self, max_bytes: Optional[int] = None):
        if max_bytes is None:
            gb = os.environ.get("STNERF_BKGD_CACHE_GB")
            max_bytes = int(float(gb) * (1 << 30)) if gb else DEFAULT_MAX_BYTES
        self.max_bytes = int(max_bytes)
        self._entries: "OrderedDict[tuple, Tuple[torch.Tensor, Optional[torch.Tensor]]]" = OrderedDict()
        self.bytes_used = 0
        self.stats = dict(hits=0, misses=0, captures=0, skipped_over_budget=0)

    def __len__(self):
        return len(self._entries)

    @staticmethod
    def _nbytes(entry) -> int:
        return sum(t.numel() * 4 for t in entry if t is not None)

    def lookup(self, key):
        """The (raw_c, raw_f | None) tensors captured under ``key``, or None."""
        entry = self._entries.get(key)
        if entry is None:
            self.stats["misses"] += 1
            return None
        self._entries.move_to_end(key)
        self.stats["hits"] += 1
        return entry

    def reserve(self, key, n: int, n1: int, n2: int, only_coarse: bool, device):
        """Fresh tensors for the piece ``key`` (to be filled by a capture render), or None when the budget has no room."""
        need = piece_bytes(n, n1, n2, only_coarse)
        self.discard(key)
        if self.bytes_used + need > self.max_bytes:
            for other in [k for k in self._entries if k[0] != key[0]]:
                self.discard(other)
                if self.bytes_used + need <= self.max_bytes:
                    break
        if self.bytes_used + need > self.max_bytes:
            self.stats["skipped_over_budget"] += 1
            return None
        raw_c = torch.empty(n, n1, 4, dtype=torch.float32, device=device)
        raw_f = None if only_coarse else torch.empty(n, n1 + n2, 4, dtype=torch.float32, device=device)
        self._entries[key] = (raw_c, raw_f)
        self.bytes_used += need
        self.stats["captures"] += 1
        return raw_c, raw_f

    def discard(self, key) -> None:
        entry = self._entries.pop(key, None)
        if entry is not None:
            self.bytes_used -= self._nbytes(entry)

    def clear(self) -> None:
        """Drop every entry (the statistics stay)."""
        self._entries.clear()
        self.bytes_used = 0


def view_key(K, T, h: int, w: int, frame_ids=None):
    """What identifies the rays of a view generated from its camera (ops.generate_rays): the fp32 bytes of K and T, h and w --
    plus the background's frame id (``frame_ids[0]``), which the model adds to a piece's key only where the background networks
    take it.  -> the value of ``LayeredRFRender.view_key``."""
    kb = torch.as_tensor(K, dtype=torch.float32).detach().cpu().contiguous().numpy().tobytes()
    tb = torch.as_tensor(T, dtype=torch.float32).detach().cpu().contiguous().numpy().tobytes()
    bkgd_frame = float(frame_ids[0]) if frame_ids is not None and len(frame_ids) else None
    return ("view", kb, tb, int(h), int(w)), bkgd_frame


def tag_view_rays(rays, K, T, h: int, w: int, frame_ids=None):
    """Mark `rays` as the untouched rays of the whole view (K, T, h, w) -- for callers that generate them from a camera and hand
    the TENSOR on (the drop-in's device ray generation: the reference's render_pose passes it to layered_batchify_ray)."""
    rays.stnerf_view_key = (view_key(K, T, h, w, frame_ids), rays._version, tuple(rays.shape))
    rays.stnerf_view_frame_ids = view_frame_ids(frame_ids)
    return rays


def view_frame_ids(frame_ids):
    """The host values a view's frame-id columns were generated with, as a tuple of floats (None without any) -> the value of
    ``LayeredRFRender.view_frame_ids``: what the layer cache reads a layer's frame id from (no device read per frame)."""
    if frame_ids is None or len(frame_ids) == 0:
        return None
    return tuple(float(f) for f in frame_ids)


def tagged_view_frame_ids(rays):
    """The frame ids `tag_view_rays` put on this very tensor (None where ``tagged_view_key`` gives None)."""
    return getattr(rays, "stnerf_view_frame_ids", None) if tagged_view_key(rays) is not None else None


def tagged_view_key(rays):
    """The view key `tag_view_rays` put on this very tensor, or None: a copy, a slice or a tensor written to since carries none."""
    tag = getattr(rays, "stnerf_view_key", None)
    if tag is None or tag[1] != rays._version or tag[2] != tuple(rays.shape):
        return None
    return tag[0]
