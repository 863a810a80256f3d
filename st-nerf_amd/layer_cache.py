"""The layer cache: the performers' raw network outputs of a fixed view, kept on the device across frames.

What ``BackgroundCache`` does for layer 0 holds for every performer: ``stnerf_resample`` works per layer, the device RNG is keyed by
(seed, global ray index, layer, stream, sample), and a layer's sample points depend on the rays and on that layer's own box, edit,
rotation and frame id.  So layer i's slices of ``raw_c`` / ``raw_f`` are a function of the view and of layer i's own inputs: nudging
performer 2 leaves performer 1's untouched, and fading a layer (``layer_alpha``), sweeping ``bkgd_density_threshold`` or hiding
another layer needs no network at all.  (``density_threshold`` is different under retiming: the coarse composite applies it to the
performers before the resampler reads their weights, so a performer's fine samples follow it and the key holds it.)
``LayeredRFRender.layer_cache_key`` says when "nothing changed" holds for a layer; this module owns the tensors and the policy.

A performer covers a fraction of the view, so an entry is COMPACT: slot j holds the raw outputs of hit ray ``rays[j]`` --
16 (2 n1 + n2) + 4 bytes per hit ray (stnerf_copy_layer_raw_listed, csrc/layer_cache.hip).  Its capacity must be known before the
capture, and a performer that moves every frame must not churn the cache, hence three sightings of a key:

  1. rendered uncached; the layer's hit count stays behind as a device scalar (the sum of the returned ray mask: no sync);
  2. ``capacity = int(count)`` (one sync), the entry is reserved and the frame CAPTURES into it;
  3. and later: REUSE.  The captured count is read once (4 bytes) before an entry's first reuse; -1 (the list did not fit) drops it.

Attach with ``model.set_layer_cache(LayerCache())`` or ``LayeredNeuralRenderer(..., cache_layers=True)``.  Rank-local: frames are
bit-identical with and without it, so nothing crosses ranks.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Optional

import torch

DEFAULT_MAX_BYTES = 8 << 30
MAX_SIGHTINGS = 4096          # first sightings remembered (one device scalar each), oldest first out

OFF, CAPTURE, REUSE = 0, 1, 2   # hip.LAYER_CACHE_*


def entry_bytes(capacity: int, n1: int, n2: int, only_coarse: bool) -> int:
    """Bytes the cache holds for a layer's entry of ``capacity`` hit rays: 16 (2 n1 + n2) + 4 per ray (16 n1 + 4 with only_coarse)."""
    return capacity * (16 * (n1 if only_coarse else 2 * n1 + n2) + 4)


def dense_bytes(n: int, n1: int, n2: int, only_coarse: bool) -> int:
    """What a dense slice of the piece's n rays would take (the background cache's layout): the figure an entry is compared with."""
    return 16 * n * (n1 if only_coarse else 2 * n1 + n2)


class Entry:
    """One (layer, piece) under one set of inputs: raw_c (capacity,n1,4), raw_f (capacity,n1+n2,4) | None, rays (capacity,) int32,
    count (1,) int32 -- all on the device -- and whether the count has been read since the capture."""
    __slots__ = ("raw_c", "raw_f", "rays", "count", "capacity", "nbytes", "checked", "hits")

    def __init__(self, raw_c, raw_f, rays, count, capacity, nbytes):
        self.raw_c, self.raw_f, self.rays, self.count = raw_c, raw_f, rays, count
        self.capacity, self.nbytes, self.checked, self.hits = capacity, nbytes, False, None

    def arg(self, mode):
        """The tuple ``ops.render_rays(layer_caches=...)`` takes for this layer."""
        return (self.raw_c, self.raw_f, self.rays, self.count, mode)


def _allocate(capacity, n1, n2, only_coarse, device):
    raw_c = torch.empty(capacity, n1, 4, dtype=torch.float32, device=device)
    raw_f = None if only_coarse else torch.empty(capacity, n1 + n2, 4, dtype=torch.float32, device=device)
    rays = torch.empty(capacity, dtype=torch.int32, device=device)
    count = torch.zeros(1, dtype=torch.int32, device=device)
    return raw_c, raw_f, rays, count


class LayerCache:
    """Entries keyed by ``(group, piece)`` (``LayeredRFRender.layer_cache_key``): the group is the layer and everything its raw
    outputs depend on but the piece's place in the view.

    ``max_bytes``: the budget (default 8 GiB, or ``STNERF_LAYER_CACHE_GB``), with ``BackgroundCache``'s rule: an entry that does not
    fit is given the room of OTHER groups' entries, oldest first -- when that makes room: if it would not fit even then, nothing is
    evicted, the layer is rendered without the cache and counted in ``stats()["skipped_over_budget"]`` -- never an error.
    ``stats()``: hits, misses (lookups that found no entry), sightings (first sightings of a key), captures, skipped_over_budget;
    ``stats(mismatch=True)`` adds the restore copies' guard counter (one device read): restores whose frame had another hit count
    than the entry -- 0 unless a key misses an input.

    ``allocate``: the function that makes an entry's four tensors (tests put a stub in its place).
    Entries are filled and read by kernels enqueued on the stream current at the call: use one stream per cache."""

    def __init__(self, max_bytes: Optional[int] = None, allocate=_allocate):
        if max_bytes is None:
            gb = os.environ.get("STNERF_LAYER_CACHE_GB")
            max_bytes = int(float(gb) * (1 << 30)) if gb else DEFAULT_MAX_BYTES
        self.max_bytes = int(max_bytes)
        self._allocate = allocate
        self._entries: "OrderedDict[tuple, Entry]" = OrderedDict()
        self._seen: "OrderedDict[tuple, object]" = OrderedDict()   # key -> the hit count of its first sighting (device scalar, later an int)
        self._mismatch = None
        self.bytes_used = 0
        self._stats = dict(hits=0, misses=0, sightings=0, captures=0, skipped_over_budget=0)

    def __len__(self):
        return len(self._entries)

    def stats(self, mismatch: bool = False) -> dict:
        out = dict(self._stats)
        if mismatch:
            out["mismatch"] = 0 if self._mismatch is None else int(self._mismatch.item())
        return out

    def mismatch_counter(self, device) -> torch.Tensor:
        """The device counter the restore copies add to: int64 (1,)."""
        if self._mismatch is None or self._mismatch.device != torch.device(device):
            self._mismatch = torch.zeros(1, dtype=torch.int64, device=device)
        return self._mismatch

    # ---- the policy ---------------------------------------------------------------------------------------------------------
    def plan(self, key, n1: int, n2: int, only_coarse: bool, device):
        """What this frame does with the layer ``key`` names -> (mode, entry | None).
        REUSE with the entry; CAPTURE with a freshly reserved one (second sighting, room in the budget); OFF otherwise -- and then the
        caller reports the layer's hit count of the frame with ``sighted`` when ``wants_count(key)``."""
        entry = self._entries.get(key)
        if entry is not None and not entry.checked:
            # the one read of a captured count: 4 bytes, before the entry's first reuse
            got = int(entry.count.reshape(-1)[0])
            if got < 0 or got > entry.capacity:
                self.discard(key)             # (the frame's list did not fit the capacity of the sighting: start over)
                entry = None
            else:
                entry.checked, entry.hits = True, got
        if entry is not None:
            self._entries.move_to_end(key)
            self._stats["hits"] += 1
            return REUSE, entry
        self._stats["misses"] += 1
        seen = self._seen.get(key)
        if seen is None:
            return OFF, None
        if not isinstance(seen, int):
            seen = self._seen[key] = int(seen)                     # the one sync of a key's second sighting
        entry = self._reserve(key, max(seen, 1), n1, n2, only_coarse, device)
        if entry is None:
            return OFF, None
        del self._seen[key]
        return CAPTURE, entry

    def wants_count(self, key) -> bool:
        """The key has neither an entry nor a remembered sighting: its frame's hit count is wanted (``sighted``)."""
        return key not in self._entries and key not in self._seen

    def sighted(self, key, count) -> None:
        """First sighting of ``key``: remember the layer's hit count (a device scalar, not read here)."""
        self._seen[key] = count
        self._stats["sightings"] += 1
        while len(self._seen) > MAX_SIGHTINGS:
            self._seen.popitem(last=False)

    def _reserve(self, key, capacity, n1, n2, only_coarse, device):
        need = entry_bytes(capacity, n1, n2, only_coarse)
        self.discard(key)
        others = [k for k in self._entries if k[0] != key[0]]
        if self.bytes_used - sum(self._entries[k].nbytes for k in others) + need > self.max_bytes:
            self._stats["skipped_over_budget"] += 1            # (no room even without the other groups: none of them is touched)
            return None
        for other in others:
            if self.bytes_used + need <= self.max_bytes:
                break
            self.discard(other)
        entry = Entry(*self._allocate(capacity, n1, n2, only_coarse, device), capacity, need)
        self._entries[key] = entry
        self.bytes_used += need
        self._stats["captures"] += 1
        return entry

    def discard(self, key) -> None:
        entry = self._entries.pop(key, None)
        if entry is not None:
            self.bytes_used -= entry.nbytes

    def clear(self) -> None:
        """Drop every entry and every remembered sighting (the statistics stay)."""
        self._entries.clear()
        self._seen.clear()
        self.bytes_used = 0

    def held(self):
        """Per entry (key, capacity, bytes, hit rays | None before the count was read) -- for reports."""
        return [(k, e.capacity, e.nbytes, e.hits) for k, e in self._entries.items()]
