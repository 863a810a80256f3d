"""Shared by tests/test_occupancy_cpu.py and tests/test_gpu_occupancy.py: numpy restatements of the occupancy grids' rules
(DESIGN.md section 7 / include/stnerf.h: stnerf_occupancy) -- the build from vertex densities, the bit layout and the
point -> cell -> keep rule, in fp32 with the stated operation order, written from those definitions and never from the HIP source --
the test grids, and the oracle's expectation of a culled render: ``scene_edits_common.oracle_render`` with ``O.sample_coarse``
wrapped (by the test, with pytest's monkeypatch) so that ``masks[i] &= keep_i`` at its return, and nothing else."""
import math

import numpy as np
import torch

from oracle import stnerf_oracle as O

import scene_edits_common as S

F32 = np.float32


# ---------------------------------------------------------------------------------------- the rules, in numpy
def np_bounds(box):
    """lo, hi (fp32) of a box's 8 corners."""
    b = np.asarray(torch.as_tensor(box, dtype=torch.float32).reshape(-1, 3).numpy(), F32)
    return b.min(0), b.max(0)


def np_inv_cell(res, lo, hi):
    """inv_a = (float)R_a / (hi_a - lo_a), fp32."""
    return np.array([F32(res[a]) / F32(F32(hi[a]) - F32(lo[a])) for a in range(3)], F32)


def np_vertices(res, lo, hi):
    """Per axis: vertex j at lo_a + j ((hi_a - lo_a) / R_a) in fp32, vertex R_a at hi_a itself."""
    out = []
    for a in range(3):
        step = F32(F32(hi[a]) - F32(lo[a])) / F32(res[a])
        v = np.array([F32(lo[a]) + F32(j) * step for j in range(res[a] + 1)], F32)
        v[res[a]] = F32(hi[a])
        out.append(v)
    return out


def np_dilate(occupied, dilate):
    """The occupied set [Rz][Ry][Rx] grown by ``dilate`` cells in Chebyshev distance (cut at the grid's border)."""
    occ = np.asarray(occupied, bool)
    if dilate == 0:
        return occ.copy()
    rz, ry, rx = occ.shape
    pad = np.zeros((rz + 2 * dilate, ry + 2 * dilate, rx + 2 * dilate), bool)
    pad[dilate:dilate + rz, dilate:dilate + ry, dilate:dilate + rx] = occ
    out = np.zeros_like(occ)
    for dz in range(2 * dilate + 1):
        for dy in range(2 * dilate + 1):
            for dx in range(2 * dilate + 1):
                out |= pad[dz:dz + rz, dy:dy + ry, dx:dx + rx]
    return out


def np_build(sigma_c, sigma_f, threshold, dilate):
    """Vertex densities [Rz+1][Ry+1][Rx+1] (either may be None) -> occupied bool [Rz][Ry][Rx]: a vertex is dense when
    !(sigma <= threshold) in either array (a NaN is dense), a cell occupied when one of its 8 corners is, then grown."""
    dense = None
    for s in (sigma_c, sigma_f):
        if s is None:
            continue
        with np.errstate(invalid="ignore"):
            d = ~(np.asarray(s, F32) <= F32(threshold))
        dense = d if dense is None else (dense | d)
    rz, ry, rx = (k - 1 for k in dense.shape)
    cell = np.zeros((rz, ry, rx), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cell |= dense[dz:dz + rz, dy:dy + ry, dx:dx + rx]
    return np_dilate(cell, dilate)


def np_pack(occupied):
    """Cell (x, y, z) is bit c & 31 of word c >> 5, c = (z Ry + y) Rx + x; ceil(cells / 32) uint32 words, the rest 0."""
    occ = np.asarray(occupied, bool)
    rz, ry, rx = occ.shape
    words = np.zeros((rz * ry * rx + 31) // 32, np.uint32)
    for z, y, x in zip(*np.nonzero(occ)):
        c = (int(z) * ry + int(y)) * rx + int(x)
        words[c >> 5] |= np.uint32(1 << (c & 31))
    return words


def np_unpack(words, res):
    """The inverse of ``np_pack`` for res = (Rx, Ry, Rz) (the unused bits are not looked at)."""
    rx, ry, rz = res
    w = np.asarray(words).view(np.uint32)
    c = np.arange(rx * ry * rz)
    return ((w[c >> 5] >> (c & 31).astype(np.uint32)) & 1).astype(bool).reshape(rz, ry, rx)


def np_cell(p, lo, inv, r):
    """c_a = min(max((int)floorf((p_a - lo_a) * inv_a), 0), R_a - 1): the subtraction and the product separate fp32 operations
    (the clamp is taken before the conversion, which changes nothing and keeps huge values in range)."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (np.asarray(p, F32) - F32(lo)).astype(F32)
        f = np.floor((d * F32(inv)).astype(F32))
        return np.clip(np.nan_to_num(f, nan=0.0, posinf=r - 1, neginf=0.0), 0, r - 1).astype(np.int64)


def np_points_occupied(xyz, occupied, lo, inv):
    """xyz (..., 3) fp32 -> bool (...): the point's cell is occupied; a point with a NaN coordinate counts as occupied."""
    occ = np.asarray(occupied, bool)
    rz, ry, rx = occ.shape
    x = np.asarray(xyz, F32)
    cx, cy, cz = (np_cell(x[..., a], lo[a], inv[a], r) for a, r in ((0, rx), (1, ry), (2, rz)))
    return occ[cz, cy, cx] | np.isnan(x).any(-1)


def np_keep(xyz, occupied, lo, inv):
    """xyz (n, n1, 3) -> keep (n,) bool: one of the pair's n1 points lies in an occupied cell."""
    return np_points_occupied(xyz, occupied, lo, inv).any(-1)


def np_cull(xyz, mask, table):
    """xyz (n,l,n1,3), mask (n,l) uint8, table: per layer None | (occupied, lo, inv) -> (the mask after the cull, counts (l,2)):
    bit 0 cleared where it was set and no point is in an occupied cell; nothing else changes."""
    out = np.array(mask, np.uint8, copy=True)
    counts = np.zeros((out.shape[1], 2), np.int64)
    for i, g in enumerate(table):
        if g is None:
            continue
        tested = (out[:, i] & 1) != 0
        keep = np_keep(xyz[:, i], *g)
        out[tested & ~keep, i] &= np.uint8(0xFE)
        counts[i] = int(tested.sum()), int((tested & ~keep).sum())
    return out, counts


# ---------------------------------------------------------------------------------------- test grids
def half_y(res=8):
    """Lower half in y occupied, [Rz][Ry][Rx]."""
    occ = np.zeros((res, res, res), bool)
    occ[:, :res // 2, :] = True
    return occ


def ball(res=8, radius=0.3):
    """Centred ball: the cells whose centre is within ``radius`` (in units of the box's extent per axis) of the box's centre."""
    c = (np.arange(res) + 0.5) / res - 0.5
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    return (x * x + y * y + z * z) <= radius * radius


def half_x(res=8):
    """Lower half in x occupied: splits the rays of ONE image row (the first rows of the view graze the boxes' y faces)."""
    occ = np.zeros((res, res, res), bool)
    occ[:, :, :res // 2] = True
    return occ


GRIDS = {"half": half_y, "ball": ball, "half_x": half_x}


# ---------------------------------------------------------------------------------------- the oracle's expectation
def plain_case(**over):
    """The base scene of scene_edits_common WITHOUT edits: no scale, shift, rotation or opacity table (the instance stays)."""
    kw = dict(scale=None, shift=None, rotation=None, layer_alpha=None)
    kw.update(over)
    return S.make_case(**kw)


def case_table(case):
    """The box table (F, L + K, 8, 3) of the case: the synthetic scene's, the instances' columns copied from their sources."""
    _, _, per = S._state(case["L"])
    return torch.cat([per] + [per[:, s - 1:s] for s in case["sources"]], 1)


def layer_bounds(case, layer, group=0):
    """lo, hi of layer >= 1's UNEDITED box at its frame id (of chunk group ``group``), from the case's own spec."""
    table = case_table(case).float()
    if case["frame"] is not None:
        return np_bounds(table[int(case["frame"]) - 1, layer - 1])
    f = torch.tensor(case["groups"][group][1][layer], dtype=torch.float32) - 1
    return np_bounds(torch.lerp(table[math.floor(f), layer - 1], table[math.ceil(f), layer - 1], f - math.floor(f)))


def case_pivot(case):
    """The edit pivot of the case in fp32, as the oracle makes it (None without a scale)."""
    return O.layer_boxes(S.oracle_model(case), S.case_rays(case)[:1])[1]


def manual_grids(case, name, dilate=0, res=8, layers=None):
    """{layer: (occupied [Rz][Ry][Rx], lo, hi)}: the named test grid, grown by ``dilate``, over each performer's bounds."""
    layers = range(1, S.total_layers(case)) if layers is None else layers
    occ = np_dilate(GRIDS[name](res), dilate)
    return {i: (occ,) + layer_bounds(case, i) for i in layers}


def culled_sampler(case, grids, record=None):
    """The wrapper for ``O.sample_coarse``: calls the original, un-edits the returned points from the case's own spec (shift, then
    scale about the pivot, as the oracle's coarse ``unedit`` does), and ANDs each gridded performer's mask with the numpy keep.
    The rule is an fp32 one: an fp64 oracle's masks take the keep of the fp32 points of the same call.
    grids: {layer: (occupied, lo, hi)}.  record (a list): gets {layer: (mask before, keep)} per call."""
    original = O.sample_coarse
    pivot = case_pivot(case)

    def unedit(x, i):
        if case["shift"] is not None and i < len(case["shift"]) and case["shift"][i] is not None:
            x = x - torch.tensor(case["shift"][i], dtype=x.dtype)
        if case["scale"] is not None and i < len(case["scale"]):
            x = (x - pivot) / case["scale"][i] + pivot
        return x

    def wrapped(rays, boxes, n_coarse, jitter, layer_rays=None):
        ts, pts, masks = original(rays, boxes, n_coarse, jitter, layer_rays)
        pts32 = pts
        if rays.dtype != torch.float32:
            f = lambda t: t.float()
            _, pts32, _ = original(f(rays), f(boxes), n_coarse, [f(j) for j in jitter], None if layer_rays is None else [f(r) for r in layer_rays])
        seen = {}
        for i, (occ, lo, hi) in grids.items():
            res = (occ.shape[2], occ.shape[1], occ.shape[0])
            keep = torch.from_numpy(np_keep(unedit(pts32[i], i).numpy(), occ, lo, np_inv_cell(res, lo, hi)))
            seen[i] = (masks[i].clone(), keep)
            masks[i] = masks[i] & keep
        if record is not None:
            record.append(seen)
        return ts, pts, masks

    return wrapped


def kept_and_culled(record):
    """{layer: (kept pairs, culled pairs)} among the hit rays, summed over the recorded calls."""
    out = {}
    for seen in record:
        for i, (before, keep) in seen.items():
            k, c = out.get(i, (0, 0))
            out[i] = (k + int((before & keep).sum()), c + int((before & ~keep).sum()))
    return out


def assert_cull_bites(record, what=""):
    """The condition on the inputs of every oracle-compared case: each culled layer has at least 8 kept and at least 8 culled
    pairs among its hit rays."""
    counts = kept_and_culled(record)
    assert counts, what
    for i, (kept, culled) in counts.items():
        assert kept >= 8 and culled >= 8, f"{what}: layer {i} has {kept} kept and {culled} culled pairs among its hit rays"
    return counts
