"""Shared by tests/test_sample_cull_cpu.py and tests/test_gpu_sample_cull.py: the sample cull's rule (DESIGN.md section 7 /
include/stnerf.h: "Sample cull") restated in numpy from that text -- a sample is LISTED when its point lies in an occupied cell or
has a NaN coordinate (``occupancy_common.np_points_occupied``, the existing point -> cell rule, unchanged), a sample that is not
listed gets four zero words -- and the oracle's expectation of a sample-culled render: ``O.motion_net`` / ``O.space_net`` wrapped
(by the test, with pytest's monkeypatch) so that a gridded performer's colour and sigma are zeroed at its not-listed samples."""
import numpy as np
import torch

from oracle import stnerf_oracle as O

import occupancy_common as OC
import sample_rows_common as SR
import scene_edits_common as S


def grid_entry(occ, lo, hi):
    """(occupied [Rz][Ry][Rx], lo, hi) -> the numpy form of the table entry: (occupied, lo, inv_cell)."""
    res = (occ.shape[2], occ.shape[1], occ.shape[0])
    return occ, np.asarray(lo, np.float32), OC.np_inv_cell(res, lo, hi)


def device_entry(occ, lo, hi):
    """... -> what ``ops.occupancy_rows`` / ``ops.occupancy_cull`` take: (bits int32 on the GPU, res, lo, inv_cell)."""
    res = (occ.shape[2], occ.shape[1], occ.shape[0])
    return (torch.from_numpy(OC.np_pack(occ).view(np.int32)).cuda(), res, np.asarray(lo, np.float32).tolist(),
            OC.np_inv_cell(res, lo, hi).tolist())


def checker_xz(res=(8, 8, 8), block=2, odd=False):
    """A checkerboard of ``block``-cell squares in x and z, the same at every y, [Rz][Ry][Rx] for res = (Rx, Ry, Rz): a ray that
    runs along the x-z plane alternates between occupied and empty cells -- listed and skipped samples on almost every kept ray,
    also among the view's first rows, which cross the boxes in a few cell layers of y only (``half`` in y keeps or drops such rays
    whole).  ``odd``: the other colour of the board."""
    rx, ry, rz = res
    z, _, x = np.meshgrid(np.arange(rz) // block, np.arange(ry), np.arange(rx) // block, indexing="ij")
    return (x + z) % 2 == (1 if odd else 0)


def checker_grids(case, layers, res=(8, 8, 8), block=2, odd=False):
    """{layer: (occupied, lo, hi)}: the checkerboard over each layer's bounds (``occupancy_common.manual_grids``'s form)."""
    return {i: (checker_xz(res, block, odd),) + OC.layer_bounds(case, i) for i in layers}


def grids_64(case):
    """The grids of the 64 + 64 case on the view's first 64 rays (layers 1 and 3; layer 2 has 5 hit pairs there): a 4 x 1 x 4
    board.  Those rows only graze the boxes' tops -- 16 to 18 hit rays per layer, none crossing a mid-plane -- and at 128 fine
    samples per ray the res-8 grids leave 7 of the 64 rays within eps of a face, more than the 5 % the comparison may leave out;
    res 4 without faces in y leaves 1 (tests/test_sample_cull_cpu.py measures it)."""
    return checker_grids(case, (1, 3), res=(4, 1, 4), block=1, odd=True)


def np_listed(xyz, grid):
    """xyz (..., ns, 3) fp32, grid = (occupied, lo, inv_cell) -> bool (..., ns): the sample is listed."""
    return OC.np_points_occupied(np.asarray(xyz, np.float32), *grid)


def np_rows(xyz, rays, grid):
    """One layer's expected row list.  xyz (n, ns, 3); rays: the listed ray indices (any order) -> (the sorted words
    ``ray << 8 | k`` of the listed samples of those rays, listed (n, ns) bool with False on rays not tested)."""
    rays = np.asarray(rays, np.int64)
    occupied = np.zeros(xyz.shape[:2], bool)
    occupied[rays] = np_listed(xyz[rays], grid)
    return SR.np_sample_rows(xyz.shape[0], xyz.shape[1], rays=rays, occupied=occupied)


def rows_are_contiguous_and_ascending(words):
    """The rows of one ray are contiguous in the list and ascending in k (the order of the rays is free)."""
    words = np.asarray(words, np.int64)
    ray, k = words >> 8, words & 255
    seen, prev_ray, prev_k = set(), None, -1
    for r, kk in zip(ray.tolist(), k.tolist()):
        if r != prev_ray:
            if r in seen:
                return False
            seen.add(r)
            prev_ray, prev_k = r, -1
        if kk <= prev_k:
            return False
        prev_k = kk
    return True


def interior_face_distance(x, lo, hi, res):
    """x (..., 3) -> (...): the distance of each point to the nearest INTERIOR cell face of the grid, per axis the planes
    lo_a + j (hi_a - lo_a) / R_a, j = 1 .. R_a - 1.  The outer faces (j = 0, R_a) separate nothing: a point beyond them is clamped
    into the border cell on their inner side, so no classification changes across them."""
    x = np.asarray(x, np.float64)
    best = np.full(x.shape[:-1], np.inf)
    for a in range(3):
        r = res[a]
        if r < 2:
            continue
        planes = float(lo[a]) + np.arange(1, r) * ((float(hi[a]) - float(lo[a])) / r)
        best = np.minimum(best, np.abs(x[..., a, None] - planes).min(-1))
    return best


# ---------------------------------------------------------------------------------------- the oracle's expectation
def case_keys(case, grids):
    """{(module index, frame id): (layer, (occupied, lo, inv_cell), (lo, hi, res))} over every chunk group of the case: what a
    ``time_deform_nets.<module>`` call with that frame id column belongs to.  Two layers on one key (an instance at its source's
    frame id) must carry the same grid: then it does not matter which of them a call is."""
    m = S.oracle_model(case)
    ids = [[float(case["frame"])] * S.total_layers(case)] if case["frame"] is not None else [list(g[1]) for g in case["groups"]]
    keys = {}
    for row in ids:
        for i, (occ, lo, hi) in grids.items():
            key = (m.module_of(i), float(np.float32(row[i])))
            entry = (i, grid_entry(occ, lo, hi), (np.asarray(lo, np.float32), np.asarray(hi, np.float32), (occ.shape[2], occ.shape[1], occ.shape[0])))
            if key in keys and keys[key][0] != i:
                o = keys[key]
                assert np.array_equal(o[1][0], entry[1][0]) and np.array_equal(o[1][1], entry[1][1]) and np.array_equal(o[1][2], entry[1][2]), key
            keys.setdefault(key, entry)
    return keys


class SampledNets:
    """The wrappers for ``O.motion_net`` and ``O.space_net`` (the case must deform its performers: every performer SpaceNet call
    is then preceded by the MotionNet call on the same rows).  The MotionNet wrapper notes the call's UNDEFORMED points -- the
    points the rule speaks of -- with its flow; the SpaceNet wrapper finds the note whose points + flow are its input, applies the
    rule to the fp32 value of those undeformed points, and zeroes colour and sigma at the samples that are not listed.  A call of
    a layer without a grid, and the background's, pass through.  ``calls``: per sample-culled SpaceNet call, in call order,
    (layer, undeformed points (m, ns, 3) as given, listed (m, ns) bool, (lo, hi, res))."""

    def __init__(self, case, grids):
        self.keys = case_keys(case, grids)
        self.motion, self.space = O.motion_net, O.space_net
        self.notes, self.calls = [], []

    def motion_net(self, params, prefix, xyzt, input_time=True):
        flow = self.motion(params, prefix, xyzt, input_time=input_time)
        if prefix.startswith("time_deform_nets."):
            key = (int(prefix.rsplit(".", 1)[1]), float(np.float32(float(xyzt[0, 0, 3]))))
            if key in self.keys:
                self.notes.append((key, xyzt[..., :3].detach().clone(), flow.detach().clone()))
        return flow

    def space_net(self, params, prefix, pos, dirs, times=None):
        rgb, sigma = self.space(params, prefix, pos, dirs, times)
        if not prefix.startswith("spacenets"):
            return rgb, sigma
        for j, (key, und, flow) in enumerate(self.notes):
            if und.shape == pos.shape and int(prefix.rsplit(".", 1)[1]) == key[0] and torch.equal(und + flow, pos.detach()):
                layer, grid, geo = self.keys[key]
                listed = np_listed(und.float().numpy(), grid)
                self.calls.append((layer, und, listed, geo))
                del self.notes[j]
                off = torch.from_numpy(~listed)
                rgb, sigma = rgb.clone(), sigma.clone()
                rgb[off] = 0
                sigma[off] = 0
                break
        return rgb, sigma


def oracle_render_sampled(case, grids_ray, grids_sample, rays, dtype, monkeypatch):
    """The oracle on the case with the ray cull (``occupancy_common.culled_sampler`` on ``grids_ray``) and the sample cull
    (``SampledNets`` on ``grids_sample``) -> (``scene_edits_common.flat`` dict with t_coarse, per reference chunk the list of
    sample-culled calls with the chunk's masks: [(first ray, masks, calls)])."""
    rays = rays.to(torch.float32)
    m = S.oracle_model(case, dtype)
    jitter, u = S.case_draws(case)
    l, step = S.total_layers(case), case["chunk"]
    monkeypatch.setattr(O, "sample_coarse", OC.culled_sampler(case, grids_ray))
    nets = SampledNets(case, grids_sample)
    monkeypatch.setattr(O, "motion_net", nets.motion_net)
    monkeypatch.setattr(O, "space_net", nets.space_net)
    outs, ts, chunks = [], [], []
    try:
        with torch.no_grad():
            for s in range(0, rays.shape[0], step):
                e = min(s + step, rays.shape[0])
                draws = iter([jitter[i, s:e] for i in range(l)] + [u[i, s:e] for i in range(l)])
                trace = {}
                nets.notes, nets.calls = [], []
                outs.append(O.render_chunk(m, rays[s:e].to(dtype), only_coarse=case["only_coarse"], rand=lambda shape: next(draws),
                                           trace=trace, scene=True, density_threshold=case["thr"], bkgd_density_threshold=case["bthr"]))
                ts.append(torch.stack([t.squeeze(-1) for t in trace["t_coarse"]], 1))
                chunks.append((s, [mk.clone() for mk in trace["mask"]], nets.calls))
    finally:
        monkeypatch.undo()
    cat3 = lambda trips: tuple(torch.cat([t[j] for t in trips], 0) for j in range(3))
    whole = (cat3([o[0] for o in outs]), cat3([o[1] for o in outs]))
    whole += tuple([cat3([o[k][i] for o in outs]) for i in range(l)] for k in (2, 3))
    whole += ([torch.cat([o[4][i] for o in outs], 0) for i in range(l)], [cat3([o[5][i] for o in outs]) for i in range(l)])
    return S.flat(whole, torch.cat(ts, 0)), chunks


def per_ray(chunks, n, ns, what):
    """The chunks' calls of the stage with ``ns`` samples, scattered to rays -> {layer: (value (n, ns, ...) of ``what(call)``,
    present (n,) bool)}; what(call) -> an array (m, ns, ...)."""
    out = {}
    for first, masks, calls in chunks:
        for layer, und, listed, geo in calls:
            if und.shape[1] != ns:
                continue
            rows = first + np.nonzero(masks[layer].numpy())[0]
            assert rows.shape[0] == und.shape[0], (layer, rows.shape, und.shape)
            v = np.asarray(what((layer, und, listed, geo)))
            if layer not in out:
                out[layer] = (np.zeros((n,) + v.shape[1:], v.dtype), np.zeros(n, bool))
            out[layer][0][rows] = v
            out[layer][1][rows] = True
    return out


def fine_point_gap_and_excluded(case, chunks32, chunks64, n):
    """-> (the largest distance between the fp32 and the fp64 oracle's undeformed fine points over the gridded layers' rays that
    both evaluate, eps = 4 x that, excluded (n,) bool: the rays on which a gridded layer's fp32 fine point lies within eps of an
    interior cell face of its grid)."""
    ns = case["n1"] + case["n2"]
    p32 = per_ray(chunks32, n, ns, lambda c: c[1].double().numpy())
    p64 = per_ray(chunks64, n, ns, lambda c: c[1].double().numpy())
    gap = 0.0
    for layer, (x32, has32) in p32.items():
        x64, has64 = p64[layer]
        both = has32 & has64
        if both.any():
            gap = max(gap, float(np.sqrt(((x32[both] - x64[both]) ** 2).sum(-1)).max()))
    eps = 4.0 * gap
    dist = per_ray(chunks32, n, ns, lambda c: interior_face_distance(c[1].double().numpy(), *c[3]))
    excluded = np.zeros(n, bool)
    for layer, (d, has) in dist.items():
        excluded |= has & (np.where(has[:, None], d, np.inf).min(-1) <= eps)
    return gap, eps, excluded


def rays_with_listed_and_skipped(chunks, n, ns):
    """{layer: the number of rays of the stage with ``ns`` samples that have both listed and skipped samples}."""
    out = {}
    for layer, (listed, has) in per_ray(chunks, n, ns, lambda c: c[2]).items():
        out[layer] = int((has & listed.any(-1) & ~listed.all(-1)).sum())
    return out


def assert_sample_cull_bites(chunks, case, n, what=""):
    """The condition on every oracle-compared case, in the manner of ``occupancy_common.assert_cull_bites``: at least 8 rays with
    both listed and skipped samples on a gridded layer, in every stage the case runs."""
    stages = [case["n1"]] + ([] if case["only_coarse"] else [case["n1"] + case["n2"]])
    for ns in stages:
        counts = rays_with_listed_and_skipped(chunks, n, ns)
        assert counts and max(counts.values()) >= 8, f"{what}: stage of {ns} samples: rays with listed and skipped samples per layer {counts}"
    return counts
