"""Shared by tests/test_background_grid_cpu.py and tests/test_gpu_background_grid.py: the background's sample cull (DESIGN.md
section 7 / include/stnerf.h: "Background sample cull") restated in numpy from that text -- in a stage of ns samples and on EVERY
ray, sample k is LISTED when the point xyz[ray][0][k] lies in an occupied cell or has a NaN coordinate
(``occupancy_common.np_points_occupied``, the existing point -> cell rule, unchanged) and, with early ray termination on layer 0,
is not hidden (``not t > t_stop``); a sample that is not listed gets four zero words -- and the oracle's expectation of a render
under a background grid: ``O.space_net`` wrapped (by the test, with pytest's monkeypatch) so that the background's colour and sigma
are zero at its not-listed samples, which is ``sig[0]`` / ``rgbs[0]`` zeroed at the return of ``run_nets`` in both stages: the cut
and the factor between the network and that return keep a zero a zero."""
import numpy as np
import torch

from oracle import stnerf_oracle as O

import occupancy_common as OC
import sample_cull_common as SC
import sample_rows_common as SR
import scene_edits_common as S

EPS = 5.5e-5      # the project's fp32 / fp64 point spread (tests/termination_common.py, tests/test_sample_cull_cpu.py: "full edits")


# ---------------------------------------------------------------------------------------- the rule
def np_background_rows(xyz, grid, t=None, t_stop=None):
    """Layer 0's expected row list of one stage.  xyz (n, ns, 3) fp32, grid = (occupied [Rz][Ry][Rx], lo, inv_cell); t (n, ns) and
    t_stop (n,) or None -> (the sorted words ``ray << 8 | k`` of the listed samples of every ray, listed (n, ns) bool)."""
    occupied = OC.np_points_occupied(np.asarray(xyz, np.float32), *grid)
    return SR.np_sample_rows(xyz.shape[0], xyz.shape[1], t=t, t_stop=t_stop, occupied=occupied)


def bkgd_bounds(case):
    """lo, hi (fp32) of the 8 corners of the case's UNEDITED background box."""
    _, bk, _ = S._state(case["L"])
    return OC.np_bounds(bk)


def checker_grid(case, res=(4, 4, 4), block=1, odd=False):
    """(occupied, lo, hi): an x-z checkerboard over the background's box, the same at every y."""
    return (SC.checker_xz(res, block, odd),) + bkgd_bounds(case)


def attach_background(model, grid, **kw):
    """A manual background grid (occupied, lo, hi) on the model, nothing on the performers -> the OccupancyGrids."""
    from stnerf_amd.occupancy import OccupancyGrids
    grids = OccupancyGrids(auto=False, **kw)
    occ, lo, hi = grid
    grids.set_background_manual(torch.from_numpy(np.ascontiguousarray(occ)), lo, hi)
    model.set_occupancy(grids)
    return grids


# ---------------------------------------------------------------------------------------- the oracle's expectation
class BackgroundNets:
    """The wrapper for ``O.space_net``: a call of ``bkgd_spacenet`` / ``bkgd_spacenet_fine`` (the case does not deform the
    background: ``pos`` is the point the rule speaks of) gets colour and sigma zeroed at the samples the rule does not list, on
    the fp32 value of its points; every other call passes through.  ``calls``: per background call (points (n, ns, 3) as
    given, listed (n, ns) bool)."""

    def __init__(self, grid):
        occ, lo, hi = grid
        self.grid = SC.grid_entry(occ, lo, hi)
        self.space = O.space_net
        self.calls = []

    def space_net(self, params, prefix, pos, dirs, times=None):
        rgb, sigma = self.space(params, prefix, pos, dirs, times)
        if prefix not in ("bkgd_spacenet", "bkgd_spacenet_fine"):
            return rgb, sigma
        listed = OC.np_points_occupied(pos.detach().float().numpy(), *self.grid)
        self.calls.append((pos.detach().clone(), listed))
        off = torch.from_numpy(~listed)
        rgb, sigma = rgb.clone(), sigma.clone()
        rgb[off] = 0
        sigma[off] = 0
        return rgb, sigma


def oracle_render_background(case, grid, rays, dtype, monkeypatch):
    """The oracle on the case under the background grid -> (``scene_edits_common.flat`` dict with t_coarse, {ns: (points
    (n, ns, 3), listed (n, ns))} of the background per stage)."""
    rays = rays.to(torch.float32)
    m = S.oracle_model(case, dtype)
    assert not m.bkgd_use_deform_time
    jitter, u = S.case_draws(case)
    l, step = S.total_layers(case), case["chunk"]
    nets = BackgroundNets(grid)
    monkeypatch.setattr(O, "space_net", nets.space_net)
    outs, ts = [], []
    try:
        with torch.no_grad():
            for s in range(0, rays.shape[0], step):
                e = min(s + step, rays.shape[0])
                draws = iter([jitter[i, s:e] for i in range(l)] + [u[i, s:e] for i in range(l)])
                trace = {}
                outs.append(O.render_chunk(m, rays[s:e].to(dtype), only_coarse=case["only_coarse"], rand=lambda shape: next(draws),
                                           trace=trace, scene=True, density_threshold=case["thr"], bkgd_density_threshold=case["bthr"]))
                ts.append(torch.stack([t.squeeze(-1) for t in trace["t_coarse"]], 1))
    finally:
        monkeypatch.undo()
    cat3 = lambda trips: tuple(torch.cat([t[j] for t in trips], 0) for j in range(3))
    whole = (cat3([o[0] for o in outs]), cat3([o[1] for o in outs]))
    whole += tuple([cat3([o[k][i] for o in outs]) for i in range(l)] for k in (2, 3))
    whole += ([torch.cat([o[4][i] for o in outs], 0) for i in range(l)], [cat3([o[5][i] for o in outs]) for i in range(l)])
    stages = {}
    for ns in sorted({c[0].shape[1] for c in nets.calls}):
        stages[ns] = (torch.cat([c[0] for c in nets.calls if c[0].shape[1] == ns], 0).double().numpy(),
                      np.concatenate([c[1] for c in nets.calls if c[0].shape[1] == ns], 0))
    return S.flat(whole, torch.cat(ts, 0)), stages


def excluded_rays(stages, grid):
    """(n,) bool: the rays with a background point, of either stage, within EPS of an interior cell face of the grid."""
    occ, lo, hi = grid
    res = (occ.shape[2], occ.shape[1], occ.shape[0])
    out = None
    for ns, (pts, _) in stages.items():
        near = (SC.interior_face_distance(pts, lo, hi, res) <= EPS).any(-1)
        out = near if out is None else (out | near)
    return out


def rays_with_listed_and_skipped(stages, keep=None):
    """{ns: the number of (kept) rays of that stage whose background has both listed and skipped samples}."""
    out = {}
    for ns, (_, listed) in stages.items():
        both = listed.any(-1) & ~listed.all(-1)
        out[ns] = int((both if keep is None else both & keep).sum())
    return out


def assert_conditions(case, stages, grid, what=""):
    """The two conditions of every oracle-compared case, on the oracle alone: at most 5 % of the rays left out, at least 8 rays
    with both listed and skipped background samples in each stage the case runs -> (excluded (n,) bool, {ns: count})."""
    excluded = excluded_rays(stages, grid)
    want = [case["n1"]] + ([] if case["only_coarse"] else [case["n1"] + case["n2"]])
    assert sorted(stages) == want, (what, sorted(stages), want)
    counts = rays_with_listed_and_skipped(stages, ~excluded)
    assert excluded.mean() <= 0.05, f"{what}: {int(excluded.sum())} of {excluded.size} rays left out"
    assert min(counts.values()) >= 8, f"{what}: rays with listed and skipped background samples per stage {counts}"
    return excluded, counts
