"""Shared by the numpy restatements of the four rows calls (tests/sample_cull_common.py, termination_common.py,
background_grid_common.py, background_rays_common.py): the row-list rule (include/stnerf.h: "Row lists")
restated once from that text.  In a stage of ns samples, sample k of a tested ray r is LISTED if and only if
  with a per-ray mask, the ray's flag byte is nonzero, and
  with a stop depth, ``not t[r][k] > t_stop[r]`` (a NaN depth is not hidden), and
  with a grid, the point's cell is occupied (the caller's verdict: ``occupancy_common.np_points_occupied``);
the tested rays are those of a ray list, or every ray.  A sample of a tested ray that is not listed gets four zero words."""
import numpy as np


def np_sample_rows(n, ns, rays=None, flags=None, t=None, t_stop=None, occupied=None):
    """rays: the tested ray indices (any order) | None (every ray); flags (n,) uint8 | None; t (n, ns) and t_stop (n,) | None;
    occupied (n, ns) bool | None (read on the tested rays only) -> (the sorted words ``ray << 8 | k`` of the listed samples, listed
    (n, ns) bool with False on rays not tested)."""
    rays = np.arange(n, dtype=np.int64) if rays is None else np.asarray(rays, np.int64)
    keep = np.ones((rays.size, ns), bool)
    if flags is not None:
        keep &= (np.asarray(flags)[rays] != 0)[:, None]
    if t_stop is not None:
        with np.errstate(invalid="ignore"):
            keep &= ~(np.asarray(t)[rays] > np.asarray(t_stop)[rays][:, None])
    if occupied is not None:
        keep &= np.asarray(occupied)[rays]
    listed = np.zeros((n, ns), bool)
    listed[rays] = keep
    r, k = np.nonzero(listed)
    return np.sort((r.astype(np.int64) << 8) | k.astype(np.int64)), listed
