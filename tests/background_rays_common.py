"""Shared by tests/test_background_rays_cpu.py and tests/test_gpu_background_rays.py: the per-ray background mask (include/stnerf.h:
"Per-ray background mask") restated in numpy from that text.  In a stage of ns samples, sample k of ray r is
LISTED if and only if
  the ray's flag byte is nonzero, and
  with a grid, the point xyz[r][k] lies in an occupied cell or has a NaN coordinate (``occupancy_common.np_points_occupied``, the
  existing point -> cell rule, unchanged), and
  with a stop depth, ``not t[r][k] > t_stop[r]`` (a NaN depth is not hidden);
a sample that is not listed gets four zero words; counts += (n ns, samples not listed)."""
import numpy as np

import occupancy_common as OC
import sample_rows_common as SR

BLOCK_CAP = 2048         # the rows kernels' persistent grid: at most this many workgroups of 4 waves, 16 rays per wave and run
RUN = 16


def np_background_ray_rows(flags, ns, xyz=None, grid=None, t=None, t_stop=None):
    """flags (n,) uint8; xyz (n, ns, 3) fp32 and grid = (occupied [Rz][Ry][Rx], lo, inv_cell) or None; t (n, ns) and t_stop (n,) or
    None -> (the sorted words ``ray << 8 | k`` of the listed samples, listed (n, ns) bool)."""
    occupied = None if grid is None else OC.np_points_occupied(np.asarray(xyz, np.float32), *grid)
    return SR.np_sample_rows(np.asarray(flags).shape[0], ns, flags=flags, t=t, t_stop=t_stop, occupied=occupied)


def flag_pattern(name, n, seed=0):
    """The masks of the kernel test, (n,) uint8 with nonzero values other than 1 among them."""
    f = np.zeros(n, np.uint8)
    if name == "all on":
        f[:] = 1
        f[::3] = 0x80                                    # (any nonzero byte is "on")
    elif name == "alternating":
        f[::2] = 1
    elif name == "one whole run off":
        f[:] = 7
        f[RUN:2 * RUN] = 0                               # the second run of 16 (nothing at n <= 16: then every ray is on)
    elif name == "off only in the ragged last run":
        f[:] = 1
        f[n // RUN * RUN:] = 0                           # the rays past the last whole run (none when 16 divides n)
    elif name == "random":
        f[:] = np.random.RandomState(seed).rand(n) < 0.5
    else:
        assert name == "all off", name
    return f


FLAG_PATTERNS = ["all on", "all off", "alternating", "one whole run off", "off only in the ragged last run"]


def rows_per_ray_are_contiguous_and_ascending(words):
    """The rows of one ray are contiguous in the list and ascending in k; the order of the rays is free (vectorised: the list of a
    large launch has 4e5 words)."""
    words = np.asarray(words, np.int64)
    if words.size == 0:
        return True
    ray, k = words >> 8, words & 255
    new_ray = np.ones(words.size, bool)
    new_ray[1:] = ray[1:] != ray[:-1]
    ascending = bool(np.all((k[1:] > k[:-1]) | new_ray[1:]))
    return ascending and int(new_ray.sum()) == np.unique(ray).size        # (as many segments as rays: no ray comes back)
