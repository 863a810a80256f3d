"""The four rows calls are one kernel (csrc/sample_rows.hip), so where two of them are asked for the same tests on the same rays
they must agree in everything a caller can see: the listed words (sorted: the order of the runs is free), the per-ray order
(contiguous, ascending in k), the raw bits over poison (zeros at exactly the same samples, every other byte kept), the words past
the count, and what is added to the counters.  Each call is pinned to the numpy restatement by its own test file; these are the
agreements BETWEEN the calls, on the data of tests/test_gpu_background_rays.py's kernel test (a NaN coordinate, a clamped point, a
tie t == t_stop, a NaN depth), at the edges of a run of 16 rays (n) and of every NC = ceil(ns / 64)."""
import functools

import numpy as np
import pytest
import torch

import background_rays_common as BR
import test_gpu_background_grid as BGT
import test_gpu_background_rays as BRT
from pipeline_chain import bits
from stnerf_amd import ops

pytestmark = pytest.mark.gpu

POISON = BGT.POISON
SHAPES = [(n, ns) for n in (1, 16, 17, 197) for ns in (1, 64, 65, 129, 256)]
L = 2                                  # the layers of the case's arrays; every call below works on slice 0 of them


@functools.lru_cache(maxsize=None)
def _case(n, ns):
    """The kernel case on the device, made once per shape and left unchanged: points, depths, stop depths, the grid."""
    xyz, t, stop, _, g_dev = BRT._kernel_case(n, ns)
    return torch.from_numpy(xyz).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(stop).cuda(), g_dev


def _launch(n, ns, call, counts):
    """call(raw slice, row_list, row_count, counts) over poisoned buffers of exactly n x ns words (and canaries around them) ->
    (the words in list order, the raw bits)."""
    cap = n * ns
    raw = torch.full((n, L, ns, 4), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    buf = torch.full((cap + 16,), POISON, dtype=torch.int32, device="cuda")
    count = torch.full((3,), POISON, dtype=torch.int32, device="cuda")
    call(raw[:, 0], buf[:cap], count[1:2], counts)
    torch.cuda.synchronize()
    got_n = int(count[1])
    assert 0 <= got_n <= cap and int(count[0]) == POISON and int(count[2]) == POISON
    assert bool((buf[got_n:] == POISON).all())                     # no word past the count, none past the capacity
    return buf[:got_n].cpu().numpy().astype(np.int64), bits(raw).cpu()


def _agree(what, n, ns, tested, call_a, counts_a, row_a, call_b, counts_b, row_b):
    """Both calls list the same words in a valid order, leave the same raw bits and add the same (tested, not listed)."""
    start_a, start_b = counts_a.clone(), counts_b.clone()
    words_a, raw_a = _launch(n, ns, call_a, counts_a)
    words_b, raw_b = _launch(n, ns, call_b, counts_b)
    assert np.array_equal(np.sort(words_a), np.sort(words_b)), what
    assert BR.rows_per_ray_are_contiguous_and_ascending(words_a) and BR.rows_per_ray_are_contiguous_and_ascending(words_b), what
    assert torch.equal(raw_a, raw_b), what
    assert bool((raw_a[:, 1] == POISON).all()), what               # the other layer's slice is not touched
    added_a, added_b = (counts_a - start_a).cpu(), (counts_b - start_b).cpu()
    want = [tested, tested - len(words_a)]
    assert added_a.reshape(-1, 2)[row_a].tolist() == want and added_b.reshape(-1, 2)[row_b].tolist() == want, what
    assert int(added_a.abs().sum()) == int(added_b.abs().sum()) == sum(want), what     # ... and to no other row


def _layer_counts():
    return torch.tensor([[5, 3], [11, 7], [77, 78]], dtype=torch.int64, device="cuda")


def _own_counts():
    return torch.tensor([5, 3], dtype=torch.int64, device="cuda")


def test_visibility_rows_without_a_stop_is_occupancy_rows():
    """t_stop = +inf hides nothing (not even a NaN depth), so the depth test drops out: the same ray list, the same device count."""
    for n, ns in SHAPES:
        x, t, _, g = _case(n, ns)
        never = torch.full((n,), float("inf"), device="cuda")
        rays = torch.from_numpy(np.random.RandomState(n + ns).permutation(n).astype(np.int32)).cuda()
        for c in sorted({n, n // 2, 0}):
            rc = torch.tensor([c], dtype=torch.int32, device="cuda")
            _agree((n, ns, c), n, ns, c * ns,
                   lambda raw, rl, cnt, counts: ops.visibility_rows(t[:, 0], never, raw, xyz=x[:, 0], grid=g, layer=1, ray_list=rays, ray_count=rc,
                                                                    row_list=rl, row_count=cnt, counts=counts), _layer_counts(), 1,
                   lambda raw, rl, cnt, counts: ops.occupancy_rows(x[:, 0], raw, g, layer=1, ray_list=rays, ray_count=rc, row_list=rl,
                                                                   row_count=cnt, counts=counts), _layer_counts(), 1)


def test_visibility_rows_on_every_ray_is_background_rows():
    """Without a ray list the slot is the ray, which is how the background's call walks: the first adds to row 1 of its counter
    table, the second to its own two words."""
    for n, ns in SHAPES:
        x, t, stop, g = _case(n, ns)
        _agree((n, ns), n, ns, n * ns,
               lambda raw, rl, cnt, counts: ops.visibility_rows(t[:, 0], stop, raw, xyz=x[:, 0], grid=g, layer=1, row_list=rl, row_count=cnt,
                                                                counts=counts), _layer_counts(), 1,
               lambda raw, rl, cnt, counts: ops.background_rows(x[:, 0], raw, g, t=t[:, 0], t_stop=stop, row_list=rl, row_count=cnt,
                                                                counts=counts), _own_counts(), 0)


def test_background_ray_rows_with_every_flag_on_is_visibility_rows_of_layer_0():
    """Every flag on and no grid leaves the depth test alone, which is layer 0 under early ray termination without a grid."""
    for n, ns in SHAPES:
        x, t, stop, _ = _case(n, ns)
        flags = torch.from_numpy(BR.flag_pattern("all on", n)).cuda()
        _agree((n, ns), n, ns, n * ns,
               lambda raw, rl, cnt, counts: ops.background_ray_rows(x[:, 0], raw, flags, t=t[:, 0], t_stop=stop, row_list=rl, row_count=cnt,
                                                                    counts=counts), _own_counts(), 0,
               lambda raw, rl, cnt, counts: ops.visibility_rows(t[:, 0], stop, raw, layer=0, row_list=rl, row_count=cnt, counts=counts),
               _layer_counts(), 0)
