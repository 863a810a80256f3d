"""The sample cull without a GPU: the flag of ``OccupancyGrids`` and what depends on it, the refusals (one
launch per network, training, layer 0, the packed word's ranges) before any launch, the new entries of the C ABI, the workspace
of a render without the flag, and -- on the CPU oracle alone -- the conditions of the oracle-compared GPU cases of
tests/test_gpu_sample_cull.py: how far the fp32 and the fp64 oracle's fine points lie apart, how many rays the face margin
leaves out, and that every case has rays with both listed and skipped samples."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import occupancy_common as OC
import sample_cull_common as SC
import scene_edits_common as S
from instances_common import base_model
from stnerf_amd import hip, occupancy as occ, ops
from test_occupancy_cpu import OnDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------- the flag
def test_the_flag_is_off_by_default_and_in_the_fingerprint():
    a, b = occ.OccupancyGrids(), occ.OccupancyGrids(samples=True)
    assert a.samples is False and b.samples is True
    assert a.fingerprint() != b.fingerprint() and len(a.fingerprint()) == len(b.fingerprint()) == 8
    assert occ.OccupancyGrids(samples=False).fingerprint() == a.fingerprint()
    assert occ.OccupancyGrids(samples=True, auto=False).fingerprint() not in (a.fingerprint(), b.fingerprint(), occ.OccupancyGrids(auto=False).fingerprint())
    with pytest.raises(TypeError):
        occ.OccupancyGrids(samples=1)
    st = b.stats()
    assert st["samples"] == {} and st["pairs"] == {}
    counts = b.sample_counts("cpu")
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (hip.MAX_LAYERS, 2)
    counts[2] = torch.tensor([1 << 40, 7])                          # 64 bits wide
    assert b.stats()["samples"] == {2: (1 << 40, 7)} and not bool(counts.any())
    counts[2] = torch.tensor([5, 1])
    assert b.stats()["samples"] == {2: ((1 << 40) + 5, 8)}
    b.reset_stats()
    assert b.stats()["samples"] == {}


def test_the_cross_rank_fingerprint_of_a_model_sees_the_flag():
    from stnerf_amd.parallel import layers_fingerprint
    model = base_model(2)
    model.set_occupancy(occ.OccupancyGrids())
    off = layers_fingerprint(model)
    model.set_occupancy(occ.OccupancyGrids(samples=True))
    on = layers_fingerprint(model)
    assert len(on) == len(off) and on != off
    model.set_occupancy(None)


def test_the_renderer_takes_the_word_samples():
    import types
    from stnerf_amd.render.layered_neural_renderer import LayeredNeuralRenderer
    model = base_model(2)
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=2, FRAME_NUM=3, FRAME_OFFSET=0), INPUT=types.SimpleNamespace(SIZE_TEST=[23, 17]))
    K, T = S.camera()
    r = LayeredNeuralRenderer(cfg, model=model, gt_poses=T.reshape(1, 4, 4), gt_Ks=[K], occupancy="samples")
    first = r.occupancy
    assert isinstance(first, occ.OccupancyGrids) and first.samples and model._occupancy is first
    r.occupancy = "samples"
    assert r.occupancy is first
    r.occupancy = True                                              # grids are attached: stays as it is
    assert r.occupancy is first
    r.occupancy = False
    r.occupancy = True
    assert r.occupancy.samples is False
    r.occupancy = "samples"
    assert r.occupancy.samples is True
    with pytest.raises(TypeError):
        r.occupancy = "sample"
    model.set_occupancy(None)


# ---------------------------------------------------------------------------------------- refusals
def test_refusals_of_the_render_path():
    model = base_model(2)
    rays = torch.cat([torch.zeros(8, 6), torch.tensor([[1.0, 2.5, 3.0]]).repeat(8, 1)], 1)
    grids = occ.OccupancyGrids(samples=True)
    model.set_occupancy(grids)
    assert "occupancy" in model._inference_only_edits()
    model.train()
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="occupancy"):       # training: as for grids without the flag
        model.render_rays_raw(rays.as_subclass(OnDevice))
    model.eval()
    model.set_precision("fp32")
    model.mlp_schedule = "per_net"
    with pytest.raises(ValueError, match="per_net"):                                       # one launch per network
        model.render_rays_raw(rays.as_subclass(OnDevice))
    model.mlp_schedule = "stage"
    model.set_precision("bf16x3")
    with pytest.raises(ValueError, match="layer 0"):                                        # the background is never listed
        grids.set_manual(0, torch.ones(2, 2, 2, dtype=torch.bool), [0, 0, 0], [1, 1, 1])
    model.set_occupancy(None)


def _grid():
    g = hip.Occupancy()
    g.bits = 0x1000
    for a in range(3):
        g.res[a], g.lo[a], g.inv_cell[a] = 8, 0.0, 4.0
    return g


def test_the_rows_entry_refuses_before_any_launch():
    f = hip.lib().stnerf_occupancy_rows
    fake, g = C.c_void_p(0x1000), _grid()                          # never dereferenced: the checks come before any launch
    call = lambda n=4, layer=1, ns=12, cap=48, grid=g: f(None, None, n, layer, fake, 3 * ns, ns, C.byref(grid), fake, 4 * ns, fake, cap, fake, None, None)
    for kw, what in ((dict(layer=0), "layer 0"), (dict(ns=257, cap=4 * 257), "1..256"), (dict(n=(1 << 23) + 1, ns=1, cap=1 << 24), "2^23"),
                     (dict(cap=47), "capacity")):
        assert call(**kw) == hip.EINVAL and what in hip.last_error(), (kw, what, hip.last_error())
    bad = _grid()
    bad.res[1] = 300
    assert call(grid=bad) == hip.EINVAL and "1..256" in hip.last_error()
    bad = _grid()
    bad.bits = None
    assert call(grid=bad) == hip.EINVAL and "no grid" in hip.last_error()
    with pytest.raises(ValueError, match="grid"):
        ops.occupancy_rows(torch.zeros(4, 12, 3).as_subclass(OnDevice), torch.zeros(4, 12, 4).as_subclass(OnDevice), None)


def _render_args(l, precision, shown=False):
    p, nets = hip.RenderParams(), hip.Nets()
    p.l, p.n1, p.n2, p.ray_stride, p.retiming, p.precision = l, 12, 6, 6 + l, 1, precision
    for i in range(l):
        p.shown[i] = int(shown)
    nets.bkgd = nets.bkgd_fine = 0x1000
    fake = C.c_void_p(0x1000)
    head = (fake, 8, fake, 0, C.byref(nets), C.byref(p), None, None, fake, 1 << 30, fake, fake, fake, fake, fake, None, None, None, None)
    return head, (p, nets)


def test_the_pipeline_entry_refuses_before_any_launch():
    f = hip.lib().stnerf_render_rays_samples
    l = 3
    table = (hip.Occupancy * l)()
    for i in (1, 2):
        table[i] = _grid()
    flags = lambda *v: (C.c_int32 * l)(*v)
    head, keep = _render_args(l, 2)
    assert f(*head, table, None, flags(0, 1, 1), None, None) == hip.EINVAL and "precision 2" in hip.last_error()     # per_net
    head, keep = _render_args(l, 3)
    assert f(*head, table, None, flags(1, 1, 0), None, None) == hip.EINVAL and "layer 0" in hip.last_error()
    table[2].bits = None
    assert f(*head, table, None, flags(0, 1, 1), None, None) == hip.EINVAL and "no occupancy grid" in hip.last_error()
    assert f(*head, None, None, flags(0, 1, 0), None, None) == hip.EINVAL and "no occupancy grid" in hip.last_error()
    small = list(head)
    small[9] = hip.lib().stnerf_render_workspace_bytes(8, l, 12, 6, 0)                     # the workspace of a render without the flag
    assert f(*small, table, None, flags(0, 1, 0), None, None) == hip.EINVAL and "workspace" in hip.last_error()
    head, keep = _render_args(l, 3)
    keep[0].n1, keep[0].n2 = 200, 100                                                       # n1 + n2 > 256: the sample does not fit the word
    assert f(*head, table, None, flags(0, 1, 0), None, None) == hip.EINVAL and "256" in hip.last_error()


def test_a_stage_with_a_row_list_refuses_what_the_word_cannot_hold():
    f = hip.lib().stnerf_mlp_stage_rows
    fake = C.c_void_p(0x1000)
    layers, rows = (hip.StageLayer * 1)(), (hip.StageRows * 1)()
    layers[0].space = layers[0].xyz = layers[0].raw = 0x1000
    rows[0].row_list = rows[0].row_count = 0x1000
    assert f(layers, rows, 1, 4, 257, fake, 3, 0, 3 * 257, 4 * 257, 0, fake, fake, None) == hip.EINVAL and "ns <= 256" in hip.last_error()
    assert f(layers, rows, 1, (1 << 23) + 1, 4, fake, 3, 0, 12, 16, 0, fake, fake, None) == hip.EINVAL and "2^23" in hip.last_error()
    rows[0].row_count = None
    assert f(layers, rows, 1, 4, 12, fake, 3, 0, 36, 48, 0, fake, fake, None) == hip.EINVAL and "row count" in hip.last_error()
    x = torch.zeros(4, 12, 3).as_subclass(OnDevice)
    net = type("Net", (), dict(precision="fp32", use_time=False, blob=x))()
    with pytest.raises(ValueError, match="go together"):
        ops.mlp_stage([dict(space=net, xyz=x, raw=torch.zeros(4, 12, 4).as_subclass(OnDevice), row_list=torch.zeros(4, dtype=torch.int32).as_subclass(OnDevice))],
                      torch.zeros(4, 3).as_subclass(OnDevice), 12)


# ---------------------------------------------------------------------------------------- the ABI, the workspace
def test_entries_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "stnerf.h")).read()
    for name in ("stnerf_occupancy_rows", "stnerf_mlp_stage_rows", "stnerf_render_rays_samples", "stnerf_render_workspace_bytes_samples"):
        assert name in hip.exported_symbols() and getattr(hip.lib(), name) is not None and name + "(" in header
    assert "typedef struct stnerf_stage_rows {" in header and "Sample cull." in header
    assert C.sizeof(hip.StageRows) == 16
    assert ops.PROFILE_KERNELS[9] == "occupancy_rows" and ops.PROFILE_KERNELS[7:9] == ("occupancy_cull", "occupancy_build")
    assert all(callable(getattr(ops, f)) for f in ("occupancy_rows", "mlp_stage", "render_rays"))


@pytest.mark.parametrize("n,l,n1,n2,only_coarse,parent", [(128, 4, 12, 6, False, 637256), (128, 4, 12, 6, True, 465224), (64, 4, 64, 64, False, 1250568)])
def test_the_workspace_grows_only_with_the_flag(n, l, n1, n2, only_coarse, parent):
    """``parent``: stnerf_render_workspace_bytes of the commit before the sample cull, for these shapes."""
    assert hip.lib().stnerf_render_workspace_bytes(n, l, n1, n2, int(only_coarse)) == parent
    assert ops.render_workspace_bytes(n, l, n1, n2, only_coarse) == parent
    assert ops.render_workspace_bytes(n, l, n1, n2, only_coarse, occupancy_samples=[False] * l) == parent
    assert hip.lib().stnerf_render_workspace_bytes_samples(n, l, n1, n2, int(only_coarse), None) == parent
    one = ops.render_workspace_bytes(n, l, n1, n2, only_coarse, occupancy_samples=[False, True, False, False])
    two = ops.render_workspace_bytes(n, l, n1, n2, only_coarse, occupancy_samples=[False, True, False, True])
    rows = n * (n1 if only_coarse else n1 + n2) * 4
    assert one >= parent + rows and two - one == (rows + 255) // 256 * 256
    with pytest.raises(ValueError, match="one entry per layer"):
        ops.render_workspace_bytes(n, l, n1, n2, only_coarse, occupancy_samples=[True])


# ---------------------------------------------------------------------------------------- the rule's helpers
def test_row_order_check_and_face_distance():
    w = lambda r, k: (r << 8) | k
    assert SC.rows_are_contiguous_and_ascending([w(5, 0), w(5, 3), w(2, 1), w(9, 0), w(9, 255)])
    assert SC.rows_are_contiguous_and_ascending([])
    assert not SC.rows_are_contiguous_and_ascending([w(5, 3), w(5, 0)])                     # descending
    assert not SC.rows_are_contiguous_and_ascending([w(5, 0), w(2, 1), w(5, 3)])            # a ray in two runs
    assert not SC.rows_are_contiguous_and_ascending([w(5, 0), w(5, 0)])                     # a row twice
    lo, hi = np.array([-1.0, 0.0, 0.0], np.float32), np.array([1.0, 4.0, 1.0], np.float32)
    d = SC.interior_face_distance(np.array([[0.1, 0.5, 0.5], [-1.0, 3.9, 0.0], [5.0, 2.0, 9.0]]), lo, hi, (2, 4, 1))
    assert np.allclose(d, [0.1, 0.9, 0.0])                          # x = 0 and y = 1, 2, 3 are the interior faces; z has none
    grid = SC.grid_entry(OC.half_y(8), lo, hi)
    x = np.zeros((3, 4, 3), np.float32)
    x[..., 1] = np.array([0.5, 1.9, 2.0, np.nan], np.float32)       # y cells 1, 3, 4; NaN
    rows, listed = SC.np_rows(x, [2, 0], grid)
    assert listed.tolist() == [[True, True, False, True], [False] * 4, [True, True, False, True]]
    assert rows.tolist() == [w(0, 0), w(0, 1), w(0, 3), w(2, 0), w(2, 1), w(2, 3)]


# ---------------------------------------------------------------------------------------- the oracle cases' conditions
def _cases():
    plain = OC.plain_case()
    c64 = OC.plain_case(n1=64, n2=64)
    full = S.make_case()
    return {"plain half_x 0": (plain, OC.manual_grids(plain, "half_x", 0), None),
            "plain ball 1": (plain, OC.manual_grids(plain, "ball", 1), None),
            "full edits": (full, OC.manual_grids(full, "half_x", 0), None),
            "64+64": (c64, SC.grids_64(c64), 64),
            "only_coarse": (OC.plain_case(only_coarse=True, near=4.0), None, None)}


@pytest.mark.parametrize("name", ["plain half_x 0", "plain ball 1", "full edits", "64+64", "only_coarse"])
def test_conditions_of_the_oracle_compared_cases(monkeypatch, name):
    """Measured here (CPU oracle, grids at res 8): the largest distance between the fp32 and the fp64 oracle's undeformed fine points
    of a gridded layer, eps = 4 x that, and the rays left out of the GPU comparison because a gridded layer's fine point lies within
    eps of an interior cell face -- at most 5 % of the rays, asserted here before anything runs on a GPU.  The figures are printed
    (`-s`).  Measured: plain half_x 2.3e-5 apart, eps 9.3e-5, 9 of 391 rays left out; plain ball (dilate 1) 5.1e-5, 2.0e-4, 17 of 391;
    full edits 5.5e-5, 2.2e-4, 15 of 391; 64 + 64 on the first 64 rays 2.4e-5, 9.4e-5, 1 of 64.  (The distance is no rounding figure:
    the inverse-CDF resampler is ill-conditioned where a bin's weight is tiny, and the largest gap is such a sample.)  The grids are
    `half_x` and `ball` at res 8 -- `half`, split in y, keeps or drops this view's rays whole, so the sample cull never bites on it
    -- and for 64 + 64 a 4 x 1 x 4 board (``sample_cull_common.grids_64``), since res 8 breaks the 5 % there (7 of 64).
    Every case has at least 8 rays with both listed and skipped samples on a gridded layer, in every stage it runs."""
    case, grids, first = _cases()[name]
    if grids is None:
        grids = OC.manual_grids(case, "half_x", 0)
    rays = S.case_rays(case)
    rays = rays if first is None else rays[:first]
    n = rays.shape[0]
    ref32, ch32 = SC.oracle_render_sampled(case, grids, grids, rays, torch.float32, monkeypatch)
    counts = SC.assert_sample_cull_bites(ch32, case, n, name)
    # the sample cull changes the picture: some performer output differs from the ray-culled oracle's
    monkeypatch.setattr(SC.O, "sample_coarse", OC.culled_sampler(case, grids))
    ray_culled = S.oracle_render(case, rays)
    monkeypatch.undo()
    assert any(not torch.equal(ref32[k], ray_culled[k]) for k in ref32 if k.startswith("coarse_layer") and k != "coarse_layer0")
    assert all(torch.equal(ref32[k], ray_culled[k]) for k in ref32 if k.startswith("mask")) and torch.equal(ref32["t_coarse"], ray_culled["t_coarse"])
    assert torch.equal(ref32["coarse_layer0"], ray_culled["coarse_layer0"])                  # the background is never listed
    if case["only_coarse"]:
        print(f"{name}: rays with listed and skipped samples per layer {counts}")
        return
    ref64, ch64 = SC.oracle_render_sampled(case, grids, grids, rays, torch.float64, monkeypatch)
    gap, eps, excluded = SC.fine_point_gap_and_excluded(case, ch32, ch64, n)
    print(f"{name}: fp32 / fp64 fine points at most {gap:.3e} apart, eps {eps:.3e}, {int(excluded.sum())} of {n} rays left out; "
          f"rays with listed and skipped samples per layer {counts}")
    assert 0.0 < gap < 1e-4 and excluded.mean() <= 0.05, (name, gap, int(excluded.sum()), n)
