"""Grid proposals (stnerf_amd.ProposalGrids) without a GPU: the host logic of the grids -- argument checks, the
keying, LRU eviction, manual grids --, the model's refusals, the properties of the numpy restatement of the lookup
(tests/proposal_common.py: what tests/test_gpu_proposal.py holds the kernel to, bit for bit), and the C entry's checks before any
launch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import proposal_common as PC
import scene_edits_common as S
from instances_common import base_model
from stnerf_amd import hip, occupancy as occ, ops, proposal as prop
from test_occupancy_cpu import OnDevice

F = np.float32


# ---------------------------------------------------------------------------------------- the grids' host logic
def fake_builds(monkeypatch, model, calls):
    def density_grid(layer_id, frame_id, res=64, fine=True, direction=(0.0, 0.0, 1.0), retiming=True):
        calls.append((layer_id, float(frame_id), bool(fine)))
        rx, ry, rz = occ.normalise_res(res)
        lo, hi = occ.box_bounds(model.bkgd_bbox if layer_id == 0 else model.layer_box_at(layer_id, frame_id, retiming))
        return torch.zeros(rz + 1, ry + 1, rx + 1), lo, hi
    monkeypatch.setattr(model, "density_grid", density_grid, raising=False)


def test_constructor_checks_and_defaults():
    g = prop.ProposalGrids()
    assert (g.res, g.layers, g.background, g.background_res, g.max_grids) == ((128, 128, 128), None, False, None, 16)
    assert prop.ProposalGrids(res=(4, 5, 6), layers=[2, 1, 2], background=True, background_res=32).layers == [1, 2]
    for bad in (dict(res=0), dict(res=257), dict(res=(4, 4)), dict(max_grids=0), dict(max_grids=1.5), dict(layers=[0]), dict(layers=[1.0]),
                dict(layers=[True]), dict(background_res=0)):
        with pytest.raises(ValueError):
            prop.ProposalGrids(**bad)
    with pytest.raises(TypeError):
        prop.ProposalGrids(background=1)
    import stnerf_amd
    assert stnerf_amd.ProposalGrids is prop.ProposalGrids


def test_grid_keys_rebuild_on_a_parameter_version_bump_and_lru(monkeypatch):
    model = base_model(2)
    model.add_instance(1)
    calls = []
    fake_builds(monkeypatch, model, calls)
    grids = prop.ProposalGrids(res=(5, 7, 9), max_grids=3)
    g = grids.grid(model, 1, 2.5, "cpu")
    assert g.res == (5, 7, 9) and tuple(g.sigma.shape) == (10, 8, 6) and calls == [(1, 2.5, True)]      # the FINE network, once
    assert np.array_equal(g.inv_cell, (np.asarray(g.res, F) / (g.hi - g.lo)).astype(F))
    assert g.entry()[0] is g.sigma and g.entry()[1] == g.lo.tolist() and g.nbytes() == 4 * 10 * 8 * 6
    assert grids.grid(model, 1, 2.5, "cpu") is g and (grids.built, grids.reused) == (1, 1)
    assert grids.grid(model, 3, 2.5, "cpu") is g            # the instance of performer 1 at the same id: the source's grid
    assert grids.grid(model, 3, 1.5, "cpu") is not g        # ... at its own id: another one
    assert grids.grid(model, 2, 2.5, "cpu") is not g and len(grids) == 3 and grids.built == 3
    k = grids.key(model, 1, 2.5, g.lo, g.hi)
    with torch.no_grad():
        model.spacenets[0].stage1[0].weight.add_(0.0)       # the COARSE SpaceNet is no input of the grid
    assert grids.key(model, 1, 2.5, g.lo, g.hi) == k
    with torch.no_grad():
        model.spacenets_fine[0].stage1[0].weight.add_(0.0)  # the fine one is: its version counter moves
    assert grids.key(model, 1, 2.5, g.lo, g.hi) != k
    assert grids.grid(model, 1, 2.5, "cpu") is not g and grids.built == 4 and len(grids) == 3      # rebuilt; the oldest left
    k = grids.key(model, 1, 2.5, g.lo, g.hi)
    with torch.no_grad():
        model.time_deform_nets[0].motion_net[0].weight.add_(0.0)
    assert grids.key(model, 1, 2.5, g.lo, g.hi) != k
    k2 = grids.key(model, 2, 2.5, g.lo, g.hi)
    model.use_space_time, flag = False, model.use_space_time
    assert grids.key(model, 2, 2.5, g.lo, g.hi) != k2
    model.use_space_time = flag
    assert prop.ProposalGrids(res=(5, 7, 8)).key(model, 2, 2.5, g.lo, g.hi) != k2
    assert grids.key(model, 2, 2.5, g.lo + 1, g.hi) != k2 and grids.key(model, 2, 1.5, g.lo, g.hi) != k2
    # least recently used first out
    grids.clear()
    a = grids.grid(model, 1, 1.0, "cpu")
    b = grids.grid(model, 1, 2.0, "cpu")
    c = grids.grid(model, 1, 3.0, "cpu")
    assert grids.grid(model, 1, 1.0, "cpu") is a            # touched: b is now the oldest
    d = grids.grid(model, 2, 1.0, "cpu")
    assert len(grids) == 3 and grids.grid(model, 1, 3.0, "cpu") is c and grids.grid(model, 1, 1.0, "cpu") is a and grids.grid(model, 2, 1.0, "cpu") is d
    before = grids.built
    assert grids.grid(model, 1, 2.0, "cpu") is not b and grids.built == before + 1
    st = grids.stats()
    assert st["built"] == grids.built and st["reused"] == grids.reused and st["grids"] == 3 and st["bytes"] == 3 * 4 * 10 * 8 * 6
    grids.reset_stats()
    assert grids.stats()["built"] == 0


def test_the_background_grid_and_the_flagged_layers(monkeypatch):
    model = base_model(2)
    calls = []
    fake_builds(monkeypatch, model, calls)
    grids = prop.ProposalGrids(res=4)
    assert grids.flagged_layers(model) == [1, 2] and not grids.has_background()
    model.hide_layer(2)
    assert grids.flagged_layers(model) == [1]
    model.show_layer(2)
    assert prop.ProposalGrids(res=4, layers=[2]).flagged_layers(model) == [2]
    with pytest.raises(ValueError, match="does not have"):
        prop.ProposalGrids(res=4, layers=[3]).flagged_layers(model)
    bg = prop.ProposalGrids(res=4, layers=[], background=True, background_res=(2, 3, 4))
    assert bg.flagged_layers(model) == [0] and bg.has_background()
    table, held = bg.table(model, [1.0, 2.5, 3.0], "cpu")
    assert table[1] is None and table[2] is None and calls == [(0, 1.0, True)]
    assert held[0].res == (2, 3, 4) and tuple(table[0][0].shape) == (5, 4, 3)
    lo, hi = occ.box_bounds(model.bkgd_bbox)
    assert np.array_equal(held[0].lo, lo) and np.array_equal(held[0].hi, hi)
    # the background's frame id is in its key only where the flags make it an input of the density
    timed = prop.ProposalGrids.background_timed(model)
    assert (bg.key(model, 0, 1.0, lo, hi) != bg.key(model, 0, 2.0, lo, hi)) == timed
    both = prop.ProposalGrids(res=4, background=True)
    table, held = both.table(model, [1.0, 2.5, 3.0], "cpu")
    assert all(e is not None for e in table) and [g.res for g in held] == [(4, 4, 4)] * 3


def test_set_manual_shapes():
    grids = prop.ProposalGrids(res=4, layers=[])
    ok = torch.rand(3, 4, 5)
    for bad_layer in (-1, 1.5, True):
        with pytest.raises(ValueError, match="not a layer"):
            grids.set_manual(bad_layer, ok, [0, 0, 0], [1, 1, 1])
    with pytest.raises(ValueError, match="float tensor"):
        grids.set_manual(1, ok > 0.5, [0, 0, 0], [1, 1, 1])
    with pytest.raises(ValueError, match="float tensor"):
        grids.set_manual(1, ok[0], [0, 0, 0], [1, 1, 1])
    with pytest.raises(ValueError, match="float tensor"):
        grids.set_manual(1, torch.rand(1, 4, 5), [0, 0, 0], [1, 1, 1])          # no cell along z
    with pytest.raises(ValueError, match="1..256"):
        grids.set_manual(1, torch.rand(2, 2, 258), [0, 0, 0], [1, 1, 1])
    with pytest.raises(ValueError, match="bounds"):
        grids.set_manual(1, ok)
    with pytest.raises(ValueError, match="lo < hi"):
        grids.set_manual(1, ok, [0, 0, 0], [1, 0, 1])
    grids.set_manual(1, ok.double(), [0, 0, 0], [1, 2, 4])
    assert grids.manual_layers() == [1] and grids._manual[1][1] == (4, 3, 2)
    model = base_model(2)
    assert grids.flagged_layers(model) == [1]                # a manual grid flags its layer
    g = grids.grid(model, 1, 2.5, "cpu")
    assert g.sigma.dtype == torch.float32 and torch.equal(g.sigma, ok) and g.inv_cell.tolist() == [4.0, 1.5, 0.5]
    assert grids.grid(model, 1, 1.0, "cpu") is g             # at every frame id
    grids.set_manual(0, ok, [0, 0, 0], [1, 1, 1])
    assert grids.has_background() and grids.flagged_layers(model) == [0, 1]
    ident = grids.identity()
    grids.set_manual(0, ok + 1, [0, 0, 0], [1, 1, 1])
    assert grids.identity() != ident
    grids.set_manual(0, None)
    grids.set_manual(1, None)
    assert grids.manual_layers() == [] and grids.flagged_layers(model) == []
    with pytest.raises(ValueError, match="one entry per layer"):
        ops._density_grid_table([None, None], 3)
    assert ops._density_grid_table([None, None, None], 3) is None and ops._density_grid_table(None, 3) is None
    with pytest.raises(ValueError, match="sigma must be"):
        ops._density_grid_table([(torch.zeros(2, 2), [0] * 3, [1] * 3)], 1)


# ---------------------------------------------------------------------------------------- the model's refusals
def test_refusals_of_the_render_path(monkeypatch):
    from stnerf_amd import parallel
    from stnerf_amd.bkgd_cache import BackgroundCache
    from stnerf_amd.layer_cache import LayerCache
    model = base_model(2)
    rays = torch.cat([torch.zeros(8, 6), torch.tensor([[1.0, 2.5, 3.0]]).repeat(8, 1)], 1)
    dev = rays.as_subclass(OnDevice)
    assert model.proposal is None and model._inference_only_edits() is None
    grids = prop.ProposalGrids(res=4, background=True)
    assert model.set_proposal(grids) is model and model.proposal is grids
    assert "proposal" in model._inference_only_edits()
    model.train()
    with torch.enable_grad(), pytest.raises(RuntimeError, match="grid proposals"):       # training mode
        model.render_rays_raw(dev)
    model.eval()
    with pytest.raises(ValueError, match="background cache"):
        model.set_background_cache(BackgroundCache())
        model.render_rays_raw(dev)
    model.set_background_cache(None)
    with pytest.raises(ValueError, match="layer cache"):
        model.set_layer_cache(LayerCache())
        model.render_rays_raw(dev)
    model.set_layer_cache(None)
    with pytest.raises(ValueError, match="background occupancy grid"):
        model.set_occupancy(occ.OccupancyGrids(background=True))
        model.render_rays_raw(dev)
    model.set_occupancy(None)
    with pytest.raises(ValueError, match="per-ray background mask"):
        model.render_rays_raw(dev, background_rays=torch.ones(8, dtype=torch.uint8))
    model.mlp_schedule, model_schedule = "per_net", model.mlp_schedule
    model.set_precision("fp32")
    with pytest.raises(ValueError, match="per_net"):
        model.render_rays_raw(dev)
    model.mlp_schedule = model_schedule
    monkeypatch.setattr(parallel, "active_group", lambda m=None: (0, 2, None))            # more than one rank
    with pytest.raises(RuntimeError, match="more than one rank"):
        model.render_rays_raw(dev)
    monkeypatch.undo()
    # the caches are refused only on the layers they would hold
    perf = prop.ProposalGrids(res=4)
    model.set_proposal(perf)
    model.set_background_cache(BackgroundCache())
    model._check_proposal(perf.flagged_layers(model), None)
    model.set_background_cache(None)
    # one frame id per flagged layer and chunk group
    flagged = grids.flagged_layers(model)
    assert flagged == [0, 1, 2]
    model.set_proposal(grids)
    assert model._proposal_frame_ids(rays, [(0, 8)], True, flagged) == [[1.0, 2.5, 3.0]]
    mixed = rays.clone()
    mixed[5, 8] = 2.0
    with pytest.raises(ValueError, match="proposal: layer 2"):
        model._proposal_frame_ids(mixed, [(0, 8)], True, flagged)
    assert model._proposal_frame_ids(mixed, [(0, 8)], True, [0, 1])[0][:2] == [1.0, 2.5]              # layer 2 is not flagged: its ids may differ
    assert len(model._proposal_frame_ids(mixed, [(0, 5), (5, 6), (6, 8)], True, flagged)) == 3
    bg_mixed = rays.clone()
    bg_mixed[:, 6] = torch.arange(8.0)
    if prop.ProposalGrids.background_timed(model):
        with pytest.raises(ValueError, match="proposal: layer 0"):
            model._proposal_frame_ids(bg_mixed, [(0, 8)], True, flagged)
    else:
        assert len(model._proposal_frame_ids(bg_mixed, [(0, 8)], True, flagged)) == 1
    wide7 = torch.cat([torch.zeros(8, 6), torch.full((8, 1), 2.0)], 1)
    assert model._proposal_frame_ids(wide7, [(0, 8)], False, [1, 2]) == [[2.0, 2.0, 2.0]]
    wide7[3, 6] = 1.0
    with pytest.raises(ValueError, match="proposal: layer 1"):
        model._proposal_frame_ids(wide7, [(0, 8)], False, [1, 2])
    model.set_proposal(None)
    assert model._inference_only_edits() is None


def test_renderer_property_attaches_and_detaches():
    import types
    from stnerf_amd.render.layered_neural_renderer import LayeredNeuralRenderer
    model = base_model(2)
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=2, FRAME_NUM=3, FRAME_OFFSET=0), INPUT=types.SimpleNamespace(SIZE_TEST=[23, 17]))
    K, T = S.camera()
    mk = lambda **kw: LayeredNeuralRenderer(cfg, model=model, gt_poses=T.reshape(1, 4, 4), gt_Ks=[K], **kw)
    r = mk()
    assert r.proposal is None and model.proposal is None
    r.proposal = True
    first = r.proposal
    assert isinstance(first, prop.ProposalGrids) and model.proposal is first
    r.proposal = True
    assert r.proposal is first
    mine = prop.ProposalGrids(res=32)
    r.proposal = mine
    assert model.proposal is mine
    r.proposal = False
    assert model.proposal is None
    assert mk(proposal=mine).proposal is mine
    model.set_proposal(None)
    with pytest.raises(TypeError):
        r.proposal = "yes"


# ---------------------------------------------------------------------------------------- the restatement's own properties
def unit_grid(sigma):
    """A grid over [0, R] per axis with unit cells: g = p exactly."""
    rz, ry, rx = (s - 1 for s in sigma.shape)
    return np.zeros(3, F), np.ones(3, F)


def test_restatement_returns_the_vertex_values_exactly_at_f_0_and_f_1():
    g = np.random.default_rng(3)
    sigma = (g.random((4, 5, 6)) * 1e3).astype(F)
    lo, inv = unit_grid(sigma)
    z, y, x = np.meshgrid(np.arange(4), np.arange(5), np.arange(6), indexing="ij")
    pts = np.stack([x, y, z], -1).astype(F)                                  # every vertex: f = 0, and f = 1 at the last of an axis
    got = PC.np_lookup(pts, sigma, lo, inv)
    assert np.array_equal(got.view(np.uint32), sigma.view(np.uint32))
    ix, fx, ux = PC.np_axis(np.array([0, 2, 5], F), 0.0, 1.0, 5)
    assert ix.tolist() == [0, 2, 4] and fx.tolist() == [0.0, 0.0, 1.0] and ux.tolist() == [1.0, 1.0, 0.0]
    # the other form of a lerp does not: v0 + 1 * (v1 - v0) rounds twice
    v0, v1 = (g.random(1000) * 1e3).astype(F), g.random(1000).astype(F)
    assert np.array_equal(PC.np_lerp(v0, F(0), v1, F(1)), v1) and np.array_equal(PC.np_lerp(v0, F(1), v1, F(0)), v0)
    assert (v0 + F(1) * (v1 - v0) != v1).any()
    # the fp64 interpolation agrees at the vertices too
    assert np.array_equal(PC.exact_lookup(pts, sigma, lo, inv), sigma.astype(np.float64))


def test_restatement_clamps_to_the_faces():
    sigma, lo, hi, inv = PC.grid_of((5, 3, 2), 1, infs=False)
    inside = np.array([[0.3, 0.9, 2.1]], F)
    for a in range(3):
        for far, face in ((F(-1e30), lo[a]), (F(1e30), hi[a]), (F(-np.inf), lo[a]), (F(np.inf), hi[a]),
                          (np.nextafter(lo[a], F(-np.inf)), lo[a])):
            p, q = inside.copy(), inside.copy()
            p[0, a], q[0, a] = far, face
            assert PC.same_sigma(PC.np_lookup(p, sigma, lo, inv), PC.np_lookup(q, sigma, lo, inv)), (a, far)
    # the far corner outside on every axis is the last vertex, the near one the first
    assert PC.np_lookup(np.full((1, 3), np.inf, F), sigma, lo, inv)[0] == sigma[-1, -1, -1]
    assert PC.np_lookup(np.full((1, 3), -np.inf, F), sigma, lo, inv)[0] == sigma[0, 0, 0]
    i, f, u = PC.np_axis(np.array([-np.inf, np.inf, -5.0, 1e9], F), lo[0], inv[0], 5)
    assert i.tolist() == [0, 4, 0, 4] and f.tolist() == [0.0, 1.0, 0.0, 1.0]


def test_restatement_propagates_a_nan_coordinate_and_only_that():
    sigma, lo, hi, inv = PC.grid_of((5, 3, 2), 2, infs=False)
    pts = np.tile(((lo + hi) / 2).astype(F), (4, 1))
    for a in range(3):
        pts[a, a] = np.nan
    got = PC.np_lookup(pts, sigma, lo, inv)
    assert np.isnan(got[:3]).all() and np.isfinite(got[3])
    raw = PC.np_proposal_raw(pts, sigma, lo, inv)
    assert raw.shape == (4, 4) and not raw[:, :3].any() and PC.same_sigma(raw[:, 3], got)
    assert PC.same_sigma(np.array([np.nan], F), np.array([-np.nan], F)) and not PC.same_sigma(np.array([0.0], F), np.array([-0.0], F))


def test_restatement_is_monotone_along_an_axis_between_two_vertices():
    """With the other two coordinates on vertices the lookup along an axis is (v0 u) + (v1 f) with u = 1 - f: both products are
    monotone in f under round-to-nearest and so is their sum."""
    g = np.random.default_rng(5)
    sigma = (g.random((3, 3, 3)) * 10).astype(F)
    lo, inv = unit_grid(sigma)
    steps = np.linspace(0, 1, 4097).astype(F)
    for a in range(3):
        for cell in (0, 1):
            pts = np.ones((steps.size, 3), F)
            pts[:, a] = F(cell) + steps
            s = PC.np_lookup(pts, sigma, lo, inv)
            idx = [1, 1, 1]
            idx[2 - a] = cell
            v0 = sigma[tuple(idx)]
            idx[2 - a] = cell + 1
            v1 = sigma[tuple(idx)]
            assert s[0] == v0 and s[-1] == v1
            d = np.diff(s.astype(np.float64))
            assert (d >= 0).all() if v1 >= v0 else (d <= 0).all(), (a, cell)
    # against fp64 on random interior points: a few roundings of the largest vertex value
    sigma, lo, hi, inv = PC.grid_of((16, 16, 16), 6, infs=False)
    pts, _ = PC.points_of(20, 50, lo, hi, 7)
    ok = np.isfinite(pts).all(-1) & (np.abs(pts) < 1e3).all(-1)
    err = np.abs(PC.np_lookup(pts, sigma, lo, inv)[ok] - PC.exact_lookup(pts[ok].astype(np.float64), sigma, lo, inv))
    grad = sum(np.abs(np.diff(sigma.astype(np.float64), axis=2 - a)).max() * float(inv[a]) * 4 * np.spacing(np.maximum(np.abs(pts[ok][:, a]), abs(lo[a])))
               for a in range(3))
    assert (err <= grad + 8 * PC.U * sigma.max()).all()


# ---------------------------------------------------------------------------------------- the C ABI's checks before any launch
def _grid(res=(4, 4, 4)):
    g = hip.DensityGrid()
    g.sigma = 0x1000
    for a in range(3):
        g.res[a], g.lo[a], g.inv_cell[a] = res[a], 0.0, 4.0
    return g


def _call(lib, g, ray_list=None, ray_count=None, n=4, layer=1, xyz=0x1000, ns=8, raw=0x1000, raw_stride=32):
    p = lambda v: None if v is None else C.c_void_p(v)      # never dereferenced: the checks come before any launch
    return lib.stnerf_proposal_density(p(ray_list), p(ray_count), n, layer, p(xyz), 24, ns, None if g is None else C.byref(g), p(raw), raw_stride, None)


@pytest.mark.parametrize("what,kw,spoil", [
    ("null pointer", dict(xyz=None), None), ("null pointer", dict(raw=None), None), ("null pointer", dict(), "no grid"),
    ("needs its count", dict(ray_list=0x1000), None),
    ("no sigma", dict(), lambda g: setattr(g, "sigma", None)),
    ("4-byte aligned", dict(), lambda g: setattr(g, "sigma", 0x1002)),
    ("4-byte aligned", dict(xyz=0x1001), None), ("4-byte aligned", dict(ray_list=0x1002, ray_count=0x1000), None),
    ("16-byte aligned", dict(raw=0x1008), None), ("multiple of 4", dict(raw_stride=30), None),
    ("each must be >= 1", dict(), lambda g: g.res.__setitem__(1, 0)),
    ("2^31 vertices", dict(), lambda g: [g.res.__setitem__(a, 1290) for a in range(3)]),
    ("2^31 vertices", dict(), lambda g: [g.res.__setitem__(a, 2 ** 31 - 1) for a in range(3)]),
    ("not finite", dict(), lambda g: g.lo.__setitem__(0, float("inf"))),
    ("not finite", dict(), lambda g: g.inv_cell.__setitem__(2, float("nan"))),
    ("ns = 0", dict(ns=0), None), ("ns = 257", dict(ns=257), None),
    ("layer -1", dict(layer=-1), None), ("layer 16", dict(layer=16), None), ("bad shape", dict(n=-1), None)])
def test_entry_refuses_bad_arguments_before_any_launch(what, kw, spoil):
    lib = hip.lib()
    g = _grid()
    if callable(spoil):
        spoil(g)
    assert _call(lib, None if spoil == "no grid" else g, **kw) == hip.EINVAL
    assert what in hip.last_error(), hip.last_error()


def test_entry_accepts_the_edge_values_with_no_ray():
    lib = hip.lib()
    assert _call(lib, _grid((1289, 1289, 1289)), n=0, ns=256, layer=15) == hip.OK          # 1290^3 < 2^31 vertices, n = 0: no launch
    assert _call(lib, _grid((1, 1, 1)), n=0, ns=1, layer=0, ray_list=0x1000, ray_count=0x1000) == hip.OK


def test_entries_are_exported_declared_and_laid_out_as_the_header_says(tmp_path):
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stnerf.h")).read()
    assert "stnerf_proposal_density" in hip.exported_symbols() and "stnerf_proposal_density(" in header
    assert "typedef struct stnerf_density_grid {" in header and "} stnerf_render_options_proposal;" in header
    assert ops.PROFILE_KERNELS[20] == "proposal_density" and ops.PROFILE_KERNELS[19] == "deep_composite"
    assert C.sizeof(hip.DensityGrid) == 48
    assert C.sizeof(hip.RenderOptionsProposal) == C.sizeof(hip.RenderOptionsDeep) + 8
    assert hip.RenderOptionsProposal().struct_size == C.sizeof(hip.RenderOptionsProposal)
    # the size query takes the three record sizes and no other; the proposal record asks for no workspace of its own
    lib = hip.lib()
    sizes = [lib.stnerf_render_workspace_bytes_opts(100, 3, 12, 6, 0, o) for o in (C.byref(hip.RenderOptions()), hip.RenderOptionsDeep().ref(),
                                                                                   hip.RenderOptionsProposal().ref())]
    assert sizes[0] == sizes[1] == sizes[2] == lib.stnerf_render_workspace_bytes(100, 3, 12, 6, 0) > 0
    table = (hip.DensityGrid * 3)()
    table[1] = _grid()
    opts = hip.RenderOptionsProposal()
    opts.proposal = table
    assert lib.stnerf_render_workspace_bytes_opts(100, 3, 12, 6, 0, opts.ref()) == sizes[0]
    bad = hip.RenderOptionsProposal()
    bad.struct_size += 8
    assert lib.stnerf_render_workspace_bytes_opts(100, 3, 12, 6, 0, bad.ref()) == hip.EINVAL and "struct_size" in hip.last_error()
    gcc = shutil.which("gcc")
    if gcc is None:
        return
    pairs = {"stnerf_density_grid": hip.DensityGrid, "stnerf_render_options_proposal": hip.RenderOptionsProposal}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stnerf.h"', 'int main(void){']
    for cname, cls in pairs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
    lines += ['printf("proposal %zu\\n", offsetof(stnerf_render_options_proposal, proposal));',
              'printf("sigma %zu\\n", offsetof(stnerf_density_grid, sigma));', 'printf("res %zu\\n", offsetof(stnerf_density_grid, res));',
              'printf("lo %zu\\n", offsetof(stnerf_density_grid, lo));', 'printf("inv_cell %zu\\n", offsetof(stnerf_density_grid, inv_cell));',
              'return 0;}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call([gcc, "-I" + os.path.join(root, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["stnerf_density_grid"]) == C.sizeof(hip.DensityGrid)
    assert int(got["stnerf_render_options_proposal"]) == C.sizeof(hip.RenderOptionsProposal)
    assert int(got["proposal"]) == hip.RenderOptionsProposal.proposal.offset
    for f in ("sigma", "res", "lo", "inv_cell"):
        assert int(got[f]) == getattr(hip.DensityGrid, f).offset
