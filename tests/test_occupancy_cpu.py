"""Occupancy grids without a GPU: the numpy restatements of the rules against the package's host helpers, the oracle's
expectation of a culled render and the condition on its inputs (every culled layer keeps and loses at least 8 of its hit
pairs), what ``assert_matches_oracle`` would refuse, and the host logic -- grid keys and LRU, manual-grid checks, the refusals
(layer 0, the op-by-op path, point replays, mixed frame ids) and the C ABI's checks before any launch.

Kept / culled pairs among the hit rays of the base scene without edits (391 rays, 12 + 6, one 8^3 grid per performer), as this
file measures them with the grids of ``occupancy_common`` (layers 1, 2 and the instance 3):
    half, dilate 0:  72 / 72,  74 / 74,  64 / 64          half, dilate 1:  90 / 54,  94 / 54,  80 / 48
    ball, dilate 0:  22 / 122, 24 / 124, 18 / 110         ball, dilate 1:  61 / 83,  69 / 79,  60 / 68
and with rays 7 wide (frame 2):  half 0: 64 / 64, 68 / 68, 64 / 64;  half 1: 80 / 48, 86 / 50, 80 / 48;  ball 0: 21 / 107, 27 / 109,
22 / 106.  The first 64 rays at 64 + 64 with the half-in-x grid on layers 1 and 3 (layer 2 has 5 hit pairs there): 10 / 8, 8 / 8.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import occupancy_common as OC
import scene_edits_common as S
from instances_common import base_model
from oracle import stnerf_oracle as O
from stnerf_amd import hip, occupancy as occ, ops


# ---------------------------------------------------------------------------------------- the rules
def test_package_host_helpers_agree_with_the_numpy_restatements():
    rs = np.random.RandomState(0)
    for shape in ((9, 7, 5), (3, 4, 33), (1, 1, 1), (2, 2, 8)):
        grid = rs.rand(*shape) < 0.3
        words = OC.np_pack(grid)
        assert words.dtype == np.uint32 and words.size == (grid.size + 31) // 32
        assert np.array_equal(occ.pack_bits(grid), words)
        res = (shape[2], shape[1], shape[0])
        assert np.array_equal(OC.np_unpack(words, res), grid)
        used = grid.size & 31
        if used:
            assert int(words[-1]) >> used == 0
    lo, hi = np.array([-1.2, -1.0, 0.3], np.float32), np.array([0.37, 1.0, 2.9], np.float32)
    res = (5, 7, 9)
    assert np.array_equal(occ.inv_cell(res, lo, hi), OC.np_inv_cell(res, lo, hi))
    for axis, (a, b) in enumerate(zip(occ.vertex_coordinates(res, lo, hi), OC.np_vertices(res, lo, hi))):
        assert a.dtype == np.float32 and a.shape == (res[axis] + 1,) and np.array_equal(a, b) and a[0] == lo[axis] and a[-1] == hi[axis]
    blo, bhi = occ.box_bounds(S._state(2)[2][1, 0])
    assert np.array_equal(blo, OC.np_bounds(S._state(2)[2][1, 0])[0]) and np.array_equal(bhi, OC.np_bounds(S._state(2)[2][1, 0])[1])


def test_build_rule_threshold_nan_and_dilation():
    thr = np.float32(0.25)
    sig = np.full((3, 3, 5), -1.0, np.float32)
    sig[0, 0, 0] = thr                                   # exactly at the threshold: not dense
    sig[2, 2, 4] = np.nextafter(thr, np.float32(1))      # just above: dense
    sig[0, 2, 2] = np.nextafter(thr, np.float32(-1))     # just below: not dense
    got = OC.np_build(sig, None, thr, 0)
    assert got.shape == (2, 2, 4) and got.sum() == 1 and got[1, 1, 3]
    sig[1, 1, 0] = np.nan                                # a NaN is dense: the 8 cells... here the 4 cells around vertex (1,1,0)
    got = OC.np_build(None, sig, thr, 0)
    assert got.sum() == 5 and got[:, :, 0].all()
    both = OC.np_build(sig, np.full_like(sig, 1.0), thr, 0)
    assert both.all()
    one = np.zeros((5, 5, 5), bool)
    one[2, 2, 2] = True
    assert OC.np_dilate(one, 1).sum() == 27 and OC.np_dilate(one, 2).all()
    corner = np.zeros((5, 5, 5), bool)
    corner[0, 0, 4] = True
    assert OC.np_dilate(corner, 1).sum() == 8


def test_point_to_cell_clamps_and_nan():
    lo, hi, res = np.array([0.0, 0.0, 0.0], np.float32), np.array([4.0, 2.0, 1.0], np.float32), (4, 2, 1)
    inv = OC.np_inv_cell(res, lo, hi)
    grid = np.zeros((1, 2, 4), bool)
    grid[0, 1, 3] = True
    pts = np.array([[3.5, 1.5, 0.5], [4.0, 2.0, 1.0], [1e30, 1e30, -5.0], [3.0, 1.0, 0.0], [2.9999, 1.5, 0.5], [-1.0, -1.0, -1.0],
                    [np.nan, 0.0, 0.0], [np.inf, np.inf, np.inf]], np.float32)
    assert OC.np_points_occupied(pts, grid, lo, inv).tolist() == [True, True, True, True, False, False, True, True]
    assert OC.np_keep(pts[None, 4:6], grid, lo, inv).tolist() == [False]
    mask = np.array([[1, 1], [3, 1], [2, 1], [0, 1]], np.uint8)
    xyz = np.broadcast_to(pts[4], (4, 2, 3, 3)).copy()
    out, counts = OC.np_cull(xyz, mask, [None, (grid, lo, inv)])
    assert out.tolist() == [[1, 0], [3, 0], [2, 0], [0, 0]] and counts.tolist() == [[0, 0], [4, 4]]
    out, counts = OC.np_cull(xyz, mask[:, ::-1].copy(), [None, (grid, lo, inv)])
    assert out.tolist() == [[1, 0], [1, 2], [1, 2], [1, 0]] and counts.tolist() == [[0, 0], [2, 2]]


# ---------------------------------------------------------------------------------------- the oracle's expectation
_PLAIN = {}


def plain_unculled():
    if not _PLAIN:
        _PLAIN["ref"] = S.oracle_render(OC.plain_case())
    return _PLAIN["ref"]


@pytest.mark.parametrize("name,dilate", [("half", 0), ("half", 1), ("ball", 0), ("ball", 1)])
def test_condition_on_the_inputs_base_scene(monkeypatch, name, dilate):
    case = OC.plain_case()
    plain = plain_unculled()                                # (with the oracle's own sampler: before the wrapper goes in)
    record = []
    monkeypatch.setattr(O, "sample_coarse", OC.culled_sampler(case, OC.manual_grids(case, name, dilate), record))
    culled = S.oracle_render(case)
    counts = OC.assert_cull_bites(record, f"{name} dilate {dilate}")
    print(name, dilate, counts)
    for i, (kept, lost) in counts.items():
        assert int(plain[f"mask{i}"].sum()) == kept + lost and int(culled[f"mask{i}"].sum()) == kept
    assert torch.equal(culled["t_coarse"], plain["t_coarse"]) and torch.equal(culled["mask0"], plain["mask0"])
    # the coarse mixed image barely moves (the background hides the performers there); the per-layer outputs and the masks do
    assert float((culled["coarse_mixed"] - plain["coarse_mixed"])[:, :3].abs().max()) < 0.05
    assert S.rays_changed(culled["fine_layer1"], plain["fine_layer1"]) >= 8
    # and the comparison the GPU tests apply refuses a render that did not cull (or culled something else)
    with pytest.raises(AssertionError):
        S.assert_matches_oracle(plain, culled, culled, what="unculled render against the culled oracle")


@pytest.mark.parametrize("name,dilate", [("half", 0), ("half", 1), ("ball", 0)])
def test_condition_on_the_inputs_rays_with_one_frame_id(monkeypatch, name, dilate):
    case = OC.plain_case(frame=2.0)
    record = []
    monkeypatch.setattr(O, "sample_coarse", OC.culled_sampler(case, OC.manual_grids(case, name, dilate), record))
    S.oracle_render(case)
    print(name, dilate, OC.assert_cull_bites(record, f"width 7, {name} dilate {dilate}"))


def test_condition_on_the_inputs_first_64_rays_at_64_plus_64(monkeypatch):
    case = OC.plain_case(n1=64, n2=64)
    record = []
    monkeypatch.setattr(O, "sample_coarse", OC.culled_sampler(case, OC.manual_grids(case, "half_x", 0, layers=(1, 3)), record))
    S.oracle_render(case, S.case_rays(case)[:64])
    print(OC.assert_cull_bites(record, "first 64 rays, 64 + 64"))


def test_wrapper_unedits_the_points_from_the_cases_spec(monkeypatch):
    """The full edit case: the un-edit matters (the keep of the un-edited points differs from the keep of the raw points)."""
    case = S.make_case()
    grids = OC.manual_grids(case, "half", 0)
    record = []
    monkeypatch.setattr(O, "sample_coarse", OC.culled_sampler(case, grids, record))
    S.oracle_render(case)
    OC.assert_cull_bites(record, "edited case")
    monkeypatch.undo()
    raw = []
    monkeypatch.setattr(O, "sample_coarse", OC.culled_sampler(dict(case, scale=None, shift=None), grids, raw))
    S.oracle_render(case)
    a, b = OC.kept_and_culled(record), OC.kept_and_culled(raw)
    assert a[3] != b[3], (a, b)                             # (the instance: shifted by 0.35 and scaled by 0.9)


# ---------------------------------------------------------------------------------------- host logic
def fake_builds(monkeypatch, model, calls):
    def density_grid(layer_id, frame_id, res=64, fine=True, direction=(0.0, 0.0, 1.0), retiming=True):
        calls.append((layer_id, float(frame_id), bool(fine)))
        rx, ry, rz = occ.normalise_res(res)
        lo, hi = occ.box_bounds(model.layer_box_at(layer_id, frame_id, retiming))
        return torch.zeros(rz + 1, ry + 1, rx + 1), lo, hi
    monkeypatch.setattr(model, "density_grid", density_grid, raising=False)
    monkeypatch.setattr(ops, "occupancy_build", lambda sc, sf, thr, dil: torch.zeros(ops.occupancy_words((sc.shape[2] - 1, sc.shape[1] - 1, sc.shape[0] - 1)),
                                                                                   dtype=torch.int32))


def test_grid_keys_and_lru(monkeypatch):
    model = base_model(2)
    model.add_instance(1)
    calls = []
    fake_builds(monkeypatch, model, calls)
    grids = occ.OccupancyGrids(res=(5, 7, 9), threshold=0.01, dilate=2, max_grids=3)
    g = grids.grid(model, 1, 2.5, "cpu")
    assert g.res == (5, 7, 9) and g.bits.numel() == (5 * 7 * 9 + 31) // 32 and calls == [(1, 2.5, False), (1, 2.5, True)]
    assert np.array_equal(g.inv_cell, OC.np_inv_cell(g.res, g.lo, g.hi))
    assert grids.grid(model, 1, 2.5, "cpu") is g and (grids.built, grids.reused) == (1, 1)
    assert grids.grid(model, 3, 2.5, "cpu") is g            # the instance of performer 1 at the same id: the source's grid
    assert grids.grid(model, 3, 1.5, "cpu") is not g        # ... at its own id: another one
    assert grids.grid(model, 2, 2.5, "cpu") is not g and len(grids) == 3 and grids.built == 3
    k = grids.key(model, 1, 2.5, g.lo, g.hi)
    with torch.no_grad():
        model.time_deform_nets[0].motion_net[0].weight.add_(0.0)   # the version counter moves
    assert grids.key(model, 1, 2.5, g.lo, g.hi) != k
    assert grids.grid(model, 1, 2.5, "cpu") is not g and grids.built == 4 and len(grids) == 3      # rebuilt; the oldest left
    before = grids.built
    grids.grid(model, 3, 1.5, "cpu")                       # (performer 1's MotionNet changed: its other grid is rebuilt too)
    assert grids.built == before + 1
    model.use_space_time, flag = False, model.use_space_time
    assert grids.key(model, 2, 2.5, g.lo, g.hi) != k and grids.key(model, 2, 2.5, g.lo, g.hi)[-1] != k[-1]
    model.use_space_time = flag
    other = occ.OccupancyGrids(res=(5, 7, 9), threshold=0.01, dilate=1)
    assert other.key(model, 1, 2.5, g.lo, g.hi) != grids.key(model, 1, 2.5, g.lo, g.hi)
    grids.clear()
    assert len(grids) == 0
    st = grids.stats()
    assert st["built"] == grids.built and st["reused"] == grids.reused and st["pairs"] == {}


def test_table_takes_manual_grids_as_given_and_skips_hidden_layers(monkeypatch):
    model = base_model(2)
    calls = []
    fake_builds(monkeypatch, model, calls)
    grids = occ.OccupancyGrids(res=4, auto=False)
    assert grids.culled_layers(model) == []
    lo, hi = [-1.0, -1.0, -1.0], [1.0, 1.0, 2.0]
    grids.set_manual(2, torch.from_numpy(OC.half_y(8)), lo, hi)
    assert grids.culled_layers(model) == [2] and grids.manual_layers() == [2]
    table, held = grids.table(model, [1.0, 2.5, 3.0], "cpu")
    assert table[0] is None and table[1] is None and calls == []
    bits, res, tlo, inv = table[2]
    assert res == (8, 8, 8) and np.array_equal(bits.numpy().view(np.uint32), OC.np_pack(OC.half_y(8)))
    assert tlo == lo and inv == OC.np_inv_cell(res, np.float32(lo), np.float32(hi)).tolist()
    model.hide_layer(2)
    assert grids.culled_layers(model) == []
    model.show_layer(2)
    auto = occ.OccupancyGrids(res=4)
    auto.set_manual(2, torch.from_numpy(OC.half_y(8)), lo, hi)
    assert auto.culled_layers(model) == [1, 2]
    table, _ = auto.table(model, [1.0, 2.5, 3.0], "cpu")
    assert table[1][1] == (4, 4, 4) and table[2][1] == (8, 8, 8) and calls[0] == (1, 2.5, False)
    grids.set_manual(2, None)
    assert grids.manual_layers() == []


def test_manual_grid_shape_checks_and_constructor_checks():
    grids = occ.OccupancyGrids()
    assert (grids.res, grids.threshold, grids.dilate, grids.max_grids) == ((64, 64, 64), 1e-4, 0, 64)
    ok = torch.ones(2, 3, 4, dtype=torch.bool)
    with pytest.raises(ValueError, match="layer 0"):
        grids.set_manual(0, ok, [0, 0, 0], [1, 1, 1])
    with pytest.raises(ValueError, match="bool tensor"):
        grids.set_manual(1, ok.float(), [0, 0, 0], [1, 1, 1])
    with pytest.raises(ValueError, match="bool tensor"):
        grids.set_manual(1, ok[0], [0, 0, 0], [1, 1, 1])
    with pytest.raises(ValueError, match="1..256"):
        grids.set_manual(1, torch.ones(1, 1, 257, dtype=torch.bool), [0, 0, 0], [1, 1, 1])
    with pytest.raises(ValueError, match="bounds"):
        grids.set_manual(1, ok)
    with pytest.raises(ValueError, match="lo < hi"):
        grids.set_manual(1, ok, [0, 0, 0], [1, 0, 1])
    with pytest.raises(ValueError, match="lo < hi"):
        grids.set_manual(1, ok, [0, 0, 0], [1, float("nan"), 1])
    grids.set_manual(1, ok, [0, 0, 0], [1, 1, 1])
    assert grids._manual[1][1] == (4, 3, 2)
    for bad in (dict(res=0), dict(res=257), dict(res=(4, 4)), dict(dilate=5), dict(dilate=-1), dict(dilate=1.5), dict(max_grids=0),
                dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            occ.OccupancyGrids(**bad)
    a, b = occ.OccupancyGrids(), occ.OccupancyGrids()
    assert a.fingerprint() == b.fingerprint() and len(a.fingerprint()) == 8
    assert occ.OccupancyGrids(dilate=2).fingerprint() != a.fingerprint() and occ.OccupancyGrids(res=32).fingerprint() != a.fingerprint()
    b.set_manual(1, ok, [0, 0, 0], [1, 1, 1])
    assert b.fingerprint() != a.fingerprint()
    c = occ.OccupancyGrids()
    c.set_manual(1, ~ok, [0, 0, 0], [1, 1, 1])
    assert c.fingerprint() != b.fingerprint()


def test_cross_rank_fingerprint_covers_the_grids():
    from stnerf_amd.parallel import layers_fingerprint
    model = base_model(2)
    plain = layers_fingerprint(model)
    model.set_occupancy(occ.OccupancyGrids())
    on = layers_fingerprint(model)
    assert len(on) == len(plain) and on != plain
    model.set_occupancy(occ.OccupancyGrids(threshold=0.5))
    assert layers_fingerprint(model) != on
    model.set_occupancy(None)
    assert layers_fingerprint(model) == plain


class OnDevice(torch.Tensor):
    """A CPU tensor that claims to be on the GPU: reaches the host checks that come after the device check."""
    is_cuda = True

    def contiguous(self, *a, **k):
        return self

    def float(self):
        return self


def test_refusals_of_the_render_path():
    model = base_model(2)
    rays = torch.cat([torch.zeros(8, 6), torch.tensor([[1.0, 2.5, 3.0]]).repeat(8, 1)], 1)
    assert model._inference_only_edits() is None
    model.set_occupancy(occ.OccupancyGrids())
    assert "occupancy" in model._inference_only_edits()
    model.train()
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="occupancy"):
        model.render_rays_raw(rays.as_subclass(OnDevice))
    model.eval()
    model.replay = {"jitter": torch.zeros(3, 8, 12), "xyz_c": [None, None, None]}
    with pytest.raises(ValueError, match="xyz_c"):
        model.render_rays_raw(rays.as_subclass(OnDevice))
    model.replay = None
    # one frame id per culled layer and chunk group
    assert model._occupancy_frame_ids(rays, [(0, 8)], True) == [[1.0, 2.5, 3.0]]
    mixed = rays.clone()
    mixed[5, 8] = 2.0
    with pytest.raises(ValueError, match="layer 2"):
        model._occupancy_frame_ids(mixed, [(0, 8)], True)
    assert model._occupancy_frame_ids(mixed, [(0, 5), (5, 6), (6, 8)], True) == [[1.0, 2.5, 3.0], [1.0, 2.5, 2.0], [1.0, 2.5, 3.0]]
    mixed[:, 6] = torch.arange(8.0)                         # the background is never culled: its ids may differ
    assert len(model._occupancy_frame_ids(mixed, [(0, 5)], True)) == 1
    model.hide_layer(2)                                     # neither is a hidden layer
    assert len(model._occupancy_frame_ids(mixed, [(0, 8)], True)) == 1
    model.show_layer(2)
    wide7 = torch.cat([torch.zeros(8, 6), torch.full((8, 1), 2.0)], 1)
    assert model._occupancy_frame_ids(wide7, [(0, 8)], False) == [[2.0, 2.0, 2.0]]
    wide7[3, 6] = 1.0
    with pytest.raises(ValueError, match="layer 1"):
        model._occupancy_frame_ids(wide7, [(0, 8)], False)
    model.set_occupancy(None)
    assert model._inference_only_edits() is None


def test_layer_box_at_is_the_retimed_box_before_the_edits():
    model = base_model(2)
    model.add_instance(1)
    ids = torch.tensor([1.0, 2.5, 3.0, 1.5])
    boxes, _ = model._retimed_boxes(ids)
    for i in (1, 2, 3):
        assert torch.equal(model.layer_box_at(i, float(ids[i])), boxes[i])
    assert torch.equal(model.layer_box_at(3, 1.5), model.layer_box_at(1, 1.5))
    assert torch.equal(model.layer_box_at(2, 2.0, retiming=False), model.bboxes[1, 1])
    with pytest.raises(ValueError):
        model.layer_box_at(0, 1.0)


def test_renderer_property_attaches_and_detaches():
    import types
    from stnerf_amd.render.layered_neural_renderer import LayeredNeuralRenderer
    model = base_model(2)
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=2, FRAME_NUM=3, FRAME_OFFSET=0), INPUT=types.SimpleNamespace(SIZE_TEST=[23, 17]))
    K, T = S.camera()
    mk = lambda **kw: LayeredNeuralRenderer(cfg, model=model, gt_poses=T.reshape(1, 4, 4), gt_Ks=[K], **kw)
    r = mk()
    assert r.occupancy is None and model._occupancy is None
    r.occupancy = True
    first = r.occupancy
    assert isinstance(first, occ.OccupancyGrids) and model._occupancy is first
    r.occupancy = True
    assert r.occupancy is first
    mine = occ.OccupancyGrids(res=32)
    r.occupancy = mine
    assert model._occupancy is mine
    r.occupancy = False
    assert model._occupancy is None
    assert mk(occupancy=mine).occupancy is mine
    with pytest.raises(TypeError):
        r.occupancy = "yes"
    import stnerf_amd
    assert stnerf_amd.OccupancyGrids is occ.OccupancyGrids


# ---------------------------------------------------------------------------------------- the C ABI's checks before any launch
def _table(l=3):
    t = (hip.Occupancy * l)()
    for i in range(1, l):
        t[i].bits = 0x1000
        for a in range(3):
            t[i].res[a], t[i].lo[a], t[i].inv_cell[a] = 8, 0.0, 4.0
    return t


@pytest.mark.parametrize("what,spoil", [("layer 0", lambda t: setattr(t[0], "bits", 0x1000)),
                                        ("1..256", lambda t: t[1].res.__setitem__(1, 0)),
                                        ("1..256", lambda t: t[2].res.__setitem__(2, 257)),
                                        ("inv_cell", lambda t: t[1].inv_cell.__setitem__(0, 0.0)),
                                        ("inv_cell", lambda t: t[2].inv_cell.__setitem__(2, float("inf"))),
                                        ("inv_cell", lambda t: t[2].inv_cell.__setitem__(1, float("nan"))),
                                        ("4-byte aligned", lambda t: setattr(t[2], "bits", 0x1002))])
def test_cull_entry_refuses_a_bad_table_before_any_launch(what, spoil):
    lib = hip.lib()
    t = _table()
    spoil(t)
    fake = C.c_void_p(0x1000)                               # never dereferenced: the checks come before any launch
    assert lib.stnerf_occupancy_cull(fake, 4, 3, 12, t, fake, None, None) == hip.EINVAL
    assert what in hip.last_error()


def test_entries_are_exported_and_declared():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stnerf.h")).read()
    for name in ("stnerf_occupancy_build", "stnerf_occupancy_cull", "stnerf_render_rays_occupancy"):
        assert name in hip.exported_symbols() and getattr(hip.lib(), name) is not None and name + "(" in header
    assert "typedef struct stnerf_occupancy {" in header
    assert C.sizeof(hip.Occupancy) == 48
    assert ops.PROFILE_KERNELS[7:9] == ("occupancy_cull", "occupancy_build") and ops.PROFILE_KERNELS[6] == "copy_layer_raw"
    lib = hip.lib()
    fake, res = C.c_void_p(0x1000), (C.c_int32 * 3)(4, 4, 4)
    assert lib.stnerf_occupancy_build(fake, None, res, 0.1, 5, fake, None) == hip.EINVAL and "dilate" in hip.last_error()
    assert lib.stnerf_occupancy_build(None, None, res, 0.1, 1, fake, None) == hip.EINVAL
    assert lib.stnerf_occupancy_build(fake, None, (C.c_int32 * 3)(4, 300, 4), 0.1, 1, fake, None) == hip.EINVAL
    with pytest.raises(ValueError, match="one entry per layer"):
        ops._occupancy_table([None, None], 3)
