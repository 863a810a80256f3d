"""Occupancy grids on the GPU (csrc/occupancy.hip, stnerf_render_rays_occupancy, stnerf_amd.OccupancyGrids): the build and the
cull against their numpy restatements bit for bit, all-ones grids and kept pairs against the un-culled render bit for bit, culled
renders against the CPU oracle with its sampler wrapped (``occupancy_common.culled_sampler``: ``masks[i] &= keep_i``) under
``scene_edits_common.assert_matches_oracle`` with its bars as they are, model-built grids, and the neighbours: the background
cache, the MotionNet reuse, the launch profiler.  Shapes: 391 rays or fewer, n1 <= 90, grids of at most 33 cells a side.
Needs an MI355X: `pytest -m gpu`."""
import os

import numpy as np
import pytest
import torch

import occupancy_common as OC
import scene_edits_common as S
import test_gpu_bkgd_cache as BC
import test_gpu_scene_edits_oracle as SE
from oracle import stnerf_oracle as O
from pipeline_chain import detach_models
from stnerf_amd import ops
from stnerf_amd.occupancy import OccupancyGrids
from test_gpu_ops import _net_close

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def detach():
    yield
    detach_models()


def words(bits):
    return bits.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------- 1. build vs numpy
@pytest.mark.parametrize("res", [(5, 7, 9), (33, 4, 3)])
@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_build_equals_numpy_bit_for_bit(res, dilate):
    rx, ry, rz = res
    thr = np.float32(0.25)
    rs = np.random.RandomState(7 + dilate)
    arrays = []
    # dense vertices in the first third of the longest axis only: the grid stays partly empty under every dilation
    third = np.zeros((rz + 1, ry + 1, rx + 1), bool)
    if rx > rz:
        third[:, :, :rx // 3 + 1] = True
    else:
        third[:rz // 3 + 1] = True
    for _ in range(2):
        sig = np.where((rs.rand(rz + 1, ry + 1, rx + 1) < 0.06) & third, thr + 1, thr - 1).astype(np.float32)
        flat = sig.reshape(-1)
        at = rs.choice(np.nonzero(third.reshape(-1))[0], 8, replace=False)
        flat[at[0:2]] = thr                                        # exactly at the threshold: not dense
        flat[at[2:4]] = np.nextafter(thr, np.float32(-1))          # just below
        flat[at[4:6]] = np.nextafter(thr, np.float32(1))           # just above: dense
        flat[at[6]] = np.nan                                       # dense
        arrays.append(sig)
    sc, sf = arrays
    n_words = (rx * ry * rz + 31) // 32
    for a, b in ((sc, None), (None, sf), (sc, sf)):
        want = OC.np_build(a, b, thr, dilate)
        assert 0 < want.sum() < want.size
        got = words(ops.occupancy_build(None if a is None else torch.from_numpy(a).cuda(), None if b is None else torch.from_numpy(b).cuda(),
                                        float(thr), dilate))
        assert got.shape == (n_words,) and np.array_equal(got, OC.np_pack(want)), (res, dilate, a is None, b is None)
        assert (rx * ry * rz) % 32 != 0 and int(got[-1]) >> ((rx * ry * rz) % 32) == 0        # the unused bits of the last word
    with pytest.raises(ValueError, match="dilate"):
        ops.occupancy_build(torch.from_numpy(sc).cuda(), None, float(thr), 5)


# ---------------------------------------------------------------------------------------- 2. cull op vs numpy
@pytest.mark.parametrize("n1", [5, 64, 90])
@pytest.mark.parametrize("both", [False, True])
def test_cull_equals_numpy_on_the_whole_mask(n1, both):
    n, l = 97, 3
    rs = np.random.RandomState(100 + n1 + both)
    g1 = rs.rand(8, 8, 8) < 0.12
    g1[0, 0, 0], g1[7, 7, 7], g1[0, 0, 3], g1[0, 0, 2] = True, False, True, False
    lo1, hi1 = np.array([-1, -1, -1], np.float32), np.array([1, 1, 1], np.float32)       # cells of 0.25: faces are exact
    g2 = rs.rand(9, 7, 5) < 0.12                                                         # (Rx, Ry, Rz) = (5, 7, 9)
    lo2, hi2 = np.array([-1.2, -0.9, 0.31], np.float32), np.array([0.37, 1.05, 2.9], np.float32)
    grids = [None, (g1, lo1, hi1), (g2, lo2, hi2) if both else None]
    # every pair's points run along a short segment inside (and a little beyond) the bounds of layer 2's grid / layer 1's
    start = rs.uniform(-1.3, 1.3, (n, l, 1, 3))
    step = rs.uniform(-0.4, 0.4, (n, l, 1, 3)) / n1
    xyz = (start + step * np.arange(n1).reshape(1, 1, n1, 1)).astype(np.float32)
    xyz[:, 2] = (xyz[:, 2] * np.float32(0.6) + np.array([-0.4, 0.1, 1.6], np.float32)).astype(np.float32)
    mask = rs.randint(0, 4, (n, l)).astype(np.uint8)                                     # bits 0 and 1 in all four combinations
    mask[:6, 1] = 1
    xyz[0, 1] = np.array([-0.25, -1.0, -1.0], np.float32)                                # on the faces of cell (3, 0, 0): occupied
    below = np.float32(-1.0) + np.nextafter(np.float32(0.75), np.float32(0))             # (exact: the next float below would round back up)
    xyz[1, 1] = np.array([below, -1.0, -1.0], np.float32)                                # just below the face: cell (2, 0, 0)
    xyz[2, 1] = np.array([-1.5, -1.001, -7.0], np.float32)                               # outside lo: clamped to cell (0, 0, 0)
    xyz[3, 1] = np.array([1.5, 1.0, 1e30], np.float32)                                   # outside hi: clamped to cell (7, 7, 7)
    xyz[4, 1] = xyz[3, 1]
    xyz[4, 1, n1 - 1, 1] = np.nan                                                        # one NaN coordinate: occupied
    xyz[5, 1] = xyz[1, 1]
    xyz[5, 1, n1 - 1] = xyz[0, 1, 0]                                                     # the hit is the last point (a ragged trip's)
    table = [None if g is None else (g[0], g[1], OC.np_inv_cell((g[0].shape[2], g[0].shape[1], g[0].shape[0]), g[1], g[2])) for g in grids]
    want, want_counts = OC.np_cull(xyz, mask, table)
    assert want[:6, 1].tolist() == [1, 0, 1, 0, 1, 1]
    for i in (1, 2) if both else (1,):
        assert want_counts[i, 1] >= 5 and want_counts[i, 0] - want_counts[i, 1] >= 5, want_counts
    dev_table = []
    for g in grids:
        if g is None:
            dev_table.append(None)
            continue
        res = (g[0].shape[2], g[0].shape[1], g[0].shape[0])
        dev_table.append((torch.from_numpy(OC.np_pack(g[0]).view(np.int32)).cuda(), res, g[1].tolist(), OC.np_inv_cell(res, g[1], g[2]).tolist()))
    x_dev, m_dev = torch.from_numpy(xyz).cuda(), torch.from_numpy(mask).cuda()
    counts = torch.zeros(l, 2, dtype=torch.int32, device="cuda")
    x_before = x_dev.clone()
    assert ops.occupancy_cull(x_dev, m_dev, dev_table, counts) is m_dev
    assert torch.equal(m_dev.cpu(), torch.from_numpy(want))
    assert torch.equal(m_dev.cpu()[:, 0], torch.from_numpy(mask[:, 0])) and (both or torch.equal(m_dev.cpu()[:, 2], torch.from_numpy(mask[:, 2])))
    assert torch.equal((m_dev.cpu() & 2), torch.from_numpy(mask & 2))                    # bit 1 comes back unchanged
    assert torch.equal(counts.cpu().long(), torch.from_numpy(want_counts))
    assert torch.equal(x_dev.view(torch.int32), x_before.view(torch.int32))
    m2 = torch.from_numpy(mask).cuda()
    ops.occupancy_cull(x_dev, m2, dev_table)                                             # without counters: the same mask
    assert torch.equal(m2, m_dev)
    with pytest.raises(ValueError, match="layer 0"):
        ops.occupancy_cull(x_dev, m2, [dev_table[1], None, None])


# ---------------------------------------------------------------------------------------- renders
def attach(model, grids_spec, **kw):
    """Manual grids {layer: (occupied, lo, hi)} on the model -> the OccupancyGrids."""
    grids = OccupancyGrids(auto=False, **kw)
    for i, (occ, lo, hi) in grids_spec.items():
        grids.set_manual(i, torch.from_numpy(np.ascontiguousarray(occ)), lo, hi)
    model.set_occupancy(grids)
    return grids


def assert_same_bits(a, b, what, rows=None):
    assert set(a) == set(b)
    for k in sorted(a):
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        same = torch.equal(x, y) if x.dtype == torch.bool else torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
        assert same, f"{what}: {k} differs"


@pytest.mark.parametrize("precision,schedule", [("bf16x3", "stage"), ("fp32", "stage"), ("fp32", "per_net")])
@pytest.mark.parametrize("only_coarse", [False, True])
def test_all_ones_grids_change_nothing(precision, schedule, only_coarse):
    case = S.make_case(only_coarse=only_coarse)
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case, precision, schedule)
    plain = SE.gpu_render(model, case, rays)
    grids = attach(model, {i: (np.ones((8, 8, 8), bool),) + OC.layer_bounds(case, i) for i in (1, 2, 3)})
    culled = SE.gpu_render(model, case, rays)
    assert_same_bits(culled, plain, f"all-ones grids, {precision}/{schedule}")
    pairs = grids.stats()["pairs"]
    assert sorted(pairs) == [1, 2, 3] and all(c == 0 and t == int(plain[f"mask{i}"].sum()) for i, (t, c) in pairs.items())


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_kept_pairs_are_untouched(precision):
    case = S.make_case()
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case, precision)
    plain = SE.gpu_render(model, case, rays)
    grids = attach(model, OC.manual_grids(case, "half", 0))
    culled = SE.gpu_render(model, case, rays)
    same = torch.ones(S.N, dtype=torch.bool)
    for i in range(4):
        same &= culled[f"mask{i}"] == plain[f"mask{i}"]
        assert not bool((culled[f"mask{i}"] & ~plain[f"mask{i}"]).any())
    assert 8 <= int(same.sum()) <= S.N - 8
    assert_same_bits(culled, plain, "rays on which no layer was culled", rows=same)
    # (the pipeline's t_c is no output of a render, and the cull entry is not handed it: the xyz bytes are held at op level above,
    # the depths of culled pairs by the oracle cases below, through every per-layer output)
    pairs = grids.stats()["pairs"]
    for i in (1, 2, 3):
        assert pairs[i] == (int(plain[f"mask{i}"].sum()), int(plain[f"mask{i}"].sum()) - int(culled[f"mask{i}"].sum())) and pairs[i][1] >= 8


# ---------------------------------------------------------------------------------------- 5. against the oracle
_ORACLE = {}


def culled_oracle(name, case, grids_spec, rays, monkeypatch):
    """(fp32, fp64) oracle renders with the wrapped sampler, once per case; the condition on the inputs is asserted here."""
    if name not in _ORACLE:
        record = []
        monkeypatch.setattr(O, "sample_coarse", OC.culled_sampler(case, grids_spec, record))
        ref32 = S.oracle_render(case, rays)
        counts = OC.assert_cull_bites(record, name)
        monkeypatch.undo()                                       # the second wrapper wraps the oracle's own sampler, not the first
        monkeypatch.setattr(O, "sample_coarse", OC.culled_sampler(case, grids_spec))
        ref64 = S.oracle_render(case, rays, torch.float64)
        monkeypatch.undo()
        _ORACLE[name] = (ref32, ref64, counts)
    return _ORACLE[name]


def run_culled(name, case, grids_spec, monkeypatch, precision, schedule="stage", rays=None):
    rays = S.case_rays(case) if rays is None else rays
    ref32, ref64, counts = culled_oracle(name, case, grids_spec, rays, monkeypatch)
    model = SE.make_model(case, precision, schedule)
    grids = attach(model, grids_spec)
    got = SE.gpu_render(model, case, rays.cuda())
    SE.report(f"{name} {precision}/{schedule}", S.assert_matches_oracle(got, ref32, ref64, case["only_coarse"], name))
    pairs = grids.stats()["pairs"]
    for i, (kept, lost) in counts.items():
        assert pairs[i] == (kept + lost, lost), (name, i, pairs, counts)
    return got, ref32, model


PRECISIONS = ["bf16x3", "fp32"]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("grid,dilate", [("half", 0), ("ball", 1)])
def test_plain_retiming(monkeypatch, precision, grid, dilate):
    case = OC.plain_case()
    run_culled(f"plain {grid} {dilate}", case, OC.manual_grids(case, grid, dilate), monkeypatch, precision)


def test_plain_retiming_one_launch_per_network(monkeypatch):
    case = OC.plain_case()
    run_culled("plain half 0", case, OC.manual_grids(case, "half", 0), monkeypatch, "fp32", "per_net")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rays_with_one_frame_id(monkeypatch, precision):
    case = OC.plain_case(frame=2.0)
    run_culled("width 7", case, OC.manual_grids(case, "half", 1), monkeypatch, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_only_coarse(monkeypatch, precision):
    case = OC.plain_case(only_coarse=True, near=4.0)
    got, _, _ = run_culled("only_coarse", case, OC.manual_grids(case, "half", 0), monkeypatch, precision)
    assert torch.equal(got["fine_mixed"], got["coarse_mixed"])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_full_edit_case(monkeypatch, precision):
    """Rotation, shift and scale, an instance with a manual grid on its own slot, the opacity table, scene passes."""
    case = S.make_case()
    got, ref32, model = run_culled("full edits", case, OC.manual_grids(case, "half", 0), monkeypatch, precision)
    assert model.instances == (1,) and model._occupancy.manual_layers() == [1, 2, 3]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_frame_ids_that_change_at_a_chunk_boundary(monkeypatch, precision):
    """Two chunk groups, the same manual grids in both."""
    ids = OC.plain_case()["groups"][0][1]
    case = OC.plain_case(groups=[(0, ids), (256, [1.0, 1.5, 2.0, 3.0])])
    run_culled("two groups", case, OC.manual_grids(case, "half", 0), monkeypatch, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_sixty_four_plus_sixty_four_on_the_first_64_rays(monkeypatch, precision):
    """Layer 2 has 5 hit pairs among these rays: the grids are on layers 1 and 3, halved in x (the rays are the view's first rows)."""
    case = OC.plain_case(n1=64, n2=64)
    run_culled("64+64", case, OC.manual_grids(case, "half_x", 0, layers=(1, 3)), monkeypatch, precision, rays=S.case_rays(case)[:64])


def test_mixed_frame_ids_in_a_group_are_refused():
    case = OC.plain_case()
    rays = S.case_rays(case).cuda()
    rays[100, 7] = 1.0
    model = SE.make_model(case)
    attach(model, OC.manual_grids(case, "half", 0))
    with pytest.raises(ValueError, match="layer 1"):
        model.render_rays_raw(rays, False, case["thr"], case["bthr"], ref_chunk=case["chunk"])


# ---------------------------------------------------------------------------------------- 6. model-built grids
BUILT = dict(res=8, threshold=2.3, dilate=0)      # the synthetic fields are dense almost everywhere at 1e-4: a threshold at which
                                                  # the CPU oracle culls 84 of layer 1's 144 and 79 of layer 3's 128 hit pairs


def test_density_grid_against_the_fp64_oracle_and_the_direction():
    case = OC.plain_case()
    model = SE.make_model(case)
    fid = 2.5
    sd = {k: v.double() for k, v in S._state(2)[0].items()}
    for fine in (False, True):
        sig, lo, hi = model.density_grid(1, fid, 8, fine=fine)
        other, _, _ = model.density_grid(1, fid, 8, fine=fine, direction=(0.6, 0.0, -0.8))
        assert sig.shape == (9, 9, 9) and torch.equal(sig.view(torch.int32), other.view(torch.int32))
        wlo, whi = OC.layer_bounds(case, 1)
        assert np.array_equal(lo, wlo) and np.array_equal(hi, whi)
        vx, vy, vz = OC.np_vertices((8, 8, 8), lo, hi)
        Z, Y, X = np.meshgrid(vz, vy, vx, indexing="ij")
        x = torch.from_numpy(np.stack([X, Y, Z], -1).reshape(-1, 3)).double()
        t = torch.full((x.shape[0], 1), fid, dtype=torch.float64)
        moved = x + O.motion_net(sd, "time_deform_nets.0", torch.cat([x, t], -1))
        _, sig64 = O.space_net(sd, "spacenets_fine.0" if fine else "spacenets.0", moved.unsqueeze(1),
                               torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64).repeat(x.shape[0], 1), t)
        err = (sig.cpu().double().reshape(-1) - sig64.reshape(-1)).abs()
        print(f"density_grid fine={fine}: max |err| {float(err.max()):.3e}, max |sigma| {float(sig64.abs().max()):.3e}")
        _net_close(sig.cpu().reshape(-1), sig64.reshape(-1), 60.0, f"density_grid sigma (fine={fine})")
    bk, _, _ = model.density_grid(0, 1.0, (3, 2, 4))
    assert bk.shape == (5, 3, 4) and bool(torch.isfinite(bk).all())


def test_model_built_grids_bits_render_and_reuse(monkeypatch):
    case = OC.plain_case(hidden=(2,))
    rays = S.case_rays(case)
    model = SE.make_model(case)
    grids = OccupancyGrids(**BUILT)
    model.set_occupancy(grids)
    assert grids.culled_layers(model) == [1, 3]
    got = SE.gpu_render(model, case, rays.cuda())
    assert grids.built == 2 and grids.reused == 2 * 3            # (four launch pieces: the first builds, the others reuse)
    ids = case["groups"][0][1]
    spec = {}
    for i in (1, 3):
        g = grids.grid(model, i, ids[i], rays.cuda().device)
        sc, lo, hi = model.density_grid(i, ids[i], 8, fine=False)
        sf, _, _ = model.density_grid(i, ids[i], 8, fine=True)
        want = OC.np_build(sc.cpu().numpy(), sf.cpu().numpy(), BUILT["threshold"], BUILT["dilate"])     # of the DEVICE's sigma
        assert np.array_equal(words(g.bits), OC.np_pack(want)) and 0.05 < want.mean() < 0.6
        assert np.array_equal(g.lo, OC.layer_bounds(case, i)[0]) and np.array_equal(g.inv_cell, OC.np_inv_cell((8, 8, 8), lo, hi))
        spec[i] = (OC.np_unpack(words(g.bits), (8, 8, 8)), g.lo, g.hi)                                  # the same bits, on the host
    ref32, ref64, counts = culled_oracle("model-built", case, spec, rays, monkeypatch)
    SE.report("model-built", S.assert_matches_oracle(got, ref32, ref64, False, "model-built grids"))
    pairs = grids.stats()["pairs"]
    assert all(pairs[i] == (k + c, c) for i, (k, c) in counts.items())
    built, reused = grids.built, grids.reused
    again = SE.gpu_render(model, case, rays.cuda())
    assert (grids.built, grids.reused) == (built, reused + 2 * 4)
    assert_same_bits(again, got, "a second frame at the same ids")
    with torch.no_grad():
        model.spacenets[0].density_net[0].bias.add_(0.0)         # a parameter update, through the version counter
    SE.gpu_render(model, case, rays.cuda())
    assert grids.built == built + 2


# ---------------------------------------------------------------------------------------- 7. neighbours
def cache_grids(model):
    bounds = lambda i: OC.np_bounds(model.layer_box_at(i, 2.5))
    return attach(model, {i: (OC.half_y(8),) + bounds(i) for i in (1, 2)})


def test_background_cache_reuse_frame_equals_the_culled_uncached_frame():
    model = BC.make_model(2)
    from stnerf_amd import synthetic as syn
    K, T = syn.camera(BC.H, BC.W, 15.0)
    fa, fb = BC.fids(True, 2, (1.0, 1.0)), BC.fids(True, 2, (2.5, 3.0))
    plain = BC.uncached(model, K, T, fb)
    grids = cache_grids(model)
    BC.render(model, K, T, fa)                                   # capture
    hit = BC.render(model, K, T, fb)
    assert BC.stats(model)[0] == BC.PIECES                       # the cache's key does not see the grids: every piece hits
    ref = BC.uncached(model, K, T, fb)
    BC.assert_bit_equal(hit, ref, "culled reuse frame")
    culled = sum(c for _, c in grids.stats()["pairs"].values())
    assert culled >= 16 and not torch.equal(ref[4], plain[4])


def test_motion_reuse_and_fused_give_equal_bits_under_a_cull():
    case = S.make_case()
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case)
    attach(model, OC.manual_grids(case, "half", 0))
    old = os.environ.get("STNERF_MOTION_REUSE")
    outs = []
    try:
        for value in ("0", None):
            os.environ.pop("STNERF_MOTION_REUSE", None)
            if value is not None:
                os.environ["STNERF_MOTION_REUSE"] = value
            outs.append(SE.gpu_render(model, case, rays))
    finally:
        os.environ.pop("STNERF_MOTION_REUSE", None)
        if old is not None:
            os.environ["STNERF_MOTION_REUSE"] = old
    assert_same_bits(outs[0], outs[1], "STNERF_MOTION_REUSE=0 against the default")


def test_a_render_without_occupancy_records_no_occupancy_kernel():
    case = OC.plain_case()
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case)

    def records():
        ops.profile_begin()
        with torch.no_grad():
            model.render_rays_raw(rays, False, case["thr"], case["bthr"], ref_chunk=case["chunk"])
        torch.cuda.synchronize()
        return ops.profile_end()
    plain = records()
    assert plain and not [r for r in plain if r["kernel"].startswith("occupancy")]
    attach(model, OC.manual_grids(case, "half", 0, layers=(1, 3)))
    culled = [r for r in records() if r["kernel"].startswith("occupancy")]
    pieces = (S.N + S.CAP - 1) // S.CAP
    assert [r["kernel"] for r in culled] == ["occupancy_cull"] * (2 * pieces) and sorted({r["tag"] for r in culled}) == [1, 3]
    assert all(r["ns"] == case["n1"] and r["bytes_per_ray"] == 12 * case["n1"] + 2 for r in culled)
    names = lambda recs: [r["kernel"] for r in recs if not r["kernel"].startswith("occupancy")]
    assert names(records()) == names(plain)                      # everything else is launched as before
