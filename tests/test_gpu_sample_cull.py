"""The sample cull on the GPU (csrc/sample_rows.hip: sample_rows_kernel; the row-list flavours of the stage
kernels, csrc/mlp_wave_rows.hip and csrc/mlp_bf16x3_rows.hip; stnerf_render_rays_samples; OccupancyGrids(samples=True)):
  1. the rows kernel against the numpy restatement of the rule, bit for bit, with every byte around it;
  2. the row-list stage kernels against the unlisted launch, bit for bit at the listed samples, nothing written elsewhere;
  3. the sample-culled pipeline against its definition, a chain of op-level entries, bit for bit;
  4. all-ones grids with samples=True change no bit;
  5. sample-culled renders against the CPU oracle (``sample_cull_common.SampledNets``) under ``assert_matches_oracle`` as it is;
  7. a render without the sample cull launches no rows kernel and no row-list stage kernel, in the workspace it always had.
Shapes: the 17 x 23 view with (12, 6) samples, 64 + 64 on the first 64 rays, op-level launches of 37 / 200 rays.
Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import occupancy_common as OC
import sample_cull_common as SC
import scene_edits_common as S
import test_gpu_bkgd_cache as BC
import test_gpu_scene_edits_oracle as SE
from pipeline_chain import assert_pairs_equal, bits, detach_models, with_chain
from stnerf_amd import hip, ops, synthetic as syn
from stnerf_amd.occupancy import OccupancyGrids
from test_gpu_occupancy import assert_same_bits, attach

pytestmark = pytest.mark.gpu

POISON = 0x7FC0BEEF      # a NaN pattern no kernel writes


@pytest.fixture(autouse=True)
def detach():
    yield
    detach_models()


# ---------------------------------------------------------------------------------------- 1. the rows kernel vs numpy
def _grid(name, rs):
    if name == "ones":
        return np.ones((8, 8, 8), bool)
    if name == "zeros":
        return np.zeros((8, 8, 8), bool)
    return OC.GRIDS[name](8)


@pytest.mark.parametrize("ns", [5, 64, 90, 192])
@pytest.mark.parametrize("grid", ["half", "ball", "ones", "zeros"])
def test_rows_kernel_equals_numpy(ns, grid):
    n, l, layer = 37, 3, 1
    rs = np.random.RandomState(1000 + ns)
    occ = _grid(grid, rs)
    lo, hi = np.array([-1, -1, -1], np.float32), np.array([1, 1, 1], np.float32)         # cells of 0.25: faces are exact
    start = rs.uniform(-1.3, 1.3, (n, l, 1, 3))
    step = rs.uniform(-1.5, 1.5, (n, l, 1, 3)) / ns
    xyz = (start + step * np.arange(ns).reshape(1, 1, ns, 1)).astype(np.float32)
    xyz[0, layer, 0] = np.array([-0.25, -1.0, -1.0], np.float32)                         # on the faces of cell (3, 0, 0)
    xyz[0, layer, 1] = np.array([np.float32(-1.0) + np.nextafter(np.float32(0.75), np.float32(0)), -1.0, -1.0], np.float32)   # just below
    xyz[1, layer, ns - 1] = np.array([1.5, 1.0, 1e30], np.float32)                       # outside hi: clamped to cell (7, 7, 7)
    xyz[2, layer, ns // 2, 1] = np.nan                                                   # a NaN coordinate: listed
    xyz[3, layer, 0] = np.array([-1.5, -1.001, -7.0], np.float32)                        # outside lo: cell (0, 0, 0)
    g_np, g_dev = SC.grid_entry(occ, lo, hi), SC.device_entry(occ, lo, hi)
    x_dev = torch.from_numpy(xyz).cuda()
    perm = rs.permutation(n).astype(np.int32)
    cap = n * ns
    for rays, give_list in ((perm[:29], True), (perm[:0], True), (np.arange(n, dtype=np.int32), False)):
        want_rows, listed = SC.np_rows(xyz[:, layer], rays, g_np)
        if grid in ("half", "ball") and len(rays):
            assert 0 < listed[rays].sum() < len(rays) * ns
        raw = torch.full((n, l, ns, 4), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        buf = torch.full((cap + 16,), POISON, dtype=torch.int32, device="cuda")
        count = torch.full((3,), POISON, dtype=torch.int32, device="cuda")
        counts = torch.zeros(l, 2, dtype=torch.int64, device="cuda")
        counts[2, 0], counts[layer, 0], counts[layer, 1] = 77, 5, 3                      # accumulated into, the other rows untouched
        lst = cnt = None
        if give_list:
            lst = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            lst[:len(rays)] = torch.from_numpy(rays).cuda()
            cnt = torch.tensor([len(rays)], dtype=torch.int32, device="cuda")
        rl, rc = ops.occupancy_rows(x_dev[:, layer], raw[:, layer], g_dev, layer=layer, ray_list=lst, ray_count=cnt, row_list=buf[:cap],
                                    row_count=count[1:2], counts=counts)
        torch.cuda.synchronize()
        got_n = int(count[1])
        got = buf[:got_n].cpu().numpy().astype(np.int64)
        assert got_n == len(want_rows) and np.array_equal(np.sort(got), want_rows), (ns, grid, got_n, len(want_rows))
        assert SC.rows_are_contiguous_and_ascending(got)
        assert int(count[0]) == POISON and int(count[2]) == POISON
        assert bool((buf[cap:] == POISON).all()) and bool((buf[got_n:cap] == POISON).all())           # canaries, and no word past the count
        want_raw = np.full((n, l, ns, 4), POISON, np.int32)
        tested = np.zeros(n, bool)
        tested[rays] = True
        want_raw[:, layer][tested[:, None] & ~listed] = 0
        assert np.array_equal(bits(raw).cpu().numpy(), want_raw)                                       # zeros exactly there, every other byte kept
        t = len(rays) * ns
        assert counts.cpu().tolist() == [[0, 0], [5 + t, 3 + t - len(want_rows)], [77, 0]]
        assert torch.equal(bits(x_dev).cpu(), torch.from_numpy(xyz).view(torch.int32))
    with pytest.raises(ValueError, match="layer 0"):
        ops.occupancy_rows(x_dev[:, 0], raw[:, 0], g_dev, layer=0)
    with pytest.raises(ValueError, match="capacity"):
        ops.occupancy_rows(x_dev[:, 1], raw[:, 1], g_dev, layer=1, row_list=buf[:cap - 1])


# ---------------------------------------------------------------------------------------- 2. the row-list stage kernels
def _stage_scene(precision, deep, n, ns):
    torch.manual_seed(7)
    rs = np.random.RandomState(77)
    l = 3
    sd_b = syn.spacenet_state("net", rs, False, deep_rgb=deep)
    sd_p = [syn.spacenet_state("net", rs, True, deep_rgb=deep) for _ in range(l - 1)]
    sd_m = [syn.motionnet_state("net", rs) for _ in range(l - 1)]
    xyz = ((torch.rand(n, l, ns, 3) - 0.5) * 5.0).cuda()
    dirs = torch.nn.functional.normalize(torch.randn(n, 3), dim=-1)
    times = torch.where(torch.rand(n, l) < 0.5, torch.floor(torch.rand(n, l) * 30), torch.rand(n, l) * 30) + 1
    mask = (torch.rand(n, l) < 0.6).to(torch.uint8)
    mask[:, 0] = 1
    rays = torch.cat([torch.zeros(n, 3), dirs, times], -1).cuda()
    lst, cnt = ops.compact_rays(mask.cuda())
    bk = ops.pack_spacenet(sd_b, "net", precision=precision)
    sp = [ops.pack_spacenet(s_, "net", precision=precision) for s_ in sd_p]
    mo = [ops.pack_motionnet(s_, "net", precision=precision) for s_ in sd_m]

    def launch(rows):
        """rows: {layer: (row_list, row_count)} -> raw (n,l,ns,4) over poison"""
        raw = torch.full((n, l, ns, 4), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        layers = []
        for i in (1, 2):
            ly = dict(space=sp[i - 1], motion=mo[i - 1], xyz=xyz[:, i], raw=raw[:, i], times=rays[:, 6 + i], ray_list=lst[i], ray_count=cnt[i:i + 1])
            if i in rows:
                ly["row_list"], ly["row_count"] = rows[i]
            layers.append(ly)
        layers.append(dict(space=bk, motion=None, xyz=xyz[:, 0], raw=raw[:, 0], times=None, plain_time=True))
        ops.mlp_stage(layers, rays[:, 3:6], ns, deep_rgb=deep, sigmoid_rgb=True)
        torch.cuda.synchronize()
        return bits(raw).cpu()
    return mask.bool(), launch


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("deep", [False, True])
def test_row_list_stage_kernels_write_the_unlisted_launch_s_bytes(precision, deep):
    n, ns, l = 200, 12, 3
    hit, launch = _stage_scene(precision, deep, n, ns)
    plain = launch({})
    poison = torch.full_like(plain, POISON)
    assert torch.equal(plain[~hit], poison[~hit]) and not bool((plain[hit] == POISON).all(-1).all(-1).any())
    rs = np.random.RandomState(5)
    hit1 = np.nonzero(hit[:, 1].numpy())[0]
    assert len(hit1) > 64 + 16
    order = rs.permutation(hit1)                                                        # a shuffled ray order
    dense = (order[:, None].astype(np.int64) << 8 | np.arange(ns)[None, :]).reshape(-1)  # every sample of every hit ray
    sparse = (order.astype(np.int64) << 8) | rs.randint(0, ns, len(order))               # one sample per ray: an item spans 128 rays
    cases = [("dense", dense, c) for c in (0, 1, 127, 128, 129, len(dense))] + [("sparse", sparse, len(sparse))]
    for name, words, c in cases:
        buf = torch.full((n * ns,), -1, dtype=torch.int32, device="cuda")                # (a word past the count names no valid row)
        buf[:len(words)] = torch.from_numpy(words.astype(np.int32)).cuda()
        count = torch.tensor([c], dtype=torch.int32, device="cuda")
        got = launch({1: (buf, count)})
        listed = torch.zeros(n, ns, dtype=torch.bool)
        w = torch.from_numpy(words[:c])
        listed[w >> 8, w & 255] = True
        assert int(listed.sum()) == c
        assert torch.equal(got[:, 1][listed], plain[:, 1][listed]), (name, c)           # the same 16 bytes at every listed sample
        assert torch.equal(got[:, 1][~listed], poison[:, 1][~listed]), (name, c)        # nothing elsewhere
        assert torch.equal(got[:, 2], plain[:, 2]) and torch.equal(got[:, 0], plain[:, 0]), (name, c)   # the unlisted layer, the background
    # both performers listed, each with its own list
    hit2 = np.nonzero(hit[:, 2].numpy())[0]
    w2 = (hit2[:, None].astype(np.int64) << 8 | np.arange(0, ns, 2)[None, :]).reshape(-1)
    b1 = torch.from_numpy(dense.astype(np.int32)).cuda()
    b2 = torch.from_numpy(w2.astype(np.int32)).cuda()
    got = launch({1: (b1, torch.tensor([len(dense)], dtype=torch.int32, device="cuda")),
                  2: (b2, torch.tensor([len(w2)], dtype=torch.int32, device="cuda"))})
    assert torch.equal(got[:, 1], plain[:, 1]) and torch.equal(got[:, 0], plain[:, 0])
    even = torch.zeros(n, ns, dtype=torch.bool)
    even[torch.from_numpy(hit2)[:, None], torch.arange(0, ns, 2)[None, :]] = True
    assert torch.equal(got[:, 2][even], plain[:, 2][even]) and torch.equal(got[:, 2][~even], poison[:, 2][~even])


# ---------------------------------------------------------------------------------------- 3. the pipeline equals its definition
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
@pytest.mark.parametrize("only_coarse", [False, True])
@pytest.mark.parametrize("edits", ["plain", "full"])
def test_pipeline_equals_its_definition(monkeypatch, precision, only_coarse, edits):
    case = OC.plain_case(only_coarse=only_coarse) if edits == "plain" else S.make_case(only_coarse=only_coarse)
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case, precision)
    grids = attach(model, OC.manual_grids(case, "half_x", 0), samples=True)
    pairs = []
    with_chain(model, monkeypatch, pairs)
    SE.gpu_render(model, case, rays)
    assert len(pairs) == (S.N + S.CAP - 1) // S.CAP
    assert_pairs_equal(pairs, f"{edits} {precision} only_coarse={only_coarse}")
    samples = grids.stats()["samples"]
    assert sorted(samples) == [1, 2, 3] and all(0 < skipped < tested for tested, skipped in samples.values()), samples


def test_pipeline_equals_its_definition_on_a_background_cache_reuse_frame(monkeypatch):
    model = BC.make_model(2)
    K, T = syn.camera(BC.H, BC.W, 15.0)
    fa, fb = BC.fids(True, 2, (1.0, 1.0)), BC.fids(True, 2, (2.5, 3.0))
    bounds = lambda i: OC.np_bounds(model.layer_box_at(i, 2.5))
    grids = attach(model, {i: (OC.half_x(8),) + bounds(i) for i in (1, 2)}, samples=True)
    BC.render(model, K, T, fa)                                   # capture
    pairs = []
    with_chain(model, monkeypatch, pairs)
    BC.render(model, K, T, fb)                                   # reuse: layer 0's raw comes from the cache, the chain evaluates it
    assert BC.stats(model)[0] == BC.PIECES and len(pairs) == BC.PIECES
    assert_pairs_equal(pairs, "background cache reuse frame")
    assert all(0 < skipped < tested for tested, skipped in grids.stats()["samples"].values())


# ---------------------------------------------------------------------------------------- 4. all-ones grids change no bit
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
@pytest.mark.parametrize("only_coarse", [False, True])
def test_all_ones_grids_with_samples_change_no_bit(precision, only_coarse):
    case = S.make_case(only_coarse=only_coarse)
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case, precision)
    plain = SE.gpu_render(model, case, rays)
    grids = attach(model, {i: (np.ones((8, 8, 8), bool),) + OC.layer_bounds(case, i) for i in (1, 2, 3)}, samples=True)
    culled = SE.gpu_render(model, case, rays)
    assert_same_bits(culled, plain, f"all-ones grids with samples=True, {precision}")
    st = grids.stats()
    per_pair = case["n1"] if only_coarse else 2 * case["n1"] + case["n2"]
    assert sorted(st["samples"]) == [1, 2, 3]
    for i, (tested, skipped) in st["samples"].items():
        assert skipped == 0 and tested == int(plain[f"mask{i}"].sum()) * per_pair == st["pairs"][i][0] * per_pair, (i, st)


# ---------------------------------------------------------------------------------------- 5. against the oracle
_ORACLE = {}


def run_sampled(name, case, grids_spec, monkeypatch, precision, rays=None):
    """A sample-culled render under ``assert_matches_oracle`` as it is.  only_coarse: every ray (the coarse depths are the fp32
    oracle's bits, so the GPU classifies every sample as the oracle does).  Two-stage: without the rays on which a gridded layer's
    fine point lies within eps of an interior cell face (tests/test_sample_cull_cpu.py measures eps and holds the 5 % condition)."""
    rays = S.case_rays(case) if rays is None else rays
    n = rays.shape[0]
    if name not in _ORACLE:
        ref32, ch32 = SC.oracle_render_sampled(case, grids_spec, grids_spec, rays, torch.float32, monkeypatch)
        ref64, ch64 = SC.oracle_render_sampled(case, grids_spec, grids_spec, rays, torch.float64, monkeypatch)
        SC.assert_sample_cull_bites(ch32, case, n, name)
        keep = np.ones(n, bool)
        if not case["only_coarse"]:
            gap, eps, excluded = SC.fine_point_gap_and_excluded(case, ch32, ch64, n)
            print(f"{name}: fp32 / fp64 fine points at most {gap:.3e} apart, eps {eps:.3e}, {int(excluded.sum())} of {n} rays left out")
            assert excluded.mean() <= 0.05, (name, int(excluded.sum()), n)
            keep = ~excluded
        _ORACLE[name] = (ref32, ref64, torch.from_numpy(keep))
    ref32, ref64, keep = _ORACLE[name]
    model = SE.make_model(case, precision)
    grids = attach(model, grids_spec, samples=True)
    got = SE.gpu_render(model, case, rays.cuda())
    rows = lambda d: {k: v[keep] for k, v in d.items()}
    SE.report(f"{name} {precision}", S.assert_matches_oracle(rows(got), rows(ref32), rows(ref64), case["only_coarse"], name))
    assert all(0 < skipped < tested for tested, skipped in grids.stats()["samples"].values())
    return got


PRECISIONS = ["bf16x3", "fp32"]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("grid,dilate", [("half_x", 0), ("ball", 1)])
def test_oracle_plain_retiming(monkeypatch, precision, grid, dilate):
    case = OC.plain_case()
    run_sampled(f"plain {grid} {dilate}", case, OC.manual_grids(case, grid, dilate), monkeypatch, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_oracle_only_coarse(monkeypatch, precision):
    case = OC.plain_case(only_coarse=True, near=4.0)
    got = run_sampled("only_coarse", case, OC.manual_grids(case, "half_x", 0), monkeypatch, precision)
    assert torch.equal(got["fine_mixed"], got["coarse_mixed"])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_oracle_full_edit_case(monkeypatch, precision):
    """Rotation, shift and scale, an instance with a manual grid on its own slot, the opacity table, scene passes."""
    case = S.make_case()
    run_sampled("full edits", case, OC.manual_grids(case, "half_x", 0), monkeypatch, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_oracle_sixty_four_plus_sixty_four_on_the_first_64_rays(monkeypatch, precision):
    case = OC.plain_case(n1=64, n2=64)
    run_sampled("64+64", case, SC.grids_64(case), monkeypatch, precision, rays=S.case_rays(case)[:64])


# ---------------------------------------------------------------------------------------- 7. nothing new without the flag
def test_a_render_without_the_sample_cull_launches_what_it_always_did():
    case = OC.plain_case()
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case)
    l = model.total_layers

    def records():
        ops.profile_begin()
        with torch.no_grad():
            model.render_rays_raw(rays, False, case["thr"], case["bthr"], ref_chunk=case["chunk"])
        torch.cuda.synchronize()
        return ops.profile_end()
    new = lambda recs: [r for r in recs if r["kernel"] == "occupancy_rows" or (r["kernel"] == "mlp_stage" and r["kind"] & 4)]
    model._workspace = None
    plain = records()
    parent_bytes = hip.lib().stnerf_render_workspace_bytes(S.CAP, l, case["n1"], case["n2"], 0)
    assert plain and not new(plain) and model._workspace.numel() == parent_bytes == 637256
    attach(model, OC.manual_grids(case, "half", 0))
    model._workspace = None
    culled = records()
    assert not new(culled) and model._workspace.numel() == parent_bytes
    attach(model, OC.manual_grids(case, "half_x", 0), samples=True)
    sampled = records()
    pieces = (S.N + S.CAP - 1) // S.CAP
    rows = [r for r in sampled if r["kernel"] == "occupancy_rows"]
    assert len(rows) == pieces * 3 * 2 and sorted({r["tag"] for r in rows}) == [1, 2, 3]
    assert sorted({r["ns"] for r in rows}) == [case["n1"], case["n1"] + case["n2"]]
    assert len([r for r in sampled if r["kernel"] == "mlp_stage"]) == len(new(sampled)) - len(rows) == 2 * pieces
    assert not [r for r in sampled if r["kernel"] == "motionnet"]                       # a listed layer's MotionNet runs fused
    assert model._workspace.numel() == ops.render_workspace_bytes(S.CAP, l, case["n1"], case["n2"], False, [False, True, True, True]) > parent_bytes


def test_render_rays_refuses_short_counter_buffers(monkeypatch):
    """The cull's counters are written at [layer][0..1]: a buffer that is not (l, 2) is refused before anything is launched."""
    case = OC.plain_case()
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case)
    grids = attach(model, OC.manual_grids(case, "half_x", 0), samples=True)
    l = model.total_layers
    monkeypatch.setattr(grids, "counts", lambda device: torch.zeros(l - 1, 2, dtype=torch.int32, device=device))
    with pytest.raises(ValueError, match="occupancy_counts"):
        SE.gpu_render(model, case, rays)
    monkeypatch.undo()
    monkeypatch.setattr(grids, "sample_counts", lambda device: torch.zeros(l - 1, 2, dtype=torch.int64, device=device))
    with pytest.raises(ValueError, match="sample_counts"):
        SE.gpu_render(model, case, rays)
