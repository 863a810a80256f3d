"""The background's occupancy grid on the GPU (csrc/sample_rows.hip: sample_rows_kernel;
stnerf_render_rays_background; OccupancyGrids(background=True) / set_background_manual):
  1. the rows kernel against the numpy restatement of the rule, bit for bit, with every byte around it and every EINVAL;
  2. the row-list stage kernels with layer 0 listed at ns = n1 (the coarse shape) against the unlisted launch, both arithmetics;
  3. the pipeline against its definition, a chain of op-level entries that zeroes raw[:, 0] in torch, bit for bit;
  4. the no-ops: an all-ones grid changes no bit, no grid launches what stnerf_render_rays_terminated launched in its workspace;
  5. renders under a background grid against the CPU oracle (``background_grid_common.oracle_render_background``) under
     ``assert_matches_oracle`` as it is, the two conditions of tests/test_background_grid_cpu.py asserted again.
Shapes: op-level launches of 1 / 17 / 70 rays, the 17 x 23 view with (12, 6) samples.  Needs an MI355X: `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

import background_grid_common as BG
import occupancy_common as OC
import sample_cull_common as SC
import scene_edits_common as S
import test_background_grid_cpu as CPU
import test_gpu_bkgd_cache as BC
import test_gpu_scene_edits_oracle as SE
from pipeline_chain import assert_pairs_equal, bits, detach_models, with_chain
from stnerf_amd import hip, ops, synthetic as syn
from stnerf_amd.occupancy import OccupancyGrids
from test_gpu_occupancy import assert_same_bits

pytestmark = pytest.mark.gpu

POISON = 0x7FC0BEEF      # a NaN pattern no kernel writes
TAU = 1e-3               # (tests/test_gpu_termination.py: at this tau the dense synthetic background hides a good part of the fine samples)


@pytest.fixture(autouse=True)
def detach():
    yield
    detach_models()


# ---------------------------------------------------------------------------------------- 1. the rows kernel vs numpy
def _occupied(name):
    rs = np.random.RandomState(len(name))
    if name == "5x3x4":
        return rs.rand(4, 3, 5) < 0.5                     # [Rz][Ry][Rx] of res (5, 3, 4): 60 cells, two words
    if name == "33x1x2":
        return rs.rand(2, 1, 33) < 0.5                    # rows of 33 cells: the word boundary falls inside the second row
    return np.ones((4, 3, 5), bool) if name == "ones" else np.zeros((4, 3, 5), bool)


@pytest.mark.parametrize("ns", [3, 64, 96, 256])
@pytest.mark.parametrize("grid", ["5x3x4", "33x1x2", "ones", "zeros"])
def test_rows_kernel_equals_numpy(ns, grid):
    occ = _occupied(grid)
    res = (occ.shape[2], occ.shape[1], occ.shape[0])
    lo, hi = np.array([-1, -1, -1], np.float32), np.array([1, 1, 1], np.float32)     # z cells of 0.5 (res 4) / 1.0 (res 2): exact faces
    g_np, g_dev = SC.grid_entry(occ, lo, hi), SC.device_entry(occ, lo, hi)
    l = 2
    for n in (1, 17, 70):
        rs = np.random.RandomState(1000 * n + ns)
        start = rs.uniform(-1.3, 1.3, (n, l, 1, 3))
        step = rs.uniform(-1.5, 1.5, (n, l, 1, 3)) / ns
        xyz = (start + step * np.arange(ns).reshape(1, 1, ns, 1)).astype(np.float32)
        xyz[0, 0, 0] = np.array([0.25, 0.3, 0.0], np.float32)                         # exactly on a z face (z = 0 in every grid here)
        xyz[0, 0, 1] = np.array([1.5, -1.001, 1e30], np.float32)                      # outside the bounds: clamped
        xyz[0, 0, 2] = np.array([0.1, np.nan, 0.2], np.float32)                       # a NaN coordinate: listed
        xyz[n - 1, 0, ns - 1] = np.array([-1.0, -1.0, -1.0], np.float32)              # the low corner: cell (0, 0, 0)
        t = np.sort(rs.uniform(0.5, 6.0, (n, l, ns)).astype(np.float32), -1)
        stop = rs.uniform(0.0, 7.0, n).astype(np.float32)
        stop[rs.rand(n) < 0.2] = np.inf
        stop[0] = t[0, 0, ns // 2]                                                    # a tie t == t_stop: listed
        if n > 3:
            stop[1], stop[2] = np.inf, 0.0
            t[2, 0, ns - 1] = np.nan                                                  # a NaN depth where every real one is hidden: listed
        x_dev, t_dev, s_dev = torch.from_numpy(xyz).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(stop).cuda()
        cap = n * ns                                                                  # a capacity of exactly n x ns
        for stopped in (False, True):
            want_rows, listed = BG.np_background_rows(xyz[:, 0], g_np, t[:, 0] if stopped else None, stop if stopped else None)
            if grid in ("5x3x4", "33x1x2") and n > 1 and ns > 3:
                assert 0 < listed.sum() < n * ns
            raw = torch.full((n, l, ns, 4), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
            buf = torch.full((cap + 16,), POISON, dtype=torch.int32, device="cuda")
            count = torch.full((3,), POISON, dtype=torch.int32, device="cuda")
            counts = torch.tensor([5, 3, 77], dtype=torch.int64, device="cuda")       # accumulated onto non-zero values; a canary behind
            ops.background_rows(x_dev[:, 0], raw[:, 0], g_dev, t=t_dev[:, 0] if stopped else None, t_stop=s_dev if stopped else None,
                                row_list=buf[:cap], row_count=count[1:2], counts=counts[:2])
            torch.cuda.synchronize()
            got_n = int(count[1])
            got = buf[:got_n].cpu().numpy().astype(np.int64)
            what = (grid, n, ns, stopped, got_n, len(want_rows))
            assert got_n == len(want_rows) and np.array_equal(np.sort(got), want_rows), what
            assert SC.rows_are_contiguous_and_ascending(got), what
            assert int(count[0]) == POISON and int(count[2]) == POISON, what
            assert bool((buf[cap:] == POISON).all()) and bool((buf[got_n:cap] == POISON).all()), what       # canaries, no word past the count
            want_raw = np.full((n, l, ns, 4), POISON, np.int32)
            want_raw[:, 0][~listed] = 0
            assert np.array_equal(bits(raw).cpu().numpy(), want_raw), what            # zeros exactly there, every other byte kept
            assert counts.cpu().tolist() == [5 + n * ns, 3 + n * ns - len(want_rows), 77], what
        for a, b in ((x_dev, xyz), (t_dev, t), (s_dev, stop)):
            assert torch.equal(bits(a).cpu(), torch.from_numpy(b).view(torch.int32))
    if grid == "5x3x4" and ns == 64:
        _every_einval(g_dev)


def _every_einval(g_dev):
    """Every refusal of stnerf_background_rows, on real device buffers, before any launch."""
    n, ns = 4, 8
    xyz = torch.zeros(n, ns, 3, device="cuda")
    raw = torch.full((n, ns, 4), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    t, stop = torch.ones(n, ns, device="cuda"), torch.ones(n, device="cuda")
    rl, rc = torch.full((n * ns,), POISON, dtype=torch.int32, device="cuda"), torch.full((1,), POISON, dtype=torch.int32, device="cuda")
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="1..256"):
        ops.background_rows(torch.zeros(2, 257, 3, device="cuda"), torch.zeros(2, 257, 4, device="cuda"), g_dev)
    with pytest.raises(ValueError, match="capacity"):
        ops.background_rows(xyz, raw, g_dev, row_list=rl[:n * ns - 1])
    with pytest.raises(ValueError, match="t_stop without"):
        ops.background_rows(xyz, raw, g_dev, t_stop=stop)
    with pytest.raises(ValueError, match="grid"):
        ops.background_rows(xyz, raw, None)
    b, res, lo, inv = g_dev
    for bad in ((b, (0, 3, 4), lo, inv), (b, (5, 3, 257), lo, inv), (b, res, lo, [2.5, float("nan"), 2.0]), (b, res, lo, [2.5, -1.0, 2.0]),
                (b, res, [float("inf"), -1.0, -1.0], inv)):
        with pytest.raises(ValueError):
            ops.background_rows(xyz, raw, bad)

    def call(n_=n, ns_=ns, grid=g_dev, raw_ptr=None, raw_stride=ns * 4, counts_ptr=0, cap=n * ns):
        entry = ops._occupancy_table([grid], 1)
        return hip.lib().stnerf_background_rows(n_, hip.dptr(xyz), ns * 3, ns_, entry, hip.dptr(t), ns, hip.dptr(stop),
                                                C.c_void_p(raw.data_ptr() if raw_ptr is None else raw_ptr), raw_stride, hip.dptr(rl, torch.int32),
                                                cap, hip.dptr(rc, torch.int32), C.c_void_p(counts_ptr), hip.stream_ptr())
    assert call(ns_=0) == hip.EINVAL and call(n_=(1 << 23) + 1, cap=1 << 40) == hip.EINVAL
    assert call(raw_ptr=raw.data_ptr() + 4) == hip.EINVAL and call(raw_stride=ns * 4 + 2) == hip.EINVAL
    assert call(counts_ptr=counts.data_ptr() + 4) == hip.EINVAL
    entry = (hip.Occupancy * 1)()                                                     # a grid without bits
    assert hip.lib().stnerf_background_rows(n, hip.dptr(xyz), ns * 3, ns, entry, None, 0, None, hip.dptr(raw), ns * 4, hip.dptr(rl, torch.int32),
                                            n * ns, hip.dptr(rc, torch.int32), None, hip.stream_ptr()) == hip.EINVAL
    torch.cuda.synchronize()
    assert bool((bits(raw) == POISON).all()) and bool((rl == POISON).all()) and int(rc[0]) == POISON and not bool(counts.any())
    assert call(counts_ptr=counts.data_ptr()) == hip.OK                               # ... and the same call with everything in order


# ---------------------------------------------------------------------------------------- 2. the row-list stage kernels, layer 0 at ns = n1
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_row_list_stage_kernels_with_the_background_listed_in_the_coarse_shape(precision):
    """Layer 0 listed with ray_list == NULL at ns = n1 = 12, by the rows kernel itself, next to two unlisted performers: every listed
    sample has the 16 bytes the unlisted launch stores, every other background sample the rows kernel's zeros (over the poison
    that was there), the performers the unlisted launch's bytes."""
    n, ns, l = 70, 12, 3
    torch.manual_seed(7)
    rs = np.random.RandomState(77)
    sd_b = syn.spacenet_state("net", rs, False)
    sd_p = [syn.spacenet_state("net", rs, True) for _ in range(l - 1)]
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
    occ = SC.checker_xz((4, 4, 4), 1)
    lo, hi = np.float32([-2.5, -2.5, -2.5]), np.float32([2.5, 2.5, 2.5])
    g_np, g_dev = SC.grid_entry(occ, lo, hi), SC.device_entry(occ, lo, hi)

    def launch(listed_background):
        raw = torch.full((n, l, ns, 4), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        layers = []
        for i in (1, 2):
            layers.append(dict(space=sp[i - 1], motion=mo[i - 1], xyz=xyz[:, i], raw=raw[:, i], times=rays[:, 6 + i], ray_list=lst[i], ray_count=cnt[i:i + 1]))
        layers.append(dict(space=bk, motion=None, xyz=xyz[:, 0], raw=raw[:, 0], times=None, plain_time=True))
        if listed_background:
            layers[2]["row_list"], layers[2]["row_count"] = ops.background_rows(xyz[:, 0], raw[:, 0], g_dev)
        ops.mlp_stage(layers, rays[:, 3:6], ns, sigmoid_rgb=True)
        torch.cuda.synchronize()
        return bits(raw).cpu()

    plain, got = launch(False), launch(True)
    assert not bool((plain[:, 0] == POISON).all(-1).any())                            # the background runs on every ray
    _, listed = BG.np_background_rows(xyz[:, 0].cpu().numpy(), g_np)
    listed = torch.from_numpy(listed)
    assert 100 < int(listed.sum()) < n * ns - 100 and bool((listed.any(-1) & ~listed.all(-1)).sum() >= 8)
    assert torch.equal(got[:, 0][listed], plain[:, 0][listed]), precision
    assert not bool(got[:, 0][~listed].any()), precision
    assert torch.equal(got[:, 1:], plain[:, 1:]), precision


# ---------------------------------------------------------------------------------------- 3. the pipeline equals its definition
def _attach(model, case, performers=(), **kw):
    """The res-4 x-z checkerboard on the background; ``performers``: those layers get the half_x grid (ray cull; samples=True: both)."""
    grids = OccupancyGrids(auto=False, **kw)
    occ, lo, hi = BG.checker_grid(case, (4, 4, 4))
    grids.set_background_manual(torch.from_numpy(np.ascontiguousarray(occ)), lo, hi)
    for i, (o, plo, phi) in OC.manual_grids(case, "half_x", 0, layers=performers).items():
        grids.set_manual(i, torch.from_numpy(np.ascontiguousarray(o)), plo, phi)
    model.set_occupancy(grids)
    return grids


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("variant", ["grid alone", "with a sample-culled performer and termination", "only_coarse"])
def test_pipeline_equals_its_definition(monkeypatch, precision, variant):
    """Scene passes on in every variant (the chain compares the sixth output too)."""
    only_coarse = variant == "only_coarse"
    case = OC.plain_case(only_coarse=only_coarse)
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case, precision)
    l, per_ray = model.total_layers, case["n1"] if only_coarse else 2 * case["n1"] + case["n2"]
    flags = [False] * l
    if variant.startswith("with"):
        grids = _attach(model, case, performers=(1,), samples=True)
        model.set_termination(TAU, layers=[2], background=True)
        flags = [True, False, True, False]
        assert model.termination.flags(model) == flags
    else:
        grids = _attach(model, case)
    pairs = []
    with_chain(model, monkeypatch, pairs, flags, TAU)
    SE.gpu_render(model, case, rays)
    assert len(pairs) == (S.N + S.CAP - 1) // S.CAP and all(chain.launch.get("background_id") is not None for _, chain in pairs)
    assert_pairs_equal(pairs, f"{variant} {precision}")
    st = grids.stats()
    tested, skipped = st["background"]
    if variant.startswith("with"):
        # the fine stage's rows launch tested the background too, with the hidden samples among the not listed; termination's own
        # counters saw no background launch (stnerf_visibility_rows is replaced)
        assert tested == S.N * per_ray and 0 < skipped < tested and sorted(st["samples"]) == [1]
        assert sorted(model.termination.stats()["rows"]) == [2]
    else:
        assert tested == S.N * per_ray and 0 < skipped < tested and st["samples"] == {} and st["pairs"] == {}


def test_background_cache_capture_then_reuse_equal_the_uncached_culled_frame_and_a_changed_grid_misses():
    model = BC.make_model(2)
    K, T = syn.camera(BC.H, BC.W, 15.0)
    fa, fb = BC.fids(True, 2, (1.0, 1.0)), BC.fids(True, 2, (2.5, 3.0))
    plain_b = BC.uncached(model, K, T, fb)
    grids = OccupancyGrids(auto=False)
    lo, hi = OC.np_bounds(model.bkgd_bbox)
    board = SC.checker_xz((4, 4, 4), 1)
    grids.set_background_manual(torch.from_numpy(board), lo, hi)
    model.set_occupancy(grids)
    want_a, want_b = BC.uncached(model, K, T, fa), BC.uncached(model, K, T, fb)
    assert any(not torch.equal(bits(x), bits(y)) for x, y in zip(want_b[:4], plain_b[:4]))           # the grid bites
    grids.reset_stats()
    BC.assert_bit_equal(BC.render(model, K, T, fa), want_a, "capture frame")
    assert BC.stats(model)[:3] == (0, BC.PIECES, BC.PIECES)
    captured = grids.stats()["background"]
    assert captured[0] == BC.H * BC.W * (2 * 12 + 6) and 0 < captured[1] < captured[0]
    got_b, recs = BC.render(model, K, T, fb, profile=True)
    BC.assert_bit_equal(got_b, want_b, "reuse frame")
    assert BC.stats(model)[0] == BC.PIECES
    assert not [r for r in recs if r["kernel"] == "background_rows"] and grids.stats()["background"] == captured   # layer 0 is in no stage
    # a changed grid misses: the other colour of the board
    grids.set_background_manual(torch.from_numpy(~board), lo, hi)
    want_c = BC.uncached(model, K, T, fb)
    hits = BC.stats(model)[0]
    BC.assert_bit_equal(BC.render(model, K, T, fb), want_c, "the other grid")
    assert BC.stats(model)[0] == hits and BC.stats(model)[1] == 2 * BC.PIECES
    assert any(not torch.equal(bits(x), bits(y)) for x, y in zip(want_c[:4], want_b[:4]))
    # ... and a render without the grid is not served the culled outputs
    model.set_occupancy(None)
    BC.assert_bit_equal(BC.render(model, K, T, fb), plain_b, "no grid")
    assert BC.stats(model)[0] == hits


# ---------------------------------------------------------------------------------------- 4. the no-ops
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
@pytest.mark.parametrize("only_coarse", [False, True])
def test_an_all_ones_grid_changes_no_bit(precision, only_coarse):
    case = S.make_case(only_coarse=only_coarse)
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case, precision)
    plain = SE.gpu_render(model, case, rays)
    lo, hi = BG.bkgd_bounds(case)
    grids = BG.attach_background(model, (np.ones((3, 5, 7), bool), lo, hi))
    culled = SE.gpu_render(model, case, rays)
    assert_same_bits(culled, plain, f"an all-ones background grid, {precision}")
    per_ray = case["n1"] if only_coarse else 2 * case["n1"] + case["n2"]
    assert grids.stats()["background"] == (S.N * per_ray, 0)


def test_no_grid_launches_what_the_terminated_entry_launched_in_its_workspace(monkeypatch):
    case = OC.plain_case()
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case)
    l = model.total_layers
    term = [True] * l

    def records():
        model._workspace = None
        ops.profile_begin()
        out = SE.gpu_render(model, case, rays)
        return out, [(r["kernel"], r["kind"], r["ns"], r["tag"], r["n_rays"]) for r in ops.profile_end()]
    model.set_termination(TAU)
    plain, names = records()                                     # through stnerf_render_rays_terminated
    parent_bytes = hip.lib().stnerf_render_workspace_bytes_terminated(S.CAP, l, case["n1"], case["n2"], 0, None, (C.c_int32 * l)(*[1] * l))
    assert names and model._workspace.numel() == parent_bytes and not [r for r in names if r[0] == "background_rows"]
    # the new entry with a grid WITHOUT bits: the same launch list, the same workspace, the same bits
    real, calls = ops.render_rays, []

    def no_bits(*a, **kw):
        calls.append(1)
        return real(*a, background_grid=(None, (1, 1, 1), [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]), **kw)
    monkeypatch.setattr(ops, "render_rays", no_bits)
    same, names0 = records()
    monkeypatch.undo()
    assert calls and names0 == names and model._workspace.numel() == parent_bytes
    assert_same_bits(same, plain, "stnerf_render_rays_background without a grid")
    assert ops.render_workspace_bytes(S.CAP, l, case["n1"], case["n2"], False, terminate=term) == parent_bytes
    assert hip.lib().stnerf_render_workspace_bytes_background(S.CAP, l, case["n1"], case["n2"], 0, None, (C.c_int32 * l)(*[1] * l), 0) == parent_bytes
    # with a grid the new launches are there: two per piece, tagged layer 0, and layer 0's visibility_rows launch is gone
    _attach(model, case)
    _, names1 = records()
    pieces = (S.N + S.CAP - 1) // S.CAP
    rows = [r for r in names1 if r[0] == "background_rows"]
    assert len(rows) == 2 * pieces and {r[3] for r in rows} == {0} and sorted({(r[1], r[2]) for r in rows}) == [(0, case["n1"]), (1, case["n1"] + case["n2"])]
    assert sorted({r[3] for r in names1 if r[0] == "visibility_rows"}) == list(range(1, l))
    assert model._workspace.numel() == ops.render_workspace_bytes(S.CAP, l, case["n1"], case["n2"], False, terminate=term, background=True) == parent_bytes
    # precision 2 (one launch per network) is refused
    model.set_termination(None)
    model.set_precision("fp32")
    model.mlp_schedule = "per_net"
    with pytest.raises(ValueError, match="per_net"):
        SE.gpu_render(model, case, rays)
    model.mlp_schedule = "stage"


# ---------------------------------------------------------------------------------------- 5. against the oracle
_ORACLE = {}


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
@pytest.mark.parametrize("name", ["plain", "full edits", "only_coarse"])
def test_oracle(monkeypatch, name, precision):
    """A render under the background's grid under ``assert_matches_oracle`` as it is, without the rays on which a background point
    of the fp32 or the fp64 oracle lies within eps = 5.5e-5 of an interior cell face; the two conditions hold (asserted again).
    Found on the CPU oracle with the res-4 x-z checkerboard, the first grid tried: 2 of 391 rays left out, 389 rays with both listed
    and skipped background samples in either stage."""
    case, grid = CPU.oracle_cases()[name]
    rays = S.case_rays(case)
    n = rays.shape[0]
    if name not in _ORACLE:
        ref32, st32 = BG.oracle_render_background(case, grid, rays, torch.float32, monkeypatch)
        ref64, st64 = BG.oracle_render_background(case, grid, rays, torch.float64, monkeypatch)
        excluded, counts = BG.assert_conditions(case, st32, grid, name)              # the two conditions, on the oracle alone
        both = excluded | BG.excluded_rays(st64, grid)
        print(f"{name}: {int(both.sum())} of {n} rays left out ({int(excluded.sum())} by the fp32 oracle's points); rays with listed and "
              f"skipped background samples per stage {counts}")
        assert both.mean() <= 0.05, (name, int(both.sum()), n)
        assert min(BG.rays_with_listed_and_skipped(st32, ~both).values()) >= 8
        _ORACLE[name] = (ref32, ref64, torch.from_numpy(~both))
    ref32, ref64, keep = _ORACLE[name]
    model = SE.make_model(case, precision)
    grids = BG.attach_background(model, grid)
    got = SE.gpu_render(model, case, rays.cuda())
    rows = lambda d: {k: v[keep] for k, v in d.items()}
    SE.report(f"{name} {precision}", S.assert_matches_oracle(rows(got), rows(ref32), rows(ref64), case["only_coarse"], name))
    tested, skipped = grids.stats()["background"]
    assert tested == n * (case["n1"] if case["only_coarse"] else 2 * case["n1"] + case["n2"]) and 0 < skipped < tested
