"""Early ray termination on the GPU (csrc/termination.hip: ray_stop_kernel; csrc/sample_rows.hip: sample_rows_kernel;
stnerf_render_rays_terminated; model.set_termination):
  1. stnerf_ray_stop against the numpy restatement of the rule, bit for bit, with canaries around t_stop;
  2. stnerf_visibility_rows against the numpy restatement, bit for bit, with every byte around it;
  3. the row-list stage kernels with LAYER 0 listed (ray_list == NULL) against the unlisted launch;
  4. the terminated pipeline against its definition, a chain of op-level entries, bit for bit;
  5. the no-op cases: no flag, a table of zeros, t_stop = +inf everywhere;
  6. terminated renders against the CPU oracle (``termination_common.oracle_render_terminated``) under ``assert_matches_oracle``
     as it is, with the two conditions of tests/test_termination_cpu.py asserted again.
Shapes: op-level launches of 1 .. 1030 rays, the 17 x 23 view with (12, 6) samples.  Needs an MI355X: `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

import occupancy_common as OC
import sample_cull_common as SC
import scene_edits_common as S
import termination_common as TC
import test_gpu_bkgd_cache as BC
import test_gpu_scene_edits_oracle as SE
import test_termination_cpu as CPU
from pipeline_chain import assert_pairs_equal, bits, detach_models, with_chain
from stnerf_amd import hip, ops, synthetic as syn
from test_gpu_occupancy import assert_same_bits, attach

pytestmark = pytest.mark.gpu

POISON = 0x7FC0BEEF      # a NaN pattern no kernel writes
INF = float("inf")


@pytest.fixture(autouse=True)
def detach():
    yield
    detach_models()


# ---------------------------------------------------------------------------------------- 1. the stop depth vs numpy
def special_rays(l, n1):
    """The hand-made rays of the issue, for any (l, n1): a list of (t [l][n1], wM [l][n1]) fp32 arrays."""
    f = np.float32
    out = []
    # equal depths across layers and within a layer (pairs of equal depths, the same in every layer); the weights put the stop
    # inside the ties at small tau
    t = np.tile((1.0 + (np.arange(n1) // 2)).astype(f), (l, 1))
    w = np.full((l, n1), 0.0, f)
    w[:, : max(1, n1 // 2)] = f(1.0 / (l * max(1, n1 // 2)))
    out.append((t, w))
    # a layer of all -1000 with zero weights (the last layer; for l = 1 the whole ray)
    t = np.tile(np.linspace(1, 3, n1).astype(f), (l, 1)) + np.arange(l, dtype=f)[:, None] * f(0.01)
    w = np.full((l, n1), f(0.9 / n1), f)
    t[l - 1], w[l - 1] = -1000.0, 0.0
    out.append((t, w))
    # never reaches any tau below 0.9: the weights sum to 0.05
    t = np.tile(np.linspace(1, 3, n1).astype(f), (l, 1)) + np.arange(l, dtype=f)[:, None] * f(0.01)
    out.append((t, np.full((l, n1), f(0.05 / (l * n1)), f)))
    # stopped at its LAST merged sample: everything on the deepest sample of the deepest layer
    w = np.zeros((l, n1), f)
    w[l - 1, n1 - 1] = 1.0
    out.append((t.copy(), w))
    # A rounds to exactly 1 after three samples (tau = 0 stops there): 0.5 + 0.25 + 0.25 on the first samples of the merge
    w = np.zeros((l, n1), f)
    firsts = [(0, 0), (1 % l, 0 if l > 1 else 1), (2 % l if l > 2 else 0, 0 if l > 2 else (1 if l > 1 else 2))]
    for (i, k), v in zip(firsts, (0.5, 0.25, 0.25)):
        w[i, k] = v
    out.append((t.copy(), w))
    # a NaN weight in the middle of the walk
    w = np.full((l, n1), f(0.01 / (l * n1)), f)
    w[l // 2, n1 // 2] = np.nan
    out.append((t.copy(), w))
    # the first merged sample already heavy: tau = 0.9 gives j* = 0
    w = np.zeros((l, n1), f)
    w[0, 0] = 0.2
    out.append((t.copy(), w))
    return out


def stop_inputs(n, l, n1, seed):
    rs = np.random.RandomState(seed)
    t = np.sort(rs.uniform(0.5, 6.0, (n, l, n1)).astype(np.float32), -1)
    w = ((rs.uniform(0, 1, (n, l, n1)) ** 8) * rs.uniform(0, 1.5, (n, 1, 1)) * (4.0 / (l * n1)) * 4).astype(np.float32)
    return t, w


@pytest.mark.parametrize("l,n1", [(1, 5), (3, 16), (9, 64)])
@pytest.mark.parametrize("n", [1, 67, 1030])
def test_ray_stop_equals_numpy(n, l, n1):
    special = special_rays(l, n1)
    batches = []
    if n == 1:
        batches = [(np.stack([t]), np.stack([w])) for t, w in special]            # one launch of one ray per hand-made ray
    else:
        t, w = stop_inputs(n, l, n1, 100 * l + n)
        for j, (ts, ws) in enumerate(special):
            t[3 * j + 1], w[3 * j + 1] = ts, ws
        batches = [(t, w)]
    seen_inf = seen_finite = 0
    for t, w in batches:
        t_dev, w_dev = torch.from_numpy(t).cuda(), torch.from_numpy(w).cuda()
        for tau in (0.0, 1e-4, 0.9):
            want = TC.np_ray_stop(t, w, tau)
            got = ops.ray_stop(t_dev, w_dev, tau)
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), (n, l, n1, tau)
            seen_inf, seen_finite = seen_inf + int(np.isinf(want).sum()), seen_finite + int(np.isfinite(want).sum())
        # canaries before and after t_stop
        buf = torch.full((t.shape[0] + 64,), POISON, dtype=torch.int32, device="cuda")
        hip.check(hip.lib().stnerf_ray_stop(hip.dptr(t_dev), hip.dptr(w_dev), t.shape[0], l, n1, 1e-4, C.c_void_p(buf.data_ptr() + 128), hip.stream_ptr()),
                  "stnerf_ray_stop")
        torch.cuda.synchronize()
        assert bool((buf[:32] == POISON).all()) and bool((buf[32 + t.shape[0]:] == POISON).all())
        assert np.array_equal(buf[32:32 + t.shape[0]].cpu().numpy(), TC.np_ray_stop(t, w, 1e-4).view(np.int32))
        assert torch.equal(bits(t_dev).cpu(), torch.from_numpy(t).view(torch.int32)) and torch.equal(bits(w_dev).cpu(), torch.from_numpy(w).view(torch.int32))
    assert seen_inf and seen_finite
    # the hand-made rays do what they were made for
    t, w = (np.stack(x) for x in zip(*special))
    s0, s4, s9 = TC.np_ray_stop(t, w, 0.0), TC.np_ray_stop(t, w, 1e-4), TC.np_ray_stop(t, w, 0.9)
    assert np.isinf(s4[2]) and np.isinf(s4[3]) and np.isinf(s0[3])                # never there; stopped at the last sample
    assert np.isfinite(s0[4]) and np.isfinite(s4[5]) and (l * n1 < 2 or np.isfinite(s9[6]))
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        ops.ray_stop(torch.zeros(1, l, n1, device="cuda"), torch.zeros(1, l, n1, device="cuda"), 1.0)
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        ops.ray_stop(torch.zeros(1, l, n1, device="cuda"), torch.zeros(1, l, n1, device="cuda"), -0.25)


# ---------------------------------------------------------------------------------------- 2. the rows kernel vs numpy
@pytest.mark.parametrize("ns", [1, 64, 65, 192, 256])
@pytest.mark.parametrize("n", [1, 17, 1030])
def test_visibility_rows_equal_numpy(n, ns):
    l = 3
    rs = np.random.RandomState(7 * n + ns)
    occ = OC.GRIDS["ball"](8)
    lo, hi = np.array([-1, -1, -1], np.float32), np.array([1, 1, 1], np.float32)
    g_np, g_dev = SC.grid_entry(occ, lo, hi), SC.device_entry(occ, lo, hi)
    start = rs.uniform(-1.3, 1.3, (n, l, 1, 3))
    step = rs.uniform(-1.5, 1.5, (n, l, 1, 3)) / ns
    xyz = (start + step * np.arange(ns).reshape(1, 1, ns, 1)).astype(np.float32)
    t = np.sort(rs.uniform(0.5, 6.0, (n, l, ns)).astype(np.float32), -1)
    stop = rs.uniform(0.0, 7.0, n).astype(np.float32)
    stop[rs.rand(n) < 0.2] = np.inf                                                # everything listed
    stop[0] = t[0, 1, ns // 2]                                                     # t == t_stop: listed
    if n > 3:
        stop[1], stop[2] = np.inf, t[2, 0, 0]
        t[3, :, ns - 1] = np.nan                                                   # a NaN depth: listed
        stop[3] = 0.0                                                              # ... where every real depth is hidden
    x_dev, t_dev, s_dev = torch.from_numpy(xyz).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(stop).cuda()
    perm = rs.permutation(n).astype(np.int32)
    some = perm[: max(1, (3 * n) // 4)]
    cap = n * ns                                                                   # a capacity of exactly n x ns
    combos = [(1, some, True, True), (1, some, True, False), (2, perm[:0], True, False), (0, np.arange(n, dtype=np.int32), False, False)]
    for layer, rays, give_list, gridded in combos:
        occupied = SC.np_listed(xyz[:, layer], g_np) if gridded else None
        want_rows, listed = TC.np_visibility_rows(t[:, layer], stop, rays, occupied)
        raw = torch.full((n, l, ns, 4), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        buf = torch.full((cap + 16,), POISON, dtype=torch.int32, device="cuda")
        count = torch.full((3,), POISON, dtype=torch.int32, device="cuda")
        counts = torch.zeros(l, 2, dtype=torch.int64, device="cuda")
        counts[(layer + 1) % l, 0], counts[layer, 0], counts[layer, 1] = 77, 5, 3    # accumulated into, the other rows untouched
        lst = cnt = None
        if give_list:
            lst = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            lst[:len(rays)] = torch.from_numpy(rays).cuda()
            cnt = torch.tensor([len(rays)], dtype=torch.int32, device="cuda")
        ops.visibility_rows(t_dev[:, layer], s_dev, raw[:, layer], xyz=x_dev[:, layer] if gridded else None, grid=g_dev if gridded else None,
                            layer=layer, ray_list=lst, ray_count=cnt, row_list=buf[:cap], row_count=count[1:2], counts=counts)
        torch.cuda.synchronize()
        got_n = int(count[1])
        got = buf[:got_n].cpu().numpy().astype(np.int64)
        assert got_n == len(want_rows) and np.array_equal(np.sort(got), want_rows), (n, ns, layer, gridded, got_n, len(want_rows))
        assert SC.rows_are_contiguous_and_ascending(got)
        assert int(count[0]) == POISON and int(count[2]) == POISON
        assert bool((buf[cap:] == POISON).all()) and bool((buf[got_n:cap] == POISON).all())
        want_raw = np.full((n, l, ns, 4), POISON, np.int32)
        tested = np.zeros(n, bool)
        tested[rays] = True
        want_raw[:, layer][tested[:, None] & ~listed] = 0
        assert np.array_equal(bits(raw).cpu().numpy(), want_raw)                   # zeros exactly there, every other byte kept
        tot = len(rays) * ns
        want_counts = [[0, 0] for _ in range(l)]
        want_counts[(layer + 1) % l][0] = 77
        want_counts[layer] = [5 + tot, 3 + tot - len(want_rows)]
        assert counts.cpu().tolist() == want_counts
    for a, b in ((x_dev, xyz), (t_dev, t), (s_dev, stop)):
        assert torch.equal(bits(a).cpu(), torch.from_numpy(b).view(torch.int32))
    if n == 17 and ns == 64:
        big = torch.zeros(4, 257, device="cuda")
        with pytest.raises(ValueError, match="1..256"):
            ops.visibility_rows(big, s_dev[:4], torch.zeros(4, 257, 4, device="cuda"))
        with pytest.raises(ValueError, match="capacity"):
            ops.visibility_rows(t_dev[:, 1], s_dev, raw[:, 1], row_list=buf[:cap - 1])
        with pytest.raises(ValueError, match="layer 0"):
            ops.visibility_rows(t_dev[:, 0], s_dev, raw[:, 0], xyz=x_dev[:, 0], grid=g_dev, layer=0)


# ---------------------------------------------------------------------------------------- 3. the row-list stage kernels, layer 0 listed
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_row_list_stage_kernels_with_the_background_listed(precision):
    """Layer 0 listed with ray_list == NULL next to a listed and an unlisted performer: every listed sample has the 16 bytes the
    unlisted launch stores, every other sample of a listed layer keeps the pattern that was there."""
    n, ns, l = 67, 20, 3
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

    def launch(rows):
        raw = torch.full((n, l, ns, 4), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        layers = []
        for i in (1, 2):
            layers.append(dict(space=sp[i - 1], motion=mo[i - 1], xyz=xyz[:, i], raw=raw[:, i], times=rays[:, 6 + i], ray_list=lst[i], ray_count=cnt[i:i + 1]))
        layers.append(dict(space=bk, motion=None, xyz=xyz[:, 0], raw=raw[:, 0], times=None, plain_time=True))
        for j, i in enumerate((1, 2, 0)):
            if i in rows:
                layers[j]["row_list"], layers[j]["row_count"] = rows[i]
        ops.mlp_stage(layers, rays[:, 3:6], ns, sigmoid_rgb=True)
        torch.cuda.synchronize()
        return bits(raw).cpu()

    hit = mask.bool()
    plain = launch({})
    poison = torch.full_like(plain, POISON)
    assert not bool((plain[:, 0] == POISON).all(-1).any())                          # the background runs on every ray
    listed = {0: torch.from_numpy(rs.rand(n, ns) < 0.5), 1: torch.from_numpy(rs.rand(n, ns) < 0.5) & hit[:, 1, None]}
    listed[0][5] = False                                                            # a ray without a row, a ray with all of them
    listed[0][6] = True
    rows = {}
    for i, m in listed.items():
        order = rs.permutation(n)                                                   # rays in any order, a ray's rows ascending in k
        words = np.concatenate([(r << 8) | np.nonzero(m[r].numpy())[0] for r in order]).astype(np.int32)
        assert len(words) == int(m.sum()) > 128
        buf = torch.full((n * ns,), -1, dtype=torch.int32, device="cuda")
        buf[:len(words)] = torch.from_numpy(words).cuda()
        rows[i] = (buf, torch.tensor([len(words)], dtype=torch.int32, device="cuda"))
    for pick in ((0,), (0, 1)):
        got = launch({i: rows[i] for i in pick})
        for i in range(l):
            if i in pick:
                assert torch.equal(got[:, i][listed[i]], plain[:, i][listed[i]]), (precision, pick, i)
                assert torch.equal(got[:, i][~listed[i]], poison[:, i][~listed[i]]), (precision, pick, i)
            else:
                assert torch.equal(got[:, i], plain[:, i]), (precision, pick, i)


# ---------------------------------------------------------------------------------------- 4. the pipeline equals its definition
TAU = 1e-3     # (a large tau, at which the dense synthetic background hides about a third of layer 1's fine samples and most of
               # layer 2's: tests/test_termination_cpu.py ``oracle_cases`` has the scene's story)


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
@pytest.mark.parametrize("background", [True, False])
def test_pipeline_equals_its_definition(monkeypatch, precision, background):
    """A grid (sample-culled) on layer 1 and none on the others; layers 1 and 2 terminated, layer 3 not; scene passes on."""
    case = OC.plain_case()
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case, precision)
    attach(model, OC.manual_grids(case, "half_x", 0, layers=(1,)), samples=True)
    model.set_termination(TAU, layers=[1, 2], background=background)
    flags = [background, True, True, False]
    assert model.termination.flags(model) == flags
    pairs = []
    with_chain(model, monkeypatch, pairs, flags, TAU)
    SE.gpu_render(model, case, rays)
    assert len(pairs) == (S.N + S.CAP - 1) // S.CAP
    assert_pairs_equal(pairs, f"{precision} background={background}")
    stops = torch.cat([p[1].stop for p in pairs]).cpu()
    assert bool(torch.isfinite(stops).any())
    rows = model.termination.stats()["rows"]
    assert sorted(rows) == ([0] if background else []) + [1, 2] and all(0 < skipped < tested for tested, skipped in rows.values()), rows
    assert rows[2][0] == int(sum(int(p[0][4][:, 2].sum()) for p in pairs)) * (case["n1"] + case["n2"])     # the fine samples of the hit rays
    if background:
        assert rows[0][0] == S.N * (case["n1"] + case["n2"])
    samples = model._occupancy.stats()["samples"]
    assert sorted(samples) == [1] and samples[1][0] * (case["n1"] + case["n2"]) == rows[1][0] * case["n1"]   # layer 1's coarse stage only


def test_pipeline_equals_its_definition_with_a_background_cache(monkeypatch):
    """CAPTURE then REUSE: the background is not terminated in either frame (its raw outputs are the unterminated render's, which
    the chain evaluates itself), the performers are.  This scene's fields are thin (on the CPU oracle no ray reaches a
    transmittance of 1e-2): tau = 0.6 hides 36 to 400 of a performer's ~1700 coarse samples in either frame."""
    tau = 0.6
    model = BC.make_model(2)
    K, T = syn.camera(BC.H, BC.W, 15.0)
    fa, fb = BC.fids(True, 2, (1.0, 1.0)), BC.fids(True, 2, (2.5, 3.0))
    model.set_termination(tau)
    assert model.termination.flags(model) == [True, True, True]
    pairs = []
    with_chain(model, monkeypatch, pairs, [False, True, True], tau)
    BC.render(model, K, T, fa)                                   # capture
    assert len(pairs) == BC.PIECES
    BC.render(model, K, T, fb)                                   # reuse
    assert BC.stats(model)[0] == BC.PIECES and len(pairs) == 2 * BC.PIECES
    assert_pairs_equal(pairs, "background cache capture + reuse frames")
    rows = model.termination.stats()["rows"]
    assert sorted(rows) == [1, 2] and all(0 < skipped < tested for tested, skipped in rows.values()), rows
    # without the cache the background is terminated too
    model.set_background_cache(None)
    pairs.clear()
    monkeypatch.undo()
    with_chain(model, monkeypatch, pairs, [True, True, True], tau)
    BC.render(model, K, T, fb)
    assert_pairs_equal(pairs, "the same frame without the cache")
    assert 0 in model.termination.stats()["rows"]


# ---------------------------------------------------------------------------------------- 5. the no-op cases
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_no_flag_changes_no_bit_and_launches_nothing_new(monkeypatch, precision):
    case = OC.plain_case()
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case, precision)
    l = model.total_layers

    def records():
        model._workspace = None
        ops.profile_begin()
        out = SE.gpu_render(model, case, rays)
        return out, ops.profile_end()
    new = lambda recs: [r for r in recs if r["kernel"] in ("ray_stop", "visibility_rows") or (r["kernel"] == "mlp_stage" and r["kind"] & 4)]
    plain, recs = records()
    parent_bytes = hip.lib().stnerf_render_workspace_bytes(S.CAP, l, case["n1"], case["n2"], 0)
    assert recs and not new(recs) and model._workspace.numel() == parent_bytes
    names = [r["kernel"] for r in recs]
    # a table of zeros through stnerf_render_rays_terminated (tau is not even looked at)
    real = ops.render_rays
    calls = []

    def zero_flags(*a, **kw):
        calls.append(1)
        return real(*a, terminate=[False] * l, tau=0.5, **kw)
    monkeypatch.setattr(ops, "render_rays", zero_flags)
    zeros, recs0 = records()
    monkeypatch.undo()
    assert calls and [r["kernel"] for r in recs0] == names and not new(recs0) and model._workspace.numel() == parent_bytes
    assert_same_bits(zeros, plain, "a flag table of zeros")
    assert ops.render_workspace_bytes(S.CAP, l, case["n1"], case["n2"], False, terminate=[False] * l) == parent_bytes
    # termination attached with no layer and no background: no flag
    model.set_termination(TAU, layers=[], background=False)
    none, recs1 = records()
    assert [r["kernel"] for r in recs1] == names and model._workspace.numel() == parent_bytes
    assert_same_bits(none, plain, "termination of no layer")
    # only_coarse: nothing to terminate
    model.set_termination(TAU)
    oc = dict(case, only_coarse=True)
    model.replay.pop("u", None)
    with_t = SE.gpu_render(model, oc, rays)
    model.set_termination(None)
    assert_same_bits(with_t, SE.gpu_render(model, oc, rays), "only_coarse")
    # and with flags the new launches are there: one ray_stop per piece, one visibility_rows per terminated layer and piece
    model = SE.make_model(case, precision)
    model.set_termination(TAU)
    _, recs2 = records()
    pieces = (S.N + S.CAP - 1) // S.CAP
    assert len([r for r in recs2 if r["kernel"] == "ray_stop"]) == pieces
    vis = [r for r in recs2 if r["kernel"] == "visibility_rows"]
    assert len(vis) == pieces * l and sorted({r["tag"] for r in vis}) == list(range(l)) and {r["ns"] for r in vis} == {case["n1"] + case["n2"]}
    assert len([r for r in recs2 if r["kernel"] == "mlp_stage" and r["kind"] & 4]) == pieces       # the fine stage alone walks lists
    assert model._workspace.numel() == ops.render_workspace_bytes(S.CAP, l, case["n1"], case["n2"], False, terminate=[True] * l) > parent_bytes


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_an_infinite_stop_depth_changes_no_bit(monkeypatch, precision):
    """t_stop = +inf everywhere, through ``ops.visibility_rows`` and the row-list fine stage: the un-terminated render's bits."""
    case = OC.plain_case()
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case, precision)
    l = model.total_layers
    pairs = []
    with_chain(model, monkeypatch, pairs, [True] * l, TAU, t_stop=INF, via_rows=True)
    SE.gpu_render(model, case, rays)                             # (no termination attached: the un-terminated pipeline)
    assert_pairs_equal(pairs, f"t_stop = +inf, {precision}")


# ---------------------------------------------------------------------------------------- 6. against the oracle
_ORACLE = {}


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
@pytest.mark.parametrize("name", ["all layers, tau 5e-3", "performers 1 and 3, tau 3e-3"])
def test_oracle(monkeypatch, name, precision):
    """A terminated render under ``assert_matches_oracle`` as it is, without the rays on which the fp32 and the fp64 evaluation may
    classify a sample differently (``termination_common.excluded_rays``); the two conditions hold (asserted again)."""
    case, tau, flags = CPU.oracle_cases()[name]
    rays = S.case_rays(case)
    n = rays.shape[0]
    if name not in _ORACLE:
        ref32, i32 = TC.oracle_render_terminated(case, rays, torch.float32, tau, flags, monkeypatch)
        ref64, i64 = TC.oracle_render_terminated(case, rays, torch.float64, tau, flags, monkeypatch)
        excluded = TC.excluded_rays(i32, i64, flags)
        counts = TC.assert_termination_bites(i32, flags, ~excluded, name)
        print(f"{name}: {int(excluded.sum())} of {n} rays left out; rays with listed and hidden samples per terminated layer {counts}")
        assert excluded.mean() <= 0.05, (name, int(excluded.sum()), n)
        _ORACLE[name] = (ref32, ref64, torch.from_numpy(~excluded))
    ref32, ref64, keep = _ORACLE[name]
    model = SE.make_model(case, precision)
    model.set_termination(tau, layers=[i for i in range(1, len(flags)) if flags[i]], background=flags[0])
    assert model.termination.flags(model) == flags
    got = SE.gpu_render(model, case, rays.cuda())
    rows = lambda d: {k: v[keep] for k, v in d.items()}
    SE.report(f"{name} {precision}", S.assert_matches_oracle(rows(got), rows(ref32), rows(ref64), False, name))
    st = model.termination.stats()["rows"]
    assert sorted(st) == [i for i, f in enumerate(flags) if f] and all(0 < skipped < tested for tested, skipped in st.values()), st
