"""The per-ray background mask on the GPU (include/stnerf.h: "Per-ray background mask"; csrc/sample_rows.hip:
sample_rows_kernel; stnerf_render_options.bkgd_rays; ``ReprojectSpec(exclusive=True)``):
  1. the rows kernel against the numpy restatement (tests/background_rays_common.py), bit for bit, with every zero, every byte
     around the outputs and the counters;
  2. the pipeline: all flags on changes no bit; a mixed mask is, row by row, ``where(flag, the plain call, the call under an
     all-empty background grid)``; with a real grid and termination of layer 0 -- and with only_coarse -- it is the chain of op-level
     entries that zeroes raw[:, 0] in torch (the method of tests/test_gpu_background_grid.py);
  3. the model: launch pieces, and the background cache left alone;
  4. reprojection with ``exclusive=True`` against the calls made by hand.
Shapes: op-level launches of 1 .. 197 rays and one of 16 x 4 x 2048 + 5 rays at ns = 3 (a wave's second run); the 128-ray piece of
tests/test_gpu_render_entries.py; the 17 x 23 view and dense-background model of tests/test_gpu_reproject.py.
Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import background_grid_common as BG
import background_rays_common as BR
import occluder_common as OCL
import occupancy_common as OC
import sample_cull_common as SC
import scene_edits_common as S
import test_gpu_background_grid as BGT
import test_gpu_render_entries as RE
import test_gpu_reproject as GR
import test_gpu_scene_edits_oracle as SE
from pipeline_chain import assert_pairs_equal, bits, detach_models, with_chain
from stnerf_amd import BackgroundCache, ops, parallel, synthetic as syn
from stnerf_amd import reproject as rp
from stnerf_amd.bkgd_cache import view_key
from test_gpu_reproject import dense_model, model  # noqa: F401  (fixtures: the dense-background model, restored after each test)

pytestmark = pytest.mark.gpu

POISON = BGT.POISON
TAU = BGT.TAU


@pytest.fixture(autouse=True)
def detach():
    yield
    detach_models()


# ---------------------------------------------------------------------------------------- 1. the rows kernel vs numpy
def _kernel_case(n, ns):
    """Points, depths, stop depths and a half-occupied grid for a launch of n rays x ns samples (layer 0 of l = 2)."""
    rs = np.random.RandomState(1000 * (n % 1009) + ns)
    occ = np.random.RandomState(5).rand(4, 3, 5) < 0.5                               # [Rz][Ry][Rx] of res (5, 3, 4): 60 cells, two words
    lo, hi = np.array([-1, -1, -1], np.float32), np.array([1, 1, 1], np.float32)
    l = 2
    start = rs.uniform(-1.3, 1.3, (n, l, 1, 3))
    step = rs.uniform(-1.5, 1.5, (n, l, 1, 3)) / ns
    xyz = (start + step * np.arange(ns).reshape(1, 1, ns, 1)).astype(np.float32)
    xyz[0, 0, 0] = np.array([0.1, np.nan, 0.2], np.float32)                           # a NaN coordinate: occupied
    xyz[n - 1, 0, ns - 1] = np.array([1.5, -1.001, 1e30], np.float32)                 # outside the bounds: clamped
    t = np.sort(rs.uniform(0.5, 6.0, (n, l, ns)).astype(np.float32), -1)
    stop = rs.uniform(0.0, 7.0, n).astype(np.float32)
    stop[rs.rand(n) < 0.2] = np.inf
    stop[0] = t[0, 0, ns // 2]                                                        # a tie t == t_stop: listed
    if n > 3:
        stop[2] = 0.0
        t[2, 0, ns - 1] = np.nan                                                      # a NaN depth where every real one is hidden: listed
    return xyz, t, stop, SC.grid_entry(occ, lo, hi), SC.device_entry(occ, lo, hi)


def _check_launches(n, ns):
    xyz, t, stop, g_np, g_dev = _kernel_case(n, ns)
    x_dev, t_dev, s_dev = torch.from_numpy(xyz).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(stop).cuda()
    l, cap = xyz.shape[1], n * ns                                                     # a capacity of exactly n x ns
    for pattern in BR.FLAG_PATTERNS:
        flags = BR.flag_pattern(pattern, n)
        f_dev = torch.from_numpy(flags).cuda()
        for gridded in (False, True):
            for stopped in (False, True):
                what = (n, ns, pattern, gridded, stopped)
                want_rows, listed = BR.np_background_ray_rows(flags, ns, xyz[:, 0], g_np if gridded else None, t[:, 0] if stopped else None,
                                                              stop if stopped else None)
                raw = torch.full((n, l, ns, 4), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
                buf = torch.full((cap + 16,), POISON, dtype=torch.int32, device="cuda")
                count = torch.full((3,), POISON, dtype=torch.int32, device="cuda")
                counts = torch.tensor([5, 3, 77], dtype=torch.int64, device="cuda")   # accumulated onto non-zero values; a canary behind
                ops.background_ray_rows(x_dev[:, 0], raw[:, 0], f_dev, grid=g_dev if gridded else None, t=t_dev[:, 0] if stopped else None,
                                        t_stop=s_dev if stopped else None, row_list=buf[:cap], row_count=count[1:2], counts=counts[:2])
                torch.cuda.synchronize()
                got_n = int(count[1])
                got = buf[:got_n].cpu().numpy().astype(np.int64)
                assert got_n == len(want_rows) and np.array_equal(np.sort(got), want_rows), what + (got_n, len(want_rows))
                assert BR.rows_per_ray_are_contiguous_and_ascending(got), what        # per ray: the order of the runs is free
                assert int(count[0]) == POISON and int(count[2]) == POISON, what
                assert bool((buf[got_n:] == POISON).all()), what                      # no word past the count, none past the capacity
                want_raw = np.full((n, l, ns, 4), POISON, np.int32)
                want_raw[:, 0][~listed] = 0
                assert np.array_equal(bits(raw).cpu().numpy(), want_raw), what        # zeros exactly there, every other byte kept
                assert counts.cpu().tolist() == [5 + n * ns, 3 + n * ns - len(want_rows), 77], what
                if pattern == "all on" and gridded:                                   # the sibling's listed set and zeros
                    raw2 = torch.full((n, l, ns, 4), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
                    rl2, rc2 = ops.background_rows(x_dev[:, 0], raw2[:, 0], g_dev, t=t_dev[:, 0] if stopped else None,
                                                   t_stop=s_dev if stopped else None)
                    torch.cuda.synchronize()
                    assert int(rc2) == got_n and np.array_equal(np.sort(rl2[:got_n].cpu().numpy().astype(np.int64)), want_rows), what
                    assert torch.equal(bits(raw2), bits(raw)), what
    for a, b in ((x_dev, xyz), (t_dev, t), (s_dev, stop)):                            # the inputs are as they were
        assert torch.equal(bits(a).cpu(), torch.from_numpy(b).view(torch.int32))


@pytest.mark.parametrize("ns", [1, 63, 64, 65, 129, 256])
def test_rows_kernel_equals_the_restatement(ns):
    for n in (1, 15, 16, 17, 197):
        _check_launches(n, ns)


def test_rows_kernel_when_a_wave_takes_a_second_run():
    """16 rays x 4 waves x the block cap is one run per wave; five rays more give the first wave a second one."""
    _check_launches(BR.RUN * 4 * BR.BLOCK_CAP + 5, 3)


def test_rows_kernel_refusals_leave_the_buffers_untouched():
    n, ns = 4, 8
    xyz = torch.zeros(n, ns, 3, device="cuda")
    raw = torch.full((n, ns, 4), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    flags = torch.ones(n, dtype=torch.uint8, device="cuda")
    rl = torch.full((n * ns,), POISON, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="uint8 or bool"):
        ops.background_ray_rows(xyz, raw, None)
    with pytest.raises(ValueError, match="uint8 or bool"):
        ops.background_ray_rows(xyz, raw, flags[:3])
    with pytest.raises(ValueError, match="capacity"):
        ops.background_ray_rows(xyz, raw, flags, row_list=rl[:n * ns - 1])
    with pytest.raises(ValueError, match="t_stop without"):
        ops.background_ray_rows(xyz, raw, flags, t_stop=torch.ones(n, device="cuda"))
    torch.cuda.synchronize()
    assert bool((bits(raw) == POISON).all()) and bool((rl == POISON).all())
    # ... and a bool mask is taken as it is
    rows, count = ops.background_ray_rows(xyz, raw, torch.tensor([True, False, True, False], device="cuda"))
    torch.cuda.synchronize()
    assert int(count) == 2 * ns and sorted(set((rows[:2 * ns] >> 8).tolist())) == [0, 2]
    assert not bool(bits(raw)[1].any()) and bool((bits(raw)[0] == POISON).all())


# ---------------------------------------------------------------------------------------- 2. the pipeline
def _mixed_flags(n):
    """A mask with whole runs on, whole runs off and mixed runs (16 rays per run)."""
    f = BR.flag_pattern("random", n, seed=3)
    f[16:32], f[48:64] = 0, 1
    return f


def _all_empty_grid(pc):
    return RE.grid_entry(np.zeros((2, 2, 2), bool), *OC.np_bounds(pc["bkgd_bbox"]))


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_all_flags_on_changes_no_bit(precision):
    pc = RE.piece(precision)
    on = torch.ones(S.CAP, dtype=torch.uint8, device="cuda")
    plain = RE.through_ops(pc, scene=True)
    got = RE.through_ops(pc, workspace_kw=dict(background_rays=True), scene=True, background_rays=on)
    RE.assert_same(got, plain, f"{precision}: all flags on")
    grid = RE.grid_entry(OC.half_x(8), *OC.np_bounds(pc["bkgd_bbox"]))
    culled = RE.through_ops(pc, workspace_kw=dict(background=True), scene=True, background_grid=grid)
    assert any(not torch.equal(RE.bits(a), RE.bits(b)) for a, b in zip(culled, plain))          # (the grid bites)
    both = RE.through_ops(pc, workspace_kw=dict(background=True, background_rays=True), scene=True, background_grid=grid, background_rays=on > 0)
    RE.assert_same(both, culled, f"{precision}: all flags on, with a grid")


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_a_mixed_mask_selects_per_ray_between_the_plain_call_and_the_call_without_background(precision):
    pc = RE.piece(precision)
    flags = torch.from_numpy(_mixed_flags(S.CAP)).cuda()
    assert 20 < int(flags.sum()) < S.CAP - 20
    plain = RE.through_ops(pc, scene=True)
    empty = RE.through_ops(pc, workspace_kw=dict(background=True), scene=True, background_grid=_all_empty_grid(pc))
    got = RE.through_ops(pc, workspace_kw=dict(background_rays=True), scene=True, background_rays=flags)
    assert len(got) == len(plain) == len(empty) == 6
    names = ("fine_mixed", "coarse_mixed", "fine_layer", "coarse_layer", "mask", "scene")
    for name, g, p, e in zip(names, got, plain, empty):
        on = flags.bool().reshape((-1,) + (1,) * (g.dim() - 1))
        want = torch.where(on, p, e)
        assert torch.equal(RE.bits(g), RE.bits(want)), f"{precision}: {name} is not where(flag, plain, no background)"
        if name != "mask":
            assert not torch.equal(RE.bits(p), RE.bits(e)), f"{precision}: {name}: the two source renders agree, the comparison means nothing"
            assert not torch.equal(RE.bits(p)[flags == 0], RE.bits(e)[flags == 0]), name
    assert torch.equal(got[4], plain[4]) and torch.equal(plain[4], empty[4])                     # (the mask bits follow the boxes only)
    # the same mask with the scene passes off, and the counters: a masked ray's samples are tested and not listed
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    five = RE.through_ops(pc, workspace_kw=dict(background_rays=True), background_rays=flags, background_counts=counts)
    RE.assert_same(five, got[:5], f"{precision}: without the scene passes")
    per_ray = 2 * pc["n1"] + pc["n2"]
    assert counts.tolist() == [S.CAP * per_ray, int((flags == 0).sum()) * per_ray]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("variant", ["mask alone", "with a grid and termination of layer 0", "only_coarse with a grid"])
def test_pipeline_equals_its_definition(monkeypatch, precision, variant):
    only_coarse = variant.startswith("only_coarse")
    case = OC.plain_case(only_coarse=only_coarse)
    rays = S.case_rays(case)[:S.CAP].contiguous().cuda()
    model = SE.make_model(case, precision)
    l = model.total_layers
    term = [False] * l
    grids = None
    if variant != "mask alone":
        grids = BGT._attach(model, case)
    if variant.startswith("with"):
        model.set_termination(TAU, layers=[2], background=True)
        term = [True, False, True, False]
        assert model.termination.flags(model) == term
    flags = torch.from_numpy(_mixed_flags(S.CAP)).cuda()
    pairs = []
    with_chain(model, monkeypatch, pairs, term, TAU)
    with torch.no_grad():
        model.render_rays_scene(rays, only_coarse, case["thr"], case["bthr"], ref_chunk=case["chunk"], background_rays=flags)
    torch.cuda.synchronize()
    launch = pairs[0][1].launch
    assert len(pairs) == 1 and launch["scene"] and launch["background_rays"].shape == (S.CAP,)
    assert (launch.get("background_id") is not None) == (grids is not None)
    assert_pairs_equal(pairs, f"{variant} {precision}")
    per_ray = case["n1"] if only_coarse else 2 * case["n1"] + case["n2"]
    if grids is not None:        # the one rows launch per stage counted every sample, the masked rays' among the not listed
        tested, skipped = grids.stats()["background"]
        assert tested == S.CAP * per_ray and int((flags == 0).sum()) * per_ray < skipped < tested
    if variant.startswith("with"):
        assert sorted(model.termination.stats()["rows"]) == [2]                       # (layer 0's visibility_rows launch is replaced)


def test_the_model_refuses_the_mask_where_it_cannot_act():
    case = OC.plain_case()
    rays = S.case_rays(case)[:S.CAP].contiguous().cuda()
    model = SE.make_model(case, "fp32")
    flags = torch.ones(S.CAP, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="one entry per ray"):
        model.render_rays_raw(rays, background_rays=flags[:5])
    with pytest.raises(ValueError, match="one entry per ray"):
        model.render_rays_raw(rays, background_rays=flags.float())
    model.mlp_schedule = "per_net"                                                    # precision 2: one launch per network
    try:
        with pytest.raises(ValueError, match="per_net"):
            with torch.no_grad():
                model.render_rays_raw(rays, background_rays=flags)
    finally:
        model.mlp_schedule = "stage"
    model.train(True)
    try:
        with pytest.raises(RuntimeError, match="training mode"):
            model.render_rays_raw(rays, background_rays=flags)
    finally:
        model.train(False)


# ---------------------------------------------------------------------------------------- 3. the model
H, W, N, IDS = GR.H, GR.W, GR.N, GR.IDS


def _view(model, orbit=GR.ORBIT):
    K, T = syn.camera(H, W, orbit)
    return K, T, ops.generate_rays(K, T, H, W, frame_ids=IDS)


def test_launch_pieces_are_the_pieces_rendered_by_hand(model):
    _, _, rays = _view(model)
    occluder = torch.from_numpy(OCL.case_occluder(N)).cuda()
    flags = torch.from_numpy(BR.flag_pattern("random", N, seed=9)).cuda()
    assert N > 3 * S.CAP and model.max_rays_per_launch == S.CAP                       # four launch pieces
    with torch.no_grad():
        whole = model.render_rays_occluded(rays, occluder, background_rays=flags)
        unmasked = model.render_rays_occluded(rays, occluder)
        parts = []
        try:
            for s in range(0, N, S.CAP):
                e = min(s + S.CAP, N)
                model.ray_window = (s, 0, 0)                                          # (the piece's place in the view keys its draws)
                parts.append(GR.flat(model.render_rays_occluded(rays[s:e].contiguous(), occluder[s:e], background_rays=flags[s:e].bool())))
        finally:
            model.ray_window = (0, 0, 0)
    torch.cuda.synchronize()
    got = GR.flat(whole)
    assert len(parts) == 4 and all(len(p) == len(got) for p in parts)
    for j, x in enumerate(got):
        y = torch.cat([p[j] for p in parts], 0)
        assert x.dtype == y.dtype and (torch.equal(x, y) if x.dtype == torch.bool else GR.same_bits(x, y)), j
    off = flags == 0
    plain = GR.flat(unmasked)
    assert not GR.same_bits(got[0][off], plain[0][off]) and GR.same_bits(got[0][~off], plain[0][~off])    # the mask bites, and only there


def test_a_masked_call_leaves_the_background_cache_alone(model):
    K, T, rays = _view(model)
    flags = torch.from_numpy(BR.flag_pattern("random", N, seed=4)).cuda()
    pieces = (N + S.CAP - 1) // S.CAP

    def render(**kw):
        with torch.no_grad():
            out = model.render_rays_raw(rays, **kw)
        torch.cuda.synchronize()
        return [o.clone() for o in out]
    want_masked, want_plain = render(background_rays=flags), render()
    cache = BackgroundCache()
    model.set_background_cache(cache)
    model.view_key = view_key(K, T, H, W, IDS)
    try:
        render()
        render()
        assert (cache.stats["hits"], cache.stats["misses"], cache.stats["captures"]) == (pieces, pieces, pieces)
        before = dict(cache.stats)
        entries = {k: tuple(None if x is None else x.clone() for x in v) for k, v in cache._entries.items()}
        got = render(background_rays=flags)
        assert dict(cache.stats) == before and list(cache._entries) == list(entries)
        for k, kept in entries.items():
            assert all(GR.same_bits(a, b) for a, b in zip(cache._entries[k], kept) if b is not None)
        GR_same = lambda a, b: all(torch.equal(x, y) if x.dtype == torch.uint8 else GR.same_bits(x, y) for x, y in zip(a, b))
        assert GR_same(got, want_masked) and not GR_same(got, want_plain)
        assert GR_same(render(), want_plain) and cache.stats["hits"] == 2 * pieces     # ... and the next plain frame is served as before
    finally:
        model.view_key = None
        model.set_background_cache(None)


# ---------------------------------------------------------------------------------------- 4. reprojection, exclusive
SPEC_X = rp.ReprojectSpec(3, GR.REL, GR.A_MIN, exclusive=True)


def _zero(x):
    return not bool(x.contiguous().view(torch.int32).any())


def test_exclusive_reprojection_is_the_calls_made_by_hand(model):
    K, T, _ = _view(model)
    K2, T2, rays2 = _view(model, GR.ORBIT + 3.0)
    plate = rp.BackgroundPlate.render(model, K, T, H, W, IDS, SPEC_X, index=0)
    state = lambda: (dict(model.display_layers), getattr(model, "view_key", None), getattr(model, "view_frame_ids", None), model.seed)
    before = state()
    # no hole is rendered separately: the layer-0-only render is not called at all
    real = model.render_rays_raw
    model.render_rays_raw = lambda *a, **k: (_ for _ in ()).throw(AssertionError("a separate render in exclusive mode"))
    try:
        five, scene, occluded, stats = parallel.render_view_reprojected(model, K2, T2, H, W, IDS, [plate], SPEC_X)
    finally:
        del model.render_rays_raw
    assert model.render_rays_raw.__func__ is real.__func__ and state() == before
    assert before[0] == {0: 1, 1: 1, 2: 1} and model.seed == 11
    print("exclusive, 3 degrees on:", stats)
    # by hand: the warp alone, the flags by the occluder's own rule, one call
    values, t, src, holes, n_holes = ops.reproject([plate.source()], K2, T2, H, W, GR.REL)
    rows = values.clone()
    rows[:, 4] = t
    absent = ~(rows[:, 3] > 0) | ~torch.isfinite(rows[:, 4])
    flags = absent.to(torch.uint8)
    warped_rows, got_holes, got_n, _ = rp.warp_plates(model, K2, T2, H, W, IDS, [plate], SPEC_X, render_holes=False)
    assert got_n == n_holes and torch.equal(got_holes, holes) and GR.same_bits(warped_rows, rows)
    assert bool(absent[holes.long()].all())                                          # every hole of the warp is flagged
    with torch.no_grad():
        hand = model.render_rays_occluded(rays2, rows, background_rays=flags)
        unmasked = model.render_rays_occluded(rays2, rows)
    torch.cuda.synchronize()
    GR.assert_same_outputs((five, scene, occluded), hand)
    # the stats identities
    flagged = int(flags.sum())
    assert stats == dict(holes=flagged, reused=N - flagged, rays_background=flagged, keys=(0,))
    assert 0 < n_holes <= flagged < N
    # one source of background per ray: where the plate has a row, layer 0 has no share in the frame (nor an image of its own) ...
    present = ~absent
    for x in occluded["scene"][0] + scene[0] + five[2][0]:
        assert _zero(x[present])
    assert float(occluded["share"][2][present].min()) > 0.0 and _zero(occluded["share"][2][absent])
    # ... and where it has none, the frame is the unmasked call's, bit for bit
    for x, y in zip(GR.flat((five, scene, occluded)), GR.flat(unmasked)):
        assert torch.equal(x[absent], y[absent]) if x.dtype == torch.bool else GR.same_bits(x[absent], y[absent])
    assert not _zero(unmasked[2]["scene"][0][2][present])                             # (unmasked, the real background is composited beside the plate)


def test_exclusive_at_a_keys_own_pose_evaluates_no_background(model):
    K, T, rays = _view(model)
    plate = rp.BackgroundPlate.render(model, K, T, H, W, IDS, SPEC_X, index=0)
    assert int(torch.isnan(plate.t).sum()) == 0                                       # a whole plate
    ops.profile_begin()
    five, scene, occluded, stats = parallel.render_view_reprojected(model, K, T, H, W, IDS, [plate], SPEC_X)
    torch.cuda.synchronize()
    recs = ops.profile_end()
    assert stats == dict(holes=0, reused=N, rays_background=0, keys=(0,))
    rows = [r for r in recs if r["kernel"] == "background_rows"]
    pieces = (N + S.CAP - 1) // S.CAP
    assert len(rows) == 2 * pieces and all(r["kind"] & 2 and r["tag"] == 0 for r in rows)     # the per-ray flavour, once per stage and piece
    assert all(_zero(x) for x in occluded["scene"][0]) and float(occluded["mixed"][2].min()) > 0.0
    # the non-exclusive frame of the same pose carries the same plate: the frames agree closely, and the default spec is unchanged
    _, _, plain, plain_stats = parallel.render_view_reprojected(model, K, T, H, W, IDS, [plate], GR.SPEC)
    assert plain_stats == dict(holes=0, reused=N, rays_background=0, keys=(0,))
    assert not any(_zero(x) for x in plain["scene"][0])                               # (there layer 0 is evaluated and composited)


def test_the_renderer_takes_the_exclusive_spec(model):
    r = GR.renderer(model, [GR.ORBIT + 3.0 * i for i in range(4)], reproject=dict(key_every=3, rel=GR.REL, a_min=GR.A_MIN, exclusive=True))
    assert r.reproject.exclusive is True
    r.render_path()
    stats = r.reproject_stats
    print([dict(s) for s in stats])
    assert [s["keys"] for s in stats] == [(0, 3), (0, 3), (0, 3), (3,)]
    assert all(s["holes"] + s["reused"] == N and s["rays_background"] == s["holes"] for s in stats)
    assert stats[0]["holes"] == 0 and stats[3]["holes"] == 0 and stats[1]["holes"] > 0
    torch.cuda.synchronize()
