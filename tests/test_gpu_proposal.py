"""Grid proposals on the MI355X (include/stnerf.h: stnerf_density_grid): a flagged layer's coarse densities
are a trilinear lookup in a grid of vertex densities and its coarse networks do not run.

1. ``ops.proposal_density`` bit for bit against the numpy restatement (tests/proposal_common.py): ns on either side of a wave, three
   grid shapes with +-inf vertices, points on, beside and far outside the faces, +-inf and NaN coordinates, ray lists with count 0, n
   and a strict subset, no list; unlisted rows keep a sentinel.
2. The lookup against fp64 on points rebuilt in fp64 from rays, depths and a shift + scale + rotation edit.
3. The pipeline against the chain of op-level entries, bit for bit, in both arithmetics.
4. A flagged layer's coarse networks are not run: another coarse SpaceNet changes no bit, the profiler shows no coarse launch for it.
5. The option absent changes no launch, no bit and no workspace; the render call's refusals launch nothing.
6. Hand-checkable grids: a constant one against the compositor itself, a half-dense one on a layer turned by 90 degrees.
7. A quality fence against the exact pipeline's own seed-to-seed difference (profiles/proposal_ab.md has the measured ratios).
Needs an MI355X: `pytest -m gpu`."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import occupancy_common as OCC
import pipeline_chain as CHAIN
import proposal_common as PC
import scene_edits_common as S
import test_gpu_scene_edits_oracle as SE
from oracle import stnerf_oracle as O
from stnerf_amd import hip, ops, synthetic as syn
from stnerf_amd.deep import DeepSpec
from stnerf_amd.proposal import ProposalGrids
from pipeline_chain import bits, cu, same_bits, with_chain
from test_gpu_occluder import POISON
from test_gpu_termination import TAU
from test_gpu_occupancy import attach

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(autouse=True)
def detach():
    yield
    CHAIN.detach_models()


# ---------------------------------------------------------------------------------------- 1. the lookup, bit for bit
N_RAYS, N_LAYERS = 37, 3


@pytest.mark.parametrize("res", [(1, 1, 1), (5, 3, 2), (16, 16, 16)])
@pytest.mark.parametrize("ns", [1, 63, 64, 65, 200])
def test_lookup_equals_the_restatement_bit_for_bit(ns, res):
    n, l = N_RAYS, N_LAYERS
    sigma, lo, hi, inv = PC.grid_of(res, seed=100 * ns + res[0], infs=res != (1, 1, 1))      # (one cell with an inf corner has no finite value)
    assert np.isinf(sigma).any() == (res != (1, 1, 1))
    pts = np.zeros((n, l, ns, 3), F)
    for i in range(l):
        pts[:, i], placed = PC.points_of(n, ns, lo, hi, seed=7 * ns + i)
        assert placed == min(n * ns, PC.special_points(lo, hi).shape[0])
    assert np.isnan(pts).any() and np.isinf(pts).any()
    xyz = cu(pts)
    grid = (cu(sigma), lo.tolist(), inv.tolist())
    g = np.random.default_rng(ns)
    subset = np.sort(g.permutation(n)[:n // 3]).astype(np.int32)
    for layer in range(l):
        want_all = PC.np_proposal_raw(pts[:, layer], sigma, lo, inv)
        lists = {"none": None, "count 0": (g.permutation(n).astype(np.int32), 0), "count n": (g.permutation(n).astype(np.int32), n),
                 "subset": (np.concatenate([subset, np.full(n - subset.size, 5, np.int32)]), subset.size)}
        for name, spec in lists.items():
            raw = torch.full((n, l, ns, 4), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
            kw = {}
            listed = np.ones(n, bool)
            if spec is not None:
                kw = dict(ray_list=cu(spec[0], torch.int32), ray_count=cu([spec[1]], torch.int32))
                listed = np.zeros(n, bool)
                listed[spec[0][:spec[1]]] = True
            out = ops.proposal_density(xyz[:, layer], raw[:, layer], grid, layer=layer, **kw)
            torch.cuda.synchronize()
            assert out.data_ptr() == raw[:, layer].data_ptr()
            got = raw.cpu().numpy()
            what = f"ns={ns} res={res} layer={layer} list={name}"
            assert PC.same_sigma(got[listed, layer], want_all[listed]), what
            assert not got[listed, layer, :, :3].view(np.uint32).any(), f"{what}: the colour words are not +0"
            keep = got.view(np.uint32) == POISON
            assert keep[~listed].all(), f"{what}: a row of an unlisted ray was written"
            assert keep[:, [j for j in range(l) if j != layer]].all(), f"{what}: another layer's slice was written"
    # the cases bite: the clamps, the exact vertices and the NaN are all there
    s = PC.np_lookup(pts[:, 0], sigma, lo, inv)
    assert np.isnan(s).any() and np.isfinite(s).any()


def test_lookup_argument_errors():
    z = lambda *s: torch.zeros(*s, device="cuda")
    grid = (z(3, 3, 3), [0.0] * 3, [1.0] * 3)
    with pytest.raises(ValueError, match="grid"):
        ops.proposal_density(z(4, 8, 3), z(4, 8, 4), None)
    with pytest.raises(ValueError, match=r"\(n,ns,3\)"):
        ops.proposal_density(z(4, 8, 3), z(4, 9, 4), grid)
    with pytest.raises(ValueError, match="come together"):
        ops.proposal_density(z(4, 8, 3), z(4, 8, 4), grid, ray_list=torch.zeros(4, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="ns = 257"):
        ops.proposal_density(z(2, 257, 3), z(2, 257, 4), grid)
    with pytest.raises(ValueError, match="layer 16"):
        ops.proposal_density(z(2, 8, 3), z(2, 8, 4), grid, layer=16)
    with pytest.raises(ValueError, match="not finite"):
        ops.proposal_density(z(2, 8, 3), z(2, 8, 4), (grid[0], [0.0, float("inf"), 0.0], grid[2]))
    assert ops.proposal_density(z(0, 8, 3), z(0, 8, 4), grid).shape == (0, 8, 4)


# ---------------------------------------------------------------------------------------- 2. the lookup against fp64
def test_lookup_against_fp64_on_points_rebuilt_from_rays_depths_and_edits():
    """The sampler's points of a layer that is shifted, scaled and turned; the grid lies over the layer's UNEDITED box.  The fp64 points
    are o' = m (o - c) + c, d' = m d, p = t d' + o', then the un-edit p - shift, (p - pivot) / scale + pivot (include/stnerf.h), from
    the fp32 rays, depths and edit promoted to fp64 -- not xyz_c.  Bound, from the inputs: the largest change of the fp64 result when
    every coordinate moves by 4 ulp of max(|p_a|, |lo_a|) either way, plus 8 x 2^-24 x max|v|.  The scene is laid out so that the
    intermediate values of the point arithmetic stay within the binade of the points (the bound is in ulps of those).  A grid applied in
    the EDITED frame is off by the shift: far outside this bound."""
    n, n1 = 96, 64
    lo_u, hi_u = np.array([2.1, 2.2, 2.3]), np.array([3.3, 3.4, 3.5])
    pivot = torch.tensor([2.5, 2.5, 2.5])
    shift, scale, angle = [0.25, -0.125, 0.5], 1.25, 0.4
    unedited = syn.aabb_corners(lo_u.tolist(), hi_u.tolist())
    edited = (unedited - pivot) * scale + pivot + torch.tensor(shift)
    centre = edited.mean(0)
    m = S.ray_matrix(angle)
    bkgd = syn.aabb_corners((0.0, 0.0, 0.0), (6.0, 6.0, 6.0))
    boxes = torch.stack([bkgd, edited]).cuda()
    g = np.random.default_rng(11)
    o = np.stack([g.uniform(2.6, 3.6, n), g.uniform(2.5, 3.5, n), np.full(n, 2.0)], -1)
    d = np.stack([g.uniform(-0.15, 0.15, n), g.uniform(-0.15, 0.15, n), np.ones(n)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rays = cu(np.concatenate([o, d, np.ones((n, 1))], -1).astype(F))
    edits = [(None, None), (shift, scale)]
    t, xyz, mask = ops.sample_coarse(rays, boxes, n1, seed=5, edits=edits, pivot=pivot, rotations=[None, (m, centre)])
    hit = mask[:, 1].bool().cpu().numpy()
    assert hit.sum() > n // 2
    res = (9, 7, 8)
    sigma = (np.random.default_rng(12).random((res[2] + 1, res[1] + 1, res[0] + 1)) * 20).astype(F)
    lo, hi = OCC.np_bounds(unedited)
    inv = OCC.np_inv_cell(res, lo, hi)
    raw = torch.zeros(n, 2, n1, 4, device="cuda")
    ops.proposal_density(xyz[:, 1], raw[:, 1], (cu(sigma), lo.tolist(), inv.tolist()), layer=1)
    torch.cuda.synchronize()
    got = raw[:, 1, :, 3].cpu().numpy().astype(np.float64)[hit]
    # the points again, in fp64, from the documented transforms
    r64 = rays.cpu().numpy().astype(np.float64)[hit]
    t64 = t[:, 1].cpu().numpy().astype(np.float64)[hit]
    m64, c64 = m.numpy().astype(np.float64), centre.numpy().astype(np.float64)
    o2 = (r64[:, 0:3] - c64) @ m64.T + c64
    d2 = r64[:, 3:6] @ m64.T
    p = t64[..., None] * d2[:, None, :] + o2[:, None, :]
    p = p - np.asarray(torch.tensor(shift, dtype=torch.float32).numpy(), np.float64)
    pv = pivot.numpy().astype(np.float64)
    p = (p - pv) / float(F(scale)) + pv
    assert np.abs(p - xyz[:, 1].cpu().numpy().astype(np.float64)[hit]).max() < 1e-5         # the same points, up to fp32
    inside = ((p > lo.astype(np.float64) - 1e-5) & (p < hi.astype(np.float64) + 1e-5)).all(-1)
    assert inside.mean() > 0.99                                                              # the un-edited points lie in the unedited box
    want = PC.exact_lookup(p, sigma, lo, inv)
    delta = 4 * np.spacing(np.maximum(np.abs(p), np.abs(lo.astype(np.float64))).astype(F)).astype(np.float64)
    change = np.zeros_like(want)
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                change = np.maximum(change, np.abs(PC.exact_lookup(p + delta * np.array([sx, sy, sz]), sigma, lo, inv) - want))
    bound = change + 8 * PC.U * float(sigma.max())
    err = np.abs(got - want)
    print(f"lookup vs fp64: max err {err.max():.3e}, max err / bound {float((err / bound).max()):.3f}, median bound {np.median(bound):.3e}")
    assert (err <= bound).all(), float((err / bound).max())
    # what the test is for: the same grid applied to the points BEFORE the un-edit misses the bound on most samples
    edited_frame = PC.exact_lookup((p - pv) * float(F(scale)) + pv + np.asarray(shift), sigma, lo, inv)
    assert (np.abs(edited_frame - want) > bound).mean() > 0.5


# ---------------------------------------------------------------------------------------- 3. the pipeline is the chain
def assert_pairs_equal(pairs, what, pieces):
    CHAIN.assert_pairs_equal(pairs, what, pieces)
    for piece, (got, chain) in enumerate(pairs):
        launch = chain.launch
        assert not launch["only_coarse"] and launch.get("proposal_ids") is not None, what
        assert all(launch.get(k) is None for k in ("background_id", "background_rays", "occluder")), what
        if chain.deep is not None:
            total = int(got[8])
            assert torch.equal(got[6], chain.deep[0]) and total == chain.deep[1].shape[0] > 0, f"{what}: piece {piece}: the deep offsets differ"
            assert same_bits(got[7][:total], chain.deep[1]), f"{what}: piece {piece}: the deep records differ"


PIECES = (S.N + S.CAP - 1) // S.CAP
RES = 8                 # grid cells per axis of the pipeline tests: coarse enough to differ from the networks everywhere
VARIANTS = ["performers", "background", "one_of_two", "edits", "culls", "terminated", "deep"]


def setup_variant(model, case, variant):
    """-> (the termination flags, tau, the deep spec) of a variant, the model set up for it."""
    l = model.total_layers
    flags, tau, spec = [False] * l, 0.0, None
    grids = ProposalGrids(res=RES)
    if variant == "background":
        grids = ProposalGrids(res=RES, layers=[], background=True, background_res=(6, 5, 7))
    if variant == "one_of_two":
        grids = ProposalGrids(res=RES, layers=[1])
    if variant == "culls":
        attach(model, OCC.manual_grids(case, "half_x", 0, layers=(1, 2)), samples=True)
    if variant == "terminated":
        model.set_termination(TAU, layers=[1, 2], background=True)
        flags, tau = [True, True, True, False], TAU
    if variant == "deep":
        spec = DeepSpec(1e-4, 0.25)
    model.set_proposal(grids)
    return flags, tau, spec


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_pipeline_is_the_chain_of_op_level_entries(monkeypatch, precision, variant):
    case = S.make_case() if variant == "edits" else OCC.plain_case()      # (edits: shift, scale, layer 1 turned, the opacity table)
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case, precision)
    flags, tau, spec = setup_variant(model, case, variant)
    pairs = []
    with_chain(model, monkeypatch, pairs, flags, tau)
    with torch.no_grad():
        if spec is not None:
            model.render_rays_deep(rays, spec, False, case["thr"], case["bthr"], ref_chunk=case["chunk"])
        else:
            model.render_rays_scene(rays, False, case["thr"], case["bthr"], ref_chunk=case["chunk"])
    torch.cuda.synchronize()
    assert_pairs_equal(pairs, f"{precision} {variant}", PIECES)
    flagged = model.proposal.flagged_layers(model)
    assert flagged == {"background": [0], "one_of_two": [1]}.get(variant, [1, 2, 3])
    # a flagged layer's coarse output carries zero colour; where it has alpha the grid gave it
    lo_c = torch.cat([p[0][3] for p in pairs])
    for i in flagged:
        assert not bool(bits(lo_c[:, i, 0:3]).any()), f"layer {i}: a coarse colour word is not +0"
        assert float(lo_c[:, i, 4].max()) > 0
    if variant == "culls":
        st = model._occupancy.stats()
        assert sorted(st["samples"]) == [1, 2] and all(0 < skipped < tested for tested, skipped in st["samples"].values())
        hits = {i: int(sum(int(p[0][4][:, i].sum()) for p in pairs)) for i in (1, 2)}
        assert all(st["samples"][i][0] == hits[i] * (case["n1"] + case["n2"]) for i in (1, 2))      # the fine stage only
    if variant == "terminated":
        rows = model.termination.stats()["rows"]
        assert sorted(rows) == [0, 1, 2] and all(0 <= skipped < tested for tested, skipped in rows.values()), rows
        assert sum(skipped for _, skipped in rows.values()) > 0, rows          # (the stop depths come from the grids' weights, and bite)


# ---------------------------------------------------------------------------------------- 4. the coarse networks are not run
def profiled(model, case, rays):
    model._workspace = None
    ops.profile_begin()
    with torch.no_grad():
        out = S.flat(model.render_rays_scene(rays, False, case["thr"], case["bthr"], ref_chunk=case["chunk"]))
    torch.cuda.synchronize()
    return out, ops.profile_end()


def assert_same(a, b, what):
    assert set(a) == set(b)
    for k in sorted(a):
        assert torch.equal(a[k], b[k]) if a[k].dtype == torch.bool else same_bits(a[k], b[k]), f"{what}: {k} differs"


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_the_coarse_networks_of_a_flagged_layer_are_not_run(precision):
    """Layers 1 and 3 (the instance of performer 1) share module 0.  With both flagged, module 0's COARSE SpaceNet is an input of no
    launch: putting performer 2's coarse network in its place changes no bit (unflagged it does).  The profiler: no stand-alone coarse
    MotionNet launch (tag = the layer, ns = n1) for a flagged layer, as many as before for the others; with every evaluated layer flagged
    no coarse stage launch at all (tag 0), and with it no coarse ray-bias launch, which the stage entry makes per item."""
    case = OCC.plain_case()
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case, precision)
    n1, S_ = case["n1"], case["n1"] + case["n2"]
    plain, recs_plain = profiled(model, case, rays)
    own = model.spacenets[0]

    def swapped():
        model.spacenets[0] = model.spacenets[1]
        try:
            return profiled(model, case, rays)
        finally:
            model.spacenets[0] = own
    assert any(not same_bits(plain[k], v) for k, v in swapped()[0].items() if v.dtype != torch.bool)     # the probe bites
    coarse_stage = lambda recs: [r for r in recs if r["kernel"] == "mlp_stage" and r["tag"] == 0]
    coarse_motion = lambda recs, i: [r for r in recs if r["kernel"] == "motionnet" and r["tag"] == i and r["ns"] == n1]
    lookups = lambda recs: [(r["tag"], r["ns"]) for r in recs if r["kernel"] == "proposal_density"]
    assert len(coarse_stage(recs_plain)) == PIECES and not lookups(recs_plain)
    reuse = precision == "bf16x3"                             # (the split-bf16 stages run the performers' MotionNets in launches of their own)
    assert all(len(coarse_motion(recs_plain, i)) == (PIECES if reuse else 0) for i in (1, 2, 3))

    model.set_proposal(ProposalGrids(res=RES, layers=[1, 3]))
    profiled(model, case, rays)                                                  # (the grids are built on first use: keep that out of the records)
    a, recs_a = profiled(model, case, rays)
    b, recs_b = swapped()
    assert_same(a, b, f"{precision}: another coarse SpaceNet under a flagged layer")
    assert [r["kernel"] for r in recs_a] == [r["kernel"] for r in recs_b]
    assert lookups(recs_a) == [(1, n1), (3, n1)] * PIECES
    assert len(coarse_stage(recs_a)) == PIECES                                   # the background and layer 2 are still evaluated
    assert not coarse_motion(recs_a, 1) and not coarse_motion(recs_a, 3) and len(coarse_motion(recs_a, 2)) == (PIECES if reuse else 0)
    # the fine MotionNet of a flagged layer runs fused: no stand-alone fine launch either
    assert not [r for r in recs_a if r["kernel"] == "motionnet" and r["tag"] in (1, 3)]
    assert any(not same_bits(plain[k], a[k]) for k in a if a[k].dtype != torch.bool)          # (and the proposal is no no-op)

    model.set_proposal(ProposalGrids(res=RES, background=True))                 # every evaluated layer
    profiled(model, case, rays)
    c, recs_c = profiled(model, case, rays)
    assert not coarse_stage(recs_c) and not [r for r in recs_c if r["kernel"] == "motionnet"]
    assert lookups(recs_c) == [(0, n1), (1, n1), (2, n1), (3, n1)] * PIECES
    assert len([r for r in recs_c if r["kernel"] == "mlp_stage" and r["tag"] == 1 and r["ns"] == S_]) == PIECES   # the fine stage is whole


# ---------------------------------------------------------------------------------------- 5. the option absent; the refusals
def direct_call(model, case, rays, **kw):
    """One ``ops.render_rays`` call on the first launch piece with the model's own tables -> the outputs."""
    r = rays[:S.CAP].contiguous()
    boxes, pivot = model._retimed_boxes(r[0, 6:].cpu())
    p = model._render_params(r.shape[1], pivot, True, False, case["thr"], case["bthr"], (0, 0, 0))
    for k in [k for k in kw if k.startswith("p_")]:
        v = kw.pop(k)
        v(p) if callable(v) else setattr(p, k[2:], v)
    keep = []
    nets = model._net_pointers(keep)
    l = model.total_layers
    ws = torch.empty(4 * ops.render_workspace_bytes(S.CAP, l, p.n1, p.n2, False, background=True), dtype=torch.uint8, device="cuda")
    return ops.render_rays(r, boxes.cuda(), nets, p, ws, jitter=model.replay["jitter"][:, :S.CAP].contiguous(),
                           u=model.replay["u"][:, :S.CAP].contiguous(), **kw)


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_no_proposal_changes_no_bit_no_launch_and_no_workspace(monkeypatch, precision):
    case = OCC.plain_case()
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case, precision)
    l, n1, n2 = model.total_layers, case["n1"], case["n2"]
    plain, recs = profiled(model, case, rays)
    bytes_plain = model._workspace.numel()
    # attached grids that flag nothing: the same launches, the same bits, the same workspace
    model.set_proposal(ProposalGrids(res=RES, layers=[]))
    got, recs1 = profiled(model, case, rays)
    assert_same(plain, got, "grids that flag no layer")
    assert [r["kernel"] for r in recs1] == [r["kernel"] for r in recs] and model._workspace.numel() == bytes_plain
    # with a flagged layer the workspace is still that size
    model.set_proposal(ProposalGrids(res=RES))
    profiled(model, case, rays)
    assert model._workspace.numel() == bytes_plain == hip.lib().stnerf_render_workspace_bytes(S.CAP, l, n1, n2, 0)
    model.set_proposal(None)
    # the record itself: a NULL table and an all-NULL table are the deep record with a zero tail
    opts = hip.RenderOptionsProposal()
    assert hip.lib().stnerf_render_workspace_bytes_opts(S.CAP, l, n1, n2, 0, opts.ref()) == bytes_plain
    assert hip.lib().stnerf_render_workspace_bytes_opts(S.CAP, l, n1, n2, 0, hip.RenderOptionsDeep().ref()) == bytes_plain
    table = (hip.DensityGrid * l)()
    opts.proposal = table
    assert hip.lib().stnerf_render_workspace_bytes_opts(S.CAP, l, n1, n2, 0, opts.ref()) == bytes_plain
    ops.profile_begin()
    base = direct_call(model, case, rays)
    torch.cuda.synchronize()
    recs_base = ops.profile_end()
    assert ops._density_grid_table([None] * l, l) is None       # (``ops`` sends the shorter record for such a table: hand it through)
    monkeypatch.setattr(ops, "_density_grid_table", lambda t, l_: table)
    ops.profile_begin()
    out = direct_call(model, case, rays, proposal=[None] * l)
    torch.cuda.synchronize()
    recs_null = ops.profile_end()
    assert [r["kernel"] for r in recs_null] == [r["kernel"] for r in recs_base] and recs_base
    assert all(torch.equal(a, b) if a.dtype == torch.uint8 else same_bits(a, b) for a, b in zip(out, base))


def test_the_render_calls_refusals_launch_nothing():
    case = OCC.plain_case()
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case, "fp32")
    l, n1, n2 = model.total_layers, case["n1"], case["n2"]
    z = lambda *s: torch.zeros(*s, device="cuda")
    entry = (z(3, 3, 3), [-1.0] * 3, [1.0] * 3)
    on = lambda *layers: [entry if i in layers else None for i in range(l)]
    cache = lambda mode: (z(S.CAP, n1, 4), z(S.CAP, n1 + n2, 4), mode)
    lcache = lambda mode: [None, (z(S.CAP, n1, 4), z(S.CAP, n1 + n2, 4), torch.zeros(S.CAP, dtype=torch.int32, device="cuda"),
                                  torch.zeros(1, dtype=torch.int32, device="cuda"), mode)] + [None] * (l - 2)
    some_bits = torch.full((16,), -1, dtype=torch.int32, device="cuda")
    cases = [("precision 2", dict(proposal=on(1), p_precision=2)),
             ("hidden", dict(proposal=on(2), p_shown=lambda p: p.shown.__setitem__(2, 0))),
             ("layer cache", dict(proposal=on(1), layer_caches=lcache(hip.LAYER_CACHE_CAPTURE))),
             ("layer cache", dict(proposal=on(1), layer_caches=lcache(hip.LAYER_CACHE_REUSE))),
             ("background cache", dict(proposal=on(0), cache=cache(hip.BKGD_CACHE_CAPTURE))),
             ("background cache", dict(proposal=on(0), cache=cache(hip.BKGD_CACHE_REUSE))),
             ("per-ray background mask", dict(proposal=on(0), background_rays=torch.ones(S.CAP, dtype=torch.uint8, device="cuda"))),
             ("background grid", dict(proposal=on(0), background_grid=(some_bits, (8, 8, 8), [-3.0] * 3, [8 / 6] * 3))),
             ("not finite", dict(proposal=[None, (entry[0], [0.0, float("nan"), 0.0], entry[2])] + [None] * (l - 2)))]
    for what, kw in cases:
        ops.profile_begin()
        try:
            with pytest.raises(ValueError, match=what):
                direct_call(model, case, rays, **kw)
        finally:
            torch.cuda.synchronize()
            assert ops.profile_end() == [], f"{what}: something was launched"
    # the same tables are fine where nothing conflicts: a performer beside a background cache, the background beside a layer cache
    direct_call(model, case, rays, proposal=on(1), cache=cache(hip.BKGD_CACHE_CAPTURE))
    direct_call(model, case, rays, proposal=on(0), layer_caches=lcache(hip.LAYER_CACHE_CAPTURE))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------- 6. hand-checkable grids
def test_a_constant_grid_gives_the_compositors_own_alpha_for_constant_density():
    case = OCC.plain_case()
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case, "bf16x3")
    c = 4.0                     # a power of two: (c u) + (c f) with u = 1 - f is c itself, so the grid returns the constant exactly
    lo, hi = OCC.layer_bounds(case, 1)
    grids = ProposalGrids(layers=[])
    grids.set_manual(1, torch.full((3, 4, 5), c), lo, hi)
    model.set_proposal(grids)
    with torch.no_grad():
        raw = model.render_rays_raw(rays, False, case["thr"], case["bthr"], ref_chunk=case["chunk"])
        t_c = SE.coarse_depths(model, case, rays)
    torch.cuda.synchronize()
    lo_c, mask = raw[3], raw[4]
    hit = mask[:, 1].bool()
    assert 20 < int(hit.sum()) < S.N
    l, n1 = model.total_layers, case["n1"]
    hand = torch.zeros(S.N, l, n1, 4, device="cuda")
    hand[:, 1, :, 3] = c
    want, _, _, _ = ops.composite(t_c, hand, mask, border=float(model.boarder_weight), near=float(model.near), fine=False, cut_negative_t=True,
                                  thresholds=[None] + [case["thr"]] * (l - 1), evaluated=[2] + [1] * (l - 1), rgb_activated=True)
    torch.cuda.synchronize()
    assert same_bits(lo_c[hit][:, 1], want[hit][:, 1])
    assert not bool(bits(lo_c[hit][:, 1, 0:3]).any()) and float(lo_c[hit][:, 1, 4].max()) > 0.9      # zero colour; opaque where the path is long


def test_a_half_dense_grid_follows_a_layer_turned_by_90_degrees():
    """Layer 1's grid is dense in the half x < mid of its UNEDITED box and zero elsewhere.  Turned by +90 degrees about z through the
    box's centre, that half shows in world y < cy.  Rays along +z at (cx + dx, cy -+ a): those at cy - a cross the dense half only
    (coarse alpha near 1), those at cy + a the empty half only (coarse alpha exactly 0).  Unturned the split is by x: both rows of rays
    straddle it, and alpha follows dx."""
    case = OCC.plain_case()
    model = SE.make_model(case, "bf16x3")
    model.replay = None
    l = model.total_layers
    ids = case["groups"][0][1]
    lo, hi = OCC.layer_bounds(case, 1)
    ext = (hi - lo).astype(np.float64)
    cx, cy = (lo[0] + hi[0]) / 2.0, (lo[1] + hi[1]) / 2.0
    a = 0.25 * min(ext[0], ext[1])
    R = 8
    assert a > ext[0] / R and a < 0.45 * min(ext[0], ext[1])             # a whole cell past the half-dense cell at mid; inside the turned box
    sigma = torch.zeros(R + 1, R + 1, R + 1)
    sigma[:, :, :R // 2] = 200.0
    grids = ProposalGrids(layers=[])
    grids.set_manual(1, sigma, lo, hi)
    model.set_proposal(grids)
    dxs = np.array([-0.3, -0.15, 0.15, 0.3]) * min(ext[0], ext[1])
    rows = [(cx + dx, cy + sy * a) for sy in (-1, 1) for dx in dxs]
    rays6 = torch.tensor([[x, y, float(lo[2]) - 1.0, 0.0, 0.0, 1.0] for x, y in rows], dtype=torch.float32)
    rays = torch.cat([rays6, torch.tensor(ids, dtype=torch.float32).repeat(len(rows), 1)], 1).cuda()

    def coarse_alpha(rotation):
        model.rotation = rotation
        with torch.no_grad():
            raw = model.render_rays_raw(rays, False, 0.0, 0.0)
        torch.cuda.synchronize()
        assert bool(raw[4][:, 1].all()), "every ray crosses layer 1's box"
        return raw[3][:, 1, 4].cpu().numpy()
    turned = coarse_alpha([None, math.pi / 2] + [None] * (l - 2))
    assert (turned[:4] > 0.99).all() and (turned[4:] == 0).all(), turned
    plain = coarse_alpha(None)
    assert (plain[[0, 1, 4, 5]] > 0.99).all() and (plain[[2, 3, 6, 7]] == 0).all(), plain
    model.rotation = None


# ---------------------------------------------------------------------------------------- 7. the quality fence
FENCE_SEEDS = [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)]
FENCE_K = 0.0170    # the largest measured ratio, 0.0136, x 1.25 (profiles/proposal_ab.md)


def fence_ratios(precision):
    """E_prop / E_seed for the eight seed pairs on the test model at a 32 x 32 view, performers flagged at res = 128."""
    case = OCC.plain_case()
    model = SE.make_model(case, precision)
    model.replay = None
    model.max_rays_per_launch = 1 << 16
    K, T = syn.camera(32, 32, S.ORBIT)
    rays = S.with_frame_ids(O.generate_rays(K, T, 32, 32), case).cuda()
    grids = ProposalGrids(res=128)

    def mixed_fine(seed, on):
        model.set_proposal(grids if on else None)
        model.seed = seed
        with torch.no_grad():
            out = model.render_rays_raw(rays, False, case["thr"], case["bthr"])[0]
        torch.cuda.synchronize()
        return out.double()
    ratios = []
    for a, b in FENCE_SEEDS:
        exact_a = mixed_fine(a, False)
        e_prop = float((mixed_fine(a, True) - exact_a).abs().mean())
        e_seed = float((mixed_fine(b, False) - exact_a).abs().mean())
        assert e_seed > 0
        ratios.append(e_prop / e_seed)
    model.set_proposal(None)
    st = grids.stats()              # performers 1 and 2, and the instance of 1 where its frame id is its own
    assert st["built"] in (2, 3) and st["bytes"] == st["built"] * 4 * 129 ** 3
    return ratios


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_quality_fence_against_the_exact_pipelines_own_seed_noise(precision):
    """E_prop = mean |proposal(seed a) - exact(seed a)| of mixed_fine, E_seed = mean |exact(seed b) - exact(seed a)|: the exact pipeline
    against itself.  E_prop <= k E_seed, k = 1.25 x the largest of the sixteen ratios measured on the MI355X (eight seed pairs, both
    arithmetics; profiles/proposal_ab.md lists them).  The seeds are fixed: a run repeats itself."""
    ratios = fence_ratios(precision)
    print(f"quality fence {precision}: E_prop / E_seed = " + ", ".join(f"{r:.5f}" for r in ratios))
    assert max(ratios) <= FENCE_K, (max(ratios), FENCE_K)
