"""In-scene layer passes (stnerf_composite_scene / stnerf_render_rays_scene): `merged_weights`, the weight every sample gets in the
MERGED composite, stored at its source index, and `scene`, layer i's share of the mixed image (sum_k wM {r, g, b, t, 1}).
Checked against the CPU oracle's composite of the stably sorted union, between the compositor's three routes bit for bit, for
neutrality towards the outputs `ops.composite` returns, for exact zeros where a layer has no output / takes no part, for the
identity sum_i scene[i] == mixed, for `scene` layer by layer against the sums over the oracle's weights, for overruns, and
through the whole pipeline up to `render_pose`.  Needs an MI355X: `pytest -m gpu`."""
import ctypes as C
import functools
import types

import pytest
import torch

from pipeline_chain import bits

from oracle import stnerf_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from stnerf_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def scene(n, l, S, seed, hit=0.5, ties=True):
    """(the generator of tests/test_gpu_composite_merge.py)  Depth lists as the sampler leaves them: ascending per layer inside
    the layer's own interval, -1000 everywhere on a ray the layer misses; plus the special rows: a ray that misses the background
    box (0 .. -1000, strictly descending), a descending performer (edited box), grazing hits (mask clear, all samples at one real
    depth), exact ties between layers (a performer sample copied from the background list)."""
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand(n, l, 1, generator=g) * 3.0
    hi = lo + 0.2 + torch.rand(n, l, 1, generator=g) * 3.0
    t = torch.sort(lo + (hi - lo) * torch.rand(n, l, S, generator=g), -1)[0]
    t[:, 0] = torch.sort(torch.rand(n, S, generator=g) * 6.5 - 0.3, -1)[0]
    hitm = torch.rand(n, l, generator=g) < hit
    hitm[:, 0] = True
    t[~hitm] = -1000.0
    mask = hitm.clone()
    bk_miss = torch.rand(n, generator=g) < 0.05
    t[bk_miss, 0] = -(torch.arange(S).float() + torch.rand(int(bk_miss.sum()), S, generator=g)) * (1000.0 / S)
    mask[bk_miss, 0] = torch.rand(int(bk_miss.sum()), generator=g) < 0.5
    if l > 1:
        rev = (torch.rand(n, generator=g) < 0.05) & hitm[:, 1]
        t[rev, 1] = t[rev, 1].flip(-1) + torch.linspace(0.0, -1e-3, S)      # strictly descending
        graze = (torch.rand(n, generator=g) < 0.05) & ~hitm[:, l - 1]
        t[graze, l - 1] = (torch.rand(int(graze.sum()), 1, generator=g) * 4.0).expand(-1, S)
        if ties and S >= 3:
            tie = (torch.rand(n, generator=g) < 0.2) & hitm[:, 1] & ~rev & ~bk_miss
            k = S // 3
            t[tie, 1, k] = t[tie, 0, k].clamp(min=t[tie, 1, k - 1], max=t[tie, 1, k + 1])
    raw = torch.randn(n, l, S, 4, generator=g) * torch.tensor([2.0, 2.0, 2.0, 4.0])
    return t, raw, mask.to(torch.uint8)


# (3, 64), (3, 128): the FULL instantiations; (4, 150), (3, 17), (6, 1): ragged; (16, 64): the l = 16 mask packing
ORACLE_SHAPES = [(3, 64), (3, 128), (4, 150), (3, 17), (6, 1), (16, 64)]
# + (16, 192): two launches, more than 64 KB of LDS per workgroup, the scratch cleared by the library
ROUTE_SHAPES = ORACLE_SHAPES + [(16, 192)]
NEAR, THR, BTHR, ALPHA = 0.6, 0.4, 0.2, 0.5       # NEAR lies inside the background's depths (-0.3 .. 6.2): the :605 cut bites
ROUTES = (("staged", dict(want_order=True)), ("two_pass", dict(two_pass=True)), ("one_launch", dict(two_pass=False)))


def rays_of(l, S):
    return 3000 if l * S <= 400 else 1200 if l * S <= 2000 else 500


# ---- the oracle's configuration: every layer evaluated (test_merge_kernel_vs_oracle's), one GPU call and one CPU reference per case
@functools.lru_cache(maxsize=None)
def oracle_case(l, S, fine):
    from stnerf_amd import ops
    n = rays_of(l, S)
    t, raw, mask = scene(n, l, S, seed=31 * l + S + fine, hit=0.7 if l <= 6 else 0.35)
    sig = [raw[:, i, :, 3:].clone() for i in range(l)]
    rgb = [raw[:, i, :, :3].clone() for i in range(l)]
    for i in range(1, l):
        dead = mask[:, i] == 0
        sig[i][dead] = 0
        rgb[i][dead] = 0
    if fine:
        sig[0][sig[0] < BTHR] = 0
    for i in range(1, l):
        if not fine:
            sig[i][t[:, i].unsqueeze(-1) < 0] = 0
        sig[i][sig[i] < THR] = 0
        if fine and i == l - 1:
            sig[i] = sig[i] * ALPHA
    if not fine:
        sig[0][t[:, 0].unsqueeze(-1) < NEAR] = 0
    ts = [t[:, i].unsqueeze(-1) for i in range(l)]
    t_mix, order = torch.sort(torch.cat(ts, -2), dim=-2, stable=True)
    rgb_mix = torch.cat(rgb, -2).gather(1, order.repeat(1, 1, 3))
    sig_mix = torch.cat(sig, -2).gather(1, order)
    if fine:
        sig_mix[t_mix < NEAR] = 0
    mix = O.composite(t_mix, rgb_mix, sig_mix)
    want = torch.zeros(n, l * S).scatter_(1, order.squeeze(-1), mix[3].squeeze(-1)).reshape(n, l, S)   # back to the source index
    ok = torch.isfinite(mix[0]).all(-1) & torch.isfinite(mix[2]).all(-1)     # descending rows: inf / NaN in the reference too
    # scene_out from those weights, in fp64: layer i's sum_k w {sigmoid(rgb), t, 1} over its own samples
    w64 = want.double()
    colour = torch.sigmoid(torch.stack(rgb, 1).double())
    want_scene = torch.cat([(w64.unsqueeze(-1) * colour).sum(2), (w64 * t.double()).sum(2, keepdim=True), w64.sum(2, keepdim=True)], -1)
    got = ops.composite_scene(t.cuda(), raw.cuda(), mask.cuda(), near=NEAR, fine=fine, cut_negative_t=not fine,
                              thresholds=[BTHR if fine else None] + [THR] * (l - 1), evaluated=[2] + [1] * (l - 1),
                              sigma_scale=[1.0] * (l - 1) + [ALPHA if fine else 1.0], want_weights=True)
    return dict(ok=ok, want=want, want_scene=want_scene, got=[None if g is None else g.cpu() for g in got])


# ---- the routes' configuration: a hidden performer (real depths, no output) as well; every route, raw and activated colours
@functools.lru_cache(maxsize=None)
def route_case(l, S, fine):
    from stnerf_amd import ops
    n = rays_of(l, S)
    t, raw, mask = scene(n, l, S, seed=100 * l + S + fine, hit=0.6 if l <= 6 else 0.35)
    ev = [2] + [1] * (l - 1)
    if l > 2:
        ev[1 if l == 3 else 2] = 0          # (the generator's grazing hits are the LAST layer's: keep that one evaluated)
    kw = dict(near=NEAR, fine=fine, cut_negative_t=not fine, thresholds=[0.3 if fine else None] + [0.5] * (l - 1),
              sigma_scale=[1.0] * (l - 1) + [0.4 if fine else 1.0], evaluated=ev, want_weights=True)
    td, md = t.cuda(), mask.cuda()
    out, plain = {}, {}
    for activated in (False, True):
        r_in = raw.cuda()
        if activated:
            r_in[..., :3] = torch.sigmoid(r_in[..., :3])
        for name, route in ROUTES:
            out[name, activated] = ops.composite_scene(td, r_in, md, rgb_activated=activated, **route, **kw)
            plain[name, activated] = ops.composite(td, r_in, md, rgb_activated=activated, **route, **kw)
    torch.cuda.synchronize()
    return dict(t=t, mask=mask, ev=ev, out=out, plain=plain)


# ---- 1
@pytest.mark.parametrize("fine", [False, True])
@pytest.mark.parametrize("l, S", ORACLE_SHAPES)
def test_merged_weights_match_the_oracles_composite_of_the_sorted_union(ops, l, S, fine):
    """Expectation as in test_merge_kernel_vs_oracle: a stable torch.sort of the concatenation, the edits, O.composite; its weight
    output scattered back through the sort index.  Bar: that test's for `weights`."""
    c = oracle_case(l, S, fine)
    ok, mw = c["ok"], c["got"][3]
    print(f"kept rows {float(ok.float().mean()):.3f}, max |d| {float((mw[ok] - c['want'][ok]).abs().max()):.3e}")
    assert float(ok.float().mean()) > 0.8
    torch.testing.assert_close(mw[ok], c["want"][ok], rtol=1e-5, atol=1e-6)


# ---- 2
@pytest.mark.parametrize("fine", [False, True])
@pytest.mark.parametrize("l, S", ROUTE_SHAPES)
def test_routes_agree_bit_for_bit(ops, l, S, fine):
    c = route_case(l, S, fine)
    for activated in (False, True):
        ref = c["out"]["staged", activated]
        for name in ("two_pass", "one_launch"):
            got = c["out"][name, activated]
            for what, k in (("merged_weights", 3), ("scene", 4)):
                bad = bits(got[k]) != bits(ref[k])
                assert not bool(bad.any()), (what, name, activated, int(bad.sum()), bad.nonzero()[:5].tolist())
    multi = ((c["t"][:, :, 0] > -999).sum(1) >= 2).sum()
    assert int(multi) > c["t"].shape[0] // 4


# ---- 3
@pytest.mark.parametrize("fine", [False, True])
@pytest.mark.parametrize("l, S", ROUTE_SHAPES)
def test_the_other_outputs_carry_the_bits_of_composite(ops, l, S, fine):
    c = route_case(l, S, fine)
    for key, got in c["out"].items():
        want = c["plain"][key]
        for what, a, b in zip(("layer_out", "mixed", "weights"), got[:3], want[:3]):
            bad = bits(a) != bits(b)
            assert not bool(bad.any()), (what, key, int(bad.sum()), bad.nonzero()[:5].tolist())


# ---- 4
@pytest.mark.parametrize("fine", [False, True])
@pytest.mark.parametrize("l, S", [(3, 64), (3, 128), (4, 150), (3, 17), (16, 64)])
def test_one_live_ascending_layer_has_the_layers_own_weights(ops, l, S, fine):
    """With one live, ascending layer and no near cut the merged composite IS the layer's: same bits.  (`near` below every
    ascending list's first depth, so the fine stage's cut never bites here; where it does, test 2 holds the routes together.)"""
    n = 2000
    t, raw, mask = scene(n, l, S, seed=7 * l + S + fine, hit=0.3 if l <= 4 else 0.04)
    live = (t != -1000.0).any(-1)
    asc = (t[:, :, 1:] >= t[:, :, :-1]).all(-1)
    rows = (live.sum(1) == 1) & (live & asc).any(1)
    assert int(rows.sum()) >= n // 4, int(rows.sum())
    for name, route in ROUTES:
        _, _, w, mw, _ = ops.composite_scene(t.cuda(), raw.cuda(), mask.cuda(), near=-0.5, fine=fine, cut_negative_t=not fine,
                                             thresholds=[None] + [0.5] * (l - 1), evaluated=[2] + [1] * (l - 1), want_weights=True,
                                             **route)
        bad = bits(w.cpu()[rows]) != bits(mw.cpu()[rows])
        assert not bool(bad.any()), (name, int(bad.sum()))


# ---- 5
@pytest.mark.parametrize("fine", [False, True])
@pytest.mark.parametrize("l, S", ROUTE_SHAPES)
def test_layers_without_output_get_exact_zeros(ops, l, S, fine):
    c = route_case(l, S, fine)
    t, mask, ev = c["t"], c["mask"], c["ev"]
    evt = torch.tensor(ev)
    have = (evt == 2).unsqueeze(0) | ((evt == 1).unsqueeze(0) & (mask != 0))           # (n, l): the layer has network output
    live = have | (t != -1000.0).any(-1)
    hidden, missed, grazing = (evt == 0).expand_as(have), ~have & ~live, ~have & live & (evt != 0)
    assert int(hidden.sum()) > 0 or l <= 2
    assert int(missed.sum()) > 0 and int(grazing.sum()) > 0
    for key, got in c["out"].items():
        mw, sc = got[3].cpu(), got[4].cpu()
        assert not bool(bits(sc)[~have].any()), ("scene", key)            # all 32 bits: +0.0
        assert not bool(bits(mw)[~live].any()), ("merged_weights", key)


# ---- 6
@pytest.mark.parametrize("fine", [False, True])
@pytest.mark.parametrize("l, S", ORACLE_SHAPES)
def test_the_passes_sum_to_the_mixed_image(ops, l, S, fine):
    """sum_i scene[i] == mixed and sum_k merged_weights == mixed[..., 4], at twice the bar of `mixed` against the oracle: each side is
    an fp32 sum within that bar of the exact value."""
    c = oracle_case(l, S, fine)
    ok = c["ok"]
    _, mixed, _, mw, sc = c["got"]
    assert float(ok.float().mean()) > 0.8
    total = sc.sum(1)
    print(f"max |sum scene - mixed| {float((total[ok] - mixed[ok]).abs().max()):.3e}, "
          f"max |sum wM - acc| {float((mw.sum((1, 2))[ok] - mixed[ok][:, 4]).abs().max()):.3e}")
    torch.testing.assert_close(total[ok], mixed[ok], rtol=2e-5, atol=6e-6)
    torch.testing.assert_close(mw.sum((1, 2))[ok], mixed[ok][:, 4], rtol=2e-5, atol=6e-6)


# ---- 6b
@pytest.mark.parametrize("fine", [False, True])
@pytest.mark.parametrize("l, S", ORACLE_SHAPES)
def test_scene_out_matches_the_sums_over_the_oracles_weights(ops, l, S, fine):
    """scene_out[:, i] against sum_k w {sigmoid(rgb), t, 1} formed in fp64 from the oracle's merged weights (test 1's
    expectation), layer by layer: the sum over the layers (test 6) does not see two layers' passes swapped, nor a sample credited
    to the wrong layer.  Bar: test 6's."""
    c = oracle_case(l, S, fine)
    ok, sc, want = c["ok"], c["got"][4], c["want_scene"]
    assert sc.shape == want.shape == (ok.numel(), l, 5)
    d = (sc[ok].double() - want[ok]).abs()
    print(f"max |d| colour {float(d[..., :3].max()):.3e}, depth {float(d[..., 3].max()):.3e}, alpha {float(d[..., 4].max()):.3e}")
    torch.testing.assert_close(sc[ok], want[ok].float(), rtol=2e-5, atol=6e-6)


# ---- 7
def test_scene_out_without_merged_weights_is_refused_before_any_launch(ops):
    from stnerf_amd import hip
    n, l, S = 300, 3, 17
    t, raw, mask = scene(n, l, S, seed=1)
    td, rd, md = t.cuda(), raw.cuda(), mask.cuda()
    p = ops.composite_params(evaluated=[2, 1, 1])
    lo, mo, sc = (torch.full(s, 7.25, device="cuda") for s in ((n, l, 5), (n, 5), (n, l, 5)))
    scratch = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    rc = hip.lib().stnerf_composite_scene(hip.dptr(td), hip.dptr(rd), hip.dptr(md, torch.uint8), n, l, S, C.byref(p), hip.dptr(lo),
                                          hip.dptr(mo), None, None, hip.dptr(scratch, torch.uint8), None, hip.dptr(sc), hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == hip.EINVAL and "merged_weights" in hip.last_error()
    assert bool((lo == 7.25).all()) and bool((mo == 7.25).all()) and bool((sc == 7.25).all()) and bool((scratch == 9).all())


# ---- 8
GUARD_BYTES, PATTERN = 4096, 0x7FC00A5A            # (tests/test_gpu_canaries.py: a quiet-NaN payload no kernel produces)


def guarded(shape):
    n = 4
    for d in shape:
        n *= d
    body = (n + 255) // 256 * 256
    buf = torch.empty(body + 2 * GUARD_BYTES, dtype=torch.uint8, device="cuda")
    buf.view(torch.int32).fill_(PATTERN)
    return buf, buf[GUARD_BYTES:GUARD_BYTES + n].view(torch.float32).reshape(shape), n


def guards_intact(buf, n):
    words = buf.view(torch.int32)
    return bool((words[: GUARD_BYTES // 4] == PATTERN).all()) and bool((words[(GUARD_BYTES + n + 3) // 4:] == PATTERN).all())


@pytest.mark.parametrize("l, S, n", [(4, 150, 333), (3, 17, 1001), (16, 64, 259)])
def test_guard_words_around_the_new_outputs_survive(ops, l, S, n):
    from stnerf_amd import hip
    t, raw, mask = scene(n, l, S, seed=3 + S, hit=0.5 if l <= 4 else 0.3)
    td, rd, md = t.cuda(), raw.cuda(), mask.cuda()
    ev = [2] + [1] * (l - 1)
    ev[2] = 0
    p = ops.composite_params(near=NEAR, fine=True, thresholds=[0.3] + [0.5] * (l - 1), evaluated=ev)
    for name, route in ROUTES:
        lo, mo = torch.empty(n, l, 5, device="cuda"), torch.empty(n, 5, device="cuda")
        order = torch.empty(n, l * S, dtype=torch.int32, device="cuda") if route.get("want_order") else None
        scratch = torch.empty(n, dtype=torch.uint8, device="cuda") if route.get("two_pass") else None
        (mw_buf, mw, mw_n), (sc_buf, sc, sc_n) = guarded((n, l, S)), guarded((n, l, 5))
        rc = hip.lib().stnerf_composite_scene(hip.dptr(td), hip.dptr(rd), hip.dptr(md, torch.uint8), n, l, S, C.byref(p), hip.dptr(lo),
                                              hip.dptr(mo), None, hip.dptr(order, torch.int32), hip.dptr(scratch, torch.uint8),
                                              hip.dptr(mw), hip.dptr(sc), hip.stream_ptr())
        torch.cuda.synchronize()
        assert rc == hip.OK, hip.last_error()
        assert guards_intact(mw_buf, mw_n), f"{name}: a kernel wrote outside merged_weights"
        assert guards_intact(sc_buf, sc_n), f"{name}: a kernel wrote outside scene_out"
        assert not bool((bits(mw) == PATTERN).any()) and not bool((bits(sc) == PATTERN).any()), f"{name}: an output element was left unwritten"


# ---- 9: the pipeline.  l = 3, n1 = n2 = 16, a 16 x 16 view from 45 degrees: rays through one performer, both, and neither
H = W = 16
N1 = N2 = 16
L = 2


@functools.lru_cache(maxsize=None)
def _model():
    from stnerf_amd import synthetic as syn
    from stnerf_amd.modeling import build_layered_model
    m = types.SimpleNamespace(BOARDER_WEIGHT=1e10, SAMPLE_METHOD="BBOX", SAME_SPACENET=False, TKERNEL_INC_RAW=True,
                              POSE_REFINEMENT=False, USE_DIR=True, USE_DEFORM_VIEW=False, USE_DEFORM_TIME=True,
                              USE_SPACE_TIME=True, BKGD_USE_DEFORM_TIME=False, BKGD_USE_SPACE_TIME=False,
                              DEEP_RGB=False, COARSE_RAY_SAMPLING=N1, FINE_RAY_SAMPLING=N2)
    cfg = types.SimpleNamespace(MODEL=m, DATASETS=types.SimpleNamespace(LAYER_NUM=L))
    model = build_layered_model(cfg, camera_num=1)
    model.load_state_dict(syn.make_state_dict(L, True, True, seed=3))
    return model.cuda().eval()


def make_model(precision):
    from stnerf_amd import synthetic as syn
    model = _model()
    bk, per = syn.scene_boxes(L)
    model.set_bkgd_bbox(bk)
    model.set_bboxes(per)
    model.set_precision(precision)
    model.seed, model.fresh_draws_per_call = 11, False
    model.scale = model.shift = model.rotation = None
    model.near, model.alpha = 0, 1
    model.set_background_cache(None)
    for i in range(L + 1):
        model.show_layer(i)
    return model


def view(ops, frame_ids=(1.0, 2.5, 1.0)):
    from stnerf_amd import synthetic as syn
    K, T = syn.camera(H, W, 45.0)
    return K, T, ops.generate_rays(K, T, H, W, frame_ids=list(frame_ids))


def same_bits(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, (tuple, list)):
            same_bits(x, y, f"{what}[{k}]")
        else:
            assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
            assert torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else bits(x), y.view(torch.uint8) if y.dtype == torch.bool else bits(y)), (what, k)


def check_passes(model, rays, only_coarse, what, bthr=0.02):
    with torch.no_grad():
        ref = model.render_rays(rays, only_coarse, 0.05, bthr)
        out, sc = model.render_rays_scene(rays, only_coarse, 0.05, bthr)
    same_bits(out, ref, what)
    assert len(sc) == L + 1 and all(c.shape == (H * W, 3) and d.shape == (H * W, 1) and a.shape == (H * W, 1) for c, d, a in sc)
    final = out[1] if only_coarse else out[0]
    for j, name in enumerate(("colour", "depth", "alpha")):
        total = sum(s[j] for s in sc)
        print(f"{what}: max |sum {name} - mixed| {float((total - final[j]).abs().max()):.3e}")
        torch.testing.assert_close(total, final[j], rtol=2e-5, atol=6e-6)
    return out, sc


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_pipeline_passes(ops, precision):
    model = make_model(precision)
    K, T, rays = view(ops)
    out, sc = check_passes(model, rays, False, "fine")
    m = out[4]
    assert int((m[1] & m[2]).sum()) > 0 and int((m[1] ^ m[2]).sum()) > 0 and int((~m[1] & ~m[2]).sum()) > 0
    # with the background's fine densities cut (a threshold above them all) its pass is exact zeros, and a performer's share of
    # the mixed image never exceeds what it shows alone: in the merged list its samples' deltas can only shrink and the
    # transmittance in front of them can only fall
    out_p, sc_p = check_passes(model, rays, False, "performers only", bthr=1e9)
    assert not bool(bits(sc_p[0][2]).any()) and not bool(bits(sc_p[0][0]).any())
    for i in (1, 2):
        print(f"performer {i}: alpha alone at most {float(out_p[2][i][2].max()):.4f}, in the scene {float(sc_p[i][2].max()):.4f}, "
              f"lost to occlusion at most {float((out_p[2][i][2] - sc_p[i][2]).max()):.4f}")
        assert bool((sc_p[i][2] <= out_p[2][i][2] + 1e-5).all())
    # the coarse stage's pass when it is the final one
    _, sc_c = check_passes(model, rays, True, "only_coarse")
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(sc, sc_c))
    # a rotation set
    model.rotation = [None, 0.4, (-0.3, [0.5, 0.0, 0.0])]
    check_passes(model, rays, False, "rotated")
    model.rotation = None
    # a layer hidden: its pass is exact zeros, the others still sum to the mix
    model.hide_layer(2)
    _, sc_h = check_passes(model, rays, False, "hidden")
    assert all(not bool(bits(x).any()) for x in sc_h[2])
    model.show_layer(2)


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_pipeline_passes_with_the_background_cache(ops, precision):
    import stnerf_amd
    from stnerf_amd.bkgd_cache import view_key
    model = make_model(precision)
    K, T, rays = view(ops)
    with torch.no_grad():
        want = model.render_rays_scene(rays, False, 0.05, 0.02)
    model.set_background_cache(stnerf_amd.BackgroundCache())
    model.view_key = view_key(K, T, H, W, [1.0, 2.5, 1.0])
    try:
        with torch.no_grad():
            capture = model.render_rays_scene(rays, False, 0.05, 0.02)
            reuse = model.render_rays_scene(rays, False, 0.05, 0.02)
        s = model._bkgd_cache.stats
        assert s["captures"] >= 1 and s["hits"] >= 1, s
    finally:
        model.view_key = None
        model.set_background_cache(None)
    same_bits(reuse, capture, "reuse frame vs capture frame")
    same_bits(capture, want, "capture frame vs no cache")


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_render_pose_scene_passes(ops, precision):
    from stnerf_amd import synthetic as syn
    from stnerf_amd.render.render_pose import render_pose
    model = make_model(precision)
    K, T = syn.camera(H, W, 45.0)
    pairs, far = [(0, 1), (1, 2.5), (2, 1)], 20.0
    plain = render_pose(model, T, K, H, W, pairs, far, 0.05, 0.02)
    got = render_pose(model, T, K, H, W, pairs, far, 0.05, 0.02, scene_passes=True)
    assert len(plain) == 4 and len(got) == 5
    same_bits(got[:4], plain, "render_pose")
    passes = got[4]
    assert sorted(passes) == ["alpha_scene", "color_scene", "depth_scene"]
    for key, ch in (("color_scene", 3), ("alpha_scene", 1), ("depth_scene", 1)):
        assert len(passes[key]) == L + 1 and all(x.shape == (H, W, ch) and x.is_cuda for x in passes[key])
    torch.testing.assert_close(sum(passes["color_scene"]), got[0], rtol=2e-5, atol=6e-6)


# ---- 10
def test_render_rays_scene_refusals(ops, monkeypatch):
    from stnerf_amd import parallel
    model = make_model("bf16x3")
    _, _, rays = view(ops)
    model.train()
    try:
        with pytest.raises(RuntimeError, match="training mode"):
            model.render_rays_scene(rays)
    finally:
        model.eval()
    # a view sharded over two ranks (a stand-in process group: nothing is rendered, the call must refuse first)
    monkeypatch.setattr(parallel.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(parallel.dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(parallel.dist, "get_rank", lambda group=None: 0)
    model.shard_views = True
    try:
        with torch.no_grad(), pytest.raises(RuntimeError, match="scene.*gather mode"):
            model.render_rays_scene(rays)
    finally:
        model.shard_views = False
