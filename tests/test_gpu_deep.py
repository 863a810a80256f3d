"""Deep frames on the GPU (include/stnerf.h / DESIGN.md sections 4.2 and 7; csrc/deep.hip), on the shapes and hand-made inputs of
tests/test_gpu_occluder.py:
1. deep_count / deep_offsets / deep_fill bit for bit against the numpy restatement (tests/deep_common.py) for four (w_min,
   merge_dz) and both rgb_activated settings, canaries round every output, overflow at capacity == total and total - 1.  Without
   rgb_activated the colours are the kernel's hardware sigmoid, which numpy does not have: its bits are taken from the shipped
   stnerf_scene_occluder on one-sample rays of weight 1 (``kernel_sigmoid``) and fed to the restatement.
2. deep_composite bit for bit against the numpy restatement for E in {0, 1, 2, 8}, the rows over the occluder test's a x z table;
   against fp64 sums under gamma sum |x|; tied to composite_scene's mixed_out / scene_out (flatten) and to stnerf_scene_occluder
   (E = 1) on the same buffers under the same kind of bound; with w_min > 0 the flatten against mixed_out within the dropped mass.
3. ``ops.render_rays(deep=)`` through the model bit for bit the chain composite_scene -> deep_count / deep_offsets / deep_fill on
   the chain's own buffers: plain, only_coarse, a sample-culling grid, termination, a background cache in CAPTURE then REUSE; no
   option = no new launch, no changed bit, the same workspace; the oracle case under ``assert_matches_oracle`` with deep on.
4. One 32 x 24 ``render_pose(deep=)`` frame: save / load round-trips, a two-element stack equals ``ops.deep_composite``.
Needs an MI355X: `pytest -m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import deep_common as DC
import occluder_common as OCL
import occupancy_common as OCC
import scene_edits_common as S
import test_gpu_bkgd_cache as BC
import test_gpu_scene_edits_oracle as SE
from pipeline_chain import assert_pairs_equal, bits, cu, detach_models, np_bits, same_bits, with_chain
from stnerf_amd import hip, ops, parallel, synthetic as syn
from stnerf_amd.deep import DeepFrame, DeepSpec
from test_gpu_occluder import A_VALUES, POISON, PAD, Z_KINDS, kernel_inputs, np_same, padded
from test_gpu_occupancy import attach

pytestmark = pytest.mark.gpu

F = np.float32
U = DC.U
CONFIGS = [(0.0, 0.0), (1e-3, 0.0), (0.0, 0.25), (1e-3, 0.25)]


@pytest.fixture(autouse=True)
def detach():
    yield
    detach_models()


def deep_inputs(n, l, S_, seed):
    """tests/test_gpu_occluder.py's hand-made inputs (ties across layers, a NaN depth, masks with cleared bits, evaluated 2, 1, 0,
    1) with the merged weights, of the order of 1 / S, sprinkled with exact zeros, a few weights at and next to 1e-3, and a NaN."""
    d = kernel_inputs(n, l, S_, seed)
    g = np.random.default_rng(seed + 7)
    wm = d["wm"].copy()
    wm[g.random(wm.shape) < 0.3] = 0.0
    pick = g.random(wm.shape)
    wm[pick < 0.03] = F(1e-3)                                     # w == w_min is dropped
    wm[(pick >= 0.03) & (pick < 0.05)] = np.nextafter(F(1e-3), F(1))
    if n > 1:
        wm[1, 0, S_ // 3] = np.nan                                # a NaN weight is kept
    if n > 4:
        wm[4] = 0.0                                               # a ray with nothing kept
    d["wm"] = wm
    return d


def canary_ok(whole):
    w = whole.view(torch.int32)
    return bool((w[:PAD] == POISON).all()) and bool((w[-PAD:] == POISON).all())


def run_list(d, w_min, merge_dz, rgb_activated, capacity=None):
    """count -> offsets -> fill through ``ops`` on canaried buffers -> (counts, offsets, records, total, written (capacity,) bool)."""
    t, raw, mask, wm = cu(d["t"]), cu(d["raw"]), cu(d["mask"], torch.uint8), cu(d["wm"])
    n, l, S_ = t.shape
    kw = dict(w_min=w_min, merge_dz=merge_dz, rgb_activated=rgb_activated, evaluated=d["evaluated"])
    cbuf = torch.full((n + 2 * PAD,), POISON, dtype=torch.int32, device="cuda")
    counts = ops.deep_count(t, mask, wm, counts=cbuf[PAD:PAD + n], **kw)
    obuf = torch.full((n + 1 + 2 * PAD,), POISON, dtype=torch.int64, device="cuda")
    offsets = ops.deep_offsets(counts, l * S_, offsets=obuf[PAD:PAD + n + 1])
    torch.cuda.synchronize()
    total = int(offsets[-1])
    cap = total if capacity is None else capacity
    sbuf, samples = padded((max(cap, 1), 8))
    samples = samples[:cap]
    tot = torch.full((3,), POISON, dtype=torch.int64, device="cuda")
    ops.deep_fill(t, raw, mask, wm, offsets, samples, total=tot[1:2], **kw)
    torch.cuda.synchronize()
    assert bool((cbuf[:PAD] == POISON).all()) and bool((cbuf[-PAD:] == POISON).all()), "counts: a canary was overwritten"
    assert bool((obuf[:PAD] == POISON).all()) and bool((obuf[-PAD:] == POISON).all()), "offsets: a canary was overwritten"
    assert canary_ok(sbuf), "samples: a canary was overwritten"
    assert int(tot[0]) == POISON and int(tot[2]) == POISON
    written = ~(samples.view(torch.int32) == POISON).all(1).cpu().numpy()
    return counts.cpu().numpy(), offsets.cpu().numpy(), samples.cpu().numpy(), int(tot[1]), written


def kernel_sigmoid(rgb):
    """The colours the compositor's sample edit makes of raw rgb WITHOUT rgb_activated -- the hardware exponential and reciprocal,
    which numpy does not have -- bit for bit, from the shipped ``stnerf_scene_occluder``: every sample is a ray of its own with l = 1,
    S = 1, wM = 1 and depth 0, under a present row at z = 1, so that front[0:3] = 0 + 1 * sigmoid(rgb) and the wave scan adds zeros."""
    rgb = np.asarray(rgb, F)
    m = rgb.size // 3
    raw = torch.zeros(m, 1, 1, 4, device="cuda")
    raw[:, 0, 0, 0:3] = cu(rgb.reshape(m, 3))
    z = lambda *s: torch.zeros(*s, device="cuda")
    row = z(m, 5)
    row[:, 3], row[:, 4] = 1.0, 1.0
    front = ops.scene_occluder(z(m, 1, 1), raw, None, torch.ones(m, 1, 1, device="cuda"), z(m, 1, 5), z(m, 5), row, rgb_activated=False,
                               evaluated=[1], want_scene=False, want_share=False, want_front_behind=True)[3]
    torch.cuda.synchronize()
    out = front[:, 0, 0:3].cpu().numpy().reshape(rgb.shape)
    assert ((out > 0) & (out < 1)).all() and np.abs(out - 1 / (1 + np.exp(-rgb.astype(np.float64)))).max() < 1e-6
    return out


# ---------------------------------------------------------------------------------------- 1. the list
@pytest.mark.parametrize("S_", [3, 64, 65, 192])
@pytest.mark.parametrize("l", [1, 3, 4])
@pytest.mark.parametrize("n", [1, 5, 70])
def test_deep_list_kernels(n, l, S_):
    d = deep_inputs(n, l, S_, seed=1000 * n + 10 * l + S_)
    sig = kernel_sigmoid(d["raw"][..., 0:3])
    for w_min, merge_dz in CONFIGS:
        want_c, want_o, want_r = DC.np_deep(d["t"], d["wm"], d["raw"][..., 0:3], d["have"], w_min, merge_dz)
        want_sig = DC.np_deep(d["t"], d["wm"], sig, d["have"], w_min, merge_dz)[2]
        for rgb_activated in (True, False):
            what = f"n={n} l={l} S={S_} w_min={w_min} merge_dz={merge_dz} rgb_activated={rgb_activated}"
            counts, offsets, rec, total, written = run_list(d, w_min, merge_dz, rgb_activated)
            assert np.array_equal(counts, want_c), what
            assert np.array_equal(offsets, want_o) and total == int(want_o[-1]) == rec.shape[0], what
            assert written.all(), f"{what}: a record was not written"
            want = want_r if rgb_activated else want_sig
            assert np_same(rec, want), f"{what}: the records differ from the numpy restatement"
        if n == 70 and l == 4 and S_ == 192:            # the cases bite: drops, merges, a NaN weight kept, an empty ray
            kept_all = int((~(d["wm"] <= 0) & d["have"][:, :, None]).sum())
            assert want_c[4] == 0 and 0 < want_o[-1] <= kept_all
            if merge_dz > 0:
                assert DC.meta_of(want_r)[2].max() > 1 and want_o[-1] < kept_all
            if w_min > 0:
                assert want_o[-1] < DC.np_deep(d["t"], d["wm"], d["raw"][..., 0:3], d["have"], 0.0, merge_dz)[1][-1]


@pytest.mark.parametrize("n,l,S_", [(5, 3, 65), (70, 4, 64)])
def test_deep_fill_overflow_is_detected_and_leaves_the_rays_past_capacity_unwritten(n, l, S_):
    d = deep_inputs(n, l, S_, seed=n + S_)
    for w_min, merge_dz in ((0.0, 0.0), (1e-3, 0.25)):
        _, offsets, want, total, _ = run_list(d, w_min, merge_dz, True)
        assert total > 1
        _, _, rec, tot, written = run_list(d, w_min, merge_dz, True, capacity=total)              # it fits
        assert tot == total and written.all() and np_same(rec, want)
        counts = np.diff(offsets)
        k = int(np.flatnonzero((counts >= 2) & (offsets[:-1] > 0))[0])                            # a later ray cut in the middle of its records
        for cap in (total - 1, int(offsets[k]) + 1):
            _, _, rec, tot, written = run_list(d, w_min, merge_dz, True, capacity=cap)
            assert tot == total, "deep_total must hold the needed total whatever the capacity"
            fits = np.repeat(offsets[1:] <= cap, counts)[:cap]                                    # the record's ray ends within the capacity
            assert np.array_equal(written, fits) and fits.any()
            assert np_same(rec[fits], want[:cap][fits])
        assert not fits.all()


def test_deep_argument_errors():
    n, l, S_ = 4, 3, 8
    z = lambda *s: torch.zeros(*s, device="cuda")
    t, raw, wm = z(n, l, S_), z(n, l, S_, 4), z(n, l, S_)
    for bad in (dict(w_min=-1.0), dict(w_min=float("nan")), dict(merge_dz=-0.5), dict(merge_dz=float("nan"))):
        with pytest.raises(ValueError, match="negative or NaN"):
            ops.deep_count(t, None, wm, **bad)
    with pytest.raises(ValueError, match="S <= 256"):
        ops.deep_count(z(1, 1, 257), None, z(1, 1, 257))
    with pytest.raises(ValueError, match="bad shape"):
        ops.deep_count(z(n, 17, S_), None, z(n, 17, S_))
    counts = ops.deep_count(t, None, wm)
    with pytest.raises(ValueError, match="2\\^31"):
        ops.deep_offsets(counts, 1 << 30)
    with pytest.raises(ValueError, match="workspace"):
        ops.deep_offsets(counts, l * S_, workspace=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    offsets = ops.deep_offsets(counts, l * S_)
    off = torch.zeros(n * l * S_ * 4 + 1, device="cuda")[1:].view(n, l, S_, 4)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.deep_fill(t, off, None, wm, offsets, z(4, 8))
    with pytest.raises(ValueError, match="E = 9"):
        ops.deep_composite(offsets, z(0, 8), l, z(n, 9, 5))
    mixed, scene, shares = ops.deep_composite(offsets, z(0, 8), l, z(n, 2, 5))                    # no sample, no present row
    torch.cuda.synchronize()
    assert not bits(mixed).any() and not bits(scene).any() and not bits(shares).any()


# ---------------------------------------------------------------------------------------- 2. the composite
def element_rows(d, E, seed):
    """(n,E,5) rows over the occluder test's a x z table, z kinds resolved on the ray's own depths; slot pairs tied in z."""
    g = np.random.default_rng(seed)
    n, l, S_ = d["t"].shape
    combos = [(a, z) for z in Z_KINDS for a in A_VALUES]
    el = np.zeros((n, E, 5), F)
    el[..., 0:3] = g.random((n, E, 3))
    for r in range(n):
        lo, hi = np.nanmin(d["t"][r]), np.nanmax(d["t"][r])
        for e in range(E):
            a, kind = combos[(r * E + e * 5 + seed) % len(combos)]
            exact = d["t"][r, min(1, l - 1), min(S_ - 1, 1 + (r + e) % S_)]
            z = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "exact": d["t"][r, 0, 0] if np.isnan(exact) else exact,
                 "below": lo - 0.5, "above": hi + 0.5, "middle": lo + (hi - lo) * (e + 1) / (E + 1)}[kind]
            el[r, e, 3], el[r, e, 4] = a, z
        if E >= 2 and r % 3 == 0:                                   # a tie in z between two present rows: stable by index
            el[r, 1, 3:5] = 0.5, d["t"][r, 0, S_ // 2]
            el[r, 0, 3:5] = 0.25, d["t"][r, 0, S_ // 2]
    el[..., 0:3][np.isnan(el[..., 4])] = np.nan                     # an absent row's words are never read into a result
    return el


def run_composite(offsets, rec, l, el):
    """``ops.deep_composite`` -> numpy (mixed, scene, shares | None); the canaries are the allocator's: outputs made by ops."""
    e = None if el is None else cu(el)
    mixed, scene, shares = ops.deep_composite(cu(offsets, torch.int64), cu(rec) if rec.shape[0] else torch.zeros(0, 8, device="cuda"), l, e)
    torch.cuda.synchronize()
    return mixed.cpu().numpy(), scene.cpu().numpy(), None if shares is None else shares.cpu().numpy()


def run_composite_canaried(offsets, rec, l, el):
    n, E = offsets.shape[0] - 1, el.shape[1]
    bufs = {k: padded(s) for k, s in dict(mixed=(n, 5), scene=(n, l, 5), shares=(n, E, 5)).items()}
    o, r, e = cu(offsets, torch.int64), cu(rec), cu(el)
    hip.check(hip.lib().stnerf_deep_composite(hip.dptr(o, torch.int64), hip.dptr(r), n, l, hip.dptr(e), E, hip.dptr(bufs["mixed"][1]),
                                              hip.dptr(bufs["scene"][1]), hip.dptr(bufs["shares"][1]), hip.stream_ptr()), "stnerf_deep_composite")
    torch.cuda.synchronize()
    for k, (whole, view) in bufs.items():
        assert canary_ok(whole), f"{k}: a canary was overwritten"
        assert not bool((view.contiguous().view(torch.int32) == POISON).any()), f"{k}: an element was not written"
    return tuple(bufs[k][1].cpu().numpy() for k in ("mixed", "scene", "shares"))


@pytest.mark.parametrize("S_", [3, 64, 65, 192])
@pytest.mark.parametrize("l", [1, 3, 4])
@pytest.mark.parametrize("n", [1, 5, 70])
def test_deep_composite_kernel(n, l, S_):
    d = deep_inputs(n, l, S_, seed=1000 * n + 10 * l + S_)
    colour = d["raw"][..., 0:3]
    for w_min, merge_dz in ((0.0, 0.0), (1e-3, 0.25)):
        _, offsets, rec = DC.np_deep(d["t"], d["wm"], colour, d["have"], w_min, merge_dz)
        for E in (0, 1, 2, 8):
            what = f"n={n} l={l} S={S_} w_min={w_min} merge_dz={merge_dz} E={E}"
            el = element_rows(d, E, seed=E + n) if E else None
            want = DC.np_deep_composite(offsets, rec, l, el)
            got = run_composite_canaried(offsets, rec, l, el) if E and rec.shape[0] else run_composite(offsets, rec, l, el)
            for name, g_, w_ in zip(("mixed", "scene", "shares"), got, want):
                if g_ is not None:
                    assert np_same(g_, w_), f"{what}: {name} differs from the numpy restatement"
            # against fp64 at the same rows: a pass is a sum of m rounded products q x in some order, gamma(m) sum |x| (q <= 1, its
            # own product chain of E factors adds E u); the mix adds l + E terms; a share is four rounded operations on Af, itself a sum
            exact_mixed, exact_scene, exact_shares, mag = DC.exact_deep_composite(offsets, rec, l, el)
            m = np.diff(offsets).max(initial=0)
            per = np.nan_to_num((DC.gamma(m) + (E + 1) * U) * mag, nan=np.inf)           # (a NaN weight on the ray: nothing to hold)
            nan = np.isnan(exact_scene)
            assert np.array_equal(np.isnan(got[1]), nan), what
            worst = np.max(np.where(nan, -np.inf, np.abs(got[1] - exact_scene) - per[:, None, :]), initial=-np.inf)
            assert worst <= 0.0, (what, "scene", worst)
            if E:
                ap = np.stack([DC.np_rows(el[r])[0] for r in range(n)])
                rows_mag = np.abs(np.where((ap > 0)[..., None], np.concatenate([el[..., 0:3], el[..., 4:5], np.ones((n, E, 1), F)], -1), 0))
                share_bound = np.nan_to_num((DC.gamma(m) * (1 + mag[:, 4])[:, None, None] + (E + 4) * U) * rows_mag, nan=np.inf)
                nan_s = np.isnan(exact_shares)
                assert np.array_equal(np.isnan(got[2]), nan_s), what
                worst = np.max(np.where(nan_s, -np.inf, np.abs(got[2] - exact_shares) - share_bound), initial=-np.inf)
                assert worst <= 0.0, (what, "shares", worst)
                nan_m = np.isnan(exact_mixed)
                total = np.nan_to_num(per * (1 + (l + E) * U) + share_bound.sum(1) + (l + E) * U * (np.abs(exact_scene).sum(1) + np.abs(exact_shares).sum(1)), nan=np.inf)
                assert np.array_equal(np.isnan(got[0]), nan_m), what
                worst = np.max(np.where(nan_m, -np.inf, np.abs(got[0] - exact_mixed) - total), initial=-np.inf)
                print(f"{what}: largest |mixed - exact| - bound = {worst:.3e}")
                assert worst <= 0.0, (what, "mixed", worst)


@pytest.mark.parametrize("n,l,S_", [(5, 1, 3), (70, 3, 65), (70, 4, 192)])
def test_deep_composite_ties_to_the_scene_pass_and_to_the_occluder(n, l, S_):
    """A real composite's merged weights: at w_min = 0, merge_dz = 0 the flatten is mixed_out / scene_out and E = 1 is
    stnerf_scene_occluder, each up to the order of the sums: both sides sum the same S rounded products per layer, so they differ
    by at most 2 gamma(S) sum |w x| per pass (gamma: the bound tests/test_gpu_occluder.py uses), plus the mix's few operations."""
    d = kernel_inputs(n, l, S_, seed=1000 * n + 10 * l + S_)
    t, raw, mask = cu(d["clean"]), cu(d["raw"]), cu(d["mask"], torch.uint8)
    _, mixed, _, merged, scene = ops.composite_scene(t, raw, mask, fine=True, evaluated=d["evaluated"], rgb_activated=True)
    kw = dict(rgb_activated=True, evaluated=d["evaluated"])
    wm = merged.cpu().numpy()
    x = np.concatenate([d["raw"][..., 0:3], d["clean"][..., None], np.ones_like(d["clean"])[..., None]], -1).astype(np.float64)
    wx = np.where(d["have"][:, :, None, None], np.abs(wm.astype(np.float64)[..., None] * x), 0.0)     # (n,l,S,5)
    g = DC.gamma(S_)
    for w_min in (0.0, 1e-3):
        counts = ops.deep_count(t, mask, merged, w_min=w_min, **kw)
        offsets = ops.deep_offsets(counts, l * S_)
        torch.cuda.synchronize()
        samples = torch.empty(int(offsets[-1]), 8, device="cuda")
        ops.deep_fill(t, raw, mask, merged, offsets, samples, w_min=w_min, **kw)
        flat_mixed, flat_scene, _ = ops.deep_composite(offsets, samples, l)
        torch.cuda.synchronize()
        # the dropped mass per channel, from the inputs: the samples with wM <= w_min
        dropped = np.where((wm <= w_min)[..., None], wx, 0.0).sum(2)                                  # (n,l,5)
        bound_scene = 2 * g * wx.sum(2) + dropped
        diff = np.abs(flat_scene.cpu().numpy().astype(np.float64) - scene.cpu().numpy())
        assert (diff <= bound_scene).all(), (w_min, float((diff - bound_scene).max()))
        # (mixed_out is one sum of the ray's l S products, gamma(l S); the flatten sums l passes, one rounding each)
        bound_mixed = (DC.gamma(l * S_) + g + (l + 1) * U) * wx.sum((1, 2)) + dropped.sum(1)
        diff = np.abs(flat_mixed.cpu().numpy().astype(np.float64) - mixed.cpu().numpy())
        assert (diff <= bound_mixed).all(), (w_min, float((diff - bound_mixed).max()))
        if w_min > 0:
            assert S_ < 64 or dropped.max() > 0        # (at S = 3 every weight is far above the threshold)
            continue
        occ = cu(d["occ"])
        o_mixed, o_scene, o_share, _, _ = ops.scene_occluder(t, raw, mask, merged, scene, mixed, occ, **kw)
        c_mixed, c_scene, c_share = ops.deep_composite(offsets, samples, l, occ[:, None, :].contiguous())
        torch.cuda.synchronize()
        _, present = OCL.np_present(d["occ"])
        diff = np.abs(c_scene.cpu().numpy().astype(np.float64) - o_scene.cpu().numpy())[present]
        assert (diff <= (bound_scene + 2 * U * wx.sum(2))[present]).all(), float((diff - bound_scene[present]).max())
        # the share: a' T {r, g, b, z, 1}, T = 1 - Af, Af a sum of the front weights in two orders: |dT| <= 2 gamma(l S) sum w
        rows = np.abs(np.concatenate([d["occ"][:, 0:3], d["occ"][:, 4:5], np.ones((n, 1), F)], 1)).astype(np.float64)
        bound_share = (2 * DC.gamma(l * S_) * wx[..., 4].sum((1, 2)) + 6 * U)[:, None] * rows
        diff = np.abs(c_share.cpu().numpy()[:, 0].astype(np.float64) - o_share.cpu().numpy())[present]
        assert (diff <= bound_share[present]).all(), float((diff - bound_share[present]).max())
        diff = np.abs(c_mixed.cpu().numpy().astype(np.float64) - o_mixed.cpu().numpy())[present]
        bound_occ = bound_scene.sum(1) + bound_share + 2 * (l + 2) * U * (wx.sum((1, 2)) + rows)
        assert (diff <= bound_occ[present]).all(), float((diff - bound_occ[present]).max())
        absent = ~present                                          # an absent row: the flatten, bit for bit
        assert np.array_equal(np_bits(c_mixed.cpu().numpy()[absent]), np_bits(flat_mixed.cpu().numpy()[absent]))
        assert not np_bits(c_share.cpu().numpy()[absent]).any()


# ---------------------------------------------------------------------------------------- 3. the pipeline is the chain
def assert_pairs(pairs, what, pieces):
    """The six outputs against the chain (tests/pipeline_chain.py), then the deep list against deep_count -> deep_offsets ->
    deep_fill on the buffers the chain's final composite_scene took and returned."""
    assert_pairs_equal(pairs, what, pieces)
    for piece, (got, chain) in enumerate(pairs):
        assert len(got) == 9 and chain.launch.get("background_id") is None
        offsets, samples = chain.deep
        total = int(got[8])
        assert torch.equal(got[6], offsets) and total == samples.shape[0] > 0, f"{what}: piece {piece}: the offsets differ from the chain's"
        assert same_bits(got[7][:total], samples), f"{what}: piece {piece}: the records differ from deep_fill on the chain's buffers"


def deep_render(model, case, rays, spec=None, **kw):
    with torch.no_grad():
        out = model.render_rays_deep(rays, spec, case["only_coarse"], case["thr"], case["bthr"], ref_chunk=case["chunk"], **kw)
    torch.cuda.synchronize()
    return out


PIECES = (S.N + S.CAP - 1) // S.CAP
TAU = 1e-3


@pytest.mark.parametrize("variant", ["plain", "only_coarse", "grid", "terminated"])
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_pipeline_is_the_chain_of_op_level_entries(monkeypatch, precision, variant):
    case = OCC.plain_case(only_coarse=variant == "only_coarse")
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case, precision)
    l = model.total_layers
    flags, tau = [False] * l, 0.0
    if variant == "grid":
        attach(model, OCC.manual_grids(case, "half_x", 0, layers=(1,)), samples=True)
    if variant == "terminated":
        model.set_termination(TAU, layers=[1, 2], background=True)
        flags, tau = [True, True, True, False], TAU
    pairs = []
    with_chain(model, monkeypatch, pairs, flags, tau)
    spec = DeepSpec(1e-4, 0.25) if variant == "plain" else DeepSpec()
    _, scene, frame = deep_render(model, case, rays, spec)
    assert_pairs(pairs, f"{precision} {variant}", PIECES)
    # the frame is the pieces' lists joined: its flatten is the scene pass up to the dropped mass (exactly the records' sum)
    assert frame.offsets.shape[0] == S.N + 1 and int(frame.offsets[-1]) == frame.samples.shape[0] == sum(p[1].deep[1].shape[0] for p in pairs)
    joined = torch.cat([p[1].deep[1] for p in pairs])
    assert same_bits(frame.samples, joined)
    st = frame.stats()
    assert st["samples"] == frame.samples.shape[0] and st["max"] <= l * (case["n1"] + (0 if case["only_coarse"] else case["n2"]))
    assert sum(st["histogram"]) == S.N and st["bytes"] == 32 * st["samples"] + 8 * (S.N + 1)


def test_pipeline_is_the_chain_with_a_background_cache(monkeypatch):
    """CAPTURE then REUSE through ``parallel.render_view(deep=)``, which sets the view key the cache needs."""
    model = BC.make_model(2)
    assert model._bkgd_cache is not None
    K, T = syn.camera(BC.H, BC.W, 15.0)
    pairs = []
    with_chain(model, monkeypatch, pairs)
    frames = []
    for fids in (BC.fids(True, 2, (1.0, 1.0)), BC.fids(True, 2, (2.5, 3.0))):
        out = parallel.render_view(model, K, T, BC.H, BC.W, fids, chuncks=BC.CHUNK, deep=DeepSpec())
        torch.cuda.synchronize()
        frames.append(out[-1])
    assert BC.stats(model)[0] == BC.PIECES and BC.stats(model)[2] == BC.PIECES
    assert_pairs(pairs, "background cache: capture + reuse frames", 2 * BC.PIECES)
    assert (frames[0].H, frames[0].W) == (BC.H, BC.W) and not torch.equal(frames[0].offsets, frames[1].offsets)


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_no_deep_option_changes_no_bit_no_launch_and_no_workspace(precision):
    case = OCC.plain_case()
    rays = S.case_rays(case).cuda()
    model = SE.make_model(case, precision)
    l = model.total_layers

    def records(render):
        model._workspace = None
        ops.profile_begin()
        out = render()
        torch.cuda.synchronize()
        return out, ops.profile_end()
    new = lambda recs: [r for r in recs if r["kernel"].startswith("deep_")]

    def scene_render():
        with torch.no_grad():
            return S.flat(model.render_rays_scene(rays, False, case["thr"], case["bthr"], ref_chunk=case["chunk"]))
    plain, recs = records(scene_render)
    bytes_plain = model._workspace.numel()
    assert recs and not new(recs)
    out, recs1 = records(lambda: deep_render(model, case, rays))
    assert model._workspace.numel() == bytes_plain == hip.lib().stnerf_render_workspace_bytes(S.CAP, l, case["n1"], case["n2"], 0)
    got = S.flat((out[0], out[1]))
    for k in got:                                                  # the 5-tuple and the scene passes: the bits of render_rays_scene
        assert torch.equal(got[k], plain[k]) if got[k].dtype == torch.bool else same_bits(got[k], plain[k]), k
    added = new(recs1)
    assert [r["kernel"] for r in added] == ["deep_count", "deep_offsets", "deep_fill"] * PIECES
    assert [r["kernel"] for r in recs1 if r not in added] == [r["kernel"] for r in recs]
    # an all-zero deep record is "no feature" too, and both record sizes give the plain workspace
    opts = hip.RenderOptionsDeep()
    assert opts.struct_size == C.sizeof(hip.RenderOptionsDeep) > C.sizeof(hip.RenderOptions)
    assert hip.lib().stnerf_render_workspace_bytes_opts(S.CAP, l, case["n1"], case["n2"], 0, opts.ref()) == bytes_plain
    # an explicit capacity that overflows is an error that names the needed total
    need = int(out[2].offsets[:S.CAP + 1][-1])
    with pytest.raises(RuntimeError, match=f"needs {need} deep records"):
        deep_render(model, case, rays, capacity=need - 1)
    with pytest.raises(ValueError, match="scene"):
        ops.render_rays(rays[:4], torch.zeros(l, 8, 3, device="cuda"), hip.Nets(), hip.RenderParams(l=l), torch.zeros(8, dtype=torch.uint8, device="cuda"),
                        deep=dict())


def test_a_multi_piece_deep_render_holds_one_piece_buffer_at_a_time():
    """The worst-case record buffer of a launch piece goes back to the allocator once its records are copied: the peak of a render of
    many pieces stays near ONE piece's buffer plus the frame's own list, not the sum over the pieces."""
    case = OCC.plain_case()
    model = SE.make_model(case)
    model.replay = None                                            # (more rays than the case's replayed draws cover)
    l, ns = model.total_layers, case["n1"] + case["n2"]
    rays = S.case_rays(case).cuda().repeat(16, 1)                  # 6256 rays: 49 pieces of 128
    pieces = (rays.shape[0] + S.CAP - 1) // S.CAP
    one = S.CAP * l * ns * 32
    deep_render(model, case, rays[:S.CAP])                         # (workspace and packed networks exist)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = deep_render(model, case, rays)
    peak = torch.cuda.max_memory_allocated() - base
    held = out[2].samples.numel() * 4 + out[2].offsets.numel() * 8
    assert pieces >= 40 and held <= pieces * one
    # the frame's list twice (the pieces' copies and their concatenation), two piece buffers of slack, the standard outputs
    small = rays.shape[0] * (5 + 5 + 3 * 5 * l + l) * 4 * 2 + (4 << 20)
    print(f"peak {peak / 2**20:.1f} MiB, one piece buffer {one / 2**20:.1f} MiB, all pieces {pieces * one / 2**20:.1f} MiB, list {held / 2**20:.1f} MiB")
    assert peak <= 2 * held + 2 * one + small, (peak, held, one)
    assert held + 2 * one + small < pieces * one                   # (kept buffers would peak at pieces * one + held or more: above the bound)


@functools.lru_cache(maxsize=None)
def oracle_refs():
    case = OCL.oracle_case()
    rays = S.case_rays(case)
    return case, rays, S.oracle_render(case, rays), S.oracle_render(case, rays, torch.float64)


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_oracle_with_deep_on(precision):
    """The oracle case under ``scene_edits_common.assert_matches_oracle`` as it is, rendered with deep output on; and the deep
    frame's flatten against the same call's mixed image within the bound of a sum of l S products in another order."""
    case, rays, r32, r64 = oracle_refs()
    model = SE.make_model(case, precision)
    out = deep_render(model, case, rays.cuda())
    plain = S.flat((out[0], out[1]))
    drop = lambda d: {k: v for k, v in d.items() if k != "t_coarse"}
    S.assert_matches_oracle(plain, drop(r32), drop(r64), False, f"deep on, {precision}")
    mixed, scene = out[2].flatten()
    torch.cuda.synchronize()
    ns, l = case["n1"] + case["n2"], model.total_layers
    got = torch.cat(out[0][0], -1).cpu().numpy().astype(np.float64)
    far = 10.0                                                     # (the depths of the case lie below it: |x| <= far in every channel)
    assert float(torch.cat(out[0][0], -1)[:, 3].max()) < far
    bound = 2 * DC.gamma(l * ns) * far + 2 * (l + 1) * U * far     # sum wM <= 1
    assert (np.abs(mixed.cpu().numpy().astype(np.float64) - got) <= bound).all()


# ---------------------------------------------------------------------------------------- 4. a frame
def test_render_pose_deep_frame_round_trips_and_composites_a_stack(tmp_path):
    from stnerf_amd.render.render_pose import render_pose
    H, W = 24, 32
    case = OCC.plain_case(chunk=S.N, thr=1e-4, bthr=0.0)
    ids, far = case["groups"][0][1], 20.0
    K, T = syn.camera(H, W, case["orbit"])
    model = SE.make_model(case)
    model.replay = None             # (the case's replayed draws are per ray of ITS 17 x 23 view: this frame has more rays, so the device RNG draws)
    l = model.total_layers
    color, dimg, color_layer, depth_layer, passes = render_pose(model, T, K, H, W, list(enumerate(ids)), far, 0.05, 0.02, deep=DeepSpec())
    torch.cuda.synchronize()
    frame = passes["deep"]
    assert sorted(passes) == ["deep"] and isinstance(frame, DeepFrame) and (frame.H, frame.W, frame.layers, frame.far) == (H, W, l, far)
    assert frame.offsets.shape[0] == H * W + 1 and frame.samples.shape[0] == int(frame.offsets[-1]) > H * W
    path = str(tmp_path / "frame.npz")
    frame.save(path)
    back = DeepFrame.load(path, device="cuda")
    assert torch.equal(back.offsets, frame.offsets) and same_bits(back.samples, frame.samples)
    assert (back.H, back.W, back.layers, back.far) == (H, W, l, far)
    # a title card in front of a half-transparent prop
    g = torch.Generator().manual_seed(3)
    el = torch.rand(H, W, 2, 5, generator=g)
    el[..., 0, 3], el[..., 0, 4] = 0.5, 4.0
    el[..., 1, 3], el[..., 1, 4] = 1.0, 2.5
    el[: H // 2, :, 1, 3] = 0.0                                     # the card covers the lower half only
    mixed, scene, shares = back.composite(el)
    want = ops.deep_composite(frame.offsets, frame.samples, l, el.reshape(H * W, 2, 5).cuda().contiguous())
    torch.cuda.synchronize()
    for g_, w_ in zip((mixed, scene, shares), want):
        assert same_bits(g_, w_)
    assert not bits(shares[: H // 2 * W, 1]).any() and float(shares[H // 2 * W:, 1, 4].min()) > 0
    with pytest.raises(ValueError, match="not one sample list per pixel"):
        render_pose(model, T, K, H, W, list(enumerate(ids)), far, deep=DeepSpec(), accumulate=dict(passes=2))
