"""Depth-tested occluder compositing on the GPU (include/stnerf.h / DESIGN.md sections 4.2 and 7; csrc/occluder.hip):
1. scene_occluder_kernel bit for bit: front / behind against the scene pass of a real composite where z lies beyond / below every
   depth, absent rows as copies, the mix against the numpy restatement applied to the kernel's own front / behind, canaries around
   every output, NULL optional outputs, the argument errors; and at a general z against the sums in fp64 under the rounding bound
   of a sum in any order.
2. occluder_stop_kernel bit for bit against numpy.
3. ``model.render_rays_occluded`` bit for bit the chain of op-level entries (composite_scene -> scene_occluder on the chain's own
   buffers): plain, only_coarse, with a sample-culling grid, with termination, with a background cache; no occluder = no new
   launch and no changed bit.
4. The occluder stop: the occluded outputs keep their bits, fewer rows are listed, rays without an opaque row keep their outputs.
5. The oracle case through the model against the fp32 and fp64 oracle statements, under
   ``scene_edits_common.assert_matches_oracle`` as it is.
Needs an MI355X: `pytest -m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import occluder_common as OCL
import occupancy_common as OCC
import scene_edits_common as S
import test_gpu_bkgd_cache as BC
import test_gpu_scene_edits_oracle as SE
from pipeline_chain import assert_pairs_equal, bits, chain_render, cu, detach_models, np_bits, same_bits, with_chain
from stnerf_amd import hip, ops, parallel, synthetic as syn
from test_gpu_occupancy import attach

pytestmark = pytest.mark.gpu

POISON = 0x7FC0BEEF      # a NaN pattern no kernel writes
PAD = 64
F = np.float32
U = 2.0 ** -24


@pytest.fixture(autouse=True)
def detach():
    yield
    detach_models()


def np_same(a, b):
    """The same bits, a NaN matching any NaN (the payload of a NaN an operation produces is the hardware's own)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(((np_bits(a) == np_bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------------------------------- 1. the kernel
A_VALUES = (0.0, -1.0, float("nan"), 0.5, 1.0, 2.0)
Z_KINDS = ("nan", "+inf", "-inf", "exact", "below", "above", "middle")


def kernel_inputs(n, l, S_, seed):
    """Hand-made inputs: per layer ascending random depths, layer 1 tied to layer 0 on the even rays, one NaN depth; merged weights
    random positive of the order of 1 / S; random raw; masks with cleared bits; evaluated 2, 1, 0, 1; occluder rows over every
    combination of a in A_VALUES and z in Z_KINDS (all 42 with n = 70)."""
    g = np.random.default_rng(seed)
    t = (1.0 + np.cumsum(g.random((n, l, S_)) * 0.1 + 0.01, -1)).astype(F)
    if l > 1:
        t[0::2, 1] = t[0::2, 0]
    clean = t.copy()
    if n > 3:
        t[3, l - 1, S_ // 2] = np.nan
    wm = ((0.25 + g.random((n, l, S_))) / S_).astype(F)
    raw = (g.standard_normal((n, l, S_, 4)) * 2).astype(F)
    mask = (g.random((n, l)) < 0.7).astype(np.uint8)
    mask[0] = 1
    evaluated = [2, 1, 0, 1][:l]
    combos = [(a, z) for z in Z_KINDS for a in A_VALUES]
    order = g.permutation(len(combos))
    occ = np.zeros((n, 5), F)
    occ[:, 0:3] = g.random((n, 3))
    for r in range(n):
        a, kind = combos[order[r % len(combos)]]
        if n == 1:
            a, kind = 0.5, "exact"
        lo, hi = np.nanmin(t[r]), np.nanmax(t[r])
        exact = t[r, min(1, l - 1), min(S_ - 1, 1 + r % S_)]          # (on an even ray layer 0 has a sample at the same depth)
        z = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "exact": t[r, 0, 0] if np.isnan(exact) else exact,
             "below": lo - 0.5, "above": hi + 0.5, "middle": 0.5 * (lo + hi)}[kind]
        occ[r, 3], occ[r, 4] = a, z
    have = np.stack([np.ones(n, bool) if e == 2 else (mask[:, i] & 1).astype(bool) if e == 1 else np.zeros(n, bool)
                     for i, e in enumerate(evaluated)], 1)
    return dict(t=t, clean=clean, wm=wm, raw=raw, mask=mask, evaluated=evaluated, occ=occ, have=have)


def padded(shape):
    """A poisoned buffer with PAD floats of canary on either side -> (whole buffer, the view the kernel writes)."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * PAD,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    return buf, buf[PAD:PAD + numel].view(*shape)


def run_kernel(d, scene_in, mixed_in, occ, rgb_activated, t=None, wm=None, optional=True):
    """stnerf_scene_occluder through the library on canaried outputs -> dict of CPU numpy outputs (None for a NULL one)."""
    t_, raw, mask, wm_ = cu(d["t"] if t is None else t), cu(d["raw"]), cu(d["mask"], torch.uint8), cu(d["wm"] if wm is None else wm)
    n, l, S_ = t_.shape
    p = ops.composite_params(evaluated=d["evaluated"], rgb_activated=rgb_activated)
    shapes = dict(mixed=(n, 5), scene=(n, l, 5), share=(n, 5), front=(n, l, 5), behind=(n, l, 5))
    bufs = {k: padded(s) for k, s in shapes.items() if optional or k == "mixed"}
    ptr = lambda k: hip.dptr(bufs[k][1]) if k in bufs else C.c_void_p(0)
    scene_d, mixed_d, occ_d = cu(scene_in), cu(mixed_in), cu(occ)      # (held: a temporary's memory is handed to the next allocation)
    hip.check(hip.lib().stnerf_scene_occluder(hip.dptr(t_), hip.dptr(raw), hip.dptr(mask, torch.uint8), hip.dptr(wm_), n, l, S_, C.byref(p),
                                              hip.dptr(scene_d), hip.dptr(mixed_d), hip.dptr(occ_d), ptr("mixed"), ptr("scene"),
                                              ptr("share"), ptr("front"), ptr("behind"), hip.stream_ptr()), "stnerf_scene_occluder")
    torch.cuda.synchronize()
    out = {}
    for k, (whole, view) in bufs.items():
        w = whole.view(torch.int32)
        assert bool((w[:PAD] == POISON).all()) and bool((w[-PAD:] == POISON).all()), f"{k}: a canary was overwritten"
        assert not bool((view.contiguous().view(torch.int32) == POISON).any()), f"{k}: an element was not written"
        out[k] = view.cpu().numpy()
    return out


def colours(raw, rgb_activated):
    """The colours the compositor uses, as the GPU computes them (the sigmoid through torch on the device is NOT the kernel's
    hardware one: only for the fp64 bound, with rgb_activated = 1, are they used)."""
    assert rgb_activated
    return raw[..., 0:3]


@pytest.mark.parametrize("S_", [3, 64, 65, 192])
@pytest.mark.parametrize("l", [1, 3, 4])
@pytest.mark.parametrize("n", [1, 5, 70])
def test_scene_occluder_kernel(n, l, S_):
    d = kernel_inputs(n, l, S_, seed=1000 * n + 10 * l + S_)
    g = np.random.default_rng(5)
    for rgb_activated in (False, True):
        # ---- (a) a real composite: z beyond every depth reproduces scene_out in front, z below every depth behind, bit for bit
        _, mixed, _, merged, scene = ops.composite_scene(cu(d["clean"]), cu(d["raw"]), cu(d["mask"], torch.uint8), fine=True,
                                                         evaluated=d["evaluated"], rgb_activated=rgb_activated)
        merged_h, scene_h, mixed_h = merged.cpu().numpy(), scene.cpu().numpy(), mixed.cpu().numpy()
        occ = np.zeros((n, 5), F)
        occ[:, 0:3], occ[:, 3] = g.random((n, 3)), np.where(np.arange(n) % 3 == 0, 1.0, 0.5)
        above = np.arange(n) % 2 == 0
        occ[:, 4] = np.where(above, d["clean"].max((1, 2)) + 0.25, d["clean"].min((1, 2)) - 0.25)
        out = run_kernel(d, scene_h, mixed_h, occ, rgb_activated, t=d["clean"], wm=merged_h)
        side, other = np.where(above[:, None, None], out["front"], out["behind"]), np.where(above[:, None, None], out["behind"], out["front"])
        assert np.array_equal(np_bits(side), np_bits(scene_h)), "the side that holds every sample is not the scene pass, bit for bit"
        assert not np_bits(other).any(), "the empty side is not +0"
        want = OCL.np_mix(out["front"], out["behind"], occ, scene_h, mixed_h)
        for k, w in zip(("mixed", "scene", "share"), want):
            assert np.array_equal(np_bits(out[k]), np_bits(w)), f"{k} (real composite, rgb_activated={rgb_activated})"
        hidden = ~d["have"]
        assert not np_bits(out["front"][hidden]).any() and not np_bits(out["behind"][hidden]).any() and not np_bits(out["scene"][hidden]).any()
        # ---- (b) hand-made weights, every kind of row, a NaN depth, ties
        scene_in, mixed_in = g.standard_normal((n, l, 5)).astype(F), g.standard_normal((n, 5)).astype(F)
        out = run_kernel(d, scene_in, mixed_in, d["occ"], rgb_activated)
        _, present = OCL.np_present(d["occ"])
        f_abs, b_abs = OCL.np_front_behind(d["occ"], scene_in)
        assert np.array_equal(np_bits(out["front"][~present]), np_bits(f_abs[~present])) and not np_bits(out["behind"][~present]).any()
        want = OCL.np_mix(out["front"], out["behind"], d["occ"], scene_in, mixed_in)
        for k, w in zip(("mixed", "scene", "share"), want):
            assert np_same(out[k], w), f"{k} (hand-made, rgb_activated={rgb_activated})"
        assert np.array_equal(np_bits(out["mixed"][~present]), np_bits(mixed_in[~present]))
        assert np.array_equal(np_bits(out["scene"][~present]), np_bits(scene_in[~present])) and not np_bits(out["share"][~present]).any()
        hidden = ~d["have"] & present[:, None]
        assert not np_bits(out["front"][hidden]).any() and not np_bits(out["behind"][hidden]).any()
        alone = run_kernel(d, scene_in, mixed_in, d["occ"], rgb_activated, optional=False)
        assert sorted(alone) == ["mixed"] and np_same(alone["mixed"], out["mixed"])
        if not rgb_activated:
            continue
        # ---- (c) a general z: the sums in fp64, |got - exact| <= gamma sum |wM x| with gamma = (S + 1) u / (1 - (S + 1) u), the bound
        # of an fp32 sum of S rounded products in ANY order (derived, not measured); a sample AT z is behind
        exact_f, exact_b, scale = OCL.exact_front_behind(d["t"], d["wm"], colours(d["raw"], True), d["occ"], d["have"])
        gamma = (S_ + 1) * U / (1 - (S_ + 1) * U)
        for name, got, exact in (("front", out["front"], exact_f), ("behind", out["behind"], exact_b)):
            got, exact, bound = got[present].astype(np.float64), exact[present], gamma * scale[present]
            nan = np.isnan(exact)
            assert np.array_equal(np.isnan(got), nan), name
            worst = np.max(np.where(nan, -np.inf, np.abs(got - exact) - bound), initial=-np.inf)
            print(f"n={n} l={l} S={S_} {name}: largest |got - exact| - bound = {worst:.3e}")
            assert worst <= 0.0, (name, worst)
        if n == 70:        # a misplaced sample would show: the exact-z rows move a whole weight to the other side under `>`
            assert (np.abs(exact_b[present]).max(-1) > 0).any() and (np.abs(exact_f[present]).max(-1) > 0).any()


def test_scene_occluder_argument_errors():
    n, l, S_ = 4, 3, 8
    z = lambda *s: torch.zeros(*s, device="cuda")
    t, raw, wm, scene, mixed, occ = z(n, l, S_), z(n, l, S_, 4), z(n, l, S_), z(n, l, 5), z(n, 5), z(n, 5)
    ops.scene_occluder(t, raw, None, wm, scene, mixed, occ)
    off = torch.zeros(n * l * S_ * 4 + 1, device="cuda")[1:].view(n, l, S_, 4)        # 4 bytes off a 16-byte boundary
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.scene_occluder(t, off, None, wm, scene, mixed, occ)
    with pytest.raises(ValueError, match="bad shape"):
        ops.scene_occluder(z(n, 17, S_), z(n, 17, S_, 4), None, z(n, 17, S_), z(n, 17, 5), mixed, occ)
    with pytest.raises(ValueError, match="65535"):
        ops.scene_occluder(z(1, 16, 4096), z(1, 16, 4096, 4), None, z(1, 16, 4096), z(1, 16, 5), z(1, 5), z(1, 5))
    p = ops.composite_params()
    null = C.c_void_p(0)
    args = [hip.dptr(t), hip.dptr(raw), null, hip.dptr(wm), n, l, S_, C.byref(p), hip.dptr(scene), hip.dptr(mixed), hip.dptr(occ),
            hip.dptr(z(n, 5)), null, null, null, null, hip.stream_ptr()]
    for i in (0, 1, 3, 8, 9, 10, 11):
        bad = list(args)
        bad[i] = null
        assert hip.lib().stnerf_scene_occluder(*bad) == hip.EINVAL, i
    assert hip.lib().stnerf_scene_occluder(*args) == hip.OK
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------- 2. the stop kernel
@pytest.mark.parametrize("n", [1, 257, 1000])
def test_occluder_stop_kernel_equals_numpy(n):
    g = np.random.default_rng(n)
    occ = np.zeros((n, 5), F)
    occ[:, 3] = g.choice([0.0, -1.0, np.nan, 0.5, np.nextafter(F(1), F(0)), 1.0, 2.0], n)
    occ[:, 4] = g.choice([np.nan, np.inf, -np.inf, 1.0, 2.0, 3.0, -4.0], n)
    stop = g.choice([np.inf, 2.0, 2.5, 0.5], n).astype(F)                      # (z equal to t_stop; t_stop = +inf)
    if n > 8:
        occ[:8, 3:5] = [[1, 2], [1, 2], [np.nextafter(F(1), F(0)), 1], [1, 1], [2, 1], [1, np.nan], [0, 1], [1, -np.inf]]
        stop[:8] = [2.0, np.inf, 2.0, np.inf, 2.0, 2.0, 2.0, 2.0]
    buf, view = padded((n,))
    view.copy_(torch.from_numpy(stop))
    got = ops.occluder_stop(torch.from_numpy(occ).cuda(), view)
    torch.cuda.synchronize()
    assert got is view and bool((buf.view(torch.int32)[:PAD] == POISON).all()) and bool((buf.view(torch.int32)[-PAD:] == POISON).all())
    want = OCL.np_stop(occ, stop)
    assert np.array_equal(np_bits(view.cpu().numpy()), np_bits(want))
    if n > 8:
        assert want[:8].tolist() == [2.0, 2.0, 2.0, 1.0, 1.0, 2.0, 2.0, 2.0] and (want != stop).sum() >= 3


# ---------------------------------------------------------------------------------------- 3. the pipeline is the chain
def occluder_after(model, flags, tau):
    """What follows the chain (tests/pipeline_chain.py) in an occluded launch: ``ops.scene_occluder`` on the buffers the chain's final
    composite_scene took and returned, kept as ``chain.occluded``; with the occluder stop the chain runs again on
    ``ops.occluder_stop`` of its own stop depths first."""
    def after(chain, launch):
        occluder = launch["occluder"]
        assert launch.get("background_id") is None
        if launch.get("occluder_stops") and any(flags) and not launch["only_coarse"]:
            chain = chain_render(model, launch, flags, tau, t_stop=ops.occluder_stop(occluder, chain.stop.clone()))
        chain.occluded = ops.scene_occluder(chain.t, chain.raw, chain.mask, chain.merged, chain.scene, chain.mixed, occluder, rgb_activated=True,
                                            evaluated=chain.evaluated)[:3]
        return chain
    return after


def assert_pairs(pairs, what, pieces):
    assert_pairs_equal(pairs, what, pieces)
    for piece, (got, chain) in enumerate(pairs):
        assert len(got) == 9
        for name, g, w in zip(("occluded_mixed", "occluded_scene", "occluder_share"), got[6:], chain.occluded):
            assert same_bits(g, w), f"{what}: piece {piece}: {name} differs from ops.scene_occluder on the chain's buffers"


def occluded_render(model, case, rays, occ, **kw):
    with torch.no_grad():
        out = model.render_rays_occluded(rays, occ, case["only_coarse"], case["thr"], case["bthr"], ref_chunk=case["chunk"], **kw)
    torch.cuda.synchronize()
    return out


def flat_all(out):
    """(5-tuple, scene, occluded) -> one flat dict of CPU tensors (masks as bool)."""
    d = S.flat((out[0], out[1]))
    d.update(OCL.flat_occluded(out[2]))
    return d


PIECES = (S.N + S.CAP - 1) // S.CAP
TAU = 1e-3


@pytest.mark.parametrize("variant", ["plain", "only_coarse", "grid", "terminated", "terminated+stops"])
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_pipeline_is_the_chain_of_op_level_entries(monkeypatch, precision, variant):
    case = OCC.plain_case(only_coarse=variant == "only_coarse")
    rays = S.case_rays(case).cuda()
    occ = torch.from_numpy(OCL.case_occluder()).cuda()
    model = SE.make_model(case, precision)
    l = model.total_layers
    flags, tau = [False] * l, 0.0
    if variant == "grid":
        attach(model, OCC.manual_grids(case, "half_x", 0, layers=(1,)), samples=True)
    if variant.startswith("terminated"):
        model.set_termination(TAU, layers=[1, 2], background=True)
        flags, tau = [True, True, True, False], TAU
    pairs = []
    with_chain(model, monkeypatch, pairs, flags, tau, after=occluder_after(model, flags, tau))
    stops = variant.endswith("stops")
    first = flat_all(occluded_render(model, case, rays, occ, stops=stops))
    assert_pairs(pairs, f"{precision} {variant}", PIECES)
    # twice: the same bits
    pairs.clear()
    again = flat_all(occluded_render(model, case, rays, occ, stops=stops))
    assert set(first) == set(again)
    for k in first:
        assert torch.equal(first[k], again[k]) if first[k].dtype == torch.bool else same_bits(first[k], again[k]), k
    # the occluder shows on the present rays and nowhere else
    present = torch.from_numpy(OCL.np_present(OCL.case_occluder())[1])
    diff = (first["fine_occluded_mixed"] - first["fine_mixed"]).abs().amax(1)
    assert same_bits(first["fine_occluded_mixed"][~present], first["fine_mixed"][~present])
    if variant != "only_coarse":      # (the coarse stage's uncut background hides the occluder: DESIGN.md section 7, "only_coarse")
        assert int((diff[present] > 1e-2).sum()) >= 100
    assert not bits(first["fine_occluder_share"][~present]).any()
    for i in range(l):
        assert same_bits(first[f"fine_occluded_scene{i}"][~present], first[f"scene{i}"][~present])


def test_pipeline_is_the_chain_with_a_background_cache(monkeypatch):
    """CAPTURE then REUSE through ``parallel.render_view(occluder=)``, which sets the view key the cache needs."""
    import stnerf_amd
    model = BC.make_model(2)
    assert model._bkgd_cache is not None
    K, T = syn.camera(BC.H, BC.W, 15.0)
    n = BC.H * BC.W
    occ = torch.from_numpy(OCL.case_occluder(n)).cuda()
    pairs = []
    with_chain(model, monkeypatch, pairs, after=occluder_after(model, [False] * 3, 0.0))
    outs = []
    for fids in (BC.fids(True, 2, (1.0, 1.0)), BC.fids(True, 2, (2.5, 3.0))):
        outs.append(flat_all(parallel.render_view(model, K, T, BC.H, BC.W, fids, chuncks=BC.CHUNK, occluder=occ)))
        torch.cuda.synchronize()
    assert BC.stats(model)[0] == BC.PIECES and BC.stats(model)[2] == BC.PIECES
    assert_pairs(pairs, "background cache: capture + reuse frames", 2 * BC.PIECES)
    assert not same_bits(outs[0]["fine_occluded_mixed"], outs[1]["fine_occluded_mixed"])


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_no_occluder_changes_no_bit_and_no_launch(precision):
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
    new = lambda recs: [r for r in recs if r["kernel"] in ("scene_occluder", "occluder_stop")]
    def scene_render():
        with torch.no_grad():
            return S.flat(model.render_rays_scene(rays, False, case["thr"], case["bthr"], ref_chunk=case["chunk"]))
    plain, recs = records(scene_render)
    bytes_plain = model._workspace.numel()
    assert recs and not new(recs)
    occ = torch.from_numpy(OCL.case_occluder()).cuda()
    out, recs1 = records(lambda: occluded_render(model, case, rays, occ))
    assert model._workspace.numel() == bytes_plain == hip.lib().stnerf_render_workspace_bytes(S.CAP, l, case["n1"], case["n2"], 0)
    got = S.flat((out[0], out[1]))
    for k in got:                                                  # the 5-tuple and the scene passes: the bits of render_rays_scene
        assert torch.equal(got[k], plain[k]) if got[k].dtype == torch.bool else same_bits(got[k], plain[k]), k
    added = new(recs1)
    assert [r["kernel"] for r in added] == ["scene_occluder"] * PIECES and {r["ns"] for r in added} == {case["n1"] + case["n2"]}
    assert [r["kernel"] for r in recs1 if r not in added] == [r["kernel"] for r in recs]
    # the newest entry with a NULL occluder is stnerf_render_rays_layers: ops.render_rays never takes it without an occluder
    assert "stnerf_render_rays_occluded" in hip.exported_symbols()


# ---------------------------------------------------------------------------------------- 4. the occluder stop
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_occluder_stop_keeps_the_occluded_bits_and_lists_fewer_rows(precision):
    """The oracle case's occluder, termination at tau = 0 on every layer (nothing but an exactly opaque coarse ray stops by itself:
    what the row lists lose is the occluder's doing)."""
    case = OCC.plain_case()
    rays = S.case_rays(case).cuda()
    occ_h = OCL.case_occluder()
    occ = torch.from_numpy(occ_h).cuda()
    model = SE.make_model(case, precision)
    model.set_termination(0.0)
    l, ns = model.total_layers, case["n1"] + case["n2"]
    assert model.termination.flags(model) == [True] * l
    model.termination.reset_stats()
    off = flat_all(occluded_render(model, case, rays, occ, stops=False))
    rows_off = model.termination.stats()["rows"]
    model.termination.reset_stats()
    on = flat_all(occluded_render(model, case, rays, occ, stops=True))
    rows_on = model.termination.stats()["rows"]
    for k in on:
        if "occlude" in k:
            assert same_bits(on[k], off[k]), f"{k} changes with the occluder stop"
    assert sorted(rows_on) == sorted(rows_off) == list(range(l))
    listed = lambda rows: {i: t - s for i, (t, s) in rows.items()}
    print("rows listed, stop off / on:", listed(rows_off), listed(rows_on))
    for i in range(l):
        assert rows_on[i][0] == rows_off[i][0] and listed(rows_on)[i] < listed(rows_off)[i], (i, rows_off, rows_on)
    assert rows_on[0][0] == S.N * ns
    # rays without an opaque row keep every output; some ray with one loses part of its plain image
    ap, present = OCL.np_present(occ_h)
    opaque = torch.from_numpy(present & (ap >= 1))
    for k in on:
        assert torch.equal(on[k][~opaque], off[k][~opaque]) if on[k].dtype == torch.bool else same_bits(on[k][~opaque], off[k][~opaque]), k
    assert int(((on["fine_mixed"] - off["fine_mixed"]).abs().amax(1)[opaque] > 1e-3).sum()) >= 20
    # stops without a terminated layer is refused by the library as well
    model.set_termination(None)
    with pytest.raises(ValueError, match="without early ray termination"):
        occluded_render(model, case, rays, occ, stops=True)


# ---------------------------------------------------------------------------------------- 5. the oracle
@functools.lru_cache(maxsize=None)
def oracle_refs():
    """The oracle case, its occluder and rays, the fp32 and fp64 statements of the occluded and of the plain outputs: made once."""
    case, occ = OCL.oracle_case(), OCL.case_occluder()
    rays = S.case_rays(case)
    return (case, occ, rays, OCL.oracle_occluded(case, occ, torch.float32, rays), OCL.oracle_occluded(case, occ, torch.float64, rays),
            S.oracle_render(case, rays), S.oracle_render(case, rays, torch.float64))


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_oracle(precision):
    case, occ, rays, (ref32, info32), (ref64, info64), r32, r64 = oracle_refs()
    keep, figures = OCL.oracle_conditions(info32, info64, occ)
    model = SE.make_model(case, precision)
    out = occluded_render(model, case, rays.cuda(), torch.from_numpy(occ).cuda())
    got = OCL.flat_occluded(out[2])
    fig = OCL.assert_occluded_matches_oracle(got, ref32, ref64, keep, f"occluded {precision}")
    print(figures, {k: tuple(f"{x:.2e}" if isinstance(x, float) else x for x in v) for k, v in fig.items()})
    # the plain outputs of the same call against the plain oracle, as tests/test_gpu_scene_edits_oracle.py holds them
    plain = S.flat((out[0], out[1]))
    drop = lambda d: {k: v for k, v in d.items() if k != "t_coarse"}
    S.assert_matches_oracle(plain, drop(r32), drop(r64), False, f"plain {precision}")


def test_render_pose_with_an_occluder():
    """Through ``render_pose(occluder=(rgba, depth))``: the images are the model's occluded outputs, the depths divided by far."""
    from stnerf_amd.render.render_pose import render_pose
    case = OCC.plain_case(chunk=S.N, thr=1e-4, bthr=0.0)
    ids, far = case["groups"][0][1], 20.0
    K, T = syn.camera(S.H, S.W, case["orbit"])
    model = SE.make_model(case)
    l = model.total_layers
    occ = torch.from_numpy(OCL.case_occluder()).cuda()
    rgba, depth = occ[:, 0:4].reshape(S.H, S.W, 4), occ[:, 4].reshape(S.H, S.W)
    color, dimg, color_layer, depth_layer, passes = render_pose(model, T, K, S.H, S.W, list(enumerate(ids)), far, 0.05, 0.02,
                                                                occluder=(rgba, depth))
    rays = ops.generate_rays(K, T, S.H, S.W, frame_ids=ids)
    with torch.no_grad():
        _, scene, occluded = model.render_rays_occluded(rays, occ)
    torch.cuda.synchronize()
    assert sorted(passes) == sorted(["color_scene", "alpha_scene", "depth_scene", "color_occluded", "alpha_occluded", "depth_occluded",
                                     "color_scene_occluded", "alpha_scene_occluded", "depth_scene_occluded", "occluder_share"])
    img = lambda t, c: t.reshape(S.H, S.W, c)
    assert same_bits(passes["color_occluded"], img(occluded["mixed"][0], 3)) and same_bits(passes["alpha_occluded"], img(occluded["mixed"][2], 1))
    assert same_bits(passes["depth_occluded"], img(occluded["mixed"][1], 1) / far)
    for i in range(l):
        assert same_bits(passes["color_scene_occluded"][i], img(occluded["scene"][i][0], 3))
        assert same_bits(passes["depth_scene_occluded"][i], img(occluded["scene"][i][1], 1) / far)
        assert same_bits(passes["color_scene"][i], img(scene[i][0], 3))
    assert same_bits(passes["occluder_share"][1], img(occluded["share"][2], 1)) and passes["color_occluded"].shape == (S.H, S.W, 3)
    # z from a camera-space z-buffer: ops.ray_parameter puts the point at that depth
    t = ops.ray_parameter(rays, T, 4.0)
    point = rays[:, 0:3] + t[:, None] * rays[:, 3:6]
    cam = (point - torch.as_tensor(T, dtype=torch.float32)[:3, 3].cuda()) @ torch.as_tensor(T, dtype=torch.float32)[:3, :3].cuda()
    assert float((cam[:, 2] - 4.0).abs().max()) <= 1e-4
