"""Progressive multi-sample frames, the host side (no GPU): the pass schedule, ``AccumulateSpec``'s validation, the driver's
refusals, the library's argument checks, and the numpy oracle (tests/accumulate_common.py) against fp64 numpy."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import accumulate_common as A
from stnerf_amd import accumulate as acc
from stnerf_amd import hip, parallel

F = np.float32


# ---------------------------------------------------------------------------------------- schedule
def test_pass_zero_is_the_plain_render_and_every_pass_is_inside_the_pixel():
    assert acc.pass_schedule(0) == (0.0, 0.0, 0.0)
    for p in range(512):
        got = acc.pass_schedule(p)
        assert all(isinstance(x, float) and -0.5 <= x < 0.5 and float(F(x)) == x for x in got), (p, got)
        assert got == tuple(float(x) for x in A.pass_schedule(p)), p
    # the first passes by hand: phi_2 = 0, 1/2, 1/4, 3/4; phi_3 = 0, 1/3, 2/3, 1/9; phi_5 = 0, 1/5, 2/5, 3/5; a phi >= 1/2 wraps to phi - 1
    assert [acc.pass_schedule(p)[0] for p in range(4)] == [0.0, -0.5, 0.25, -0.25]
    assert [acc.pass_schedule(p)[1] for p in range(4)] == [float(F(x)) for x in (0.0, 1 / 3, -1 / 3, 1 / 9)]
    assert [acc.pass_schedule(p)[2] for p in range(4)] == [float(F(x)) for x in (0.0, 0.2, 0.4, -0.4)]


def _cells(n_passes, g):
    counts = np.zeros((g, g), int)
    for p in range(n_passes):
        du, dv, _ = acc.pass_schedule(p)
        counts[int((dv + 0.5) * g), int((du + 0.5) * g)] += 1
    return counts


def test_every_prefix_is_spread_over_the_pixel():
    """"About equally": no cell of the grid is empty and none holds more than half again its share (n / g^2) -- a prefix of
    independent uniform draws misses a cell of the 4x4 grid with probability 1 - (1 - (15/16)^64)^16 = 23 % at 64 draws; a
    low-discrepancy prefix does not."""
    for n, g in ((8, 2), (64, 2), (64, 4)):
        counts = _cells(n, g)
        share = n / (g * g)
        print(n, g, counts.tolist())
        assert counts.min() >= 0.5 * share and counts.max() <= 1.5 * share, (n, g, counts)
    dts = sorted(acc.pass_schedule(p)[2] for p in range(25))            # base 5: 25 passes = one per 1/25 of the shutter
    assert np.allclose(np.diff(dts), 1 / 25, atol=1e-6)


def test_layer_frame_ids_follow_the_shutter_and_the_clamp():
    spec = acc.AccumulateSpec(8, shutter=[0.0, 2.0, -1.0])
    ids = [1.0, 3.0, 5.5]
    for p in range(8):
        dt = acc.pass_schedule(p)[2]
        assert spec.frame_ids(p, ids) == [1.0, float(F(3.0 + 2.0 * dt)), float(F(5.5 - dt))]
        assert spec.frame_ids(p, ids) == [float(x) for x in A.layer_frame_ids(p, ids, [0.0, 2.0, -1.0])]
    assert spec.frame_ids(0, ids) == ids                                # pass 0: the frame itself
    # a scalar reaches the performers only
    assert acc.AccumulateSpec(4, shutter=2.0).shutters(3) == [0.0, 2.0, 2.0]
    assert acc.AccumulateSpec(4).shutters(3) == [0.0, 0.0, 0.0] and not acc.AccumulateSpec(4).has_shutter(3)
    assert acc.AccumulateSpec(4, shutter=2.0).frame_ids(1, ids)[0] == 1.0
    # the clamp: pass 3 has dt = -0.4, pass 2 dt = 0.4; every layer's id is clamped, the still background's too
    clamped = acc.AccumulateSpec(8, shutter=4.0, frame_range=(2.5, 6.0))
    assert clamped.frame_ids(3, ids) == [2.5, 2.5, float(F(5.5 + 4.0 * acc.pass_schedule(3)[2]))]
    assert clamped.frame_ids(2, ids) == [2.5, float(F(3.0 + 4.0 * acc.pass_schedule(2)[2])), 6.0]
    assert 3.89 < clamped.frame_ids(3, ids)[2] < 3.91 and 4.59 < clamped.frame_ids(2, ids)[1] < 4.61
    with pytest.raises(ValueError, match="one entry per layer"):
        acc.AccumulateSpec(4, shutter=[1.0, 2.0]).shutters(3)
    # the offsets are the schedule's, scaled by the filter width
    assert acc.AccumulateSpec(4).offset(3) == acc.pass_schedule(3)[:2]
    assert acc.AccumulateSpec(4, pixel_filter=0.0).offset(3) == (0.0, 0.0)
    wide = acc.AccumulateSpec(4, pixel_filter=1.5).offset(3)
    assert wide == tuple(float(x) for x in A.offset(3, 1.5)) == tuple(float(F(1.5 * x)) for x in acc.pass_schedule(3)[:2])


# ---------------------------------------------------------------------------------------- the spec
def test_spec_defaults_and_validation():
    s = acc.AccumulateSpec(8)
    assert (s.max_spp, s.min_spp, s.tol, s.pixel_filter, s.shutter, s.frame_range, s.adaptive) == (8, 8, 0.0, 1.0, None, None, False)
    s = acc.AccumulateSpec(8, 2, 0.01)
    assert (s.min_spp, s.tol, s.adaptive) == (2, 0.01, True)
    assert acc.as_spec(dict(max_spp=4, min_spp=2, tol=0.5)).min_spp == 2 and acc.as_spec(s) is s
    import stnerf_amd
    assert stnerf_amd.AccumulateSpec is acc.AccumulateSpec
    for bad in (dict(max_spp=0), dict(max_spp=4, min_spp=0), dict(max_spp=4, min_spp=5), dict(max_spp=2.5), dict(max_spp=40000),
                dict(max_spp=4, tol=-1e-3), dict(max_spp=4, tol=float("nan")), dict(max_spp=4, tol=1e30),
                dict(max_spp=4, pixel_filter=-0.5), dict(max_spp=4, pixel_filter=float("inf")),
                dict(max_spp=4, shutter=float("nan")), dict(max_spp=4, shutter=[0.0, float("inf")]),
                dict(max_spp=4, frame_range=(3.0, 1.0)), dict(max_spp=4, frame_range=(1.0,))):
        with pytest.raises(ValueError):
            acc.AccumulateSpec(**bad)
    with pytest.raises(TypeError):
        acc.as_spec(8)


# ---------------------------------------------------------------------------------------- the driver's refusals
def _fake_model(**over):
    m = types.SimpleNamespace(total_layers=3, layer_num=2, seed=5, fresh_draws_per_call=True, replay=None, ray_window=(0, 0, 0),
                              _bkgd_cache=None, _layer_cache=None, _occupancy=None, shard_views=False)
    for k, v in over.items():
        setattr(m, k, v)
    return m


K, T = torch.eye(3), torch.eye(4)
IDS = [1.0, 2.0, 3.0]


def test_the_driver_names_what_it_refuses(monkeypatch):
    """Every refusal is raised before anything touches the device (there is none here) and leaves the seed alone."""
    spec = acc.AccumulateSpec(4, 2, 0.01)
    call = lambda model, spec=spec, **kw: parallel.render_view_accumulated(model, K, T, 4, 4, IDS, spec, 0.0, 0.0, device="cpu", **kw)
    for over, exc, what in ((dict(_bkgd_cache=object()), ValueError, "one jitter pattern"),
                            (dict(_layer_cache=object()), ValueError, "one jitter pattern"),
                            (dict(replay={"jitter": None}), ValueError, "replay")):
        m = _fake_model(**over)
        with pytest.raises(exc, match=what):
            call(m)
        assert m.seed == 5
    with pytest.raises(ValueError, match="out of scope"):
        call(_fake_model(), scene=True)
    with pytest.raises(ValueError, match="out of scope"):
        call(_fake_model(), occluder=torch.zeros(16, 5))
    # shutter with grids: refused; the same grids with shutter 0 get past this check (and then need the device)
    grids = _fake_model(_occupancy=object())
    with pytest.raises(ValueError, match="keyed by frame"):
        call(grids, acc.AccumulateSpec(4, shutter=1.0))
    with pytest.raises(ValueError, match="keyed by frame"):
        call(grids, dict(max_spp=4, shutter=[0.0, 0.0, 0.5]))
    with pytest.raises(ValueError, match="one entry per layer"):
        call(_fake_model(), acc.AccumulateSpec(4, shutter=[0.0, 1.0]))
    # an active process group with shard_views
    monkeypatch.setattr(parallel, "active_group", lambda model=None: (0, 2, None))
    with pytest.raises(RuntimeError, match="one rank"):
        call(_fake_model(shard_views=True))


def test_render_pose_refuses_scene_passes_and_an_occluder_with_accumulate():
    from stnerf_amd.render.render_pose import render_pose
    m = _fake_model()
    with pytest.raises(ValueError, match="out of scope"):
        render_pose(m, T, K, 4, 4, list(enumerate(IDS)), 20.0, accumulate=acc.AccumulateSpec(2), scene_passes=True, device="cpu")
    with pytest.raises(ValueError, match="out of scope"):
        render_pose(m, T, K, 4, 4, list(enumerate(IDS)), 20.0, accumulate=dict(max_spp=2), device="cpu",
                    occluder=(torch.zeros(4, 4, 4), torch.zeros(4, 4)))


# ---------------------------------------------------------------------------------------- the library's host checks
def test_entries_check_their_arguments_before_any_launch():
    lib = hip.lib()
    fake, null = C.c_void_p(1 << 20), C.c_void_p(0)           # (never dereferenced)
    kin, tin, fin = (C.c_float * 9)(), (C.c_float * 16)(), (C.c_float * 3)()
    gen = lambda h, w, n, du=0.0, dv=0.0, cols=3, stride=9, rays=fake, k=kin: lib.stnerf_generate_rays_list(
        k, tin, h, w, null, n, du, dv, fin, cols, rays, stride, None)
    assert gen(4, 4, 0) == hip.OK                                                   # nothing to do: no launch
    for bad in (gen(4, 4, 17), gen(4, 4, -1), gen(0, 4, 1), gen(4, 0, 1), gen(1 << 16, 1 << 16, 1), gen(4, 4, 4, du=float("nan")),
                gen(4, 4, 4, cols=18), gen(4, 4, 4, stride=8), gen(4, 4, 4, rays=null), gen(4, 4, 4, k=None)):
        assert bad == hip.EINVAL
    assert gen(4, 4, 17) == hip.EINVAL and "at most once" in hip.last_error()
    accu = lambda n, Cw=15, stride=15, P=100, V=3, values=fake, count=fake: lib.stnerf_accumulate(
        values, n, Cw, stride, null, P, V, fake, fake, count, None)
    assert accu(0) == hip.OK
    for bad in (accu(101), accu(-1), accu(10, stride=14), accu(10, V=0), accu(10, V=16), accu(10, Cw=0), accu(10, P=0), accu(10, P=1 << 31),
                accu(10, values=null), accu(10, count=null)):
        assert bad == hip.EINVAL
    assert accu(10, stride=14) == hip.EINVAL and "stride" in hip.last_error()
    # the workspace: one int32 per 256 pixels, rounded up to 256 B
    ws = lib.stnerf_accumulate_select_workspace_bytes
    assert [ws(P) for P in (1, 256, 257, 64 * 256, 64 * 256 + 1, 1920 * 1080)] == [256, 256, 256, 256, 512, 32512]
    assert ws(0) == hip.EINVAL and ws(1 << 31) == hip.EINVAL
    sel = lambda P=1000, V=3, lo=2, hi=8, tol2=0.0, nbytes=256, out=fake, work=fake: lib.stnerf_accumulate_select(
        fake, fake, P, V, lo, hi, tol2, out, fake, work, nbytes, None)
    for bad in (sel(P=0), sel(V=0), sel(lo=0), sel(lo=9), sel(hi=32769), sel(tol2=-1.0), sel(tol2=float("nan")), sel(out=null), sel(work=null),
                sel(P=70001, nbytes=1024)):
        assert bad == hip.EINVAL
    assert sel(P=70001, nbytes=1024) == hip.EINVAL and "workspace too small" in hip.last_error()


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from stnerf_amd import ops
    with pytest.raises(ValueError, match="ray window"):
        ops.generate_rays(K, T, 4, 4, first_ray=4, offset=(0.25, 0.0), device="cpu")
    with pytest.raises(ValueError, match="1-D int32"):
        ops.generate_rays(K, T, 4, 4, pixels=torch.zeros(2, 2, dtype=torch.int32), device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        ops.generate_rays(K, T, 4, 4, pixels=torch.zeros(2, dtype=torch.int32), device="cpu")
    state = ops.accumulate_state(8, 10, device="cpu")
    assert state.mean.shape == (8, 10) and state.m2.shape == (8, 3) and state.count.dtype == torch.int32 and state.n_pixels == 8
    with pytest.raises(RuntimeError, match="GPU"):
        ops.accumulate(torch.zeros(8, 10), state)
    with pytest.raises(ValueError):
        ops.accumulate_state(8, 2, 3, device="cpu")


# ---------------------------------------------------------------------------------------- the oracle against fp64 numpy
@pytest.mark.parametrize("k", [2, 3, 8, 32])
def test_the_oracle_agrees_with_fp64_numpy(k):
    """After k updates of fp32 samples with |x| <= 1, against the fp64 statistics of the same samples; e = 2^-24, the unit roundoff.

    Mean: update j rounds d (<= e |d|, carried on as e / j), d / j (<= e / j) and the sum (<= e |mean| <= e); the error it
    inherits is scaled by 1 - 1/j.  The first update is exact, so |mean - mean64| <= B_mean = (k + 2 ln k + 2) e.

    m2: each of the k - 1 products and sums rounds three times, a relative (3 k + 4) e in all; and a mean that is off by B_mean
    changes product j by at most B_mean (|d_j| + |x_j - mean_j|) <= 2 B_mean |d_j|, where sum |d_j| <= sqrt(2 k m2) because
    m2 = sum d_j^2 (1 - 1/j) >= sum d_j^2 / 2.  Divided by k - 1 (k >= 2: sqrt(2 k / (k - 1)) <= 2):
        |m2 / (k - 1) - var64| <= e ((3 k + 4) var64 + 4 (k + 2 ln k + 2) sqrt(var64)).
    The second term is what a quiet channel about a large mean pays (channel 1 below: sigma ~ 3e-4 about 0.5); "a few ulps"
    holds for the first alone.  Both bounds are asserted; the figures the oracle reaches are printed (measured: at most 0.17 of
    the mean's bound and 0.04 of the variance's)."""
    rng = np.random.RandomState(7 + k)
    P, Cw = 500, 10
    x = rng.rand(k, P, Cw).astype(F)
    x[:, :, 1] = x[:, :, 1] * F(1e-3) + F(0.5)                    # a quiet channel: small variance about a large mean
    state = A.State(P, Cw, 3)
    for j in range(k):
        A.update(state, x[j])
    assert (state.count == k).all()
    e = 2.0 ** -24
    mean64, var64 = x.astype(np.float64).mean(0), x.astype(np.float64).var(0, ddof=1)[:, :3]
    b_mean = (k + 2 * np.log(k) + 2) * e
    err_mean = np.abs(state.mean - mean64).max() / b_mean
    var = state.m2.astype(np.float64) / (k - 1)
    err_var = (np.abs(var - var64) / (e * ((3 * k + 4) * var64 + 4 * (k + 2 * np.log(k) + 2) * np.sqrt(var64)))).max()
    print(f"k={k}: mean error / bound = {err_mean:.3f}, variance error / bound = {err_var:.3f}")
    assert err_mean <= 1.0
    assert err_var <= 1.0
    # and the variance of the mean as the driver reports it: m2 / (k (k - 1)), one fp32 operation each
    assert A.same_bits(A.variance_of_mean(state), state.m2 / (F(k) * F(k - 1)))


def test_the_oracle_first_sample_rule_and_select_rule():
    s = A.State(4, 5, 3)
    x = np.array([[-0.0, 1.0, 2.0, 3.0, 4.0]] * 4, F)
    A.update(s, x[:2], pixels=[3, 1])
    assert s.count.tolist() == [0, 1, 0, 1] and np.signbit(s.mean[3, 0]) and not np.signbit(s.mean[0, 0]) and not s.m2.any()
    A.update(s, x[:1] + F(1), pixels=[3])
    assert s.count.tolist() == [0, 1, 0, 2] and s.mean[3].tolist() == [0.5, 1.5, 2.5, 3.5, 4.5] and s.m2[3].tolist() == [0.5, 0.5, 0.5]
    # pixel 3: variance of the mean = 0.5 / 2 = 0.25 = tol^2 at tol = 0.5: NOT above it
    assert A.select(s, 1, 4, 0.5).tolist() == [0, 2]
    assert A.select(s, 1, 4, 0.49).tolist() == [0, 2, 3]
    assert A.select(s, 2, 4, 0.5).tolist() == [0, 1, 2] and A.select(s, 1, 2, 0.0).tolist() == [0, 2] and A.select(s, 1, 1, 0.0).tolist() == [0, 2]
    assert A.select(s, 1, 4, 0.0).tolist() == [0, 2, 3]             # tol 0: m2 > 0 goes on; a pixel whose samples agree (m2 = 0) stops
