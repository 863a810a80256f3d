"""Early ray termination without a GPU: the rule's numpy restatement against a plain-Python walk on ten
hand-made rays, the host checks of the four new entries of the C ABI (all before any launch), the workspace function, the
``Termination`` state and the cross-rank fingerprint, the refusals of the render path, and -- on the CPU oracle alone -- the two
conditions of the oracle-compared GPU cases of tests/test_gpu_termination.py: at most 5 % of the rays left out by the margins,
at least 8 rays per terminated layer with both listed and hidden samples."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import occupancy_common as OC
import scene_edits_common as S
import termination_common as TC
from instances_common import base_model
from stnerf_amd import hip, ops
from stnerf_amd.termination import Termination
from test_occupancy_cpu import OnDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


# ---------------------------------------------------------------------------------------- the rule
def hand_made_rays():
    """Ten rays of l = 2 layers x n1 = 4 samples: (t [l][n1], wM [l][n1], tau, t_stop worked out by hand from the rule's text)."""
    t = [[1.0, 2.0, 3.0, 4.0], [1.5, 2.5, 3.5, 4.5]]          # merged: 1, 1.5, 2, 2.5, 3, 3.5, 4, 4.5
    z = [0.0] * 4
    tie = [[1.0, 2.0, 2.0, 4.0], [2.0, 2.0, 3.0, 5.0]]        # merged: 1, 2(0,1), 2(0,2), 2(1,0), 2(1,1), 3, 4, 5
    miss = [[-1000.0] * 4, [1.0, 2.0, 3.0, 4.0]]              # a layer the ray misses: first in the merge, weighs nothing
    return [
        (t, [[0.5, 0.25, 0.0, 0.0], [0.25, 0.0, 0.0, 0.0]], 0.125, 2.5),    # A = .5, .75, 1.0 -> j* = 2 (sample t = 2), next 2.5
        (t, [[0.1, 0.1, 0.1, 0.1], [0.1, 0.1, 0.1, 0.1]], 0.125, INF),      # never there: 1 - 0.8 > 0.125
        (t, [[0.1, 0.1, 0.1, 0.1], [0.1, 0.1, 0.1, 0.7]], 0.125, INF),      # stopped at its last sample
        (t, [[0.5, 0.25, 0.0, 0.0], [0.25, 0.0, 0.0, 0.0]], 0.0, 2.5),      # tau = 0, A exactly 1 at j = 2: !(0 > 0)
        (t, [[0.5, z[0], 0.0, 0.0], [float("nan"), 0.0, 0.0, 0.0]], 0.125, 2.0),   # a NaN weight at j = 1 stops the walk
        (t, [[0.01, 0.0, 0.0, 0.0], z], 0.995, 1.5),                        # tau so large that j* = 0
        (tie, [[0.0, 0.0, 1.0, 0.0], z], 0.5, 2.0),                         # j* = 2 (layer 0's second 2); next: layer 1's first 2
        (tie, [z, [0.0, 1.0, 0.0, 0.0]], 0.5, 3.0),                         # j* = 4 (layer 1's second 2), next 3
        (miss, [z, [0.0, 0.9, 0.0, 0.0]], 0.5, 3.0),                        # four zero-weight samples at -1000 come first
        (miss, [z, [1.0, 0.0, 0.0, 0.0]], 0.5, 2.0),
    ]


def test_the_numpy_rule_equals_a_plain_python_walk_on_ten_hand_made_rays():
    for k, (t, wm, tau, want) in enumerate(hand_made_rays()):
        assert TC.py_ray_stop(t, wm, tau) == want, (k, TC.py_ray_stop(t, wm, tau), want)
        got = TC.np_ray_stop(np.array([t], np.float32), np.array([wm], np.float32), tau)
        assert got.dtype == np.float32 and float(got[0]) == want, (k, float(got[0]), want)
    # all ten in one call (tau is per call: group by tau)
    rays = hand_made_rays()
    for tau in sorted({r[2] for r in rays}):
        sel = [r for r in rays if r[2] == tau]
        got = TC.np_ray_stop(np.array([r[0] for r in sel], np.float32), np.array([r[1] for r in sel], np.float32), tau)
        assert got.tolist() == [r[3] for r in sel]
    # random rays: the two restatements agree bit for bit
    rs = np.random.RandomState(3)
    t = np.sort(rs.uniform(0, 5, (40, 3, 7)).astype(np.float32), -1)
    t[:, 1, 3] = t[:, 0, 2]                                                      # ties across layers
    t = np.sort(t, -1)
    wm = (rs.uniform(0, 1, (40, 3, 7)) ** 4 * 0.4).astype(np.float32)
    got = TC.np_ray_stop(t, wm, 0.05)
    assert np.isfinite(got).any() and np.isinf(got).any()
    assert got.tolist() == [TC.py_ray_stop(t[i].tolist(), wm[i].tolist(), 0.05) for i in range(40)]


def test_hidden_samples_and_expected_rows():
    t = np.array([[1.0, 2.0, np.nan, 3.0], [1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0]], np.float32)
    stop = np.array([2.0, INF, 0.0], np.float32)
    assert TC.np_hidden(t, stop).tolist() == [[False, False, False, True], [False] * 4, [True] * 4]    # t == t_stop and NaN: listed
    w = lambda r, k: (r << 8) | k
    rows, listed = TC.np_visibility_rows(t, stop, [2, 0])
    assert rows.tolist() == [w(0, 0), w(0, 1), w(0, 2)] and not listed[1].any()
    occ = np.array([[True, False, True, True]] * 3)
    rows, _ = TC.np_visibility_rows(t, stop, [0, 1, 2], occ)
    assert rows.tolist() == [w(0, 0), w(0, 2), w(1, 0), w(1, 2), w(1, 3)]


# ---------------------------------------------------------------------------------------- the ABI
def test_entries_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "stnerf.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("stnerf_ray_stop", "stnerf_visibility_rows", "stnerf_render_workspace_bytes_terminated", "stnerf_render_rays_terminated"):
        assert name in hip.exported_symbols() and getattr(hip.lib(), name) is not None and name + "(" in header
    assert "Stop depth." in header and "Hidden sample." in header and "Stop depth." in design and "Hidden sample." in design
    assert ops.PROFILE_KERNELS[10:12] == ("ray_stop", "visibility_rows") and ops.PROFILE_KERNELS[9] == "occupancy_rows"
    assert all(callable(getattr(ops, f)) for f in ("ray_stop", "visibility_rows"))


def test_ray_stop_refuses_before_any_launch():
    f = hip.lib().stnerf_ray_stop
    fake = C.c_void_p(0x1000)
    call = lambda t=fake, w=fake, n=4, l=3, n1=8, tau=1e-4, out=fake: f(t, w, n, l, n1, tau, out, None)
    for kw, what in ((dict(t=None), "null"), (dict(w=None), "null"), (dict(out=None), "null"), (dict(l=0), "shape"),
                     (dict(l=hip.MAX_LAYERS + 1), "shape"), (dict(n1=0), "shape"), (dict(n=-1), "shape"), (dict(tau=-1e-6), "[0, 1)"),
                     (dict(tau=1.0), "[0, 1)"), (dict(tau=float("nan")), "[0, 1)")):
        assert call(**kw) == hip.EINVAL and what in hip.last_error(), (kw, hip.last_error())
    assert call(n=0) == hip.OK                                                    # nothing to do, nothing launched
    with pytest.raises(ValueError, match="alike"):
        ops.ray_stop(torch.zeros(4, 3, 8).as_subclass(OnDevice), torch.zeros(4, 3, 7).as_subclass(OnDevice), 1e-4)


def _grid():
    g = hip.Occupancy()
    g.bits = 0x1000
    for a in range(3):
        g.res[a], g.lo[a], g.inv_cell[a] = 8, 0.0, 4.0
    return g


def test_visibility_rows_refuses_before_any_launch():
    f = hip.lib().stnerf_visibility_rows
    fake, g = C.c_void_p(0x1000), _grid()
    def call(n=4, layer=1, ns=12, cap=48, grid=None, xyz=fake, t=fake, stop=fake):
        return f(None, None, n, layer, xyz, 3 * ns, t, ns, stop, ns, None if grid is None else C.byref(grid), fake, 4 * ns, fake, cap, fake, None, None)
    for kw, what in ((dict(ns=257, cap=4 * 257), "1..256"), (dict(n=(1 << 23) + 1, ns=1, cap=1 << 24), "2^23"), (dict(cap=47), "capacity"),
                     (dict(t=None), "null"), (dict(stop=None), "null"), (dict(layer=-1), "layer"), (dict(layer=hip.MAX_LAYERS), "layer"),
                     (dict(layer=0, grid=g), "layer 0"), (dict(grid=g, xyz=None), "points")):
        assert call(**kw) == hip.EINVAL and what in hip.last_error(), (kw, what, hip.last_error())
    bad = _grid()
    bad.res[1] = 300
    assert call(grid=bad) == hip.EINVAL and "1..256" in hip.last_error()
    x = torch.zeros(4, 12)
    with pytest.raises(ValueError, match="t_stop"):
        ops.visibility_rows(x.as_subclass(OnDevice), torch.zeros(3).as_subclass(OnDevice), torch.zeros(4, 12, 4).as_subclass(OnDevice))
    with pytest.raises(ValueError, match="points"):
        ops.visibility_rows(x.as_subclass(OnDevice), torch.zeros(4).as_subclass(OnDevice), torch.zeros(4, 12, 4).as_subclass(OnDevice),
                            grid=(torch.zeros(16, dtype=torch.int32), (8, 8, 8), [0, 0, 0], [4, 4, 4]))


def _render_args(l, precision, alpha=1.0):
    p, nets = hip.RenderParams(), hip.Nets()
    p.l, p.n1, p.n2, p.ray_stride, p.retiming, p.precision, p.alpha = l, 12, 6, 6 + l, 1, precision, alpha
    nets.bkgd = nets.bkgd_fine = 0x1000
    fake = C.c_void_p(0x1000)
    head = [fake, 8, fake, 0, C.byref(nets), C.byref(p), None, None, fake, 1 << 30, fake, fake, fake, fake, fake, None, None, None]
    return head, (p, nets)


def test_the_pipeline_entry_refuses_before_any_launch():
    f = hip.lib().stnerf_render_rays_terminated
    l = 3
    flags = lambda *v: (C.c_int32 * l)(*v)
    tail = lambda tau, fl, alpha=None: (alpha, None, None, None, None, tau, fl, None, None)
    head, keep = _render_args(l, 3)
    for tau in (-0.5, 1.0, float("nan")):
        assert f(*head, *tail(tau, flags(1, 1, 1))) == hip.EINVAL and "[0, 1)" in hip.last_error(), tau
    head, keep = _render_args(l, 2)
    assert f(*head, *tail(1e-4, flags(0, 1, 0))) == hip.EINVAL and "precision 2" in hip.last_error()
    head, keep = _render_args(l, 3, alpha=0.5)
    assert f(*head, *tail(1e-4, flags(1, 0, 0))) == hip.EINVAL and "alpha = 0.5" in hip.last_error()
    head, keep = _render_args(l, 3)
    table = (C.c_float * l)(1.0, 1.0, 0.75)
    assert f(*head, *tail(1e-4, flags(1, 0, 0), table)) == hip.EINVAL and "layer_alpha[2]" in hip.last_error()
    small = list(head)
    small[9] = hip.lib().stnerf_render_workspace_bytes(8, l, 12, 6, 0)                     # the workspace of a render without the flags
    assert f(*small, *tail(1e-4, flags(1, 0, 0))) == hip.EINVAL and "workspace" in hip.last_error()
    head, keep = _render_args(l, 3)
    keep[0].n1, keep[0].n2 = 200, 100
    assert f(*head, *tail(1e-4, flags(0, 1, 0))) == hip.EINVAL and "256" in hip.last_error()
    head, keep = _render_args(l, 3)
    big = list(head)
    big[1] = (1 << 23) + 1
    assert f(*big, *tail(1e-4, flags(0, 1, 0))) == hip.EINVAL and "2^23" in hip.last_error()
    head, keep = _render_args(l, 3)
    odd = C.c_void_p(0x1004)
    assert f(*head, None, None, None, None, None, 1e-4, flags(0, 1, 0), odd, None) == hip.EINVAL and "8-byte" in hip.last_error()
    # without a flag none of this is looked at: tau is not, and the call gets as far as the checks stnerf_render_rays_samples makes
    head, keep = _render_args(l, 2, alpha=0.5)
    small = list(head)
    small[9] = 16
    assert f(*small, *tail(7.0, None)) == hip.EINVAL and "workspace" in hip.last_error()
    assert f(*small, *tail(7.0, flags(0, 0, 0))) == hip.EINVAL and "workspace" in hip.last_error()


@pytest.mark.parametrize("n,l,n1,n2", [(128, 4, 12, 6), (64, 4, 64, 64), (7, 1, 5, 3)])
def test_the_workspace_grows_only_with_a_flag_and_a_fine_stage(n, l, n1, n2):
    lib = hip.lib()
    fl = lambda *v: (C.c_int32 * l)(*(list(v) + [0] * l)[:l])
    sam = fl(0, 1) if l > 1 else None
    for only_coarse in (0, 1):
        base = lib.stnerf_render_workspace_bytes_samples(n, l, n1, n2, only_coarse, None)
        base_s = lib.stnerf_render_workspace_bytes_samples(n, l, n1, n2, only_coarse, sam)
        assert base == lib.stnerf_render_workspace_bytes(n, l, n1, n2, only_coarse)
        assert lib.stnerf_render_workspace_bytes_terminated(n, l, n1, n2, only_coarse, None, None) == base
        assert lib.stnerf_render_workspace_bytes_terminated(n, l, n1, n2, only_coarse, None, fl()) == base
        assert lib.stnerf_render_workspace_bytes_terminated(n, l, n1, n2, only_coarse, sam, None) == base_s
        assert lib.stnerf_render_workspace_bytes_terminated(n, l, n1, n2, only_coarse, sam, fl()) == base_s
        assert ops.render_workspace_bytes(n, l, n1, n2, bool(only_coarse), terminate=[False] * l) == base
        if only_coarse:                                                            # nothing to terminate: the size of before
            assert lib.stnerf_render_workspace_bytes_terminated(n, l, n1, n2, 1, sam, fl(1, 1)) == base_s
            continue
        rows, stops = (n * (n1 + n2) * 4 + 255) // 256 * 256, (n * 4 + 255) // 256 * 256
        one = lib.stnerf_render_workspace_bytes_terminated(n, l, n1, n2, 0, None, fl(1))
        assert one >= base + rows + stops and one == ops.render_workspace_bytes(n, l, n1, n2, False, terminate=[True] + [False] * (l - 1))
        if l > 1:
            two = lib.stnerf_render_workspace_bytes_terminated(n, l, n1, n2, 0, None, fl(1, 1))
            assert two - one == rows
            both = lib.stnerf_render_workspace_bytes_terminated(n, l, n1, n2, 0, sam, fl(0, 1))     # the sample cull's list serves
            assert both - base_s == stops + 256
    assert lib.stnerf_render_workspace_bytes_terminated(-1, l, n1, n2, 0, None, None) == hip.EINVAL
    with pytest.raises(ValueError, match="one entry per layer"):
        ops.render_workspace_bytes(n, l, n1, n2, False, terminate=[True] * (l + 1))


# ---------------------------------------------------------------------------------------- the Python state
def test_set_termination_state_and_state_dict():
    model = base_model(2)
    keys = list(model.state_dict())
    assert model.termination is None and model._inference_only_edits() is None
    assert model.set_termination() is model
    t = model.termination
    assert isinstance(t, Termination) and t.tau == float(np.float32(1e-4)) and t.layers is None and t.background is True
    assert t.flags(model) == [True, True, True]
    model.hide_layer(2)
    assert t.flags(model) == [True, True, False]
    model.show_layer(2)
    model.set_termination(tau=0.01, layers=[2], background=False)
    assert model.termination.flags(model) == [False, False, True] and model.termination.tau == float(np.float32(0.01))
    assert "termination" in model._inference_only_edits()
    assert list(model.state_dict()) == keys                                        # no parameter, no buffer
    own = Termination(0.5)
    assert model.set_termination(own).termination is own
    model.set_termination(None)
    assert model.termination is None and model._inference_only_edits() is None
    for bad in (-0.1, 1.0, float("nan"), 2):
        with pytest.raises(ValueError, match="tau"):
            Termination(bad)
    with pytest.raises(ValueError, match="layers"):
        Termination(layers=[0])
    with pytest.raises(TypeError):
        Termination(background=1)
    with pytest.raises(ValueError, match="layers"):
        Termination(layers=[5]).flags(model)
    st = own.stats()
    assert st == dict(rows={})
    counts = own.counts("cpu")
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (hip.MAX_LAYERS, 2)
    counts[0] = torch.tensor([1 << 40, 9])
    assert own.stats()["rows"] == {0: (1 << 40, 9)} and not bool(counts.any())
    own.reset_stats()
    assert own.stats()["rows"] == {}


def test_the_cross_rank_fingerprint_covers_tau_and_the_flags():
    from stnerf_amd.parallel import layers_fingerprint
    model = base_model(2)
    off = layers_fingerprint(model)
    seen = [off]
    for kw in (dict(), dict(tau=1e-3), dict(background=False), dict(layers=[1]), dict(layers=[2]), dict(layers=[1, 2])):
        model.set_termination(**kw)
        fp = layers_fingerprint(model)
        assert len(fp) == len(off) and fp not in seen, kw
        seen.append(fp)
    model.set_termination(None)
    assert layers_fingerprint(model) == off
    assert len(Termination().fingerprint()) == 3


def test_the_renderer_takes_the_keyword():
    import types
    from stnerf_amd.render.layered_neural_renderer import LayeredNeuralRenderer
    model = base_model(2)
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=2, FRAME_NUM=3, FRAME_OFFSET=0), INPUT=types.SimpleNamespace(SIZE_TEST=[23, 17]))
    K, T = S.camera()
    r = LayeredNeuralRenderer(cfg, model=model, gt_poses=T.reshape(1, 4, 4), gt_Ks=[K])
    assert r.terminate is None and model.termination is None                       # off by default
    r = LayeredNeuralRenderer(cfg, model=model, gt_poses=T.reshape(1, 4, 4), gt_Ks=[K], terminate=True)
    first = r.terminate
    assert isinstance(first, Termination) and model.termination is first and first.tau == float(np.float32(1e-4))
    r.terminate = True
    assert r.terminate is first
    r.terminate = 0.01
    assert r.terminate.tau == float(np.float32(0.01))
    r.terminate = False
    assert model.termination is None
    with pytest.raises(TypeError):
        r.terminate = "yes"


def test_refusals_of_the_render_path():
    model = base_model(2)
    rays = torch.cat([torch.zeros(8, 6), torch.tensor([[1.0, 2.5, 3.0]]).repeat(8, 1)], 1)
    model.set_termination()
    model.train()
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="termination"):       # training: the op-by-op path
        model.render_rays_raw(rays.as_subclass(OnDevice))
    model.eval()
    model.alpha = 0.5
    with pytest.raises(ValueError, match="alpha = 0.5"):
        model.render_rays_raw(rays.as_subclass(OnDevice))
    model.alpha = 1.0
    model.layer_alpha = [1.0, None, 0.75]
    with pytest.raises(ValueError, match="layer_alpha"):
        model.render_rays_raw(rays.as_subclass(OnDevice))
    model.layer_alpha = None
    model.set_precision("fp32")
    model.mlp_schedule = "per_net"
    with pytest.raises(ValueError, match="per_net"):
        model.render_rays_raw(rays.as_subclass(OnDevice))
    model.mlp_schedule = "stage"
    model.set_precision("bf16x3")
    model.set_termination(None)


# ---------------------------------------------------------------------------------------- the oracle cases' conditions
def oracle_cases():
    """name -> (case, tau, flags).  The synthetic scene's random background net is dense: the coarse transmittance falls through
    1e-2 within the first samples of most rays, the performers are then wholly hidden, and at tau = 1e-4 three quarters of the rays
    (305 of 391) have 1 - A within EPS of tau at some merged sample -- the accumulated weight creeps up on 1.  So the cases use a
    LARGE tau (no scaled density head): 5e-3 with every layer terminated, 3e-3 with the performers 1 and 3 alone."""
    case = OC.plain_case()
    l = S.total_layers(case)
    return {"all layers, tau 5e-3": (case, 5e-3, [True] * l),
            "performers 1 and 3, tau 3e-3": (case, 3e-3, [False, True, False, True])}


@pytest.mark.parametrize("name", ["all layers, tau 5e-3", "performers 1 and 3, tau 3e-3"])
def test_conditions_of_the_oracle_compared_cases(monkeypatch, name):
    """Measured here (CPU oracle, the 17 x 23 view, (12, 6) samples), printed with `-s`: all layers at tau 5e-3: 5 of 391 rays left
    out, rays with listed and hidden samples per layer {0: 386, 1: 30, 2: 18, 3: 28}; performers 1 and 3 at tau 3e-3: 17 of 391 left
    out, {1: 40, 3: 41}.  Both conditions are asserted here before anything runs on a GPU."""
    case, tau, flags = oracle_cases()[name]
    rays = S.case_rays(case)
    n = rays.shape[0]
    ref32, i32 = TC.oracle_render_terminated(case, rays, torch.float32, tau, flags, monkeypatch)
    ref64, i64 = TC.oracle_render_terminated(case, rays, torch.float64, tau, flags, monkeypatch)
    excluded = TC.excluded_rays(i32, i64, flags)
    counts = TC.assert_termination_bites(i32, flags, ~excluded, name)
    print(f"{name}: {int(excluded.sum())} of {n} rays left out; rays with listed and hidden samples per terminated layer {counts}")
    assert excluded.mean() <= 0.05, (name, int(excluded.sum()), n)
    # termination changes the fine picture and nothing of the coarse one
    plain = S.oracle_render(case, rays)
    assert all(torch.equal(ref32[k], plain[k]) for k in ref32 if k.startswith(("coarse", "mask")) or k == "t_coarse")
    assert any(not torch.equal(ref32[k], plain[k]) for k in ref32 if k.startswith("fine_layer"))
    for i, f in enumerate(flags):
        if not f:
            assert torch.equal(ref32[f"fine_layer{i}"], plain[f"fine_layer{i}"]), i
    # (measured, not asserted: the stop depth bounds what the COARSE networks saw, and the synthetic fine networks are another random
    # field -- the mixed fine colour moves by up to 0.59 / 0.53 here)
    print(f"{name}: fine_mixed colour moves by at most {float((ref32['fine_mixed'][:, :3] - plain['fine_mixed'][:, :3]).abs().max()):.3e}")
