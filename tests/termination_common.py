"""Shared by tests/test_termination_cpu.py and tests/test_gpu_termination.py: early ray termination's rule (include/stnerf.h /
DESIGN.md section 7: "Stop depth", "Hidden sample") restated in numpy from that text, and the oracle's expectation of a terminated
render: ``O.space_net`` wrapped (by the test, with pytest's monkeypatch) so that colour and sigma of a terminated layer are zero at
its hidden fine samples -- which is ``sig[i]``, ``rgbs[i]`` zeroed at the return of the fine ``run_nets``: the cuts and factors
between the network and that return keep a zero a zero.  The oracle's OWN coarse weights decide what is hidden."""
import numpy as np
import torch

from oracle import stnerf_oracle as O

import sample_rows_common as SR
import scene_edits_common as S

EPS = 5.5e-5      # the fp32 / fp64 resampling spread the sample cull measured (tests/test_sample_cull_cpu.py: "full edits")


# ---------------------------------------------------------------------------------------- the rule
def np_ray_stop(t, wm, tau, dtype=np.float32, margin=None):
    """t, wm (n,l,n1) -> t_stop (n,) in ``dtype`` (fp32: the rule itself; fp64: the same walk for an fp64 oracle).  The l n1
    samples of a ray are merged by depth, stably, ties broken by the source index; one accumulator A <- A + wM[src(j)] walks the
    merged list; j* is the first j with not (1 - A > tau); t_stop is the depth of merged sample j* + 1, +inf without one.
    margin (a float): also return close (n,) bool: |(1 - A) - tau| <= margin at some merged sample up to and including j*."""
    t, wm = np.asarray(t, dtype), np.asarray(wm, dtype)
    n, l, n1 = t.shape
    total = l * n1
    order = np.argsort(t.reshape(n, total), axis=1, kind="stable")
    ts = np.take_along_axis(t.reshape(n, total), order, 1)
    ws = np.take_along_axis(wm.reshape(n, total), order, 1)
    one, tau = dtype(1.0), dtype(tau)
    acc = np.zeros(n, dtype)
    out = np.full(n, np.inf, dtype)
    walking = np.ones(n, bool)
    close = np.zeros(n, bool)
    with np.errstate(invalid="ignore"):
        for j in range(total):
            acc = np.where(walking, (acc + ws[:, j]).astype(dtype), acc)
            left = (one - acc).astype(dtype)
            if margin is not None:
                close |= walking & (np.abs(left.astype(np.float64) - float(tau)) <= margin)
            stop = walking & ~(left > tau)
            if j + 1 < total:
                out[stop] = ts[stop, j + 1]
            walking &= ~stop
    return (out, close) if margin is not None else out


def py_ray_stop(t, wm, tau):
    """One ray, plain Python: t, wm [l][n1] lists of floats -> t_stop.  An l-way merge in which the lower layer wins a tie."""
    f = np.float32
    l, n1 = len(t), len(t[0])
    cur = [0] * l
    acc, tau = f(0.0), f(tau)
    merged = []
    for _ in range(l * n1):
        best = None
        for i in range(l):
            if cur[i] < n1 and (best is None or f(t[i][cur[i]]) < f(t[best][cur[best]])):
                best = i
        merged.append((f(t[best][cur[best]]), f(wm[best][cur[best]])))
        cur[best] += 1
    for j, (_, w) in enumerate(merged):
        acc = f(acc + w)
        if not (f(f(1.0) - acc) > tau):
            return float(merged[j + 1][0]) if j + 1 < len(merged) else float("inf")
    return float("inf")


def np_hidden(t_f, t_stop):
    """t_f (n, ns), t_stop (n,) -> bool (n, ns): the sample is hidden (a NaN depth is not)."""
    with np.errstate(invalid="ignore"):
        return np.asarray(t_f) > np.asarray(t_stop)[:, None]


def np_visibility_rows(t, t_stop, rays, occupied=None):
    """One layer's expected row list.  t (n, ns); rays: the listed ray indices; occupied (n, ns) bool | None: the grid rule's
    verdict -> (sorted words ray << 8 | k, listed (n, ns) bool with False on rays not tested)."""
    return SR.np_sample_rows(t.shape[0], t.shape[1], rays=rays, t=t, t_stop=t_stop, occupied=occupied)


# ---------------------------------------------------------------------------------------- the oracle's expectation
class TerminatedNets:
    """The wrapper for ``O.space_net`` during the FINE stage of one chunk.  hidden[i] (n, S) bool per layer (None: the layer is not
    terminated); masks[i] (n,) bool; performer calls come in layer order, one per shown layer with a hit ray."""

    def __init__(self, m, hidden, masks, ns):
        self.m, self.hidden, self.masks, self.ns = m, hidden, masks, ns
        self.space = O.space_net
        self.pending = [i for i in range(1, len(masks)) if bool(masks[i].any()) and m.is_shown_layer(i)]

    def space_net(self, params, prefix, pos, dirs, times=None):
        rgb, sigma = self.space(params, prefix, pos, dirs, times)
        if pos.shape[1] != self.ns:
            return rgb, sigma
        if prefix == "bkgd_spacenet_fine":
            i, rows = 0, slice(None)
        else:
            assert prefix.startswith("spacenets_fine."), prefix
            i = self.pending.pop(0)
            assert int(prefix.rsplit(".", 1)[1]) == self.m.module_of(i), (prefix, i)
            rows = self.masks[i]
        if self.hidden[i] is None:
            return rgb, sigma
        off = self.hidden[i][rows]
        assert off.shape == sigma.shape[:2], (off.shape, sigma.shape)
        rgb, sigma = rgb.clone(), sigma.clone()
        rgb[off] = 0
        sigma[off] = 0
        return rgb, sigma


def oracle_render_terminated(case, rays, dtype, tau, flags, monkeypatch, params=None):
    """The oracle on the case with the fine stage terminated by the rule, on its own coarse merged weights, reference chunk by
    reference chunk -> (``scene_edits_common.flat`` dict with t_coarse, info): info = dict of (n, ...) arrays: t_stop, close (a
    merged sample with 1 - A within EPS of tau), per terminated layer i hidden{i} (n, S) bool, near{i} (n,) bool (a fine depth of a
    ray the layer is evaluated on within EPS of t_stop without being t_stop itself) and both{i} (n,) bool (evaluated, with listed and hidden samples).
    flags: one per layer.  params: a state dict in place of the case's (a scaled density head)."""
    rays = rays.to(torch.float32)
    m = S.oracle_model(case, dtype)
    if params is not None:
        m.params = {k: v.to(dtype) for k, v in params.items()}
    npdt = np.float32 if dtype == torch.float32 else np.float64
    jitter, u = S.case_draws(case)
    l, step, n, ns = S.total_layers(case), case["chunk"], rays.shape[0], case["n1"] + case["n2"]
    assert len(flags) == l and not case["only_coarse"]
    kw = dict(density_threshold=case["thr"], bkgd_density_threshold=case["bthr"])
    outs, ts = [], []
    info = dict(t_stop=np.zeros(n, npdt), close=np.zeros(n, bool))
    for i in range(l):
        if flags[i]:
            info[f"hidden{i}"], info[f"near{i}"], info[f"both{i}"] = np.zeros((n, ns), bool), np.zeros(n, bool), np.zeros(n, bool)
    with torch.no_grad():
        for s in range(0, n, step):
            e = min(s + step, n)
            chunk = rays[s:e].to(dtype)
            mk = lambda: iter([jitter[i, s:e] for i in range(l)] + [u[i, s:e] for i in range(l)])
            d, ta, tb = mk(), {}, {}
            O.render_chunk(m, chunk, only_coarse=True, rand=lambda shape: next(d), trace=ta, **kw)        # the coarse merged weights
            d = mk()
            O.render_chunk(m, chunk, rand=lambda shape: next(d), trace=tb, **kw)                            # the fine depths
            t_c = torch.stack([t.squeeze(-1) for t in ta["t_coarse"]], 1).numpy()
            t_stop, close = np_ray_stop(t_c, ta["merged_weights"].numpy(), tau, npdt, margin=EPS)
            info["t_stop"][s:e], info["close"][s:e] = t_stop, close
            hidden = [None] * l
            for i in range(l):
                if not flags[i] or (i > 0 and not m.is_shown_layer(i)):
                    continue
                t_f = tb["t_fine"][i].numpy()
                hidden[i] = torch.from_numpy(np_hidden(t_f, t_stop))
                evaluated = np.ones(e - s, bool) if i == 0 else tb["mask"][i].numpy()
                with np.errstate(invalid="ignore"):
                    # (a depth EQUAL to t_stop is the coarse sample that defines it, copied into the fine list in every arithmetic:
                    # listed by the rule, everywhere -- the margin is for the depths beside it)
                    near = ((np.abs(t_f.astype(np.float64) - t_stop.astype(np.float64)[:, None]) <= EPS) & (t_f != t_stop[:, None])).any(-1)
                info[f"hidden{i}"][s:e] = hidden[i].numpy() & evaluated[:, None]
                info[f"near{i}"][s:e] = near & evaluated
                info[f"both{i}"][s:e] = evaluated & hidden[i].numpy().any(-1) & ~hidden[i].numpy().all(-1)
            nets = TerminatedNets(m, hidden, tb["mask"], ns)
            monkeypatch.setattr(O, "space_net", nets.space_net)
            try:
                d, trace = mk(), {}
                outs.append(O.render_chunk(m, chunk, rand=lambda shape: next(d), trace=trace, scene=True, **kw))
            finally:
                monkeypatch.undo()
            assert not nets.pending
            ts.append(torch.stack([t.squeeze(-1) for t in trace["t_coarse"]], 1))
    cat3 = lambda trips: tuple(torch.cat([t[j] for t in trips], 0) for j in range(3))
    whole = (cat3([o[0] for o in outs]), cat3([o[1] for o in outs]))
    whole += tuple([cat3([o[k][i] for o in outs]) for i in range(l)] for k in (2, 3))
    whole += ([torch.cat([o[4][i] for o in outs], 0) for i in range(l)], [cat3([o[5][i] for o in outs]) for i in range(l)])
    return S.flat(whole, torch.cat(ts, 0)), info


def excluded_rays(info32, info64, flags):
    """The rays left out of the oracle comparison: the fp32 and the fp64 evaluation may classify a sample differently where 1 - A
    lies within EPS of tau at some merged sample, or a terminated layer's fine depth within EPS of t_stop -- in either oracle."""
    out = info32["close"] | info64["close"]
    for i, f in enumerate(flags):
        if f:
            out = out | info32[f"near{i}"] | info64[f"near{i}"]
    return out


def assert_termination_bites(info, flags, keep, what=""):
    """At least 8 kept rays per terminated layer with both listed and hidden samples -> {layer: count}."""
    counts = {i: int((info[f"both{i}"] & keep).sum()) for i, f in enumerate(flags) if f}
    assert counts and min(counts.values()) >= 8, f"{what}: rays with listed and hidden samples per terminated layer {counts}"
    return counts
