"""What the compositor-backward tests share (tests/test_composite_backward_cpu.py, tests/test_gpu_composite_backward.py,
tests/test_gpu_training.py): the reference autograd graph of a stage's composites, the merged order built on the host, the
input regimes and the per-segment error measure.  Importable without a GPU.

The yardstick is torch.autograd through the oracle's arithmetic (oracle/stnerf_oracle.py: gen_weight, composite) in fp64; the same
graph in fp32 is "the reference's own autograd arithmetic", the yardstick's own error (tests/test_gpu_backward.py).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import stnerf_oracle as O                                               # noqa: E402

GRAD_RTOL = 2e-5               # of the largest entry of the colour part / of the sigma part (tests/test_gpu_backward.py)
OPAQUE = 120.0                 # sigma' * delta of an "exactly opaque" sample: exp(-120) is 0 in fp32 and 8e-53 in fp64
NEAR = 0.35


# ---------------------------------------------------------------------------------------------------------------------
def _edited_sigma(t, sig, layer, fine, cut_neg, thresholds, scale, near):
    """The reference's in-place density edits on one layer's (n, S) densities (functional form: masked writes -> where)."""
    s = sig
    if (not fine) and cut_neg and layer > 0:
        s = torch.where(t < 0, torch.zeros_like(s), s)                 # :414
    if thresholds[layer] is not None:
        s = torch.where(s < thresholds[layer], torch.zeros_like(s), s)  # :416-418 / :538-547 / :564-566
    s = s * scale[layer]                                               # :575-576
    if (not fine) and layer == 0:
        s = torch.where(t < near, torch.zeros_like(s), s)              # :422
    return s


def _composite(t, rgb, sigma, border, rgb_activated):
    """O.composite, or the same with colours that are activated already (layers/render_layer.py:47 skipped)."""
    if not rgb_activated:
        return O.composite(t, rgb, sigma, border)
    delta = (t[:, 1:] - t[:, :-1]).squeeze(-1)
    delta = torch.cat([delta, border * torch.ones(delta.shape[0], 1, dtype=t.dtype)], dim=-1)
    w = O.gen_weight(sigma.squeeze(-1), delta).unsqueeze(-1)
    return torch.sum(rgb * w, dim=1), torch.sum(w * t, dim=1), torch.sum(w, dim=1), w


def _reference_composite(t, raw, mask, fine, cut_neg, thresholds, scale, near, evaluated, border=1e10, rgb_activated=False):
    """Autograd graph of a stage's composites in raw's dtype: per-layer (render_layer.py:25-58 on every evaluated layer) and the
    depth merge (:425-448 / :587-606), from raw (n,l,S,4) requiring grad.  ``mask`` None: every evaluated layer on every ray.
    ``rgb_activated``: raw[..., :3] are colours, no sigmoid is applied (the gradient is with respect to the activated colour)."""
    n, l, S = t.shape
    t = t.to(raw.dtype)
    rgbs, sigs = [], []
    for i in range(l):
        have = (torch.ones(n, dtype=torch.bool) if evaluated[i] == 2 or (evaluated[i] == 1 and mask is None) else
                (mask[:, i] != 0) if evaluated[i] == 1 else torch.zeros(n, dtype=torch.bool))
        hv = have.reshape(n, 1, 1).to(raw.dtype)
        rgbs.append(raw[:, i, :, :3] * hv + 0.0)
        s = _edited_sigma(t[:, i], raw[:, i, :, 3], i, fine, cut_neg, thresholds, scale, near) * have.reshape(n, 1).to(raw.dtype)
        sigs.append(s.unsqueeze(-1))
    layer = [_composite(t[:, i].unsqueeze(-1), rgbs[i], sigs[i], border, rgb_activated) for i in range(l)]
    # rgb of a layer without network output is a ZERO tensor in the reference: sigmoid(0) = 0.5, but its sigma = 0 makes it moot
    t_mix, order = torch.sort(t.reshape(n, l * S), dim=-1, stable=True)
    rgb_mix = torch.cat(rgbs, 1).gather(1, order.unsqueeze(-1).repeat(1, 1, 3))
    sig_mix = torch.cat(sigs, 1).gather(1, order.unsqueeze(-1))
    if fine:
        sig_mix = torch.where(t_mix.unsqueeze(-1) < near, torch.zeros_like(sig_mix), sig_mix)     # :605
    mixed = _composite(t_mix.unsqueeze(-1), rgb_mix, sig_mix, border, rgb_activated)
    layer_out = torch.stack([torch.cat([c[0], c[1], c[2]], -1) for c in layer], 1)                 # (n,l,5)
    mixed_out = torch.cat([mixed[0], mixed[1], mixed[2]], -1)
    return layer_out, mixed_out


def host_order(t):
    """The merged order of ``ops.composite(want_order=True)``, bit for bit (test_composite_merge_vs_oracle): a stable sort of the
    concatenated depths.  (n, l*S) int32."""
    n, l, S = t.shape
    return torch.sort(t.reshape(n, l * S), dim=-1, stable=True).indices.int()


def reference_kwargs(kw):
    """params-kwargs of a builder (those of ``ops.composite_params``) -> the keyword arguments of ``_reference_composite``."""
    l = len(kw["evaluated"])
    return dict(fine=kw["fine"], cut_neg=kw["cut_negative_t"], thresholds=list(kw.get("thresholds") or [None] * l),
                scale=list(kw.get("sigma_scale") or [1.0] * l), near=kw["near"], evaluated=kw["evaluated"], border=kw["border"],
                rgb_activated=kw.get("rgb_activated", False))


def reference_grad(t, raw, mask, kw, g_layer, g_mixed, dtype=torch.float64):
    """d (sum layer_out g_layer + sum mixed_out g_mixed) / d raw by autograd in ``dtype`` (either g may be None) -> (n,l,S,4) fp64."""
    r = raw.to(dtype).requires_grad_(True)
    lo, mo = _reference_composite(t.to(dtype), r, mask, **reference_kwargs(kw))
    loss = (0 if g_layer is None else (lo * g_layer.to(dtype)).sum()) + (0 if g_mixed is None else (mo * g_mixed.to(dtype)).sum())
    (grad,) = torch.autograd.grad(loss, r)
    return grad.double()


def reference_forward(t, raw, mask, kw, dtype=torch.float64):
    with torch.no_grad():
        return _reference_composite(t.to(dtype), raw.to(dtype), mask, **reference_kwargs(kw))


def part_errors(got, want):
    """(colour, sigma): max |got - want| of each part as a fraction of that part's largest reference entry."""
    got, want = got.double(), want.double()
    out = []
    for sl in (slice(0, 3), slice(3, 4)):
        scale = float(want[..., sl].abs().max())
        out.append(float((got[..., sl] - want[..., sl]).abs().max()) / max(scale, 1e-300))
    return tuple(out)


def dead_entries(mask, evaluated, n=None):
    """(n,l) bool: what the reference's zero tensors / overwritten densities cannot receive a gradient through."""
    l = len(evaluated)
    ev = torch.tensor(list(evaluated)).reshape(1, l)
    if mask is None:
        return (ev == 0).expand(n, l)
    return ((mask == 0) & (ev != 2)) | (ev == 0)


# ---------------------------------------------------------------------------------------------------------------------
# input regimes
def _params_kwargs(l, fine, evaluated=None, thresholds=None, sigma_scale=None, cut_negative_t=None, rgb_activated=False):
    if thresholds is None:
        thresholds = [0.05 if fine else None] + [0.1] * (l - 1)
    if sigma_scale is None:
        sigma_scale = [1.0] * l
        if fine and l > 2:
            sigma_scale[2] = 0.6
    if evaluated is None:
        evaluated = [2] + [1] * (l - 1)
        if l > 3:
            evaluated[3] = 0                                           # a hidden layer
    return dict(border=1e10, near=NEAR, fine=fine, cut_negative_t=(not fine) if cut_negative_t is None else cut_negative_t,
                thresholds=thresholds, sigma_scale=sigma_scale, evaluated=evaluated, rgb_activated=rgb_activated)


def _off_the_kinks(sig, thresholds_of_layer):
    """Move densities (n,l,S) that are within 2e-3 of 0 or of their layer's threshold away from it (the ReLU and the threshold are
    kinks: neither autograd nor a finite difference is defined across them)."""
    for i, th in enumerate(thresholds_of_layer):
        for k in (0.0,) + (() if th is None else (float(th),)):
            close = (sig[:, i] - k).abs() < 2e-3
            sig[:, i] = torch.where(close, torch.full_like(sig[:, i], k + 4e-3), sig[:, i])
    return sig


def soft_inputs(n, l, S, fine, seed=0, **params):
    """The regime of test_composite_backward_matches_fp64_autograd: ascending depths per layer over bins of about 6/S (some
    layers start below zero / below `near`), sigma ~ 0.3 +- 1.5, a missed layer (mask 0, half of them at depth -1000) on some
    rays.  -> t (n,l,S), raw (n,l,S,4), mask (n,l) uint8, params-kwargs, g_layer (n,l,5), g_mixed (n,5)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * l + S + int(fine))
    t = (torch.rand(n, l, S, generator=g) * 0.9 + 0.05).cumsum(-1) * (6.0 / S) - 0.4
    mask = (torch.rand(n, l, generator=g) < 0.7).to(torch.uint8)
    mask[:, 0] = 1
    t = torch.where((mask == 0).unsqueeze(-1) & (torch.rand(n, l, 1, generator=g) < 0.5), torch.full_like(t, -1000.0), t)
    raw = torch.randn(n, l, S, 4, generator=g)
    raw[..., 3] = raw[..., 3] * 1.5 + 0.3
    kw = _params_kwargs(l, fine, **params)
    if kw["rgb_activated"]:
        raw[..., :3] = torch.sigmoid(raw[..., :3])
    raw[..., 3] = _off_the_kinks(raw[..., 3].clone(), kw["thresholds"])
    g_layer, g_mixed = torch.randn(n, l, 5, generator=g), torch.randn(n, 5, generator=g)
    return t, raw, mask, kw, g_layer, g_mixed


def dense_inputs(n, l, S, fine, seed=0):
    """soft_inputs with sigma * 40: sigma' * delta up to about 10, alpha within a few ulp of 1 on many samples."""
    t, raw, mask, kw, g_layer, g_mixed = soft_inputs(n, l, S, fine, seed + 50)
    raw[..., 3] = raw[..., 3] * 40.0
    return t, raw, mask, kw, g_layer, g_mixed


def _stream_deltas(t, kw):
    """The bin widths every sample sees: in its layer's own composite (n,l,S) and in the merged one, at the source index."""
    n, l, S = t.shape
    border = kw["border"]
    d_layer = torch.cat([t[..., 1:] - t[..., :-1], torch.full((n, l, 1), border)], -1)
    order = host_order(t).long()
    tm = t.reshape(n, l * S).gather(1, order)
    d_m = torch.cat([tm[:, 1:] - tm[:, :-1], torch.full((n, 1), border)], -1)
    d_merged = torch.empty(n, l * S).scatter_(1, order, d_m).reshape(n, l, S)
    return d_layer, d_merged, order


def edited_sigma(t, raw, mask, kw):
    """sigma' (n,l,S) of the layers' own composites and of the merged one (the fine stage cuts the latter below `near`)."""
    r = reference_kwargs(kw)
    n, l, S = t.shape
    out = []
    for i in range(l):
        have = (torch.ones(n, dtype=torch.bool) if r["evaluated"][i] == 2 or (r["evaluated"][i] == 1 and mask is None) else
                (mask[:, i] != 0) if r["evaluated"][i] == 1 else torch.zeros(n, dtype=torch.bool))
        out.append(_edited_sigma(t[:, i], raw[:, i, :, 3], i, r["fine"], r["cut_neg"], r["thresholds"], r["scale"], r["near"])
                   * have.reshape(n, 1).to(raw.dtype))
    s = torch.stack(out, 1)
    return s, (torch.where(t < r["near"], torch.zeros_like(s), s) if r["fine"] else s)


def opaque_in_front(t, raw, mask, kw):
    """Per sample, the number of exactly opaque samples (relu(sigma') * delta >= 104: exp is 0 in fp32) in front of it:
    (in its layer's own composite (n,l,S), in the merged composite (n,l,S) at the source index, opaque-anywhere (n,l,S) bool)."""
    n, l, S = t.shape
    d_layer, d_merged, order = _stream_deltas(t, kw)
    s_layer, s_merged = edited_sigma(t, raw, mask, kw)
    op_layer = s_layer.clamp(min=0) * d_layer >= 104.0
    op_merged = s_merged.clamp(min=0) * d_merged >= 104.0
    front_layer = op_layer.long().cumsum(-1) - op_layer.long()
    om = op_merged.reshape(n, l * S).gather(1, order).long()
    front_merged = torch.empty(n, l * S, dtype=torch.long).scatter_(1, order, om.cumsum(-1) - om).reshape(n, l, S)
    return front_layer, front_merged, op_layer | op_merged


def opaque_inputs(n, l, S, fine, seed=0, most=3, gap_layer=16, gap_merged=24):
    """soft_inputs with up to ``most`` = 3 samples per ray made exactly opaque, sigma' * delta >= 120 in the sample's own layer
    and in the merged stream (three per ray are at most three per stream, the merged one included: a fourth would put T at 1e-40,
    subnormal in fp32).  exp(-120) is 0 in fp32 and 8e-53 in fp64: both arithmetics have om = 1e-10 there.
    The opaque samples stand at least ``gap_layer`` samples apart (and from the ends) in their layer and ``gap_merged`` in the merged
    stream: a segment of one or two live samples has nothing to be normalised by but its own entry, and d alpha = gw T - behind / om
    cancels to any degree in a single entry -- there the fp32 reference itself is 2.4e-5 off fp64 (measured: a one-sample segment).
    -> t, raw, mask, params-kwargs, g_layer, g_mixed, (front_layer, front_merged, opaque): ``opaque_in_front``."""
    t, raw, mask, kw, g_layer, g_mixed = soft_inputs(n, l, S, fine, seed + 100)
    g = torch.Generator().manual_seed(77 + seed)
    d_layer, d_merged, order = _stream_deltas(t, kw)
    r = reference_kwargs(kw)
    live = dead_entries(mask, kw["evaluated"]).logical_not().reshape(n, l, 1).expand(n, l, S)
    # where an opaque sample can stand: a layer the ray reads, behind `near`, not the last of either stream, a bin that is no sliver
    ok = live & (t > r["near"] + 0.05) & (d_layer < 1e9) & (d_merged < 1e9) & (torch.minimum(d_layer, d_merged) > 1e-3)
    pos = torch.empty(n, l * S, dtype=torch.long).scatter_(1, order, torch.arange(l * S).expand(n, l * S)).reshape(n, l, S)
    ok &= (pos >= gap_merged) & (pos < l * S - gap_merged)
    ok[..., :gap_layer] = False
    ok[..., S - gap_layer:] = False
    for ray in range(n):
        cand = ok[ray].nonzero()
        want = int(torch.randint(0, most + 1, (1,), generator=g))
        pick = []
        for i, k in cand[torch.randperm(len(cand), generator=g)].tolist():
            if len(pick) == want:
                break
            if all(abs(int(pos[ray, i, k] - pos[ray, j, m])) >= gap_merged and (i != j or abs(k - m) >= gap_layer) for j, m in pick):
                pick.append((i, k))
        for i, k in pick:
            raw[ray, i, k, 3] = OPAQUE / (float(torch.minimum(d_layer, d_merged)[ray, i, k]) * r["scale"][i])
    fronts = opaque_in_front(t, raw, mask, kw)
    assert int(fronts[0].max()) <= most and int(fronts[1].max()) <= most
    return t, raw, mask, kw, g_layer, g_mixed, fronts


def alternating_inputs(n, l, S, fine, seed=0):
    """soft_inputs for the long batches: rays with every layer live alternate with rays whose performers are missed (mask 0, depths
    -1000; with one layer, that layer) -- a wave's next ray then runs over the LDS its previous ray filled.  The kernel's grid-stride
    is an even number of rays, so the alternation is drawn per ray (a fair coin), not by parity: a wave meets every succession."""
    t, raw, mask, kw, g_layer, g_mixed = soft_inputs(n, l, S, fine, seed, evaluated=[2] + [1] * (l - 1) if l > 1 else [1])
    missed = torch.rand(n, generator=torch.Generator().manual_seed(5 + seed)) < 0.5
    mask[:] = 1
    first = 1 if l > 1 else 0
    mask[missed, first:] = 0
    t[missed, first:] = -1000.0
    return t, raw, mask, kw, g_layer, g_mixed


def order_inputs(seed=23):
    """The depth patterns of test_composite_descending_and_unsorted_layers (l = 3, S = 17, n = 60) plus two layers with identical
    depth lists, grazing rays (all samples of a layer at one depth) and missed layers at -1000 (mask 0).  No edits: the merged
    composite only (a descending layer's own composite is inf / NaN in the reference as well), so g_layer is None."""
    g = torch.Generator().manual_seed(seed)
    n, l, S = 60, 3, 17
    t = torch.sort(torch.rand(n, l, S, generator=g) * 4.0, -1)[0]
    t[:20, 0] = t[:20, 0].flip(-1)                                # strictly descending background
    t[10:30, 2] = t[10:30, 2].flip(-1)                            # ... and / or a descending performer
    t[40:50, 1] = t[40:50, 1][:, torch.randperm(S, generator=g)]  # unsorted
    t[50:, 1] = t[50:, 1].flip(-1)
    t[50:, 1, 3] = t[50:, 1, 2]                                   # a tie inside a descending list: general rank
    t[30:36, 2] = t[30:36, 1]                                     # two layers with identical depth lists
    t[36:40, 1] = t[36:40, 1, 5:6].clone()                        # grazing: all samples of a layer at one depth
    t[38:40, 0] = t[38:40, 0, 2:3].clone()
    mask = torch.ones(n, l, dtype=torch.uint8)
    t[5:10, 1], mask[5:10, 1] = -1000.0, 0                        # missed layers
    t[44:48, 2], mask[44:48, 2] = -1000.0, 0
    raw = torch.randn(n, l, S, 4, generator=g)
    raw[..., 3] = _off_the_kinks(raw[..., 3].clone(), [None] * l)
    kw = _params_kwargs(l, False, evaluated=[2, 1, 1], thresholds=[None] * l, sigma_scale=[1.0] * l, cut_negative_t=False)
    kw["near"] = 0.0
    return t, raw, mask, kw, None, torch.randn(n, 5, generator=g)


# ---------------------------------------------------------------------------------------------------------------------
def segment_errors(got, want, front, opaque):
    """Per ray and per segment -- the run of samples of a stream with the same count of opaque samples in front -- the largest
    |got - want| as a fraction of the segment's largest |want|.  got, want (n,l,S,4); front (n,l,S) counts; opaque (n,l,S) bool:
    left out of the sigma comparison (fp64 gives them ~1e-50, fp32 exactly 0).  ``front`` counted per layer groups the samples of a
    (ray, layer); counted in the merged stream, of a ray.  Segments whose (remaining) fp64 maximum is 0 are skipped.
    -> (colour, sigma): the worst segment of each part."""
    got, want = got.double(), want.double()
    n, l, S = front.shape
    worst = []
    for part in ("colour", "sigma"):
        if part == "colour":
            e, w = (got[..., :3] - want[..., :3]).abs().amax(-1), want[..., :3].abs().amax(-1)
        else:
            keep = (~opaque).double()
            e, w = (got[..., 3] - want[..., 3]).abs() * keep, want[..., 3].abs() * keep
        m = 0.0
        for c in range(int(front.max()) + 1):
            sel = (front == c).double()
            emax, wmax = (e * sel).amax(-1), (w * sel).amax(-1)       # (n,l): per ray, per layer
            emax, wmax = emax.reshape(n, -1), wmax.reshape(n, -1)
            live = wmax > 0
            if live.any():
                m = max(m, float((emax[live] / wmax[live]).max()))
        worst.append(m)
    return tuple(worst)


def merged_segment_errors(got, want, front_merged, opaque):
    """``segment_errors`` with the segments of the merged stream: a ray's samples of every layer together."""
    n, l, S = front_merged.shape
    flat = lambda x: x.reshape(n, 1, l * S, *x.shape[3:])
    return segment_errors(flat(got), flat(want), flat(front_merged), flat(opaque))
