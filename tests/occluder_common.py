"""Shared by tests/test_occluder_cpu.py and tests/test_gpu_occluder.py: depth-tested occluder compositing (include/stnerf.h /
DESIGN.md sections 4.2 and 7) restated from that text -- the present / absent rule, the mix and the stop rule in numpy, fp32, one
rounding per operation in the order written -- the CPU oracle's statement of the occluded outputs (the front / behind sums and the
mix applied in torch, in the oracle's dtype, to what ``O.render_chunk`` traces), the oracle case with its occluder, the conditions
the case must meet on the oracle alone, and the comparison with the oracle (``scene_edits_common.assert_matches_oracle`` as it is,
on the rays the conditions keep)."""
import numpy as np
import torch

from oracle import stnerf_oracle as O

import scene_edits_common as S

EPS = 5.5e-5          # the fp32 / fp64 spread of a fine depth (tests/termination_common.py: the project's figure)
MAX_LEFT_OUT = 0.05   # of the rays
MIN_SPLIT_RAYS = 8    # compared present rays per layer with samples on both sides of z
SPLIT_WEIGHT = 1e-6
F = np.float32


# ---------------------------------------------------------------------------------------- the rules, numpy fp32
def np_present(occ):
    """occ (n,5) rows {r, g, b, a, z} -> (a' (n,) fp32, present (n,) bool): a' = a clamped to [0, 1], a NaN counts as 0; present
    when a' > 0 and z is finite."""
    occ = np.asarray(occ, F)
    a, z = occ[:, 3], occ[:, 4]
    with np.errstate(invalid="ignore"):
        ap = np.where(a > 0, a, F(0)).astype(F)
        ap = np.where(ap < 1, ap, F(1)).astype(F)
    return ap, (ap > 0) & np.isfinite(z)


def np_mix(front, behind, occ, scene_in, mixed_in):
    """front, behind, scene_in (n,l,5), occ, mixed_in (n,5) -> (occluded_mixed (n,5), occluded_scene (n,l,5), share (n,5)), fp32,
    every product, sum and difference rounded once, in the order the definition writes them; absent rows: the plain outputs."""
    front, behind, occ = np.asarray(front, F), np.asarray(behind, F), np.asarray(occ, F)
    n, l, _ = front.shape
    ap, present = np_present(occ)
    with np.errstate(invalid="ignore", over="ignore"):
        af = front[:, 0, 4].copy()
        for i in range(1, l):
            af = (af + front[:, i, 4]).astype(F)
        left = (F(1) - af).astype(F)
        T = np.where(left > 0, left, F(0)).astype(F)
        s = (ap * T).astype(F)
        q = (F(1) - ap).astype(F)
        passes = (front + (q[:, None, None] * behind).astype(F)).astype(F)
        x = np.concatenate([occ[:, 0:3], occ[:, 4:5], np.ones((n, 1), F)], 1)
        share = (s[:, None] * x).astype(F)
        total = passes[:, 0].copy()
        for i in range(1, l):
            total = (total + passes[:, i]).astype(F)
        mixed = (total + share).astype(F)
    p1, p2 = present[:, None], present[:, None, None]
    return (np.where(p1, mixed, np.asarray(mixed_in, F)), np.where(p2, passes, np.asarray(scene_in, F)),
            np.where(p1, share, F(0)).astype(F))


def np_front_behind(occ, scene_in):
    """What front_out / behind_out hold on ABSENT rows: the scene pass and zeros (present rows: NaN, to be filled by the caller)."""
    _, present = np_present(occ)
    scene_in = np.asarray(scene_in, F)
    p = present[:, None, None]
    return np.where(p, F(np.nan), scene_in), np.where(p, F(np.nan), F(0)).astype(F)


def np_stop(occ, t_stop):
    """t_stop[ray] = (present && a' >= 1 && z < t_stop[ray]) ? z : t_stop[ray]."""
    occ, t_stop = np.asarray(occ, F), np.asarray(t_stop, F)
    ap, present = np_present(occ)
    with np.errstate(invalid="ignore"):
        take = present & (ap >= 1) & (occ[:, 4] < t_stop)
    return np.where(take, occ[:, 4], t_stop)


def exact_front_behind(t, wm, colour, occ, have):
    """The two sums in fp64 from fp32 inputs: t, wm (n,l,S), colour (n,l,S,3) as the compositor uses it, have (n,l) bool (the layer
    has network output on the ray) -> (front, behind, magnitude) (n,l,5) fp64; magnitude = sum_k |wM x| over ALL samples of the
    layer, the scale of the rounding bound.  Present rows only are meaningful."""
    t64, w64 = np.asarray(t, np.float64), np.asarray(wm, np.float64)
    x = np.concatenate([np.asarray(colour, np.float64), t64[..., None], np.ones(t64.shape + (1,))], -1)
    with np.errstate(invalid="ignore"):
        behind = np.asarray(t, F) >= np.asarray(occ, F)[:, 4][:, None, None]
    wx = np.where(np.asarray(have, bool)[:, :, None, None], w64[..., None] * x, 0.0)     # (a layer without output is not read)
    return (wx * ~behind[..., None]).sum(2), (wx * behind[..., None]).sum(2), np.abs(wx).sum(2)


# ---------------------------------------------------------------------------------------- the oracle's statement
def torch_occluded(t, colour, wm, scene, mixed, occ, wrong=None):
    """One chunk in the oracle's dtype.  t, wm (n,l,S); colour (n,l,S,3) = sigmoid(rgb); scene (n,l,5) and mixed (n,5) the oracle's
    scene passes and mix; occ (n,5) -> dict(mixed (n,5), scene (n,l,5), share (n,5), behind (n,l,S) bool, present (n,)).
    wrong (the CPU tests' deliberate errors): "gt" = `>` in place of `>=`; "q_front" = q applied to front; "T_whole" = T taken from
    the whole ray."""
    one, zero = torch.ones((), dtype=t.dtype), torch.zeros((), dtype=t.dtype)
    a, z = occ[:, 3], occ[:, 4]
    ap = torch.where(a > 0, a, zero)
    ap = torch.where(ap < 1, ap, one)
    present = (ap > 0) & torch.isfinite(z)
    zz = z.view(-1, 1, 1)
    behind = (t > zz) if wrong == "gt" else (t >= zz)
    x = torch.cat([colour, t.unsqueeze(-1), torch.ones_like(t).unsqueeze(-1)], -1)
    front = (torch.where(behind, zero, wm).unsqueeze(-1) * x).sum(2)
    back = (torch.where(behind, wm, zero).unsqueeze(-1) * x).sum(2)
    l = t.shape[1]
    af = front[:, 0, 4]
    for i in range(1, l):
        af = af + front[:, i, 4]
    if wrong == "T_whole":
        for i in range(l):
            af = af + back[:, i, 4]
    T = torch.clamp(1 - af, min=0)
    s, q = ap * T, (1 - ap).view(-1, 1, 1)
    passes = (q * front + back) if wrong == "q_front" else (front + q * back)
    share = s.view(-1, 1) * torch.cat([occ[:, 0:3], z.view(-1, 1), torch.ones_like(z).view(-1, 1)], -1)
    total = passes[:, 0]
    for i in range(1, l):
        total = total + passes[:, i]
    p1, p2 = present.view(-1, 1), present.view(-1, 1, 1)
    return dict(mixed=torch.where(p1, total + share, mixed), scene=torch.where(p2, passes, scene),
                share=torch.where(p1, share, zero), behind=behind, present=present)


def oracle_occluded(case, occ, dtype=torch.float32, rays=None, wrong=None):
    """The oracle on the case, reference chunk by reference chunk as ``scene_edits_common.oracle_render`` runs it, with the
    occluder ``occ`` (N,5) fp32 composited by the definition -> (flat dict: fine_occluded_mixed, fine_occluded_scene{i},
    fine_occluder_share, each (N,5) in ``dtype``; info: t_fine, merged_weights (N,l,S), behind (N,l,S) bool, present (N,) bool)."""
    assert not case["only_coarse"]
    rays = S.case_rays(case) if rays is None else rays
    m = S.oracle_model(case, dtype)
    jitter, u = S.case_draws(case)
    l, step, n = S.total_layers(case), case["chunk"], rays.shape[0]
    occ = torch.as_tensor(np.asarray(occ, F))
    assert tuple(occ.shape) == (n, 5)
    parts = {k: [] for k in ("mixed", "scene", "share", "behind", "present", "t", "wm")}
    with torch.no_grad():
        for s in range(0, n, step):
            e = min(s + step, n)
            draws = iter([jitter[i, s:e] for i in range(l)] + [u[i, s:e] for i in range(l)])
            trace = {}
            out = O.render_chunk(m, rays[s:e].to(dtype), rand=lambda shape: next(draws), trace=trace, scene=True,
                                 density_threshold=case["thr"], bkgd_density_threshold=case["bthr"])
            t = torch.stack(trace["t_fine"], 1)
            colour = torch.stack([torch.sigmoid(c) for c in trace["rgb_fine"]], 1)
            scene = torch.stack([torch.cat(p, -1) for p in out[5]], 1)
            r = torch_occluded(t, colour, trace["merged_weights"], scene, torch.cat(out[0], -1), occ[s:e].to(dtype), wrong)
            for k in ("mixed", "scene", "share", "behind", "present"):
                parts[k].append(r[k])
            parts["t"].append(t)
            parts["wm"].append(trace["merged_weights"])
    cat = {k: torch.cat(v, 0) for k, v in parts.items()}
    flat = {"fine_occluded_mixed": cat["mixed"], "fine_occluder_share": cat["share"]}
    for i in range(l):
        flat[f"fine_occluded_scene{i}"] = cat["scene"][:, i].contiguous()
    info = dict(t_fine=cat["t"], merged_weights=cat["wm"], behind=cat["behind"], present=cat["present"])
    return flat, info


# ---------------------------------------------------------------------------------------- the oracle case
def oracle_case():
    """``scene_edits_common.make_case()``: l = 4, 12 + 6 samples, the 17 x 23 view of 391 rays."""
    return S.make_case()


def case_occluder(n=S.N):
    """The oracle case's occluder: a = {1, 0.5, 0} for ray mod 3 = {0, 1, 2}, rgb = (0.25, 0.5, 0.75), z = fp32(3.5 + 0.5 (ray mod
    23) / 22) -- a plane tilted across the view's columns, inside the fine depths' span (0.87 .. 8.25)."""
    ray = np.arange(n)
    a = np.array([1.0, 0.5, 0.0])[ray % 3]
    z = 3.5 + 0.5 * (ray % 23) / 22
    return np.stack([np.full(n, 0.25), np.full(n, 0.5), np.full(n, 0.75), a, z], 1).astype(F)


def near_z(info, occ, eps=EPS):
    """(N,) bool: a fine depth of the ray lies within ``eps`` of the row's z."""
    z = torch.as_tensor(np.asarray(occ, F))[:, 4].double().view(-1, 1, 1)
    return ((info["t_fine"].double() - z).abs() <= eps).flatten(1).any(1)


def oracle_conditions(info32, info64, occ):
    """The conditions of the comparison, on the oracle alone -> (keep (N,) bool, figures): the rays left out are those with a fine
    depth within EPS of z in either oracle, at most 5 % of them; every layer keeps at least 8 present rays with in-front and behind
    samples of merged weight above 1e-6; the two oracles classify every sample of a kept ray alike."""
    left_out = near_z(info32, occ) | near_z(info64, occ)
    keep = ~left_out
    n = keep.numel()
    assert int(left_out.sum()) <= MAX_LEFT_OUT * n, f"{int(left_out.sum())} of {n} rays have a fine depth within {EPS} of z"
    assert torch.equal(info32["present"], info64["present"])
    assert torch.equal(info32["behind"][keep], info64["behind"][keep]), "the fp32 and the fp64 oracle classify a kept ray's samples differently"
    heavy = info32["merged_weights"] > SPLIT_WEIGHT
    split = (heavy & info32["behind"]).any(2) & (heavy & ~info32["behind"]).any(2) & (keep & info32["present"]).view(-1, 1)
    counts = [int(c) for c in split.sum(0)]
    assert min(counts) >= MIN_SPLIT_RAYS, f"compared present rays with samples on both sides of z, per layer: {counts}"
    return keep, dict(left_out=int(left_out.sum()), split=counts)


def flat_occluded(occluded):
    """``model.render_rays_occluded``'s third result -> the flat dict's three kinds of entries, on the CPU."""
    cat = lambda trip: torch.cat([x.detach().cpu() for x in trip], -1)
    d = {"fine_occluded_mixed": cat(occluded["mixed"]), "fine_occluder_share": cat(occluded["share"])}
    for i, trip in enumerate(occluded["scene"]):
        d[f"fine_occluded_scene{i}"] = cat(trip)
    return d


def assert_occluded_matches_oracle(got, ref32, ref64, keep, what=""):
    """``scene_edits_common.assert_matches_oracle`` as it is on the occluded outputs of the kept rays."""
    rows = lambda d, dt: {k: v[keep].to(dt) for k, v in d.items()}
    return S.assert_matches_oracle(rows(got, torch.float32), rows(ref32, torch.float32), rows(ref64, torch.float64), False, what)
