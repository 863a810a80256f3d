"""What the one-call pipeline (``stnerf_render_rays_opts``, csrc/pipeline.hip) is DEFINED to compute, stated once as a chain of
op-level entries, and what the GPU tests need to hold a render to it bit for bit:
sampler -> [ray cull] -> compaction -> stage -> zeros -> composite_scene -> [ray_stop] -> resample -> stage -> zeros ->
composite_scene [-> deep list].  Every optional term is applied only when its option is in the launch.  The chain calls neither
``model._render_launch`` nor ``ops.render_rays``, and no row-list entry outside ``via_rows``: the zeros are torch writes driven by the
numpy rules of tests/occupancy_common.py and tests/sample_cull_common.py."""
import dataclasses

import numpy as np
import torch

import occupancy_common as OC
import sample_cull_common as SC
import test_gpu_bkgd_cache as BC
import test_gpu_scene_edits_oracle as SE
from stnerf_amd import ops

NAMES = ("fine_mixed", "coarse_mixed", "fine_layer", "coarse_layer", "mask", "scene")
# the arguments of a launch the chain has a term for (``occluder`` goes through ``with_chain``'s ``after``)
EXPRESSED = ("rotations", "occupancy_ids", "background_id", "background_rays", "proposal_ids", "deep")


def bits(x):
    return x.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def np_bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def cu(x, dt=torch.float32):
    return torch.as_tensor(x).to("cuda", dt).contiguous()


def detach_models():
    """The models of tests/test_gpu_scene_edits_oracle.py and tests/test_gpu_bkgd_cache.py are shared by the whole session: leave
    none with anything attached."""
    for m in list(SE._BASE.values()) + list(BC._MODELS.values()):
        m.set_proposal(None)
        m.set_termination(None)
        m.set_occupancy(None)
        m.set_background_cache(None)
        m.set_layer_cache(None)
        m.replay = None
        m.fresh_draws_per_call = False


@dataclasses.dataclass
class Chain:
    """outputs: the six tensors of a launch with the scene passes.  stop: the stop depths (None where nothing is terminated).
    t, raw, mask, merged, scene, mixed, evaluated: what the FINAL composite_scene took and returned (the coarse one under
    only_coarse).  deep: (offsets, samples) when the launch asks for the deep list.  launch: the arguments, for the caller's asserts."""
    outputs: tuple
    stop: object
    t: torch.Tensor
    raw: torch.Tensor
    mask: torch.Tensor
    merged: torch.Tensor
    scene: torch.Tensor
    mixed: torch.Tensor
    evaluated: list
    deep: object
    launch: dict


def _np_grid(g):
    return OC.np_unpack(g.bits.cpu().numpy().view(np.uint32), g.res), g.lo, g.inv_cell


def chain_render(model, launch, flags=None, tau=0.0, t_stop=None, via_rows=False):
    """launch: the arguments ``_render_launch`` received, by its names; an absent key is a feature that is off.  flags, tau: early
    ray termination's, one flag per layer, stated by the caller.  t_stop: a tensor (n,) or a number in place of ray_stop's.
    via_rows: the flagged layers' fine stage through ``ops.visibility_rows`` and the row-list stage launch instead of the unlisted
    launch and torch's zeros."""
    rays, boxes, pivot, retiming, only_coarse = (launch[k] for k in ("rays", "boxes", "pivot", "retiming", "only_coarse"))
    thr, bthr, replay = launch["thr"], launch["bthr"], launch["replay"]
    rotations, occupancy_ids, background_id, background_rays, proposal_ids, deep = (launch.get(k) for k in EXPRESSED)
    l, n1, n2 = model.total_layers, model.coarse_ray_sample, model.fine_ray_sample
    n, dev = rays.shape[0], rays.device
    prec = model.bkgd_spacenet.precision
    flags = [False] * l if flags is None else flags
    grids = model._occupancy
    table, held = grids.table(model, occupancy_ids, dev, retiming) if occupancy_ids is not None else (None, [None] * l)
    culled = {i: _np_grid(g) for i, g in enumerate(held) if g is not None} if table is not None and grids.samples else {}
    if background_id is not None:
        culled[0] = _np_grid(grids.background_grid(model, background_id, dev))
    masked = None if background_rays is None else (background_rays == 0).to(dev)
    assert not via_rows or (background_id is None and masked is None)        # (there the pipeline lists layer 0 by another entry)
    proposal = model.proposal.table(model, proposal_ids, dev, retiming)[0] if proposal_ids is not None else [None] * l
    ec, ef = model._point_edits(l, False), model._point_edits(l, True)
    first, stripe, period = (int(x) for x in launch["window"])
    rng = dict(seed=int(model.seed) & 0xFFFFFFFFFFFFFFFF, ray_index_base=first, ray_index_stripe=stripe, ray_index_period=period)
    t_c, xyz_c, mask = ops.sample_coarse(rays, boxes, n1, jitter=replay["jitter"] if replay else None, edits=ec, pivot=pivot, raw_mask=True,
                                         rotations=rotations, **rng)
    if table is not None:
        ops.occupancy_cull(xyz_c, mask, table)
    lst, cnt = ops.compact_rays(mask)
    shown = [True] + [model.is_shown_layer(i) for i in range(1, l)]
    hit = (mask & 1).bool()
    hit[:, 0] = True                                             # layer 0 acts on every ray

    def stage(xyz, ns, fine, t=None, stop=None):
        raw = torch.full((n, l, ns, 4), 7.0, device=dev)
        layers, zeroed = [], []
        for i in range(l):
            if not shown[i] or (not fine and proposal[i] is not None):
                continue
            deform = model.bkgd_use_deform_time if i == 0 else model.use_deform_time
            timed = (True if i > 0 else model.bkgd_use_space_time) and model.use_space_time
            if i == 0:
                space, motion = (model.bkgd_spacenet_fine if fine else model.bkgd_spacenet), model.bkgd_time_deform_net if deform else None
            else:
                j = model._module_index(i)
                space, motion = (model.spacenets_fine if fine else model.spacenets)[j], model.time_deform_nets[j] if deform else None
            ly = dict(space=space._packed(prec), motion=None if motion is None else motion._packed(prec), xyz=xyz[:, i], raw=raw[:, i],
                      times=rays[:, (6 + i) if retiming else 6] if (timed or deform) else None,
                      ray_list=None if i == 0 else lst[i], ray_count=None if i == 0 else cnt[i:i + 1], plain_time=i == 0,
                      rotation=None if rotations is None else rotations[i])
            if fine and via_rows and flags[i]:
                g = held[i] if i in culled else None
                ly["row_list"], ly["row_count"] = ops.visibility_rows(t[:, i], stop, raw[:, i], xyz=xyz[:, i] if g is not None else None,
                                                                      grid=None if g is None else g.entry(), layer=i, ray_list=ly["ray_list"],
                                                                      ray_count=ly["ray_count"])
            else:
                zeroed.append(i)
            layers.append(ly)
        if layers:
            ops.mlp_stage(layers, rays[:, 3:6], ns, deep_rgb=model.deep_rgb, sigmoid_rgb=True)
        pts = xyz.cpu().numpy() if culled else None              # the rules, on the chain's own points
        for i in zeroed:
            off = torch.zeros(n, ns, dtype=torch.bool, device=dev)
            if i in culled:                                      # the background's grid, the performers' sample cull
                kept = OC.np_points_occupied(pts[:, 0], *culled[0]) if i == 0 else SC.np_listed(pts[:, i], culled[i])
                off |= torch.from_numpy(~kept).to(dev)
            if i == 0 and masked is not None:                    # the per-ray mask: every sample of a masked ray
                off |= masked[:, None]
            if fine and flags[i]:                                # the hidden samples
                off |= t[:, i] > stop[:, None]
            raw[:, i][off & hit[:, i, None]] = 0.0
        if not fine:
            for i in range(l):
                if proposal[i] is not None:
                    ops.proposal_density(xyz[:, i], raw[:, i], proposal[i], layer=i, ray_list=None if i == 0 else lst[i],
                                         ray_count=None if i == 0 else cnt[i:i + 1])
        return raw

    evaluated = [2] + [int(s) for s in shown[1:]]
    kw = dict(border=float(model.boarder_weight), near=float(model.near), evaluated=evaluated, rgb_activated=True)
    raw_c = stage(xyz_c, n1, False)
    lo_c, mix_c, w_c, merged_c, scene_c = ops.composite_scene(t_c, raw_c, mask, fine=False, cut_negative_t=True, want_weights=True,
                                                              thresholds=[None] + [thr if retiming else None] * (l - 1), **kw)
    if only_coarse:
        outputs, stop, final = (mix_c, mix_c, lo_c, lo_c, mask & 1, scene_c), None, (t_c, raw_c, merged_c, scene_c, mix_c)
    else:
        stop = None
        if t_stop is not None:
            stop = torch.as_tensor(t_stop, dtype=torch.float32, device=dev).expand(n).contiguous()
        elif any(flags):
            stop = ops.ray_stop(t_c, merged_c, tau)
        t_f, xyz_f = ops.resample(t_c, w_c, n2, rays, u=replay.get("u") if replay else None, edits=ef, pivot=pivot, mask=mask,
                                  rotations=rotations, **rng)
        raw_f = stage(xyz_f, n1 + n2, True, t_f, stop)
        alpha = model._layer_alpha_table()
        if alpha is None:
            alpha = [1.0] * l
            if l > 2:
                alpha[2] = float(model.alpha)
        lo_f, mix_f, _, merged_f, scene_f = ops.composite_scene(t_f, raw_f, mask, fine=True, cut_negative_t=False, sigma_scale=alpha,
                                                                thresholds=([bthr] + [thr] * (l - 1)) if retiming else None, **kw)
        outputs, final = (mix_f, mix_c, lo_f, lo_c, mask & 1, scene_f), (t_f, raw_f, merged_f, scene_f, mix_f)
    t, raw, merged, scene, mixed = final
    dlist = None
    if deep is not None:
        dkw = dict(w_min=deep["w_min"], merge_dz=deep["merge_dz"], rgb_activated=True, evaluated=evaluated)
        offsets = ops.deep_offsets(ops.deep_count(t, mask, merged, **dkw), l * t.shape[2])
        samples = torch.empty(int(offsets[-1]), 8, device=dev)
        ops.deep_fill(t, raw, mask, merged, offsets, samples, **dkw)
        dlist = (offsets, samples)
    return Chain(outputs, stop, t, raw, mask, merged, scene, mixed, evaluated, dlist, launch)


def with_chain(model, monkeypatch, pairs, flags=None, tau=0.0, force_scene=True, after=None, **chain_kw):
    """Every launch of the model also runs the chain on the same arguments; ``pairs`` gets (pipeline outputs, the Chain).
    after(chain, launch) -> the Chain to record: what a caller adds behind the chain (the occluder), or a second chain."""
    real = model._render_launch

    def wrapped(rays, boxes, pivot, retiming, only_coarse, thr, bthr, window, replay, piece=None, scene=False, **kw):
        live = {k for k, v in kw.items() if v is not None and v is not False}
        assert live <= set(EXPRESSED) | ({"occluder", "occluder_stops"} if after is not None else set()), live
        got = real(rays, boxes, pivot, retiming, only_coarse, thr, bthr, window, replay, piece, scene=scene or force_scene, **kw)
        launch = dict(rays=rays, boxes=boxes, pivot=pivot, retiming=retiming, only_coarse=only_coarse, thr=thr, bthr=bthr, window=window,
                      replay=replay, scene=scene, **kw)
        chain = chain_render(model, launch, flags, tau, **chain_kw)
        if after is not None:
            chain = after(chain, launch)
        pairs.append((got, chain))
        return got if scene or not force_scene else got[:5]
    monkeypatch.setattr(model, "_render_launch", wrapped)


def assert_pairs_equal(pairs, what, pieces=None):
    assert pairs and (pieces is None or len(pairs) == pieces), (what, len(pairs))
    for piece, (got, chain) in enumerate(pairs):
        for name, g, w in zip(NAMES, got, chain.outputs):
            same = torch.equal(g, w) if g.dtype == torch.uint8 else same_bits(g, w)
            assert same, f"{what}: piece {piece}: {name} differs from the chain of op-level entries"
