"""Shared by tests/test_gpu_scene_edits_oracle.py and tests/test_oracle_scene_edits_cpu.py: the scene-edit cases (per-layer
rotation, layer instances, the per-layer opacity table, the in-scene layer passes -- DESIGN.md section 7), their evaluation by the
CPU oracle and THE comparison the GPU tests apply (``assert_matches_oracle``).  The CPU tests feed that same function oracle
outputs made from deliberately wrong inputs, so that what it would catch on the GPU is known without one.

Everything the oracle is given is derived here from the case's own spec (angles, centres, tables), never from
``LayeredRFRender``'s host arithmetic: m = R^T from the angle (built in fp64, rounded to fp32, transposed), the default centre left
to the oracle, the instance table as a tuple of sources."""
import functools
import math

import torch

from oracle import stnerf_oracle as O
from stnerf_amd import synthetic as syn

from instances_common import CASES, CENTRE, base_model, frame_ids, instance_edits, wide_state_dict
from test_gpu_render import COLOR_ATOL, DEPTH_ATOL, fine_stage_bar

H, W, CAP, CHUNK = 17, 23, 128, 64          # 391 rays: no multiple of 64; launch pieces of 128 (the last of 7 rays); reference chunks
N = H * W
ORBIT = 15.0
THR, BTHR = 0.05, 0.02
ANGLE = 0.4                                 # layer 1's rotation, about the DEFAULT centre
LAYER_ALPHA = (0.8, 0.6, 0.5, 0.35)
TRIPLE = (("colour", slice(0, 3)), ("depth", slice(3, 4)), ("acc", slice(4, 5)))


def ray_matrix(angle):
    """m = R^T of a rotation by ``angle`` about +z: the matrix built in fp64, rounded to fp32, transposed."""
    c, s = math.cos(angle), math.sin(angle)
    R = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64).to(torch.float32)
    return R.T.contiguous()


def oracle_rotation(spec):
    """A case's rotation list (None | angle | (angle, centre) per layer, what ``model.rotation`` takes) -> the oracle's."""
    if spec is None:
        return None
    out = []
    for e in spec:
        if e is None:
            out.append(None)
        elif isinstance(e, (tuple, list)):
            out.append((ray_matrix(e[0]), e[1]))
        else:
            out.append((ray_matrix(e), None))
    return out


def make_case(**over):
    """The base scene: case A of instances_common (L = 2, one instance of performer 1, seed 4), its edits plus layer 1 turned by
    0.4 about the default centre, the opacity table, thresholds 0.05 / 0.02, one frame id per layer, (12, 6) samples.
    ``groups``: [(first ray, row of frame ids)]: the frame-id columns change at those rays (multiples of the reference chunk);
    ``frame``: a single id instead -- rays 7 wide."""
    L, sources = CASES["A"]
    l = 1 + L + len(sources)
    scale, shift, rotation = instance_edits(l, L + 1)
    rotation[1] = ANGLE
    c = dict(L=L, sources=sources, n1=12, n2=6, only_coarse=False, groups=[(0, frame_ids(L, len(sources)))], frame=None,
             scale=scale, shift=shift, rotation=rotation, layer_alpha=list(LAYER_ALPHA), alpha=1.0, near=0.0, hidden=(),
             thr=THR, bthr=BTHR, chunk=CHUNK, orbit=ORBIT, draw_seed=23)
    assert set(over) <= set(c), set(over) - set(c)
    c.update(over)
    return c


def total_layers(case):
    return 1 + case["L"] + len(case["sources"])


def camera():
    return syn.camera(H, W, ORBIT)


def with_frame_ids(rays6, case):
    """(N,6) rays -> the case's ray tensor: one frame-id column per layer (changing at the case's groups), or one column."""
    n = rays6.shape[0]
    if case["frame"] is not None:
        return torch.cat([rays6, torch.full((n, 1), float(case["frame"]))], 1)
    cols = torch.zeros(n, total_layers(case))
    for first, ids in case["groups"]:
        assert first % case["chunk"] == 0 and len(ids) == total_layers(case)
        cols[first:] = torch.tensor(ids, dtype=torch.float32)
    return torch.cat([rays6, cols], 1)


def case_rays(case):
    """The view's rays on the CPU (the oracle's own generator), with the case's frame-id columns."""
    K, T = syn.camera(H, W, case["orbit"])
    return with_frame_ids(O.generate_rays(K, T, H, W), case)


def case_draws(case):
    """jitter (l,N,n1), u (l,N,n2): the uniform draws, replayed by the model (``model.replay``) and by the oracle's ``rand``."""
    g = torch.Generator().manual_seed(case["draw_seed"])
    l = total_layers(case)
    return torch.rand(l, N, case["n1"], generator=g), torch.rand(l, N, case["n2"], generator=g)


@functools.lru_cache(maxsize=None)
def _state(L):
    model = base_model(L)
    return {k: v.detach().clone() for k, v in model.state_dict().items()}, model.bkgd_bbox.clone(), model.bboxes.clone()


def wide_of(case):
    """The case on its WIDE model -> (case with L + K performers and no instance, (state dict, background
    box, box table)): the sources' modules copied under the instances' indices (``instances_common.wide_state_dict``), their box
    columns appended."""
    model = base_model(case["L"])
    for src in case["sources"]:
        model.add_instance(src)
    _, bk, per = _state(case["L"])
    table = torch.cat([per] + [per[:, s - 1:s].clone() for s in case["sources"]], 1)
    return dict(case, L=case["L"] + len(case["sources"]), sources=()), (wide_state_dict(model), bk, table)


def oracle_model(case, dtype=torch.float32, state=None, **over):
    """The case as an OracleModel in ``dtype``.  ``state``: (state dict, background box, box table) instead of the synthetic
    model's of the case's L (``wide_of``)."""
    sd, bk, per = _state(case["L"]) if state is None else state
    m = O.OracleModel(layer_num=case["L"], n_coarse=case["n1"], n_fine=case["n2"], params={k: v.to(dtype) for k, v in sd.items()},
                      use_deform_time=True, use_space_time=True, bkgd_bbox=bk.to(dtype), bboxes=per.to(dtype),
                      near=case["near"], alpha=case["alpha"], scale=case["scale"], shift=case["shift"], hidden=set(case["hidden"]),
                      sources=tuple(case["sources"]), rotation=oracle_rotation(case["rotation"]), layer_alpha=case["layer_alpha"])
    for k, v in over.items():
        assert hasattr(m, k), k
        setattr(m, k, v)
    return m


def flat(out, t_coarse=None):
    """(5-tuple of triples, scene) or the oracle's 6-tuple -> {name: (n,5) [colour, depth, acc] | (n,) bool mask | t_coarse (n,l,n1)}."""
    five, scene = (out[:5], out[5]) if len(out) == 6 else out
    fm, cm, fl, cl, masks = five
    cat = lambda trip: torch.cat([x.detach().cpu() for x in trip], -1)
    d = {"fine_mixed": cat(fm), "coarse_mixed": cat(cm)}
    for i in range(len(masks)):
        d[f"fine_layer{i}"], d[f"coarse_layer{i}"], d[f"scene{i}"] = cat(fl[i]), cat(cl[i]), cat(scene[i])
        d[f"mask{i}"] = masks[i].detach().cpu().bool()
    if t_coarse is not None:
        d["t_coarse"] = t_coarse.detach().cpu()
    return d


def oracle_render(case, rays=None, dtype=torch.float32, model=None, chunked=True):
    """The oracle on the case, reference chunk by reference chunk (each takes its boxes, and so its default centres, from its own
    row 0), with the case's draws, scene passes included -> ``flat`` with t_coarse.  ``chunked=False``: one chunk with the
    model's default thresholds -- what a view smaller than ``layered_batchify_ray``'s chunk gets (``render_pose``)."""
    rays = case_rays(case) if rays is None else rays
    m = oracle_model(case, dtype) if model is None else model
    jitter, u = case_draws(case)
    l, step = total_layers(case), case["chunk"] if chunked else rays.shape[0]
    kw = dict(density_threshold=case["thr"], bkgd_density_threshold=case["bthr"]) if chunked else {}
    outs, ts = [], []
    with torch.no_grad():
        for s in range(0, rays.shape[0], step):
            e = min(s + step, rays.shape[0])
            draws = iter([jitter[i, s:e] for i in range(l)] + [u[i, s:e] for i in range(l)])
            trace = {}
            outs.append(O.render_chunk(m, rays[s:e].to(dtype), only_coarse=case["only_coarse"], rand=lambda shape: next(draws),
                                       trace=trace, scene=True, **kw))
            ts.append(torch.stack([t.squeeze(-1) for t in trace["t_coarse"]], 1))
    cat3 = lambda trips: tuple(torch.cat([t[j] for t in trips], 0) for j in range(3))
    whole = (cat3([o[0] for o in outs]), cat3([o[1] for o in outs]))
    whole += tuple([cat3([o[k][i] for o in outs]) for i in range(l)] for k in (2, 3))
    whole += ([torch.cat([o[4][i] for o in outs], 0) for i in range(l)], [cat3([o[5][i] for o in outs]) for i in range(l)])
    return flat(whole, torch.cat(ts, 0))


def assert_matches_oracle(got, ref32, ref64, only_coarse=False, what=""):
    """THE comparison of the GPU tests.  got / ref32 / ref64: ``flat`` dicts of the render under test, the fp32 oracle and the
    fp64 oracle.  Bars, all tests/test_gpu_render.py's: masks and coarse sample depths ``torch.equal`` to the fp32 oracle; coarse
    outputs -- and every output when the coarse stage is the final one -- within COLOR_ATOL / DEPTH_ATOL of it on EVERY ray; fine
    outputs and the scene passes no further from the fp64 oracle than the fp32 oracle itself is (``fine_stage_bar``).
    -> for the record, {output_quantity: the largest error against the fp32 oracle (per-ray bars) | fine_stage_bar's four figures
    + the median and the 90th percentile of the error against fp64, each of ``got`` and of the fp32 oracle}."""
    assert set(got) == set(ref32) == set(ref64), (sorted(got), sorted(ref32))
    figures = {}
    for k in sorted(ref32):
        g, r = got[k], ref32[k]
        assert g.shape == r.shape and g.dtype == r.dtype, (what, k, g.shape, r.shape, g.dtype, r.dtype)
        if k.startswith("mask") or k == "t_coarse":
            assert torch.equal(g, r), f"{what} {k}: {int((g != r).sum())} of {g.numel()} entries differ from the fp32 oracle"
            continue
        for name, cols in TRIPLE:
            tol = DEPTH_ATOL if name == "depth" else COLOR_ATOL
            if k.startswith("coarse") or only_coarse:
                err = float((g[:, cols] - r[:, cols]).abs().max())
                figures[f"{k}_{name}"] = err
                assert err <= tol, f"{what} {k} {name}: max abs err {err:.3e} > {tol} against the fp32 oracle"
            else:
                bar = fine_stage_bar(g[:, cols], r[:, cols], ref64[k][:, cols], tol, f"{what} {k} {name}")
                errs = [(x[:, cols].double() - ref64[k][:, cols]).abs().amax(-1) for x in (g, r)]
                figures[f"{k}_{name}"] = bar + tuple(float(torch.quantile(e, q)) for q in (0.5, 0.9) for e in errs)
    return figures


def rays_changed(a, b, tol=100 * COLOR_ATOL, cols=slice(0, 3)):
    """How many rays differ by more than ``tol`` (5e-3: a hundred times the colour bar) in the given columns."""
    return int(((a[:, cols] - b[:, cols]).abs().amax(-1) > tol).sum())
