"""The eleven named render entries of include/stnerf.h are the fixed-argument forms of stnerf_render_rays_opts, and
``ops.render_rays`` calls only the latter: here each named entry is called directly through ctypes, on the device, and held to
``ops.render_rays`` bit for bit -- (a) with every optional argument NULL / 0 against the call without keywords, the launches
included, (b) with exactly the argument the entry introduced live against the call with that keyword.

The case is ``occupancy_common.plain_case()`` on the model and rays of ``scene_edits_common`` (l = 4, 12 + 6 samples, draws
replayed), ONE launch piece: the first CAP = 128 rays.  What the model hands ``ops.render_rays`` for that piece (boxes, network
pointers, params, draws) is recorded once per precision and reused by every call.  Needs an MI355X: `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

import occluder_common as OCL
import occupancy_common as OCC
import scene_edits_common as S
import test_gpu_scene_edits_oracle as SE
from stnerf_amd import hip, ops
from test_gpu_termination import TAU

pytestmark = pytest.mark.gpu

# (entry, how many of stnerf_render_options' fields -- after struct_size, in order -- it takes)
ENTRIES = [("stnerf_render_rays", 0), ("stnerf_render_rays_cached", 1), ("stnerf_render_rays_rot", 2), ("stnerf_render_rays_scene", 3),
           ("stnerf_render_rays_opacity", 4), ("stnerf_render_rays_occupancy", 6), ("stnerf_render_rays_samples", 8),
           ("stnerf_render_rays_terminated", 11), ("stnerf_render_rays_background", 13), ("stnerf_render_rays_layers", 15),
           ("stnerf_render_rays_occluded", 20)]
FIELDS = [name for name, _ in hip.RenderOptions._fields_[1:]]
NOTHING = {**dict.fromkeys(FIELDS), "tau": 0.0, "occluder_stops": 0}


def bits(x):
    return x.contiguous().view(torch.uint8 if x.dtype == torch.uint8 else torch.int32)


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(bits(g), bits(w)), f"{what}: tensor {j} differs"


_PIECES = {}


def piece(precision):
    """The arguments of the one launch piece, as the model makes them: recorded from a render of the first CAP rays."""
    if precision not in _PIECES:
        case = OCC.plain_case()
        model = SE.make_model(case, precision)
        rays = S.case_rays(case)[:S.CAP].contiguous().cuda()
        seen, real = [], ops.render_rays

        def recording(rays, boxes, nets, params, workspace, **kw):
            seen.append(dict(rays=rays, boxes=boxes, nets=nets, params=params, jitter=kw.get("jitter"), u=kw.get("u"), kw=sorted(kw)))
            return real(rays, boxes, nets, params, workspace, **kw)
        ops.render_rays = recording
        try:
            with torch.no_grad():
                model.render_rays_raw(rays, False, case["thr"], case["bthr"], ref_chunk=case["chunk"])
        finally:
            ops.render_rays = real
        assert len(seen) == 1 and seen[0]["kw"] == ["cache", "jitter", "rotations", "u"] and seen[0]["rays"].shape[0] == S.CAP
        # (the recorded pointers name the modules' packed blobs: held here, so that they outlive a repack of the shared base model)
        blobs = [m._packed(model.bkgd_spacenet.precision) for m in model.modules() if hasattr(m, "_packed")]
        _PIECES[precision] = dict(seen[0], blobs=blobs, case=case, l=model.total_layers, n1=case["n1"], n2=case["n2"], bkgd_bbox=model.bkgd_bbox.cpu())
    return _PIECES[precision]


def through_ops(pc, profile=False, workspace_kw=None, **kw):
    n, l = S.CAP, pc["l"]
    ws = torch.empty(ops.render_workspace_bytes(n, l, pc["n1"], pc["n2"], False, **(workspace_kw or {})), dtype=torch.uint8, device="cuda")
    if profile:
        ops.profile_begin()
    out = ops.render_rays(pc["rays"], pc["boxes"], pc["nets"], pc["params"], ws, jitter=pc["jitter"], u=pc["u"], **kw)
    torch.cuda.synchronize()
    return (out, [(r["kernel"], r["kind"], r["n_rays"], r["ns"], r["tag"]) for r in ops.profile_end()]) if profile else out


def through_entry(pc, name, count, live=None, profile=False, workspace_kw=None):
    """The named entry through ctypes: the 15 shared arguments, the first ``count`` options (``live``, else NULL / 0), the stream."""
    n, l = S.CAP, pc["l"]
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device="cuda")
    mix_f, mix_c, lo_f, lo_c = new(n, 5), new(n, 5), new(n, l, 5), new(n, l, 5)
    mask = torch.empty(n, l, dtype=torch.uint8, device="cuda")
    ws = torch.empty(ops.render_workspace_bytes(n, l, pc["n1"], pc["n2"], False, **(workspace_kw or {})), dtype=torch.uint8, device="cuda")
    assert not set(live or {}) - set(FIELDS[:count]), (name, live)
    tail = [{**NOTHING, **(live or {})}[f] for f in FIELDS[:count]]
    if profile:
        ops.profile_begin()
    rc = getattr(hip.lib(), name)(hip.dptr(pc["rays"]), n, hip.dptr(pc["boxes"]), 0, C.byref(pc["nets"]), C.byref(pc["params"]),
                                  hip.dptr(pc["jitter"]), hip.dptr(pc["u"]), hip.dptr(ws, torch.uint8), ws.numel(), hip.dptr(mix_f),
                                  hip.dptr(mix_c), hip.dptr(lo_f), hip.dptr(lo_c), hip.dptr(mask, torch.uint8), *tail, hip.stream_ptr())
    hip.check(rc, name)
    torch.cuda.synchronize()
    out = (mix_f, mix_c, lo_f, lo_c, mask)
    return (out, [(r["kernel"], r["kind"], r["n_rays"], r["ns"], r["tag"]) for r in ops.profile_end()]) if profile else out


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_every_entry_without_options_is_the_plain_call(precision):
    pc = piece(precision)
    assert pc["boxes"].dim() == 3                       # (shared boxes: a box ray stride of 0)
    want, launches = through_ops(pc, profile=True)
    assert launches and not torch.equal(bits(want[0]), bits(want[1]))
    for name, count in ENTRIES:
        got, recs = through_entry(pc, name, count, profile=True)
        assert_same(got, want, f"{precision} {name}")
        assert recs == launches, f"{precision} {name}: other launches"


def grid_entry(occupied, lo, hi):
    """(bits, res, lo, inv_cell), the table entry ``ops.render_rays`` takes, of an occupied [Rz][Ry][Rx] array over lo .. hi."""
    res = (occupied.shape[2], occupied.shape[1], occupied.shape[0])
    words = torch.from_numpy(OCC.np_pack(occupied).view(np.int32).copy()).cuda()
    return (words, res, [float(x) for x in lo], [float(x) for x in OCC.np_inv_cell(res, lo, hi)])


def live_arguments(pc, which):
    """-> (the ops keywords, {field: value} for the entry, workspace keywords, the tensors the call fills beyond the five, as
    ``ops.render_rays`` would append them, further tensors it writes) -- made afresh for each of the two calls."""
    n, l, n1, S_ = S.CAP, pc["l"], pc["n1"], pc["n1"] + pc["n2"]
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device="cuda")
    if "inputs" not in pc:      # the device inputs both calls read, made once and kept: the ctypes tables hold addresses only
        pc["inputs"] = (grid_entry(OCC.half_x(8), *OCC.layer_bounds(pc["case"], 1)), grid_entry(OCC.half_x(8), *OCC.np_bounds(pc["bkgd_bbox"])),
                        torch.from_numpy(OCL.case_occluder(n)).cuda())
    layer_grid, grid, occluder = pc["inputs"]
    table = [None, layer_grid, None, None]
    if which == "cached":
        raw_c, raw_f = new(n, n1, 4), new(n, S_, 4)
        cache = hip.BkgdCache(raw_c.data_ptr(), raw_f.data_ptr(), hip.BKGD_CACHE_CAPTURE)
        return dict(cache=(raw_c, raw_f, hip.BKGD_CACHE_CAPTURE)), dict(cache=C.pointer(cache)), {}, (), (raw_c, raw_f)
    if which == "rot":
        rotations = [None, (S.ray_matrix(S.ANGLE), torch.tensor([0.1, -0.2, 0.3])), None, None]
        return dict(rotations=rotations), dict(rot=ops._rotations(rotations, l)), {}, (), ()
    if which == "scene":
        scene = new(n, l, 5)
        return dict(scene=True), dict(scene_out=hip.dptr(scene)), {}, (scene,), ()
    if which == "opacity":
        return dict(layer_alpha=list(S.LAYER_ALPHA)), dict(layer_alpha=(C.c_float * l)(*S.LAYER_ALPHA)), {}, (), ()
    if which == "occupancy":
        return dict(occupancy=table), dict(occ=ops._occupancy_table(table, l)), {}, (), ()
    if which == "samples":
        flags = [False, True, False, False]
        return (dict(occupancy=table, occupancy_samples=flags), dict(occ=ops._occupancy_table(table, l), samples=(C.c_int32 * l)(0, 1, 0, 0)),
                dict(occupancy_samples=flags), (), ())
    if which == "terminated":
        return (dict(terminate=[True] * l, tau=TAU), dict(tau=TAU, terminate=(C.c_int32 * l)(*[1] * l)), dict(terminate=[True] * l), (), ())
    if which == "background":
        return dict(background_grid=grid), dict(bkgd_grid=ops._occupancy_table([grid], 1)), dict(background=True), (), ()
    if which == "layers":
        raw_c, raw_f = new(n, n1, 4).zero_(), new(n, S_, 4).zero_()
        rays, count = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        caches = [None, (raw_c, raw_f, rays, count, hip.LAYER_CACHE_CAPTURE), None, None]
        return (dict(layer_caches=caches), dict(layers=ops._layer_cache_table(caches, l, n1, pc["n2"], False)), {}, (),
                (raw_c, raw_f, rays, count))
    assert which == "occluded"
    scene, mixed, shares, share = new(n, l, 5), new(n, 5), new(n, l, 5), new(n, 5)
    return (dict(scene=True, occluder=occluder),
            dict(scene_out=hip.dptr(scene), occluder=hip.dptr(occluder), occluded_mixed=hip.dptr(mixed), occluded_scene=hip.dptr(shares),
                 occluder_share=hip.dptr(share)), {}, (scene, mixed, shares, share), ())


@pytest.mark.parametrize("name,count", ENTRIES[1:], ids=[name[len("stnerf_render_rays_"):] for name, _ in ENTRIES[1:]])
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_every_entry_with_its_own_argument_is_the_call_with_that_keyword(precision, name, count):
    pc = piece(precision)
    which = name[len("stnerf_render_rays_"):]
    plain = through_ops(pc)
    kw, _, ws_kw, _, written_ops = live_arguments(pc, which)
    want = through_ops(pc, workspace_kw=ws_kw, **kw) + tuple(written_ops)
    _, live, ws_kw, appended, written = live_arguments(pc, which)
    got = through_entry(pc, name, count, live, workspace_kw=ws_kw) + tuple(appended) + tuple(written)
    if which == "layers":
        # slots beyond the captured count are never written, and the order of a compacted ray list is free: the filled slots, by ray
        c = int(want[-1])
        assert c == int(got[-1]) and 0 < c < S.CAP
        def by_ray(out):
            order = out[7][:c].argsort()
            return out[:5] + tuple(t[:c][order] for t in out[5:8]) + out[8:]
        got, want = by_ray(got), by_ray(want)
    assert_same(got, want, f"{precision} {name}")
    # the argument is live: it shows in the outputs, or in what the call wrote beside them
    if which in ("rot", "opacity", "occupancy", "samples", "terminated", "background"):
        assert any(not torch.equal(bits(g), bits(p)) for g, p in zip(got[:5], plain)), f"{precision} {name}: the argument changed nothing"
    else:
        assert_same(got[:5], plain, f"{precision} {name}: the five standard outputs")
        assert all(bool(t.float().abs().sum() > 0) for t in got[5:]), f"{precision} {name}: an output was not written"
