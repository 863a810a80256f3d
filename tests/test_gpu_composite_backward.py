"""The compositor's backward (csrc/render_bwd.hip: stnerf_composite_bwd, ops.composite_bwd, CompositeFunction) held to fp64 autograd
at its edges: saturated and exactly opaque samples, every launch shape the host code can choose, the merged order of descending /
unsorted / tied layers, every parameter of the stage, the three "skip this stream" shortcuts, overruns and the autograd node.
Needs a GPU: `pytest -m gpu`.

The reference is tests/composite_backward_common.py (fp64 autograd through the oracle's arithmetic; tests/test_composite_backward_cpu.py
checks it and the inputs on a CPU).  The bar, unless a test says otherwise, is GRAD_RTOL = 2e-5 of the largest entry of the colour
part and of the sigma part, with exact zeros where the reference's zero tensors and overwritten densities cannot receive a gradient.
`order` is built on the host (a stable sort: what ops.composite(want_order=True) returns bit for bit, test_composite_merge_vs_oracle),
so these tests do not depend on which shapes the forward admits.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composite_backward_common as B                                               # noqa: E402
from test_gpu_canaries import PATTERN, Canaries                                      # noqa: E402

pytestmark = pytest.mark.gpu

# HIP's per-segment error behind opaque samples <= K_SEGMENT x the fp32 reference's on the same inputs + 1e-7: twice the worst
# ratio measured on the MI355X over the committed seeds, 2.24 (profiles/composite_backward_bars.md); the ceiling is the 12 of
# tests/test_gpu_backward.py.
K_SEGMENT = 4.5


@pytest.fixture(scope="module")
def ops():
    from stnerf_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def _dev(x):
    return None if x is None else x.cuda()


def _bwd(ops, t, raw, mask, kw, g_layer, g_mixed):
    """ops.composite_bwd on host tensors, with the host-built order when the merged stream has a gradient -> (n,l,S,4) on the GPU."""
    order = B.host_order(t).cuda() if g_mixed is not None else None
    return ops.composite_bwd(_dev(t), _dev(raw), _dev(mask), order, ops.composite_params(**kw), _dev(g_layer), _dev(g_mixed))


def _bits(x):
    return x.contiguous().view(torch.int32)


def _hold(what, got, want, mask, kw):
    """Bar (a): finite, each part within GRAD_RTOL of its largest reference entry, dead entries exactly zero."""
    got = got.cpu()
    assert bool(torch.isfinite(got).all()), what
    ec, es = B.part_errors(got, want)
    print(f"{what}: colour {ec:.2e}, sigma {es:.2e} of the largest entry")
    assert ec <= B.GRAD_RTOL and es <= B.GRAD_RTOL, (what, ec, es)
    dead = B.dead_entries(mask, kw["evaluated"], got.shape[0])
    if dead.any():
        assert float(got[dead].abs().max()) == 0.0, what
        assert float(want[dead].abs().max()) == 0.0, what
    return ec, es


def _three_ways(ops, what, t, raw, mask, kw, g_layer, g_mixed):
    for gl, gm in ((g_layer, g_mixed), (g_layer, None), (None, g_mixed)):
        want = B.reference_grad(t, raw, mask, kw, gl, gm)
        _hold(f"{what} layer={gl is not None} mixed={gm is not None}", _bwd(ops, t, raw, mask, kw, gl, gm), want, mask, kw)


# ------------------------------------------------------------------------------------------------------------- a. saturation
@pytest.mark.parametrize("fine", [False, True])
@pytest.mark.parametrize("regime", ["dense", "opaque"])
def test_saturated_streams_match_fp64_autograd(ops, regime, fine):
    """l = 3, S = 80, n = 97.  dense: sigma' * delta up to about 10; opaque: up to three samples per ray with sigma' * delta >= 120,
    where exp is 0 in fp32 and om = 1e-10 in both arithmetics -- `behind / om` where 1 - alpha has no bits left."""
    build = B.dense_inputs if regime == "dense" else B.opaque_inputs
    t, raw, mask, kw, g_layer, g_mixed = build(97, 3, 80, fine)[:6]
    _three_ways(ops, f"{regime} fine={fine}", t, raw, mask, kw, g_layer, g_mixed)


# ------------------------------------------------------------------------------------------------ b. behind an opaque sample
@pytest.mark.parametrize("fine", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_gradients_behind_opaque_samples_follow_fp64_segment_by_segment(ops, seed, fine):
    """Behind an opaque sample the gradients are 1e-10 of the tensor's largest (1e-30 behind the third): bar (a) cannot see them.
    Per ray and per segment -- the run of samples of a stream with the same count of opaque samples in front -- normalised by the
    segment's largest fp64 entry; the opaque samples are left out of the sigma part (fp64 gives them ~1e-50, fp32 exactly 0) and
    segments whose remaining fp64 maximum is 0 are skipped.  HIP's segment error <= K_SEGMENT x the fp32 reference's + 1e-7.
    The layers' own streams and the merged stream are asked separately: a sample's segment is a property of the stream."""
    t, raw, mask, kw, g_layer, g_mixed, (front_layer, front_merged, opaque) = B.opaque_inputs(97, 3, 80, fine, seed)
    for what, gl, gm, measure, front in (("layer streams", g_layer, None, B.segment_errors, front_layer),
                                         ("merged stream", None, g_mixed, B.merged_segment_errors, front_merged)):
        r64 = B.reference_grad(t, raw, mask, kw, gl, gm)
        r32 = B.reference_grad(t, raw, mask, kw, gl, gm, dtype=torch.float32)
        got = _bwd(ops, t, raw, mask, kw, gl, gm).cpu()
        assert bool(torch.isfinite(got).all())
        (hc, hs), (rc, rs) = measure(got, r64, front, opaque), measure(r32, r64, front, opaque)
        print(f"SEGMENT seed={seed} fine={fine} {what}: HIP colour {hc:.3e} sigma {hs:.3e} | fp32 reference colour {rc:.3e} sigma {rs:.3e}"
              f" | ratio colour {hc / rc:.2f} sigma {hs / rs:.2f}")
        assert hc <= K_SEGMENT * rc + 1e-7 and hs <= K_SEGMENT * rs + 1e-7, (what, hc, rc, hs, rs)


# ----------------------------------------------------------------------------------------------------------- c. launch shapes
LAUNCH_SHAPES = [
    # (l, S, n): what it reaches
    (1, 1, 33), (1, 64, 33), (1, 65, 33), (2, 129, 33), (16, 4, 33),      # block edges: one sample, a full block, the carry, 16 layers
    (5, 100, 33),                                                         # three waves per workgroup (454 < l S <= 605)
    (16, 128, 9), (16, 192, 9),                                           # dynamic LDS above 64 KB (l S >= 1817)
    (1, 4519, 3),                                                         # the largest the LDS bound admits
]


@pytest.mark.parametrize("l, S, n", LAUNCH_SHAPES)
def test_every_launch_shape_matches_fp64_autograd(ops, l, S, n):
    t, raw, mask, kw, g_layer, g_mixed = B.soft_inputs(n, l, S, fine=(l + S) % 2 == 1)
    _three_ways(ops, f"({l},{S}) n={n}", t, raw, mask, kw, g_layer, g_mixed)


@pytest.mark.parametrize("l, S, n", [(1, 3, 32805),      # four waves per workgroup: 16384 rays per pass, a second and a third pass
                                     (1, 910, 4101)])    # one wave per workgroup: 4096 rays per pass, a second pass
def test_grid_stride_passes_reuse_a_waves_lds(ops, l, S, n):
    """Rays with the layer live and rays that miss it (mask 0, depths -1000) in a fair-coin succession: a wave's second ray runs
    over the dacc / T / gww its first ray filled.  The missed rays' entries must be exact zeros."""
    t, raw, mask, kw, g_layer, g_mixed = B.alternating_inputs(n, l, S, fine=True)
    dead = B.dead_entries(mask, kw["evaluated"])
    assert bool(dead[:4096].any()) and bool(dead[-5:].any()) and not bool(dead[-5:].all())
    want = B.reference_grad(t, raw, mask, kw, g_layer, g_mixed)
    _hold(f"({l},{S}) n={n}", _bwd(ops, t, raw, mask, kw, g_layer, g_mixed), want, mask, kw)


def test_an_empty_batch_is_an_empty_tensor_and_no_launch(ops):
    t, raw, mask, kw, g_layer, g_mixed = B.soft_inputs(0, 3, 20, True)
    got = _bwd(ops, t, raw, mask, kw, g_layer, g_mixed)
    torch.cuda.synchronize()
    assert got.shape == (0, 3, 20, 4) and got.dtype == torch.float32 and got.is_cuda


# --------------------------------------------------------------------------------------------------------------- d. refusals
@pytest.mark.parametrize("l, S, with_order, match", [(1, 4520, True, "LDS"), (16, 283, True, "LDS"), (2, 20, False, "order")])
def test_refusals_are_host_checks_in_front_of_the_launch(ops, l, S, with_order, match):
    """More samples per ray than a wave's LDS holds, and a merged gradient without the forward's order: ValueError naming the
    need, and the d_raw the call allocated (a canary-filled, guarded buffer) is untouched.  Every argument is a valid tensor of its
    stated size: nothing here could reach a launch with memory it should not touch."""
    n = 3
    t, raw, mask, kw, g_layer, g_mixed = B.soft_inputs(n, l, S, True)
    args = [_dev(t), _dev(raw), _dev(mask), B.host_order(t).cuda() if with_order else None, ops.composite_params(**kw), _dev(g_layer), _dev(g_mixed)]
    with Canaries() as c:
        with pytest.raises(ValueError, match=match):
            ops.composite_bwd(*args)
        torch.cuda.synchronize()
        assert len(c.buffers) == 1 and c.buffers[0][1] == n * l * S * 16
        assert bool((c.buffers[0][0].view(torch.int32) == PATTERN).all())


# ----------------------------------------------------------------------------------------------------------- e. merged order
def test_merged_order_of_descending_unsorted_and_tied_layers(ops):
    """l = 3, S = 17, n = 60: reversed background, reversed performer, a shuffled layer, a tie inside a descending list, two layers
    with identical depth lists, grazing rays and missed layers.  The loss is the merged composite only (a descending layer's own
    composite is inf / NaN in the reference as well); fp64 autograd runs through the gathered stream."""
    t, raw, mask, kw, g_layer, g_mixed = B.order_inputs()
    assert g_layer is None
    want = B.reference_grad(t, raw, mask, kw, None, g_mixed)
    _hold("merged order", _bwd(ops, t, raw, mask, kw, None, g_mixed), want, mask, kw)


# -------------------------------------------------------------------------------------------------------------- f. parameters
PARAMETERS = {
    "rgb_activated": dict(fine=True, rgb_activated=True),
    "rgb_activated_coarse": dict(fine=False, rgb_activated=True),
    "sigma_scale": dict(fine=True, sigma_scale=[1.0, 0.0, 2.5, 0.6], evaluated=[2, 1, 1, 1]),
    "coarse_background_threshold": dict(fine=False, thresholds=[0.2, 0.1, 0.1, 0.1]),
    "coarse_keeps_negative_t": dict(fine=False, cut_negative_t=False),
    "no_mask": dict(fine=True),
    "no_mask_coarse": dict(fine=False),
    "background_by_mask": dict(fine=True, evaluated=[1, 1, 0, 1]),
}


@pytest.mark.parametrize("name", list(PARAMETERS))
def test_every_parameter_matches_the_extended_reference(ops, name):
    """l = 4, S = 33, n = 61."""
    t, raw, mask, kw, g_layer, g_mixed = B.soft_inputs(61, 4, 33, seed=3, **PARAMETERS[name])
    if name.startswith("no_mask"):
        mask = None
    if name == "background_by_mask":
        mask[::3, 0] = 0                                               # background mask bits clear on some rays
    for gl, gm in ((g_layer, g_mixed), (g_layer, None), (None, g_mixed)):
        want = B.reference_grad(t, raw, mask, kw, gl, gm)
        got = _bwd(ops, t, raw, mask, kw, gl, gm)
        _hold(f"{name} layer={gl is not None} mixed={gm is not None}", got, want, mask, kw)
        if name == "sigma_scale":                                      # the scale-0 layer: no density gradient at all
            assert float(got[:, 1, :, 3].abs().max()) == 0.0 and float(want[:, 1, :, 3].abs().max()) == 0.0
            assert float(got[:, 1, :, :3].abs().max()) == 0.0        # ... and, with sigma' = 0, no weight for its colours


# --------------------------------------------------------------------------------------------------------------- g. shortcuts
def test_zero_gradient_rows_among_live_ones(ops):
    """A third of the (ray, stream) rows of g_layer and of the rows of g_mixed hold five zeros: the kernel skips those streams.
    Within bar (a) of the reference; and skipping is neutral bit for bit: a ray whose merged row is zero gets what the call without
    g_mixed gives it, a ray whose layer rows are all zero what the call without g_layer gives it, a ray with every row zero exact
    zeros, and rows of -0.0 the same bits as rows of 0.0."""
    n, l, S = 150, 3, 40
    t, raw, mask, kw, g_layer, g_mixed = B.soft_inputs(n, l, S, True, seed=4)
    g = torch.Generator().manual_seed(11)
    zl, zm = torch.rand(n, l, generator=g) < 1 / 3, torch.rand(n, generator=g) < 1 / 3
    zl[:6], zm[:3] = True, True                                        # (rays 0-2: nothing live; 3-5: the merged stream only)
    zm[3:6] = False
    g_layer, g_mixed = g_layer.clone(), g_mixed.clone()
    g_layer[zl], g_mixed[zm] = 0.0, 0.0
    got = _bwd(ops, t, raw, mask, kw, g_layer, g_mixed)
    _hold("zero rows", got, B.reference_grad(t, raw, mask, kw, g_layer, g_mixed), mask, kw)
    only_layer, only_mixed = _bwd(ops, t, raw, mask, kw, g_layer, None), _bwd(ops, t, raw, mask, kw, None, g_mixed)
    all_zl = zl.all(-1)
    assert int(zm.sum()) > 20 and int(all_zl.sum()) >= 6
    assert torch.equal(_bits(got.cpu()[zm]), _bits(only_layer.cpu()[zm]))
    assert torch.equal(_bits(got.cpu()[all_zl]), _bits(only_mixed.cpu()[all_zl]))
    assert float(got[:3].abs().max()) == 0.0
    neg = _bwd(ops, t, raw, mask, kw, torch.where(zl.unsqueeze(-1), -torch.zeros_like(g_layer), g_layer),
               torch.where(zm.unsqueeze(-1), -torch.zeros_like(g_mixed), g_mixed))
    assert torch.equal(_bits(got), _bits(neg))


@pytest.mark.parametrize("fine", [False, True])
def test_unread_inputs_may_hold_anything_and_two_calls_agree(ops, fine):
    """raw is NaN wherever the ray does not read it (mask 0 on an evaluated = 1 layer, every ray of an evaluated = 0 layer): d_raw
    has the bits of the unpoisoned call and is finite.  Two calls give equal bits."""
    t, raw, mask, kw, g_layer, g_mixed = B.soft_inputs(61, 4, 33, fine, seed=5)
    dead = B.dead_entries(mask, kw["evaluated"])
    assert bool(dead[:, 1].any()) and bool(dead[:, 3].all()) and not bool(dead[:, 0].any())
    poisoned = raw.clone()
    poisoned[dead] = float("nan")
    clean = _bwd(ops, t, raw, mask, kw, g_layer, g_mixed)
    again = _bwd(ops, t, raw, mask, kw, g_layer, g_mixed)
    got = _bwd(ops, t, poisoned, mask, kw, g_layer, g_mixed)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(_bits(clean), _bits(again)) and torch.equal(_bits(clean), _bits(got))
    _hold("clean", clean, B.reference_grad(t, raw, mask, kw, g_layer, g_mixed), mask, kw)


# ---------------------------------------------------------------------------------------------------------------- h. overruns
@pytest.mark.parametrize("l, S, n", [(1, 65, 33), (2, 129, 33), (5, 100, 33)])
def test_ragged_shapes_write_nothing_outside_their_buffers(ops, l, S, n):
    """Every tensor of the call -- inputs, order, gradients and the d_raw the wrapper allocates -- sits between canary guards."""
    t, raw, mask, kw, g_layer, g_mixed = B.soft_inputs(n, l, S, fine=True)
    with Canaries() as c:
        guarded = [torch.empty(x.shape, dtype=x.dtype, device="cuda").copy_(x) for x in (t, raw, mask, B.host_order(t), g_layer, g_mixed)]
        td, rd, md, od, gld, gmd = guarded
        got = ops.composite_bwd(td, rd, md, od, ops.composite_params(**kw), gld, gmd)
        assert c.check(f"composite_bwd ({l},{S})") == 7
    _hold(f"guarded ({l},{S})", got, B.reference_grad(t, raw, mask, kw, g_layer, g_mixed), mask, kw)


# ------------------------------------------------------------------------------------------------------- i. the autograd node
@pytest.mark.parametrize("loss_on", ["both", "mixed", "layer_acc"])
def test_the_autograd_node_hands_the_kernel_what_a_call_by_hand_does(ops, loss_on):
    """CompositeFunction with a non-contiguous raw (a slice of a wider tensor) and losses that use one output only: raw.grad is
    ops.composite_bwd called by hand, bit for bit (an unused output's zero gradient and no gradient at all are the same call),
    and within bar (a) of fp64."""
    from stnerf_amd.modeling.training import CompositeFunction
    n, l, S = 45, 3, 40
    t, raw, mask, kw, g_layer, g_mixed = B.soft_inputs(n, l, S, True, seed=6)
    wide = torch.zeros(n, l, S, 6)
    wide[..., 1:5] = raw
    wide = wide.cuda().requires_grad_(True)
    view = wide[..., 1:5]
    assert not view.is_contiguous()
    p = ops.composite_params(**kw)
    layer_out, mixed_out, w = CompositeFunction.apply(_dev(t), view, _dev(mask), p)
    acc = torch.zeros(n, l, 5)
    acc[..., 4] = g_layer[..., 4]
    gl, gm = {"both": (g_layer, g_mixed), "mixed": (None, g_mixed), "layer_acc": (acc, None)}[loss_on]
    loss = 0
    if gm is not None:
        loss = loss + (mixed_out * gm.cuda()).sum()
    if loss_on == "both":
        loss = loss + (layer_out * gl.cuda()).sum()
    if loss_on == "layer_acc":
        loss = loss + (layer_out[..., 4] * g_layer[..., 4].cuda()).sum()
    loss.backward()
    grad = wide.grad
    assert float(grad[..., 0].abs().max()) == 0.0 and float(grad[..., 5].abs().max()) == 0.0
    by_hand = _bwd(ops, t, raw, mask, kw, gl, gm)
    assert torch.equal(_bits(grad[..., 1:5]), _bits(by_hand))
    _hold(f"node {loss_on}", grad[..., 1:5], B.reference_grad(t, raw, mask, kw, gl, gm), mask, kw)
