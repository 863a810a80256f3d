"""The yardstick and the inputs of the compositor-backward tests (tests/test_gpu_composite_backward.py), checked on a CPU before a
GPU is involved:

  * the fp64 autograd gradient of the reference graph (tests/composite_backward_common.py) is the derivative of its forward
    (central finite differences);
  * on every input regime the same graph in fp32 -- the reference's own autograd arithmetic -- is finite and within GRAD_RTOL of
    fp64: the regime asks nothing of the HIP kernel that the reference's own arithmetic cannot do;
  * behind opaque samples, where the gradients are 1e-10 .. 1e-30 of the tensor's largest, the fp32 graph follows fp64 segment by
    segment: the per-segment bar of the GPU test is measured against a yardstick that holds there.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composite_backward_common as B                                               # noqa: E402

REGIMES = {"soft": B.soft_inputs, "dense": B.dense_inputs, "opaque": B.opaque_inputs}


@pytest.mark.parametrize("fine", [False, True])
@pytest.mark.parametrize("rgb_activated", [False, True])
def test_fp64_reference_gradient_is_the_derivative_of_its_forward(fine, rgb_activated):
    """n = 3, l = 2, S = 5: every entry of d raw against (f(x + h) - f(x - h)) / 2h of the fp64 forward.  The ReLU and threshold
    kinks are excluded by construction (no sigma within 2e-3 of 0 or of a threshold; h = 1e-6)."""
    t, raw, mask, kw, g_layer, g_mixed = B.soft_inputs(3, 2, 5, fine, seed=1, rgb_activated=rgb_activated)
    mask[1, 1], mask[2, 1] = 0, 1
    want = B.reference_grad(t, raw, mask, kw, g_layer, g_mixed)
    assert float(want[..., :3].abs().max()) > 1e-3 and float(want[..., 3].abs().max()) > 1e-3

    def loss(r):
        lo, mo = B.reference_forward(t, r, mask, kw)
        return float((lo * g_layer.double()).sum() + (mo * g_mixed.double()).sum())

    h = 1e-6
    fd = torch.zeros_like(want)
    x = raw.double()
    for idx in torch.cartesian_prod(*[torch.arange(s) for s in raw.shape]).tolist():
        up, dn = x.clone(), x.clone()
        up[tuple(idx)] += h
        dn[tuple(idx)] -= h
        fd[tuple(idx)] = (loss(up) - loss(dn)) / (2 * h)
    ec, es = B.part_errors(fd, want)
    print(f"finite differences vs fp64 autograd: colour {ec:.2e}, sigma {es:.2e}")
    # central differences: truncation ~ h^2 f''' and rounding ~ 1e-16 |f| / h = 1e-10 |f|
    assert ec <= 1e-7 and es <= 1e-7
    assert float(want[B.dead_entries(mask, kw["evaluated"])].abs().max()) == 0.0


@pytest.mark.parametrize("fine", [False, True])
@pytest.mark.parametrize("regime", list(REGIMES))
def test_fp32_reference_is_within_the_bar_of_fp64_on_every_regime(regime, fine):
    """The condition that the inputs are fair (l = 3, S = 80, n = 97, the shapes of the GPU test)."""
    t, raw, mask, kw, g_layer, g_mixed = REGIMES[regime](97, 3, 80, fine)[:6]
    for gl, gm in ((g_layer, g_mixed), (g_layer, None), (None, g_mixed)):
        r64 = B.reference_grad(t, raw, mask, kw, gl, gm)
        r32 = B.reference_grad(t, raw, mask, kw, gl, gm, dtype=torch.float32)
        assert bool(torch.isfinite(r32).all()) and bool(torch.isfinite(r64).all())
        ec, es = B.part_errors(r32, r64)
        print(f"{regime} fine={fine} layer={gl is not None} mixed={gm is not None}: fp32 vs fp64 colour {ec:.2e}, sigma {es:.2e}")
        assert ec <= B.GRAD_RTOL and es <= B.GRAD_RTOL


def test_regimes_are_what_they_claim():
    """dense reaches sigma' * delta of about 10; opaque has rays with one, two and three exactly opaque samples in front of live
    ones, in the layers' own streams and in the merged one."""
    t, raw, mask, kw = B.dense_inputs(97, 3, 80, True)[:4]
    s_layer, _ = B.edited_sigma(t, raw, mask, kw)
    sd = (s_layer.clamp(min=0)[..., :-1] * (t[..., 1:] - t[..., :-1]))
    assert 8.0 <= float(sd.max()) <= 20.0
    for fine in (False, True):
        t, raw, mask, kw, _, _, (front_layer, front_merged, opaque) = B.opaque_inputs(97, 3, 80, fine)
        assert int(front_layer.max()) >= 2 and int(front_merged.max()) == 3
        assert bool(opaque[..., :-1].any())


@pytest.mark.parametrize("fine", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fp32_reference_follows_fp64_behind_opaque_samples(fine, seed):
    """Per ray and per segment (the run of samples with the same count of opaque samples in front), normalised by the segment's
    largest fp64 entry; the opaque samples themselves are left out of the sigma part (fp64 gives them ~1e-50, fp32 exactly 0) and
    segments without a gradient are skipped.  The fp32 graph stays within GRAD_RTOL of fp64 on every segment: what the GPU test
    multiplies by K is a small number."""
    t, raw, mask, kw, g_layer, g_mixed, (front_layer, front_merged, opaque) = B.opaque_inputs(97, 3, 80, fine, seed)
    r64 = B.reference_grad(t, raw, mask, kw, g_layer, None)
    r32 = B.reference_grad(t, raw, mask, kw, g_layer, None, dtype=torch.float32)
    ec, es = B.segment_errors(r32, r64, front_layer, opaque)
    print(f"layer streams, fine={fine} seed={seed}: fp32 segment error colour {ec:.2e}, sigma {es:.2e}")
    assert 0 < ec <= B.GRAD_RTOL and 0 < es <= B.GRAD_RTOL
    r64 = B.reference_grad(t, raw, mask, kw, None, g_mixed)
    r32 = B.reference_grad(t, raw, mask, kw, None, g_mixed, dtype=torch.float32)
    ec, es = B.merged_segment_errors(r32, r64, front_merged, opaque)
    print(f"merged stream, fine={fine} seed={seed}: fp32 segment error colour {ec:.2e}, sigma {es:.2e}")
    assert 0 < ec <= B.GRAD_RTOL and 0 < es <= B.GRAD_RTOL
    # the segments are real: the gradients behind the third opaque sample are ~1e-30 of the largest
    behind = r64[..., 3][(front_merged == 3) & ~opaque].abs().max()
    assert 0 < float(behind) < 1e-20 * float(r64[..., 3].abs().max())


def test_other_inputs_are_fair():
    """The merged-order patterns and the alternating batches: fp32 within the bar of fp64, dead entries exactly zero."""
    t, raw, mask, kw, gl, gm = B.order_inputs()
    assert B.part_errors(B.reference_grad(t, raw, mask, kw, gl, gm, torch.float32), B.reference_grad(t, raw, mask, kw, gl, gm)) <= (B.GRAD_RTOL,) * 2
    t, raw, mask, kw, gl, gm = B.alternating_inputs(200, 1, 3, True)
    r64 = B.reference_grad(t, raw, mask, kw, gl, gm)
    assert max(B.part_errors(B.reference_grad(t, raw, mask, kw, gl, gm, torch.float32), r64)) <= B.GRAD_RTOL
    dead = B.dead_entries(mask, kw["evaluated"])
    assert 0.3 < float(dead.float().mean()) < 0.7 and float(r64[dead].abs().max()) == 0.0
