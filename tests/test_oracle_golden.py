"""Pin the CPU oracle against fixtures produced by the reference's own code
(tests/golden/make_golden.py).  CPU only; no GPU, no /root/reference at test time."""
import numpy as np
import pytest
import torch

from golden_io import load_golden, load_ray_views
from oracle import stnerf_oracle as O
from stnerf_amd import synthetic as syn

FWD_CASES = ["fwd_c1", "fwd_c3", "fwd_edit", "fwd_hide", "fwd_nonretime", "fwd_only_coarse",
             "batchify_chunked", "batchify_small", "fwd_bkgd_time", "fwd_same_spacenet", "fwd_deep_rgb", "fwd_no_raw_no_dir", "fwd_c4", "fwd_c5",
             "fwd_c3_90_30", "fwd_c3_90_30_chunked", "fwd_c3_64_64", "fwd_grazing", "fwd_bkgd_time_mixed_ids",
             # the BASELINE configurations at their own sample and layer counts, and the chunked call at its default chunk
             "fwd_c1_full", "fwd_c4_64_64", "fwd_c5_128_64", "batchify_default_chunk", "tf_c4_64_64", "tf_c5_128_64"]
TF_ONLY = ("pdf_", "u", "z_vals_fine", "coarse_weights", "xyz_fine_", "density_fine_", "raw_")   # a tf_ fixture's intermediates


def test_generate_rays():
    meta, a = load_golden("generate_rays")
    rays = O.generate_rays(a["K"], a["T"], meta["h"], meta["w"])
    assert torch.equal(rays, a["rays"])
    # production view sizes, where the order of torch.norm's sum shows (fused, x first): a whole 270 x 480 view and a pixel list of
    # a 1080p view, with at least 100 rays on which the unfused order gives another norm
    views = load_ray_views()
    assert sum(v["norms_differ"] for v in views.values()) >= 100
    for v in views.values():
        rays = O.generate_rays(v["K"], v["T"], v["h"], v["w"])
        assert torch.equal(rays if v["pixels"] is None else rays[v["pixels"].long()], v["rays"])


def test_sampler_bit_exact():
    meta, a = load_golden("sampler")
    n = a["rays"].shape[0]
    boxes = a["boxes"].unsqueeze(0).repeat(n, 1, 1, 1)
    for i in range(meta["L"] + 1):
        assert torch.equal(O.intersection(a["rays"], boxes[:, i]), a["far_near"][i])
    t, xyz, mask = O.sample_coarse(a["rays"], boxes, meta["n1"], list(a["jitter"]))
    assert torch.equal(torch.stack(t), a["t"])
    assert torch.equal(torch.stack(xyz), a["xyz"])
    assert torch.equal(torch.stack(mask), a["mask"])
    # the fixture really contains hits, misses and the layer-0 clamp
    assert a["mask"][1].any() and not a["mask"][1].all()


def test_encoding():
    _, a = load_golden("encoding")
    for tag, nf in (("pos", 10), ("dir", 4), ("time", 10), ("motion", 10)):
        assert torch.equal(O.positional_encoding(a[f"x_{tag}"], nf), a[f"y_{tag}"])


def test_nets():
    meta, a = load_golden("nets")
    rs = np.random.RandomState(meta["weight_seed"])
    sd_t = syn.spacenet_state("net", rs, True)
    sd_n = syn.spacenet_state("net", rs, False)
    sd_m = syn.motionnet_state("net", rs)
    rgb, sig = O.space_net(sd_t, "net", a["pos"], a["dirs"], a["times"])
    torch.testing.assert_close(rgb, a["rgb_t"], rtol=0, atol=2e-6)
    torch.testing.assert_close(sig, a["sigma_t"], rtol=1e-6, atol=2e-5)
    rgb, sig = O.space_net(sd_n, "net", a["pos"], a["dirs"])
    torch.testing.assert_close(rgb, a["rgb_n"], rtol=0, atol=2e-6)
    torch.testing.assert_close(sig, a["sigma_n"], rtol=1e-6, atol=2e-5)
    n, s = a["pos"].shape[:2]
    xt = torch.cat([a["pos"], a["times"].view(n, 1, 1).repeat(1, s, 1)], -1)
    torch.testing.assert_close(O.motion_net(sd_m, "net", xt), a["flow_frac"], rtol=0, atol=1e-6)
    xt = torch.cat([a["pos"], torch.floor(a["times"]).view(n, 1, 1).repeat(1, s, 1)], -1)
    torch.testing.assert_close(O.motion_net(sd_m, "net", xt), a["flow_int"], rtol=0, atol=1e-6)


def test_composite():
    meta, a = load_golden("composite")
    color, depth, acc, w = O.composite(a["t"], a["rgb"], a["sigma"], meta["border"])
    assert torch.equal(w, a["weights"])
    assert torch.equal(color, a["color"]) and torch.equal(depth, a["depth"]) and torch.equal(acc, a["acc"])


def test_sample_pdf():
    meta, a = load_golden("sample_pdf")
    z, cdf, inds = O.sample_pdf(a["t"], a["w"], a["u"], return_aux=True)
    assert torch.equal(z, a["z"])
    assert inds.dtype == torch.int64 and inds.min() >= 1 and inds.max() <= a["t"].shape[1] - 1
    assert O.sample_pdf(a["t"], a["w"], a["u"][:, :0]).shape == a["z_empty"].shape


@pytest.mark.parametrize("name", ["sample_pdf_90_30", "sample_pdf_128_64"])
def test_sample_pdf_at_production_sample_counts(name):
    """The shipped yml's 90 + 30 and the metric's 64 + 64 (per layer 128 + 64 at C5) on peaky weights: z bit-equal."""
    _, a = load_golden(name)
    assert torch.equal(O.sample_pdf(a["t"], a["w"], a["u"]), a["z"])


def test_grazing_fixture_has_the_background_corner_cases():
    """fwd_grazing pins what the reference does with rays that touch the background box in one point (ray_mask[0]
    False, bin width 0) -- it still evaluates and composites the background there (layered_rfrender.py:382-392) --
    and with rays that miss it (far = -1000, descending depths)."""
    _, a = load_golden("fwd_grazing")
    grazing = ~a["mask0"]
    assert int(grazing.sum()) == 2
    assert float(a["fine_mixed_acc"][grazing].min()) > 0.99 and float(a["fine_layer0_color"][grazing].min()) > 0.1
    miss = a["mask0"] & (a["fine_mixed_acc"].squeeze(-1) == 0)
    assert int(miss.sum()) >= 2


def _replayer(draws):
    it = iter(draws)

    def rand(shape):
        x = next(it)
        assert tuple(x.shape) == tuple(shape), (x.shape, shape)
        return x
    return rand


def _model_from_meta(meta):
    L = meta["L"]
    bk, per = syn.scene_boxes(L)
    fl = meta.get("flags", {})
    sd = syn.state_dict_for_flags(L, meta["space_time"], meta["deform_time"], meta["weight_seed"], fl)
    m = O.OracleModel(layer_num=L, n_coarse=meta["n1"], n_fine=meta["n2"], params=sd,
                      use_deform_time=meta["deform_time"], use_space_time=meta["space_time"],
                      bkgd_use_deform_time=fl.get("BKGD_USE_DEFORM_TIME", False),
                      bkgd_use_space_time=fl.get("BKGD_USE_SPACE_TIME", False), bkgd_bbox=bk, bboxes=per)
    e = meta["edit"]
    m.scale, m.shift = e.get("scale"), e.get("shift")
    m.alpha, m.near = e.get("alpha", 1.0), e.get("near", 0.0)
    m.hidden = set(e.get("hide", []))
    return m


def _flatten(out):
    fm, cm, fl, cl, masks = out
    d = {}
    for tag, trip in (("fine_mixed", fm), ("coarse_mixed", cm)):
        for nm, x in zip(("color", "depth", "acc"), trip):
            d[f"{tag}_{nm}"] = x
    for tag, lst in (("fine_layer", fl), ("coarse_layer", cl)):
        for i, trip in enumerate(lst):
            for nm, x in zip(("color", "depth", "acc"), trip):
                d[f"{tag}{i}_{nm}"] = x
    for i, mk in enumerate(masks):
        d[f"mask{i}"] = mk
    return d


def _compare_with_reference(name, batchify=None):
    """Render fixture ``name`` with the oracle and hold every output to the reference's.  ``batchify``: a stand-in for
    O.layered_batchify_ray (the tests that show a fixture can fail)."""
    meta, a = load_golden(name)
    m = _model_from_meta(meta)
    draws = [a[f"draw{i}"] for i in range(meta["n_draws"])]
    rand = _replayer(draws)
    kw = meta["call_kwargs"]
    with torch.no_grad():
        if meta["chunk"] is None:
            out = O.render_chunk(m, a["rays"], only_coarse=meta["only_coarse"], rand=rand, **kw)
        else:
            out = (batchify or O.layered_batchify_ray)(m, a["rays"], chuncks=meta["chunk"], rand=rand, **kw)
    got = _flatten(out)
    keys = [k for k in a if k not in ("rays",) and not k.startswith("draw") and not (name.startswith("tf_") and k.startswith(TF_ONLY))]
    assert set(keys) == set(got)
    for k in keys:
        if k.startswith("mask"):
            assert torch.equal(got[k], a[k]), k
        else:
            # same ATen ops on the same machine class: agreement is at rounding level
            torch.testing.assert_close(got[k], a[k], rtol=1e-5, atol=2e-6, msg=lambda s, k=k: f"{k}: {s}")
    # fixtures are not numerically trivial: something is actually composited
    assert float(a["fine_mixed_acc"].max()) > 0.1
    return meta, a


@pytest.mark.parametrize("name", FWD_CASES)
def test_forward_matches_reference(name):
    _compare_with_reference(name)


def test_real_count_fixtures_reach_every_layer_without_depth_ties():
    """What tests/golden/make_golden.py --real-counts asserts when it writes them, read back from the files: every performer
    layer hit by at least 8 rays, at most 0.5 % of the rays swapped for an exact depth tie, the sample counts the names say."""
    counts = dict(fwd_c1_full=(1, 32, 0), fwd_c4_64_64=(4, 64, 64), tf_c4_64_64=(4, 64, 64), fwd_c5_128_64=(8, 128, 64),
                  tf_c5_128_64=(8, 128, 64), batchify_default_chunk=(2, 12, 6))
    for name, want in counts.items():
        meta, a = load_golden(name)
        assert (meta["L"], meta["n1"], meta["n2"]) == want
        assert min(int(a[f"mask{i}"].sum()) for i in range(1, meta["L"] + 1)) >= 8, name
        assert len(meta["swapped_rays"]) <= 0.005 * a["rays"].shape[0], name
    meta, a = load_golden("batchify_default_chunk")
    n, chunk = a["rays"].shape[0], meta["chunk"]
    assert chunk == 3584 and n >= 2 * chunk + 1 and meta["call_kwargs"] == dict(density_threshold=0.05, bkgd_density_threshold=0.02)
    assert a["rays"][[0, chunk, 2 * chunk], 7:].tolist() == [[2.5, 2.5], [1.0, 2.75], [3.0, 1.5]]
    assert a["rays"][4000, 7:].tolist() == [3.0, 2.75] and a["rays"][3999, 7:].tolist() == [1.0, 2.75]
    assert load_golden("fwd_c1_full")[1]["rays"].shape[0] > 3584        # two reference chunks


def test_default_chunk_fixture_refuses_boxes_taken_from_the_first_chunk():
    """batchify_default_chunk can fail (a): an oracle whose every chunk takes its boxes from the CALL's row 0, not from its own
    (modeling/layered_rfrender.py:195-200 reads row 0 of what the model is handed, which is one chunk), is refused -- on the masks."""
    _, a = load_golden("batchify_default_chunk")
    orig = O.layer_boxes

    def boxes_of_chunk0(m, rays):
        mine = orig(m, rays)
        first = orig(m, a["rays"][:rays.shape[0]])
        return (first[0], first[1]) + tuple(mine[2:])

    def batchify(m, rays, **kw):
        O.layer_boxes = boxes_of_chunk0
        try:
            return O.layered_batchify_ray(m, rays, **kw)
        finally:
            O.layer_boxes = orig
    with pytest.raises(AssertionError, match="mask|coarse|fine"):
        _compare_with_reference("batchify_default_chunk", batchify)
    assert O.layer_boxes is orig


def test_default_chunk_fixture_refuses_dropped_thresholds():
    """batchify_default_chunk can fail (b): an oracle that drops both thresholds in the chunked branch, as the small-call branch
    does (utils/batchify_rays.py:52-54), is refused."""
    def batchify(m, rays, chuncks, rand, density_threshold, bkgd_density_threshold):
        return O.layered_batchify_ray(m, rays, chuncks=chuncks, rand=rand, density_threshold=0.0001, bkgd_density_threshold=0.0)
    with pytest.raises(AssertionError, match="coarse|fine"):
        _compare_with_reference("batchify_default_chunk", batchify)
