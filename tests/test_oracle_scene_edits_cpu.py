"""The oracle's statement of the scene edits (oracle/stnerf_oracle.py: ``sources``, ``rotation``, ``layer_alpha``, the in-scene
layer passes -- DESIGN.md section 7), without a GPU.  Three questions: is the extension right (it agrees with the oracle it extends
wherever one definition can be turned into the other); do the inputs of tests/test_gpu_scene_edits_oracle.py have power (every
opacity entry and every rotation shows where that file looks); and does the comparison that file applies
(``scene_edits_common.assert_matches_oracle``) refuse a render with one of the errors a self-comparison lets through."""
import functools
import math

import pytest
import torch

from oracle import stnerf_oracle as O

import scene_edits_common as S
from instances_common import CENTRE, frame_ids
from test_gpu_rotation import rotated_rays

L_BASE = 4


@functools.lru_cache(maxsize=None)
def base(dtype=torch.float32):
    return S.oracle_render(S.make_case(), dtype=dtype)


def assert_same(a, b, what=""):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what} {k}: {int((a[k] != b[k]).sum())} of {a[k].numel()} entries differ"


# ---- 1. the extension is right
@pytest.mark.parametrize("only_coarse", [False, True])
def test_one_rotation_on_every_layer_is_the_plain_oracle_on_rotated_rays(only_coarse):
    case = S.make_case(rotation=[(0.6, CENTRE)] * L_BASE, only_coarse=only_coarse)
    rays = S.case_rays(case)
    turned = rotated_rays(rays, S.ray_matrix(0.6), torch.tensor(CENTRE))
    assert torch.equal(turned[:, 6:], rays[:, 6:]) and not torch.equal(turned[:, :6], rays[:, :6])
    got = S.oracle_render(case, rays)
    assert_same(got, S.oracle_render(dict(case, rotation=None), turned), "rotated")
    assert not torch.equal(got["coarse_mixed"], S.oracle_render(dict(case, rotation=None), rays)["coarse_mixed"])


def test_sources_are_the_wide_state_dict():
    case = S.make_case()
    wide_case, state = S.wide_of(case)
    assert wide_case["L"] == 3 and wide_case["sources"] == () and state[2].shape[1] == 3
    assert any(k.startswith("spacenets.2.") for k in state[0]) and any(k.startswith("time_deform_nets.2.") for k in state[0])
    assert_same(base(), S.oracle_render(wide_case, model=S.oracle_model(wide_case, state=state)), "wide")
    # the instance is on the picture and is no copy of its source
    assert int(base()["mask3"].sum()) >= 0.05 * S.N and not torch.equal(base()["coarse_layer3"], base()["coarse_layer1"])


def test_layer_alpha_one_one_a_is_alpha():
    a = 0.3
    plain3 = dict(L=2, sources=(), scale=None, shift=None, rotation=None, groups=[(0, [1.0, 2.5, 3.0])])
    for over, table in ((plain3, [1, 1, a]), ({}, [1, 1, a, None]), ({}, [None, 1.0, a, 1])):
        ref = S.oracle_render(S.make_case(layer_alpha=None, alpha=a, **over))
        assert_same(S.oracle_render(S.make_case(layer_alpha=table, **over)), ref, f"layer_alpha {table}")
        assert not torch.equal(ref["fine_mixed"], S.oracle_render(S.make_case(layer_alpha=None, **over))["fine_mixed"])
    # while a table is set alpha is ignored, and only_coarse ignores the table
    assert_same(S.oracle_render(S.make_case(alpha=a)), base(), "alpha under a table")
    assert_same(S.oracle_render(S.make_case(only_coarse=True)), S.oracle_render(S.make_case(only_coarse=True, layer_alpha=None)),
                "only_coarse")


@pytest.mark.parametrize("only_coarse", [False, True])
def test_the_passes_sum_to_the_mixed_image(only_coarse):
    """The bar of tests/test_gpu_scene_passes.py::test_the_passes_sum_to_the_mixed_image."""
    out = S.oracle_render(S.make_case(only_coarse=True)) if only_coarse else base()
    total = sum(out[f"scene{i}"] for i in range(L_BASE))
    torch.testing.assert_close(total, out["coarse_mixed" if only_coarse else "fine_mixed"], rtol=2e-5, atol=6e-6)
    if only_coarse:
        assert torch.equal(out["fine_mixed"], out["coarse_mixed"])
        assert not torch.equal(out["scene1"], base()["scene1"])
    # under a trace the weights come back at their source index: their sum is the mixed alpha, a missed layer's are zeros
    trace, case = {}, S.make_case(only_coarse=only_coarse)
    jitter, u = S.case_draws(case)
    draws = iter([j[:64] for j in jitter] + [x[:64] for x in u])
    got = O.render_chunk(S.oracle_model(case), S.case_rays(case)[:64], only_coarse=only_coarse, density_threshold=S.THR,
                         bkgd_density_threshold=S.BTHR, rand=lambda shape: next(draws), trace=trace)
    assert len(got) == 5
    mw = trace["merged_weights"]
    assert mw.shape == (64, L_BASE, 12 if only_coarse else 18)
    torch.testing.assert_close(mw.sum((1, 2)), got[0][2].squeeze(-1), rtol=2e-5, atol=6e-6)
    for i in range(1, L_BASE):
        assert not bool(mw[:, i][~got[4][i]].any())
        torch.testing.assert_close(trace["scene"][i][2].squeeze(-1), mw[:, i].sum(-1))


def test_a_quarter_turn_swaps_the_extents_of_layer_one():
    """tests/test_gpu_rotation.py::test_a_quarter_turn_swaps_the_extents_of_layer_one, on the oracle: layer 1's box spans x in
    [-1.2, -0.12], y, z in [-1, 1]; turned by pi / 2 about z through its centre (-0.66, 0, 0) it spans x in [-1.66, 0.34], y in
    [-0.54, 0.54]."""
    case = S.make_case(sources=(), scale=None, shift=None, layer_alpha=None, groups=[(0, [1.0, 1.0, 1.0])], n1=2, n2=0,
                       rotation=[None, math.pi / 2, None])
    m = S.oracle_model(case)
    rays = torch.tensor([[-2.0, 0.8, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0],            # along +x through (., 0.8, 0)
                         [-2.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0]])           # along +x through the centre
    boxes = O.layer_boxes(m, rays)[0]
    seen = O.layer_rays(m, rays, boxes)
    assert seen[0] is not None and torch.equal(seen[0], rays[:, :6]) and torch.equal(seen[2], rays[:, :6])
    zero = [torch.zeros(2, 2)] * 3                                                  # no jitter: t = near + k (far - near) / 2
    extent = lambda t: 2.0 * (t[1][:, 1, 0] - t[1][:, 0, 0])
    t0, _, m0 = O.sample_coarse(rays, boxes, 2, zero)
    t1, _, m1 = O.sample_coarse(rays, boxes, 2, zero, seen)
    assert m0[1].tolist() == [True, True] and m1[1].tolist() == [False, True]       # the off-centre ray misses the turned box
    assert t1[1][0, :, 0].tolist() == [-1000.0, -1000.0]
    assert abs(float(extent(t0)[0]) - 1.08) <= 1e-5 and abs(float(extent(t0)[1]) - 1.08) <= 1e-5
    assert abs(float(extent(t1)[1]) - 2.0) <= 1e-5
    assert abs(float(t0[1][1, 0, 0]) - 0.8) <= 1e-5 and abs(float(t1[1][1, 0, 0]) - 0.34) <= 1e-5      # entry points: x = -1.2, x = -1.66
    for i in (0, 2):
        assert torch.equal(t0[i], t1[i])


def test_the_defaults_are_absent():
    m = S.oracle_model(S.make_case())
    plain = O.OracleModel(layer_num=2, n_coarse=12, n_fine=6, params=m.params)
    assert plain.sources == () and plain.rotation is None and plain.layer_alpha is None
    assert plain.performers == 2 and plain.module_of(1) == 0 and plain.module_of(2) == 1
    assert m.performers == 3 and m.module_of(3) == 0
    with pytest.raises(ValueError, match="ray dimension"):                 # 7 or 7 + L + K wide
        O.layer_boxes(m, torch.zeros(4, 9))
    for field, bad in (("rotation", [None] * 3), ("layer_alpha", [1.0] * 3)):
        case = S.make_case()
        with pytest.raises(ValueError, match="one entry per layer"):
            S.oracle_render(case, model=S.oracle_model(case, **{field: bad}))


# ---- 2. the inputs have power
@pytest.mark.parametrize("i", range(L_BASE))
def test_every_opacity_entry_shows_in_the_mixed_image_and_in_its_pass(i):
    """One entry of the table alone against no table: the mixed fine colour, and that layer's scene pass, move by more than 5e-3
    (a hundred times COLOR_ATOL) on at least 40 of the 391 rays.  (On these scenes a performer's own fine output does not move:
    its last sample has delta = border, so its alpha stays 1 whatever the table says.)"""
    plain = S.oracle_render(S.make_case(layer_alpha=None))
    table = [None] * L_BASE
    table[i] = S.LAYER_ALPHA[i]
    got = S.oracle_render(S.make_case(layer_alpha=table))
    mixed, own = S.rays_changed(got["fine_mixed"], plain["fine_mixed"]), S.rays_changed(got[f"scene{i}"], plain[f"scene{i}"])
    print(f"opacity entry {i} ({S.LAYER_ALPHA[i]}) alone: mixed_fine moves on {mixed} rays, scene pass {i} on {own}")
    assert mixed >= 40 and own >= 40, (mixed, own)
    for k in plain:
        if k.startswith("coarse") or k.startswith("mask") or k == "t_coarse":
            assert torch.equal(got[k], plain[k]), k


@pytest.mark.parametrize("i", [1, 3])
def test_every_performer_rotation_shows_in_its_mask(i):
    rotation = list(S.make_case()["rotation"])
    assert rotation[i] is not None
    rotation[i] = None
    got = S.oracle_render(S.make_case(rotation=rotation))
    changed = int((got[f"mask{i}"] != base()[f"mask{i}"]).sum())
    print(f"rotation of layer {i} removed: its mask changes on {changed} rays")
    assert changed >= 20
    assert all(torch.equal(got[f"mask{j}"], base()[f"mask{j}"]) for j in range(L_BASE) if j != i)


def test_the_base_scene_hits_every_layer_and_both_precisions_agree_on_the_masks():
    hits = [int(base()[f"mask{i}"].sum()) for i in range(L_BASE)]
    print(f"hits per layer {hits}")
    assert hits[0] == S.N and all(h >= 0.2 * S.N for h in hits[1:])
    assert all(torch.equal(base()[f"mask{i}"], base(torch.float64)[f"mask{i}"]) for i in range(L_BASE))


# ---- 3. mutants: the GPU tests' comparison refuses each of them
def mutant_transposed_matrix():
    case = S.make_case()
    rot = S.oracle_rotation(case["rotation"])
    rot[1] = (rot[1][0].T.contiguous(), rot[1][1])                     # m = R instead of R^T on layer 1
    return S.oracle_render(case, model=S.oracle_model(case, rotation=rot))


def mutant_centre_of_the_unedited_box():
    case = S.make_case()
    unedited = O.layer_boxes(S.oracle_model(case, scale=None, shift=None), S.case_rays(case))[0]
    centre = torch.mean(unedited[0, 1], 0)
    edited = torch.mean(O.layer_boxes(S.oracle_model(case), S.case_rays(case))[0][0, 1], 0)
    assert float((centre - edited).abs().max()) >= 0.04                # (layer 1 is scaled by 1.1 and shifted by 0.05 in x)
    rot = S.oracle_rotation(case["rotation"])
    rot[1] = (rot[1][0], centre.tolist())
    return S.oracle_render(case, model=S.oracle_model(case, rotation=rot))


def mutant_table_rolled_by_one_layer():
    return S.oracle_render(S.make_case(layer_alpha=list(S.LAYER_ALPHA[-1:] + S.LAYER_ALPHA[:-1])))


def mutant_table_applied_at_coarse_too():
    """On the wide model (bit for bit the instanced one: test_sources_are_the_wide_state_dict) every layer owns its coarse
    network, whose density head is linear: scaled by the layer's entry, the coarse pass composites entry x density."""
    wide_case, (sd, bk, table) = S.wide_of(S.make_case())
    sd = dict(sd)
    for i, a in enumerate(S.LAYER_ALPHA):
        head = "bkgd_spacenet.density_net.0." if i == 0 else f"spacenets.{i - 1}.density_net.0."
        for k in ("weight", "bias"):
            sd[head + k] = sd[head + k] * a
    return S.oracle_render(wide_case, model=S.oracle_model(wide_case, state=(sd, bk, table)))


def mutant_instance_on_its_sources_frame_id():
    case = S.make_case()
    rays = S.case_rays(case)
    assert float(rays[0, 6 + 3]) != float(rays[0, 6 + 1])
    rays[:, 6 + 3] = rays[:, 6 + 1]
    return S.oracle_render(case, rays)


def mutant_two_passes_swapped():
    got = dict(base())
    got["scene1"], got["scene2"] = got["scene2"], got["scene1"]
    total = sum(got[f"scene{i}"] for i in range(L_BASE))                   # (the sum does not notice)
    torch.testing.assert_close(total, got["fine_mixed"], rtol=2e-5, atol=6e-6)
    return got


MUTANTS = [mutant_transposed_matrix, mutant_centre_of_the_unedited_box, mutant_table_rolled_by_one_layer,
           mutant_table_applied_at_coarse_too, mutant_instance_on_its_sources_frame_id, mutant_two_passes_swapped]


def test_the_comparison_accepts_the_oracle_itself():
    S.assert_matches_oracle(base(), base(), base(torch.float64), what="fp32 oracle")


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda f: f.__name__)
def test_the_comparison_refuses_the_mutant(mutant):
    got = mutant()
    with pytest.raises(AssertionError) as info:
        S.assert_matches_oracle(got, base(), base(torch.float64), what=mutant.__name__)
    print(f"{mutant.__name__}: {str(info.value).splitlines()[0]}")
