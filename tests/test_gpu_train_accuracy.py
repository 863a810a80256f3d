"""The split-bf16 training kernels held to "fp32-faithful" against fp64 (include/stnerf.h promises it for stnerf_train_dw_batch's
2 x 2 bundles and for stnerf_train_spacenet_dx_bf16x3).  Needs an MI355X: `pytest -m gpu`.

One measure and one yardstick (tests/train_accuracy_common.py; tests/test_train_accuracy_cpu.py shows on the CPU that the bar tells
six bf16 products from five):

  * dW / db: the componentwise error max |got - want64| / sum_s |dy_si x_sj| of the kernel is at most BAR = 3 x that of torch's fp32
    CPU matmul on the same operands, per problem -- on randn operands, on operands whose columns are scaled apart by 2^-20 .. 2^20,
    and on two designs in which the bf16-exact part of one operand cancels.  Every kind of tile, sample counts on both sides of the
    split-bf16 bundle's 32-sample unit, the shared-input bundle at op level, operands that are row ranges of taller buffers with live
    (NaN) rows before and after; dw, db and a workspace of exactly the planner's byte count between guard zones in every call.
  * the dx chain, both arithmetics, and the activations the training forward stores: the error relative to the matrix's largest entry
    at most BAR x that of the same chain in fp32 on the CPU, both against the chain in fp64.
  * the kept-activation counter of modeling/autograd.py returns to where it was.

The tests print their kernel / yardstick ratios as table rows (profiles/train_bf16x3_accuracy.md holds a run's)."""
import functools
import gc

import numpy as np
import pytest
import torch

from oracle import stnerf_oracle as O
from stnerf_amd import synthetic as syn
from test_gpu_canaries import Canaries
import train_accuracy_common as T

pytestmark = pytest.mark.gpu

NAN = float("nan")
DW0, DB0 = 0.5, -0.25                         # what accumulate = True adds onto
MS = (63, 64, 65, 96, 127, 128, 255, 256)     # 63: below 4 * DWW_BLOCK, no bundle -- the same shapes on the f32 tiles
# (n, k, with db): the split-bf16 bundle; the bundle with its second column tile 31 columns past k; bundle + a 64-wide f32 tile; bundle + a
# 96-wide tile; a 64-wide tile alone; a 96-wide tile; the 32-row head tiles; several row blocks with remainders on both sides
SHAPES = ((256, 256, True), (256, 225, True), (256, 319, False), (256, 352, True), (256, 63, True), (128, 84, True), (3, 128, True),
          (1, 256, True), (300, 300, True))
TILE_BUNDLES = (4, 0, 0)                      # the four 256-output shapes of 256 columns and more, in split bf16
ROW_RANGE_MS, ROW_RANGE_R0 = (65, 128, 255), (0, 32, 37 * 4)


@pytest.fixture(scope="module")
def ops():
    from stnerf_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


# ---- operands, references (computed once, never written to), the guarded launch ---------------------------------------------------
def _operand(t, r0=None, extra=0):
    """t (m, cols) -> a CUDA view of 16-byte aligned rows holding it, NaN in the column padding (+ `extra` NaN columns).  r0: the view is
    rows r0 .. r0 + m of a taller buffer with NaN in every other row (the chunks of kept activation planes in the autograd path)."""
    m, cols = t.shape
    before, after = (0, 0) if r0 is None else (r0, 37)
    buf = torch.full((before + m + after, (cols + 3) // 4 * 4 + extra), NAN, device="cuda")
    buf[before:before + m, :cols] = torch.from_numpy(np.ascontiguousarray(t)).cuda()
    return buf[before:before + m, :cols]


class Problem:
    """One (dy, x) of a launch with its fp64 references' yardsticks: the componentwise error of torch's fp32 CPU matmul (and of the
    fp32 column sums as the same matmul against ones, with the floor T.U32), plain and accumulated onto DW0 / DB0 in fp32."""

    def __init__(self, tag, dy, x, with_db=True):
        self.tag, self.dy, self.x, self.with_db = tag, dy, x, with_db
        self.n, self.k = dy.shape[1], x.shape[1]
        prod, sums = T.fp32_matmul(dy, x), T.fp32_column_sums(dy)
        self.yard_dw = {False: T.componentwise(prod, dy, x), True: T.componentwise(np.float32(DW0) + prod, dy, x, base=DW0)}
        self.yard_db = {False: max(T.componentwise_sum(sums, dy), T.U32), True: max(T.componentwise_sum(np.float32(DB0) + sums, dy, base=DB0), T.U32)}

    def dw_error(self, got, accumulate):
        return T.componentwise(got, self.dy, self.x, base=DW0 if accumulate else None)

    def db_error(self, got, accumulate):
        return T.componentwise_sum(got, self.dy, base=DB0 if accumulate else None)


@functools.lru_cache(maxsize=None)
def _tile_problems(name, m):
    return tuple(Problem(f"({n}, {k})", *T.design(name, m, n, k), with_db=db) for n, k, db in SHAPES)


@functools.lru_cache(maxsize=None)
def _shared_problems(name, m):
    """What SpaceNetFunction.backward passes for stage1.0, stage2.0 and one plain layer: X (m, 320) = [h | PE | 0], the problems
    (dyA, X[:, 256:319]), (dyB, X[:, :319]) and a (256, 256) layer.  -> (X, problems, stage2.0's 63 skip columns as a problem of their
    own: beside 256 columns of h they are a small block of a 256 x 319 tensor)"""
    dyB, xB = T.design(name, m, 256, 319)
    dyA, _ = T.design(name, m, 256, 63, seed=1)
    X = np.zeros((m, 320), dtype=np.float32)
    X[:, :319] = xB
    return X, (Problem("stage1.0 on X[:, 256:319]", dyA, X[:, 256:319]), Problem("stage2.0 on X[:, :319]", dyB, X[:, :319]),
               Problem("plain (256, 256)", *T.design(name, m, 256, 256, seed=2))), Problem("skip columns", dyB, np.ascontiguousarray(X[:, 256:319]))


def _launch(ops, monkeypatch, problems, operands, accumulate, what, bundles):
    """ops.train_dw_batch on `operands` = [(dy, x)] device views of `problems`, with every dw, db and a workspace of EXACTLY the bytes the
    planner asks for between guard zones; every guard intact afterwards.  `bundles`: the plan's (split-bf16 2 x 2, f32 2 x 2,
    shared-input) bundle counts (stnerf_train_dw_batch_plan) -- no bundle below 4 * DWW_BLOCK = 64 samples -- so that a planner that
    stops forming them cannot leave these tests green on the f32 tiles.  -> [(dw, db | None)] as numpy."""
    ops.free_workspaces()
    monkeypatch.setattr(ops, "_dw_workspace", lambda need, device: torch.empty(int(need), dtype=torch.uint8, device=device))
    with Canaries() as c:
        dws = [torch.full((p.n, p.k), DW0 if accumulate else NAN, device="cuda") for p in problems]
        dbs = [torch.full((p.n,), DB0 if accumulate else NAN, device="cuda") if p.with_db else None for p in problems]
        layers = [(dy, x, dw, db) for (dy, x), dw, db in zip(operands, dws, dbs)]
        plan = ops.train_dw_batch_bundles(layers)
        assert plan == (bundles if operands[0][0].shape[0] >= 64 else (0, 0, 0)), (what, plan, bundles)
        ops.train_dw_batch(layers, accumulate)
        guarded = c.check(what)
    ops.free_workspaces()
    assert guarded == len(dws) + sum(db is not None for db in dbs) + 1, (what, guarded)          # ... + the workspace
    return [(dw.cpu().numpy(), None if db is None else db.cpu().numpy()) for dw, db in zip(dws, dbs)]


def _ratio(err, yard):
    return err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))


def _judge(problems, results, accumulate, what):
    """Print every figure, then hold each problem to BAR x its yardstick.  -> [(dw ratio, db ratio | None)]"""
    ratios, failures = [], []
    for p, (dw, db) in zip(problems, results):
        assert np.isfinite(dw).all() and (db is None or np.isfinite(db).all()), (what, p.tag)
        e_dw, e_db = p.dw_error(dw, accumulate), (p.db_error(db, accumulate) if db is not None else None)
        r_dw, r_db = _ratio(e_dw, p.yard_dw[accumulate]), (_ratio(e_db, p.yard_db[accumulate]) if db is not None else None)
        print(f"    {what} accumulate={int(accumulate)} {p.tag}: dW {e_dw:.2e} (fp32 CPU {p.yard_dw[accumulate]:.2e}) = {r_dw:.2f} x" +
              ("" if db is None else f"; db {e_db:.2e} ({p.yard_db[accumulate]:.2e}) = {r_db:.2f} x"))
        ratios.append((r_dw, r_db))
        if r_dw > T.BAR or (r_db is not None and r_db > T.BAR):
            failures.append((p.tag, r_dw, r_db))
    assert not failures, (what, accumulate, failures)
    return ratios


def _row(case, name, m, problems, ratios_by_mode):
    """One table row: per problem the worse of the two modes' dW ratios, then the worst db ratio."""
    dw = [max(r[i][0] for r in ratios_by_mode) for i in range(len(problems))]
    db = [r[i][1] for r in ratios_by_mode for i in range(len(problems)) if r[i][1] is not None]
    print(f"| {case} | {name} | {m} | " + " | ".join(f"{v:.2f}" for v in dw) + f" | {max(db):.2f} |")


# ---- (a), (d): every kind of tile ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("name", T.DESIGNS)
def test_dw_batch_is_fp32_faithful_componentwise_on_every_kind_of_tile(ops, monkeypatch, name, m):
    """(columns of the printed row: the SHAPES in order, then db)"""
    problems = _tile_problems(name, m)
    operands = [(_operand(p.dy), _operand(p.x, extra=4)) for p in problems]
    ratios = []
    for accumulate in (False, True):
        what = f"tiles {name} m={m}"
        ratios.append(_judge(problems, _launch(ops, monkeypatch, problems, operands, accumulate, what, TILE_BUNDLES), accumulate, what))
    _row("dW tiles", name, m, problems, ratios)


# ---- (b): the shared-input bundle (dww_plan case (b)) at op level -----------------------------------------------------------------
def _shared_operands(X, problems, r0=None, own_x=False):
    Xd = _operand(X, r0)
    xa = _operand(problems[0].x, r0) if own_x else Xd[:, 256:319]
    return [(_operand(problems[0].dy, r0), xa), (_operand(problems[1].dy, r0), Xd[:, :319]),
            (_operand(problems[2].dy, r0), _operand(problems[2].x, r0, extra=4))]


def _check_shared(ops, monkeypatch, name, m, r0, case):
    X, problems, skip = _shared_problems(name, m)
    ratios = []
    for accumulate in (False, True):
        what = f"{case} {name} m={m}" + ("" if r0 is None else f" r0={r0}")
        shared = _launch(ops, monkeypatch, problems, _shared_operands(X, problems, r0), accumulate, what, (2, 0, 1))      # dww_plan case (b)
        ratios.append(_judge(problems, shared, accumulate, what))
        e, y = skip.dw_error(shared[1][0][:, 256:319], accumulate), skip.yard_dw[accumulate]
        print(f"    {what} accumulate={int(accumulate)} skip columns alone: {e:.2e} (fp32 CPU {y:.2e}) = {_ratio(e, y):.2f} x")
        assert e <= T.BAR * y, (what, accumulate, e, y)
        # the same problems with stage1.0's x in a tensor of its own: nothing to share, another summation order, the same result within
        # BAR x the yardstick
        apart = _launch(ops, monkeypatch, problems, _shared_operands(X, problems, r0, own_x=True), accumulate, what + " (own x)", (2, 0, 0))
        _judge(problems, apart, accumulate, what + " (own x)")
        for p, (dw_s, db_s), (dw_a, db_a) in zip(problems[:2], shared, apart):
            den = np.abs(p.dy.astype(np.float64)).T @ np.abs(p.x.astype(np.float64)) + (DW0 if accumulate else 0.0)
            diff = T.worst_ratio(np.abs(dw_s.astype(np.float64) - dw_a), den)
            assert diff <= T.BAR * p.yard_dw[accumulate], (what, p.tag, diff, p.yard_dw[accumulate])
            den_b = np.abs(p.dy.astype(np.float64)).sum(0) + (abs(DB0) if accumulate else 0.0)
            diff_b = T.worst_ratio(np.abs(db_s.astype(np.float64) - db_a), den_b)
            assert diff_b <= T.BAR * p.yard_db[accumulate], (what, p.tag, diff_b, p.yard_db[accumulate])
    _row(case, name, m if r0 is None else f"{m} @ {r0}", problems, ratios)


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("name", T.DESIGNS)
def test_shared_input_bundle_is_fp32_faithful_at_op_level(ops, monkeypatch, name, m):
    """(columns of the printed row: stage1.0, stage2.0, the plain layer, then db)"""
    _check_shared(ops, monkeypatch, name, m, None, "dW shared")


# ---- (c): operands that are row ranges of taller buffers ------------------------------------------------------------------------------
@pytest.mark.parametrize("r0", ROW_RANGE_R0)
@pytest.mark.parametrize("m", ROW_RANGE_MS)
@pytest.mark.parametrize("name", T.DESIGNS)
def test_rows_around_a_sample_range_contribute_nothing(ops, monkeypatch, name, m, r0):
    """dy and x = buf[r0 : r0 + m] of buffers with NaN in every other row: the same bars, no NaN in any output."""
    problems = _tile_problems(name, m)
    operands = [(_operand(p.dy, r0), _operand(p.x, r0, extra=4)) for p in problems]
    for accumulate in (False, True):
        what = f"row range {name} m={m} r0={r0}"
        _judge(problems, _launch(ops, monkeypatch, problems, operands, accumulate, what, TILE_BUNDLES), accumulate, what)
    _check_shared(ops, monkeypatch, name, m, r0, "dW shared, row range")


# ---- (e), (f): the dx chain and the stored activations against fp64 -----------------------------------------------------------------
KEYS = ("stage1.0", "stage1.2", "stage1.4", "stage1.6", "stage2.0", "stage2.2", "stage2.4", "density_net.0", "rgb_net.1", "rgb_net.3")


def _net_case(use_time, n, ns=19, seed=5, wide=False):
    """The setup of test_split_bf16_backward_chain_matches_the_exact_f32_chain; wide: the weights of
    test_bf16x3_operands_have_no_range_limits (activations of 1e6 behind stage1.2, divided away again by stage2.4)."""
    from stnerf_amd.modeling.spacenet import SpaceNet
    sd = syn.spacenet_state("net", np.random.RandomState(seed), use_time)
    if wide:
        sd["net.stage1.0.weight"] = sd["net.stage1.0.weight"] * 3000.0
        sd["net.stage1.2.weight"] = sd["net.stage1.2.weight"] * 40.0
        sd["net.stage2.4.weight"] = sd["net.stage2.4.weight"] / 120000.0
    net = SpaceNet(use_time=use_time)
    net.load_state_dict({k[4:]: v for k, v in sd.items()})
    net = net.cuda()
    g = torch.Generator().manual_seed(seed)
    pos = (torch.rand(n, ns, 3, generator=g) - 0.5) * 4
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    tm = torch.rand(n, 1, generator=g) * 20 + 1 if use_time else None
    return net, sd, pos, dirs, tm


def _forward_tap(ops, net, precision, pos, dirs, tm):
    from stnerf_amd.modeling import autograd as A
    n, ns = pos.shape[0], pos.shape[1]
    bufs = A._activation_buffers(n * ns, 48, "cuda")
    for b in bufs[:8]:
        b.fill_(NAN)
    raw = torch.empty(n, ns, 4, device="cuda")
    ops.train_spacenet_fwd(net._packed(precision), pos.cuda(), dirs.cuda(), tm.reshape(n).cuda() if tm is not None else None, raw,
                           A._act_views(bufs), bufs[0][:, 256:320], bufs[8])
    torch.cuda.synchronize()
    return bufs, raw


def _layer_outputs(sd, pos, dirs, tm, dtype):
    """The oracle's SpaceNet (oracle/stnerf_oracle.py: space_net) layer by layer, with its own encoding and linear layers: the eight
    post-ReLU matrices the training forward stores, PE(pos), and (rgb, sigma)."""
    p = {k: v.to(dtype) for k, v in sd.items()}
    n, s = pos.shape[0], pos.shape[1]
    pe = O.positional_encoding(pos.to(dtype).reshape(-1, 3), 10, True)
    acts, h = [], pe
    for j in (0, 2, 4, 6):
        h = torch.relu(O._linear(p, f"net.stage1.{j}", h))
        acts.append(h)
    h = torch.cat([h, pe], 1)
    for j in (0, 2, 4):
        h = torch.relu(O._linear(p, f"net.stage2.{j}", h))
        acts.append(h)
    sigma = O._linear(p, "net.density_net.0", h)
    feat = [h, O.positional_encoding(dirs.to(dtype).unsqueeze(1).repeat(1, s, 1).reshape(-1, 3), 4, True)]
    if tm is not None:
        feat.append(O.positional_encoding(tm.to(dtype).reshape(n, 1, 1).repeat(1, s, 1).reshape(-1, 1), 10, True))
    t0 = torch.relu(O._linear(p, "net.rgb_net.1", torch.relu(torch.cat(feat, 1))))
    acts.append(t0)
    return acts, pe, O._linear(p, "net.rgb_net.3", t0).reshape(n, s, 3), sigma.reshape(n, s, 1)


def _chain(W, masks, d_raw, dtype):
    """include/stnerf.h: d act_{s-1} = (d act_s * [act_s > 0]) W_s from the heads back (modeling/spacenet.py:101-160 under autograd):
    -> the eight pre-activation gradients (stage1.0 .. stage2.4, rgb_net.1) and d PE(pos).  W: the ten weights in KEYS' order."""
    W, m, d = [w.to(dtype) for w in W], [k.to(dtype) for k in masks], d_raw.to(dtype)
    dy = [None] * 8
    dy[7] = (d[:, :3] @ W[9]) * m[7]
    dy[6] = (dy[7] @ W[8][:, :256] + d[:, 3:] @ W[7]) * m[6]
    dy[5] = (dy[6] @ W[6]) * m[5]
    dy[4] = (dy[5] @ W[5]) * m[4]
    into_skip = dy[4] @ W[4]                          # [h4 | PE(pos)]
    dy[3] = into_skip[:, :256] * m[3]
    dy[2] = (dy[3] @ W[3]) * m[2]
    dy[1] = (dy[2] @ W[2]) * m[1]
    dy[0] = (dy[1] @ W[1]) * m[0]
    return dy, dy[0] @ W[0] + into_skip[:, 256:]


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("use_time, n, want_dpos", [(True, 1, True), (False, 7, True), (True, 37, True), (True, 128, True), (False, 37, False)])
def test_dx_chain_matches_the_fp64_chain_as_well_as_the_fp32_cpu_chain(ops, use_time, n, want_dpos, wide):
    """(columns of the printed rows: d y of stage1.0 .. stage2.4, rgb_net.1, then d PE(pos))

    Both kernels on the masks of a split-bf16 forward tap.  What this test found: stnerf_train_spacenet_dx (exact f32) was 5.0 - 8.5 x the
    yardstick at d y of stage2.4 (6e-7 of the largest entry where the fp32 CPU chain and the split-bf16 kernel have 8e-8 and 4e-8): the
    density head's rank-1 term d sigma w_sigma, ~12 x the 128-deep product d y7 W_rgb1 it is added to, was that product's C operand, so
    each of the 64 K = 2 steps rounded at its size (a CPU restatement gives 5.5e-7 with the term first, 7.9e-8 with it last).  It is
    added behind the product now (csrc/train_wave.hip)."""
    from stnerf_amd.modeling import autograd as A
    net, sd, pos, dirs, tm = _net_case(use_time, n, wide=wide)
    M = pos.shape[0] * pos.shape[1]
    bufs, _ = _forward_tap(ops, net, "bf16x3", pos, dirs, tm)
    masks = [(a > 0).cpu() for a in A._act_views(bufs)]
    d_raw = torch.randn(M, 4, generator=torch.Generator().manual_seed(11))
    W = [sd[f"net.{k}.weight"] for k in KEYS]
    want64, dpe64 = _chain(W, masks, d_raw, torch.float64)
    cpu32, dpe32 = _chain(W, masks, d_raw, torch.float32)
    yard = [T.rel_to_max(a.numpy(), b.numpy()) for a, b in zip(cpu32, want64)] + [T.rel_to_max(dpe32.numpy(), dpe64.numpy())]
    params = [p.detach() for p in net.training_parameters()]
    mk = lambda: [torch.full((M, 256), NAN, device="cuda") for _ in range(7)] + [torch.full((M, 128), NAN, device="cuda")]
    d_dev = d_raw.cuda()
    results = {}
    got = mk()
    dpe = torch.full((M, 64), NAN, device="cuda") if want_dpos else None
    dpe_skip = torch.full((M, 64), NAN, device="cuda") if want_dpos else None
    ops.train_spacenet_dx_bf16x3(A.dx_blob_bf16x3(net, params, want_dpos), d_dev, bufs[8], got, dpe, dpe_skip)
    results["bf16x3"] = (got, dpe + dpe_skip if want_dpos else None)
    got = mk()
    dpe = torch.full((M, 64), NAN, device="cuda") if want_dpos else None
    wt, offsets = A.transposed_spacenet(net, params)
    ops.train_spacenet_dx(wt, offsets, d_dev, bufs[8], got, dpe)
    results["f32"] = (got, dpe)
    torch.cuda.synchronize()
    failures = []
    for kernel, (dys, total) in results.items():
        errs = [T.rel_to_max(a.cpu().numpy(), b.numpy()) for a, b in zip(dys, want64)]
        if want_dpos:
            assert float(total[:, 63].abs().max()) == 0.0                                     # (the pad column)
            errs.append(T.rel_to_max(total[:, :63].cpu().numpy(), dpe64.numpy()))
        assert all(np.isfinite(e) for e in errs), (kernel, errs)
        ratios = [_ratio(e, y) for e, y in zip(errs, yard)]
        print(f"    dx {kernel} wide={int(wide)} n={n}: kernel " + " ".join(f"{e:.2e}" for e in errs) + " | fp32 CPU " + " ".join(f"{y:.2e}" for y in yard))
        print(f"| dx {kernel} | {'wide' if wide else 'plain'} weights{'' if use_time else ', no time'} | {n} x 19 | " + " | ".join(f"{r:.2f}" for r in ratios) +
              ("" if want_dpos else " | - ") + " |")
        failures += [(kernel, s_, r) for s_, r in enumerate(ratios) if r > T.BAR]
    assert not failures, failures


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
@pytest.mark.parametrize("use_time, n", [(True, 1), (False, 37), (True, 37), (True, 128)])
def test_stored_activations_match_the_fp64_oracle_as_well_as_the_fp32_cpu_chain(ops, use_time, n, precision):
    """(columns of the printed row: the outputs of stage1.0 .. stage2.4, rgb_net.1, then PE(pos))

    Split bf16 met the bar everywhere from the start (0.30 - 1.00 x for the matrices, 2.3 - 2.5 x for PE(pos), whose yardstick is
    torch's fp32 sin / cos at 1.8e-8).  What this test found: exact f32 was 3.1 - 5.6 x at rgb_net.1's output (8.1e-7 - 1.1e-6 of the
    largest entry, the fp32 CPU chain 1.7e-7 - 3.5e-7).  The ray's row of the bias table (rgb_net.1's bias + its direction / time
    columns, csrc/mlp_raybias.hip) was the C operand of the layer's chain of 128 K = 2 steps (csrc/mlp_wave_core.h) and ~10 x the backbone
    product added to it, so each step rounded the running sum at the bias's size (a CPU restatement: 8.1e-7 with the bias first, 9e-8
    with it last).  The exact-f32 kernels now start that chain from 0 and add the row behind it, as the split-bf16 kernels always did:
    0.91 - 1.15 x in that column."""
    from stnerf_amd.modeling import autograd as A
    net, sd, pos, dirs, tm = _net_case(use_time, n, seed=0)
    bufs, raw = _forward_tap(ops, net, precision, pos, dirs, tm)
    acts64, pe64, rgb64, sig64 = _layer_outputs(sd, pos, dirs, tm, torch.float64)
    acts32, pe32, _, _ = _layer_outputs(sd, pos, dirs, tm, torch.float32)
    o_rgb, o_sig = O.space_net({k: v.double() for k, v in sd.items()}, "net", pos.double(), dirs.double(), tm.double() if use_time else None)
    assert torch.equal(o_rgb, rgb64) and torch.equal(o_sig, sig64)               # (the restatement IS the oracle's network)
    got = [a.cpu().numpy() for a in A._act_views(bufs)] + [bufs[0][:, 256:319].cpu().numpy()]
    want = [a.numpy() for a in acts64] + [pe64.numpy()]
    yard = [T.rel_to_max(a.numpy(), b) for a, b in zip(acts32 + [pe32], want)]
    errs = [T.rel_to_max(a, b) for a, b in zip(got, want)]
    ratios = [_ratio(e, y) for e, y in zip(errs, yard)]
    print(f"    activations {precision} n={n}: kernel " + " ".join(f"{e:.2e}" for e in errs) + " | fp32 CPU " + " ".join(f"{y:.2e}" for y in yard))
    print(f"| activations {precision} | {'time' if use_time else 'no time'} | {n} x 19 | " + " | ".join(f"{r:.2f}" for r in ratios) + " |")
    assert all(np.isfinite(e) for e in errs) and float(bufs[0][:, 319].abs().max()) == 0.0
    assert all(r <= T.BAR for r in ratios), [(s_, r) for s_, r in enumerate(ratios) if r > T.BAR]


# ---- (g): the kept-activation accounting ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_backward", [True, False])
def test_kept_activation_bytes_return_to_where_they_were(ops, run_backward):
    from stnerf_amd.modeling import autograd as A
    gc.collect()
    start = A._kept_now[0]
    net, _, pos, dirs, tm = _net_case(True, 37)
    net.train()
    rays = torch.cat([torch.zeros(37, 3), dirs], -1).cuda()
    rgb, sig = net(pos.cuda().requires_grad_(True), rays, tm.cuda())
    assert rgb.requires_grad and A._kept_now[0] == start + 37 * 19 * A.ACT_FLOATS_PER_SAMPLE * 4 > start
    if run_backward:
        (rgb.sum() + sig.sum()).backward()
    del rgb, sig
    gc.collect()
    assert A._kept_now[0] == start
