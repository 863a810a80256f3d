"""What "fp32-faithful" means for the split-bf16 training kernels, stated without a GPU (numpy / torch on the CPU only).

stnerf_train_dw_batch's 2 x 2 bundles (csrc/train_dw.hip: dwb_run_bx) split both operands of dW = dY^T X into three bf16 pieces on the
fly and issue six bf16 MFMAs per product; stnerf_train_spacenet_dx_bf16x3 (csrc/train_bf16x3.hip) multiplies a gradient split on the
fly with pre-split weights, a0 b0 into a `big` accumulator and the five small terms into a second one.  This module holds

  * ``split3`` / ``emulate``: that arithmetic restated -- NOT the code under test: when a kernel misses its bar, comparing its output
    with the six-term emulation and with each five-term variant says which product or which piece is wrong;
  * ``componentwise`` / ``rel_to_max``: the two measures.  The componentwise one, max |got - want| / sum_s |dy_si x_sj|, does not
    change when a row or a column of the result is scaled, so small columns count as much as large ones;
  * the seeded input designs;
  * the yardstick: the same measure for torch's fp32 CPU matmul on the same inputs (what the reference's autograd computes), and
    BAR = 3 of them (the FP32_NOISE_FACTOR of tests/test_gpu_training.py).

tests/test_train_accuracy_cpu.py shows that BAR x the yardstick holds the six-term scheme and refuses every five-term one;
tests/test_gpu_train_accuracy.py holds the kernels to it."""
import numpy as np
import torch

BAR = 3.0
KERNEL_TERMS = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)]        # bx_product's order (csrc/train_dw.hip)
# the dx chain's unit (csrc/mlp_bf16x3_core.h): five small terms into `small`, then a0 b0 into `big`; (i, j) = (gradient piece, weight piece)
CHAIN_TERMS = [(0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)]
STEP = 16                                                               # samples per bf16 MFMA (32x32x16)
DESIGNS = ("randn", "scaled", "cancel_x", "cancel_dy")
# db's yardstick has a floor of one fp32 rounding of a partial sum as large as the normaliser sum_s |dy_si|: where the column sums cancel
# (cancel_x: rows in pairs +v, -v) an fp32 sum that happens to add each pair first is EXACT -- torch's is, a yardstick of 0 -- and any
# other order of the same fp32 additions is not.  No summation order is asked to be exact; a lost or twice-counted row is at 1 / m.
U32 = 2.0 ** -24
OLD_REL_TO_MAX_BAR = 4e-6                                               # test_dw_batch_matches_fp64_matmuls_layer_by_layer's


def _bf16(x):
    """fp32 array -> its round-to-nearest-even bf16 value, as fp32 (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def split3(x):
    """The three bf16 pieces of an fp32 array, each the round-to-nearest-even of the remainder (bx_split8 / split8): x ~ p0 + p1 + p2,
    the subtractions exact in fp32."""
    x = np.asarray(x, dtype=np.float32)
    p0 = _bf16(x)
    r = x - p0
    p1 = _bf16(r)
    p2 = _bf16(r - p1)
    return p0, p1, p2


def emulate(a, b, terms, big_small=False):
    """a^T b for a (m, n), b (m, k), contracted over the m rows in steps of 16: per step and per (i, j) of `terms` the products of piece
    i of a with piece j of b are summed in fp64 and added into an fp32 accumulator, term by term (one MFMA each).  big_small: the (0, 0)
    term has an accumulator of its own, the result is their fp32 sum (the dx chain)."""
    pa, pb = [p.astype(np.float64) for p in split3(a)], [p.astype(np.float64) for p in split3(b)]
    acc = np.zeros((a.shape[1], b.shape[1]), dtype=np.float32)
    big = np.zeros_like(acc)
    for s in range(0, a.shape[0], STEP):
        for i, j in terms:
            step64 = pa[i][s:s + STEP].T @ pb[j][s:s + STEP]
            if big_small and (i, j) == (0, 0):
                big = (big.astype(np.float64) + step64).astype(np.float32)
            else:
                acc = (acc.astype(np.float64) + step64).astype(np.float32)
    return (big + acc).astype(np.float32) if big_small else acc


def five_term_variants(terms=KERNEL_TERMS):
    """[(the dropped term, the other five)]"""
    return [(t, [u for u in terms if u != t]) for t in terms]


def want64(dy, x):
    return np.asarray(dy, dtype=np.float64).T @ np.asarray(x, dtype=np.float64)


def worst_ratio(err, den):
    """max err / den; an entry whose normaliser is zero must be exact."""
    out = np.zeros_like(err)
    np.divide(err, den, out=out, where=den > 0)
    out[(den == 0) & (err != 0)] = np.inf
    return float(out.max()) if out.size else 0.0


def componentwise(got, dy, x, base=None):
    """max_ij |got_ij - want64_ij| / sum_s |dy_si x_sj|, want64 = the fp64 product of the fp32 inputs.  base: got was accumulated onto
    it -- one more term of the sum, in want64 and in the normaliser."""
    dy64, x64 = np.asarray(dy, dtype=np.float64), np.asarray(x, dtype=np.float64)
    want, den = dy64.T @ x64, np.abs(dy64).T @ np.abs(x64)
    if base is not None:
        want, den = want + np.float64(base), den + np.abs(np.float64(base))
    return worst_ratio(np.abs(np.asarray(got, dtype=np.float64) - want), den)


def componentwise_sum(got, dy, base=None):
    """The same measure for db = the column sums of dy: normaliser sum_s |dy_si|."""
    dy64 = np.asarray(dy, dtype=np.float64)
    want, den = dy64.sum(0), np.abs(dy64).sum(0)
    if base is not None:
        want, den = want + np.float64(base), den + np.abs(np.float64(base))
    return worst_ratio(np.abs(np.asarray(got, dtype=np.float64).reshape(-1) - want), den)


def rel_to_max(got, want):
    """The suite's existing measure: max |got - want| / max |want|."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(float(np.abs(want).max()), 1e-300))


def fp32_matmul(dy, x):
    """The yardstick's product: torch's fp32 CPU matmul dy^T x."""
    return (torch.from_numpy(np.ascontiguousarray(dy, dtype=np.float32)).T @ torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).numpy()


def fp32_column_sums(dy):
    """db's yardstick: the same fp32 CPU matmul, dy^T against a column of ones."""
    return fp32_matmul(dy, np.ones((np.asarray(dy).shape[0], 1), dtype=np.float32)).reshape(-1)


def _pairs(rs, m, n):
    """(m, n): rows in pairs +v, -v (an odd m's last row stands alone)."""
    v = rs.standard_normal(((m + 1) // 2, n)).astype(np.float32)
    out = np.empty((2 * v.shape[0], n), dtype=np.float32)
    out[0::2], out[1::2] = v, -v
    return np.ascontiguousarray(out[:m])


def _near_one(rs, m, n):
    return (1.0 + 2.0 ** -8 * rs.uniform(-1.0, 1.0, (m, n))).astype(np.float32)


def design(name, m, n, k, seed=0):
    """-> dy (m, n), x (m, k), fp32, seeded.
    randn: dy ~ N(0, 1), x = relu(N(0, 1)); scaled: randn with every column of dy and of x times its own power of two in 2^-20 .. 2^20;
    cancel_x: rows of dy in pairs +v, -v and x = fp32(1 + 2^-8 u), u ~ U(-1, 1): the bf16-exact part of x cancels, the result is made of
    x's second and third pieces; cancel_dy: the mirror image (rows of x in pairs, dy near one) -- cancel_x cannot see a missing a2 b0."""
    rs = np.random.RandomState(1000003 * DESIGNS.index(name) + 7919 * m + 31 * n + k + seed)
    if name in ("randn", "scaled"):
        dy = rs.standard_normal((m, n)).astype(np.float32)
        x = np.maximum(rs.standard_normal((m, k)), 0.0).astype(np.float32)
        if name == "scaled":
            dy = dy * (2.0 ** rs.randint(-20, 21, n)).astype(np.float32)
            x = x * (2.0 ** rs.randint(-20, 21, k)).astype(np.float32)
        return dy, x
    if name == "cancel_x":
        return _pairs(rs, m, n), _near_one(rs, m, k)
    if name == "cancel_dy":
        return _near_one(rs, m, n), _pairs(rs, m, k)
    raise ValueError(name)


CHAIN_DESIGNS = ("randn", "cancel_w", "cancel_dy")
OLD_CHAIN_BAR = 2e-5                                                    # test_split_bf16_backward_chain_matches_the_exact_f32_chain's


def chain_layer_case(name="randn", M=128, seed=0):
    """One layer of the dx chain, d x = dy W contracting over 256: -> dy (M, 256), W (256, 256), fp32, seeded.
    randn: dy ~ N(0, 1), W ~ N(0, 1) / 16; cancel_w: along the contraction dy comes in pairs +v, -v and W = fp32(1 + 2^-8 u): the
    bf16-exact part of the (pre-split) weights cancels; cancel_dy: the mirror image, W's rows in pairs and the gradient near one."""
    rs = np.random.RandomState(4242 + 1009 * CHAIN_DESIGNS.index(name) + M + seed)
    if name == "randn":
        return rs.standard_normal((M, 256)).astype(np.float32), (rs.standard_normal((256, 256)) / 16.0).astype(np.float32)
    if name == "cancel_w":
        return np.ascontiguousarray(_pairs(rs, 256, M).T), _near_one(rs, 256, 256)
    if name == "cancel_dy":
        return np.ascontiguousarray(_near_one(rs, 256, M).T), (_pairs(rs, 256, 256) / 16.0).astype(np.float32)
    raise ValueError(name)


def emulate_chain_layer(dy, W, terms):
    """dy W with the gradient split on the fly, the weights pre-split, big + small accumulators: (M, 256)."""
    return emulate(np.ascontiguousarray(dy.T), W, terms, big_small=True)


def f32_chain(a, b, c, c_first, k=2):
    """a (M, D) @ b (D, N) + c as an f32 MFMA chain of K = k steps (each step's products summed exactly, the running sum rounded to
    fp32): c as the chain's C operand (c_first) or added behind the product.  What the exact-f32 kernels do at rgb_net.1 (c = the ray's
    row of the bias table) and at d act6 (c = the density head's rank-1 term)."""
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    acc = np.array(c, dtype=np.float32, copy=True) if c_first else np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    for s in range(0, a.shape[1], k):
        acc = (acc.astype(np.float64) + a64[:, s:s + k] @ b64[s:s + k]).astype(np.float32)
    return acc if c_first else (acc + np.asarray(c, dtype=np.float32)).astype(np.float32)


def dominant_term_case(depth, M=703, N=256, ratio=12.0, seed=0):
    """A product of `depth` terms beside a term `ratio` x its size: -> a (M, depth), b (depth, N), c (M, N), fp32, seeded."""
    rs = np.random.RandomState(777 + depth + seed)
    a = (rs.standard_normal((M, depth)) * (rs.uniform(size=(M, depth)) < 0.5)).astype(np.float32)
    b = (rs.standard_normal((depth, N)) / np.sqrt(depth)).astype(np.float32)
    c = (ratio * rs.standard_normal((M, 1)) * rs.standard_normal((1, N))).astype(np.float32)
    return a, b, c
