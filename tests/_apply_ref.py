"""CPU reference, emulation and inputs of the apply kernels' tests
(tests/test_apply_ref_cpu.py, tests/test_gpu_apply.py).  Plain torch.

The apply kernels of csrc/hip/block.hip compute Y = X T for a block of
columns X and a small square T.  The split-bf16 ones work in delta form,
Y = X + X (T - I): X and T - I are split into np bf16 parts by successive
round-to-nearest-even conversions, the products of total order < np are
accumulated in fp32 and the identity is added in fp32.  The quad apply keeps
only the products 00, 01, 10 in a "cheap" 128-row half of a 32-column tile of
T - I, one whose largest part 0 is <= 2^-cheap_log2.

Error measure of a result Y against the fp64 product Y64 = X T:
    max over entries of |Y - Y64| / (|X| @ |T - I| + |X|).
A kernel passes when its measure is at most RATIO_MAX times that of this
file's emulation of the same arithmetic on the same inputs (e_ref): the
factor covers the MFMA's different accumulation order and its internal
accumulation, which is not round-to-nearest.
"""
import numpy as np
import torch

RATIO_MAX = 4.0
QN = 256  # columns of a quad: four 64-column blocks [a b c d]


# ------------------------------------------------------------------ inputs
def graded(ncols, rows, seed):
    """At-layout (ncols, rows) fp32 data: rand - 0.3 with column norms graded
    over logspace(-2, 2)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(ncols, rows, generator=g, dtype=torch.float64) - 0.3
    return (x * torch.logspace(-2, 2, ncols, dtype=torch.float64)[:, None]).float()


def random_orthogonal(n, seed):
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))
    return q


def near_identity(n, seed, eps=1e-3):
    """I + eps * skew, re-orthogonalised in fp64."""
    g = torch.Generator().manual_seed(seed)
    s = torch.rand(n, n, generator=g, dtype=torch.float64) - 0.5
    q, r = torch.linalg.qr(torch.eye(n, dtype=torch.float64) + eps * (s - s.t()))
    return q * torch.sign(torch.diagonal(r))[None, :]


def quad_blocks(nq, seed):
    """A block permutation and the 2 nq pairs in quad order: quad q is the
    blocks perm[4q .. 4q+3] = (a, b, c, d), its pairs (a, c), (b, d)."""
    g = torch.Generator().manual_seed(seed)
    blk = torch.randperm(4 * nq, generator=g).view(nq, 4)
    pairs = torch.stack([blk[:, [0, 2]], blk[:, [1, 3]]], 1).reshape(2 * nq, 2)
    return blk, pairs.to(torch.int32)


def quad_cols(blk):
    """(nq, 256) column indices of every quad in [a b c d] order."""
    return (blk[:, :, None] * 64 + torch.arange(64)).reshape(blk.shape[0], QN)


def synthetic_tm(seed, mag):
    """A 256 x 256 T - I with random signs and magnitudes mag[h][ct] * [0.5, 1]
    in the 128-row half h of the 32-column tile ct (fp32 values; T need not be
    orthogonal: the apply is a product)."""
    g = torch.Generator().manual_seed(seed)
    u = 0.5 + 0.5 * torch.rand(QN, QN, generator=g, dtype=torch.float64)
    sgn = torch.where(torch.rand(QN, QN, generator=g) < 0.5, -1.0, 1.0).double()
    m = torch.as_tensor(mag, dtype=torch.float64)  # (2, 8)
    return (u * sgn * m.repeat_interleave(128, 0).repeat_interleave(32, 1)).float()


BIG, SMALL = 0.1, 2.0 ** -8
MASK_MAGS = {  # cheap mask of every wave -> magnitudes of the (upper, lower) k half
    0: [[BIG] * 8, [BIG] * 8],
    1: [[SMALL] * 8, [BIG] * 8],
    2: [[BIG] * 8, [SMALL] * 8],
    3: [[SMALL] * 8, [SMALL] * 8],
    # the late-sweep pattern: columns of a, b cheap in the upper half (rows of
    # a, b), those of c, d in the lower half -- masks 1 and 2 in one workgroup
    "mixed": [[SMALL] * 4 + [BIG] * 4, [BIG] * 4 + [SMALL] * 4],
}


def threshold_tm(seed):
    """All of T - I at 2^-8 or below (mask 3 everywhere), except: in tile 2 the
    upper half's largest part 0 is exactly 2^-7 (still cheap), in tile 5 the
    lower half's is the next bf16 above 2^-7 (not cheap: mask 1 there)."""
    tm = synthetic_tm(seed, MASK_MAGS[3])
    tm[17, 2 * 32 + 5] = 2.0 ** -7
    tm[128 + 40, 5 * 32 + 21] = -(2.0 ** -7) * (1 + 2.0 ** -7)
    return tm


def tie_diagonal_tm(seed):
    """Near-identity T for the 2-part split: tiny off-diagonal entries and a
    diagonal T_cc - 1 = +-2^-9 (1 + 2^-8 - 2^-12).  T - I splits to 2^-18
    relative; 1 + that value, split in two parts, is off by 2^-17 absolute."""
    g = torch.Generator().manual_seed(seed)
    tm = (torch.rand(QN, QN, generator=g, dtype=torch.float64) - 0.5) * 2.0 ** -15
    d = 2.0 ** -9 * (1 + 2.0 ** -8 - 2.0 ** -12)
    sgn = torch.where(torch.rand(QN, generator=g) < 0.5, -1.0, 1.0).double()
    tm[torch.arange(QN), torch.arange(QN)] = d * sgn
    return tm.float()


def dense_quad_t(seed):
    """T = T1 T2 of a quad step in fp64: T1 = Q_ac on the rows and columns of
    (a, c) and Q_bd on (b, d), T2 = Q_ad on (a, d) and Q_bc on (b, c), each a
    random 128 x 128 orthogonal matrix ([a b c d] order, 64 columns each)."""
    ia, ib, ic, id_ = (torch.arange(64) + 64 * k for k in range(4))

    def place(x, y, q1, x2, y2, q2):
        t = torch.zeros(QN, QN, dtype=torch.float64)
        i1, i2 = torch.cat([x, y]), torch.cat([x2, y2])
        t[i1[:, None], i1[None, :]] = q1
        t[i2[:, None], i2[None, :]] = q2
        return t

    q = [random_orthogonal(128, seed + k) for k in range(4)]
    return place(ia, ic, q[0], ib, id_, q[1]) @ place(ia, id_, q[2], ib, ic, q[3])


# --------------------------------------------------------------- emulation
def split_bf16(x, np_):
    """np_ bf16 parts of the fp32 tensor x by successive round-to-nearest-even
    conversions (block_apply.hpp split_bf16)."""
    r = x.float().clone()
    parts = []
    for i in range(np_):
        p = r.to(torch.bfloat16)
        parts.append(p)
        if i + 1 < np_:
            r = r - p.float()
    return parts


def cheap_mask(tm, cheap_log2=7):
    """(K / 128, N / 32) bool: the 128-row half h of the 32-column tile ct of
    T - I is cheap when the largest |part 0| in it is <= 2^-cheap_log2."""
    p0 = tm.float().to(torch.bfloat16).float().abs()
    K, N = p0.shape
    mx = p0.view(K // 128, 128, N // 32, 32).amax(dim=(1, 3))
    return mx <= 2.0 ** -cheap_log2


def matmul_kblocked(x, t, kblock):
    """fp32 matmul of bf16-valued operands accumulated as an MFMA chain does
    it at best: every kblock-deep block of products summed exactly (fp64 holds
    it) and rounded to fp32 once, the blocks added in fp32 in k order.  (A
    library fp32 matmul adds one product at a time: at K = 256 its rounding
    noise, 5-8 x 2^-24 of |X| @ |T - I| on the graded inputs here, hid a
    first-order form used where it must not be, 0.9 x 2^-18.)"""
    acc = torch.zeros(x.shape[0], t.shape[1])
    for k in range(0, x.shape[1], kblock):
        acc = acc + (x[:, k:k + kblock].double() @ t[k:k + kblock].double()).float()
    return acc


def emulate_split_apply(X, tm, np_, cheap_halves=None, drop=None, tparts=None, kblock=32):
    """Y = X + X (T - I) as the split-bf16 applies compute it.  X (rows, K)
    fp32, tm (K, N) fp32 = T - I.  Products of total order < np_ of the bf16
    parts, each an fp32 matmul (matmul_kblocked; kblock = the MFMA's depth:
    32 in the quad apply, 16 in apply_split_kernel); in a cheap half
    (cheap_halves: (K / 128, N / 32) bool, see cheap_mask) only 00, 01, 10
    (the order-2 ones see zeros there); the order-0 product in one
    accumulator, the others, small first, in a second; the identity added in
    fp32.  ``drop`` = (i, j) leaves the product T part i x X part j out and
    ``tparts`` replaces the parts of T - I (wrong variants, for the tests of
    the bound)."""
    xs = [p.float() for p in split_bf16(X, np_)]
    ts = [p.float() for p in (tparts if tparts is not None else split_bf16(tm, np_))]
    K, N = ts[0].shape
    keep2 = torch.ones(K, N)
    if cheap_halves is not None:
        keep2 = (~cheap_halves).float().repeat_interleave(128, 0).repeat_interleave(32, 1)
    lo = torch.zeros(X.shape[0], N)
    for order in range(np_ - 1, 0, -1):
        for a in range(order + 1):
            if drop == (a, order - a):
                continue
            t = ts[a] * keep2 if order >= 2 else ts[a]
            lo = lo + matmul_kblocked(xs[order - a], t, kblock)
    acc = matmul_kblocked(xs[0], ts[0], kblock)
    return X.float() + (acc + lo)


def emulate_plain(X, T):
    """Y = X T in X's precision, one k at a time (the textbook loop: the same
    on every host, whatever its BLAS blocks)."""
    acc = torch.zeros(X.shape[0], T.shape[1], dtype=X.dtype)
    for k in range(T.shape[0]):
        acc = acc + X[:, k:k + 1] * T[k:k + 1, :]
    return acc


def product_longdouble(X, T):
    """X T in extended precision (fp64 results need a reference above fp64)."""
    assert np.finfo(np.longdouble).nmant >= 63, "needs an 80-bit long double"
    return X.numpy().astype(np.longdouble) @ T.numpy().astype(np.longdouble)


def measure(Y, Y_ref, X, tm, own=1.0):
    """max |Y - Y_ref| / (|X| @ |T - I| + own |X|); square T.  own < 1 is the
    sharper measure for a near-identity T on 2 parts: there the split's error
    is 2^-18 of |X| @ |T - I| and the output's rounding 2^-24 |X|, and own =
    2^-6 weighs the two alike, so that an error of 2^-17 |X| -- the identity
    split along with T -- stands out."""
    den = X.double().abs() @ tm.double().abs() + own * X.double().abs()
    if isinstance(Y_ref, np.ndarray):
        num = torch.from_numpy(np.abs(Y.numpy().astype(np.longdouble) - Y_ref).astype(np.float64))
    else:
        num = (Y.double() - Y_ref).abs()
    ok = den > 0
    return float((num[ok] / den[ok]).max())


# ------------------------------------------------------ quad apply operands
def pack_ts(tm, np_, kb_shift=0, swap_cs=False):
    """tm (nq, 256, 256) fp32 = T - I  ->  the quad apply's Ts (bfloat16, flat):
    part p of (T - I)[32 kb + 8 g + e][32 ct + 16 cs + i] at
    [q][kb][ct][cs][p][lane = 16 g + i][e].  kb_shift / swap_cs build the wrong
    layouts of tests/test_apply_ref_cpu.py."""
    nq = tm.shape[0]
    parts = torch.stack(split_bf16(tm, np_), 0)           # (p, q, k, c)
    x = parts.view(np_, nq, 8, 4, 8, 8, 2, 16)             # p q kb g e ct cs i
    if kb_shift:
        x = torch.roll(x, kb_shift, dims=2)
    if swap_cs:
        x = x.flip(6)
    return x.permute(1, 2, 5, 6, 0, 3, 7, 4).contiguous().view(-1)  # q kb ct cs p g i e


def unpack_ts(ts, nq, np_):
    """Inverse of pack_ts: the np_ parts, each (nq, 256, 256) bf16."""
    x = ts.view(nq, 8, 8, 2, np_, 4, 16, 8)                # q kb ct cs p g i e
    x = x.permute(4, 0, 1, 5, 7, 2, 3, 6).contiguous()     # p q kb g e ct cs i
    return list(x.view(np_, nq, QN, QN))


def tm_of(T64):
    """T - I as the Q builds form it: T rounded to fp32 first."""
    return T64.float() - torch.eye(T64.shape[-1])


# ------------------------------------------------------- quad apply cases
def quad_case(name):
    """Inputs of the quad-apply cases of tests/test_gpu_apply.py: At (ncols,
    m_pad) and Vt (ncols, 128) fp32, the block permutation and pair list, and
    T - I of every quad (nq, 256, 256) fp32."""
    nq, m_pad, seed = {"dense": (2, 256, 40), "skips": (6, 128, 50), "many": (70, 128, 60),
                       "grids": (5, 128, 70)}.get(name, (1, 128, 30))
    if name == "dense":
        tm = torch.stack([tm_of(dense_quad_t(seed + 10 * q)) for q in range(nq)])
    elif name == "threshold":
        tm = threshold_tm(seed)[None]
    elif name == "tie2":
        tm = tie_diagonal_tm(seed)[None]
    elif name in MASK_MAGS:
        tm = synthetic_tm(seed, MASK_MAGS[name])[None]
    else:  # several quads: every mask pattern in turn
        kinds = [0, 1, "mixed", 2, 3]
        tm = torch.stack([synthetic_tm(seed + q, MASK_MAGS[kinds[q % 5]]) for q in range(nq)])
    blk, pairs = quad_blocks(nq, seed + 1)
    n = 4 * nq * 64
    return {"At": graded(n, m_pad, seed + 2), "Vt": graded(n, 128, seed + 3), "blk": blk,
            "pairs": pairs, "tm": tm, "nq": nq, "m_pad": m_pad}


def quad_rows(case, q):
    """The rows the apply multiplies by T of quad q: A's and V's, (m_pad + 128, 256)."""
    cols = quad_cols(case["blk"])[q]
    return torch.cat([case["At"][cols].t(), case["Vt"][cols].t()], 0).contiguous()
