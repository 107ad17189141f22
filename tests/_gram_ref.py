"""CPU reference, emulation, inputs and checks of the Gram stage's tests
(tests/test_gram_ref_cpu.py, tests/test_gpu_gram.py).  Plain numpy and torch.

The Gram kernels of csrc/hip/block_gram.hpp and block_quad.hpp write, for
every slab (a pair's cross or full Gram, one of a quad's six cross Grams) and
every row chunk c = rows [c rows, min(m_pad, (c + 1) rows)), the product
A_L^T A_R of the slab's left and right columns over that chunk's rows alone:
(P, nchunk, W, W) cross slabs, (P, nchunk, 2W, 2W) full slabs of [A_bi A_bj],
(3P, nchunk, 64, 64) quad slabs -- the pairs (a, c), (b, d) of every quad,
then per quad C_ad, C_bc, C_ab, C_cd.

Reference: the chunk products in numpy.longdouble from the data rounded once
to the data type.  Emulation in the data precision:
  fp32 / fp64   every 32-row slab of a chunk accumulated in the data type one
                row at a time (product rounded, sum rounded: the textbook loop,
                the same on every host), the slabs' sums added in the data
                type in row order.  The kernels add two (fp32) or four (fp64)
                rows per MFMA into four waves' accumulators and add those: as
                many roundings, in another order;
  quad          the data split into NP round-to-nearest-even bf16 parts, the
                products of order < NP of every 32-row slab (one MFMA deep:
                exact, then rounded to fp32) added in fp32, the leading product
                in one accumulator, the others, small first, in a second, the
                two added once at the end (gram_quad_kernel's order).
Measure of a result C: max over slabs, chunks and entries of
    |C - C_ref| / (|A_L|^T |A_R|)
where the denominator is not zero; where it is zero C must be exactly zero,
and C must hold no NaN (else the measure is inf).  Never after summing the
chunks.  A kernel passes when its measure is at most _apply_ref.RATIO_MAX
times the emulation's on the same inputs.

The kinds 'ints' and 'parts' have exact answers instead (check()).
"""
import functools

import numpy as np
import torch

from _apply_ref import RATIO_MAX, split_bf16

SLAB_ROWS = 32
PAD = 128                                   # ld = m_pad + PAD, those columns NaN
SHAPES = [(100, 128, 128), (256, 256, 256), (600, 640, 256), (384, 384, 128)]  # m, m_pad, rows
PAIRS = [[0, 5], [3, 1], [2, 4]]            # 7 blocks; block 6 holds NaN
QUADS = [(5, 0, 3, 6), (2, 7, 1, 4)]        # 9 blocks; block 8 holds NaN
KINDS = ("graded", "late", "zeros")         # checked by measure; 'ints', 'parts' exactly


def gamma_rows(dtype, rows):
    """gamma_n = n u / (1 - n u) of a sum of n = rows products in dtype."""
    u = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
    return rows * u / (1 - rows * u)


def quad_pairs(quads):
    """The pair list of quads (a, b, c, d): (a, c), (b, d) per quad."""
    return [p for a, b, c, d in quads for p in ([a, c], [b, d])]


# ------------------------------------------------------------------ inputs
def _graded(ncols, m, g):
    x = torch.rand(ncols, m, generator=g, dtype=torch.float64) - 0.4
    x = x / x.norm(dim=1, keepdim=True)
    s = torch.logspace(-3, 3, ncols, dtype=torch.float64)[torch.randperm(ncols, generator=g)]
    return x * s[:, None]


def _late(ncols, W, groups, m, g):
    """Every group of blocks (a pair, a quad) shares min(m, its columns)
    orthonormal directions, dealt to its blocks in turn (a block's remaining
    columns are zero: a rank-deficient matrix late in a solve); every column
    then gets 1e-6 of a random mix of the OTHER blocks' directions, so blocks
    stay orthogonal inside to 1e-12 and couple to about 1e-6 of their norms;
    column norms logspace(-3, 3), shuffled."""
    x = torch.zeros(ncols, m, dtype=torch.float64)
    for grp in groups:
        n = len(grp) * W
        r = min(m, n)
        u, _ = torch.linalg.qr(torch.randn(m, r, generator=g, dtype=torch.float64))
        owner = torch.arange(r) % len(grp)                  # direction k belongs to block k % len
        for k, b in enumerate(grp):
            mine = u[:, owner == k]                         # (m, nk)
            nk = mine.shape[1]
            mix = torch.randn(r, nk, generator=g, dtype=torch.float64) / r ** 0.5
            mix[owner == k] = 0.0
            x[b * W:b * W + nk] = (mine + 1e-6 * (u @ mix)).t()
    s = torch.logspace(-3, 3, ncols, dtype=torch.float64)[torch.randperm(ncols, generator=g)]
    return x * s[:, None]


def make_input(kind, dtype, W, nb, groups, m, m_pad, seed):
    """At (nb W, m_pad + PAD) in dtype: the kind's data in rows (At's columns)
    [0, m), built in fp64 and rounded once; zeros in [m, m_pad); NaN in
    [m_pad, ld) and in the whole of block nb - 1, which no group names."""
    g = torch.Generator().manual_seed(seed)
    ncols = nb * W
    if kind in ("graded", "zeros"):
        x = _graded(ncols, m, g)
        if kind == "zeros":  # ragged column counts, and a block that is all padding
            g0, gl = groups[0], groups[-1]
            x[g0[0] * W + W - 5:(g0[0] + 1) * W] = 0.0
            x[g0[-1] * W + W - 3:(g0[-1] + 1) * W] = 0.0
            x[gl[1] * W:(gl[1] + 1) * W] = 0.0
    elif kind == "late":
        x = _late(ncols, W, groups, m, g)
    elif kind == "ints":
        x = torch.randint(-7, 8, (ncols, m), generator=g).double()
    elif kind == "parts":
        k = torch.randint(1, 4, (ncols, m), generator=g).double()
        x = k * (1 + 2.0 ** -9 + 2.0 ** -18)
    else:
        raise ValueError(kind)
    At = torch.full((ncols, m_pad + PAD), float("nan"), dtype=dtype)
    At[:, :m_pad] = 0.0
    At[:, :m] = x.to(dtype)
    At[(nb - 1) * W:] = float("nan")
    return At


# ------------------------------------------------------------------ slabs
def slab_columns(pairs, W, mode):
    """(L, R): the left and right column indices (S, NL), (S, NR) of every slab
    in the kernels' order.  mode 'cross', 'full' or 'quad'."""
    blk = lambda b: torch.arange(W) + b * W  # noqa: E731
    if mode == "cross":
        lr = [(blk(i), blk(j)) for i, j in pairs]
    elif mode == "full":
        lr = [(torch.cat([blk(i), blk(j)]),) * 2 for i, j in pairs]
    else:
        lr = [(blk(i), blk(j)) for i, j in pairs]
        for q in range(len(pairs) // 2):
            (a, c), (b, d) = pairs[2 * q], pairs[2 * q + 1]
            lr += [(blk(a), blk(d)), (blk(b), blk(c)), (blk(a), blk(b)), (blk(c), blk(d))]
    return torch.stack([x for x, _ in lr]), torch.stack([y for _, y in lr])


def chunks(m_pad, rows):
    return [(r0, min(m_pad, r0 + rows)) for r0 in range(0, m_pad, rows)]


def _products(A, L, R, m_pad, rows):
    """(S, nchunk, NL, NR) chunk products of the numpy matrix A (ncols, >= m_pad)."""
    out = np.zeros((L.shape[0], len(chunks(m_pad, rows)), L.shape[1], R.shape[1]), dtype=A.dtype)
    for s in range(L.shape[0]):
        xl, xr = A[L[s].numpy()], A[R[s].numpy()]
        for c, (r0, r1) in enumerate(chunks(m_pad, rows)):
            out[s, c] = xl[:, r0:r1] @ xr[:, r0:r1].T
    return out


def reference(At, L, R, m_pad, rows):
    """The chunk products in numpy.longdouble."""
    assert np.finfo(np.longdouble).nmant >= 63, "needs an 80-bit long double"
    return _products(At.numpy().astype(np.longdouble), L, R, m_pad, rows)


def denominator(At, L, R, m_pad, rows):
    """|A_L|^T |A_R| per chunk (fp64)."""
    return _products(np.abs(At.numpy().astype(np.float64)), L, R, m_pad, rows)


# --------------------------------------------------------------- emulation
def emulate_plain(At, L, R, m_pad, rows, skip_slab=None, over_read=False):
    """The fp32 / fp64 Grams in At's precision (see the module docstring).
    Wrong variants, for the tests of the checks: skip_slab = (chunk, k) leaves
    the chunk's k-th 32-row slab out; over_read adds row m_pad to the last chunk."""
    A = At.numpy()
    xl, xr = A[L.numpy()], A[R.numpy()]                     # (S, N, ld)
    ch = chunks(m_pad, rows)
    out = np.zeros((L.shape[0], len(ch), L.shape[1], R.shape[1]), dtype=A.dtype)
    for c, (r0, r1) in enumerate(ch):
        acc = np.zeros(out.shape[:1] + out.shape[2:], dtype=A.dtype)
        for k, s0 in enumerate(range(r0, r1, SLAB_ROWS)):
            if skip_slab == (c, k):
                continue
            last = over_read and s0 + SLAB_ROWS == m_pad
            sl = np.zeros_like(acc)
            for r in range(s0, min(r1, s0 + SLAB_ROWS) + (1 if last else 0)):
                sl = sl + xl[:, :, r, None] * xr[:, None, :, r]
            acc = acc + sl
        out[:, c] = acc
    return torch.from_numpy(out)


def kept_products(np_):
    """(a, b): part a of the left operand times part b of the right, in
    gram_quad_kernel's order: orders np_ - 1 .. 1, then the leading (0, 0)."""
    return [(a, o - a) for o in range(np_ - 1, 0, -1) for a in range(o + 1)] + [(0, 0)]


def emulate_quad(At, L, R, m_pad, rows, np_, drop=None):
    """The split-bf16 Grams of gram_quad_kernel (see the module docstring);
    ``drop`` = (a, b) leaves that product class out (a wrong variant)."""
    parts = [p.double() for p in split_bf16(At[:, :m_pad], np_)]
    pl, pr = [p[L] for p in parts], [p[R] for p in parts]   # (S, 64, m_pad)
    ch = chunks(m_pad, rows)
    out = torch.zeros(L.shape[0], len(ch), L.shape[1], R.shape[1])
    for c, (r0, r1) in enumerate(ch):
        acc = torch.zeros(L.shape[0], L.shape[1], R.shape[1])
        lo = torch.zeros_like(acc)
        for s0 in range(r0, r1, SLAB_ROWS):
            rs = slice(s0, s0 + SLAB_ROWS)
            for a, b in kept_products(np_):
                if (a, b) == drop:
                    continue
                prod = (pl[a][:, :, rs] @ pr[b][:, :, rs].transpose(1, 2)).float()
                if (a, b) == (0, 0):
                    acc = acc + prod
                else:
                    lo = lo + prod
        out[:, c] = acc + lo
    return out


def exact_parts_sums(At, L, R, m_pad, rows, np_, drop=None):
    """Kind 'parts': the leading product's sum and the other kept products'
    sum per chunk, each exact in fp64 (integers up to 5760; multiples of 2^-18
    below 32 -- tests/test_gram_ref_cpu.py checks both)."""
    parts = [torch.nan_to_num(p.double()) for p in split_bf16(At, np_)]
    lead = torch.zeros(L.shape[0], len(chunks(m_pad, rows)), L.shape[1], R.shape[1],
                       dtype=torch.float64)
    rest = torch.zeros_like(lead)
    for c, (r0, r1) in enumerate(chunks(m_pad, rows)):
        for a, b in kept_products(np_):
            if (a, b) == drop:
                continue
            prod = parts[a][L][:, :, r0:r1] @ parts[b][R][:, :, r0:r1].transpose(1, 2)
            if (a, b) == (0, 0):
                lead[:, c] += prod
            else:
                rest[:, c] += prod
    return lead, rest


# ------------------------------------------------------------------ checks
def measure(C, ref, den):
    """See the module docstring.  C torch (S, nchunk, NL, NR), ref longdouble,
    den fp64.  inf: a NaN or infinity in C, or a non-zero where den is zero."""
    c = C.numpy().astype(np.longdouble)
    if not np.isfinite(C.numpy()).all():
        return float("inf")
    pos = den > 0
    if (c[~pos] != 0).any():
        return float("inf")
    if not pos.any():
        return 0.0
    return float((np.abs(c - ref)[pos] / den[pos]).max())


def ulp32(x):
    """The fp32 unit in the last place at the fp64 values x > 0."""
    return torch.ldexp(torch.ones_like(x), torch.floor(torch.log2(x)).int() - 23)


def mirrored(C, W):
    """Full slabs: the two off-diagonal quadrants are transposes, bit for bit."""
    return torch.equal(C[..., :W, W:], C[..., W:, :W].transpose(-1, -2))


def check(case, C, np_=None):
    """What a GPU test asserts of the kernel's slabs C (CPU tensor) on a case
    of pair_case / quad_case: a list of failures, empty when C passes, and the
    figures (measure, the emulation's, their ratio) for the record."""
    kind, bad, fig = case["kind"], [], {}
    if tuple(C.shape) != tuple(case["ref"].shape):
        return [f"shape {tuple(C.shape)} != {tuple(case['ref'].shape)}"], fig
    if case["mode"] == "full" and not mirrored(C, case["W"]):
        bad.append("off-diagonal quadrants are not transposes of each other")
    if kind == "ints":
        ref = torch.from_numpy(case["ref"].astype(np.float64)).to(C.dtype)
        fig["differ"] = int((C != ref).sum())  # a NaN differs
        it = torch.int32 if C.dtype == torch.float32 else torch.int64
        fig["bits_differ"] = int((C.view(it) != (ref + 0.0).view(it)).sum())  # also a -0 for a +0
        if fig["differ"] or fig["bits_differ"]:
            bad.append(f"ints: {fig['differ']} entries differ from the exact product, "
                       f"{fig['bits_differ']} bit patterns")
    elif kind == "parts":
        lead, rest = exact_parts_sums(case["At"], case["L"], case["R"], case["m_pad"],
                                      case["rows"], np_)
        s = lead + rest
        err = ((C.double() - s).abs() / ulp32(s)).nan_to_num(nan=float("inf"))
        fig["ulps"] = float(err.max())
        if not fig["ulps"] <= 1.0:
            bad.append(f"parts: {fig['ulps']:.1f} ulp from the exact sum of the kept products")
    else:
        emu = case["emu"] if np_ is None else case["emu", np_]
        fig["e_ref"] = measure(emu, case["ref"], case["den"])
        fig["e"] = measure(C, case["ref"], case["den"])
        fig["ratio"] = fig["e"] / fig["e_ref"] if fig["e_ref"] > 0 else \
            (0.0 if fig["e"] == 0 else float("inf"))
        if not fig["e"] <= RATIO_MAX * fig["e_ref"]:
            bad.append(f"measure {fig['e']:.3e} > {RATIO_MAX} x {fig['e_ref']:.3e} (emulation)")
    return bad, fig


# ------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def _pair_full(kind, dtype, W, shape):
    """The full-Gram case of (kind, dtype, W, SHAPES[shape]); the cross case is
    its upper right quadrant (the same numbers: the emulation's order is the
    same for both)."""
    m, m_pad, rows = SHAPES[shape]
    seed = 1000 * shape + 10 * W + (1 if dtype == torch.float64 else 0) + 7 * KINDS_ALL.index(kind)
    At = make_input(kind, dtype, W, 7, PAIRS, m, m_pad, seed)
    L, R = slab_columns(PAIRS, W, "full")
    return {"At": At, "ref": reference(At, L, R, m_pad, rows),
            "den": denominator(At, L, R, m_pad, rows),
            "emu": emulate_plain(At, L, R, m_pad, rows)}


KINDS_ALL = KINDS + ("ints", "parts")


def pair_case(kind, dtype, W, shape, mode):
    """A cross or full Gram case: At, the pairs, slab columns L, R, the
    reference, the denominators and the emulation.  Cached; do not write to it."""
    f = _pair_full(kind, dtype, W, shape)
    m, m_pad, rows = SHAPES[shape]
    L, R = slab_columns(PAIRS, W, mode)
    cut = (lambda x: x[:, :, :W, W:]) if mode == "cross" else (lambda x: x)
    return {"kind": kind, "mode": mode, "W": W, "m_pad": m_pad, "rows": rows, "At": f["At"],
            "pairs": PAIRS, "L": L, "R": R, "ref": np.ascontiguousarray(cut(f["ref"])),
            "den": np.ascontiguousarray(cut(f["den"])), "emu": cut(f["emu"]).contiguous()}


@functools.lru_cache(maxsize=None)
def quad_case(kind, nquads, shape):
    """A quad Gram case of QUADS[:nquads] (9 blocks, fp32, W = 64), with the
    emulations on 3 and 2 parts under the keys ('emu', 3), ('emu', 2) (not for
    the exact kinds).  Cached; do not write to it."""
    m, m_pad, rows = SHAPES[shape]
    quads, W = QUADS[:nquads], 64
    pairs = quad_pairs(quads)
    At = make_input(kind, torch.float32, W, 9, [list(q) for q in quads], m, m_pad,
                    5000 + 100 * shape + 10 * nquads + KINDS_ALL.index(kind))
    L, R = slab_columns(pairs, W, "quad")
    case = {"kind": kind, "mode": "quad", "W": W, "m_pad": m_pad, "rows": rows, "At": At,
            "pairs": pairs, "L": L, "R": R, "ref": reference(At, L, R, m_pad, rows),
            "den": denominator(At, L, R, m_pad, rows)}
    if kind in KINDS:
        for np_ in (3, 2):
            case["emu", np_] = emulate_quad(At, L, R, m_pad, rows, np_)
    return case
