"""Inputs of tests/test_gpu_apply_sparse.py: quad transforms T that leave
columns and blocks of [a b c d] unchanged, what each of them claims, and the
work counter the quad apply must report for them.  Plain torch, CPU.

The quad apply (csrc/hip/block_quad.hpp apply_quad_ts_kernel, SPARSE) decides from
the values of T - I alone: a column whose column of T - I is zero is not
stored; a wave (32 columns) none of whose columns change runs no product; a
32-row k block that is zero in a wave's slice is skipped there; a wave whose
columns neither change nor feed a product (their rows of T - I are zero) does
not load them.
"""
import math

import torch

import _apply_ref as R

PAIR_BLOCKS = ((0, 2), (1, 3), (0, 3), (1, 2))  # (a,c), (b,d) of T1; (a,d), (b,c) of T2
SUBSETS = list(range(1, 16))                    # bit k: pair k of PAIR_BLOCKS rotated


def _place(t, blocks, q):
    idx = torch.cat([torch.arange(64) + 64 * b for b in blocks])
    t[idx[:, None], idx[None, :]] = q


def subset_t(seed, subset):
    """T = T1 T2 as _apply_ref.dense_quad_t, the pair transforms outside
    ``subset`` the identity (fp64)."""
    ts = [torch.eye(R.QN, dtype=torch.float64) for _ in range(2)]
    for k, blocks in enumerate(PAIR_BLOCKS):
        if subset >> k & 1:
            _place(ts[k // 2], blocks, R.random_orthogonal(128, seed + k))
    return ts[0] @ ts[1]


def subset_changed_blocks(subset):
    """Blocks of [a b c d] some rotated pair of ``subset`` contains."""
    return sorted({b for k, bl in enumerate(PAIR_BLOCKS) if subset >> k & 1 for b in bl})


def givens_t(seed, nrot):
    """T = T1 T2, every pair transform the identity times ``nrot`` random
    plane rotations (angles of magnitude 0.01 .. 0.3), in fp64.  Returns T and
    the sorted columns some rotation touches."""
    g = torch.Generator().manual_seed(seed)
    ts = [torch.eye(R.QN, dtype=torch.float64) for _ in range(2)]
    touched = set()
    for k, blocks in enumerate(PAIR_BLOCKS):
        idx = torch.cat([torch.arange(64) + 64 * b for b in blocks])
        for _ in range(nrot):
            i, j = (int(v) for v in idx[torch.randperm(128, generator=g)[:2]])
            th = float(0.01 + 0.29 * torch.rand(1, generator=g)) * (1 if torch.rand(1, generator=g) < 0.5 else -1)
            rot = torch.eye(R.QN, dtype=torch.float64)
            rot[i, i] = rot[j, j] = math.cos(th)
            rot[i, j], rot[j, i] = math.sin(th), -math.sin(th)
            ts[k // 2] = ts[k // 2] @ rot
            touched |= {i, j}
    return ts[0] @ ts[1], sorted(touched)


def zero_columns_keep_rows(seed, cols):
    """Dense synthetic T - I (not orthogonal) whose columns ``cols`` are zero
    while their rows are not: those data columns stay but feed the others."""
    tm = R.synthetic_tm(seed, R.MASK_MAGS[0])
    tm[:, cols] = 0.0
    return tm


def zero_rows_keep_columns(seed, rows):
    """Dense synthetic T - I whose rows ``rows`` are zero while their columns
    are not: those data columns change but feed nobody."""
    tm = R.synthetic_tm(seed, R.MASK_MAGS[0])
    tm[rows, :] = 0.0
    return tm


def steady_tm(seed):
    """For the counted waits: waves 1, 4 and 5 load and split without storing
    (their 32 columns of T - I zero, their rows not), wave 2 stores half of
    its store instructions (columns 16 cs + e + 4 g with e < 2 only), wave 6
    one column, the others everything."""
    tm = R.synthetic_tm(seed, R.MASK_MAGS[0])
    for w in (1, 4, 5):
        tm[:, 32 * w:32 * w + 32] = 0.0
    for c in range(32):
        if c % 4 >= 2:
            tm[:, 64 + c] = 0.0
    tm[:, 192:224] = 0.0
    tm[:, 192 + 13] = R.synthetic_tm(seed + 1, R.MASK_MAGS[0])[:, 0]
    return tm


def changed_columns(tm):
    """bool (256,): columns of T - I that hold a nonzero."""
    return (tm != 0).any(0)


def source_columns(tm):
    """bool (256,): data columns that feed a product (rows of T - I with a nonzero)."""
    return (tm != 0).any(1)


def quarter_units(tm, np_, cheap_log2=7):
    """Products of one tile of the quad with this T - I in quarters of the
    work counter's unit (one unit per cheap 128-row half of a wave's 32
    columns, two per full half: a quarter or a half per 32-row k block): a
    wave none of whose columns change adds nothing, nor does a k block that is
    zero in a wave's slice.  Derived from T alone."""
    nz = (tm != 0).view(8, 32, 8, 32).any(3).any(1)          # (k block, wave)
    cheap = R.cheap_mask(tm, cheap_log2)                     # (half, wave)
    total = 0
    for w in range(8):
        if not bool(nz[:, w].any()):
            continue
        for kb in range(8):
            if bool(nz[kb, w]):
                total += 1 if np_ == 2 or bool(cheap[kb // 4, w]) else 2
    return total


def make_case(tms, m_pad, seed):
    """A case in the form of _apply_ref.quad_case from the quads' T - I."""
    tm = torch.stack(tms)
    nq = tm.shape[0]
    blk, pairs = R.quad_blocks(nq, seed + 1)
    n = 4 * nq * 64
    return {"At": R.graded(n, m_pad, seed + 2), "Vt": R.graded(n, 128, seed + 3), "blk": blk,
            "pairs": pairs, "tm": tm, "nq": nq, "m_pad": m_pad}
