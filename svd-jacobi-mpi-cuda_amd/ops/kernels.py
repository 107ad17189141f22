"""Tensor-level entry points of the native ops.

Device (HIP) tensors go to the gfx950 kernels in ``libsvdj_hip.so`` via
ctypes on torch's current stream; CPU tensors go to ``ops.reference``.  A
device tensor never falls back to PyTorch math: a missing/failed native
library raises :class:`NativeError`.

All matrices use the transposed column-major layout of the kernels: ``At``
has shape (ncols, ld) and row c is column c of the matrix; rows are padded to
``ROW_ALIGN`` with zeros (``m_pad``).
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import torch

from . import reference as ref
from ._native import NativeError, cpu_lib, hip_check, hip_lib
from .codes import (INNER_ORDERS, MMA_CODES, MMA_MASK, STEP_CROSS, STEP_CROSS_BIP,  # noqa: F401
                    STEP_CROSS_ONLY, STEP_FULL, STEP_QUAD, STEP_QUAD_SECOND, STEPS_GRAM2,
                    STEPS_SHARED_GPU)

ROW_ALIGN = 128
SUPPORTED_BLOCK = {torch.float32: (32, 64), torch.float64: (32, 64)}
# Matrix-core modes of the block apply (csrc/hip/block.hip): native f32/f64
# MFMA (default, fp32-exact products and sums), or fp32 data on bf16 MFMA
# with a 3-way / 2-way operand split -- faster (memory-bound instead of
# MFMA-bound at W=64) but NOT fp32-accurate on every input: the bf16 MFMA's
# internal accumulation is biased when magnitudes mix (see block.hip).
# MMA_CODES and the other codes of svdj_hip.h: ops/codes.py.


def mma_code(mma: str | int, dtype: torch.dtype) -> int:
    if isinstance(mma, int):
        return mma
    if mma == "auto":
        mma = "native"
    if mma not in MMA_CODES:
        raise ValueError(f"bad mma mode {mma!r}; one of {sorted(MMA_CODES)} or 'auto'")
    if mma != "native" and dtype != torch.float32:
        raise ValueError(f"mma={mma} needs fp32 data")
    return MMA_CODES[mma]


def tol_mode_code(tol_mode) -> int:
    """0 = relative |g_pq| > tol sqrt(g_pp g_qq) (default), 1 = absolute
    |g_pq| > tol (the reference's TOLERANCE test, lib/global.cuh:9)."""
    if tol_mode in (0, 1):
        return int(tol_mode)
    table = {"relative": 0, "absolute": 1}
    if tol_mode not in table:
        raise ValueError(f"bad tol_mode {tol_mode!r}; 'relative' or 'absolute'")
    return table[tol_mode]


def dtype_code(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return 0
    if dtype == torch.float64:
        return 1
    raise TypeError(f"unsupported dtype {dtype} (fp32/fp64)")


def _stream(t: torch.Tensor):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _check_layout(At: torch.Tensor, m_pad: int):
    if At.dim() != 2 or At.stride(1) != 1:
        raise ValueError("At must be a 2-D tensor with contiguous rows (ncols, ld)")
    if m_pad % ROW_ALIGN or At.stride(0) < m_pad or At.shape[1] < m_pad:
        raise ValueError(f"m_pad={m_pad} must be a multiple of {ROW_ALIGN} and <= ld")


# ------------------------------------------------------------------ metric
METRIC_WORDS = 8  # csrc/include/svdj_stop.h SVDJ_METRIC_WORDS


def new_metric(device, groups: int | None = None) -> torch.Tensor:
    """Per-sweep stop-test state: [0] max convergence value, [1] rotated
    pairs, the negligible-column floor of the solve (block path), and for the
    block path's second-order stop test the largest effective sine of an
    applied rotation and the number of column rotations applied.  Device:
    int32[8] (csrc/include/svdj_stop.h: floor a double in [2..3], sine float
    bits in [4], count [5]); CPU: float64[5] (floor [2], sine [3], count [4]).
    ``groups``: one such row per group, (groups, 8) or (groups, 5), for
    :func:`block_steps` with ``group_blocks``."""
    shape = () if groups is None else (int(groups),)
    if torch.device(device).type == "cpu":
        return torch.zeros(*shape, 5, dtype=torch.float64)
    return torch.zeros(*shape, METRIC_WORDS, dtype=torch.int32, device=device)


def reset_metric(metric: torch.Tensor):
    """Zero the per-sweep words; the floor (set once per solve) stays."""
    metric[:2].zero_()
    if metric.device.type == "cpu":
        metric[3:].zero_()
    else:
        metric[4:].zero_()


def norm_floor(dtype: torch.dtype, m: int, dmax: float = 1.0) -> float:
    """Negligible-column floor: the block EVDs (block_evd.hpp needs_rotation) do
    not rotate pairs with a squared column norm at or below
    max(m realmin, m realmin / eps * dmax), dmax the largest squared column
    norm of the matrix.  The second term is the round-3 floor m realmin / eps
    taken relative to the matrix's scale, so c A is solved like A (LAPACK
    xGESVJ prescales A for the same reason); the first keeps columns whose
    products would be subnormal out whatever the scale."""
    fi = torch.finfo(torch.float64 if dtype == torch.float64 else torch.float32)
    return max(m * fi.tiny, m * fi.tiny / fi.eps * float(dmax))


def set_norm_floor(metric: torch.Tensor, dtype: torch.dtype, m: int, dmax: float = 1.0):
    """Store :func:`norm_floor` in the metric (once per solve)."""
    v = norm_floor(dtype, m, dmax)
    if metric.device.type == "cpu":
        metric[2] = v
    else:
        metric[2:4].view(torch.float64).fill_(v)


def read_metric(metric: torch.Tensor):
    """(max convergence value, rotations) -- synchronises for device metrics."""
    if metric.device.type == "cpu":
        return float(metric[0]), int(metric[1])
    h = metric.cpu().numpy().astype(np.int32)
    mx = struct.unpack("<f", struct.pack("<i", int(h[0])))[0]
    return mx, int(np.uint32(h[1]))


def metric_as_float_pair(metric: torch.Tensor) -> torch.Tensor:
    """Device-side (maxconv, rotations) as float64 without host sync."""
    if metric.device.type == "cpu":
        return metric[:2].clone()
    return torch.stack([metric[0:1].view(torch.float32).double()[0], metric[1].double()])


def metric_stop_values(metric: torch.Tensor) -> torch.Tensor:
    """(maxconv, max effective sine, rotated pairs, column rotations) as
    float64, device-side for device metrics (no host sync)."""
    if metric.device.type == "cpu":
        return torch.stack([metric[0], metric[3], metric[1], metric[4]]).clone()
    f = metric.view(torch.float32)
    u = metric[5:6].view(torch.int32)[0].double()
    u = torch.where(u < 0, u + 2.0 ** 32, u)  # uint32 count
    return torch.stack([f[0].double(), f[4].double(), metric[1].double(), u])


def metric_work(metric: torch.Tensor) -> torch.Tensor:
    """The quad apply's work counters of the sweep (svdj_stop.h words 6, 7),
    float64 on the metric's device without a host sync: [MFMAs issued / 24,
    32-row x 256-column tiles moved].  Zeros for CPU metrics (the CPU
    emulation has no counters)."""
    if metric.device.type == "cpu":
        return torch.zeros(2, dtype=torch.float64)
    w = metric[6:8].double()
    return torch.where(w < 0, w + 2.0 ** 32, w)


def read_stop(metric: torch.Tensor):
    """(max convergence value, max effective sine, rotated pairs, column
    rotations) -- synchronises."""
    v = metric_stop_values(metric).cpu()
    return float(v[0]), float(v[1]), int(v[2]), int(v[3])


def reset_group_metrics(metric: torch.Tensor, groups: torch.Tensor):
    """:func:`reset_metric` on the rows ``groups`` (an index tensor on the
    metric's device) of a grouped metric."""
    last = 3 if metric.device.type == "cpu" else 4
    metric[groups, :2] = 0
    metric[groups, last:] = 0


def read_group_stops(metric: torch.Tensor):
    """A grouped metric's stop-test inputs on the host: float64 arrays (groups,)
    of the largest convergence value, the largest effective sine, the rotated
    pairs and the column rotations -- one copy, synchronises."""
    if metric.device.type == "cpu":
        h = metric.numpy()
        return h[:, 0].copy(), h[:, 3].copy(), h[:, 1].copy(), h[:, 4].copy()
    h = np.ascontiguousarray(metric.cpu().numpy())
    f, u = h.view(np.float32), h.view(np.uint32)
    return (f[:, 0].astype(np.float64), f[:, 4].astype(np.float64), u[:, 1].astype(np.float64),
            u[:, 5].astype(np.float64))


STOP_RULES = {"no_rotation": 0, "second_order": 1}


def sweep_converged(mx: float, ms: float, nrot_pairs: float, nrot_cols: float, tol: float,
                    tol_mode="relative", stop_rule="second_order") -> int:
    """The block path's sweep stop test (csrc/include/svdj_stop.h, the same
    native code every engine runs): 0 continue, 1 the sweep rotated nothing,
    2 its rotations were all noise-level (second-order rule:
    nrot_cols * mx * ms <= tol / 2)."""
    rule = STOP_RULES[stop_rule] if isinstance(stop_rule, str) else int(stop_rule)
    return int(cpu_lib().svdj_sweep_converged(float(mx), float(ms), float(nrot_pairs),
                                              float(nrot_cols), float(tol),
                                              tol_mode_code(tol_mode), rule))


# --------------------------------------------------------------- utilities
def set_identity(Vt: torch.Tensor, ncols: int, col_offset: int = 0):
    if Vt.is_cuda:
        hip_check(hip_lib().svdj_set_identity(dtype_code(Vt.dtype), _ptr(Vt), Vt.shape[1],
                                              Vt.stride(0), ncols, col_offset, _stream(Vt)),
                  "set_identity")
    else:
        Vt[:ncols].zero_()
        idx = torch.arange(ncols)
        ok = idx + col_offset < Vt.shape[1]
        Vt[idx[ok], idx[ok] + col_offset] = 1


def col_norms2(At: torch.Tensor, m_pad: int, out: torch.Tensor | None = None) -> torch.Tensor:
    _check_layout(At, m_pad)
    ncols = At.shape[0]
    if out is None:
        out = torch.empty(ncols, dtype=At.dtype, device=At.device)
    if At.is_cuda:
        hip_check(hip_lib().svdj_col_norms2(dtype_code(At.dtype), _ptr(At), m_pad, At.stride(0),
                                            ncols, _ptr(out), _stream(At)), "col_norms2")
    else:
        out.copy_(ref.col_norms2(At[:, :m_pad]))
    return out


def finalize(At: torch.Tensor, m_pad: int, scale_u: bool = True) -> torch.Tensor:
    """sigma_c = ||a_c||; optionally a_c /= sigma_c (sigma 0 untouched)."""
    _check_layout(At, m_pad)
    ncols = At.shape[0]
    sigma = torch.empty(ncols, dtype=At.dtype, device=At.device)
    if At.is_cuda:
        hip_check(hip_lib().svdj_finalize(dtype_code(At.dtype), _ptr(At), m_pad, At.stride(0),
                                          ncols, _ptr(sigma), int(scale_u), _stream(At)),
                  "finalize")
    else:
        sigma.copy_(ref.finalize(At[:, :m_pad], scale_u))
    return sigma


def spin_ns(device, ns: float):
    """Enqueue a device-side wait of ``ns`` nanoseconds on the current stream
    of ``device`` (link-time model of the simulated exchange)."""
    st = C.c_void_p(torch.cuda.current_stream(torch.device(device)).cuda_stream)
    hip_check(hip_lib().svdj_spin_ns(float(ns), st), "spin_ns")


# ---------------------------------------------------------------- scalar path
def scalar_step(At, Vt, m_pad, pairs, tol, tol_mode, metric):
    """One parallel step; pairs: int32 tensor (k, 2) on At's device."""
    _check_layout(At, m_pad)
    if At.is_cuda:
        n_v = Vt.shape[1] if Vt is not None else 0
        ldv = Vt.stride(0) if Vt is not None else 0
        hip_check(hip_lib().svdj_scalar_step(
            dtype_code(At.dtype), m_pad, _ptr(At), At.stride(0), _ptr(Vt), n_v, ldv,
            _ptr(pairs), pairs.shape[0], float(tol), int(tol_mode), _ptr(metric), _stream(At)),
            "scalar_step")
    else:
        mx, nrot = ref.scalar_step(At, Vt, pairs, tol, tol_mode)
        metric[0] = max(float(metric[0]), mx)
        metric[1] += nrot


def scalar_solve(At, Vt, m_pad, sched, tol, tol_mode, max_sweeps):
    """Repeated sweeps over ``sched`` (int32 (steps, per_step, 2)) until no
    rotation.  Returns (sweeps, per-sweep max convergence value list)."""
    _check_layout(At, m_pad)
    steps, per_step = int(sched.shape[0]), int(sched.shape[1])
    if At.is_cuda:
        metric = new_metric(At.device)
        hist = (C.c_double * max(max_sweeps, 1))()
        n_v = Vt.shape[1] if Vt is not None else 0
        ldv = Vt.stride(0) if Vt is not None else 0
        sweeps = hip_check(hip_lib().svdj_scalar_solve(
            dtype_code(At.dtype), m_pad, _ptr(At), At.stride(0), _ptr(Vt), n_v, ldv,
            _ptr(sched), steps, per_step, float(tol), int(tol_mode), int(max_sweeps),
            _ptr(metric), hist, _stream(At)), "scalar_solve")
        return sweeps, [hist[i] for i in range(sweeps)]
    hist = []
    for _ in range(max_sweeps):
        metric = new_metric("cpu")
        for s in range(steps):
            scalar_step(At, Vt, m_pad, sched[s], tol, tol_mode, metric)
        mx, nrot = read_metric(metric)
        hist.append(mx)
        if nrot == 0:
            break
    return len(hist), hist


# ----------------------------------------------------------------- block path
_WS_CACHE: dict = {}


def block_workspace(dtype, W, P, m_pad, device, slot: int = 0, pool: dict | None = None,
                    quad: bool = False) -> torch.Tensor:
    """Per (device, shape, slot, quad) workspace; concurrent chains use
    distinct slots.  ``pool`` is the caller's own cache (a solver instance owns
    one, so solvers running concurrently -- e.g. several ranks in one process
    -- never share scratch); None uses the module-wide cache.  ``quad``: the
    step list holds quad steps (their scratch is sized only then)."""
    nbytes = int(hip_lib().svdj_block_workspace_bytes(dtype_code(dtype), W, P, m_pad, int(quad)))
    cache = _WS_CACHE if pool is None else pool
    key = (torch.device(device), dtype, W, P, m_pad, slot, bool(quad))
    ws = cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        cache[key] = ws
    return ws


# the cross steps' mode and the CPU emulation's EVD order, by inner order
_CROSS_MODE = {"cyclic": STEP_CROSS, "bipartite": STEP_CROSS_BIP, "cross": STEP_CROSS_ONLY}
_EVD_ORDER = {mode: order for order, mode in _CROSS_MODE.items()}


def step_modes(modes, inner_order="cyclic"):
    """Plan modes (STEP_CROSS, STEP_FULL, quad steps) -> kernel modes: with the
    bipartite inner ordering cross steps become STEP_CROSS_BIP (block_evd.hpp
    EVD_BIP, W EVD steps instead of 2W-1), with the cross-only ordering
    STEP_CROSS_ONLY (evd_cross_kernel: the bipartite steps tracking only the
    cross couplings); full steps always use the cyclic EVD."""
    if inner_order not in INNER_ORDERS:
        raise ValueError(f"inner_order must be one of {INNER_ORDERS}, got {inner_order!r}")
    cm = _CROSS_MODE[inner_order]  # "auto": resolve first
    return [cm if int(x) == STEP_CROSS else int(x) for x in modes]


def check_block(dtype, W):
    if W not in SUPPORTED_BLOCK.get(dtype, ()):
        raise ValueError(f"block width {W} unsupported for {dtype}; supported "
                         f"{SUPPORTED_BLOCK.get(dtype, ())}")


def block_steps(At, Vt, D, m_pad, pairs, W, modes, tol, max_inner, metric, ws_slot: int = 0,
                mma="native", pool: dict | None = None, tol_mode="relative",
                inner_order="cyclic", gram_parts: int = 3, shared_gpu: bool = False,
                group_blocks: int | None = None, ws: torch.Tensor | None = None):
    """Run ``len(modes)`` block steps on the current stream.  pairs: int32
    (steps, P, 2) on At's device (block indices local to At); modes: list of
    STEP_* codes (see step_modes for ``inner_order``).  Chains running
    concurrently on different streams must use different ``ws_slot`` values.
    ``gram_parts`` 2: the quad Gram on 2 bf16 parts (STEPS_GRAM2; GPU only,
    the CPU emulation keeps the exact Gram).  ``shared_gpu``: another chain
    runs concurrently on this GPU (STEPS_SHARED_GPU: the quad apply leaves it
    a quarter of the CUs).  ``group_blocks`` (svdj_block_steps_grouped): g > 0
    -- ``metric`` is :func:`new_metric` with ``groups`` rows and a pair (bi,
    bj) reads the floor of and accumulates into row bi // g; no quad steps;
    0 -- one metric through the grouped entry; None -- svdj_block_steps.
    ``ws``: the caller's workspace (uint8, at least svdj_block_workspace_bytes)
    instead of the cached one."""
    modes = step_modes(modes, inner_order)
    _check_layout(At, m_pad)
    check_block(At.dtype, W)
    steps, P = int(pairs.shape[0]), int(pairs.shape[1])
    if group_blocks is not None and (group_blocks < 0 or (
            group_blocks and (STEP_QUAD in modes or STEP_QUAD_SECOND in modes))):
        raise ValueError(f"group_blocks={group_blocks}: must be >= 0, and no quad steps")
    if steps == 0 or P == 0:
        return
    if At.is_cuda:
        if ws is None:
            ws = block_workspace(At.dtype, W, P, m_pad, At.device, ws_slot, pool,
                                 quad=STEP_QUAD in modes)
        md = (C.c_int32 * steps)(*[int(x) for x in modes])
        n_v = Vt.shape[1] if Vt is not None else 0
        ldv = Vt.stride(0) if Vt is not None else 0
        flags = (mma_code(mma, At.dtype) | (STEPS_GRAM2 if gram_parts == 2 else 0)
                 | (STEPS_SHARED_GPU if shared_gpu else 0))
        head = (dtype_code(At.dtype), W, m_pad, _ptr(At), At.stride(0), _ptr(Vt), n_v, ldv,
                _ptr(D), _ptr(pairs), P, steps, md, float(tol), tol_mode_code(tol_mode),
                int(max_inner), _ptr(ws), ws.numel(), _ptr(metric))
        if group_blocks is None:
            hip_check(hip_lib().svdj_block_steps(*head, flags, _stream(At)), "block_steps")
        else:
            hip_check(hip_lib().svdj_block_steps_grouped(*head, int(group_blocks), flags,
                                                         _stream(At)), "block_steps_grouped")
    elif group_blocks:
        # the emulation per group: a group's pairs with its own floor, into its own row
        for s in range(steps):
            grp = torch.div(pairs[s][:, 0], group_blocks, rounding_mode="floor")
            for g in torch.unique(grp).tolist():
                row = metric[g]
                stats = {"smax": 0.0}
                mx, nrot = ref.block_step(At[:, :m_pad], Vt, D, pairs[s][grp == g], W,
                                          modes[s] == STEP_FULL, tol, max_inner,
                                          tol_mode=tol_mode_code(tol_mode), floor=float(row[2]),
                                          order=_EVD_ORDER.get(modes[s], "cyclic"), stats=stats)
                row[0] = max(float(row[0]), mx)
                row[1] += nrot
                row[3] = max(float(row[3]), stats["smax"])
                row[4] += stats.get("ncols", 0)
    else:
        for s in range(steps):
            if modes[s] == STEP_QUAD_SECOND:  # done with the quad's first step
                continue
            stats = {"smax": 0.0}
            if modes[s] == STEP_QUAD:
                mx, nrot = ref.quad_step(At[:, :m_pad], Vt, D, pairs[s], pairs[s + 1], W, tol,
                                         max_inner, tol_mode=tol_mode_code(tol_mode),
                                         floor=float(metric[2]) if metric.numel() > 2 else 0.0,
                                         stats=stats)
            else:
                mx, nrot = ref.block_step(At[:, :m_pad], Vt, D, pairs[s], W, modes[s] == STEP_FULL, tol,
                                          max_inner, tol_mode=tol_mode_code(tol_mode),
                                          floor=float(metric[2]) if metric.numel() > 2 else 0.0,
                                          order=_EVD_ORDER.get(modes[s], "cyclic"),
                                          stats=stats)
            metric[0] = max(float(metric[0]), mx)
            metric[1] += nrot
            if metric.numel() > 4:
                metric[3] = max(float(metric[3]), stats["smax"])
                metric[4] += stats.get("ncols", 0)


def _slabs(shape, At, out):
    """The Gram hooks' result: a new tensor, or ``out`` (tests: pre-filled, so
    that an entry the kernel leaves unwritten shows)."""
    if out is None:
        return torch.empty(*shape, dtype=At.dtype, device=At.device)
    if tuple(out.shape) != tuple(shape) or out.dtype != At.dtype or out.device != At.device or \
            not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {At.dtype} tensor of shape {tuple(shape)} on "
                         f"{At.device}")
    return out


def _gram(At, m_pad, pairs, W, rows_per_chunk, mode, out, what):
    _check_layout(At, m_pad)
    pairs = pairs.to(torch.int32).contiguous().to(At.device)
    P = pairs.shape[0]
    nchunk = -(-m_pad // rows_per_chunk)
    N = 2 * W if mode == STEP_FULL else W
    slabs = _slabs((P, nchunk, N, N), At, out)
    hip_check(hip_lib().svdj_gram(dtype_code(At.dtype), W, mode, _ptr(At), At.stride(0), m_pad,
                                  _ptr(pairs), P, rows_per_chunk, _ptr(slabs), _stream(At)), what)
    return slabs


def gram_cross(At: torch.Tensor, m_pad: int, pairs: torch.Tensor, W: int,
               rows_per_chunk: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """Cross Gram A_bi^T A_bj of every (bi, bj) in ``pairs`` (P, 2) on the
    device (fp32 or fp64), split over row chunks as in a block step; returns
    the chunk slabs (P, nchunk, W, W)."""
    return _gram(At, m_pad, pairs, W, rows_per_chunk, STEP_CROSS, out, "gram_cross")


def gram_full(At: torch.Tensor, m_pad: int, pairs: torch.Tensor, W: int,
              rows_per_chunk: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """Full Gram [A_bi A_bj]^T [A_bi A_bj] of every (bi, bj) in ``pairs``, the
    Gram of a STEP_FULL step; returns the chunk slabs (P, nchunk, 2W, 2W)."""
    return _gram(At, m_pad, pairs, W, rows_per_chunk, STEP_FULL, out, "gram_full")


def gram_quad(At: torch.Tensor, m_pad: int, pairs: torch.Tensor, W: int,
              rows_per_chunk: int, parts: int = 3,
              out: torch.Tensor | None = None) -> torch.Tensor:
    """The six cross Grams of a quad step (fp32, W = 64): ``pairs`` (P, 2) on
    the device in quad order ((a, c), (b, d) per quad).  Returns the slabs
    (3P, nchunk, W, W): the P pairs' Grams, then C_ad, C_bc, C_ab, C_cd of
    every quad (csrc/hip/block_quad.hpp gram_quad_kernel; ``parts`` 2: the
    early-sweep form on 2 bf16 parts)."""
    _check_layout(At, m_pad)
    if At.dtype != torch.float32 or W != 64:
        raise ValueError("gram_quad: fp32 data, W = 64")
    pairs = pairs.to(torch.int32).contiguous().to(At.device)
    P = pairs.shape[0]
    nchunk = -(-m_pad // rows_per_chunk)
    slabs = _slabs((3 * P, nchunk, W, W), At, out)
    hip_check(hip_lib().svdj_gram_quad(_ptr(At), At.stride(0), m_pad, _ptr(pairs), P,
                                       rows_per_chunk, _ptr(slabs), int(parts), _stream(At)),
              "gram_quad")
    return slabs


def apply_q(Xt: torch.Tensor, Q: torch.Tensor, W: int, mma="native"):
    """Xt (2W, ld) rows = columns of X, in place X <- X Q (device tensors)."""
    _check_layout(Xt, Xt.shape[1] // ROW_ALIGN * ROW_ALIGN)
    if Xt.shape[0] != 2 * W or tuple(Q.shape) != (2 * W, 2 * W) or not Q.is_contiguous():
        raise ValueError("Xt must be (2W, ld) and Q contiguous (2W, 2W)")
    rows = Xt.shape[1] // ROW_ALIGN * ROW_ALIGN
    hip_check(hip_lib().svdj_apply_q(dtype_code(Xt.dtype), W, mma_code(mma, Xt.dtype), _ptr(Xt),
                                     rows, Xt.stride(0), _ptr(Q), _stream(Xt)), "apply_q")


def apply_quad(At, Vt, m_pad, pairs, Ts, skip1, skip2, np: int = 3, grid: int = 256,
               cheap_log2: int = 7, work: torch.Tensor | None = None):
    """The quad step's apply alone (fp32, W = 64; csrc/hip/block_quad.hpp
    apply_quad_ts_kernel, launched as a quad step launches it): in place
    [a b c d] <- [a b c d] T on At (rows [0, m_pad)) and Vt (all n_v rows, or
    None) for the quads of ``pairs`` (2 nq, 2) in quad order ((a, c), (b, d)).
    ``Ts``: bfloat16, nq * 256 * 256 * np elements, T - I split into ``np``
    parts in the kernel's fragment layout (svdj_hip.h svdj_apply_quad);
    ``skip1`` / ``skip2``: int32 (2 nq,) flags, a quad with all four set is
    skipped.  ``work``: int32 (2,) device tensor the kernel's work counters
    are added to (see :func:`metric_work`), or None."""
    _check_layout(At, m_pad)
    if At.dtype != torch.float32 or not At.is_cuda:
        raise ValueError("apply_quad: fp32 device data")
    dev = At.device
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.shape[0] % 2 or pairs.shape[0] == 0:
        raise ValueError("apply_quad: pairs must be (2 nq, 2), nq >= 1")
    nq = pairs.shape[0] // 2
    hp = pairs.cpu()
    nb = min(At.shape[0], Vt.shape[0] if Vt is not None else At.shape[0]) // 64
    if int(hp.min()) < 0 or int(hp.max()) >= nb:
        raise ValueError(f"apply_quad: block index outside [0, {nb})")
    pairs = pairs.to(torch.int32).contiguous().to(dev)
    n_v = ldv = 0
    if Vt is not None:
        if Vt.dtype != torch.float32 or Vt.device != dev or Vt.dim() != 2 or Vt.stride(1) != 1:
            raise ValueError("apply_quad: Vt must be an fp32 (ncols, ldv) tensor on At's device")
        n_v, ldv = Vt.shape[1], Vt.stride(0)
    if (Ts.dtype != torch.bfloat16 or Ts.device != dev or not Ts.is_contiguous()
            or Ts.numel() != nq * 256 * 256 * int(np)):
        raise ValueError("apply_quad: Ts must be contiguous bfloat16 with nq * 256 * 256 * np elements")
    for sk in (skip1, skip2):
        if sk.dtype != torch.int32 or sk.device != dev or not sk.is_contiguous() or sk.numel() != 2 * nq:
            raise ValueError("apply_quad: skip flags must be contiguous int32 (2 nq,) on At's device")
    if work is not None and (work.dtype != torch.int32 or work.device != dev
                             or not work.is_contiguous() or work.numel() < 2):
        raise ValueError("apply_quad: work must be a contiguous int32 (2,) tensor on At's device")
    hip_check(hip_lib().svdj_apply_quad(_ptr(At), At.stride(0), m_pad, _ptr(Vt), n_v, ldv,
                                        _ptr(pairs), nq, _ptr(Ts), _ptr(skip1), _ptr(skip2),
                                        int(np), int(grid), int(cheap_log2), _ptr(work),
                                        _stream(At)), "apply_quad")


def _check_chain_args(what, slabs, D, pairs, metric, nb_of_d):
    dev = slabs.device
    if not slabs.is_cuda or not slabs.is_contiguous():
        raise ValueError(f"{what}: slabs must be a contiguous device tensor")
    if D.dtype != slabs.dtype or D.device != dev or D.dim() != 1 or not D.is_contiguous():
        raise ValueError(f"{what}: D must be a contiguous 1-D tensor of the slabs' type and device")
    hp = pairs.cpu()
    if int(hp.min()) < 0 or int(hp.max()) >= nb_of_d:
        raise ValueError(f"{what}: block index outside [0, {nb_of_d})")
    if (metric.dtype != torch.int32 or metric.device != dev or not metric.is_contiguous()
            or metric.numel() < METRIC_WORDS):
        raise ValueError(f"{what}: metric must be new_metric(device)")


def evd_alone(slabs, D, pairs, W: int, mode: int, tol: float, max_inner: int, metric,
              tol_mode="relative", Q: torch.Tensor | None = None):
    """The middle of a single block step alone (csrc/hip/block_launch.hpp launch_evd,
    what a step runs after its Gram): ``slabs`` (P, nchunk, W, W), or (P,
    nchunk, 2W, 2W) for ``mode`` 1, device fp32 / fp64 in the layout the Gram
    kernels write; ``D`` squared column norms by block id (updated in place);
    ``pairs`` (P, 2) block ids; ``mode`` 0 cyclic, 1 full, 2 bipartite, 3
    cross (+ chunk pre-sum and Q build, selected by P and nchunk as in a
    solve).  Returns (Q (P, 2W, 2W), skip (P,) int32); the Q of a skipped pair
    is not written (``Q``: the buffer to write into, e.g. pre-filled)."""
    check_block(slabs.dtype, W)
    P, nchunk = int(slabs.shape[0]), int(slabs.shape[1])
    side = 2 * W if mode == 1 else W
    if mode not in (0, 1, 2, 3) or slabs.dim() != 4 or tuple(slabs.shape[2:]) != (side, side):
        raise ValueError(f"evd_alone: mode 0-3 and slabs (P, nchunk, {side}, {side})")
    if pairs.dim() != 2 or tuple(pairs.shape) != (P, 2):
        raise ValueError("evd_alone: pairs must be (P, 2)")
    _check_chain_args("evd_alone", slabs, D, pairs, metric, D.numel() // W)
    dev = slabs.device
    pairs = pairs.to(torch.int32).contiguous().to(dev)
    if Q is None:
        Q = torch.zeros(P, 2 * W, 2 * W, dtype=slabs.dtype, device=dev)
    elif (Q.dtype != slabs.dtype or Q.device != dev or not Q.is_contiguous()
          or tuple(Q.shape) != (P, 2 * W, 2 * W)):
        raise ValueError("evd_alone: Q must be contiguous (P, 2W, 2W) of the slabs' type and device")
    skip = torch.zeros(P, dtype=torch.int32, device=dev)
    lib = hip_lib()
    nbytes = int(lib.svdj_evd_alone_workspace_bytes(dtype_code(slabs.dtype), W, P, nchunk))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    hip_check(lib.svdj_evd_alone(dtype_code(slabs.dtype), W, int(mode), _ptr(slabs), nchunk, _ptr(D),
                                 _ptr(pairs), P, float(tol), tol_mode_code(tol_mode), int(max_inner),
                                 _ptr(Q), _ptr(skip), _ptr(ws), ws.numel(), _ptr(metric),
                                 _stream(slabs)), "evd_alone")
    return Q, skip


def quad_chain(slabs, D, pairs0, pairs1, tol: float, max_inner: int, metric, np: int = 3,
               tol_mode="relative"):
    """The middle of a quad step alone (fp32, W = 64; csrc/hip/block_launch.hpp
    launch_quad_chain, what a quad step runs between its Gram and its apply):
    ``slabs`` (3P, nchunk, 64, 64) in :func:`gram_quad`'s order, ``D`` squared
    column norms by block id (updated in place), ``pairs0`` (P, 2) in quad
    order ((a, c), (b, d)) and ``pairs1`` ((a, d), (b, c)).  Returns a dict:
    ``T1`` (P, 128, 128) fp64, ``upd`` (P, 64, 64), ``Ts`` (bfloat16, (P / 2)
    * 256 * 256 * np, :func:`apply_quad`'s layout), ``skip1``, ``skip2``."""
    if slabs.dtype != torch.float32 or slabs.dim() != 4 or tuple(slabs.shape[2:]) != (64, 64) \
            or slabs.shape[0] % 6 or slabs.shape[0] == 0:
        raise ValueError("quad_chain: fp32 slabs (3P, nchunk, 64, 64), P even")
    P, nchunk = int(slabs.shape[0]) // 3, int(slabs.shape[1])
    if tuple(pairs0.shape) != (P, 2) or tuple(pairs1.shape) != (P, 2):
        raise ValueError("quad_chain: pairs0, pairs1 must be (P, 2)")
    pairs = torch.stack([pairs0.cpu(), pairs1.cpu()]).to(torch.int32).contiguous()
    _check_chain_args("quad_chain", slabs, D, pairs, metric, D.numel() // 64)
    if np not in (2, 3):
        raise ValueError("quad_chain: np 2 or 3")
    dev = slabs.device
    pairs = pairs.to(dev)
    out = {"T1": torch.zeros(P, 128, 128, dtype=torch.float64, device=dev),
           "upd": torch.zeros(P, 64, 64, dtype=torch.float32, device=dev),
           "Ts": torch.zeros(P // 2 * 256 * 256 * int(np), dtype=torch.bfloat16, device=dev),
           "skip1": torch.zeros(P, dtype=torch.int32, device=dev),
           "skip2": torch.zeros(P, dtype=torch.int32, device=dev)}
    lib = hip_lib()
    ws = torch.empty(int(lib.svdj_quad_chain_workspace_bytes(P)), dtype=torch.uint8, device=dev)
    hip_check(lib.svdj_quad_chain(_ptr(slabs), nchunk, _ptr(D), _ptr(pairs), P, float(tol),
                                  tol_mode_code(tol_mode), int(max_inner), int(np), _ptr(out["T1"]),
                                  _ptr(out["upd"]), _ptr(out["Ts"]), _ptr(out["skip1"]),
                                  _ptr(out["skip2"]), _ptr(ws), ws.numel(), _ptr(metric),
                                  _stream(slabs)), "quad_chain")
    return out


def block_solve(At, Vt, D, m_pad, W, tol, max_inner, max_sweeps, mma="native",
                tol_mode="relative", inner_order="cyclic", stop_rule="second_order"):
    """Single-device block Jacobi (round-robin over ncols/W blocks, first
    step of each sweep full; cross steps with ``inner_order``; stop test
    :func:`sweep_converged`).  Returns (sweeps, hist)."""
    step_modes([], inner_order)  # validates
    _check_layout(At, m_pad)
    check_block(At.dtype, W)
    ncols = At.shape[0]
    if At.is_cuda:
        nb = ncols // W
        ws = block_workspace(At.dtype, W, nb // 2, m_pad, At.device)
        metric = new_metric(At.device)
        hist = (C.c_double * max(max_sweeps, 1))()
        n_v = Vt.shape[1] if Vt is not None else 0
        ldv = Vt.stride(0) if Vt is not None else 0
        sweeps = hip_check(hip_lib().svdj_block_solve(
            dtype_code(At.dtype), W, m_pad, _ptr(At), At.stride(0), _ptr(Vt), n_v, ldv, _ptr(D),
            ncols, float(tol), tol_mode_code(tol_mode), int(max_inner), int(max_sweeps),
            INNER_ORDERS.index(inner_order), _ptr(ws), ws.numel(), _ptr(metric), hist,
            mma_code(mma, At.dtype), STOP_RULES[stop_rule], _stream(At)),
            "block_solve")
        return sweeps, [hist[i] for i in range(sweeps)]
    from ..parallel.schedule import round_robin

    nb = ncols // W
    pairs = torch.from_numpy(round_robin(nb))
    modes = [1] + [0] * (nb - 2)
    hist = []
    metric = new_metric("cpu")
    set_norm_floor(metric, At.dtype, m_pad, float(D.max()) if D.numel() else 1.0)
    for _ in range(max_sweeps):
        reset_metric(metric)
        block_steps(At, Vt, D, m_pad, pairs, W, modes, tol, max_inner, metric,
                    tol_mode=tol_mode, inner_order=inner_order)
        mx, ms, nrot, ncr = read_stop(metric)
        hist.append(mx)
        if sweep_converged(mx, ms, nrot, ncr, tol, tol_mode, stop_rule):
            break
    return len(hist), hist


# ------------------------------------------------- batched path, block engine
def stack_pack(A3: torch.Tensor, m_pad: int, ncols: int, n_v: int, want_v: bool):
    """The batch ``A3`` (B, m, n), m >= n, stacked for the block kernels
    (csrc/hip/batched_block.hip svdj_stack_pack; torch operations on the CPU):
    returns (At (B ncols, m_pad), Vt (B ncols, n_v) or None, D (B ncols,),
    metric :func:`new_metric` with B rows).  Matrix b's column j is row
    b ncols + j of At, pad rows and columns zero; Vt holds an identity block per
    matrix; D the squared column norms; every metric row its matrix's own
    floor (:func:`norm_floor` of m_pad and the matrix's largest D)."""
    B, m, n = A3.shape
    dev, dt = A3.device, A3.dtype
    metric = new_metric(dev, groups=B)
    if A3.is_cuda:
        At = torch.empty(B * ncols, m_pad, dtype=dt, device=dev)
        Vt = torch.empty(B * ncols, n_v, dtype=dt, device=dev) if want_v else None
        D = torch.empty(B * ncols, dtype=dt, device=dev)
        hip_check(hip_lib().svdj_stack_pack(
            dtype_code(dt), B, m, n, _ptr(A3), A3.stride(0), A3.stride(1), A3.stride(2), m_pad,
            ncols, _ptr(At), m_pad, _ptr(Vt), n_v, n_v, _ptr(D), _ptr(metric), _stream(A3)),
            "stack_pack")
        return At, Vt, D, metric
    At = torch.zeros(B, ncols, m_pad, dtype=dt)
    At[:, :n, :m] = A3.transpose(1, 2)
    At = At.reshape(B * ncols, m_pad)
    Vt = None
    if want_v:
        Vt = torch.zeros(B, ncols, n_v, dtype=dt)
        idx = torch.arange(ncols)
        Vt[:, idx, idx] = 1
        Vt = Vt.reshape(B * ncols, n_v)
    D = ref.col_norms2(At)
    dmax = D.reshape(B, ncols).amax(1).tolist()
    for b in range(B):
        metric[b, 2] = norm_floor(dt, m_pad, dmax[b])
    return At, Vt, D, metric


def stack_finalize(At, Vt, B: int, m: int, n: int, m_pad: int, ncols: int, want_u: bool,
                   want_v: bool):
    """Sigma, U and V of a stacked solve (svdj_stack_finalize; torch operations
    on the CPU): returns (U (B, m, n) or None, S (B, n), V (B, n, n) or None),
    sigma the fp64 column norm, U's columns divided by it (a zero sigma leaves
    the column as it is)."""
    dev, dt = At.device, At.dtype
    if At.is_cuda:
        U = torch.empty(B, m, n, dtype=dt, device=dev) if want_u else None
        S = torch.empty(B, n, dtype=dt, device=dev)
        V = torch.empty(B, n, n, dtype=dt, device=dev) if want_v else None
        n_v = Vt.shape[1] if Vt is not None else 0
        hip_check(hip_lib().svdj_stack_finalize(
            dtype_code(dt), B, m, n, m_pad, ncols, _ptr(At), At.stride(0), _ptr(Vt), n_v,
            Vt.stride(0) if Vt is not None else 0, _ptr(U), _ptr(S), _ptr(V), int(want_u),
            _stream(At)), "stack_finalize")
        return U, S, V
    sig = ref.finalize(At[:, :m_pad], want_u)
    A3 = At.reshape(B, ncols, -1)
    U = A3[:, :n, :m].transpose(1, 2).contiguous() if want_u else None
    V = Vt.reshape(B, ncols, -1)[:, :n, :n].transpose(1, 2).contiguous() if want_v else None
    return U, sig.reshape(B, ncols)[:, :n].contiguous(), V


def stack_bytes(dtype: torch.dtype, W: int, chunk: int, k: int, m_pad: int, n_v: int,
                want_v: bool, device) -> int:
    """Bytes a chunk of ``chunk`` stacked matrices of k W-wide blocks takes:
    the stacked A, the stacked V, and on a GPU svdj_block_workspace_bytes of a
    step with all its chunk * k / 2 pairs."""
    esize = 8 if dtype == torch.float64 else 4
    total = chunk * k * W * (m_pad + (n_v if want_v else 0)) * esize
    if torch.device(device).type != "cpu":
        total += int(hip_lib().svdj_block_workspace_bytes(dtype_code(dtype), W, chunk * k // 2,
                                                          m_pad, 0))
    return total


# --------------------------------------------------------------- batched path
BATCHED_MAX_N = 64  # csrc/hip/batched.hip kBatchedMaxN


def batched_lds_bytes(dtype: torch.dtype, m: int, n: int, want_v: bool = True) -> int:
    """LDS bytes one workgroup of the batched kernel takes for an (m x n)
    matrix, m >= n (csrc/hip/batched.hip batched_layout); 0: the shape is
    outside the kernel's envelope (n > 64, or it does not fit in 160 KiB)."""
    return int(hip_lib().svdj_batched_lds_bytes(dtype_code(dtype), int(m), int(n), int(want_v)))


def batched_threads(n: int) -> int:
    """Threads of the workgroup that solves a matrix of n columns (0: n
    outside the kernel's 1..64)."""
    return int(hip_lib().svdj_batched_threads(int(n)))


def batched_svd(A: torch.Tensor, tol: float, tol_mode=0, max_sweeps: int = 60,
                want_u: bool = True, want_v: bool = True):
    """SVD of every matrix of the device tensor ``A`` (batch, m, n), m >= n,
    in one launch on the current stream (csrc/hip/batched.hip).  ``A`` is read
    in place through its strides.  Returns (U (batch, m, n) or None, S (batch,
    n), V (batch, n, n) or None, sweeps int32 (batch,), off float32 (batch,))."""
    if A.dim() != 3 or not A.is_cuda:
        raise ValueError("batched_svd: a (batch, m, n) device tensor")
    B, m, n = A.shape
    dev, dt = A.device, A.dtype
    U = torch.empty(B, m, n, dtype=dt, device=dev) if want_u else None
    S = torch.empty(B, n, dtype=dt, device=dev)
    V = torch.empty(B, n, n, dtype=dt, device=dev) if want_v else None
    sweeps = torch.empty(B, dtype=torch.int32, device=dev)
    off = torch.empty(B, dtype=torch.float32, device=dev)
    hip_check(hip_lib().svdj_batched_svd(
        dtype_code(dt), B, m, n, _ptr(A), A.stride(0), A.stride(1), A.stride(2), _ptr(U), _ptr(S),
        _ptr(V), float(tol), tol_mode_code(tol_mode), int(max_sweeps), _ptr(sweeps), _ptr(off),
        _stream(A)), "batched_svd")
    return U, S, V, sweeps, off


def batched_tall_lds_bytes(dtype: torch.dtype, n: int, want_v: bool = True,
                           panel_rows: int = 8) -> int:
    """LDS bytes one workgroup of the tall batched kernel takes at n columns
    with panels of ``panel_rows`` rows (csrc/hip/batched_tall.hip
    batched_tall_layout); 0: bad arguments, or more than 160 KiB."""
    return int(hip_lib().svdj_batched_tall_lds_bytes(dtype_code(dtype), int(n), int(want_v),
                                                     int(panel_rows)))


def batched_tall_panel_rows(dtype: torch.dtype, n: int, want_v: bool = True) -> int:
    """The panel height the tall batched kernel chooses at n columns (0: n
    outside 1..64)."""
    return int(hip_lib().svdj_batched_tall_panel_rows(dtype_code(dtype), int(n), int(want_v)))


def batched_tall_balanced_rows(dtype: torch.dtype, m: int, n: int, want_v: bool = True) -> int:
    """Panel height for m rows: as many panels as the kernel's own choice
    needs, of equal height (a multiple of 8), so that the zero padding of the
    last one stays under 8 rows per panel."""
    top = batched_tall_panel_rows(dtype, n, want_v)
    if top <= 0:
        return 0
    panels = -(-int(m) // top)
    return min(top, (-(-int(m) // panels) + 7) // 8 * 8)


def batched_tall_svd(A: torch.Tensor, tol: float, tol_mode=0, max_sweeps: int = 60,
                     want_u: bool = True, want_v: bool = True, panel_rows: int = 0):
    """SVD of every matrix of the device tensor ``A`` (batch, m, n), m >= n,
    n <= 64, any m, in one launch on the current stream: QR by row panels into
    an LDS-resident R, Jacobi on R, U = Q U_R (csrc/hip/batched_tall.hip).
    ``panel_rows`` 0: the kernel's choice; a positive multiple of 8 forces
    it.  Returns what :func:`batched_svd` returns."""
    if A.dim() != 3 or not A.is_cuda:
        raise ValueError("batched_tall_svd: a (batch, m, n) device tensor")
    B, m, n = A.shape
    dev, dt = A.device, A.dtype
    rows = int(panel_rows) or batched_tall_panel_rows(dt, n, want_v)
    U = torch.empty(B, m, n, dtype=dt, device=dev) if want_u else None
    S = torch.empty(B, n, dtype=dt, device=dev)
    V = torch.empty(B, n, n, dtype=dt, device=dev) if want_v else None
    tau = (torch.empty(B, -(-m // rows), n, dtype=dt, device=dev)
           if want_u and rows > 0 else None)
    sweeps = torch.empty(B, dtype=torch.int32, device=dev)
    off = torch.empty(B, dtype=torch.float32, device=dev)
    hip_check(hip_lib().svdj_batched_tall_svd(
        dtype_code(dt), B, m, n, _ptr(A), A.stride(0), A.stride(1), A.stride(2), _ptr(U), _ptr(S),
        _ptr(V), _ptr(tau), int(panel_rows), float(tol), tol_mode_code(tol_mode), int(max_sweeps),
        _ptr(sweeps), _ptr(off), _stream(A)), "batched_tall_svd")
    return U, S, V, sweeps, off


__all__ = [
    "batched_lds_bytes", "batched_threads", "batched_svd", "BATCHED_MAX_N",
    "batched_tall_lds_bytes", "batched_tall_panel_rows", "batched_tall_balanced_rows",
    "batched_tall_svd", "stack_pack", "stack_finalize", "stack_bytes", "reset_group_metrics",
    "read_group_stops",
    "NativeError", "ROW_ALIGN", "SUPPORTED_BLOCK", "INNER_ORDERS", "step_modes", "dtype_code", "new_metric", "reset_metric", "set_norm_floor",
    "METRIC_WORDS", "read_stop", "metric_stop_values", "metric_work", "sweep_converged", "STOP_RULES",
    "read_metric", "set_identity", "col_norms2", "finalize", "scalar_step", "scalar_solve",
    "block_workspace", "block_steps", "block_solve", "check_block", "MMA_CODES", "mma_code",
    "STEP_CROSS", "STEP_FULL", "STEP_CROSS_BIP", "STEP_CROSS_ONLY", "STEP_QUAD", "STEP_QUAD_SECOND",
    "MMA_MASK", "STEPS_GRAM2", "STEPS_SHARED_GPU",
    "apply_q", "apply_quad",
    "gram_cross", "gram_full", "gram_quad", "evd_alone", "quad_chain",
]
