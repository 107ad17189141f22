"""Batched SVD of many small matrices.

Engine "kernel": one launch of csrc/hip/batched.hip, one workgroup per
matrix with the matrix and V resident in LDS (a device input with at most 64
columns after it is made tall, and a row count that fits the CU's LDS:
``ops.kernels.batched_lds_bytes``).  Engine "qr_kernel": one launch of
csrc/hip/batched_tall.hip, any row count at up to 64 columns (QR by row panels
into an LDS-resident R, the same Jacobi on R, U = Q U_R); it runs only when
the caller asks for it with ``precondition="qr"`` and the input, once made
tall, has m > n (``panel_rows`` forces the panel height).  Engine "loop": the
single-matrix :func:`svd` per matrix -- on a CPU device the oracle -- so the API is total;
``info["engine"]`` says which one ran.  An explicit ``method`` in the config
(anything but "auto") is honoured: the loop engine runs that method per
matrix.  S comes back in the working dtype on either engine (fp32 for bf16
input).

Engine "block" (``batched="block"`` in the config, never chosen by "auto"):
the batch solved by the block path's own step kernels, for any column count
and on either device.  The B matrices are stacked side by side as column
blocks of one m_pad x (B ncols) array, k = ncols / W blocks each, their V's
as n_v x (B ncols) (csrc/hip/batched_block.hip svdj_stack_pack).  A step whose
pair list holds every active matrix's pairs of the round robin over its own k
blocks, never a pair across two matrices, is then B independent block-Jacobi
steps in one launch of the MFMA Gram, the LDS EVDs and the MFMA apply, with
B k / 2 pairs to fill the GPU.  The EVD kernels keep the stop-test words per
matrix (svdj_block_steps_grouped, group_blocks = k): each matrix has its own
underflow floor, convergence value and rotation counts, stops on its own, and
leaves the pair list when it does -- its columns are not touched again.  The
sweep loop runs on the host, one copy of the B x 8 metric words per sweep;
single steps on one stream, the first step of a sweep STEP_FULL.  A matrix's
result does not depend on its place in the batch, but on the GPU it does
depend on the batch's composition: the Gram's row split and the "auto" inner
order follow the number of pairs in the step, i.e. how many matrices of the
chunk are still active, so the same matrix in another batch, or in another
chunking of the same batch, may round differently.  The batch is cut into
chunks whose stacked A, stacked V and step workspace stay under
``STACK_BYTE_CAP``; ``extra["batch_chunk"]`` asks for fewer matrices per chunk
(a value the cap or the kernels' index range does not allow is cut down to
what they allow).
On a CPU device the same driver runs on the emulation of ops/reference.py.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..config import SolverConfig, SVDOptions
from ..ops import kernels as K
from ..utils.layout import pad_rows, round_up
from .base import BatchedSVDResult, Solver, Timer

# Block engine: bytes of one chunk's stacked A, stacked V and step workspace.
# 4 GiB keeps a chunk far below the 288 GB of an MI355X next to the caller's
# own batch and the outputs, and is large enough that the shapes the engine is
# for run in one chunk (1024 x 128 x 128 fp32: 0.4 GiB; 64 x 512 x 512: 0.2 GiB).
STACK_BYTE_CAP = 4 << 30
# what the kernels index: svdj_stack_pack's grid (65535 matrices) and int32
# stacked column numbers
STACK_MAX_MATRICES = 65535
STACK_MAX_COLUMNS = 2 ** 31 - 1


def stacked_pairs(k: int, active) -> np.ndarray:
    """The block engine's pair list of one sweep: (k - 1, len(active) k / 2, 2)
    int32 block indices into the stacked array, the round robin over k blocks
    (parallel/schedule.py) replicated for every matrix g of ``active`` (its
    index in the chunk) with block offset g k.  No pair crosses a matrix."""
    from ..parallel.schedule import round_robin

    rr = round_robin(k)  # (k - 1, k / 2, 2)
    off = np.asarray(active, dtype=np.int32) * np.int32(k)
    return np.ascontiguousarray(
        (rr[:, None, :, :] + off[None, :, None, None]).reshape(k - 1, -1, 2))


def stack_chunk(B: int, k: int, ncols: int, nbytes) -> int:
    """Matrices per chunk of the block engine: the most whose ``nbytes(chunk)``
    stays under STACK_BYTE_CAP (at least one), within the kernels' index range."""
    hi = max(1, min(B, STACK_MAX_MATRICES, STACK_MAX_COLUMNS // ncols))
    if nbytes(hi) <= STACK_BYTE_CAP:
        return hi
    lo = 1  # nbytes grows with the chunk: bisect
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if nbytes(mid) <= STACK_BYTE_CAP else (lo, mid)
    return lo


class BatchedJacobi(Solver):
    name = "batched"

    def pick_engine(self, device, dtype, m: int, n: int, want_v: bool) -> str:
        """"kernel" for a device problem (m >= n) inside the kernel's envelope;
        "qr_kernel" for a tall one (m > n) when the config asks for the QR stage."""
        if self.config.method != "auto":  # the caller named a single-matrix solver
            return "loop"
        if self.config.batched == "block" and n >= 1:  # opt-in, any device, before the QR stage
            return "block"
        if torch.device(device).type != "cuda" or n < 1 or n > K.BATCHED_MAX_N:
            return "loop"
        if self.config.precondition == "qr" and m > n:
            return "qr_kernel"
        return "kernel" if K.batched_lds_bytes(dtype, m, n, want_v) > 0 else "loop"

    def solve(self, A, jobu=SVDOptions.AllVec, jobv=SVDOptions.AllVec,
              device=None) -> BatchedSVDResult:
        cfg = self.config
        jobu, jobv = SVDOptions.parse(jobu), SVDOptions.parse(jobv)
        device = torch.device(device) if device is not None else A.device
        dtype = cfg.resolved_dtype(A)
        bf16 = cfg.bf16_mode(A)
        lead = tuple(A.shape[:-2])
        A3 = A.reshape(math.prod(lead), A.shape[-2], A.shape[-1])
        wide = A3.shape[1] < A3.shape[2]
        if wide:  # A^T = U' S V'^T  =>  A = V' S U'^T: the view's strides, no copy
            A3 = A3.transpose(1, 2)
            jobu, jobv = jobv, jobu
        B, m, n = A3.shape
        want_u, want_v = jobu != SVDOptions.NoVec, jobv != SVDOptions.NoVec
        engine = self.pick_engine(device, dtype, m, n, want_v)
        # the stop test sees the columns the Jacobi rotates: those of R (n rows) after a QR
        tol = self.tolerance(cfg.precision_dtype(A), n if engine == "qr_kernel" else m)
        info = {"engine": engine, "tol": tol, "dtype": str(dtype), "device": str(device),
                "batch": B, "transposed": wide}
        with Timer(device) as tm:
            if B == 0 or n == 0:
                out = self._empty(B, m, n, want_u, want_v, dtype, device)
            elif engine == "kernel":
                out = self._kernel(A3, dtype, device, tol, want_u, want_v, info)
            elif engine == "qr_kernel":
                out = self._qr_kernel(A3, dtype, device, tol, want_u, want_v, info)
            elif engine == "block":
                out = self._block(A, A3, dtype, device, tol, want_u, want_v, info)
            else:
                out = self._loop(A3, jobu, jobv, device)
        U, S, V, sweeps, off = out
        S = S.to(dtype)
        converged = (sweeps < cfg.max_sweeps) | (off.double() <= tol)
        if bf16:
            U = U.to(torch.bfloat16) if U is not None else None
            V = V.to(torch.bfloat16) if V is not None else None
        if wide:
            U, V = V, U
        if cfg.sort:
            S, order = torch.sort(S, dim=-1, descending=True)
            if U is not None:
                U = U.gather(-1, order[:, None, :].expand_as(U))
            if V is not None:
                V = V.gather(-1, order[:, None, :].expand_as(V))

        def unflat(t):
            return t.reshape(lead + tuple(t.shape[1:])) if t is not None else None

        return BatchedSVDResult(unflat(U), unflat(S), unflat(V), unflat(sweeps), unflat(converged),
                                unflat(off), tm.seconds, info)

    @staticmethod
    def _empty(B, m, n, want_u, want_v, dtype, device):
        U = torch.empty(B, m, n, dtype=dtype, device=device) if want_u else None
        V = torch.empty(B, n, n, dtype=dtype, device=device) if want_v else None
        return (U, torch.empty(B, n, dtype=dtype, device=device), V,
                torch.zeros(B, dtype=torch.int32, device=device),
                torch.zeros(B, dtype=torch.float32, device=device))

    @staticmethod
    def _device_copy(A3, dtype, device, info):
        W = A3.to(device=device, dtype=dtype)  # keeps the strides of a dense view
        in_place = W.is_contiguous() or W.transpose(1, 2).is_contiguous()
        if not in_place:
            W = W.contiguous()
        info["in_place"] = bool(in_place)
        return W

    def _kernel(self, A3, dtype, device, tol, want_u, want_v, info):
        cfg = self.config
        W = self._device_copy(A3, dtype, device, info)
        B, m, n = W.shape
        info["lds_bytes"] = K.batched_lds_bytes(dtype, m, n, want_v)
        return K.batched_svd(W, tol, 1 if cfg.tol_mode == "absolute" else 0, cfg.max_sweeps,
                             want_u, want_v)

    def _qr_kernel(self, A3, dtype, device, tol, want_u, want_v, info):
        cfg = self.config
        W = self._device_copy(A3, dtype, device, info)
        B, m, n = W.shape
        rows = cfg.panel_rows or K.batched_tall_balanced_rows(dtype, m, n, want_v)
        info["panel_rows"] = rows
        info["panels"] = -(-m // rows)
        info["lds_bytes"] = K.batched_tall_lds_bytes(dtype, n, want_v, rows)
        return K.batched_tall_svd(W, tol, 1 if cfg.tol_mode == "absolute" else 0, cfg.max_sweeps,
                                  want_u, want_v, rows)

    def _block(self, A, A3, dtype, device, tol, want_u, want_v, info):
        from .block import resolve_inner_order

        cfg = self.config
        B, m, n = A3.shape
        W = cfg.block or 32
        K.check_block(dtype, W)
        mma = cfg.resolved_mma(A, W)
        ncols = max(round_up(n, 2 * W), 2 * W)
        k = ncols // W
        m_pad, n_v = pad_rows(m), pad_rows(ncols)
        forced = int((cfg.extra or {}).get("batch_chunk", 0))
        if forced < 0:
            raise ValueError(f"batch_chunk must be >= 1 (0: by the byte cap), got {forced}")
        # a forced chunk size is still held to the byte cap and the index range
        chunk = stack_chunk(min(forced, B) if forced else B, k, ncols,
                            lambda c: K.stack_bytes(dtype, W, c, k, m_pad, n_v, want_v, device))
        info.update(block=W, blocks_per_matrix=k, pairs_per_step=min(chunk, B) * k // 2,
                    chunks=-(-B // chunk), mma=mma, batch_chunk=chunk)
        U = torch.empty(B, m, n, dtype=dtype, device=device) if want_u else None
        S = torch.empty(B, n, dtype=dtype, device=device)
        V = torch.empty(B, n, n, dtype=dtype, device=device) if want_v else None
        sweeps = torch.zeros(B, dtype=torch.int32)
        off = torch.full((B,), float("inf"), dtype=torch.float32)
        modes = [K.STEP_FULL] + [K.STEP_CROSS] * (k - 2)
        ws = None
        for b0 in range(0, B, chunk):
            b1 = min(b0 + chunk, B)
            Wc = self._device_copy(A3[b0:b1], dtype, device, info)
            At, Vt, D, metric = K.stack_pack(Wc, m_pad, ncols, n_v, want_v)
            del Wc
            active = np.arange(b1 - b0)
            for _ in range(cfg.max_sweeps):
                P = len(active) * k // 2
                if device.type != "cpu":
                    need = int(K.hip_lib().svdj_block_workspace_bytes(K.dtype_code(dtype), W, P,
                                                                      m_pad, 0))
                    if ws is None or ws.numel() < need:
                        ws = torch.empty(need, dtype=torch.uint8, device=device)
                pairs = torch.from_numpy(stacked_pairs(k, active)).to(device)
                inner = resolve_inner_order(cfg.inner_order, W, P, dtype)
                K.block_steps(At, Vt, D, m_pad, pairs, W, modes, tol, cfg.max_inner_sweeps, metric,
                              mma=mma, tol_mode=cfg.tol_mode, inner_order=inner, group_blocks=k,
                              ws=ws)
                mx, ms, nrot, ncr = K.read_group_stops(metric)
                sweeps[b0 + active] += 1
                off[b0 + active] = torch.from_numpy(mx[active]).float()
                active = np.array([g for g in active.tolist()
                                   if not K.sweep_converged(mx[g], ms[g], nrot[g], ncr[g], tol,
                                                            cfg.tol_mode, cfg.stop_rule)],
                                  dtype=np.int64)
                if len(active) == 0:
                    break
                K.reset_group_metrics(metric, torch.from_numpy(active).to(metric.device))
            Uc, Sc, Vc = K.stack_finalize(At, Vt, b1 - b0, m, n, m_pad, ncols, want_u, want_v)
            S[b0:b1] = Sc
            if want_u:
                U[b0:b1] = Uc
            if want_v:
                V[b0:b1] = Vc
        return U, S, V, sweeps.to(device), off.to(device)

    def _loop(self, A3, jobu, jobv, device):
        from ..api import svd  # the single-matrix entry point (imports this module's package)

        cfg = SolverConfig(**{**self.config.__dict__, "sort": False})
        Us, Ss, Vs, sweeps, off = [], [], [], [], []
        for i in range(A3.shape[0]):
            r = svd(A3[i], jobu, jobv, config=cfg, device=device)
            Us.append(r.U)
            Ss.append(r.S)
            Vs.append(r.V)
            sweeps.append(int(r.sweeps))
            # a sweep limit of 0 leaves no history: nothing was measured
            off.append(float(r.history[-1]) if r.history else float("inf"))
        dev = Ss[0].device
        U = torch.stack(Us) if Us[0] is not None else None
        V = torch.stack(Vs) if Vs[0] is not None else None
        return (U, torch.stack(Ss), V, torch.tensor(sweeps, dtype=torch.int32, device=dev),
                torch.tensor(off, dtype=torch.float32, device=dev))
