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
"""
from __future__ import annotations

import math

import torch

from ..config import SolverConfig, SVDOptions
from ..ops import kernels as K
from .base import BatchedSVDResult, Solver, Timer


class BatchedJacobi(Solver):
    name = "batched"

    def pick_engine(self, device, dtype, m: int, n: int, want_v: bool) -> str:
        """"kernel" for a device problem (m >= n) inside the kernel's envelope;
        "qr_kernel" for a tall one (m > n) when the config asks for the QR stage."""
        if self.config.method != "auto":  # the caller named a single-matrix solver
            return "loop"
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
