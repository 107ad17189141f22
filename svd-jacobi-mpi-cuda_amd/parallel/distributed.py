"""Distributed block one-sided Jacobi (one process per GPU).

Reference: ``omp_mpi_cuda_dgesvd_local_matrices`` (reference main.cu:440-1423)
splits every Sameh step's pairs across MPI ranks and has rank 0 scatter the
needed columns of A and V to every worker and gather them back EVERY step
(main.cu:582-680, 854-936; 2 TB of host-staged traffic per sweep at n=5000).

MI355X design:

* owner-computes: the n columns are cut into 2P super-blocks of B columns;
  GPU g permanently holds two of them (A and V columns + tracked squared
  norms) in HBM;
* a sweep is a 2P-1 round tournament over super-blocks (every pair meets
  once); between rounds each GPU sends exactly ONE super-block to one peer
  and receives one (grouped RCCL send/recv over xGMI) -- see
  ``schedule.tournament``;
* inside a round, the GPU orthogonalises its two resident super-blocks with
  the MFMA block kernels: round 0 runs a full round robin over its 2k
  W-blocks (covering all within-super-block pairs once per sweep), later
  rounds run the k-step bipartite cross schedule;
* the stop test is an all-reduce (max off value, sum of rotations) per sweep.

Input is root-owned like the reference (rank 0 passes A, which is scattered
once), or generated in place per rank (``generator``) for large synthetic
benchmarks.  Output is gathered to rank 0 (``gather=True``) in the
reference's layout, or left distributed (parallel/dataio.py moves the data).
A solve is a :class:`_Solve` record and short parts, as the native engine's
``Solve`` (csrc/distributed/svdj_dist.cpp).
"""
from __future__ import annotations

import os
import sys
import time
from dataclasses import dataclass, field

import torch

from ..config import SolverConfig, SVDOptions, debug_knob
from ..models.base import SVDResult, Solver
from ..models import precondition as pre
from ..models.block import (choose_block, choose_merged, choose_mma, quad_size_rule,
                            resolve_inner_order, resolve_quad)
from ..ops import kernels as K
from ..utils import checkpoint as ckpt
from ..utils.layout import pad_rows, round_up
from ..utils.tracing import trace_range
from . import dataio
from .comm import Communicator
from .pipeline import PipelineExecutor
from .plan import advance_placement, sweep_plan
from .schedule import distributed_sweep_plan, tournament


@dataclass
class _Solve:
    """State of one ``DistributedBlockJacobi._solve`` call."""
    cfg: SolverConfig
    pool: dict               # the solver's kernel workspaces
    rank: int
    tour: object             # schedule.tournament(P)
    geo: dict                # DistributedBlockJacobi.geometry
    m: int
    n: int
    pdtype: torch.dtype      # problem precision; the buffers hold ``dtype``
    dtype: torch.dtype
    tol: float
    want_u: bool
    want_v: bool
    # resolved rules (_resolve_rules)
    pipelined: bool          # chains=2; False: the blocking exchange of chains=1
    W: int
    mma: str
    inner: str
    quad: bool
    merged: bool
    shared_gpu: bool         # two chains issued concurrently
    gram2: int | None        # SVDJ_DEBUG gram2=0/1, else None
    # buffers (_allocate); phys[h][s] = super-block resident in slot s of GPU h
    # (plan.advance_placement: every rank keeps the whole table)
    At: torch.Tensor = None
    Vt: torch.Tensor = None
    D: torch.Tensor = None
    metric: torch.Tensor = None
    phys: list = None
    # per-sweep state
    gram_parts: int = 3      # bf16 parts of this sweep's quad Grams
    prev_all: bool = True    # the previous sweep rotated every pair
    # work done by the quad kernels (bench.py's executed-MFMA and HBM estimates):
    # quad Grams issued (host counts), the apply's device counters (no host sync)
    gram_quads: int = 0
    gram_quads2: int = 0
    work_acc: torch.Tensor = None
    hist: list = field(default_factory=list)
    sweeps: int = 0
    t_comm: float = 0.0
    stop_reason: str | None = None   # set when the stop test holds (converged)

    def run_steps(self, pairs, modes, slot):
        """Enqueue block steps on the current stream (the executor's hook)."""
        # quads of the quad steps issued (each runs the quad Gram): host count
        nq = sum(1 for x in modes if int(x) == K.STEP_QUAD) * (pairs.shape[1] // 2)
        self.gram_quads += nq
        self.gram_quads2 += nq if self.gram_parts == 2 else 0
        K.block_steps(self.At, self.Vt, self.D, self.geo["m_pad"], pairs, self.W, modes, self.tol,
                      self.cfg.max_inner_sweeps, self.metric, slot, mma=self.mma, pool=self.pool,
                      tol_mode=self.cfg.tol_mode, inner_order=self.inner,
                      gram_parts=self.gram_parts, shared_gpu=self.shared_gpu)

    def next_gram_parts(self) -> int:
        """Quad Gram precision of the next sweep: while the previous sweep
        rotated every pair (far from convergence: the first ~12 of 19 sweeps
        at 16384^2), the couplings only steer rotation angles and the 2-part
        Gram (~2^-16) does; later sweeps need the exact one
        (profiles/r6_gram2; libsvdj_dist: the same rule in svdj_dist_solve).
        SVDJ_DEBUG gram2=0/1 forces it off / on (A/B)."""
        use2 = self.prev_all if self.gram2 is None else self.gram2 == 1
        return 2 if (self.quad and use2) else 3

    def signature(self) -> dict:
        """What a checkpoint must match to be resumed."""
        return {"m": self.m, "n": self.n, "dtype": str(self.dtype), "P": self.geo["P"],
                "W": self.W, "B": self.geo["B"], "rank": self.rank, "want_v": self.want_v}


class DistributedBlockJacobi(Solver):
    name = "distributed-block"

    def __init__(self, config: SolverConfig | None = None, comm: Communicator | None = None):
        super().__init__(config)
        if self.config.chains not in (1, 2):
            raise ValueError(f"SolverConfig.chains must be 1 (blocking exchange) or 2 "
                             f"(pipelined), got {self.config.chains}")
        self.comm = comm or Communicator()
        self._ws = {}  # this solver's kernel workspaces (never shared with another solver)

    # ------------------------------------------------------------ geometry
    def geometry(self, m: int, n: int, dtype: torch.dtype):
        P = self.comm.world
        W = self.config.block or choose_block(dtype, max(n // max(P, 1), 1), m)
        K.check_block(dtype, W)
        # pipelined sweeps split super-blocks in halves: k = B/W must be even
        parts = 2 if self.config.chains == 2 else 1
        q = 2 * parts * P * W
        ncols = round_up(max(n, q), q)
        m_pad = pad_rows(m)
        # quad steps need k % 4 == 0: a pipelined fp32/bf16 W = 64 count that
        # lands on k % 4 == 2 where the quad rule holds takes one more q of
        # zero columns (<= 6 % more columns there; quad steps save 20-25 % of
        # a solve).  Same rule as libsvdj_dist's svdj_dist_geometry.
        k = ncols // (2 * P * W)
        if parts == 2 and dtype != torch.float64 and W == 64 and k % 4 == 2 \
                and quad_size_rule((k + 2) // 2, m_pad, P) and debug_knob("quad_pad", 1) != 0:
            ncols += q
        B = ncols // (2 * P)
        return {"P": P, "W": W, "ncols": ncols, "B": B, "k": B // W, "m_pad": m_pad,
                "n_v": pad_rows(ncols)}

    # --------------------------------------------------------------- solve
    _DT_CODE = {torch.float32: 0, torch.float64: 1, torch.bfloat16: 2}

    def solve(self, A: torch.Tensor | None = None, jobu=SVDOptions.AllVec,
              jobv=SVDOptions.AllVec, m: int | None = None, n: int | None = None,
              dtype: torch.dtype | None = None, generator=None, gather: bool = True,
              time_only: bool = False) -> SVDResult:
        """Distributed SVD.  ``dtype`` is the problem precision (fp32, fp64 or
        bf16 = bf16 data on fp32 master copies and bf16 matrix cores).  Tall
        inputs (m >= qr_ratio n, or precondition="qr") are QR-preconditioned
        with a row-distributed CholeskyQR2 (``precondition.dist_qr``: local
        Gram, RCCL all-reduce, replicated Cholesky, local TRSM); the sweeps
        then run on the replicated R (n x n) and U = Q U_R is a local GEMM
        per row block.  That path returns U as this rank's row block
        (``info["u_rows"]``) with sigma and V complete on every rank, or U
        complete on rank 0 with ``gather``."""
        comm, cfg = self.comm, self.config
        dev = comm.device
        jobu, jobv = SVDOptions.parse(jobu), SVDOptions.parse(jobv)
        # ---- problem description (root-owned input is broadcast as shape)
        if A is not None:
            m, n = A.shape
            dtype = dtype or cfg.dtype or A.dtype
        dtype = dtype or cfg.dtype or torch.float32
        if dtype not in self._DT_CODE:
            dtype = torch.float32
        hdr = torch.tensor([m or 0, n or 0, self._DT_CODE[dtype]], dtype=torch.int64, device=dev)
        if generator is None and comm.distributed:
            comm.broadcast(hdr, 0)
        m, n = int(hdr[0]), int(hdr[1])
        dtype = {0: torch.float32, 1: torch.float64, 2: torch.bfloat16}[int(hdr[2])]
        if m < n:
            raise ValueError("distributed path expects m >= n")
        work = torch.float64 if dtype == torch.float64 else torch.float32
        if not pre.use_qr(cfg, m, n):
            res = self._solve(A, jobu, jobv, m, n, dtype, generator, gather, time_only)
            res.info["flops"] = pre.flops(m, n, res.sweeps, False)
            return res
        # ---- QR-preconditioned tall-skinny solve, row-distributed: rank g
        # owns rows [r0, r1) of A and of U; R (n x n) is replicated
        P, g = comm.world, comm.rank
        r0, r1 = g * m // P, (g + 1) * m // P
        t_qr = time.perf_counter()
        if generator is not None:
            A_loc = torch.cat([generator(c0, min(c0 + 1024, n))[r0:r1].to(device=dev, dtype=work)
                               for c0 in range(0, n, 1024)], dim=1)
        else:
            A_loc = dataio.scatter_rows(comm, A, m, n, work)
        out = pre.dist_qr(A_loc, work, comm)
        if out is None:  # too ill-conditioned for CholeskyQR2: replicated Householder
            Qf, R = pre.qr(dataio.allgather_rows(comm, A_loc, m, n), work, method="householder")
            Q_loc, Lt = Qf[r0:r1].contiguous(), None
            del Qf
        else:
            Q_loc, R, Lt = out
        del A_loc
        if cfg.comm_timing and dev.type == "cuda":  # phase timing costs a sync
            torch.cuda.synchronize(dev)
        t_qr = time.perf_counter() - t_qr
        res = self._solve(None, jobu, jobv, n, n, dtype, lambda c0, c1: R[:, c0:c1], False,
                          time_only)
        want_u = jobu != SVDOptions.NoVec
        U_R, S, V = dataio.allgather_columns(comm, res, n, want_u, jobv != SVDOptions.NoVec)
        U_loc = pre.apply_q(Q_loc, Lt, U_R).to(U_R.dtype) if want_u else None
        res.S, res.V = S, V
        res.info.update(precondition="qr", flops=pre.flops(m, n, res.sweeps, True),
                        qr_seconds=round(t_qr, 4),
                        distributed_output="rows" if P > 1 and not gather else False,
                        u_rows=(r0, r1))
        if gather and P > 1 and want_u:
            U_loc = dataio.gather_rows(comm, U_loc, m, n)
        res.U = U_loc
        if dtype == torch.bfloat16 and (gather or P == 1):
            res.U = res.U.to(torch.bfloat16) if res.U is not None else None
            res.V = res.V.to(torch.bfloat16) if res.V is not None else None
        return res

    def roundtrip(self, A: torch.Tensor | None, m: int, n: int, dtype=torch.float64):
        """Scatter root-owned A over the ranks' super-blocks and gather it back
        unchanged (``dataio.roundtrip``; rank 0 returns it, others None)."""
        return dataio.roundtrip(self.comm, self.geometry(m, n, dtype), A, m, n, dtype)

    def _solve(self, A, jobu, jobv, m, n, pdtype, generator, gather, time_only) -> SVDResult:
        comm, cfg = self.comm, self.config
        dev = comm.device
        s = self._resolve_rules(m, n, pdtype, jobu, jobv)
        P, k = s.geo["P"], s.geo["k"]
        if s.pipelined:
            splan = sweep_plan(P, k, s.tour.xslot[:, s.rank], quad=s.quad)
        else:
            plans = distributed_sweep_plan(P, k)
            dev_pairs = [torch.from_numpy(p.pairs).to(dev) for p in plans]
        streams = self._chain_streams(dev) if (s.pipelined and dev.type == "cuda") else None
        self._allocate(s, A, generator)
        bufs = None if s.pipelined else self._staging(s)
        start = self._restore(s)
        sync = (lambda: torch.cuda.synchronize(dev)) if dev.type == "cuda" else (lambda: None)
        sync()
        t0 = time.perf_counter()
        s.work_acc = torch.zeros(2, dtype=torch.float64, device=s.metric.device)
        ex = PipelineExecutor(comm, streams, s.At, s.Vt, s.D, k, s.W, s.tour,
                              timing=cfg.comm_timing, parts=splan.parts,
                              exchange=cfg.exchange) if s.pipelined else None
        s.prev_all = start == 0
        for sw in range(start, cfg.max_sweeps):
            s.gram_parts = s.next_gram_parts()
            with trace_range(f"svdj.sweep{sw}"):
                K.reset_metric(s.metric)
                if s.pipelined:
                    self._sweep_pipelined(s, ex, splan)
                else:
                    self._sweep_blocking(s, plans, dev_pairs, bufs)
                vals = self._reduce(s)
            if self._stop_test(s, vals, t0):
                break
            self._checkpoint(s, ex)
            self._fault_point(s.sweeps)
        return self._finish(s, ex, sync, t0, gather, time_only)

    # ------------------------------------------------- the parts of a solve
    def _resolve_rules(self, m, n, pdtype, jobu, jobv) -> _Solve:
        """Geometry, kernels and issue rules of this solve (host only;
        libsvdj_dist: resolve_rules)."""
        comm, cfg = self.comm, self.config
        dtype = torch.float64 if pdtype == torch.float64 else torch.float32
        geo = self.geometry(m, n, dtype)
        P, W, k, m_pad = geo["P"], geo["W"], geo["k"], geo["m_pad"]
        mma = cfg.mma if cfg.mma != "auto" else (
            "bf16x3" if pdtype == torch.bfloat16 else choose_mma(dtype, W))
        pipelined = cfg.chains == 2
        quad = pipelined and resolve_quad(cfg.quad, dtype, W, mma, k, P, m_pad)
        # one GPU: the two chains' parallel tasks as single launches where
        # that pays (models/block.py choose_merged)
        merged = pipelined and comm.device.type == "cuda" and choose_merged(
            P if comm.distributed else 1, k, quad)
        return _Solve(
            cfg=cfg, pool=self._ws, rank=comm.rank, tour=tournament(P), geo=geo, pdtype=pdtype,
            dtype=dtype, tol=self.tolerance(pdtype, m), want_u=jobu != SVDOptions.NoVec,
            want_v=jobv != SVDOptions.NoVec, pipelined=pipelined, W=W, mma=mma,
            # pairs per cross step: half super-blocks (pipelined) or whole ones
            inner=resolve_inner_order(cfg.inner_order, W, k // 2 if pipelined else k, dtype),
            quad=quad, merged=merged,
            # the two chains on their own streams: the quad apply leaves the other
            # chain CUs (svdj_block_steps bit 9; libsvdj_dist the same)
            shared_gpu=pipelined and quad and not (merged and not comm.distributed),
            gram2=debug_knob("gram2"), m=m, n=n)

    def _allocate(self, s: _Solve, A, generator):
        """Resident state: slot j holds super-block held[j] (A columns, V =
        identity columns, squared norms), the stop metric and its floor."""
        comm, dev = self.comm, self.comm.device
        B, m_pad = s.geo["B"], s.geo["m_pad"]
        s.phys = [[int(s.tour.held[0, h, 0]), int(s.tour.held[0, h, 1])]
                  for h in range(s.geo["P"])]
        # pipelined multi-rank storage carries one spare half buffer per half
        # index (the exchanges receive in place, plan.HalfLayout); rows
        # [0, 2B) are the canonical slots at the start and after the solve
        ncol = PipelineExecutor.storage_columns(B, comm.distributed) if s.pipelined else 2 * B
        s.At = torch.zeros(ncol, m_pad, dtype=s.dtype, device=dev)
        s.Vt = torch.zeros(ncol, s.geo["n_v"], dtype=s.dtype, device=dev) if s.want_v else None
        held = s.phys[s.rank]
        dataio.distribute(comm, A, generator, s.At, held, s.m, s.n, B)
        if s.want_v:
            for j in range(2):
                K.set_identity(s.Vt[j * B:(j + 1) * B], B, held[j] * B)
        s.D = K.col_norms2(s.At, m_pad)
        s.metric = K.new_metric(dev)
        # scale of the negligible-column floor: the largest squared column norm
        # of the whole matrix (one all-reduce at setup)
        dmax = float(s.D[:2 * B].max()) if s.D.numel() else 1.0
        if comm.distributed:
            dmax = comm.max_over_ranks(dmax)
        K.set_norm_floor(s.metric, s.dtype, m_pad, dmax)
        comm.barrier()

    def _restore(self, s: _Solve) -> int:
        """Resume from this rank's checkpoint if it matches; the first sweep to run."""
        cfg, B = self.config, s.geo["B"]
        st = ckpt.load(cfg.checkpoint_dir, s.rank, self.comm.device) if cfg.checkpoint_dir else None
        if st is None or not ckpt.compatible(st, s.signature()):
            return 0
        s.At[:2 * B].copy_(st["At"])
        s.D[:2 * B].copy_(st["D"])
        if s.want_v:
            s.Vt[:2 * B].copy_(st["Vt"])
        s.phys = [list(x) for x in st["phys"]]
        s.hist = list(st["hist"])
        s.sweeps = int(st["sweep"])
        return s.sweeps

    def _sweep_pipelined(self, s: _Solve, ex: PipelineExecutor, splan):
        """One sweep of the half-block plan (chains=2): merged single launches
        on one GPU where the rule says so, else two chains with exchanges."""
        if s.merged and not self.comm.distributed:
            ex.run_merged(splan, s.run_steps)
        else:
            s.t_comm += ex.run(splan, s.run_steps, s.phys, merge=s.merged)

    def _staging(self, s: _Solve):
        """The block that the blocking exchange (chains=1) receives into."""
        B, dev = s.geo["B"], self.comm.device
        return (torch.empty(B, s.geo["m_pad"], dtype=s.dtype, device=dev),
                torch.empty(B, s.geo["n_v"], dtype=s.dtype, device=dev) if s.want_v else None,
                torch.empty(B, dtype=s.dtype, device=dev))

    def _sweep_blocking(self, s: _Solve, plans, dev_pairs, bufs):
        """One sweep with whole super-blocks exchanged between rounds
        (chains=1): round 0's round robin, then exchange + cross per round."""
        for r in range(s.tour.rounds):
            if r > 0 and s.geo["P"] > 1:
                tc = time.perf_counter()
                with trace_range("svdj.exchange"):
                    self._exchange(s, r, bufs)
                s.t_comm += time.perf_counter() - tc
            with trace_range(f"svdj.round{r}"):
                s.run_steps(dev_pairs[r], plans[r].modes, 0)

    def _exchange(self, s: _Solve, r: int, bufs):
        """Round r of the tournament: this GPU sends the super-block in slot
        xslot[r][g] (A columns, V columns, squared norms) to send_to[r][g] and
        receives its replacement from recv_from[r][g] -- one grouped RCCL
        send/recv.  ``s.phys`` (every GPU's placement) is advanced."""
        g, tour, B = s.rank, s.tour, s.geo["B"]
        At, Vt, D = s.At, s.Vt, s.D
        rA, rV, rD = bufs
        x = int(tour.xslot[r, g])
        dst, src = int(tour.send_to[r, g]), int(tour.recv_from[r, g])
        sl = slice(x * B, (x + 1) * B)
        sends = [(At[sl], dst), (D[sl], dst)]
        recvs = [(rA, src), (rD, src)]
        if Vt is not None:
            sends.append((Vt[sl], dst))
            recvs.append((rV, src))
        # gloo on device tensors (rehearsal) is not stream-ordered, see pipeline.py
        host_sync = At.is_cuda and not getattr(self.comm, "async_device", False)
        if host_sync:
            torch.cuda.synchronize(At.device)
        self.comm.sendrecv(sends, recvs)
        if host_sync:
            torch.cuda.synchronize(At.device)
        At[sl].copy_(rA)
        D[sl].copy_(rD)
        if Vt is not None:
            Vt[sl].copy_(rV)
        advance_placement(tour, r, s.phys)

    def _reduce(self, s: _Solve):
        """Global (max off value, max effective sine, rotated pairs, column
        rotations) of the sweep (all-reduces instead of the reference's
        discarded convergence value, main.cu:710); libsvdj_dist: reduce."""
        v = K.metric_stop_values(s.metric)
        vals = self.comm.allreduce_stop(v[0], v[1], v[2], v[3])
        nbt = 2 * s.geo["P"] * s.geo["k"]
        s.prev_all = int(vals[2]) >= nbt * (nbt - 1) // 2
        s.work_acc += K.metric_work(s.metric)
        return vals

    def _stop_test(self, s: _Solve, vals, t0) -> bool:
        """Record the sweep; True when the solve has converged.  Every rank
        sees the same all-reduced values: the same decision."""
        cfg = self.config
        mx, ms, nrot, ncr = vals
        s.hist.append(mx)
        s.sweeps += 1
        if cfg.progress and s.rank == 0:
            print(f"[svdj] sweep {s.sweeps}: off {mx:.3e}, eff sin {ms:.3e}, rotated pairs "
                  f"{int(nrot)}, rotations {int(ncr)}, {time.perf_counter() - t0:.2f} s",
                  file=sys.stderr, flush=True)
        stop = K.sweep_converged(mx, ms, nrot, ncr, s.tol, cfg.tol_mode, cfg.stop_rule)
        if stop:
            s.stop_reason = "no_rotation" if stop == 1 else "second_order"
        return bool(stop)

    def _checkpoint(self, s: _Solve, ex):
        """Save every ``checkpoint_every`` sweeps.  The next sweep replays the
        same exchange pattern from the current placement: the schedule only
        depends on positions, so every physical pair still meets exactly once
        per sweep."""
        cfg, B = self.config, s.geo["B"]
        if not (cfg.checkpoint_dir and cfg.checkpoint_every
                and s.sweeps % cfg.checkpoint_every == 0):
            return
        if ex is not None:
            ex.canonicalize()
        ckpt.save(cfg.checkpoint_dir, s.rank,
                  {**s.signature(), "At": s.At[:2 * B],
                   "Vt": s.Vt[:2 * B] if s.want_v else torch.empty(0), "D": s.D[:2 * B],
                   "phys": s.phys, "hist": s.hist, "sweep": s.sweeps})

    def _finish(self, s: _Solve, ex, sync, t0, gather, time_only) -> SVDResult:
        """Canonical layout, sigma and U scaling, ``info``, and the gather."""
        cfg, B, m_pad = self.config, s.geo["B"], s.geo["m_pad"]
        converged = s.stop_reason is not None
        if converged and cfg.checkpoint_dir:
            ckpt.clear(cfg.checkpoint_dir, s.rank)
        At, Vt = s.At, s.Vt
        if ex is not None:
            ex.canonicalize()
            At = At[:2 * B]
            Vt = Vt[:2 * B] if s.want_v else None
        sigma_loc = K.finalize(At, m_pad, scale_u=s.want_u)
        sync()
        t_total = time.perf_counter() - t0
        wa = s.work_acc.cpu()
        info_work = {"apply_mfma": int(wa[0]) * 24, "apply_tiles": int(wa[1]),
                     "gram_quads": int(s.gram_quads), "gram_quads2": int(s.gram_quads2),
                     "m_pad": m_pad}
        info = {"tol": s.tol, "converged": converged, "stop_reason": s.stop_reason,
                "work": info_work, "stop_rule": cfg.stop_rule, "dtype": str(s.pdtype),
                "geometry": s.geo, "mma": s.mma, "inner_order": s.inner, "quad": s.quad,
                "merged_chains": bool(s.pipelined and s.merged),
                "exchange": ex.exchange if ex is not None else "direct",
                "comm_seconds": s.t_comm, "rank": s.rank, "held": list(s.phys[s.rank])}
        if ex is not None and s.geo["P"] > 1:
            info["comm"] = ex.comm_summary()
        if time_only or not gather:
            return SVDResult(At if s.want_u else None, sigma_loc, Vt, s.sweeps, s.hist, t_total,
                             self.name, {**info, "distributed_output": True})
        U, S, V = dataio.gather(self.comm, At, Vt, sigma_loc, info["held"], s.m, s.n, B, s.dtype,
                                s.want_v, s.want_u)
        if s.pdtype == torch.bfloat16:  # bf16 in/out (sigma stays fp32)
            U = U.to(torch.bfloat16) if U is not None else None
            V = V.to(torch.bfloat16) if V is not None else None
        return SVDResult(U, S, V, s.sweeps, s.hist, t_total, self.name, info)

    def _fault_point(self, sweeps: int):
        """Fault injection for failure-detection tests: SolverConfig.extra
        ["fault_exit"] = (rank, sweep) makes that rank exit abruptly (no
        cleanup, exit status 17) after that sweep, like a crashed peer."""
        f = self.config.extra.get("fault_exit") if self.config.extra else None
        if f and int(f[0]) == self.comm.rank and int(f[1]) == sweeps:
            print(f"[svdj] fault injection: rank {self.comm.rank} exits after sweep {sweeps}",
                  file=sys.stderr, flush=True)
            os._exit(17)

    _STREAMS: dict = {}  # device -> the two chain streams, shared by every solver in the process

    def _chain_streams(self, dev):
        """The chain streams are created ONCE per device and process and
        reused by every solver (each svd() call builds a new one): torch
        hands out pool streams round robin, and HIP binds each new stream to
        one of GPU_MAX_HW_QUEUES (4) hardware queues, so fresh streams per
        solve can land on the same queue as each other and serialise.
        Solves in one process are sequential, so sharing is safe."""
        key = str(dev)
        if key not in DistributedBlockJacobi._STREAMS:
            DistributedBlockJacobi._STREAMS[key] = [torch.cuda.Stream(dev) for _ in range(2)]
        return DistributedBlockJacobi._STREAMS[key]
