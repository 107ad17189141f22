"""Data movement of the distributed solver: root-owned input scattered over
the ranks' resident super-blocks (or row blocks, for the QR-preconditioned
path) and results gathered back.  Functions of the communicator and the
geometry only; every rank calls them in the same order (grouped batches)."""
from __future__ import annotations

import torch

from .schedule import tournament


# ------------------------------------------------------ row-distributed QR I/O
def _row_range(comm, h: int, m: int):
    """Rows [r0, r1) of an m-row matrix that rank h owns."""
    return h * m // comm.world, (h + 1) * m // comm.world


def scatter_rows(comm, A, m, n, dtype):
    """Root-owned A: rank 0 sends every rank its row block (one grouped batch)."""
    r0, r1 = _row_range(comm, comm.rank, m)
    if not comm.distributed:
        return A.to(device=comm.device, dtype=dtype)
    if comm.rank == 0:
        Ad = A.to(device=comm.device, dtype=dtype)
        sends = [(Ad[slice(*_row_range(comm, h, m))].contiguous(), h)
                 for h in range(1, comm.world)]
        comm.sendrecv(sends, [])
        return Ad[r0:r1].contiguous()
    out = torch.empty(r1 - r0, n, dtype=dtype, device=comm.device)
    comm.sendrecv([], [(out, 0)])
    return out


def allgather_rows(comm, A_loc, m, n):
    """Every rank's row block, assembled on every rank (Householder fallback)."""
    if not comm.distributed:
        return A_loc
    count = [b - a for a, b in (_row_range(comm, h, m) for h in range(comm.world))]
    buf = torch.zeros(max(count), n, dtype=A_loc.dtype, device=A_loc.device)
    buf[:A_loc.shape[0]] = A_loc
    allr = comm.allgather(buf)
    return torch.cat([allr[h, :count[h]] for h in range(comm.world)])


def gather_rows(comm, U_loc, m, n):
    """Row blocks of U to rank 0 (one grouped batch); None on other ranks."""
    if comm.rank != 0:
        comm.sendrecv([(U_loc.contiguous(), 0)], [])
        return None
    parts = [U_loc]
    recvs = []
    for h in range(1, comm.world):
        a, b = _row_range(comm, h, m)
        t = torch.empty(b - a, n, dtype=U_loc.dtype, device=U_loc.device)
        parts.append(t)
        recvs.append((t, h))
    comm.sendrecv([], recvs)
    return torch.cat(parts)


def allgather_columns(comm, res, n, want_u, want_v):
    """All of U_R (n x n), sigma (n) and V (n x n) on every rank, from each
    rank's resident super-block columns (transposed layout)."""
    geo = res.info["geometry"]
    B = geo["B"]
    held = torch.tensor(res.info["held"], dtype=torch.int64, device=res.S.device)
    ids = comm.allgather(held).cpu()
    S_all = comm.allgather(res.S)
    U_all = comm.allgather(res.U) if want_u else None
    V_all = comm.allgather(res.V) if want_v else None
    ncols = 2 * B * comm.world
    S = torch.zeros(ncols, dtype=res.S.dtype, device=res.S.device)
    Ut = torch.zeros(ncols, n, dtype=res.S.dtype, device=res.S.device) if want_u else None
    Vt = torch.zeros(ncols, n, dtype=res.S.dtype, device=res.S.device) if want_v else None
    for h in range(comm.world):
        for s_ in range(2):
            sb = int(ids[h, s_])
            dst, src = slice(sb * B, (sb + 1) * B), slice(s_ * B, (s_ + 1) * B)
            S[dst] = S_all[h, src]
            if want_u:
                Ut[dst] = U_all[h, src, :n]
            if want_v:
                Vt[dst] = V_all[h, src, :n]
    return (Ut[:n].t() if want_u else None), S[:n], (Vt[:n].t() if want_v else None)


# ------------------------------------------ resident super-blocks (columns)
def _fill(buf, held, columns, m, n, B):
    """Super-blocks ``held`` into buf's two slots; ``columns(c0, c1)`` is (m, c1 - c0)."""
    for s in range(2):
        c0, c1 = held[s] * B, min((held[s] + 1) * B, n)
        if c1 > c0:
            buf[s * B:s * B + (c1 - c0), :m].copy_(columns(c0, c1).t())


def distribute(comm, A, generator, At, held, m, n, B):
    """Fill At's canonical slots with this rank's super-blocks ``held``: from
    ``generator(c0, c1)`` on every rank, or from rank 0's A."""
    if generator is not None:
        return _fill(At, held, generator, m, n, B)
    if not comm.distributed:
        return _fill(At, held, lambda c0, c1: A[:, c0:c1], m, n, B)
    # Root-owned input: rank 0 packs every rank's two super-blocks and
    # posts all P-1 sends as ONE grouped batch, so the transfers run
    # concurrently over the P-1 xGMI links (the reference's scatter is a
    # serial loop of blocking sends, main.cu:582-619).
    if comm.rank != 0:
        return comm.sendrecv([], [(At[:2 * B], 0)])
    tour = tournament(comm.world)
    Ad = A.to(device=At.device, dtype=At.dtype)
    sends = []
    for dst in range(comm.world):
        buf = torch.zeros_like(At[:2 * B]) if dst != 0 else At
        _fill(buf, tour.held[0, dst].tolist(), lambda c0, c1: Ad[:, c0:c1], m, n, B)
        if dst != 0:
            sends.append((buf, dst))
    comm.sendrecv(sends, [])


def roundtrip(comm, geo, A: torch.Tensor | None, m: int, n: int, dtype=torch.float64):
    """Scatter root-owned A over the ranks' resident super-blocks and gather
    it back unchanged (rank 0 returns the (m, n) matrix, others None).

    The reference names this check ``test_local_matrix_distribution_*`` and has
    the comparisons commented out (reference main.cu:630-643, 866-877,
    1605-1609); here the tests call DistributedBlockJacobi.roundtrip."""
    B, m_pad = geo["B"], geo["m_pad"]
    held = [int(tournament(comm.world).held[0, comm.rank, s]) for s in range(2)]
    At = torch.zeros(2 * B, m_pad, dtype=dtype, device=comm.device)
    distribute(comm, A, None, At, held, m, n, B)
    sigma = torch.zeros(2 * B, dtype=dtype, device=comm.device)
    U, _, _ = gather(comm, At, None, sigma, held, m, n, B, dtype, False, True)
    return U


def gather(comm, At, Vt, sigma, held, m, n, B, dtype, want_v, want_u):
    ids = torch.tensor(held, dtype=torch.int64, device=At.device)
    if not comm.distributed:
        parts = [(ids, At, Vt, sigma)]
    elif comm.rank == 0:
        # all P-1 ranks' blocks arrive in one grouped batch (concurrent
        # links; the reference gathers rank by rank, main.cu:854-936)
        parts = [(ids, At, Vt, sigma)]
        recvs = []
        for src in range(1, comm.world):
            rid = torch.empty_like(ids)
            rA, rS = torch.empty_like(At), torch.empty_like(sigma)
            rV = torch.empty_like(Vt) if want_v else None
            recvs += [(rid, src), (rA, src), (rS, src)] + ([(rV, src)] if want_v else [])
            parts.append((rid, rA, rV, rS))
        comm.sendrecv([], recvs)
    else:
        sends = [(ids, 0), (At, 0), (sigma, 0)] + ([(Vt, 0)] if want_v else [])
        comm.sendrecv(sends, [])
        return None, None, None
    ncols = 2 * B * comm.world
    Ut = torch.zeros(ncols, m, dtype=dtype, device=At.device)
    Vfull = torch.zeros(ncols, Vt.shape[1], dtype=dtype, device=At.device) if want_v else None
    S = torch.zeros(ncols, dtype=dtype, device=At.device)
    for rid, a, v, s_ in parts:
        for s in range(2):
            sb = int(rid[s])
            Ut[sb * B:(sb + 1) * B] = a[s * B:(s + 1) * B, :m]
            S[sb * B:(sb + 1) * B] = s_[s * B:(s + 1) * B]
            if want_v:
                Vfull[sb * B:(sb + 1) * B] = v[s * B:(s + 1) * B]
    U = Ut[:n].t() if want_u else None
    V = Vfull[:n, :n].t() if want_v else None
    return U, S[:n], V
