"""Input families with structure, and the metrics that see it (CPU, torch and
numpy only; shared by test_spectra_cpu.py and test_gpu_spectra.py).

A U(0,1) matrix has one singular value near sqrt(mn)/2 and a bulk 15 to 30
times smaller, so "sigma error over sigma_max" and the Frobenius residual say
little about the bulk and nothing about small columns.  The families here put
the structure where a one-sided Jacobi differs from a QR-based SVD:

  graded     A = B D, unit columns of U(-0.5,0.5) times logspace(0,-6) shuffled
  lowrank    the exact product of an m x n/2 and an n/2 x n factor
  dupzero    U(0,1), every 8th column zero, every 8th (offset 4) a copy of
             its left neighbour
  clustered  half the singular values 1, half 1e-3
  triu       the reference project's own upper-triangular input (square)

Each is ``family(m, n, dtype, seed) -> A`` built in fp64 and rounded to dtype.
``metrics`` measures a result in fp64 on the CPU against a reference spectrum
that never comes from the code under test.
"""
import numpy as np
import torch

import svdj

F32, F64 = torch.float32, torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def graded(m, n, dtype, seed):
    g = _gen(seed)
    B = torch.rand(m, n, dtype=F64, generator=g) - 0.5
    B = B / B.norm(dim=0)
    d = torch.logspace(0, -6, n, dtype=F64)[torch.randperm(n, generator=g)]
    return (B * d).to(dtype)


def lowrank(m, n, dtype, seed):
    g = _gen(seed)
    L = torch.rand(m, n // 2, dtype=F64, generator=g) - 0.5
    R = torch.rand(n // 2, n, dtype=F64, generator=g) - 0.5
    return (L @ R).to(dtype)


def dupzero_columns(n):
    """(zero columns, duplicate columns) of ``dupzero`` at n columns."""
    return list(range(0, n, 8)), list(range(4, n, 8))


def dupzero(m, n, dtype, seed):
    A = torch.rand(m, n, dtype=F64, generator=_gen(seed))
    zero, dup = dupzero_columns(n)
    A[:, zero] = 0.0
    A[:, dup] = A[:, [j - 1 for j in dup]]
    return A.to(dtype)


def clustered_spectrum(n):
    s = torch.full((n,), 1e-3, dtype=F64)
    s[: n // 2] = 1.0
    return s


def clustered(m, n, dtype, seed):
    return svdj.utils.inputs.with_spectrum(m, n, clustered_spectrum(n), dtype=dtype, seed=seed)


def triu(m, n, dtype, seed):
    assert m == n, "triu is square"
    return svdj.utils.inputs.reference_triu(n).to(dtype)  # the reference's own seed


FAMILIES = {"graded": graded, "lowrank": lowrank, "dupzero": dupzero, "clustered": clustered,
            "triu": triu}


def rank_of(family, n):
    """The rank a family has by construction at n columns (None: full, or
    for triu numerically undetermined)."""
    if family == "lowrank":
        return n // 2
    if family == "dupzero":
        zero, dup = dupzero_columns(n)
        return n - len(zero) - len(dup)
    return None


def has_longdouble():
    return float(np.finfo(np.longdouble).eps) < 1e-18


def sigma_longdouble(A, max_sweeps=40, with_columns=False):
    """Singular values of ``A`` (descending, numpy.longdouble) by a plain
    one-sided Jacobi in extended precision: round-robin ordering, the n/2
    disjoint pairs of a step rotated together by array operations, until no
    coupling exceeds 1e-18 sqrt(g_pp g_qq).  ``with_columns`` also returns the
    rotated matrix (rows = columns of A V) for the orthogonality check."""
    ld = np.longdouble
    assert has_longdouble(), "numpy.longdouble is not extended precision here"
    X = np.ascontiguousarray(A.detach().cpu().double().numpy().T).astype(ld)  # row j = column j
    n = X.shape[0]
    if n % 2:
        X = np.concatenate([X, np.zeros((1, X.shape[1]), dtype=ld)])
    nn = X.shape[0]
    tol = ld(1e-18)
    for _ in range(max_sweeps):
        order = list(range(nn))
        worst = ld(0)
        for _step in range(nn - 1):
            p = np.array(order[: nn // 2])
            q = np.array(order[nn // 2:][::-1])
            xp, xq = X[p], X[q]
            gpp = (xp * xp).sum(1)
            gqq = (xq * xq).sum(1)
            gpq = (xp * xq).sum(1)
            den = np.sqrt(gpp * gqq)
            rel = np.where(den > 0, np.abs(gpq) / np.where(den > 0, den, ld(1)), ld(0))
            worst = max(worst, rel.max())
            rot = rel > tol
            if rot.any():
                safe = np.where(rot, gpq, ld(1))
                zeta = (gqq - gpp) / (ld(2) * safe)
                t = np.sign(zeta) / (np.abs(zeta) + np.sqrt(ld(1) + zeta * zeta))
                t = np.where(zeta == 0, ld(1), t)
                c = ld(1) / np.sqrt(ld(1) + t * t)
                s = c * t
                c = np.where(rot, c, ld(1))[:, None]
                s = np.where(rot, s, ld(0))[:, None]
                X[p] = c * xp - s * xq
                X[q] = s * xp + c * xq
            order = [order[0]] + [order[-1]] + order[1:-1]
        if worst <= tol:
            break
    else:
        raise RuntimeError("sigma_longdouble did not converge")
    X = X[:n]
    sig = np.sqrt((X * X).sum(1))
    idx = np.argsort(-sig)
    return (sig[idx], X[idx]) if with_columns else sig[idx]


def reference_sigma(A, family):
    """fp64 reference spectrum (descending) of the rounded matrix: LAPACK in
    fp64, except for fp64 ``graded`` where LAPACK's own ~1e-10 relative error
    on the small values would swamp the measurement: there ``sigma_longdouble``
    (None when longdouble is not extended precision: the caller skips
    ``sig_rel`` with that reason)."""
    if family == "graded" and A.dtype == F64:
        if not has_longdouble():
            return None
        return torch.from_numpy(sigma_longdouble(A).astype(np.float64))
    return torch.linalg.svdvals(A.detach().cpu().double())


def significant(ref, family, m, n, dtype):
    """Indices (into the descending reference spectrum) whose relative
    accuracy is claimed: from the reference and the construction only."""
    k = ref.numel()
    if family in ("graded", "clustered"):
        return torch.arange(k)
    if family in ("lowrank", "dupzero"):
        return torch.arange(rank_of(family, n))
    if family == "triu":
        return torch.nonzero(ref >= ref[0] * m * torch.finfo(dtype).eps).flatten()
    raise ValueError(family)


METRICS = ("sig_rel", "sig_abs", "colres", "orth_v", "orth_u")


def metrics(A, U, S, V, family, ref=None, converged=None, sweeps=None, lapack_ref=None):
    """Everything in fp64 on the CPU; columns of U and V follow S sorted
    descending.  ``ref``: the reference spectrum (``reference_sigma``), computed
    here when not given; for fp64 ``graded`` without an extended-precision
    longdouble, ``sig_rel`` is None and ``sig_abs`` uses LAPACK."""
    dtype = A.dtype
    A, U, S, V = (t.detach().cpu().double() for t in (A, U, S, V))
    m, n = A.shape
    if ref is None:
        ref = reference_sigma(A.to(dtype), family)
    finite = all(bool(torch.isfinite(t).all()) for t in (U, S, V))
    order = torch.argsort(S, descending=True)
    S, U, V = S[order], U[:, order], V[:, order]
    abs_ref = ref if ref is not None else (
        lapack_ref if lapack_ref is not None else torch.linalg.svdvals(A))
    K = significant(abs_ref, family, m, n, dtype)
    out = {}
    out["sig_rel"] = None if ref is None else float(((S[K] - ref[K]).abs() / ref[K]).max())
    out["sig_abs"] = float((S - abs_ref).abs().max() / abs_ref[0])
    E = (U * S) @ V.t() - A
    cn = A.norm(dim=0)
    nz = cn > 0
    out["colres"] = float((E.norm(dim=0)[nz] / cn[nz]).max())
    out["fro"] = float(E.norm() / A.norm())  # for contrast: what hides small columns
    out["orth_v"] = float((V.t() @ V - torch.eye(V.shape[1], dtype=F64)).abs().max())
    UK = U[:, K]
    out["orth_u"] = float((UK.t() @ UK - torch.eye(K.numel(), dtype=F64)).abs().max())
    r = rank_of(family, n)
    out["tail"] = float(S[r:].abs().max() / abs_ref[0]) if r is not None and r < n else None
    out["finite"] = finite
    out["converged"] = None if converged is None else bool(converged)
    out["sweeps"] = None if sweeps is None else int(sweeps)
    return out


def metrics_of(A, res, family, ref=None):
    """``metrics`` of an SVDResult."""
    return metrics(A, res.U, res.S, res.V, family, ref=ref, converged=res.converged,
                   sweeps=res.sweeps)


def worst(ms):
    """Per key the worst value over a list of metric dicts (a batch)."""
    out = {}
    for k in ms[0]:
        vals = [d[k] for d in ms]
        if k == "sweeps":
            out[k] = vals
        elif k in ("finite", "converged"):
            out[k] = None if any(v is None for v in vals) else all(vals)
        else:
            out[k] = None if any(v is None for v in vals) else max(vals)
    return out


def within(got, want, f, names=METRICS):
    """[(name, got, want)] for every metric of ``names`` where ``got`` exceeds
    f times the reference engine's value on the same matrix (the bound rule of
    the spectra tests).  A metric that is None on either side (fp64 graded
    sig_rel without an extended-precision longdouble) is not compared."""
    bad = []
    for k in names:
        if got[k] is None or want[k] is None:
            continue
        if not got[k] <= f * want[k]:
            bad.append((k, got[k], want[k]))
    return bad
