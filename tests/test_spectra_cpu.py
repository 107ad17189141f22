"""The instruments of the spectra tests (tests/_spectra.py), checked without a
GPU: the input families have the structure they claim, the extended-precision
reference agrees with LAPACK, each new metric catches a planted fault that the
sigma_max and Frobenius metrics let through, and the CPU oracle and the CPU
emulation of the block path meet on every family the bound rule that
test_gpu_spectra.py applies to the GPU engines.

Sweeps to convergence measured on the CPU (oracle / block path, block=32,
precondition="none"); recorded, not asserted -- the block emulation is slow:

  graded 520 x 384            fp32  8 /  7    fp64  9 /  8
  triu 256                    fp32 22 / 24    fp64 23 / 25
  clustered 520 x 384         fp32 15 / 23    fp64 28 / 40
  lowrank 200 x 128           fp32 16 / 26    fp64 19 / 47
  lowrank 520 x 384           fp32 18 / 30    fp64 23 / 53

The block path's 2.3 to 2.5 times the oracle's sweeps on rank-deficient fp64
input is explained under "Stop test" in README.md: the cause is not the stop
rule.
"""
import json

import numpy as np
import pytest
import torch

import svdj

import _spectra as sp

F32, F64 = torch.float32, torch.float64
NAME = {F32: "fp32", F64: "fp64"}


# ------------------------------------------------------------------ families
def test_graded_columns():
    A = sp.graded(96, 64, F64, 5)
    norms = A.norm(dim=0)
    want = torch.logspace(0, -6, 64, dtype=F64)
    torch.testing.assert_close(torch.sort(norms, descending=True).values, want, rtol=1e-13, atol=0)
    assert not torch.equal(torch.sort(norms, descending=True).values, norms)  # shuffled
    assert torch.equal(sp.graded(96, 64, F64, 5), A)
    assert not torch.equal(sp.graded(96, 64, F64, 6), A)
    B = A / norms
    assert float(torch.linalg.cond(B)) < 100  # A = B D with a well-conditioned B
    assert sp.graded(96, 64, F32, 5).dtype == F32
    torch.testing.assert_close(sp.graded(96, 64, F32, 5).double(), A, rtol=2 ** -23, atol=0)


def test_lowrank_rank():
    A = sp.lowrank(96, 64, F64, 5)
    s = torch.linalg.svdvals(A)
    assert sp.rank_of("lowrank", 64) == 32
    assert float(s[31] / s[0]) > 1e-3 and float(s[32] / s[0]) < 1e-14
    # rounded to fp32 the tail is the rounding of the entries, not zero
    s32 = torch.linalg.svdvals(sp.lowrank(96, 64, F32, 5).double())
    assert 1e-9 < float(s32[32] / s32[0]) < 1e-6


def test_dupzero_columns():
    for dtype in (F32, F64):
        A = sp.dupzero(37, 33, dtype, 5)
        zero, dup = sp.dupzero_columns(33)
        assert zero == [0, 8, 16, 24, 32] and dup == [4, 12, 20, 28]
        assert bool((A[:, zero] == 0).all())
        for j in dup:
            assert torch.equal(A[:, j], A[:, j - 1])
        rest = [j for j in range(33) if j not in zero]
        assert bool((A[:, rest].norm(dim=0) > 1).all())
        r = sp.rank_of("dupzero", 33)
        assert r == 24
        s = torch.linalg.svdvals(A.double())
        assert float(s[r - 1] / s[0]) > 1e-3 and float(s[r] / s[0]) < 1e-14  # exact copies


def test_clustered_spectrum():
    A = sp.clustered(96, 64, F64, 5)
    s = torch.linalg.svdvals(A)
    torch.testing.assert_close(s, sp.clustered_spectrum(64), rtol=1e-12, atol=0)
    assert int((s > 0.5).sum()) == 32


def test_triu_is_the_reference_input():
    A = sp.triu(64, 64, F64, 0)
    assert torch.equal(A, svdj.utils.inputs.reference_triu(64))
    assert torch.equal(A, torch.triu(A)) and bool((torch.diagonal(A) > 0).all())
    s = torch.linalg.svdvals(A)
    assert float(s[-1] / s[0]) < 64 * torch.finfo(F64).eps  # numerically singular
    K = sp.significant(s, "triu", 64, 64, F64)
    assert 0 < K.numel() < 64 and torch.equal(K, torch.arange(K.numel()))


# ------------------------------------------------------- extended precision
@pytest.mark.skipif(not sp.has_longdouble(),
                    reason="numpy.longdouble is not extended precision on this platform")
def test_sigma_longdouble_against_lapack():
    """LAPACK's fp64 values carry ~1e-10 relative error on the small values
    of the graded input; the extended-precision Jacobi is the reference there."""
    A = sp.graded(96, 64, F64, 1)
    sig, X = sp.sigma_longdouble(A, with_columns=True)
    assert sig.dtype == np.longdouble and bool((sig[:-1] >= sig[1:]).all())
    ref = torch.linalg.svdvals(A).numpy()
    rel = float(np.max(np.abs(sig.astype(np.float64) - ref) / ref))
    print("sigma_longdouble against LAPACK, relative:", rel)
    assert rel <= 1e-9
    Xn = X / sig[:, None]
    G = Xn @ Xn.T - np.eye(64, dtype=np.longdouble)
    print("orthogonality of its columns (longdouble):", float(np.abs(G).max()))
    assert float(np.abs(G).max()) <= 1e-17
    # an odd column count pads with a zero column and drops it again
    s63 = sp.sigma_longdouble(A[:, :63])
    ref63 = torch.linalg.svdvals(A[:, :63]).numpy()
    assert s63.shape == (63,) and float(np.max(np.abs(s63.astype(np.float64) - ref63) / ref63)) <= 1e-9


# ------------------------------------------------------------ planted faults
@pytest.fixture(scope="module")
def good():
    """A good result: the oracle on graded 200 x 128 fp32, sorted."""
    A = sp.graded(200, 128, F32, 3)
    res = svdj.svd(A, method="oracle", precondition="none", sort=True)
    ref = sp.reference_sigma(A, "graded")
    clean = sp.metrics_of(A, res, "graded", ref)
    assert clean["finite"] and clean["converged"]
    return A, res, ref, clean


def _planted(good, U=None, S=None, V=None):
    A, res, ref, clean = good
    return sp.metrics(A, res.U if U is None else U, res.S if S is None else S,
                      res.V if V is None else V, "graded", ref=ref)


def _only(got, clean, caught, f=4.0):
    """``caught`` breaks the bound rule (f x the clean value); sig_abs and the
    Frobenius residual -- what the other end-to-end tests measure -- do not:
    a fault confined to small columns is invisible to them, which is why the
    per-sigma and per-column metrics exist."""
    print(json.dumps({"caught": caught, "planted": got, "clean": clean}))
    assert got[caught] > f * clean[caught], (caught, got[caught], clean[caught])
    assert got["sig_abs"] <= f * clean["sig_abs"], (got["sig_abs"], clean["sig_abs"])
    assert got["fro"] <= f * clean["fro"], (got["fro"], clean["fro"])


def test_sig_rel_catches_a_wrong_small_sigma(good):
    S = good[1].S.clone()
    S[-1] *= 1.0 + 1e-3  # the smallest significant sigma (graded: all are)
    got = _planted(good, S=S)
    _only(got, good[3], "sig_rel")
    assert got["sig_rel"] > 5e-4


def test_colres_catches_swapped_small_columns_of_u(good):
    U = good[1].U.clone()
    U[:, [-1, -2]] = U[:, [-2, -1]]  # the two smallest sigmas' left vectors
    got = _planted(good, U=U)
    _only(got, good[3], "colres")
    assert got["colres"] > 1e-2  # of order 1 on the smallest column
    assert got["orth_u"] <= 4.0 * good[3]["orth_u"]  # still orthonormal: only colres sees it


def test_orth_v_catches_a_perturbed_column_of_v(good):
    V = good[1].V.clone()
    V[:, -1] += 1e-3 * V[:, -2]  # the smallest sigma's right vector
    got = _planted(good, V=V)
    _only(got, good[3], "orth_v")
    assert got["orth_v"] > 5e-4


# ------------------------------------------------- oracle and CPU block path
# f of the bound rule (4 where the measured block / oracle ratio is at most 2,
# else twice the measured ratio rounded up, never above 16): measured at
# 200 x 128 (triu 128), seed 3, largest ratio over the five metrics.
F_OVER = {
    # fp64 rank-deficient and clustered input: the block path takes 1.7 to 2.5
    # times the oracle's sweeps (README "Stop test"), each one more pass of
    # rounding over every column; 3.96 on sig_abs and colres, 3.4 on orth_v
    ("lowrank", "fp64"): 8,
    ("clustered", "fp64"): 6,   # colres 2.61, sig_abs 2.44, orth_v 2.34 (33 sweeps against 20)
    ("dupzero", "fp64"): 5,     # orth_v 2.16 (30 sweeps against 18)
    ("triu", "fp32"): 5,        # sig_abs 2.02
}

CASES = [(fam, d) for fam in sp.FAMILIES for d in (F32, F64)]


@pytest.mark.parametrize("family,dtype", CASES, ids=[f"{f}-{NAME[d]}" for f, d in CASES])
def test_oracle_and_block_path_on_every_family(family, dtype):
    m, n = (128, 128) if family == "triu" else (200, 128)
    A = sp.FAMILIES[family](m, n, dtype, 3)
    ref = sp.reference_sigma(A, family)
    oracle = svdj.svd(A, method="oracle", precondition="none")
    block = svdj.svd(A, method="block", block=32, precondition="none")
    want = sp.metrics_of(A, oracle, family, ref)
    got = sp.metrics_of(A, block, family, ref)
    f = F_OVER.get((family, NAME[dtype]), 4)
    assert f <= 16
    print(json.dumps({"family": family, "dtype": NAME[dtype], "f": f, "block": got,
                      "oracle": want}))
    limit = svdj.SolverConfig().max_sweeps
    for name, mt in (("oracle", want), ("block", got)):
        assert mt["finite"] and mt["converged"], (name, mt)
        assert mt["sweeps"] <= limit, (name, mt["sweeps"])
    bad = sp.within(got, want, f)
    assert not bad, (family, NAME[dtype], f, bad)
    if family == "dupzero":
        assert got["tail"] <= f * want["tail"], (got["tail"], want["tail"])
