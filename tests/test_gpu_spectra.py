"""Whole GPU solves on graded, rank-deficient, clustered and triangular input
(tests/_spectra.py), every engine against the CPU oracle on the same matrix in
the same dtype.

The other end-to-end GPU tests feed U(0,1) and divide the singular-value error
by sigma_max, which says nothing about the bulk or about small columns.  Here
each case asserts that the outputs are finite, that the solve converged within
the default sweep limit, and that each of sig_rel, sig_abs, colres, orth_v and
orth_u (``_spectra.metrics``) is at most f times the oracle's value.  f is 4
(the factor of test_gpu_batched.py: another pair order gives another rounding
trajectory) wherever the measured GPU / oracle ratio is at most 2; where it is
larger f is twice the measured ratio rounded up, listed in ``F_OVER`` with the
reason, and never above 16.  The measured table is profiles/spectra/.  Set
SVDJ_SPECTRA_ACCURACY_OUT to a file name to append each case's JSON line to it.
"""
import json
import os

import pytest
import torch

import _spectra as sp

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NAME = {F32: "fp32", F64: "fp64"}
MAX_SWEEPS = 60  # SolverConfig.max_sweeps
SEED = 3

# f other than 4: (engine, family, dtype name) -> (f, reason).  From
# profiles/spectra/accuracy.jsonl by the rule in the module docstring; every
# other case measured a ratio of at most 2 (most of them below 1.3).
_MORE_SWEEPS = ("the W=32 block path takes %s sweeps against the oracle's %s (README, Stop test: "
                "tracked norms as the Gram diagonal), each one more pass of rounding over every "
                "column; the CPU emulation of the block path shows the same, up to 3.96")
F_OVER = {
    ("pipeline_w32", "lowrank", "fp64"): (6, "colres 2.83, sig_abs 2.78: "
                                             + _MORE_SWEEPS % (53, 24)),
    ("pipeline_w32", "dupzero", "fp64"): (6, "orth_v 2.69: " + _MORE_SWEEPS % (42, 21)),
    ("pipeline_w32", "triu", "fp64"): (5, "sig_abs 2.25 (9.5e-14 against 4.2e-14): the largest "
                                          "sigma's error after 29 sweeps of W=32 block rotations "
                                          "against the oracle's scalar ones"),
    ("batched_64x64", "triu", "fp32"): (6, "sig_rel 2.58: the value at the edge of the "
                                           "significant set (sigma_i ~ m eps sigma_max) is known "
                                           "to a relative error of order 1/m only; which engine "
                                           "lands nearer is rounding luck (0.49 to 2.6 over the "
                                           "triu cases)"),
}


def _f(engine, family, dtype):
    f = F_OVER.get((engine, family, NAME[dtype]), (4, ""))[0]
    assert f <= 16
    return f


# ------------------------------------------------------------------ engines
def _dist(svdj, **kw):
    from svdj.parallel import DistributedBlockJacobi

    def run(A):
        return DistributedBlockJacobi(svdj.SolverConfig(dtype=F32, block=64, **kw)).solve(A)
    return run


def _single_engines(svdj):
    """name -> (m, n, dtypes, run(A on the GPU) -> SVDResult)."""
    return {
        "pipeline_w32": (520, 384, (F32, F64), lambda A: svdj.svd(A, precondition="none")),
        "steps_w32": (520, 384, (F32,),
                      lambda A: svdj.svd(A, precondition="none", extra={"engine": "steps"})),
        "quad_on": (1100, 1024, (F32,), _dist(svdj, mma="bf16x6", quad="on")),
        "quad_off": (1100, 1024, (F32,), _dist(svdj, mma="bf16x6", quad="off")),
        "w64_native": (1100, 1024, (F32,), _dist(svdj, mma="native", quad="off")),
        # precondition="none": 300 >= 2 x 128 would otherwise run Jacobi on R
        "scalar": (300, 128, (F32, F64),
                   lambda A: svdj.svd(A, method="scalar", precondition="none")),
    }


SINGLE = [("pipeline_w32", F32), ("pipeline_w32", F64), ("steps_w32", F32), ("quad_on", F32),
          ("quad_off", F32), ("w64_native", F32), ("scalar", F32), ("scalar", F64)]
SINGLE_SHAPE = {"pipeline_w32": (520, 384), "steps_w32": (520, 384), "quad_on": (1100, 1024),
                "quad_off": (1100, 1024), "w64_native": (1100, 1024), "scalar": (300, 128)}

_ORACLE = {}


def _oracle(svdj, family, m, n, dtype, seed=SEED):
    """(A on the CPU, reference spectrum, the oracle's metrics), once per
    (family, shape, dtype, seed).  The oracle iterates on A itself."""
    key = (family, m, n, dtype, seed)
    if key not in _ORACLE:
        A = sp.FAMILIES[family](m, n, dtype, seed)
        ref = sp.reference_sigma(A, family)
        res = svdj.svd(A, method="oracle", precondition="none")
        want = sp.metrics_of(A, res, family, ref)
        assert want["finite"] and want["converged"], want
        _ORACLE[key] = (A, ref, want)
    return _ORACLE[key]


def _record(rec):
    print(json.dumps(rec))
    out = os.environ.get("SVDJ_SPECTRA_ACCURACY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def _ratios(got, want):
    return {k: (got[k] / want[k] if got[k] is not None and want[k] else None)
            for k in sp.METRICS + ("tail",)}


def _assert_case(engine, family, dtype, shape, got, want, extra=None):
    f = _f(engine, family, dtype)
    rec = {"engine": engine, "family": family, "dtype": NAME[dtype], "shape": list(shape),
           "f": f, "f_reason": F_OVER.get((engine, family, NAME[dtype]), (4, ""))[1], "gpu": got, "oracle": want, "ratio": _ratios(got, want),
           "sweeps": got["sweeps"], "oracle_sweeps": want["sweeps"]}
    rec.update(extra or {})
    _record(rec)
    assert got["finite"], rec
    assert got["converged"], rec
    sweeps = got["sweeps"] if isinstance(got["sweeps"], list) else [got["sweeps"]]
    assert max(sweeps) <= MAX_SWEEPS, sweeps
    if family == "graded" and dtype == F64 and not sp.has_longdouble():
        print("sig_rel of fp64 graded not checked: numpy.longdouble is not extended precision")
    bad = sp.within(got, want, f)
    assert not bad, (engine, family, NAME[dtype], f, bad)
    if family == "dupzero":  # the sigmas beyond the rank, over sigma_max
        assert got["tail"] <= f * want["tail"], ("tail", got["tail"], want["tail"])


FAMILY_NAMES = list(sp.FAMILIES)


@pytest.mark.parametrize("family", FAMILY_NAMES)
@pytest.mark.parametrize("engine,dtype", SINGLE, ids=[f"{e}-{NAME[d]}" for e, d in SINGLE])
def test_single_matrix_engines(svdj, cuda, engine, dtype, family):
    m, n = SINGLE_SHAPE[engine]
    if family == "triu":
        m = n
    run = _single_engines(svdj)[engine][3]
    A, ref, want = _oracle(svdj, family, m, n, dtype)
    res = run(A.to(cuda))
    got = sp.metrics_of(A, res, family, ref)
    extra = {}
    if engine.startswith("quad") or engine == "w64_native":
        assert res.info["quad"] == (engine == "quad_on"), res.info
        assert res.info["geometry"]["W"] == 64
    if engine in ("pipeline_w32", "steps_w32"):
        assert res.info["engine"] == ("steps" if engine == "steps_w32" else "pipeline")
        assert res.info["block"] == 32
    if engine == "quad_on":
        work = res.info["work"]
        extra = {"gram_quads": work["gram_quads"], "gram_quads2": work["gram_quads2"]}
        if family == "graded":  # both the 2-part and the 3-part quad Gram ran
            assert 0 < work["gram_quads2"] < work["gram_quads"], work
    _assert_case(engine, family, dtype, (m, n), got, want, extra)


def test_qr_preconditioned_graded(svdj, cuda):
    """1200 x 128 graded fp32: kappa = 1e7 is beyond CholeskyQR2 in fp32
    (kappa^2 eps > 1), so the Householder fallback carries the solve."""
    m, n = 1200, 128
    A, ref, want = _oracle(svdj, "graded", m, n, F32)
    res = svdj.svd(A.to(cuda), precondition="qr", method="block")
    assert res.info["precondition"] == "qr" and res.info["qr"] == "householder", res.info
    got = sp.metrics_of(A, res, "graded", ref)
    _assert_case("qr_block", "graded", F32, (m, n), got, want)


# ------------------------------------------------------------------ batched
def _batched_metrics(As, res, family, refs):
    U, S, V = (t.cpu() for t in (res.U, res.S, res.V))
    ms = [sp.metrics(As[i], U[i], S[i], V[i], family, ref=refs[i],
                     converged=bool(res.converged[i]), sweeps=int(res.sweeps[i]))
          for i in range(len(As))]
    return sp.worst(ms)


BATCHED = [("batched", 37, 33, 0), ("batched", 64, 64, 0),
           ("batched_tall", 100, 16, 32), ("batched_tall", 1000, 33, 0)]


# triu is square: it runs on the LDS kernel only, at the square of the column count
BATCHED_CASES = [(c, fam, d) for c in BATCHED for fam in FAMILY_NAMES for d in (F32, F64)
                 if not (fam == "triu" and c[0] == "batched_tall")]


@pytest.mark.parametrize("case,family,dtype", BATCHED_CASES,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}-{fam}-{NAME[d]}"
                              for c, fam, d in BATCHED_CASES])
def test_batched_engines(svdj, cuda, case, family, dtype):
    kind, m, n, rows = case
    if family == "triu":
        m = n
    kw = {"precondition": "qr", "panel_rows": rows} if kind == "batched_tall" else {}
    want_engine = "qr_kernel" if kind == "batched_tall" else "kernel"
    seeds = (SEED, SEED + 1, SEED + 2)
    items = [_oracle(svdj, family, m, n, dtype, s) for s in seeds]
    As, refs = [it[0] for it in items], [it[1] for it in items]
    want = sp.worst([it[2] for it in items])
    if family == "dupzero":
        # the deficient matrices share a batch with full-rank ones, whose
        # results do not notice: bitwise those of a batch without them
        g = torch.Generator().manual_seed(77)
        R = torch.rand(2, m, n, dtype=dtype, generator=g)
        mixed = torch.stack([As[0], R[0], As[1], R[1], As[2]]).to(cuda)
        full = svdj.svd_batched(mixed, **kw)
        alone = svdj.svd_batched(R.to(cuda), **kw)
        assert full.info["engine"] == want_engine and alone.info["engine"] == want_engine
        for name in ("U", "S", "V", "sweeps"):
            assert torch.equal(getattr(full, name)[[1, 3]], getattr(alone, name)), name
        assert bool(alone.converged.all())
        pick = torch.tensor([0, 2, 4], device=cuda)
        from svdj.models.base import BatchedSVDResult
        res = BatchedSVDResult(full.U[pick], full.S[pick], full.V[pick], full.sweeps[pick],
                               full.converged[pick], full.off[pick], full.seconds, full.info)
    else:
        res = svdj.svd_batched(torch.stack(As).to(cuda), **kw)
    assert res.info["engine"] == want_engine, res.info
    if rows:
        assert res.info["panel_rows"] == rows
    got = _batched_metrics(As, res, family, refs)
    _assert_case(f"{kind}_{m}x{n}", family, dtype, (3, m, n), got, want)
