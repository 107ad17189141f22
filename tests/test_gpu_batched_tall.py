"""svd_batched(A, precondition="qr") on the GPU: the tall batched kernel
(csrc/hip/batched_tall.hip: QR by row panels into an LDS-resident R, Jacobi on
R, U = Q U_R) against two CPU references in the same dtype.

Every accuracy bound is 4x the larger of
  * ``svd(A[i], method="oracle")``, and
  * ``torch.linalg.qr`` on the CPU, the oracle on R, U = Q U_R
in the metrics of test_gpu_batched.py (residual, sigma, orth_u, orth_v, all
measured in fp64 on the CPU).  The second reference is there because a
Householder product rounds differently from rotated columns; the factor 4 is
the one test_gpu_batched.py uses.  Set SVDJ_BATCHED_ACCURACY_OUT to a file name
to append the measured pairs to it as JSON lines.
"""
import json
import os

import pytest
import torch

import svdj
from test_gpu_batched import METRICS, _metrics, _rand, _sigma_err

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
CAP = 163840


def _ref_metrics(A, key, _cache={}):
    """Per metric the larger value of the two references on the CPU batch
    ``A``, and both sets; computed once per (key, dtype)."""
    key = (key, A.dtype)
    if key not in _cache:
        rs = [svdj.svd(A[i], method="oracle") for i in range(A.shape[0])]
        assert all(r.converged for r in rs)
        direct = _metrics(A, torch.stack([r.U for r in rs]), torch.stack([r.S for r in rs]),
                          torch.stack([r.V for r in rs]))
        Us, Ss, Vs = [], [], []
        for i in range(A.shape[0]):
            Q, R = torch.linalg.qr(A[i])
            r = svdj.svd(R, method="oracle", precondition="none")
            assert r.converged
            Us.append(Q @ r.U)
            Ss.append(r.S)
            Vs.append(r.V)
        qr = _metrics(A, torch.stack(Us), torch.stack(Ss), torch.stack(Vs))
        _cache[key] = ({k: max(direct[k], qr[k]) for k in METRICS}, direct, qr)
    return _cache[key]


def _qr(A, **kw):
    return svdj.svd_batched(A, precondition="qr", **kw)


def _check(key, A, res, panel_rows=None):
    """``res`` = svd_batched(precondition="qr") of the CPU batch ``A``: engine,
    panel bookkeeping, convergence, every metric within 4x the references'."""
    info = res.info
    assert info["engine"] == "qr_kernel", info
    rows, m = info["panel_rows"], max(A.shape[-2:])
    if panel_rows:
        assert rows == panel_rows
    assert rows % 8 == 0 and rows >= 8
    assert info["panels"] == -(-m // rows)  # ceil
    assert 0 < info["lds_bytes"] <= CAP
    got = _metrics(A, res.U, res.S, res.V)
    want, direct, qr = _ref_metrics(A, key)
    rec = {"case": key, "dtype": str(A.dtype), "shape": list(A.shape), "engine": info["engine"],
           "panel_rows": rows, "panels": info["panels"], "sweeps": res.sweeps.flatten().tolist(),
           "svd_batched": got, "oracle": direct, "qr_oracle": qr}
    print(json.dumps(rec))
    out = os.environ.get("SVDJ_BATCHED_ACCURACY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert bool(res.converged.all()), res.sweeps
    for name in METRICS:
        assert got[name] <= 4.0 * want[name], (name, got[name], want[name])
    return want


# (m, n, forced panel_rows or 0, dtypes)
SHAPES = [(3, 2, 8, (F32, F64)), (8, 3, 8, (F32, F64)), (17, 3, 8, (F32, F64)),
          (16, 1, 8, (F32, F64)), (100, 16, 32, (F32, F64)), (1000, 33, 0, (F32, F64)),
          (553, 64, 0, (F32,)), (233, 64, 0, (F64,)), (2000, 64, 0, (F32, F64)),
          (10000, 3, 0, (F32, F64))]
CASES = [(m, n, p, d) for m, n, p, ds in SHAPES for d in ds]


def _id(c):
    return f"{c[0]}x{c[1]}-p{c[2] or 'auto'}-{'fp32' if c[3] == F32 else 'fp64'}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_shapes_against_references(cuda, case):
    m, n, rows, dtype = case
    A = _rand(3, m, n, dtype=dtype, seed=1000 + m + n)
    res = _qr(A.to(cuda), panel_rows=rows)
    assert res.U.shape == (3, m, n) and res.V.shape == (3, n, n) and res.S.dtype == dtype
    _check(f"tall_{m}x{n}", A, res, rows)
    if rows:
        assert res.info["panels"] == -(-m // rows)
    if (m, n) == (17, 3):
        assert res.info["panels"] == 3
    if n == 64:  # no LDS holds these whole: several panels
        assert res.info["panels"] >= 2


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("shape", [(17, 3, 8), (100, 16, 32), (2000, 64, 0)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_qr_alone(cuda, shape, dtype):
    """max_sweeps=0 leaves phases 1 and 3: V = I, S = the column norms of R
    (those of A), U = Q times the normalised columns of R, so U diag(S) = A.
    Bounds: 4x what LAPACK's QR on the CPU gives, computed the same way."""
    m, n, rows = shape
    A = _rand(3, m, n, dtype=dtype, seed=2000 + m)
    res = _qr(A.to(cuda), panel_rows=rows, max_sweeps=0)
    assert res.info["engine"] == "qr_kernel" and res.sweeps.tolist() == [0, 0, 0]
    eye = torch.eye(n, dtype=dtype)
    assert all(torch.equal(res.V[i].cpu(), eye) for i in range(3))
    A64 = A.double()
    norms = A64.norm(dim=1)  # (3, n) column norms

    def errs(U, S):
        rec = (U.double() * S.double().unsqueeze(-2) - A64).flatten(1).norm(dim=1) \
            / A64.flatten(1).norm(dim=1)
        sig = (S.double() - norms).abs().amax(1) / norms.amax(1)
        return float(rec.max()), float(sig.max())

    Uq, Sq = [], []
    for i in range(3):
        Q, R = torch.linalg.qr(A[i])
        s = R.double().norm(dim=0).to(dtype)  # fp64 sum, rounded: as the kernel's finalize
        Uq.append(Q @ (R / s))
        Sq.append(s)
    want = errs(torch.stack(Uq), torch.stack(Sq))
    got = errs(res.U.cpu(), res.S.cpu())
    print(json.dumps({"case": f"qr_alone_{m}x{n}", "dtype": str(dtype), "got": got,
                      "lapack_qr": want}))
    assert got[0] <= 4.0 * want[0] and got[1] <= 4.0 * want[1], (got, want)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
def test_panel_invariance(cuda, dtype):
    A = _rand(3, 100, 16, dtype=dtype, seed=1116)
    runs = [_qr(A.to(cuda), panel_rows=rows) for rows in (8, 32, 0)]
    assert [r.info["panels"] for r in runs] == [13, 4, 1]
    for r in runs:
        want = _check("tall_100x16", A, r)
    s = [torch.sort(r.S.cpu().double(), dim=-1, descending=True).values for r in runs]
    for other in s[1:]:
        diff = float(((other - s[0]).abs().amax(1) / s[0][:, 0]).max())
        print("panel invariance sigma diff", diff, "bound", 4.0 * want["sigma"])
        assert diff <= 4.0 * want["sigma"]


def test_against_the_lds_kernel(cuda):
    A = _rand(3, 256, 64, dtype=F32, seed=7)
    qr, ker = _qr(A.to(cuda)), svdj.svd_batched(A.to(cuda))
    assert ker.info["engine"] == "kernel"
    want = _check("tall_256x64", A, qr)
    oracle = _ref_metrics(A, "tall_256x64")[1]
    sq, sk = (torch.sort(r.S.cpu().double(), dim=-1, descending=True).values for r in (qr, ker))
    diff = float(((sq - sk).abs().amax(1) / sk[:, 0]).max())
    print("qr_kernel against kernel sigma diff", diff)
    assert diff <= 4.0 * want["sigma"] + 4.0 * oracle["sigma"]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
def test_batch_independence_bitwise(cuda, dtype):
    R = _rand(4, 40, 8, dtype=dtype, seed=21)
    zcol = R[0].clone()
    zcol[:, 3] = 0
    dup = R[1].clone()
    dup[:, 5] = dup[:, 2]
    A = torch.stack([R[0], torch.eye(40, 8, dtype=dtype), R[1], torch.zeros(40, 8, dtype=dtype),
                     zcol, dup, R[2], R[3]])
    full = _qr(A.to(cuda), panel_rows=16)
    assert full.info["engine"] == "qr_kernel" and full.info["panels"] == 3
    assert bool(full.converged.all()), full.sweeps
    rev = _qr(A.flip(0).to(cuda), panel_rows=16)
    for name in ("U", "S", "V", "sweeps"):
        assert torch.equal(getattr(rev, name).flip(0), getattr(full, name)), name
    for i in range(A.shape[0]):
        one = _qr(A[i:i + 1].to(cuda), panel_rows=16)
        for name in ("U", "S", "V", "sweeps"):
            assert torch.equal(getattr(one, name)[0], getattr(full, name)[i]), (name, i)
    U, S, V = (t.cpu() for t in full)
    assert all(bool(torch.isfinite(t).all()) for t in (U, S, V))
    sweeps = full.sweeps.tolist()
    assert sweeps[1] == 1  # the identity's R is diagonal: nothing to rotate
    assert bool((S[3] == 0).all()) and torch.equal(V[3], torch.eye(8, dtype=dtype))
    # sigma bound: 4x the references' worst over the full-rank matrices of this batch
    want = _ref_metrics(R, "independence_40x8")[0]
    sref = torch.linalg.svd(A.double()).S
    for i in (0, 2, 4, 5, 6, 7):
        err = _sigma_err(S[i], sref[i])
        print("independence", i, "sigma err", err, "bound", 4.0 * want["sigma"], "sweeps",
              sweeps[i])
        assert err <= 4.0 * want["sigma"]


def test_scale_invariance_bitwise(cuda):
    """An exact power of two changes sigma by that factor and nothing else,
    also where the running exponent rises from one panel to the next (rows 32
    to 63 are 16 times larger) and falls back."""
    A0 = _rand(3, 100, 16, dtype=F32, seed=31)
    step = A0.clone()
    step[:, 32:64] *= 16.0
    for key, A in (("scale_100x16", A0), ("scale_step_100x16", step)):
        base = _qr(A.to(cuda), panel_rows=32)
        _check(key, A, base, 32)
        for k in (40, -66):
            res = _qr((A * 2.0 ** k).to(cuda), panel_rows=32)
            assert torch.equal(res.S, base.S * 2.0 ** k), (key, k)
            assert torch.equal(res.U, base.U) and torch.equal(res.V, base.V), (key, k)
            assert torch.equal(res.sweeps, base.sweeps), (key, k)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
def test_layouts(cuda, dtype):
    A = _rand(3, 100, 16, dtype=dtype, seed=1116)
    res = _qr(A.to(cuda), panel_rows=32)
    assert res.info["in_place"] and not res.info["transposed"]
    # the transposed view of a contiguous (B, n, m) tensor: read in place, same arithmetic
    view = A.transpose(1, 2).contiguous().to(cuda).transpose(1, 2)
    assert not view.is_contiguous()
    res_t = _qr(view, panel_rows=32)
    assert res_t.info["in_place"] and res_t.info["engine"] == "qr_kernel"
    for a, b in ((res.U, res_t.U), (res.S, res_t.S), (res.V, res_t.V)):
        assert torch.equal(a, b)
    # wide (3, 16, 100): U and V on the right sides
    Aw = A.transpose(1, 2).contiguous()
    res_w = _qr(Aw.to(cuda), panel_rows=32)
    assert res_w.info["transposed"] and res_w.info["in_place"]
    assert res_w.U.shape == (3, 16, 16) and res_w.V.shape == (3, 100, 16)
    _check("tall_16x100", Aw, res_w, 32)
    assert torch.equal(res_w.U, res.V) and torch.equal(res_w.V, res.U)
    # a non-contiguous slice goes through the contiguous copy
    big = torch.zeros(3, 200, 16, dtype=dtype)
    big[:, ::2, :] = A
    res_s = _qr(big.to(cuda)[:, ::2, :], panel_rows=32)
    assert not res_s.info["in_place"] and torch.equal(res_s.S, res.S)


def test_job_options_and_bf16(cuda):
    A = _rand(3, 100, 16, dtype=F32, seed=61).to(cuda)
    full = _qr(A, panel_rows=32)
    nov = _qr(A, panel_rows=32, jobv=svdj.NoVec)
    assert nov.info["engine"] == "qr_kernel" and nov.V is None
    assert torch.equal(nov.S, full.S) and torch.equal(nov.U, full.U)
    nou = _qr(A, panel_rows=32, jobu=svdj.NoVec)
    assert nou.info["engine"] == "qr_kernel" and nou.U is None
    assert torch.equal(nou.S, full.S) and torch.equal(nou.V, full.V)
    none = _qr(A, panel_rows=32, jobu=svdj.NoVec, jobv=svdj.NoVec)
    assert none.U is None and none.V is None and torch.equal(none.S, full.S)
    one = _qr(A, panel_rows=32, max_sweeps=1)
    assert one.sweeps.tolist() == [1, 1, 1] and not bool(one.converged.any())
    srt = _qr(A, panel_rows=32, sort=True)
    assert bool((srt.S[:, :-1] >= srt.S[:, 1:]).all())
    _check("jobs_100x16", A.cpu(), srt, 32)
    Ab = A.to(torch.bfloat16)
    res = _qr(Ab, panel_rows=32)
    assert res.info["engine"] == "qr_kernel"
    assert res.U.dtype == torch.bfloat16 and res.V.dtype == torch.bfloat16
    assert res.S.dtype == torch.float32
    sref = torch.linalg.svd(Ab.cpu().double()).S
    for i in range(3):  # as test_gpu_batched.py: bf16-level tolerance, fp32 arithmetic
        assert _sigma_err(res.S[i].cpu(), sref[i]) <= 1e-4


def test_non_finite_input(cuda):
    A = _rand(3, 100, 16, dtype=F32, seed=51)
    B = A.clone()
    B[1, 45, 7] = float("nan")
    clean = _qr(A.to(cuda), panel_rows=32)
    res = _qr(B.to(cuda), panel_rows=32)  # returns: every loop of the kernel is counted
    assert res.info["engine"] == "qr_kernel"
    assert (not bool(res.converged[1])) or (not bool(torch.isfinite(res.S[1]).all()))
    assert int(res.sweeps[1]) <= 60
    for i in (0, 2):
        for name in ("U", "S", "V", "sweeps"):
            assert torch.equal(getattr(res, name)[i], getattr(clean, name)[i]), (name, i)


def test_default_engine_unchanged(cuda):
    A = _rand(3, 553, 64, dtype=F32, seed=72).to(cuda)
    assert svdj.svd_batched(A).info["engine"] == "loop"
    assert svdj.svd_batched(A[:, :552]).info["engine"] == "kernel"
    assert _qr(A[:, :552]).info["engine"] == "qr_kernel"
    # a square batch has nothing to precondition; a named method is honoured
    assert _qr(A[:, :64]).info["engine"] == "kernel"
    assert _qr(A[:, :100], method="scalar").info["engine"] == "loop"
