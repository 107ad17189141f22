"""svd_batched on the GPU: the LDS-resident batched kernel
(csrc/hip/batched.hip) against fp64 torch.linalg.svd and the CPU oracle.

Every accuracy bound here is 4x the CPU oracle's own worst value over the
same matrices (``svd(A[i], method="oracle")``, same dtype, same tolerance
rule): the factor covers the different pair order (round robin against
Sameh) and hence a different rounding trajectory.  Set
SVDJ_BATCHED_ACCURACY_OUT to a file name to append the measured (svd_batched,
oracle) pairs to it as JSON lines ("engine" says which engine ran).
"""
import json
import os

import pytest
import torch

import svdj

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
METRICS = ("residual", "sigma", "orth_u", "orth_v")


def _rand(*shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, dtype=dtype, generator=g)


def _metrics(A, U, S, V):
    """Worst value over the batch of: ||A - U S V^T||_F / ||A||_F, sigma error
    over sigma_max against fp64 torch.linalg.svd on the CPU, and the largest
    entry of U^T U - I and of V^T V - I.  Everything in fp64 on the CPU."""
    A, U, S, V = (t.detach().cpu().double() for t in (A, U, S, V))
    k = S.shape[-1]
    R = (U * S.unsqueeze(-2)) @ V.transpose(-1, -2) - A
    res = R.flatten(1).norm(dim=1) / A.flatten(1).norm(dim=1).clamp(min=1e-300)
    sref = torch.linalg.svd(A, full_matrices=False).S
    serr = (torch.sort(S, dim=-1, descending=True).values - sref).abs().amax(1) \
        / sref[:, 0].clamp(min=1e-300)
    eye = torch.eye(k, dtype=torch.float64)
    ou = (U.transpose(-1, -2) @ U - eye).abs().flatten(1).amax(1)
    ov = (V.transpose(-1, -2) @ V - eye).abs().flatten(1).amax(1)
    return {"residual": float(res.max()), "sigma": float(serr.max()),
            "orth_u": float(ou.max()), "orth_v": float(ov.max())}


_ORACLE = {}


def _oracle_metrics(key, A):
    """The oracle's metrics on the CPU batch ``A``, computed once per key."""
    key = (key, A.dtype)
    if key not in _ORACLE:
        rs = [svdj.svd(A[i], method="oracle") for i in range(A.shape[0])]
        assert all(r.converged for r in rs)
        _ORACLE[key] = _metrics(A, torch.stack([r.U for r in rs]), torch.stack([r.S for r in rs]),
                                torch.stack([r.V for r in rs]))
    return _ORACLE[key]


def _check(key, A, res, engine="kernel"):
    """``res`` = svd_batched of the CPU batch ``A`` (moved to the GPU by the
    caller): engine, convergence, and every metric within 4x the oracle's."""
    got = _metrics(A, res.U, res.S, res.V)
    want = _oracle_metrics(key, A)
    rec = {"case": key, "dtype": str(A.dtype), "shape": list(A.shape), "engine": res.info["engine"],
           "sweeps": res.sweeps.flatten().tolist(), "svd_batched": got, "oracle": want}
    print(json.dumps(rec))
    out = os.environ.get("SVDJ_BATCHED_ACCURACY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert res.info["engine"] == engine
    assert bool(res.converged.all()), res.sweeps
    for name in METRICS:
        assert got[name] <= 4.0 * want[name], (name, got[name], want[name])


def _largest_m(dtype, n, want_v=True):
    """The largest m the LDS size routine accepts at n columns."""
    f = svdj.ops.kernels.batched_lds_bytes
    lo, hi = n, 1 << 20
    assert f(dtype, lo, n, want_v) > 0 and f(dtype, hi, n, want_v) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if f(dtype, mid, n, want_v) > 0 else (lo, mid)
    return lo


SHAPES = [(1, 1), (2, 2), (3, 3), (5, 3), (8, 8), (37, 33), (64, 64)]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_against_oracle(cuda, shape, dtype):
    A = _rand(3, *shape, dtype=dtype, seed=100 + shape[0])
    res = svdj.svd_batched(A.to(cuda))
    assert res.U.shape == (3, *shape) and res.V.shape == (3, shape[1], shape[1])
    assert res.S.dtype == dtype and res.sweeps.dtype == torch.int32
    _check(f"oracle_{shape[0]}x{shape[1]}", A, res)


def test_largest_lds_fp32_with_v(cuda):
    """256 x 64 fp32 with V: 86400 bytes of LDS, above the 64 KiB that a
    kernel gets without the dynamic-LDS opt-in."""
    assert svdj.ops.kernels.batched_lds_bytes(F32, 256, 64, True) > 65536
    A = _rand(3, 256, 64, dtype=F32, seed=7)
    _check("lds_fp32_256x64", A, svdj.svd_batched(A.to(cuda)))


def test_largest_fp64_shape(cuda):
    """The fp64 LDS limit at n = 64: the largest m the size routine accepts."""
    m = _largest_m(F64, 64)
    assert svdj.ops.kernels.batched_lds_bytes(F64, m + 1, 64, True) == 0
    A = _rand(3, m, 64, dtype=F64, seed=8)
    res = svdj.svd_batched(A.to(cuda))
    assert res.info["lds_bytes"] <= 163840
    _check(f"lds_fp64_{m}x64", A, res)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
def test_layouts(cuda, dtype):
    A = _rand(3, 37, 33, dtype=dtype, seed=11)
    key = "layout_37x33"
    # contiguous (B, m, n)
    res = svdj.svd_batched(A.to(cuda))
    assert res.info["in_place"] and not res.info["transposed"]
    _check(key, A, res)
    # the transposed view of a contiguous (B, n, m) tensor: same matrices, read in place
    base = A.transpose(1, 2).contiguous().to(cuda)
    view = base.transpose(1, 2)
    assert not view.is_contiguous()
    res_t = svdj.svd_batched(view)
    assert res_t.info["in_place"]
    _check(key, A, res_t)
    for a, b in ((res.U, res_t.U), (res.S, res_t.S), (res.V, res_t.V)):
        assert torch.equal(a, b)  # the layout changes the loads, not the arithmetic
    # wide (3, 33, 37): U and V on the right sides
    Aw = A.transpose(1, 2).contiguous()
    res_w = svdj.svd_batched(Aw.to(cuda))
    assert res_w.info["transposed"] and res_w.info["in_place"]
    assert res_w.U.shape == (3, 33, 33) and res_w.V.shape == (3, 37, 33)
    _check("layout_33x37", Aw, res_w)
    assert torch.equal(res_w.U, res.V) and torch.equal(res_w.V, res.U)
    # a non-contiguous slice goes through the contiguous copy
    big = torch.zeros(3, 74, 33, dtype=dtype)
    big[:, ::2, :] = A
    res_s = svdj.svd_batched(big.to(cuda)[:, ::2, :])
    assert not res_s.info["in_place"]
    _check(key, A, res_s)
    assert torch.equal(res_s.S, res.S)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
def test_batch_independence_bitwise(cuda, dtype):
    R = _rand(4, 33, 33, dtype=dtype, seed=21)
    A = torch.stack([R[0], torch.eye(33, dtype=dtype), R[1], R[2] * 2.0 ** 40, R[3]]).to(cuda)
    full = svdj.svd_batched(A)
    assert full.info["engine"] == "kernel" and bool(full.converged.all())
    rev = svdj.svd_batched(A.flip(0))
    for name in ("U", "S", "V", "sweeps"):
        assert torch.equal(getattr(rev, name).flip(0), getattr(full, name)), name
    for i in range(5):
        one = svdj.svd_batched(A[i:i + 1])
        for name in ("U", "S", "V", "sweeps"):
            assert torch.equal(getattr(one, name)[0], getattr(full, name)[i]), (name, i)
    sweeps = full.sweeps.tolist()
    assert sweeps[1] == 1 and all(s > 1 for i, s in enumerate(sweeps) if i != 1), sweeps
    # the power-of-two scale is exact: 2^40 A iterates as A does
    alone = svdj.svd_batched((R[2:3]).to(cuda))
    assert torch.equal(alone.S[0] * 2.0 ** 40, full.S[3])
    assert torch.equal(alone.U[0], full.U[3]) and torch.equal(alone.V[0], full.V[3])


def test_many_workgroups(cuda):
    """4096 matrices of 8 x 8: more workgroups than one wave of them, several
    per CU.  Reconstruction bound: a rotation perturbs its two columns by at
    most ~3 eps relative, a column takes part in n - 1 rotations per sweep, so
    linear worst-case growth over the sweeps run is 3 (n - 1) sweeps eps."""
    A = _rand(4096, 8, 8, dtype=F32, seed=31)
    A[4095] = A[0]
    res = svdj.svd_batched(A.to(cuda))
    assert res.info["engine"] == "kernel" and bool(res.converged.all())
    U, S, V = (t.cpu().double() for t in res)
    R = (U * S.unsqueeze(-2)) @ V.transpose(-1, -2) - A.double()
    rel = R.flatten(1).norm(dim=1) / A.double().flatten(1).norm(dim=1)
    bound = 3 * 7 * int(res.sweeps.max()) * torch.finfo(F32).eps
    print("many_workgroups residual max", float(rel.max()), "bound", bound)
    assert float(rel.max()) <= bound
    for t in (res.U, res.S, res.V, res.sweeps):
        assert torch.equal(t[0], t[4095])


def _sigma_err(S, sref):
    s = torch.sort(S.double(), descending=True).values
    return float((s - sref).abs().max() / sref[0])


def test_degenerate_data(cuda):
    """Zero, rank-one and badly scaled matrices in one batch of 8 x 8.  The
    sigma bound is 4x the oracle's worst sigma error over the scale-1 matrices
    of this batch (the rank-one matrix and three random ones); the matrices
    scaled by 1e-20 and 2^-66 must meet it "as for scale 1"."""
    R = _rand(3, 8, 8, dtype=F32, seed=41)
    dup = R[0][:, :1].expand(8, 8).contiguous()
    A = torch.stack([torch.zeros(8, 8), dup, R[0] * 1e-20, R[0], R[0] * 2.0 ** -66, R[1], R[2]])
    res = svdj.svd_batched(A.to(cuda))
    assert res.info["engine"] == "kernel"
    U, S, V = (t.cpu() for t in res)
    sweeps = res.sweeps.tolist()
    assert bool(torch.isfinite(U).all()) and bool(torch.isfinite(S).all())
    assert bool(torch.isfinite(V).all())
    assert bool(res.converged.all())
    # zero matrix
    assert sweeps[0] == 1 and bool((S[0] == 0).all())
    assert torch.equal(V[0], torch.eye(8))
    sref = torch.linalg.svd(A.double()).S
    unit = (1, 3, 5, 6)  # the scale-1 matrices
    oracle = max(_sigma_err(svdj.svd(A[i], method="oracle").S, sref[i]) for i in unit)
    for i in (1, 2, 3, 4, 5, 6):
        err = _sigma_err(S[i], sref[i])
        print("degenerate", i, "sigma err over sigma_max", err, "oracle worst", oracle,
              "sweeps", sweeps[i])
        assert err <= 4.0 * oracle
    # eight copies of one column: sigma = (sqrt(8) ||c||, 0, ..., 0)
    assert int((S[1] > 4.0 * oracle * S[1].max()).sum()) == 1
    # an exact power-of-two scale changes sigma by that factor and nothing else
    assert torch.equal(S[4], S[3] * 2.0 ** -66)
    assert torch.equal(U[4], U[3]) and torch.equal(V[4], V[3]) and sweeps[4] == sweeps[3]


def test_absolute_tolerance(cuda):
    """tol_mode="absolute" means |a_p.a_q| > tol on the caller's matrix,
    whatever the kernel's internal power-of-two scaling: on A, 2^3 A and
    2^-70 A with one tol, the sweeps equal those of the scalar path with the
    same ordering (fp64, tol 1e-10: far above the 1e-15 noise of the dot
    products, so the sweep in which the last coupling drops below tol does
    not depend on the summation order), and the couplings left are <= tol."""
    tol = 1e-10
    A0 = _rand(3, 33, 33, dtype=F64, seed=81)
    base = None
    for k in (0, 3, -70):
        A = (A0 * 2.0 ** k).to(cuda)
        res = svdj.svd_batched(A, tol_mode="absolute", tol=tol)
        assert res.info["engine"] == "kernel" and bool(res.converged.all())
        want = [svdj.svd(A[i], method="scalar", ordering="round_robin", tol_mode="absolute",
                         tol=tol).sweeps for i in range(3)]
        print("absolute 2^%d" % k, "sweeps", res.sweeps.tolist(), "scalar", want)
        assert res.sweeps.tolist() == want
        US = (res.U * res.S.unsqueeze(-2)).cpu()
        G = US.transpose(-1, -2) @ US
        offd = (G - torch.diag_embed(torch.diagonal(G, dim1=-2, dim2=-1))).abs().amax()
        dmax = float(torch.diagonal(G, dim1=-2, dim2=-1).max())
        assert float(offd) <= tol + 64 * torch.finfo(F64).eps * dmax
        if k == 0:
            base = res
    assert min(base.sweeps.tolist()) > 1
    # 2^-70 A: every product is below tol, nothing rotates (the scaled matrix would)
    assert res.sweeps.tolist() == [1, 1, 1]
    # a scale with the threshold scaled to match is the same iteration bit for bit
    res = svdj.svd_batched((A0 * 2.0 ** 10).to(cuda), tol_mode="absolute", tol=tol * 2.0 ** 20)  # noqa: E501
    assert torch.equal(res.sweeps, base.sweeps) and torch.equal(res.U, base.U)
    assert torch.equal(res.V, base.V) and torch.equal(res.S, base.S * 2.0 ** 10)


def test_explicit_method_and_bf16(cuda):
    A = _rand(3, 8, 8, dtype=F32, seed=91)
    res = svdj.svd_batched(A.to(cuda), method="oracle")  # a named solver is honoured
    assert res.info["engine"] == "loop"
    _check("method_oracle_8x8", A, res, engine="loop")
    Ab = A.to(torch.bfloat16)
    res = svdj.svd_batched(Ab.to(cuda))
    assert res.info["engine"] == "kernel"
    assert res.U.dtype == torch.bfloat16 and res.V.dtype == torch.bfloat16
    assert res.S.dtype == torch.float32  # the working dtype, on either engine
    loop = svdj.svd_batched(Ab.to(cuda), method="scalar")
    assert loop.info["engine"] == "loop" and loop.S.dtype == torch.float32
    assert loop.U.dtype == torch.bfloat16
    sref = torch.linalg.svd(Ab.double()).S
    for i in range(3):  # bf16-level tolerance 4 sqrt(m) 2^-21, fp32 arithmetic
        assert _sigma_err(res.S[i].cpu(), sref[i]) <= 1e-4


def test_non_finite_input(cuda):
    A = _rand(3, 33, 33, dtype=F32, seed=51)
    B = A.clone()
    B[1, 5, 7] = float("nan")
    clean = svdj.svd_batched(A.to(cuda))
    res = svdj.svd_batched(B.to(cuda))  # returns: the sweep loop is counted
    assert (not bool(res.converged[1])) or (not bool(torch.isfinite(res.S[1]).all()))
    assert int(res.sweeps[1]) <= 60
    for i in (0, 2):
        for name in ("U", "S", "V", "sweeps"):
            assert torch.equal(getattr(res, name)[i], getattr(clean, name)[i]), (name, i)


def test_job_options(cuda):
    A = _rand(3, 37, 33, dtype=F32, seed=61).to(cuda)
    full = svdj.svd_batched(A)
    nov = svdj.svd_batched(A, jobv=svdj.NoVec)
    assert nov.V is None and torch.equal(nov.S, full.S) and torch.equal(nov.U, full.U)
    nou = svdj.svd_batched(A, jobu=svdj.NoVec)
    assert nou.U is None and torch.equal(nou.S, full.S) and torch.equal(nou.V, full.V)
    none = svdj.svd_batched(A, jobu=svdj.NoVec, jobv=svdj.NoVec)
    assert none.U is None and none.V is None and torch.equal(none.S, full.S)
    one = svdj.svd_batched(A, max_sweeps=1)
    assert one.sweeps.tolist() == [1, 1, 1] and not bool(one.converged.any())
    srt = svdj.svd_batched(A, sort=True)
    assert bool((srt.S[:, :-1] >= srt.S[:, 1:]).all())
    _check("jobs_37x33", A.cpu(), srt)


def test_engine_choice_outside_envelope(cuda):
    """65 columns, and an m the size routine rejects: the loop engine runs
    and its results pass the same checks."""
    A = _rand(3, 70, 65, dtype=F32, seed=71)
    _check("loop_70x65", A, svdj.svd_batched(A.to(cuda)), engine="loop")
    m = _largest_m(F32, 64) + 1
    assert svdj.ops.kernels.batched_lds_bytes(F32, m, 64, True) == 0
    A = _rand(3, m, 64, dtype=F32, seed=72)
    _check(f"loop_{m}x64", A, svdj.svd_batched(A.to(cuda)), engine="loop")
    inside = svdj.svd_batched(A[:, : m - 1].to(cuda))
    assert inside.info["engine"] == "kernel"
