"""Public API on CPU tensors (oracle / torch-reference paths)."""
import pytest
import torch

import svdj


@pytest.mark.parametrize("method", ["oracle", "scalar", "block"])
def test_svd_methods_cpu(method):
    A = svdj.utils.inputs.random_dense(100, 64, seed=2)
    res = svdj.svd(A, method=method, dtype=torch.float64)
    rep = svdj.utils.metrics.verify(A, res.U, res.S, res.V, torch.linalg.svdvals(A))
    assert res.converged
    assert rep["residual_rel"] < 1e-12 and rep["sigma_max_abs_err_over_smax"] < 1e-12, rep
    assert res.U.shape == (100, 64) and res.V.shape == (64, 64) and res.S.shape == (64,)


def test_wide_matrix_transposes():
    A = svdj.utils.inputs.random_dense(40, 70, seed=4)
    res = svdj.svd(A)
    assert res.info.get("transposed")
    assert res.U.shape == (40, 40) and res.V.shape == (70, 40)
    rep = svdj.utils.metrics.verify(A, res.U, res.S, res.V, torch.linalg.svdvals(A))
    assert rep["residual_rel"] < 1e-12


def test_sort_and_novec():
    A = svdj.utils.inputs.random_dense(50, 50, seed=5)
    res = svdj.svd(A, sort=True)
    assert torch.all(res.S[:-1] >= res.S[1:])
    r2 = svdj.svd(A, jobu=svdj.NoVec, jobv=svdj.NoVec)
    assert r2.U is None and r2.V is None
    torch.testing.assert_close(torch.sort(r2.S, descending=True).values, res.S)


def test_known_spectrum_graded():
    s = svdj.utils.inputs.geometric_spectrum(64, 1e8)
    A = svdj.utils.inputs.with_spectrum(80, 64, s)
    res = svdj.svd(A, method="oracle", sort=True)
    rel = ((res.S - s).abs() / s).max()
    assert rel < 1e-7  # one-sided Jacobi: relative accuracy on graded spectra


def test_gesvd_inplace_cpu():
    n, lda = 48, 64
    A = svdj.utils.inputs.random_dense(n, n, seed=6)
    buf = torch.zeros(lda * n, dtype=torch.float64)
    buf.view(n, lda)[:, :n] = A.t()
    s = torch.zeros(n, dtype=torch.float64)
    V = torch.zeros(n * n, dtype=torch.float64)
    svdj.gesvd(svdj.AllVec, svdj.AllVec, n, n, buf, lda, s, V, n)
    U = buf.view(n, lda)[:, :n].t()
    rep = svdj.utils.metrics.verify(A, U, s, V.view(n, n).t(), torch.linalg.svdvals(A))
    assert rep["residual_rel"] < 1e-12 and rep["orth_u_fro"] < 1e-12


def test_options_parse():
    assert svdj.SVDOptions.parse("A") == svdj.AllVec
    assert svdj.SVDOptions.parse("some") == svdj.SomeVec
    assert svdj.SVDOptions.parse(2) == svdj.NoVec
    with pytest.raises(ValueError):
        svdj.SVDOptions.parse("bogus")


def test_reference_ops_block_step_orthogonalises_pair():
    R = svdj.ops.reference
    W, m = 8, 50
    At = torch.rand(4 * W, m, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    Vt = torch.eye(4 * W, dtype=torch.float64)
    D = (At ** 2).sum(1)
    A0 = At.clone()
    mx, nrot = R.block_step(At, Vt, D, torch.tensor([[0, 1], [2, 3]]), W, True, 1e-14, 30)
    assert nrot == 2 and mx > 0.1
    G = At @ At.t()
    for blk in ([0, 1], [2, 3]):
        cols = torch.cat([torch.arange(b * W, (b + 1) * W) for b in blk])
        g = G[cols][:, cols]
        off = g - torch.diag(torch.diagonal(g))
        assert off.abs().max() < 1e-10 * g.diagonal().max()
    torch.testing.assert_close(Vt @ A0, At, atol=1e-12, rtol=0)  # A_new = A_old V (Vt rows = V cols)
    torch.testing.assert_close(D, torch.diagonal(G), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("method", ["oracle", "block"])
def test_qr_preconditioned_tall_skinny(method):
    """m >= 2n: A = QR, Jacobi on R, U = Q U_R (models/precondition.py)."""
    A = svdj.utils.inputs.random_dense(400, 96, seed=12)
    res = svdj.svd(A, method=method, dtype=torch.float64, precondition="qr")
    assert res.info.get("precondition") == "qr"
    assert svdj.svd(torch.rand(900, 100, dtype=torch.float64), method=method).info.get(
        "precondition") == "qr"  # auto: m >= qr_ratio (2) n
    rep = svdj.utils.metrics.verify(A, res.U, res.S, res.V, torch.linalg.svdvals(A))
    assert rep["residual_rel"] < 1e-12 and rep["orth_u_fro"] < 1e-10, rep
    assert res.U.shape == (400, 96)
    plain = svdj.svd(A, method=method, dtype=torch.float64, precondition="none")
    assert "precondition" not in plain.info
    # flop accounting: QR + sweeps on n x n + GEMM
    m, n = A.shape
    assert res.info["flops"] == svdj.models.precondition.flops(m, n, res.sweeps, True)


def test_bf16_mode_cpu():
    """bf16 problem: bf16 in/out, fp32 working copies, bf16-level stop test."""
    A = svdj.utils.inputs.random_dense(120, 96, seed=13).to(torch.bfloat16)
    res = svdj.svd(A, method="block")
    assert res.U.dtype == torch.bfloat16 and res.V.dtype == torch.bfloat16
    assert res.S.dtype == torch.float32
    assert res.info["bf16"] and res.info["mma"] == "bf16x3"
    ref = torch.linalg.svdvals(A.double())
    rep = svdj.utils.metrics.verify(A.double(), res.U, res.S, res.V, ref)
    assert rep["sigma_max_abs_err_over_smax"] < 1e-4, rep
    assert rep["residual_rel"] < 2e-2, rep  # U, V rounded to bf16
    cfg = svdj.SolverConfig(dtype=torch.bfloat16)
    assert cfg.resolved_dtype(None) == torch.float32 and cfg.precision_dtype(None) == torch.bfloat16


def test_cholqr2_matches_householder():
    pre = svdj.models.precondition
    A = svdj.utils.inputs.random_dense(500, 80, seed=16)
    Q, R = pre.qr(A, torch.float64, method="cholqr2")
    torch.testing.assert_close(Q @ R, A, rtol=1e-12, atol=1e-12)
    eye = torch.eye(80, dtype=torch.float64)
    assert (Q.t() @ Q - eye).abs().max() < 1e-13
    assert torch.allclose(R, torch.triu(R))
    B = A @ torch.diag(torch.logspace(0, -12, 80, dtype=torch.float64))  # kappa ~ 1e12
    with pytest.raises(RuntimeError):
        pre.qr(B, torch.float64, method="cholqr2")
    Q2, R2 = pre.qr(B, torch.float64, method="householder")
    torch.testing.assert_close(Q2 @ R2, B, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("order", ["cyclic", "bipartite"])
def test_block_inner_order_cpu(order):
    """Block path on CPU (reference kernels) with both EVD orderings of the
    cross steps: converges to the same SVD, sweep counts within one or two."""
    A = svdj.utils.inputs.random_dense(200, 128, seed=21)
    res = svdj.svd(A, method="block", dtype=torch.float64,
                   inner_order=order, precondition="none")
    assert res.converged, res.history
    rep = svdj.utils.metrics.verify(A, res.U, res.S, res.V, torch.linalg.svdvals(A))
    assert rep["residual_rel"] < 1e-12 and rep["orth_v_fro"] < 1e-11, rep
    with pytest.raises(ValueError):
        svdj.svd(A, method="block", inner_order="sideways")


@pytest.mark.parametrize("order", ["bipartite", "cross"])
def test_block_cpu_inner_orders_converge(svdj, order):
    """CPU oracle path of the block solver with the bipartite and cross-only
    cross-step EVDs (ops/reference.py jacobi_evd): converged, fp64-accurate."""
    import torch
    A = svdj.utils.inputs.random_dense(200, 160, dtype=torch.float64, seed=4)
    res = svdj.svd(A, method="block", block=32, inner_order=order)
    assert res.converged, res.history
    rep = svdj.utils.metrics.verify(A, res.U, res.S, res.V, torch.linalg.svdvals(A))
    assert rep["residual_rel"] < 1e-12 and rep["sigma_max_abs_err_over_smax"] < 1e-12, rep
    assert rep["orth_u_fro"] < 1e-10 and rep["orth_v_fro"] < 1e-10, rep


def test_block_converges_on_reference_triangular_input(svdj):
    """The reference's default input (upper-triangular U(0,1), numerically
    singular: sigma_min / sigma_max ~ 2^-n) converges, with U and V
    orthogonal: one-sided Jacobi keeps relative accuracy for the tiny
    columns (the underflow floor, ops.kernels.norm_floor, only acts far
    below them at this size)."""
    import torch
    A = svdj.utils.inputs.reference_triu(160)
    res = svdj.svd(A, method="block", block=32, max_sweeps=40)
    assert res.converged and res.sweeps < 40, res.history
    V, U, S = res.V, res.U, res.S
    assert (V.t() @ V - torch.eye(160, dtype=V.dtype)).norm() < 1e-10
    assert (U.t() @ U - torch.eye(160, dtype=U.dtype)).norm() < 1e-8
    assert (A @ V - U * S).norm() / A.norm() < 1e-12


def test_norm_floor_skips_underflowing_columns(svdj):
    """A pair whose column's squared norm is at or below the underflow floor
    is not rotated (ops/reference.py mirrors block_evd.hpp needs_rotation)."""
    import torch
    K, R = svdj.ops.kernels, svdj.ops.reference
    assert K.norm_floor(torch.float64, 1000) == 1000 * torch.finfo(torch.float64).tiny / \
        torch.finfo(torch.float64).eps
    G = torch.tensor([[[1.0, 0.5, 0.0, 0.0], [0.5, 1.0, 0.0, 0.0],
                       [0.0, 0.0, 1e-300, 5e-301], [0.0, 0.0, 5e-301, 1e-300]]],
                     dtype=torch.float64)
    _, _, rot = R.jacobi_evd(G, 1e-14, 1, floor=K.norm_floor(torch.float64, 8))
    assert bool(rot[0])                      # the (0, 1) pair rotates
    G[0, 0, 1] = G[0, 1, 0] = 0.0
    _, Q, rot = R.jacobi_evd(G, 1e-14, 1, floor=K.norm_floor(torch.float64, 8))
    assert not bool(rot[0])                  # the underflowing (2, 3) pair does not
    _, _, rot = R.jacobi_evd(G, 1e-14, 1, floor=0.0)
    assert bool(rot[0])


@pytest.mark.parametrize("scale", [1.0, 1e-16, 2.0 ** 40])
def test_block_solve_is_scale_invariant(svdj, scale):
    """c A solves like A: the negligible-column floor is relative
    to the matrix's largest squared column norm, so a well-conditioned fp32
    matrix with entries ~1e-16 is rotated (the round-3 absolute floor m realmin
    / eps skipped every pair and returned A's normalised columns as U)."""
    import torch
    A = svdj.utils.inputs.random_dense(96, 64, dtype=torch.float64, seed=4).float()
    ref = torch.linalg.svdvals(A.double())
    res = svdj.svd(A * scale, method="block", block=32, sort=True)
    assert res.converged
    S = res.S.double() / scale
    assert float(((S - ref).abs() / ref[0]).max()) < 1e-5
    U = res.U.double()
    assert float((U.t() @ U - torch.eye(64, dtype=torch.float64)).abs().max()) < 1e-4


def test_norm_floor_relative_to_scale(svdj):
    import torch
    K = svdj.ops.kernels
    fi = torch.finfo(torch.float32)
    assert K.norm_floor(torch.float32, 100, 1.0) == 100 * fi.tiny / fi.eps
    assert K.norm_floor(torch.float32, 100, 1e-30) == 100 * fi.tiny  # absolute guard
    assert K.norm_floor(torch.float32, 100, 4.0) == 4 * 100 * fi.tiny / fi.eps


@pytest.mark.parametrize("shape,jobs", [((220, 160), ("A", "A")), ((130, 200), ("A", "A")),
                                        ((200, 128), ("N", "A")), ((200, 128), ("A", "N"))])
def test_block_engines_agree_cpu(shape, jobs):
    """svd()'s two single-device engines (models/block.py choose_engine): the
    pipeline (the distributed plan at P = 1, what a GPU runs by default) and
    the single-stream round robin give the same factorisation quality, for
    tall and wide inputs and every job option."""
    A = svdj.utils.inputs.random_dense(*shape, dtype=torch.float64, seed=21)
    ref = torch.linalg.svdvals(A)
    out = {}
    for eng in ("pipeline", "steps"):
        r = svdj.svd(A, *jobs, method="block", device="cpu", block=32, extra={"engine": eng})
        assert r.converged and r.info["engine"] == eng and r.info["block"] == 32
        assert float((r.S.sort(descending=True).values - ref).abs().max() / ref[0]) < 1e-13
        if r.U is not None and r.V is not None:
            assert float((A @ r.V - r.U * r.S).norm() / A.norm()) < 1e-13
        assert (r.U is None) == (jobs[0] == "N" if shape[0] >= shape[1] else jobs[1] == "N")
        out[eng] = r
    assert abs(out["pipeline"].sweeps - out["steps"].sweeps) <= 2


def test_block_engine_choice():
    from svdj.models.block import choose_engine

    cfg = svdj.SolverConfig()
    assert choose_engine(cfg, torch.device("cuda", 0)) == "pipeline"
    assert choose_engine(cfg, torch.device("cpu")) == "steps"
    assert choose_engine(svdj.SolverConfig(extra={"engine": "steps"}), torch.device("cuda", 0)) == "steps"
    with pytest.raises(ValueError):
        choose_engine(svdj.SolverConfig(extra={"engine": "fast"}), torch.device("cpu"))


def test_local_communicator_is_world_one():
    from svdj.parallel import Communicator

    c = Communicator.local("cpu")
    assert (c.rank, c.world, c.distributed) == (0, 1, False)
    t = torch.arange(6.0)
    assert torch.equal(c.ordered_sum_(t.clone()), t) and c.max_over_ranks(2.5) == 2.5


def test_quad_gram_parts_follow_the_rotation_count(monkeypatch):
    """The quad Gram runs on 2 bf16 parts while the previous sweep rotated
    every block pair (and in the first sweep), on 3 parts afterwards; SVDJ_DEBUG
    gram2=0 keeps 3 parts throughout (parallel/distributed.py; libsvdj_dist has
    the same rule).  The CPU emulation keeps the exact Gram, so both runs give
    the same result -- here only the requests are checked."""
    from svdj.ops import kernels as K
    from svdj.parallel import Communicator, DistributedBlockJacobi

    A = torch.rand(512, 512, generator=torch.Generator().manual_seed(0))
    cfg = svdj.SolverConfig(dtype=torch.float32, block=64, quad="on", mma="bf16x6")
    orig = K.block_steps
    runs = {}
    for dbg in (None, "gram2=0"):
        if dbg is None:
            monkeypatch.delenv("SVDJ_DEBUG", raising=False)
        else:
            monkeypatch.setenv("SVDJ_DEBUG", dbg)
        calls = []

        def wrap(*a, **kw):
            calls.append(kw.get("gram_parts", 3))
            return orig(*a, **kw)

        monkeypatch.setattr(K, "block_steps", wrap)
        res = DistributedBlockJacobi(cfg, Communicator.local("cpu")).solve(A)
        runs[dbg] = (calls, res)
    calls, res = runs[None]
    assert res.info["quad"]
    n2 = calls.count(2)
    assert calls[0] == 2 and 0 < n2 < len(calls)
    assert calls == [2] * n2 + [3] * (len(calls) - n2), calls  # one switch, never back
    work = res.info["work"]
    assert 0 < work["gram_quads2"] < work["gram_quads"]
    calls0, res0 = runs["gram2=0"]
    assert set(calls0) == {3} and res0.info["work"]["gram_quads2"] == 0
    assert res0.sweeps == res.sweeps and torch.equal(res0.S, res.S)
