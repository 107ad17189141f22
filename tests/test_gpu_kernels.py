"""HIP kernel numerics vs plain-PyTorch fp64 references (needs MI355X)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _rand_At(ncols, m_pad, m, dtype, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    At = torch.zeros(ncols, m_pad, dtype=torch.float64)
    At[:, :m] = torch.rand(ncols, m, generator=g, dtype=torch.float64) - 0.3
    return At.to(dtype).to(device)


def test_native_loaded(svdj, cuda):
    lib = svdj.ops.hip_lib()
    assert b"gfx950" in lib.svdj_hip_version()
    assert torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_col_norms_finalize_identity(svdj, cuda, dtype):
    K = svdj.ops.kernels
    At = _rand_At(40, 256, 200, dtype, cuda)
    D = K.col_norms2(At, 256)
    ref = (At.double().cpu() ** 2).sum(1)
    torch.testing.assert_close(D.double().cpu(), ref, rtol=1e-5 if dtype == torch.float32 else 1e-12, atol=0)
    A0 = At.double().cpu().clone()
    s = K.finalize(At, 256, True)
    torch.testing.assert_close(s.double().cpu(), ref.sqrt(), rtol=1e-6 if dtype == torch.float32 else 1e-13, atol=0)
    torch.testing.assert_close(At.double().cpu(), A0 / ref.sqrt()[:, None], rtol=1e-5 if dtype == torch.float32 else 1e-12, atol=1e-7)
    V = torch.full((40, 128), 7.0, dtype=dtype, device=cuda)
    K.set_identity(V, 40)
    assert torch.equal(V.cpu(), torch.eye(40, 128, dtype=dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_scalar_step_matches_reference(svdj, cuda, dtype):
    K = svdj.ops.kernels
    R = svdj.ops.reference
    n, m, m_pad = 32, 300, 384
    At = _rand_At(n, m_pad, m, dtype, cuda, seed=1)
    Vt = torch.eye(n, 128, dtype=dtype, device=cuda)
    sched = torch.from_numpy(svdj.parallel.schedule.sameh(n)).to(cuda)
    At_ref, Vt_ref = At.double().cpu(), Vt.double().cpu()
    metric = K.new_metric(cuda)
    tol = 1e-7
    for s in range(3):
        K.scalar_step(At, Vt, m_pad, sched[s], tol, 0, metric)
        R.scalar_step(At_ref, Vt_ref, sched[s].cpu(), tol, 0)
    mx, nrot = K.read_metric(metric)
    assert nrot == 3 * (n // 2)
    assert 0 < mx <= 1
    tol_cmp = 2e-5 if dtype == torch.float32 else 1e-12
    torch.testing.assert_close(At.double().cpu(), At_ref, rtol=tol_cmp, atol=tol_cmp)
    torch.testing.assert_close(Vt.double().cpu(), Vt_ref, rtol=tol_cmp, atol=tol_cmp)


@pytest.mark.parametrize("dtype,W,mma", [(torch.float32, 32, "native"), (torch.float32, 64, "native"),
                                         (torch.float64, 32, "native"), (torch.float64, 64, "native"),
                                         (torch.float32, 32, "bf16x6"), (torch.float32, 64, "bf16x6")])
@pytest.mark.parametrize("full", [1, 0])
def test_block_step_matches_reference(svdj, cuda, dtype, W, mma, full):
    """One gram -> evd -> apply step vs the fp64 torch reference on the same input."""
    K = svdj.ops.kernels
    R = svdj.ops.reference
    nb = 4
    n, m, m_pad = nb * W, 500, 512
    At = _rand_At(n, m_pad, m, dtype, cuda, seed=2)
    if not full:
        # cross mode assumes blocks internally orthogonal: orthogonalise each block
        A64 = At.double().cpu()
        for b in range(nb):
            blk = A64[b * W:(b + 1) * W, :m]
            q, r = torch.linalg.qr(blk.t())
            A64[b * W:(b + 1) * W, :m] = (q * torch.linspace(1, 3, W, dtype=torch.float64)).t()
        At = A64.to(dtype).to(cuda)
    Vt = torch.zeros(n, 256, dtype=dtype, device=cuda)
    K.set_identity(Vt, n)
    D = K.col_norms2(At, m_pad)
    pairs = torch.tensor([[[0, 3], [1, 2]]], dtype=torch.int32)
    At64, Vt64, D64 = At.double().cpu(), Vt.double().cpu(), D.double().cpu()
    tol = 1e-6 if dtype == torch.float32 else 1e-13
    metric = K.new_metric(cuda)
    K.block_steps(At, Vt, D, m_pad, pairs.to(cuda), W, [full], tol, 12, metric, mma=mma)
    mx_ref, nrot_ref = R.block_step(At64, Vt64, D64, pairs[0], W, bool(full), tol, 12)
    mx, nrot = K.read_metric(metric)
    assert nrot == nrot_ref == 2
    assert math.isclose(mx, mx_ref, rel_tol=1e-3)
    # Columns of the rotated panels must be mutually orthogonal and span the
    # same space as the reference: compare the invariants, not the (sign /
    # order ambiguous) individual columns.
    Ag = At.double().cpu()
    for bi, bj in pairs[0].tolist():
        cols = list(range(bi * W, bi * W + W)) + list(range(bj * W, bj * W + W))
        X = Ag[cols, :m]
        G = X @ X.t()
        off = G - torch.diag(torch.diagonal(G))
        dg = torch.diagonal(G).sqrt()
        rel = (off.abs() / (dg[:, None] * dg[None, :])).max()
        assert rel < (5e-5 if dtype == torch.float32 else 1e-11), rel
        # squared norms tracked in D equal the data's
        torch.testing.assert_close(D.double().cpu()[cols], torch.diagonal(G), rtol=1e-4 if dtype == torch.float32 else 1e-10, atol=1e-6)
        # same singular values of the pair panel
        torch.testing.assert_close(torch.sort(torch.diagonal(G)).values, torch.sort(D64[cols]).values,
                                   rtol=1e-4 if dtype == torch.float32 else 1e-10, atol=1e-6)
        # A V = A0 V0 relation: X_new = X_old Q => X_new^T X_new eigenvalues
    # V stays orthogonal and A_new = A_old_full * V (columns) holds
    Vg = Vt.double().cpu()
    # fp32 W=32 accumulates Q in fp64 (orthogonal to ~eps); fp32 W=64 in fp32.
    vtol = {(torch.float32, 32): 2e-6, (torch.float32, 64): 5e-5}.get((dtype, W), 1e-13)
    torch.testing.assert_close(Vg[:, :n] @ Vg[:, :n].t(), torch.eye(n, dtype=torch.float64),
                               rtol=0, atol=vtol)


# (residual, sigma, ||U^TU-I||, ||V^TV-I||) bounds ~5x the values measured on
# MI355X with the default sqrt(m) eps threshold (tools/measure_test_accuracy.py)
_E2E_BOUNDS = {
    ("block", torch.float32, "native"): (8e-6, 1e-6, 1.5e-3, 2e-4),
    ("block", torch.float32, "bf16x6"): (8e-6, 1e-6, 1.5e-3, 2e-4),
    ("block", torch.float64, "native"): (2e-12, 1e-12, 2e-12, 1.5e-11),
    ("scalar", torch.float32, "native"): (2e-4, 4e-5, 1.5e-3, 8e-3),
    ("scalar", torch.float64, "native"): (5e-13, 3e-13, 2e-12, 8e-12),
}


@pytest.mark.parametrize("method,dtype,mma", [("block", torch.float32, "native"),
                                              ("block", torch.float32, "bf16x6"),
                                              ("block", torch.float64, "native"),
                                              ("scalar", torch.float32, "native"),
                                              ("scalar", torch.float64, "native")])
def test_svd_end_to_end(svdj, cuda, method, dtype, mma):
    m, n = 520, 384
    A = svdj.utils.inputs.random_dense(m, n, dtype=torch.float64, seed=3)
    res = svdj.svd(A.to(cuda), method=method, dtype=dtype, mma=mma)
    assert res.converged, res.history
    rep = svdj.utils.metrics.verify(A.to(cuda), res.U, res.S, res.V, torch.linalg.svdvals(A))
    r, sg, ou, ov = _E2E_BOUNDS[(method, dtype, mma)]
    assert rep["residual_rel"] < r and rep["sigma_max_abs_err_over_smax"] < sg, rep
    assert rep["orth_u_fro"] < ou and rep["orth_v_fro"] < ov, rep


def test_gesvd_inplace_reference_signature(svdj, cuda):
    n = 256
    A = svdj.utils.inputs.reference_dense(n).to(cuda)  # column-major view of a buffer
    buf = A.t().contiguous().reshape(-1).clone()  # column-major storage, lda = n
    s = torch.zeros(n, dtype=torch.float64, device=cuda)
    V = torch.zeros(n * n, dtype=torch.float64, device=cuda)
    res = svdj.gesvd(svdj.AllVec, svdj.AllVec, n, n, buf, n, s, V, n)
    U = buf.view(n, n).t()
    Vm = V.view(n, n).t()
    rep = svdj.utils.metrics.verify(A, U, s, Vm, torch.linalg.svdvals(A.cpu()))
    assert rep["residual_rel"] < 1e-12 and rep["orth_u_fro"] < 1e-9, rep
    assert res.sweeps >= 2


def test_block_bf16x3_fast_mode(svdj, cuda):
    """2-way bf16 split: ~2^-17 accurate products, so the relative threshold
    is set at that level; residual and orthogonality follow it."""
    m, n = 600, 512
    A = svdj.utils.inputs.random_dense(m, n, dtype=torch.float64, seed=8)
    res = svdj.svd(A.to(cuda), method="block", dtype=torch.float32, mma="bf16x3", tol=2e-5)
    assert res.converged, res.history
    rep = svdj.utils.metrics.verify(A.to(cuda), res.U, res.S, res.V, torch.linalg.svdvals(A))
    assert rep["residual_rel"] < 1e-4 and rep["sigma_max_abs_err_over_smax"] < 1e-4, rep
    assert rep["orth_v_fro"] < 1e-2, rep


@pytest.mark.parametrize("W", [32, 64])
def test_bf16x6_matches_native(svdj, cuda, W):
    """bf16x6 apply is as accurate as the f32 MFMA apply.  One step from the
    same input (same Gram and Q in both modes) agrees to fp32 rounding level;
    after a whole sweep (rotation sequences may legitimately diverge) V is
    as orthogonal as with the native apply."""
    K = svdj.ops.kernels
    n = 8 * W
    A = svdj.utils.inputs.random_dense(n, n, dtype=torch.float32, device=cuda, seed=11)
    pairs = torch.from_numpy(svdj.parallel.schedule.round_robin(n // W)).to(cuda)
    eye = torch.eye(n, dtype=torch.float64)
    step, orth = [], []
    for mma in ("native", "bf16x6"):
        for nsteps in (1, n // W - 1):
            At = A.t().contiguous()
            Vt = torch.zeros(n, n, dtype=torch.float32, device=cuda)
            K.set_identity(Vt, n)
            D = K.col_norms2(At, n)
            K.block_steps(At, Vt, D, n, pairs[:nsteps], W, [1] + [0] * (nsteps - 1), 1e-6, 1,
                          K.new_metric(cuda), mma=mma)
            v = Vt.double().cpu()
            if nsteps == 1:
                step.append((At.double().cpu(), v))
            else:
                orth.append(float((v @ v.t() - eye).abs().max()))
    (a0, v0), (a1, v1) = step
    assert (a0 - a1).abs().max() / a0.abs().max() < 2e-6
    assert (v0 - v1).abs().max() < 2e-6
    assert orth[1] < 4 * orth[0] + 1e-6, orth


@pytest.mark.parametrize("dtype,W", [(torch.float32, 32), (torch.float32, 64), (torch.float64, 32),
                                     (torch.float64, 64)])
@pytest.mark.parametrize("full", [1, 0])
def test_block_step_preconverged_pair_skipped(svdj, cuda, dtype, W, full):
    """One pair already orthogonal (its EVD pass is skipped: D untouched in
    cross mode, refreshed in full mode), one not: rotation count and D agree
    with the torch reference (early exit vs rotation test)."""
    K, R = svdj.ops.kernels, svdj.ops.reference
    nb, m, m_pad = 4, 500, 512
    n = nb * W
    g = torch.Generator().manual_seed(4)
    A64 = torch.zeros(n, m_pad, dtype=torch.float64)
    # blocks 0 and 3: one orthogonal 2W-column panel (pair (0, 3) converged)
    q, _ = torch.linalg.qr(torch.rand(m, 2 * W, generator=g, dtype=torch.float64))
    q = q * torch.linspace(1, 4, 2 * W, dtype=torch.float64)
    A64[0:W, :m] = q[:, :W].t()
    A64[3 * W:4 * W, :m] = q[:, W:].t()
    # blocks 1 and 2: each internally orthogonal, coupled to each other
    for b in (1, 2):
        qb, _ = torch.linalg.qr(torch.rand(m, W, generator=g, dtype=torch.float64))
        A64[b * W:(b + 1) * W, :m] = (qb * torch.linspace(1, 3, W, dtype=torch.float64)).t()
    At = A64.to(dtype).to(cuda)
    Vt = torch.zeros(n, 256, dtype=dtype, device=cuda)
    K.set_identity(Vt, n)
    D = K.col_norms2(At, m_pad)
    D0 = D.double().cpu().clone()
    pairs = torch.tensor([[[0, 3], [1, 2]]], dtype=torch.int32)
    At64, Vt64, D64 = At.double().cpu(), Vt.double().cpu(), D.double().cpu()
    tol = 1e-5 if dtype == torch.float32 else 1e-13
    metric = K.new_metric(cuda)
    K.block_steps(At, Vt, D, m_pad, pairs.to(cuda), W, [full], tol, 1, metric)
    _, nrot_ref = R.block_step(At64, Vt64, D64, pairs[0], W, bool(full), tol, 1)
    _, nrot = K.read_metric(metric)
    assert nrot == nrot_ref == 1
    c03 = list(range(0, W)) + list(range(3 * W, 4 * W))
    Dg = D.double().cpu()
    rt = 1e-5 if dtype == torch.float32 else 1e-12
    if not full:
        assert torch.equal(Dg[c03], D0[c03])  # skipped pair: D untouched
    torch.testing.assert_close(Dg[c03], D64[c03], rtol=rt, atol=0)
    # the rotated pair's tracked norms equal its columns' (one EVD sweep leaves
    # the eigenvalue order ordering-dependent, so compare with the data)
    An = At.double().cpu()[W:3 * W, :m]
    torch.testing.assert_close(Dg[W:3 * W], (An * An).sum(1), rtol=1e-4 if dtype == torch.float32
                               else 1e-10, atol=1e-6)
    # the skipped pair's columns of A and V are bit-identical to the input
    assert torch.equal(At.double().cpu()[c03], A64.to(dtype).double()[c03])


def test_block_absolute_threshold_stops(svdj, cuda):
    """tol_mode='absolute' (the reference's |g_pq| > TOLERANCE rule) on the
    block path: the sweeps stop once every |g_pq| is below tol."""
    A = svdj.utils.inputs.random_dense(300, 256, dtype=torch.float64, seed=12)
    res = svdj.svd(A.to(cuda), method="block", dtype=torch.float64, tol_mode="absolute",
                   tol=1e-9, max_sweeps=40)
    assert res.converged and res.sweeps < 40, res.history
    rep = svdj.utils.metrics.verify(A.to(cuda), res.U, res.S, res.V, torch.linalg.svdvals(A))
    assert rep["sigma_max_abs_err_over_smax"] < 1e-12, rep


@pytest.mark.parametrize("W", [32, 64])
def test_fp64_block_widths_end_to_end(svdj, cuda, W):
    """fp64 at both block widths (fp64 W=64: split full Gram, 137 KB LDS EVD,
    147 KB LDS apply) converges to fp64 accuracy against LAPACK's sigma."""
    m, n = 700, 512
    A = svdj.utils.inputs.random_dense(m, n, dtype=torch.float64, seed=21)
    res = svdj.svd(A.to(cuda), method="block", dtype=torch.float64, block=W)
    assert res.converged, res.history
    rep = svdj.utils.metrics.verify(A.to(cuda), res.U, res.S, res.V, torch.linalg.svdvals(A))
    assert rep["residual_rel"] < 5e-12 and rep["sigma_max_abs_err_over_smax"] < 1e-12, rep
    assert rep["orth_u_fro"] < 5e-11 and rep["orth_v_fro"] < 5e-11, rep


@pytest.mark.parametrize("order,inner", [("bipartite", 1), ("cross", 1), ("cross", 3)])
@pytest.mark.parametrize("dtype,W", [(torch.float32, 32), (torch.float32, 64),
                                     (torch.float64, 32), (torch.float64, 64)])
def test_block_step_bipartite_matches_reference(svdj, cuda, dtype, W, order, inner):
    """Cross step with the bipartite EVD ordering (mode 2, block_evd.hpp
    Ord<W, EVD_BIP>: W steps of the cross pairs, DPP rotate + permlane32 swap
    of the register Q) or the cross-only one (mode 3, evd_cross_kernel: the
    same steps tracking only the cross couplings, transpose-pair updates in
    position space) against the fp64 reference with the same ordering, one or
    several inner sweeps: same rotation count, D and rotated panels to
    rounding level."""
    K = svdj.ops.kernels
    R = svdj.ops.reference
    nb = 4
    n, m, m_pad = nb * W, 500, 512
    A64 = _rand_At(n, m_pad, m, torch.float64, "cpu", seed=7)
    for b in range(nb):  # cross steps start from internally orthogonal blocks
        q, _ = torch.linalg.qr(A64[b * W:(b + 1) * W, :m].t())
        A64[b * W:(b + 1) * W, :m] = (q * torch.linspace(1, 3, W, dtype=torch.float64)).t()
    At = A64.to(dtype).to(cuda)
    Vt = torch.zeros(n, 256, dtype=dtype, device=cuda)
    K.set_identity(Vt, n)
    D = K.col_norms2(At, m_pad)
    pairs = torch.tensor([[[0, 3], [1, 2]]], dtype=torch.int32)
    At64, Vt64, D64 = At.double().cpu(), Vt.double().cpu(), D.double().cpu()
    tol = 1e-6 if dtype == torch.float32 else 1e-13
    metric = K.new_metric(cuda)
    K.block_steps(At, Vt, D, m_pad, pairs.to(cuda), W, [0], tol, inner, metric,
                  inner_order=order)
    mx_ref, nrot_ref = R.block_step(At64, Vt64, D64, pairs[0], W, False, tol, inner,
                                    order=order)
    mx, nrot = K.read_metric(metric)
    assert nrot == nrot_ref == 2
    assert math.isclose(mx, mx_ref, rel_tol=1e-3)
    rt = (3e-5 if dtype == torch.float32 else 1e-11) * (1 if inner == 1 else 4)
    torch.testing.assert_close(At.double().cpu()[:, :m], At64[:, :m], rtol=rt, atol=rt)
    torch.testing.assert_close(Vt.double().cpu()[:, :n], Vt64[:, :n], rtol=rt, atol=rt)
    torch.testing.assert_close(D.double().cpu(), D64, rtol=rt, atol=rt)


@pytest.mark.parametrize("order", ["bipartite", "cross"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_svd_end_to_end_bipartite(svdj, cuda, dtype, order):
    """Whole solve with bipartite / cross-only cross steps: same accuracy
    bounds as the cyclic inner ordering."""
    m, n = 520, 384
    A = svdj.utils.inputs.random_dense(m, n, dtype=torch.float64, seed=3)
    res = svdj.svd(A.to(cuda), method="block", dtype=dtype, inner_order=order)
    assert res.converged, res.history
    rep = svdj.utils.metrics.verify(A.to(cuda), res.U, res.S, res.V, torch.linalg.svdvals(A))
    r, sg, ou, ov = _E2E_BOUNDS[("block", dtype, "native")]
    assert rep["residual_rel"] < r and rep["sigma_max_abs_err_over_smax"] < sg, rep
    assert rep["orth_u_fro"] < ou and rep["orth_v_fro"] < ov, rep


@pytest.mark.parametrize("W", [32, 64])
@pytest.mark.parametrize("m,m_pad,rows", [(100, 128, 128), (500, 512, 128), (4000, 4096, 1024),
                                          (5000, 5120, 3072), (3000, 3072, 256)])
def test_gram_cross_matches_reference(svdj, cuda, W, m, m_pad, rows):
    """Cross Gram kernel (fp32, register fragments, split over row chunks)
    vs the fp64 torch product: one to many slabs per chunk, a short last
    chunk, and a leading dimension larger than m_pad."""
    K = svdj.ops.kernels
    nb = 6
    ld = m_pad + 128
    At = torch.zeros(nb * W, ld, dtype=torch.float32, device=cuda)
    At[:, :m_pad] = _rand_At(nb * W, m_pad, m, torch.float32, cuda, seed=5)
    pairs = torch.tensor([[0, 5], [3, 1], [2, 4]], dtype=torch.int32)
    got = K.gram_cross(At, m_pad, pairs, W, rows).double().sum(1).cpu()
    A64 = At.double().cpu()[:, :m_pad]
    for p, (bi, bj) in enumerate(pairs.tolist()):
        ref = A64[bi * W:(bi + 1) * W] @ A64[bj * W:(bj + 1) * W].t()
        scale = ref.abs().max().item()
        assert (got[p] - ref).abs().max().item() < 2e-6 * scale * math.sqrt(m / 100)


@pytest.mark.parametrize("skip_one", [False, True])
@pytest.mark.parametrize("W,mode,mma", [(32, 2, "native"), (64, 3, "native"), (64, 3, "bf16x6")])
def test_single_step_equals_its_hooks(svdj, cuda, W, mode, mma, skip_one):
    """A step of block_steps is, bit for bit, gram_cross -> evd_alone ->
    apply_q per rotated pair: the hooks run the solve's launchers.  4 blocks,
    2 pairs, m_pad = 128: the step's geometry is one 128-row Gram chunk and
    one apply chunk (block_layout.hpp make_geometry), which the hooks are given.
    U(0, 1) columns, so the pairs rotate; ``skip_one``: pair (1, 2) lives on
    disjoint rows (a zero cross Gram), so its skip flag is set."""
    K = svdj.ops.kernels
    nb, m_pad, P, tol, inner = 4, 128, 2, 1e-6, 2
    A = torch.rand(nb * W, m_pad, generator=torch.Generator().manual_seed(11 + W))
    if skip_one:
        A[W:2 * W, 64:] = 0
        A[2 * W:3 * W, :64] = 0
    pairs = torch.tensor([[0, 3], [1, 2]], dtype=torch.int32, device=cuda)
    A0 = A.to(cuda)
    D0 = K.col_norms2(A0, m_pad)
    A1, D1 = A0.clone(), D0.clone()
    K.block_steps(A1, None, D1, m_pad, pairs[None], W, [mode], tol, inner, K.new_metric(cuda),
                  mma=mma)
    # the step's skip flags: skipb[0] of its workspace, behind the slab area
    # and the two Q buffers, here P x 2W x 2W fp32 each (block_layout.hpp solve_layout)
    ws = K.block_workspace(torch.float32, W, P, m_pad, A1.device)
    off = 3 * P * 4 * W * W * 4
    skip1 = ws[off:off + 4 * P].view(torch.int32).clone()
    A2, D2 = A0.clone(), D0.clone()
    slabs = K.gram_cross(A2, m_pad, pairs, W, 128)
    Q, skip2 = K.evd_alone(slabs, D2, pairs, W, mode, tol, inner, K.new_metric(cuda))
    for p, (bi, bj) in enumerate(pairs.tolist()):
        if int(skip2[p]):
            continue
        rows = list(range(bi * W, (bi + 1) * W)) + list(range(bj * W, (bj + 1) * W))
        X = A2[rows].contiguous()
        K.apply_q(X, Q[p], W, mma=mma)
        A2[rows] = X
    assert skip2.tolist() == [0, int(skip_one)] and torch.equal(skip1, skip2)
    assert torch.equal(D1, D2)
    assert torch.equal(A1, A2) and not torch.equal(A1[:W], A0[:W])


@pytest.mark.parametrize("scale", [1.0, 1e-16, 2.0 ** 40])
def test_block_solve_is_scale_invariant_gpu(svdj, cuda, scale):
    """c A solves like A on the GPU kernels (the negligible-column floor is
    relative to the largest squared column norm, svdj_set_norm_floor_scaled),
    at the flagship configuration: W = 64, split-bf16 apply, cross EVD."""
    A = svdj.utils.inputs.random_dense(1100, 1024, dtype=torch.float64, seed=4).float()
    ref = torch.linalg.svdvals(A.double())
    res = svdj.svd((A * scale).to(cuda), method="block", sort=True)
    assert res.converged and res.info["block"] == 64 and res.info["mma"] == "bf16x6", res.info
    S = res.S.double().cpu() / scale
    assert float(((S - ref).abs() / ref[0]).max()) < 2e-6
    U = res.U.double().cpu()
    assert float((U.t() @ U - torch.eye(1024, dtype=torch.float64)).abs().max()) < 1e-4
