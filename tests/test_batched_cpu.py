"""svd_batched without a GPU: the loop engine on the CPU oracle, and the host
side of the batched kernel (LDS size routine, argument validation), which
runs before any HIP call."""
import ctypes as C

import pytest
import torch

import svdj


def _rand(*shape, dtype=torch.float64, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, dtype=dtype, generator=g)


def _recon(U, S, V):
    return (U * S.unsqueeze(-2)) @ V.transpose(-1, -2)


@pytest.mark.parametrize("shape", [(5, 7, 4), (2, 3, 6, 6), (4, 3, 9)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_shapes_dtypes_and_reconstruction(shape, dtype):
    A = _rand(*shape, dtype=dtype, seed=1)
    res = svdj.svd_batched(A)
    U, S, V = res
    lead, (m, n) = shape[:-2], shape[-2:]
    k = min(m, n)
    assert U.shape == (*lead, m, k) and S.shape == (*lead, k) and V.shape == (*lead, n, k)
    assert U.dtype == S.dtype == V.dtype == dtype
    assert res.sweeps.shape == lead and res.sweeps.dtype == torch.int32
    assert res.converged.shape == lead and res.converged.dtype == torch.bool
    assert res.off.shape == lead
    assert bool(res.converged.all())
    assert res.info["engine"] == "loop"
    assert res.seconds >= 0.0
    eps = torch.finfo(dtype).eps
    err = (_recon(U, S, V) - A).abs().max()
    assert float(err) <= 50 * eps * float(A.abs().max()) * max(m, n)
    eye = torch.eye(k, dtype=dtype)
    assert float((U.transpose(-1, -2) @ U - eye).abs().max()) <= 50 * eps * m
    assert float((V.transpose(-1, -2) @ V - eye).abs().max()) <= 50 * eps * n


def test_wide_is_swapped_transpose():
    A = _rand(4, 3, 9, seed=2)
    Uw, Sw, Vw = svdj.svd_batched(A)
    Ut, St, Vt = svdj.svd_batched(A.transpose(1, 2).contiguous())
    assert torch.equal(Sw, St) and torch.equal(Uw, Vt) and torch.equal(Vw, Ut)


def test_sort_descending_and_consistent():
    A = _rand(6, 8, 5, seed=3)
    U0, S0, V0 = svdj.svd_batched(A)
    U, S, V = svdj.svd_batched(A, sort=True)
    assert bool((S[:, :-1] >= S[:, 1:]).all())
    order = torch.argsort(S0, dim=-1, descending=True)
    for i in range(A.shape[0]):
        assert torch.equal(S[i], S0[i][order[i]])
        assert torch.equal(U[i], U0[i][:, order[i]])
        assert torch.equal(V[i], V0[i][:, order[i]])
    assert float((_recon(U, S, V) - A).abs().max()) < 1e-13


def test_novec_returns_none():
    A = _rand(3, 6, 4, seed=4)
    full = svdj.svd_batched(A)
    r = svdj.svd_batched(A, jobu=svdj.NoVec)
    assert r.U is None and r.V is not None
    assert torch.allclose(r.S, full.S, rtol=1e-12, atol=0)
    r = svdj.svd_batched(A, jobv=svdj.NoVec)
    assert r.V is None and r.U is not None
    r = svdj.svd_batched(A, jobu="n", jobv="n")
    assert r.U is None and r.V is None and r.S.shape == (3, 4)
    # on a wide input the sides follow the input, not the transposed problem
    r = svdj.svd_batched(_rand(3, 4, 6, seed=5), jobu=svdj.NoVec)
    assert r.U is None and r.V.shape == (3, 6, 4)


def test_empty_batch():
    res = svdj.svd_batched(torch.empty(0, 5, 3))
    assert res.U.shape == (0, 5, 3) and res.S.shape == (0, 3) and res.V.shape == (0, 3, 3)
    assert res.sweeps.shape == (0,) and res.converged.shape == (0,) and res.off.shape == (0,)
    res = svdj.svd_batched(torch.empty(2, 0, 3, 5))
    assert res.U.shape == (2, 0, 3, 3) and res.S.shape == (2, 0, 3) and res.V.shape == (2, 0, 5, 3)


def test_rejects_bad_input():
    with pytest.raises(ValueError, match=r"svd\(\)"):
        svdj.svd_batched(torch.rand(4, 3))
    with pytest.raises(TypeError):
        svdj.svd_batched(torch.ones(2, 4, 3, dtype=torch.int64))
    with pytest.raises(ValueError):  # svd() itself still takes one matrix only
        svdj.svd(torch.rand(2, 4, 3))


def test_max_sweeps_reported_per_matrix():
    A = _rand(3, 6, 6, seed=6)
    res = svdj.svd_batched(A, max_sweeps=1)
    assert res.sweeps.tolist() == [1, 1, 1]
    assert not bool(res.converged.any())
    eye = torch.eye(6, dtype=torch.float64).expand(2, 6, 6)
    res = svdj.svd_batched(eye)
    assert res.sweeps.tolist() == [1, 1] and bool(res.converged.all())


def test_bf16_in_bf16_out():
    A = _rand(2, 8, 5, dtype=torch.float32, seed=7).to(torch.bfloat16)
    res = svdj.svd_batched(A)
    assert res.U.dtype == torch.bfloat16 and res.V.dtype == torch.bfloat16
    assert res.S.dtype == torch.float32  # S in the working dtype
    err = (_recon(res.U.float(), res.S.float(), res.V.float()) - A.float()).abs().max()
    assert float(err) < 0.05


# --------------------------------------------------------- host side, no device
def test_lds_bytes_pinned():
    """csrc/hip/batched.hip batched_layout: A image n * lda elements, lda the
    smallest value >= m that is 8 (mod 32); V image n * ldv likewise when V is
    wanted; 64 elements of sigma; 128 bytes of flags."""
    f = svdj.ops.kernels.batched_lds_bytes
    f32, f64 = torch.float32, torch.float64
    assert f(f32, 256, 64, True) == 264 * 64 * 4 + 72 * 64 * 4 + 64 * 4 + 128 == 86400
    assert f(f32, 256, 64, False) == 264 * 64 * 4 + 64 * 4 + 128 == 67968
    assert f(f64, 64, 64, True) == 2 * 72 * 64 * 8 + 64 * 8 + 128 == 74368
    assert f(f64, 64, 64, False) == 37504
    assert f(f32, 1, 1, True) == 8 * 4 + 8 * 4 + 256 + 128 == 448
    assert f(f32, 5, 3, True) == 576
    assert f(f64, 37, 33, True) == 2 * 40 * 33 * 8 + 512 + 128 == 21760
    # the 163840-byte cap
    assert f(f32, 552, 64, True) == 160128 and f(f32, 553, 64, True) == 0
    assert f(f64, 232, 64, True) == 156288 and f(f64, 233, 64, True) == 0
    # outside the envelope
    assert f(f32, 64, 65, True) == 0 and f(f32, 3, 5, True) == 0 and f(f32, 4, 0, True) == 0
    assert int(svdj.ops.hip_lib().svdj_batched_lds_bytes(2, 8, 8, 1)) == 0


def test_threads_pinned():
    """8 lanes per column pair of a step, whole waves."""
    f = svdj.ops.kernels.batched_threads
    assert [f(n) for n in (1, 2, 8, 16, 17, 32, 33, 48, 49, 63, 64)] == \
        [64, 64, 64, 64, 128, 128, 192, 192, 256, 256, 256]
    assert f(0) == 0 and f(65) == 0


def test_explicit_method_runs_the_loop():
    A = _rand(2, 6, 4, seed=8)
    res = svdj.svd_batched(A, method="oracle", ordering="round_robin")
    assert res.info["engine"] == "loop" and bool(res.converged.all())


def _call(dtype=0, batch=2, m=8, n=8, A=1, S=1, max_sweeps=60, sweeps=1, off=1):
    """svdj_batched_svd with fake non-NULL pointers: every case here returns
    before the first HIP call, so none is ever dereferenced."""
    lib = svdj.ops.hip_lib()
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    null = C.c_void_p(0)
    rc = lib.svdj_batched_svd(dtype, batch, m, n, p if A else null, m * n, n, 1, p,
                              p if S else null, p, 1e-6, 0, max_sweeps, p if sweeps else null,
                              p if off else null, null)
    return rc, lib.svdj_hip_last_error().decode()


@pytest.mark.parametrize("bad", [dict(m=4, n=8), dict(m=80, n=65), dict(m=553, n=64),
                                 dict(dtype=1, m=233, n=64), dict(A=0), dict(S=0),
                                 dict(dtype=2), dict(dtype=-1), dict(max_sweeps=-1),
                                 dict(batch=-1), dict(n=0, m=0)])
def test_entry_point_rejects_bad_arguments(bad):
    rc, msg = _call(**bad)
    assert rc == -2 and msg.startswith("batched_svd:") and len(msg) > 14


def test_entry_point_empty_batch():
    assert _call(batch=0)[0] == 0
    assert _call(batch=0, A=0, S=0, sweeps=0, off=0)[0] == 0
