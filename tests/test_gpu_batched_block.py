"""svd_batched's "block" engine on the GPU: the stacked batch through the
block path's step kernels with per-matrix stop-test words
(svdj_block_steps_grouped), the pack and finalize kernels of
csrc/hip/batched_block.hip.

Accuracy bounds are 4x the CPU oracle's own worst value over the same
matrices (``svd(A[i], method="oracle")``, same dtype, same tolerance rule),
the convention of tests/test_gpu_batched.py: the factor covers the different
pair order and hence a different rounding trajectory.  Set
SVDJ_BATCHED_ACCURACY_OUT to a file name to append the measured (engine,
oracle) pairs to it as JSON lines.
"""
import json
import os

import pytest
import torch

import svdj
from svdj.models.batched import stacked_pairs

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


def _check(key, A, res):
    got = _metrics(A, res.U, res.S, res.V)
    want = _oracle_metrics(key, A)
    rec = {"case": key, "dtype": str(A.dtype), "shape": list(A.shape), "engine": res.info["engine"],
           "block": res.info.get("block"), "mma": res.info.get("mma"),
           "sweeps": res.sweeps.flatten().tolist(), "svd_batched": got, "oracle": want}
    print(json.dumps(rec))
    out = os.environ.get("SVDJ_BATCHED_ACCURACY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert res.info["engine"] == "block"
    assert bool(res.converged.all()), res.sweeps
    for name in METRICS:
        assert got[name] <= 4.0 * want[name], (name, got[name], want[name])


CASES = [(70, 65, F32), (70, 65, F64), (128, 128, F32), (128, 128, F64), (130, 130, F64),
         (300, 96, F32), (65, 130, F32)]


@pytest.mark.parametrize("m,n,dtype", CASES,
                         ids=[f"{m}x{n}_{'fp32' if d == F32 else 'fp64'}" for m, n, d in CASES])
def test_against_oracle(cuda, m, n, dtype):
    A = _rand(3, m, n, dtype=dtype, seed=1000 + m + n)
    res = svdj.svd_batched(A.to(cuda), batched="block")
    k = min(m, n)
    assert res.U.shape == (3, m, k) and res.S.shape == (3, k) and res.V.shape == (3, n, k)
    assert res.S.dtype == dtype and res.sweeps.dtype == torch.int32
    kb = 2 * -(-k // 64)
    assert res.info["block"] == 32 and res.info["blocks_per_matrix"] == kb
    assert res.info["pairs_per_step"] == 3 * kb // 2 and res.info["chunks"] == 1
    assert res.info["mma"] == "native" and res.info["transposed"] == (m < n)
    _check(f"block_{m}x{n}", A, res)


def test_block64_split_apply_and_cross_evd(cuda):
    """block=64 in fp32: the split-bf16 apply and evd_cross_kernel with
    grouped metrics (k = 4 blocks of 64 for 130 columns)."""
    A = _rand(3, 200, 130, dtype=F32, seed=64)
    res = svdj.svd_batched(A.to(cuda), batched="block", block=64)
    assert res.info["block"] == 64 and res.info["mma"] == "bf16x6"
    assert res.info["blocks_per_matrix"] == 4
    _check("block64_200x130", A, res)


def test_batch_of_one(cuda):
    A = _rand(1, 70, 65, dtype=F32, seed=11)
    res = svdj.svd_batched(A.to(cuda), batched="block")
    assert res.info["pairs_per_step"] == 2
    _check("one_70x65", A, res)


def test_per_matrix_floor(cuda):
    """2^-200 A, A and 2^200 A in one fp64 batch: each has the floor of its
    own scale, so the three iterate alike bit for bit.  With one floor for
    the batch (that of 2^200 A) the small copy would never rotate."""
    A = _rand(70, 65, dtype=F64, seed=21)
    batch = torch.stack([A * 2.0 ** -200, A, A * 2.0 ** 200]).to(cuda)
    res = svdj.svd_batched(batch, batched="block")
    sw = res.sweeps.tolist()
    assert sw[0] == sw[1] == sw[2] and sw[0] > 1 and bool(res.converged.all())
    assert torch.equal(res.U[0], res.U[1]) and torch.equal(res.U[2], res.U[1])
    assert torch.equal(res.V[0], res.V[1]) and torch.equal(res.V[2], res.V[1])
    assert torch.equal(res.S[0], res.S[1] * 2.0 ** -200)
    assert torch.equal(res.S[2], res.S[1] * 2.0 ** 200)
    assert torch.equal(res.off[0], res.off[1]) and torch.equal(res.off[2], res.off[1])


def test_per_matrix_stop(cuda):
    R = _rand(70, 65, dtype=F32, seed=31)
    Q = torch.linalg.qr(_rand(70, 65, dtype=F64, seed=32)).Q.float()
    batch = torch.stack([Q, R, torch.zeros(70, 65)]).to(cuda)
    res = svdj.svd_batched(batch, batched="block")
    sw = res.sweeps.tolist()
    assert sw[0] == 1 and sw[2] == 1 and sw[1] > 1, sw
    assert bool(res.converged.all())
    assert bool((res.S[2] == 0).all())
    assert bool(torch.isfinite(res.U[2]).all()) and bool(torch.isfinite(res.V[2]).all())
    assert float((res.S[0] - 1).abs().max()) < 1e-5
    lim = svdj.svd_batched(batch, batched="block", max_sweeps=2)
    assert lim.sweeps.tolist() == [1, 2, 1]
    assert lim.converged.tolist() == [True, False, True]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
def test_batch_order_bitwise(cuda, dtype):
    A = _rand(3, 70, 65, dtype=dtype, seed=41).to(cuda)
    A[2] = torch.linalg.qr(A[2].double()).Q.to(dtype)  # stops early: the active set shrinks
    a = svdj.svd_batched(A, batched="block")
    perm = [2, 0, 1]
    b = svdj.svd_batched(A[perm].contiguous(), batched="block")
    assert len(set(a.sweeps.tolist())) > 1
    for name in ("U", "S", "V", "sweeps", "off"):
        assert torch.equal(getattr(b, name), getattr(a, name)[perm]), name


def test_chunks(cuda):
    A = _rand(5, 70, 65, dtype=F32, seed=51)
    res = svdj.svd_batched(A.to(cuda), batched="block", extra={"batch_chunk": 2})
    assert res.info["chunks"] == 3 and res.info["pairs_per_step"] == 4
    assert bool((res.S > 0).all()) and bool((res.sweeps > 1).all())  # every output row filled
    assert bool((res.U.abs().amax((1, 2)) > 0).all()) and bool((res.V.abs().amax((1, 2)) > 0).all())
    _check("chunks_70x65", A, res)


def test_job_options_layout_sort_and_default_route(cuda):
    A = _rand(3, 70, 65, dtype=F32, seed=61)
    key = "jobs_70x65"
    full = svdj.svd_batched(A.to(cuda), batched="block")
    assert full.info["in_place"]
    _check(key, A, full)
    want = _oracle_metrics(key, A)
    sref = torch.linalg.svd(A.double(), full_matrices=False).S

    def sigma_err(S):
        s = torch.sort(S.cpu().double(), dim=-1, descending=True).values
        return float(((s - sref).abs().amax(1) / sref[:, 0]).max())

    nov = svdj.svd_batched(A.to(cuda), jobv=svdj.NoVec, batched="block")
    assert nov.V is None and nov.U is not None and sigma_err(nov.S) <= 4.0 * want["sigma"]
    nou = svdj.svd_batched(A.to(cuda), jobu=svdj.NoVec, batched="block")
    assert nou.U is None and nou.V is not None and sigma_err(nou.S) <= 4.0 * want["sigma"]
    assert torch.equal(nou.V, full.V)  # U is only scaled at the end
    # the transposed view of a contiguous (B, n, m) tensor is read in place: same numbers
    view = A.transpose(1, 2).contiguous().to(cuda).transpose(1, 2)
    assert not view.is_contiguous()
    res_t = svdj.svd_batched(view, batched="block")
    assert res_t.info["in_place"]
    for a, b in ((res_t.U, full.U), (res_t.S, full.S), (res_t.V, full.V)):
        assert torch.equal(a, b)
    srt = svdj.svd_batched(A.to(cuda), sort=True, batched="block")
    assert bool((srt.S[:, :-1] >= srt.S[:, 1:]).all())
    _check("jobs_sorted_70x65", A, srt)
    # without the new field the call goes where it went
    assert svdj.svd_batched(A.to(cuda)).info["engine"] == "loop"


@pytest.mark.parametrize("dtype,W,inner", [(F32, 32, "bipartite"), (F32, 64, "cross"),
                                           (F64, 32, "cyclic")],
                         ids=["fp32_w32_bip", "fp32_w64_cross", "fp64_w32_cyclic"])
def test_ungrouped_path_untouched(cuda, dtype, W, inner):
    """One K.block_steps call through the grouped entry with group_blocks = 0
    against the plain call on copies of the same buffers: bitwise A, V, D and
    metric (a full step and the cross steps of a round robin over 4 blocks)."""
    K = svdj.ops.kernels
    A = _rand(1, 300, 4 * W, dtype=dtype, seed=71).to(cuda)
    n_v = 4 * W  # 128 or 256 rows
    pairs = torch.from_numpy(stacked_pairs(4, [0])).to(cuda)
    modes = [K.STEP_FULL, K.STEP_CROSS, K.STEP_CROSS]
    mma = "bf16x6" if (dtype == F32 and W == 64) else "native"
    outs = []
    for gb in (None, 0):
        At, Vt, D, metric = K.stack_pack(A, 384, 4 * W, n_v, True)
        K.block_steps(At, Vt, D, 384, pairs, W, modes, 1e-6, 1, metric[0], mma=mma,
                      inner_order=inner, group_blocks=gb)
        outs.append((At, Vt, D, metric[0].clone()))
    assert int(outs[0][3][1]) > 0  # pairs rotated
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_plain_svd_of_a_scaled_fp64_matrix(cuda):
    """The fp64 EVDs' effective-sine statistic with squared norms outside
    float's range (eff_sine, block_evd.hpp), on the ungrouped path: 2^200 A
    and 2^-200 A run the sweeps A runs (before, the statistic of 2^200 A was
    NaN and dropped, and the second-order rule ended the solve after one
    sweep), with A's sigma up to the scale."""
    A = _rand(70, 65, dtype=F64, seed=21).to(cuda)
    base = svdj.svd(A, method="block")
    assert base.converged and base.sweeps > 2
    for e in (200, -200):
        r = svdj.svd(A * 2.0 ** e, method="block")
        assert r.converged and r.sweeps == base.sweeps, (e, r.sweeps, base.sweeps)
        assert torch.allclose(r.S * 2.0 ** -e, base.S, rtol=1e-12, atol=0)
