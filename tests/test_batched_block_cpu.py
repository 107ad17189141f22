"""svd_batched's "block" engine without a GPU: the engine choice, the stacked
pair lists, the driver on CPU tensors through the emulation of
ops/reference.py, and the argument checks of the new C entry points, which
run before any HIP call.

Accuracy bounds are 4x the CPU oracle's own worst value over the same
matrices, the convention of tests/test_gpu_batched.py for a solver with a
different pair order.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import svdj
from svdj.models.batched import BatchedJacobi, stack_chunk, stacked_pairs

F32, F64 = torch.float32, torch.float64
METRICS = ("residual", "sigma", "orth_u", "orth_v")


def _rand(*shape, dtype=F64, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, dtype=dtype, generator=g)


def _metrics(A, U, S, V):
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


def _oracle_metrics(A):
    rs = [svdj.svd(A[i], method="oracle") for i in range(A.shape[0])]
    assert all(r.converged for r in rs)
    return _metrics(A, torch.stack([r.U for r in rs]), torch.stack([r.S for r in rs]),
                    torch.stack([r.V for r in rs]))


# ------------------------------------------------------------- engine choice
def _pick(device="cuda", dtype=F32, m=70, n=65, want_v=True, **cfg):
    return BatchedJacobi(svdj.SolverConfig(**cfg)).pick_engine(device, dtype, m, n, want_v)


def test_pick_engine_table():
    # every choice without the new field is what it was
    assert _pick(m=37, n=33) == "kernel"
    assert _pick(m=70, n=65) == "loop"
    assert _pick(m=2000, n=64) == "loop"
    assert _pick(m=2000, n=64, precondition="qr") == "qr_kernel"
    assert _pick(m=64, n=64, precondition="qr") == "kernel"
    assert _pick(device="cpu", m=8, n=8) == "loop"
    assert _pick(m=8, n=8, method="scalar") == "loop"
    assert _pick(m=8, n=8, batched="auto") == "kernel"
    # "block" only when asked for, on either device, for any n >= 1
    for dev, (m, n) in itertools.product(("cuda", "cpu"), ((1, 1), (8, 8), (70, 65), (2000, 64),
                                                           (512, 512))):
        assert _pick(device=dev, m=m, n=n, batched="block") == "block"
        assert _pick(device=dev, m=m, n=n) != "block"
    assert _pick(m=2000, n=64, precondition="qr", batched="block") == "block"
    # a named single-matrix solver still means the loop
    assert _pick(m=8, n=8, method="scalar", batched="block") == "loop"
    assert _pick(m=8, n=0, batched="block") == "loop"
    with pytest.raises(ValueError, match="batched"):
        svdj.SolverConfig(batched="stacked")
    with pytest.raises(ValueError, match="batched"):
        svdj.svd_batched(_rand(2, 4, 3), batched="kernel")


# ---------------------------------------------------------------- pair lists
@pytest.mark.parametrize("k", [2, 4, 6, 10])
def test_stacked_pairs_cover_every_matrix_once(k):
    active = [0, 1, 2, 3, 4]
    p = stacked_pairs(k, active)
    assert p.dtype == np.int32 and p.shape == (k - 1, len(active) * k // 2, 2)
    assert p.flags["C_CONTIGUOUS"]
    assert (p[..., 0] // k == p[..., 1] // k).all()  # no pair crosses a matrix
    seen = sorted((int(a), int(b)) for a, b in p.reshape(-1, 2))
    want = sorted((g * k + a, g * k + b) for g in active
                  for a, b in itertools.combinations(range(k), 2))
    assert [tuple(sorted(x)) for x in seen] == want  # every block pair exactly once per sweep
    for s in range(k - 1):  # a step's pairs are disjoint
        assert len(set(p[s].reshape(-1).tolist())) == p[s].size


def test_stacked_pairs_compacted_to_active():
    k = 4
    p = stacked_pairs(k, [1, 4])  # matrices 0, 2, 3 have finished
    assert p.shape == (3, 4, 2)
    assert sorted(set((p // k).reshape(-1).tolist())) == [1, 4]
    assert stacked_pairs(k, []).shape == (3, 0, 2)


def test_stack_chunk_respects_cap_and_index_range():
    from svdj.models.batched import STACK_BYTE_CAP, STACK_MAX_MATRICES

    assert stack_chunk(10, 4, 128, lambda c: c * 1000) == 10
    per = STACK_BYTE_CAP // 7
    assert stack_chunk(100, 4, 128, lambda c: c * per) == 7
    assert stack_chunk(100, 4, 128, lambda c: c * 2 * STACK_BYTE_CAP) == 1  # never zero
    assert stack_chunk(10 ** 6, 2, 64, lambda c: 0) == STACK_MAX_MATRICES
    assert stack_chunk(10 ** 6, 2, 2 ** 20, lambda c: 0) == (2 ** 31 - 1) // 2 ** 20


# ------------------------------------------------- the engine on CPU tensors
@pytest.mark.parametrize("shape,dtype,seed", [((2, 70, 65), F64, 1), ((3, 40, 20), F32, 2)],
                         ids=["2x70x65_fp64", "3x40x20_fp32"])
def test_engine_on_cpu_against_oracle(shape, dtype, seed):
    A = _rand(*shape, dtype=dtype, seed=seed)
    res = svdj.svd_batched(A, batched="block")
    B, m, n = shape
    assert res.info["engine"] == "block" and res.info["block"] == 32
    k = max(-(-n // 64) * 2, 2)
    assert res.info["blocks_per_matrix"] == k and res.info["pairs_per_step"] == B * k // 2
    assert res.info["chunks"] == 1 and res.info["mma"] == "native"
    assert res.U.shape == (B, m, n) and res.S.shape == (B, n) and res.V.shape == (B, n, n)
    assert res.U.dtype == res.S.dtype == res.V.dtype == dtype
    assert res.sweeps.dtype == torch.int32 and res.off.dtype == torch.float32
    assert bool(res.converged.all()), res.sweeps
    assert all(1 < s < 60 for s in res.sweeps.tolist())
    assert all(0.0 <= o <= 1.0 for o in res.off.tolist())
    got, want = _metrics(A, res.U, res.S, res.V), _oracle_metrics(A)
    print(shape, dtype, "block", got, "oracle", want, "sweeps", res.sweeps.tolist())
    for name in METRICS:
        assert got[name] <= 4.0 * want[name], (name, got[name], want[name])
    # the default route is what it was
    assert svdj.svd_batched(A).info["engine"] == "loop"


def test_per_matrix_sweeps_and_off():
    """A matrix with orthogonal columns next to a random one: the first stops
    after its first sweep (nothing to rotate: off = 0 up to rounding), the
    second runs on alone, and each is solved as it is alone."""
    R = _rand(40, 20, seed=3)
    Q = torch.linalg.qr(_rand(40, 20, seed=4)).Q * torch.arange(1, 21, dtype=F64)
    res = svdj.svd_batched(torch.stack([Q, R]), batched="block")
    sw = res.sweeps.tolist()
    assert sw[0] == 1 and sw[1] > 1 and bool(res.converged.all())
    assert float(res.off[0]) <= res.info["tol"] and float(res.off[1]) <= 1e-6
    alone = svdj.svd_batched(R[None], batched="block")
    assert alone.sweeps.tolist() == [sw[1]]
    for a, b in ((alone.U[0], res.U[1]), (alone.S[0], res.S[1]), (alone.V[0], res.V[1])):
        assert torch.equal(a, b)
    assert torch.equal(alone.off[0], res.off[1])
    lim = svdj.svd_batched(torch.stack([Q, R]), batched="block", max_sweeps=2)
    assert lim.sweeps.tolist() == [1, 2] and lim.converged.tolist() == [True, False]


def test_per_matrix_floor_on_cpu():
    """Each matrix has the floor of its own scale: 2^-200 A next to A is
    solved as A is (a floor shared over the batch would leave it unrotated)."""
    A = _rand(12, 6, seed=5)
    res = svdj.svd_batched(torch.stack([A * 2.0 ** -200, A, A * 2.0 ** 200]), batched="block")
    assert res.sweeps[0] == res.sweeps[1] == res.sweeps[2] and int(res.sweeps[0]) > 1
    assert torch.equal(res.U[0], res.U[1]) and torch.equal(res.U[2], res.U[1])
    assert torch.equal(res.V[0], res.V[1]) and torch.equal(res.V[2], res.V[1])
    assert torch.equal(res.S[0], res.S[1] * 2.0 ** -200)
    assert torch.equal(res.S[2], res.S[1] * 2.0 ** 200)


def test_other_inputs_on_cpu():
    A = _rand(5, 9, 6, seed=6)
    full = svdj.svd_batched(A, batched="block")
    # chunks
    ch = svdj.svd_batched(A, batched="block", extra={"batch_chunk": 2})
    assert ch.info["chunks"] == 3 and ch.info["pairs_per_step"] == 2
    for name in ("U", "S", "V", "sweeps", "off"):
        assert torch.equal(getattr(ch, name), getattr(full, name)), name
    # wide, NoVec, sort, bf16, leading dimensions, empty
    w = svdj.svd_batched(A.transpose(1, 2).contiguous(), batched="block")
    assert w.info["transposed"] and torch.equal(w.U, full.V) and torch.equal(w.V, full.U)
    nv = svdj.svd_batched(A, jobv=svdj.NoVec, batched="block")
    assert nv.V is None and torch.allclose(nv.S, full.S, rtol=1e-12, atol=0)
    nu = svdj.svd_batched(A, jobu=svdj.NoVec, batched="block")
    assert nu.U is None and nu.V is not None and torch.allclose(nu.S, full.S, rtol=1e-12, atol=0)
    srt = svdj.svd_batched(A, sort=True, batched="block")
    assert bool((srt.S[:, :-1] >= srt.S[:, 1:]).all())
    rec = (srt.U * srt.S.unsqueeze(-2)) @ srt.V.transpose(-1, -2)
    assert float((rec - A).abs().max()) < 1e-13
    bf = svdj.svd_batched(A.to(torch.bfloat16), batched="block")
    assert bf.U.dtype == torch.bfloat16 and bf.S.dtype == torch.float32
    lead = svdj.svd_batched(_rand(2, 3, 7, 4, seed=7), batched="block")
    assert lead.U.shape == (2, 3, 7, 4) and lead.sweeps.shape == (2, 3)
    e = svdj.svd_batched(torch.empty(0, 5, 3), batched="block")
    assert e.U.shape == (0, 5, 3) and e.sweeps.shape == (0,)
    e = svdj.svd_batched(torch.empty(2, 3, 0), batched="block")
    assert e.S.shape == (2, 0)
    z = svdj.svd_batched(torch.zeros(2, 5, 3), batched="block")
    assert z.sweeps.tolist() == [1, 1] and bool((z.S == 0).all())
    assert bool(torch.isfinite(z.U).all()) and bool(torch.isfinite(z.V).all())
    with pytest.raises(ValueError, match="batch_chunk"):
        svdj.svd_batched(A, batched="block", extra={"batch_chunk": -1})


def test_grouped_emulation_fills_group_rows():
    """K.block_steps with group_blocks on CPU tensors: a group's row gets its
    own pairs' values, rows of groups without pairs stay untouched, and the
    ungrouped call on one matrix gives that group's numbers."""
    K = svdj.ops.kernels
    A = _rand(3, 130, 64, seed=8)
    At, Vt, D, metric = K.stack_pack(A, 256, 64, 128, True)
    assert At.shape == (192, 256) and Vt.shape == (192, 128) and metric.shape == (3, 5)
    assert torch.equal(At[64:128, :130], A[1].t()) and not bool(At[:, 130:].any())
    assert torch.equal(Vt[64:128, :64], torch.eye(64, dtype=F64))
    assert [float(metric[b, 2]) for b in range(3)] == \
        [K.norm_floor(F64, 256, float(D[64 * b:64 * b + 64].max())) for b in range(3)]
    one = K.stack_pack(A[2:3], 256, 64, 128, True)
    pairs = torch.from_numpy(stacked_pairs(2, [0, 2]))
    K.block_steps(At, Vt, D, 256, pairs, 32, [K.STEP_FULL], 1e-14, 1, metric, group_blocks=2)
    K.block_steps(one[0], one[1], one[2], 256, torch.from_numpy(stacked_pairs(2, [0])), 32,
                  [K.STEP_FULL], 1e-14, 1, one[3][0])
    assert float(metric[0, 1]) == 1 and float(metric[1, 1]) == 0 and float(metric[1, 0]) == 0
    assert torch.equal(metric[2], one[3][0])
    assert torch.equal(At[128:], one[0]) and torch.equal(Vt[128:], one[1])
    assert torch.equal(At[64:128, :130], A[1].t())  # the finished group is not touched
    mx, ms, nrot, ncr = K.read_group_stops(metric)
    assert mx[2] == float(metric[2, 0]) and ncr[2] == float(metric[2, 4]) and nrot[1] == 0
    K.reset_group_metrics(metric, torch.tensor([2]))
    assert metric[2].tolist() == [0, 0, float(one[3][0, 2]), 0, 0] and float(metric[0, 1]) == 1
    with pytest.raises(ValueError, match="group_blocks"):
        K.block_steps(At, Vt, D, 256, pairs, 32, [K.STEP_FULL], 1e-14, 1, metric, group_blocks=-1)
    with pytest.raises(ValueError, match="group_blocks"):
        K.block_steps(At, Vt, D, 256, pairs.repeat(2, 1, 1), 32,
                      [K.STEP_QUAD, K.STEP_QUAD_SECOND], 1e-14, 1, metric, group_blocks=2)


# --------------------------------------------- C entry points, no device call
def _fake():
    buf = (C.c_double * 4)()
    return C.cast(buf, C.c_void_p), C.c_void_p(0)


def _pack(dtype=0, batch=2, m=70, n=65, m_pad=128, ncols=128, lda=128, V=1, n_v=128, ldv=128,
          A=1, At=1, D=1, metric=1):
    """svdj_stack_pack with fake non-NULL pointers: every case here returns
    before the first HIP call, so none is ever dereferenced."""
    lib = svdj.ops.hip_lib()
    p, null = _fake()
    rc = lib.svdj_stack_pack(dtype, batch, m, n, p if A else null, m * n, n, 1, m_pad, ncols,
                             p if At else null, lda, p if V else null, n_v, ldv,
                             p if D else null, p if metric else null, null)
    return rc, lib.svdj_hip_last_error().decode()


def _finalize(dtype=0, batch=2, m=70, n=65, m_pad=128, ncols=128, lda=128, V=1, n_v=128, ldv=128,
              At=1, S=1, Vout=1):
    lib = svdj.ops.hip_lib()
    p, null = _fake()
    rc = lib.svdj_stack_finalize(dtype, batch, m, n, m_pad, ncols, p if At else null, lda,
                                 p if V else null, n_v, ldv, p, p if S else null,
                                 p if Vout else null, 1, null)
    return rc, lib.svdj_hip_last_error().decode()


BAD_LAYOUT = [dict(dtype=2), dict(dtype=-1), dict(batch=-1), dict(m=0), dict(n=0), dict(m=60),
              dict(m_pad=64), dict(m_pad=200), dict(m_pad=256), dict(ncols=64), dict(ncols=96),
              dict(n_v=64), dict(n_v=192, ldv=192, ncols=256, lda=128), dict(ldv=64),
              dict(batch=65536), dict(batch=40000, ncols=65536, n_v=65536, ldv=65536)]


@pytest.mark.parametrize("bad", BAD_LAYOUT + [dict(A=0), dict(At=0), dict(D=0), dict(metric=0)],
                         ids=str)
def test_stack_pack_rejects_bad_arguments(bad):
    rc, msg = _pack(**bad)
    assert rc == -2 and msg.startswith("stack_pack:") and len(msg) > 14


@pytest.mark.parametrize("bad", BAD_LAYOUT + [dict(At=0), dict(S=0), dict(V=0)], ids=str)
def test_stack_finalize_rejects_bad_arguments(bad):
    rc, msg = _finalize(**bad)
    assert rc == -2 and msg.startswith("stack_finalize:") and len(msg) > 18


def test_stack_entry_points_empty_batch():
    assert _pack(batch=0)[0] == 0 and _pack(batch=0, A=0, At=0, D=0, metric=0)[0] == 0
    assert _finalize(batch=0)[0] == 0 and _finalize(batch=0, At=0, S=0)[0] == 0


def _steps_grouped(group_blocks, modes, W=64, dtype=0):
    lib = svdj.ops.hip_lib()
    p, null = _fake()
    md = (C.c_int32 * len(modes))(*modes)
    rc = lib.svdj_block_steps_grouped(dtype, W, 128, p, 128, p, 128, 128, p, p, 2, len(modes), md,
                                      1e-6, 0, 1, p, 1 << 40, p, group_blocks, 1, null)
    return rc, lib.svdj_hip_last_error().decode()


def test_block_steps_grouped_rejects_quad_modes_and_negative_groups():
    rc, msg = _steps_grouped(4, [4, 5])
    assert rc == -2 and "quad" in msg and "group" in msg
    rc, msg = _steps_grouped(4, [1, 4, 5])
    assert rc == -2 and "quad" in msg
    rc, msg = _steps_grouped(-1, [1, 0])
    assert rc == -2 and "group_blocks" in msg
