"""The tall batched engine without a GPU: the host side of
csrc/hip/batched_tall.hip (LDS layout, panel rule, argument validation), which
runs before any HIP call, and the engine choice of svd_batched."""
import ctypes as C

import pytest
import torch

import svdj

F32, F64 = torch.float32, torch.float64
CAP = 163840
K = svdj.ops.kernels


def _ld(rows):
    """Leading dimension of an LDS image: >= rows, = 8 (mod 32)."""
    ld = max(rows, 8)
    while ld % 32 != 8:
        ld += 1
    return ld


def _layout(esize, n, want_v, rows):
    """batched_tall_layout as documented: R image (n columns of ld(n)), V image
    likewise when wanted, two panel images (n columns of ld(rows): the panel,
    and the U panel of the last stage), tau, 1 / (alpha - beta) and beta for 64
    reflectors, 64 elements of sigma, 128 bytes of flags."""
    return ((1 + bool(want_v)) * n * _ld(n) + 2 * n * _ld(rows) + 4 * 64) * esize + 128


@pytest.mark.parametrize("dtype,n,want_v,rows", [
    (F32, 64, True, 72), (F32, 64, False, 232), (F64, 64, True, 72), (F64, 64, True, 8),
    (F32, 33, True, 40), (F32, 1, True, 8), (F64, 3, False, 1000), (F32, 16, True, 32)])
def test_layout_sizes(dtype, n, want_v, rows):
    esize = 8 if dtype == F64 else 4
    assert K.batched_tall_lds_bytes(dtype, n, want_v, rows) == _layout(esize, n, want_v, rows)


def test_layout_pinned_and_rejected():
    f = K.batched_tall_lds_bytes
    assert f(F32, 64, True, 72) == (2 * 64 * 72 + 2 * 64 * 72 + 256) * 4 + 128 == 74880
    assert f(F64, 64, True, 72) == 149632
    assert f(F64, 64, True, 104) == 0  # above the cap
    assert f(F32, 65, True, 8) == 0 and f(F32, 0, True, 8) == 0
    assert f(F32, 8, True, 12) == 0 and f(F32, 8, True, 0) == 0 and f(F32, 8, True, -8) == 0
    assert int(svdj.ops.hip_lib().svdj_batched_tall_lds_bytes(2, 8, 1, 8)) == 0


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("want_v", [True, False])
def test_auto_panel_rule(dtype, want_v):
    """A multiple of 8 whose layout fits in the CU's LDS; half of it (two
    workgroups per CU) where that still leaves 64 rows; the next multiple of
    8 does not fit in the budget taken."""
    esize = 8 if dtype == F64 else 4
    for n in (1, 2, 3, 16, 33, 63, 64):
        rows = K.batched_tall_panel_rows(dtype, n, want_v)
        assert rows >= 8 and rows % 8 == 0
        total = K.batched_tall_lds_bytes(dtype, n, want_v, rows)
        assert total == _layout(esize, n, want_v, rows) and 0 < total <= CAP
        budget = CAP // 2 if total <= CAP // 2 else CAP
        assert _layout(esize, n, want_v, rows + 8) > budget
        if budget == CAP:  # half the LDS would have left fewer than 64 rows
            assert _layout(esize, n, want_v, 64) > CAP // 2
        else:
            assert rows >= 64
    assert K.batched_tall_panel_rows(dtype, 65, want_v) == 0
    assert K.batched_tall_panel_rows(dtype, 0, want_v) == 0


def test_balanced_rows():
    """Equal panels: as many as the auto height needs, padded to 8 rows."""
    top = K.batched_tall_panel_rows(F32, 64, True)
    assert top == 72
    f = K.batched_tall_balanced_rows
    assert f(F32, 65, 64, True) == 72 and f(F32, 72, 64, True) == 72
    assert f(F32, 256, 64, True) == 64  # 4 panels of 64, not 72 + 72 + 72 + 40
    assert f(F32, 2000, 64, True) == 72  # 28 panels
    for m in (64, 73, 145, 553, 4096, 10000):
        rows = f(F32, m, 64, True)
        assert rows % 8 == 0 and rows <= top and -(-m // rows) == -(-m // top)


def _call(dtype=0, batch=2, m=80, n=8, A=1, S=1, U=1, tau=1, panel_rows=0, max_sweeps=60,
          sweeps=1, off=1):
    """svdj_batched_tall_svd with fake non-NULL pointers: every case here
    returns before the first HIP call, so none is ever dereferenced."""
    lib = svdj.ops.hip_lib()
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    null = C.c_void_p(0)
    rc = lib.svdj_batched_tall_svd(dtype, batch, m, n, p if A else null, m * n, n, 1,
                                   p if U else null, p if S else null, p, p if tau else null,
                                   panel_rows, 1e-6, 0, max_sweeps, p if sweeps else null,
                                   p if off else null, null)
    return rc, lib.svdj_hip_last_error().decode()


@pytest.mark.parametrize("bad", [dict(n=65, m=80), dict(m=4, n=8), dict(panel_rows=12),
                                 dict(panel_rows=-8), dict(dtype=1, n=64, panel_rows=104),
                                 dict(tau=0), dict(A=0), dict(S=0), dict(dtype=2),
                                 dict(max_sweeps=-1), dict(batch=-1), dict(n=0, m=0),
                                 dict(m=1 << 26, n=32)])
def test_entry_point_rejects_bad_arguments(bad):
    rc, msg = _call(**bad)
    assert rc == -2 and msg.startswith("batched_tall_svd:") and len(msg) > 19


def test_entry_point_empty_batch_and_no_u():
    assert _call(batch=0)[0] == 0
    assert _call(batch=0, A=0, S=0, U=0, tau=0, sweeps=0, off=0)[0] == 0


def test_pick_engine_never_qr_kernel_off_the_gpu():
    qr = svdj.models.BatchedJacobi(svdj.SolverConfig(precondition="qr"))
    for shape in ((100, 16), (2000, 64), (16, 16)):
        assert qr.pick_engine("cpu", F32, *shape, True) == "loop"
    named = svdj.models.BatchedJacobi(svdj.SolverConfig(precondition="qr", method="scalar"))
    assert named.pick_engine("cuda", F32, 2000, 64, True) == "loop"
    assert named.pick_engine("cpu", F32, 2000, 64, True) == "loop"
    # on a device: only tall inputs of at most 64 columns, and only when asked
    assert qr.pick_engine("cuda", F32, 2000, 64, True) == "qr_kernel"
    assert qr.pick_engine("cuda", F32, 2000, 65, True) == "loop"
    assert qr.pick_engine("cuda", F32, 64, 64, True) == "kernel"
    auto = svdj.models.BatchedJacobi(svdj.SolverConfig())
    assert auto.pick_engine("cuda", F32, 2000, 64, True) == "loop"
    assert auto.pick_engine("cuda", F32, 256, 64, True) == "kernel"


def test_cpu_input_still_runs_the_loop():
    g = torch.Generator().manual_seed(3)
    A = torch.rand(3, 40, 6, dtype=F64, generator=g)
    res = svdj.svd_batched(A, precondition="qr")
    assert res.info["engine"] == "loop" and bool(res.converged.all())
    assert "panels" not in res.info
    rec = (res.U * res.S.unsqueeze(-2)) @ res.V.transpose(-1, -2)
    assert float((rec - A).abs().max()) < 1e-13
