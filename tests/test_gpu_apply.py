"""The apply kernels of csrc/hip/block.hip alone, against fp64: apply_kernel
and apply_split_kernel through kernels.apply_q, apply_quad_ts_kernel through
kernels.apply_quad (cheap k halves, skipped quads, more than 64 quads, every
grid, V and leading dimensions).

Bound (tests/_apply_ref.py): max |Y - Y64| / (|X| @ |T - I| + |X|) of the
kernel at most 4 x that of the CPU emulation of the same arithmetic on the
same inputs (e_ref).  Every case prints "APPLY_RATIO <case> <kernel> <e_ref>
<ratio>" before it asserts.

Measured kernel / e_ref ratios on an MI355X (smallest .. largest of a group's
cases; all <= 4):
  apply_q fp32 W32 native 0.95 .. 1.16   bf16x6 0.60 .. 1.00   bf16x3 1.00 .. 1.01
  apply_q fp32 W64 native 0.87 .. 1.26   bf16x6 0.79 .. 1.24   bf16x3 1.00 .. 1.00
  apply_q fp64 W32 native 0.83 .. 1.48   W64 native 1.00 .. 1.15
  quad cheap mask 0: 2.10   1: 0.98   2: 1.52   3: 1.05   mixed: 1.00
  quad threshold 1.05, never cheap 2.06; mask 3 never cheap 2.06
    (cheap run - never-cheap run) / its bound: 0.233 on both inputs
  quad dense orthogonal np 3: 1.27 .. 2.01   np 2: 1.00 .. 1.01
  quad near-identity np 2: 1.00, sharper measure 1.00
  quad skips (each flag) 0.99 .. 1.82   grids 0.99 .. 1.79
  quad 70 quads 0.92 .. 2.22   4 of 70 active 1.00 .. 1.69
(1.00: a first-order half or the 2-part split sets the error, the same in
the kernel and the emulation; about 2: 3-part products everywhere, the
MFMA chain's accumulation against the emulation's exact k blocks.)
"""
import pytest
import torch

import _apply_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


def _check(tag, y_gpu, y_emu, y_ref, X, tm, own=1.0):
    e_ref = R.measure(y_emu, y_ref, X, tm, own=own)
    e_gpu = R.measure(y_gpu, y_ref, X, tm, own=own)
    print(f"APPLY_RATIO {tag} {e_gpu:.3e} {e_ref:.3e} {e_gpu / e_ref:.2f}")
    assert not bool(torch.isnan(y_gpu).any()), tag
    assert e_gpu <= R.RATIO_MAX * e_ref, (tag, e_gpu, e_ref, e_gpu / e_ref)
    return e_gpu / e_ref


# ------------------------------------------------------------------ apply_q
@pytest.fixture(scope="module")
def q_matrices():
    out = {}
    for W in (32, 64):
        out[W, "orth"] = R.random_orthogonal(2 * W, 100 + W)
        out[W, "near"] = R.near_identity(2 * W, 200 + W)
    return out


@pytest.mark.parametrize("kind", ["orth", "near"])
@pytest.mark.parametrize("rows", [128, 640])
@pytest.mark.parametrize("dtype,W,mma", [
    (torch.float32, 32, "native"), (torch.float32, 32, "bf16x6"), (torch.float32, 32, "bf16x3"),
    (torch.float32, 64, "native"), (torch.float32, 64, "bf16x6"), (torch.float32, 64, "bf16x3"),
    (torch.float64, 32, "native"), (torch.float64, 64, "native")])
def test_apply_q(svdj, cuda, q_matrices, dtype, W, mma, rows, kind):
    """X <- X Q for one block pair: a full 512-row chunk plus a short one
    (rows 640) and a single short chunk (128), ld = rows + 128 with the
    columns [rows, ld) of every row holding a sentinel."""
    K = svdj.ops.kernels
    ld = rows + 128
    g = torch.Generator().manual_seed(rows + W)
    x64 = (torch.rand(2 * W, rows, generator=g, dtype=torch.float64) - 0.3) * \
        torch.logspace(-2, 2, 2 * W, dtype=torch.float64)[:, None]
    Xt = torch.full((2 * W, ld), SENTINEL, dtype=dtype)
    Xt[:, :rows] = x64.to(dtype)
    Q = q_matrices[W, kind].to(dtype).contiguous()
    Xd = Xt.to(cuda)
    K.apply_q(Xd[:, :rows], Q.to(cuda), W, mma=mma)  # a view: leading dimension ld
    torch.cuda.synchronize()
    out = Xd.cpu()
    assert torch.equal(out[:, rows:], Xt[:, rows:]), "pad columns of the leading dimension written"
    X = Xt[:, :rows].t().contiguous()
    y_gpu = out[:, :rows].t().contiguous()
    tm = Q - torch.eye(2 * W, dtype=dtype)  # in the data type, as the kernels form it
    if dtype == torch.float64:
        y_ref, y_emu = R.product_longdouble(X, Q), R.emulate_plain(X, Q)
    else:
        y_ref = X.double() @ Q.double()
        y_emu = R.emulate_plain(X, Q) if mma == "native" else \
            R.emulate_split_apply(X, tm, 3 if mma == "bf16x6" else 2, kblock=16)
    _check(f"apply_q/{str(dtype)[6:]}/W{W}/{mma}/rows{rows}/{kind}", y_gpu, y_emu, y_ref, X, tm)


# --------------------------------------------------------------- quad apply
def _flags(nq, active, which=0):
    """skip1, skip2 (2 nq each): all set, but for an active quad flag `which`
    of its four (skip1[2q], skip1[2q+1], skip2[2q], skip2[2q+1])."""
    f = torch.ones(2, 2 * nq, dtype=torch.int32)
    for q in active:
        f[which // 2, 2 * q + which % 2] = 0
    return f[0].contiguous(), f[1].contiguous()


def _run_quad(svdj, cuda, case, np_=3, active=None, which=0, grid=256, cheap_log2=7, with_v=True,
              pad=0, nan_skipped=False):
    """Launch the quad apply on a case of _apply_ref.quad_case; returns A, V
    (CPU, with their pad columns) and the two work counters."""
    K = svdj.ops.kernels
    nq, m_pad = case["nq"], case["m_pad"]
    active = list(range(nq)) if active is None else list(active)
    n = case["At"].shape[0]
    At = torch.full((n, m_pad + pad), SENTINEL)
    At[:, :m_pad] = case["At"]
    Vt = torch.full((n, 128 + pad), SENTINEL)
    Vt[:, :128] = case["Vt"]
    tm = case["tm"].clone()
    ts = R.pack_ts(tm, np_)
    if nan_skipped:  # T of a skipped quad is never read
        per = R.QN * R.QN * np_
        for q in set(range(nq)) - set(active):
            ts[q * per:(q + 1) * per] = float("nan")
    s1, s2 = _flags(nq, active, which)
    Ad, Vd = At.to(cuda), Vt.to(cuda)
    work = torch.zeros(2, dtype=torch.int32, device=cuda)
    K.apply_quad(Ad, Vd[:, :128] if with_v else None, m_pad, case["pairs"].to(cuda), ts.to(cuda),
                 s1.to(cuda), s2.to(cuda), np=np_, grid=grid, cheap_log2=cheap_log2, work=work)
    torch.cuda.synchronize()
    return Ad.cpu(), Vd.cpu(), [int(w) for w in work.cpu()]


def _check_quads(tag, case, A, V, quads, np_=3, cheap_log2=7, own=1.0):
    """Accuracy of the given (active) quads' columns of A and V."""
    cols = R.quad_cols(case["blk"])
    m_pad = case["m_pad"]
    worst = 0.0
    for q in quads:
        X, tm = R.quad_rows(case, q), case["tm"][q]
        y_gpu = torch.cat([A[cols[q], :m_pad].t(), V[cols[q], :128].t()], 0)
        ch = R.cheap_mask(tm, cheap_log2) if np_ == 3 else None
        y_emu = R.emulate_split_apply(X, tm, np_, cheap_halves=ch)
        y_ref = X.double() + X.double() @ tm.double()
        worst = max(worst, _check(f"{tag}/q{q}", y_gpu, y_emu, y_ref, X, tm, own=own))
    return worst


def _untouched(case, A, V, quads, pad=0):
    cols = R.quad_cols(case["blk"])
    m_pad = case["m_pad"]
    for q in quads:
        assert torch.equal(A[cols[q], :m_pad], case["At"][cols[q]]), q
        assert torch.equal(V[cols[q], :128], case["Vt"][cols[q]]), q
    if pad:
        assert bool((A[:, m_pad:] == SENTINEL).all()) and bool((V[:, 128:] == SENTINEL).all())


def _tiles(case, nact, with_v=True):
    return nact * (case["m_pad"] + (128 if with_v else 0)) // 32


@pytest.mark.parametrize("name,units8", [(0, 32), (1, 24), (2, 24), (3, 16), ("mixed", 24)])
def test_quad_cheap_masks(svdj, cuda, name, units8):
    """Synthetic T whose k halves are ~0.1 or <= 2^-8: all eight waves take
    cheap mask 0, 1, 2 or 3, or (mixed: the late-sweep pattern) waves 0-3 mask
    1 and waves 4-7 mask 2.  The work counters prove the path: units / (8
    tiles) = 4, 3, 3, 2, 3."""
    case = R.quad_case(name)
    A, V, work = _run_quad(svdj, cuda, case)
    assert work[1] == _tiles(case, 1) and work[0] == units8 * work[1], work
    _check_quads(f"quad/mask-{name}", case, A, V, [0])


def test_quad_cheap_threshold_and_never_cheap(svdj, cuda):
    """A half whose largest part 0 is exactly 2^-7 is cheap, one with the next
    bf16 above it is not: seven waves at mask 3 and one at mask 1, 17 units
    per tile.  With cheap_log2 = 126 (never cheap) the same input takes 32
    units per tile and differs from the cheap run by the dropped order-2
    products, at most 4 x 2^-18 (|X| @ |T - I| over the cheap halves): parts
    1 and 2 are below 2^-9 and 2^-18 of a value, so x0 t2 + x1 t1 + x2 t0 <=
    3 x 2^-18 |x| |t|, and the fourth unit covers the roundings.  (Checked
    where the cheap halves are all of T, here and at mask 3: next to a half
    of ~0.1 the output's own rounding, 2^-24 |Y|, exceeds that bound.)"""
    for name, units in (("threshold", 17), (3, 16)):
        case = R.quad_case(name)
        A, V, work = _run_quad(svdj, cuda, case)
        assert work[1] == _tiles(case, 1) and work[0] == units * work[1], work
        _check_quads(f"quad/{name}", case, A, V, [0])
        A2, V2, work2 = _run_quad(svdj, cuda, case, cheap_log2=126)
        assert work2[1] == work[1] and work2[0] == 32 * work2[1], work2
        _check_quads(f"quad/{name}/never-cheap", case, A2, V2, [0], cheap_log2=126)
        X, tm = R.quad_rows(case, 0), case["tm"][0]
        ch = R.cheap_mask(tm).double().repeat_interleave(128, 0).repeat_interleave(32, 1)
        bound = 4 * 2.0 ** -18 * (X.double().abs() @ (tm.double().abs() * ch))
        cols = R.quad_cols(case["blk"])[0]
        d = torch.cat([(A - A2)[cols, :128].t(), (V - V2)[cols, :128].t()], 0).double().abs()
        print(f"APPLY_CHEAP_DIFF {name} max diff / bound {float((d / bound).max()):.3f}")
        assert bool((d <= bound).all())


@pytest.mark.parametrize("np_", [3, 2])
def test_quad_dense_orthogonal(svdj, cuda, np_):
    """T = T1 T2 of a real quad step (four random orthogonal 128 x 128 pair
    transforms), 2 quads, 256 + 128 rows, on 3 and on 2 parts."""
    case = R.quad_case("dense")
    A, V, work = _run_quad(svdj, cuda, case, np_=np_)
    assert work == [(32 if np_ == 3 else 16) * _tiles(case, 2), _tiles(case, 2)]
    _check_quads(f"quad/dense/np{np_}", case, A, V, [0, 1], np_=np_)


def test_quad_near_identity_two_parts(svdj, cuda):
    """Near-identity T on 2 parts, in the usual measure and in the sharper one
    (own = 2^-6) that tells the delta form from a split of T itself."""
    case = R.quad_case("tie2")
    A, V, _ = _run_quad(svdj, cuda, case, np_=2)
    _check_quads("quad/tie2/np2", case, A, V, [0], np_=2)
    _check_quads("quad/tie2/np2/sharp", case, A, V, [0], np_=2, own=2.0 ** -6)


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_quad_skips(svdj, cuda, which):
    """6 quads, active [0,1,0,1,1,0], an active quad having exactly one of its
    four flags clear: skipped quads stay bitwise unchanged, their Ts (NaN) is
    never read, the counters count active quads only."""
    case = R.quad_case("skips")
    active = [1, 3, 4]
    A, V, work = _run_quad(svdj, cuda, case, active=active, which=which, nan_skipped=True)
    assert not bool(torch.isnan(A).any()) and not bool(torch.isnan(V).any())
    _untouched(case, A, V, [0, 2, 5])
    assert work[1] == _tiles(case, 3), work
    _check_quads(f"quad/skips{which}", case, A, V, active)


def test_quad_all_skipped(svdj, cuda):
    case = R.quad_case("skips")
    A, V, work = _run_quad(svdj, cuda, case, active=[], nan_skipped=True)
    _untouched(case, A, V, range(6))
    assert work == [0, 0]


@pytest.mark.parametrize("active", [None, [3, 63, 64, 69]])
def test_quad_more_than_64_quads(svdj, cuda, active):
    """70 quads (280 blocks): the second trip of the ballot loops, all active
    and with actives on both sides of the 64-quad boundary."""
    case = R.quad_case("many")
    act = list(range(70)) if active is None else active
    A, V, work = _run_quad(svdj, cuda, case, active=active, nan_skipped=True)
    assert work[1] == _tiles(case, len(act)), work
    _untouched(case, A, V, sorted(set(range(70)) - set(act)))
    _check_quads("quad/many" + ("" if active is None else "-sparse"), case, A, V, act)


def test_quad_grids_bitwise(svdj, cuda):
    """3 active quads of 5 with 8 tiles each on 1 ... 1024 workgroups (1024:
    more than tiles; 5, 7: ranges that cross quads at odd offsets; 192, 224:
    the grids next to a second chain): a tile's arithmetic does not depend on
    the workgroup that runs it, so all results and counters are equal."""
    case = R.quad_case("grids")
    active = [0, 2, 3]
    ref = None
    for grid in (256, 1, 3, 5, 7, 192, 224, 1024):
        A, V, work = _run_quad(svdj, cuda, case, active=active, grid=grid, nan_skipped=True)
        if ref is None:
            ref = (A, V, work)
            assert work[1] == _tiles(case, 3)
            _untouched(case, A, V, [1, 4])
            _check_quads("quad/grids", case, A, V, active)
        else:
            assert torch.equal(A, ref[0]) and torch.equal(V, ref[1]) and work == ref[2], grid


def test_quad_without_v_and_padded_leading_dimensions(svdj, cuda):
    """V = None leaves A bitwise as with V (and V alone); lda = m_pad + 128,
    ldv = n_v + 128: the pad columns keep their sentinel."""
    case = R.quad_case("dense")
    A, V, work = _run_quad(svdj, cuda, case)
    A1, V1, work1 = _run_quad(svdj, cuda, case, with_v=False)
    assert torch.equal(A1, A) and torch.equal(V1[:, :128], case["Vt"])
    assert work1 == [32 * _tiles(case, 2, False), _tiles(case, 2, False)]
    A2, V2, work2 = _run_quad(svdj, cuda, case, pad=128)
    assert torch.equal(A2[:, :256], A) and torch.equal(V2[:, :128], V[:, :128]) and work2 == work
    assert bool((A2[:, 256:] == SENTINEL).all()) and bool((V2[:, 128:] == SENTINEL).all())


def test_quad_hook_rejects_bad_arguments(svdj, cuda):
    """np, grid, row counts and leading dimensions are validated before any
    launch: an error, and the data untouched."""
    K = svdj.ops.kernels
    case = R.quad_case(0)
    Ad, Vd = case["At"].to(cuda), case["Vt"].to(cuda)
    ts = R.pack_ts(case["tm"], 3).to(cuda)
    s1, s2 = (f.to(cuda) for f in _flags(1, [0]))
    pairs = case["pairs"].to(cuda)
    with pytest.raises(K.NativeError):
        K.apply_quad(Ad, Vd, 128, pairs, ts, s1, s2, np=3, grid=0)
    with pytest.raises(K.NativeError):
        K.apply_quad(Ad, Vd[:, :96], 128, pairs, ts, s1, s2)       # n_v not a multiple of 128
    with pytest.raises(ValueError):
        K.apply_quad(Ad, Vd, 128, pairs, ts, s1, s2, np=4)         # Ts holds 3 parts
    with pytest.raises(ValueError):
        K.apply_quad(Ad, Vd, 128, pairs + 4, ts, s1, s2)           # blocks outside the data
    torch.cuda.synchronize()
    assert torch.equal(Ad.cpu(), case["At"]) and torch.equal(Vd.cpu(), case["Vt"])
