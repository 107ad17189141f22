"""The quad apply on transforms that leave columns and blocks unchanged
(csrc/hip/block_quad.hpp apply_quad_ts_kernel, SPARSE), through kernels.apply_quad:
columns whose column of T - I is zero are not stored, waves that change
nothing run no product, k blocks that are zero in a wave's slice are skipped,
and columns that neither change nor feed a product are not loaded.

Accuracy as in tests/test_gpu_apply.py: max |Y - Y64| / (|X| @ |T - I| + |X|)
at most RATIO_MAX x that of the CPU emulation of the same arithmetic on the
same input; every case prints "APPLY_RATIO <case> <kernel> <e_ref> <ratio>"
before it asserts.  On top of that every case checks what the apply must not
touch, bitwise, and the work counters: word 7 (second) the tiles of active
quads, word 6 (first) the executed products only, tiles x quarter units of
the item's eight waves / 4 rounded down per work item (_apply_sparse.
quarter_units; exact when an item's tile count is a multiple of 4).

Measured kernel / e_ref ratios on an MI355X over all 64 checks: 0.75 .. 2.29
(0.00 where T = I: both exact); all <= 4 (profiles/sparse_apply).

The flags of every launch only mark a quad active (one of its four clear, as
in test_gpu_apply.py): what is skipped inside a quad comes from T's values.
"""
import pytest
import torch

import _apply_ref as R
import _apply_sparse as S

gpu = pytest.mark.gpu
SENTINEL = -7.25
PAD = 128


def _bits(x):
    return x.contiguous().view(torch.int32)


def _run(svdj, cuda, case, np_=3, active=None, grid=1, nan_skipped=False, At=None, Vt=None):
    """Launch on the case (A and V padded by PAD sentinel columns; At / Vt
    replace the case's data); returns A, V (CPU, padded) and the counters."""
    K = svdj.ops.kernels
    nq, m_pad = case["nq"], case["m_pad"]
    active = list(range(nq)) if active is None else list(active)
    n = case["At"].shape[0]
    A0 = torch.full((n, m_pad + PAD), SENTINEL)
    A0[:, :m_pad] = case["At"] if At is None else At
    V0 = torch.full((n, 128 + PAD), SENTINEL)
    V0[:, :128] = case["Vt"] if Vt is None else Vt
    ts = R.pack_ts(case["tm"].clone(), np_)
    if nan_skipped:
        per = R.QN * R.QN * np_
        for q in set(range(nq)) - set(active):
            ts[q * per:(q + 1) * per] = float("nan")
    f = torch.ones(2, 2 * nq, dtype=torch.int32)
    for q in active:
        f[0, 2 * q] = 0
    Ad, Vd = A0.to(cuda), V0.to(cuda)
    work = torch.zeros(2, dtype=torch.int32, device=cuda)
    K.apply_quad(Ad, Vd[:, :128], m_pad, case["pairs"].to(cuda), ts.to(cuda), f[0].contiguous().to(cuda),
                 f[1].contiguous().to(cuda), np=np_, grid=grid, work=work)
    torch.cuda.synchronize()
    A, V = Ad.cpu(), Vd.cpu()
    assert bool((A[:, m_pad:] == SENTINEL).all()) and bool((V[:, 128:] == SENTINEL).all()), "pad columns"
    return A, V, [int(w) for w in work.cpu()]


def _quad_out(case, A, V, q):
    cols = R.quad_cols(case["blk"])[q]
    return torch.cat([A[cols, :case["m_pad"]].t(), V[cols, :128].t()], 0).contiguous()


def _check_quad(tag, case, A, V, q, np_=3, X=None, keep=None):
    """Accuracy of quad q (X: its input rows if not the case's; keep: bool
    (256,) columns to judge, the others' data being zeroed in X), and bitwise
    identity of every column T - I leaves unchanged."""
    X = R.quad_rows(case, q) if X is None else X
    tm = case["tm"][q]
    y_gpu = _quad_out(case, A, V, q)
    same = ~S.changed_columns(tm)
    assert torch.equal(_bits(y_gpu[:, same]), _bits(X[:, same])), (tag, "unchanged columns rewritten")
    if keep is not None:
        X = X.clone()
        X[:, ~keep] = 0.0
        y_gpu = y_gpu.clone()
        y_gpu[:, ~keep] = 0.0
    ch = R.cheap_mask(tm) if np_ == 3 else None
    y_emu = R.emulate_split_apply(X, tm, np_, cheap_halves=ch)
    y_ref = X.double() + X.double() @ tm.double()
    e_ref, e_gpu = R.measure(y_emu, y_ref, X, tm), R.measure(y_gpu, y_ref, X, tm)
    ratio = e_gpu / e_ref if e_ref > 0 else 0.0 if e_gpu == 0 else float("inf")  # T = I: both exact
    print(f"APPLY_RATIO {tag}/q{q} {e_gpu:.3e} {e_ref:.3e} {ratio:.2f}")
    assert not bool(torch.isnan(y_gpu).any()), tag
    assert e_gpu <= R.RATIO_MAX * e_ref, (tag, e_gpu, e_ref, e_gpu / e_ref)


def _tiles(case):
    return (case["m_pad"] + 128) // 32


def _units(case, quads, np_=3):
    """Word 6 at grid = 1: one work item per quad."""
    return sum(_tiles(case) * S.quarter_units(case["tm"][q], np_) >> 2 for q in quads)


def _subset_case(subset, seed=300):
    """Quad 0: the pairs of ``subset`` rotated; quad 1: the other pairs (for
    subset 15 none: T = I in an active quad)."""
    tms = [R.tm_of(S.subset_t(seed + 16 * s, s)) for s in (subset, subset ^ 15)]
    return S.make_case(tms, 128, seed + subset)


def _givens_case(nrot, seed=400):
    tms, touched = [], []
    for q in range(2):
        t, tc = S.givens_t(seed + 7 * q + nrot, nrot)
        tms.append(R.tm_of(t))
        touched.append(tc)
    case = S.make_case(tms, 128, seed + nrot)
    # an untouched column of quad 0 with -0.0 entries: kept, not rewritten as +0.0
    free = [c for c in range(R.QN) if c not in touched[0]]
    col = int(R.quad_cols(case["blk"])[0][free[len(free) // 2]])
    case["At"][col, ::3] = -0.0
    case["Vt"][col, 1::2] = -0.0
    case["touched"], case["planted"] = touched, free[len(free) // 2]
    return case


# ------------------------------------------------------------- CPU: the cases
def test_sparse_case_builders_cpu():
    """Every case claims what its fp64 reference does: exactly the claimed
    columns come out unchanged, no exact zero sits where a case says
    "nonzero", and the expected counter follows the claimed structure."""
    for s in S.SUBSETS:
        tm = R.tm_of(S.subset_t(300 + 16 * s, s))
        blocks = S.subset_changed_blocks(s)
        claim = torch.zeros(R.QN, dtype=torch.bool)
        for b in blocks:
            claim[64 * b:64 * b + 64] = True
        assert torch.equal(S.changed_columns(tm), claim) and torch.equal(S.source_columns(tm), claim), s
        inside = tm[claim][:, claim]
        # a rotated pair's block is dense; blocks only one T2 pair joins stay structurally zero
        assert bool((inside != 0).any(0).all()) and bool((inside != 0).any(1).all()), s
        X = R.graded(R.QN, 64, s).t().contiguous()
        y = X.double() + X.double() @ tm.double()
        assert torch.equal(y[:, ~claim], X.double()[:, ~claim]) and bool((y[:, claim] != X.double()[:, claim]).any(0).all())
        # all eight k blocks of a changed wave in a dense quad, none elsewhere
        if s == 15:
            assert S.quarter_units(tm, 3) == 8 * 8 * 2 and S.quarter_units(tm, 2) == 8 * 8
        if s in (1, 2, 4, 8):  # one pair: 4 waves x 4 nonzero k blocks, full halves
            assert S.quarter_units(tm, 3) == 4 * 4 * 2, s
    assert S.quarter_units(torch.zeros(R.QN, R.QN), 3) == 0
    for nrot in (5, 30):
        case = _givens_case(nrot)
        for q in range(2):
            tm = case["tm"][q]
            claim = torch.zeros(R.QN, dtype=torch.bool)
            claim[case["touched"][q]] = True
            assert torch.equal(S.changed_columns(tm), claim) and torch.equal(S.source_columns(tm), claim)
            assert 0 < int(claim.sum()) < R.QN
        assert not bool(S.changed_columns(case["tm"][0])[case["planted"]])
        col = R.quad_cols(case["blk"])[0][case["planted"]]
        assert bool(torch.signbit(case["At"][col]).any()) and bool(torch.signbit(case["Vt"][col]).any())
    cols = [5, 77, 200]
    tm = S.zero_columns_keep_rows(500, cols)
    assert not bool(S.changed_columns(tm)[cols].any()) and int(S.changed_columns(tm).sum()) == R.QN - 3
    assert bool(S.source_columns(tm).all())
    tm = S.zero_rows_keep_columns(501, cols)
    assert not bool(S.source_columns(tm)[cols].any()) and int(S.source_columns(tm).sum()) == R.QN - 3
    assert bool(S.changed_columns(tm).all())
    tm = S.steady_tm(510)
    chg = S.changed_columns(tm).view(8, 32)
    assert [int(c.sum()) for c in chg] == [32, 0, 16, 32, 0, 0, 1, 32] and bool(S.source_columns(tm).all())
    # waves 0, 3, 7 and 2, 6: 8 full k blocks each (T - I ~ 0.1: no cheap half)
    assert S.quarter_units(tm, 3) == 5 * 8 * 2


# ------------------------------------------------------------------ GPU cases
@gpu
@pytest.mark.parametrize("subset", S.SUBSETS)
def test_pair_subsets(svdj, cuda, subset):
    """1. Each non-empty subset of the four pairs rotated (quad 1: the
    complement): blocks no rotated pair contains are bitwise the input, the
    counters those of the subset."""
    case = _subset_case(subset)
    A, V, work = _run(svdj, cuda, case)
    assert work[1] == 2 * _tiles(case), work
    assert work[0] == _units(case, [0, 1]), (work, _units(case, [0, 1]))
    for q, s in ((0, subset), (1, subset ^ 15)):
        same = torch.ones(R.QN, dtype=torch.bool)
        for b in S.subset_changed_blocks(s):
            same[64 * b:64 * b + 64] = False
        assert torch.equal(_quad_out(case, A, V, q)[:, same], R.quad_rows(case, q)[:, same]), (subset, q)
        _check_quad(f"sparse/subset{subset}", case, A, V, q)


@gpu
@pytest.mark.parametrize("subset", [1, 2, 4, 8])
def test_poisoned_blocks(svdj, cuda, subset):
    """2. One pair rotated, the two blocks T neither changes nor reads filled
    with NaN: they stay bitwise, the pair's columns are finite and accurate
    (the dense form multiplies the NaNs by zero and spreads them)."""
    case = _subset_case(subset)
    At, Vt = case["At"].clone(), case["Vt"].clone()
    keep = torch.zeros(R.QN, dtype=torch.bool)
    for b in S.subset_changed_blocks(subset):
        keep[64 * b:64 * b + 64] = True
    cols = R.quad_cols(case["blk"])[0]
    At[cols[~keep]] = float("nan")
    Vt[cols[~keep]] = float("nan")
    A, V, work = _run(svdj, cuda, case, At=At, Vt=Vt)
    X = torch.cat([At[cols].t(), Vt[cols].t()], 0).contiguous()
    y = _quad_out(case, A, V, 0)
    assert torch.equal(_bits(y[:, ~keep]), _bits(X[:, ~keep]))
    assert bool(torch.isfinite(y[:, keep]).all())
    _check_quad(f"sparse/poison{subset}", case, A, V, 0, X=X, keep=keep)
    _check_quad(f"sparse/poison{subset}", case, A, V, 1)


@gpu
@pytest.mark.parametrize("nrot", [5, 30])
def test_sparse_rotations(svdj, cuda, nrot):
    """3. T = I times 5 / 30 plane rotations per pair: untouched columns are
    bitwise the input, a planted -0.0 included."""
    case = _givens_case(nrot)
    A, V, work = _run(svdj, cuda, case)
    assert work == [_units(case, [0, 1]), 2 * _tiles(case)], work
    for q in range(2):
        _check_quad(f"sparse/givens{nrot}", case, A, V, q)
    y, X = _quad_out(case, A, V, 0), R.quad_rows(case, 0)
    assert bool(torch.signbit(y[:, case["planted"]]).any())
    assert torch.equal(torch.signbit(y[:, case["planted"]]), torch.signbit(X[:, case["planted"]]))


@gpu
def test_changed_and_source_are_separate(svdj, cuda):
    """4. Non-orthogonal T: columns of T - I zero with nonzero rows (data
    unchanged, still feeding the others), and rows zero with nonzero columns."""
    cols = [5, 77, 200]
    case = S.make_case([S.zero_columns_keep_rows(500, cols), S.zero_rows_keep_columns(501, cols)], 128, 520)
    A, V, work = _run(svdj, cuda, case)
    assert work == [2 * _tiles(case) * 32, 2 * _tiles(case)], work
    for q in range(2):
        _check_quad("sparse/chg-src", case, A, V, q)
    y, X = _quad_out(case, A, V, 0), R.quad_rows(case, 0)
    assert torch.equal(_bits(y[:, cols]), _bits(X[:, cols]))


@gpu
def test_counted_waits_steady_state(svdj, cuda):
    """5. 20 consecutive tiles per item (m_pad = 512, one workgroup) with waves
    that load without storing, store 8 or 2 of 16 instructions, or all."""
    case = S.make_case([S.steady_tm(510), S.steady_tm(511)], 512, 530)
    A, V, work = _run(svdj, cuda, case)
    assert work == [_units(case, [0, 1]), 2 * _tiles(case)], work
    for q in range(2):
        _check_quad("sparse/steady", case, A, V, q)


def _mix_tms(nq, seed):
    kinds = [lambda s: R.tm_of(S.subset_t(s, 1)), lambda s: R.tm_of(S.givens_t(s, 30)[0]),
             lambda s: R.tm_of(S.subset_t(s, 15)), lambda s: R.tm_of(S.subset_t(s, 6)),
             lambda s: R.tm_of(S.givens_t(s, 5)[0]), lambda s: S.steady_tm(s),
             lambda s: S.zero_rows_keep_columns(s, [3, 130])]
    return [kinds[q % len(kinds)](seed + 11 * q) for q in range(nq)]


@gpu
def test_grids_bitwise_sparse(svdj, cuda):
    """6. Five quads of different cost on 1, 3, 192, 224, 256 workgroups: the
    deal by cost changes no result; word 6 loses less than a unit per item."""
    case = S.make_case(_mix_tms(5, 600), 128, 610)
    exact = sum(_tiles(case) * S.quarter_units(case["tm"][q], 3) for q in range(5)) / 4.0
    ref = None
    for grid in (1, 3, 192, 224, 256):
        A, V, work = _run(svdj, cuda, case, grid=grid)
        items = min(grid, 5 * _tiles(case)) + 5  # a range, or a part of one in each quad it spans
        print(f"APPLY_SPARSE_GRID {grid} work {work} exact {exact}")
        assert work[1] == 5 * _tiles(case)
        assert exact - items < work[0] <= exact, (grid, work, exact)
        if ref is None:
            ref = (A, V)
            for q in range(5):
                _check_quad("sparse/grids", case, A, V, q)
        else:
            assert torch.equal(_bits(A), _bits(ref[0])) and torch.equal(_bits(V), _bits(ref[1])), grid


@gpu
def test_more_than_64_quads_sparse(svdj, cuda):
    """7. 70 quads cycling through the patterns, 9 of them active, on both
    sides of the 64-quad boundary; the skipped ones (NaN in their Ts) untouched."""
    case = S.make_case(_mix_tms(70, 700), 128, 710)
    active = [0, 1, 9, 24, 33, 62, 63, 64, 69]
    A, V, work = _run(svdj, cuda, case, active=active, grid=256, nan_skipped=True)
    assert work[1] == len(active) * _tiles(case), work
    for q in set(range(70)) - set(active):
        assert torch.equal(_bits(_quad_out(case, A, V, q)), _bits(R.quad_rows(case, q))), q
    for q in active:
        _check_quad("sparse/many", case, A, V, q)


@gpu
def test_two_parts(svdj, cuda):
    """8. The 2-part kernel on a pair subset and on sparse rotations."""
    for tag, case in (("subset5", _subset_case(5)), ("givens30", _givens_case(30))):
        A, V, work = _run(svdj, cuda, case, np_=2)
        assert work == [_units(case, [0, 1], np_=2), 2 * _tiles(case)], (tag, work)
        for q in range(2):
            _check_quad(f"sparse/np2/{tag}", case, A, V, q, np_=2)
