"""The apply tests' CPU helper (tests/_apply_ref.py) checked on its own: the
operand layout round-trips, the emulation is within its own bound, and the
bound has teeth -- every wrong variant of the emulation, run on the inputs of
tests/test_gpu_apply.py, exceeds RATIO_MAX x e_ref at least ten times over.
"""
import pytest
import torch

import _apply_ref as R

TEETH = 10.0


def _ref64(X, tm):
    return X.double() + X.double() @ tm.double()


def _case(name):
    c = R.quad_case(name)
    return R.quad_rows(c, 0), c["tm"][0]


def test_pack_ts_matches_the_documented_layout():
    """pack_ts against the layout sentence of svdj_hip.h, element by element,
    and unpack_ts as its inverse."""
    tm = R.quad_case("dense")["tm"]
    parts = R.split_bf16(tm, 3)
    ts = R.pack_ts(tm, 3)
    g = torch.Generator().manual_seed(0)
    for _ in range(200):
        q, kb, ct, cs, p, gg, i, e = (int(torch.randint(n, (1,), generator=g))
                                      for n in (2, 8, 8, 2, 3, 4, 16, 8))
        at = ((((((q * 8 + kb) * 8 + ct) * 2 + cs) * 3 + p) * 64) + 16 * gg + i) * 8 + e
        assert ts[at] == parts[p][q, 32 * kb + 8 * gg + e, 32 * ct + 16 * cs + i]
    assert all(torch.equal(a, b) for a, b in zip(R.unpack_ts(ts, 2, 3), parts))


def test_split_parts_sum_back():
    x = R.graded(64, 128, 1)
    p3, p2 = R.split_bf16(x, 3), R.split_bf16(x, 2)
    assert torch.equal(sum(p.double() for p in p3).float(), x)  # 3 x 8 bits hold an fp32
    err = (sum(p.double() for p in p2) - x.double()).abs() / x.double().abs()
    assert float(err.max()) <= 2.0 ** -17


@pytest.mark.parametrize("name", [0, 1, 2, 3, "mixed", "threshold"])
def test_cheap_mask_of_the_cases(name):
    m = R.cheap_mask(_case(name)[1]).int().tolist()
    if name == "threshold":
        want = [[1] * 8, [1] * 5 + [0] + [1] * 2]
    else:
        want = [[int(v == R.SMALL) for v in half] for half in R.MASK_MAGS[name]]
    assert m == want


@pytest.mark.parametrize("name,np_", [(0, 3), (3, 3), ("mixed", 3), ("dense", 3), ("dense", 2),
                                      ("tie2", 2)])
def test_emulation_within_its_bound(name, np_):
    """e_ref against what the arithmetic allows: 2^-24 (output rounding) + 9
    roundings of 2^-24 in the accumulators + the dropped products, 2^-26 (3
    parts), 3 x 2^-18 (cheap half) or 2^-17 (2 parts) of |X| @ |T - I|."""
    X, tm = _case(name)
    ch = R.cheap_mask(tm) if np_ == 3 else None
    e = R.measure(R.emulate_split_apply(X, tm, np_, cheap_halves=ch), _ref64(X, tm), X, tm)
    split = 2.0 ** -17 if np_ == 2 else 3 * 2.0 ** -18 if bool(ch.any()) else 2.0 ** -26
    assert e <= 10 * 2.0 ** -24 + split, e


def _teeth(e_bad, e_ref):
    assert e_bad >= TEETH * R.RATIO_MAX * e_ref, (e_bad, e_ref, e_bad / e_ref)


def test_wrong_variants_exceed_the_bound():
    X, tm = _case("dense")
    y64 = _ref64(X, tm)
    e_ref = R.measure(R.emulate_split_apply(X, tm, 3), y64, X, tm)
    # one order-1 product dropped
    for drop in ((0, 1), (1, 0)):
        _teeth(R.measure(R.emulate_split_apply(X, tm, 3, drop=drop), y64, X, tm), e_ref)
    # the cheap form on halves that are not small (|T - I| dense, column sums ~ 10)
    every = torch.ones(2, 8, dtype=torch.bool)
    _teeth(R.measure(R.emulate_split_apply(X, tm, 3, cheap_halves=every), y64, X, tm), e_ref)
    # fragment index kb off by one; the cs sub-tiles swapped
    for kw in ({"kb_shift": 1}, {"swap_cs": True}):
        bad = [p[0] for p in R.unpack_ts(R.pack_ts(tm[None], 3, **kw), 1, 3)]
        _teeth(R.measure(R.emulate_split_apply(X, tm, 3, tparts=bad), y64, X, tm), e_ref)


@pytest.mark.parametrize("name", [1, "mixed"])
def test_wrong_layout_caught_on_cheap_cases(name):
    X, tm = _case(name)
    ch = R.cheap_mask(tm)
    y64 = _ref64(X, tm)
    e_ref = R.measure(R.emulate_split_apply(X, tm, 3, cheap_halves=ch), y64, X, tm)
    for kw in ({"kb_shift": 1}, {"swap_cs": True}):
        bad = [p[0] for p in R.unpack_ts(R.pack_ts(tm[None], 3, **kw), 1, 3)]
        _teeth(R.measure(R.emulate_split_apply(X, tm, 3, cheap_halves=ch, tparts=bad), y64, X, tm),
               e_ref)


def test_identity_inside_the_split_is_caught():
    """The plain form Y = X T with T (identity included) split into parts, on
    a near-identity T.  With 3 parts it cannot be told from the delta form in
    an fp32 result (1 + t on 3 parts is off by 2^-27 at most, of the column's
    own |X|, below the output's rounding); with 2 parts it is off by 2^-17,
    which the measure with own = 2^-6 shows (the "tie2" case of the GPU
    tests is held to that measure as well)."""
    X, tm = _case("tie2")
    y64 = _ref64(X, tm)
    own = 2.0 ** -6
    e_ref = R.measure(R.emulate_split_apply(X, tm, 2), y64, X, tm, own=own)
    xs = [p.float() for p in R.split_bf16(X, 2)]
    ts = [p.float() for p in R.split_bf16(tm + torch.eye(R.QN), 2)]
    y = sum(R.matmul_kblocked(xs[j], ts[i], 32) for i in range(2) for j in range(2) if i + j < 2)
    _teeth(R.measure(y, y64, X, tm, own=own), e_ref)


def test_plain_emulation_and_extended_reference():
    """emulate_plain in fp32 and fp64 against the extended-precision product:
    within K roundings of the format."""
    X = R.graded(128, 128, 5).t().contiguous()
    Q = R.random_orthogonal(128, 6)
    tm = (Q - torch.eye(128, dtype=torch.float64))
    y80 = R.product_longdouble(X.double(), Q)
    assert R.measure(R.emulate_plain(X.double(), Q), y80, X, tm) <= 128 * 2.0 ** -53
    y64 = X.double() @ Q.float().double()
    assert R.measure(R.emulate_plain(X, Q.float()), y64, X, tm) <= 128 * 2.0 ** -24
