"""The EVD-chain tests' CPU helper (tests/_evd_ref.py) checked on its own: the
fp64 reference passes every check on every case, and the checks have teeth --
each wrong variant of the chain exceeds the bound of the check meant for it
(RATIO_MAX x e_ref, e_ref from the reference run in fp32) at least TEETH
times over, or breaks an exact check.
"""
import pytest
import torch

import _apply_ref as A
import _evd_ref as E

F32, F64 = torch.float32, torch.float64
TEETH = 10.0
W, P = 32, 8   # small: the reference is the same code at every size


def _teeth(e_bad, e_ref):
    assert e_bad >= TEETH * E.RATIO_MAX * e_ref, (e_bad, e_ref)


@pytest.fixture(scope="module")
def graded():
    c = E.single_case("graded", W, F32, P)
    return c, E.run_single(c["G"], c["tol"], 1, 2, F64), E.run_single(c["G"], c["tol"], 1, 2, F32)


@pytest.fixture(scope="module")
def quad():
    c = E.quad_case("graded", 2)
    return c, E.run_quad(c["slabs"], c["Dq"], c["tol"], 1, F64), E.run_quad(c["slabs"], c["Dq"], c["tol"], 1, F32)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", E.KINDS)
def test_reference_passes_single_checks(kind, mode):
    c = E.single_case(kind, W, F32, P, full_dense=(mode == 1 and kind == "graded"))
    r = E.run_single(c["G"], c["tol"], c["max_inner"], mode, F64)
    r32 = E.run_single(c["G"], c["tol"], c["max_inner"], mode, F32)
    # every measure of the fp64 reference within the bound its fp32 run sets
    assert E.orth(r["Q"]) <= E.RATIO_MAX * E.orth(r32["Q"])
    assert E.d_measure(r["lam"], r["Q"], c["G"]) <= E.RATIO_MAX * E.d_measure(r32["lam"], r32["Q"], c["G"])
    assert torch.equal(r["rot"], r32["rot"])
    rot = r["rot"]
    want = {"single": P, "graded": P, "late": P, "mixed": sum(p % 3 != 0 for p in range(P))}[kind]
    assert int(rot.sum()) == want
    assert E.orth(r["Q"]) <= 1e-13
    if mode != 3 or kind != "graded":  # the cross EVD drops second-order terms of a dense Gram
        assert E.d_measure(r["lam"], r["Q"], c["G"]) <= 1e-7
    if kind == "single":
        assert int(r["ncols"].sum()) == P and int((r["Q"] != 0).sum()) == P * (2 * W + 2)
        for p, (i, j) in enumerate(c["pos"]):
            assert r["Q"][p, i, W + j] != 0 and r["Q"][p, W + j, i] == -r["Q"][p, i, W + j]
        assert float(E.off_norm(r["Q"], c["G"]).max()) <= 1e-15
    if kind == "mixed":  # one rotation exactly where one coupling is above the threshold
        assert all(int(r["ncols"][p]) == 1 for p in range(P) if p % 3 == 1)
        assert 0.9e-3 <= E.maxconv(c["G"], mode) <= 1e-3 * (1 + 1e-6)


@pytest.mark.parametrize("kind", E.KINDS)
def test_reference_passes_quad_checks(kind):
    c = E.quad_case(kind, 7)
    r = E.run_quad(c["slabs"], c["Dq"], c["tol"], c["max_inner"], F64)
    r32 = E.run_quad(c["slabs"], c["Dq"], c["tol"], c["max_inner"], F32)
    assert E.d_measure(r["D"], r["T"], c["G"]) <= E.RATIO_MAX * E.d_measure(r32["D"], r32["T"].float(), c["G"])
    assert torch.equal(r["rot1"], r32["rot1"]) and torch.equal(r["rot2"], r32["rot2"])
    assert E.orth(r["T"]) <= 1e-13 and E.orth(r["T1"]) <= 1e-13
    assert E.upd_measure(r["upd"], r["T1"], c["slabs"], 7) == 0.0
    assert torch.equal(E.quad_slabs(c["G"]), c["slabs"])
    if kind != "graded":
        assert E.d_measure(r["D"], r["T"], c["G"]) <= 1e-7
    if kind == "single":
        eye = torch.eye(256, dtype=F64)
        for q, w in enumerate(c["which"]):
            r1, r2 = bool(r["rot1"][2 * q:2 * q + 2].any()), bool(r["rot2"][2 * q:2 * q + 2].any())
            assert (r1, r2) == {"ac": (True, False), "bd": (True, False), "ad": (False, True),
                                "bc": (False, True), "ab": (False, False), "cd": (False, False),
                                "carry": (True, True)}[w], (q, w)
            if w in ("ab", "cd"):
                assert torch.equal(r["T"][q], eye) and torch.equal(r["D"][q], c["Dq"][q].double())
        assert float(E.off_norm(r["T"], c["G"])[[q for q, w in enumerate(c["which"]) if w not in ("ab", "cd", "carry")]].max()) <= 1e-15


def test_ring_pairs_cover_every_pair_once():
    """The reference's copy of evd_kernel's cyclic order: disjoint pairs per
    step, every pair once per sweep, slot 0 holds player N - 1."""
    for N in (8, 64, 128):
        steps = E.REF.ring_pairs(N)
        assert len(steps) == N - 1 and all(s[0][0] == N - 1 for s in steps)
        assert all(sorted(x for pr in s for x in pr) == list(range(N)) for s in steps)
        assert len({(min(a, b), max(a, b)) for s in steps for a, b in s}) == N * (N - 1) // 2
    assert E.REF.ring_pairs(8)[0] == [(7, 0), (1, 6), (2, 5), (3, 4)]  # first0 / second0 of block_evd.hpp


def test_split_chunks_sum_exactly():
    c = E.single_case("graded", W, F32, P)
    for dtype in (F32, F64):
        for n in (1, 3, 5, 9):
            for cancel in (False, True):
                slabs, total = E.split_chunks(c["C"].to(dtype), n, cancel, n)
                assert slabs.shape[1] == n
                fwd = sum(slabs[:, k].double() for k in range(n))
                rev = sum(slabs[:, k].double() for k in reversed(range(n)))
                assert torch.equal(fwd, rev) and torch.equal(fwd.to(dtype), total)
                if n > 1:  # a dropped chunk shows
                    assert not torch.equal((fwd - slabs[:, 1].double()).to(dtype), total)


def test_wrong_single_variants(graded):
    c, r64, r32 = graded
    G, Q = c["G"], r64["Q"]
    e_orth, e_d = E.orth(r32["Q"]), E.d_measure(r32["lam"], r32["Q"], G)
    e_off, e_ent = E.off_measure(r32["Q"], G, Q), E.entry(r32["Q"], Q)
    # the y ring off by one position: the y columns of Q rotated by one
    ring = torch.cat([Q[:, :, :W], torch.roll(Q[:, :, W:], 1, 2)], 2)
    _teeth(E.entry(ring, Q), e_ent)
    _teeth(E.d_measure(r64["lam"], ring, G), e_d)
    # two columns swapped
    sw = Q.clone()
    sw[:, :, [3, W + 5]] = Q[:, :, [W + 5, 3]]
    _teeth(E.d_measure(r64["lam"], sw, G), e_d)
    # the sign of s flipped: Q^T
    _teeth(E.off_measure(Q.transpose(1, 2), G, Q), e_off)
    _teeth(E.entry(Q.transpose(1, 2), Q), e_ent)
    # D left stale
    _teeth(E.d_measure(c["Dp"], Q, G), e_d)
    # a rotation dropped (Q no longer orthogonal if only one column is rotated)
    bad = Q.clone()
    bad[:, :, 0] = 0
    bad[:, 0, 0] = 1
    _teeth(E.orth(bad), e_orth)


def test_wrong_quad_variants(quad):
    c, r64, r32 = quad
    nq, G = c["nq"], c["G"]
    run = lambda **kw: E.run_quad(kw.pop("slabs", c["slabs"]), c["Dq"], c["tol"], 1, F64, **kw)
    e_ent = E.entry(r32["T"].float(), r64["T"])
    e_off = E.off_measure(r32["T"].float(), G, r64["T"])
    e_upd = E.upd_measure(r32["upd"], r32["T1"], c["slabs"], nq)
    # T2 T1 in place of T1 T2
    bad = run(order21=True)
    _teeth(E.entry(bad["T"], r64["T"]), e_ent)
    _teeth(E.off_measure(bad["T"], G, r64["T"]), e_off)
    # C_ad and C_bc exchanged
    s = c["slabs"].clone()
    first = 2 * nq
    s[first + 0::4], s[first + 1::4] = c["slabs"][first + 1::4], c["slabs"][first + 0::4]
    bad = run(slabs=s)
    _teeth(E.upd_measure(bad["upd"], bad["T1"], c["slabs"], nq), e_upd)
    _teeth(E.entry(bad["T"], r64["T"]), e_ent)
    # the j = 1 transpose missing; upd transposed
    for kw in ({"swap": True}, {"transpose": True}):
        bad = run(**kw)
        _teeth(E.upd_measure(bad["upd"], bad["T1"], c["slabs"], nq), e_upd)
    # a chunk dropped
    slabs, total = E.split_chunks(c["slabs"], 3, False, 5)
    less = slabs[:, :2].double().sum(1).float()
    assert not torch.equal(less, total)
    good, bad = run(slabs=total), run(slabs=less)
    _teeth(E.entry(bad["T"], good["T"]), e_ent)
    _teeth(E.entry(bad["upd"], good["upd"]), E.entry(r32["upd"], r64["upd"]))
    # a Ts fragment shifted by one k block
    tm = A.tm_of(r64["T"])
    good = E.ts_to_t(A.pack_ts(tm, 3), nq, 3)[0]
    assert torch.equal(good, torch.eye(256, dtype=F64) + tm.double())
    shifted = E.ts_to_t(A.pack_ts(tm, 3, kb_shift=1), nq, 3)[0]
    _teeth(E.entry(shifted, r64["T"]), e_ent)
    _teeth(E.orth(shifted), E.orth(r32["T"].float()))
