"""The chain between a step's Gram and its apply (csrc/hip/block.hip) alone,
from given Grams, against the fp64 reference of tests/_evd_ref.py:
evd_kernel (cyclic, full, bipartite), evd_cross_kernel + qbuild_kernel,
slab_reduce_kernel, quad_update_kernel and qbuild_quad_kernel, through
kernels.evd_alone and kernels.quad_chain, which run what a solve runs after
its Gram.

Bound: every rounding-level measure of the kernel is at most RATIO_MAX = 4 x
e_ref, the same measure of the CPU reference run in the data precision on the
same inputs; every test prints "EVD_RATIO <case> <kernel> <e_ref> <ratio>"
before it asserts.

fp64 data: a reference above fp64 does not exist here, so e_ref of the
measures taken against the fp64 reference (entry by entry, off-norm) is the
fp32 reference's on the same Gram rounded to fp32, times 2^-29 = eps64 /
eps32: to first order a rounding error is the unit roundoff times a factor
that depends on the input alone.  The invariants (orthogonality, D) are held
to the fp64 reference's own.

The one rotation of a 'single' case, against the fp64 value in ulps of the
output type: fp64 within the issue's 2.  fp32 needs more, by the code of
rotation_fast (raw v_rcp / v_sqrt, 1 ulp = 2u each, u = 2^-24; every other
operation 1u): tau = (gqq - gpp) rcp(2 g): 1 + 2 + 1 = 4u; fma(tau, tau, 1):
at most 8u + 1u; its sqrt: half of that + 2u = 6.5u; |tau| + sqrt: the mean
of 4u and 6.5u at most, + 1u = 6.25u; rcp: + 2u = 8.25u in t.  s = t c and c
follow in fp64 and are rounded once (1u), D' = d -+ t g adds 2u: 10u, at most
10 ulps (ULPS_F32).  Measured: 2.78 (fp64 data: 2.00; quad chain 1.55).  A
quad whose second rotation is fed by its first (the 'carry' quads) compounds
two solves and the update: 3 x that; measured 2.02.

metric[4] against the reference's smax: relative margin 2^-16, 2.5 x the
largest spread measured over the cases (fp32 single steps 6.2e-6, quad chain
2.8e-6, fp64 data 1.3e-7: the statistic is formed in fp32 with raw rcp and
sqrt from rotations that carry the data precision's rounding).

metric[5] (_count_ok): equal to the fp64 reference's count in 144 of 149
launches, off by 1 in the others, where the fp32 reference is off as well.

Measured kernel / e_ref ratios on an MI355X (smallest .. largest over the
cases of a group; all <= 4):
  fp32 single steps  cyclic / full: orth .. 0.37, D .. 0.54, off .. 0.99, Q entry by entry 0.31 .. 3.83
                     bipartite: orth .. 0.37, D .. 0.54, off .. 0.45, entry 0.68 .. 1.41
                     cross: orth .. 0.37, D .. 1.00, off .. 0.21, entry 0.49 .. 2.53
  fp64 single steps  orth 0.74 .. 1.13, D 0.78 .. 2.00, off .. 0.42, entry 0.10 .. 1.02
  quad chain         orth T1 .. 1.00, upd .. 2.28, orth T .. 1.00, D .. 1.00, off .. 0.07
                     graded, entry by entry: T1 0.68 .. 1.06, upd 0.35 .. 0.96, T 0.40 .. 2.86
The launches of different P (the Q builds' forms) gave bitwise the same Q,
T1 and T on the pairs they share in all 136 comparisons.

Which parametrisation reaches which branch (P = pairs of the launch):
  evd_kernel cyclic            test_single_step mode 0, every P
  evd_kernel cyclic, full Gram test_single_step mode 1 (2W x 2W slabs)
  evd_kernel bipartite         test_single_step mode 2
  evd_cross_kernel             test_single_step mode 3; test_quad_chain (EVD 1, EVD 2)
  qbuild_kernel 2 rows / lane  mode 3, W = 64, P = 8
  qbuild_kernel 4 rows / lane  mode 3, P = 16 (W = 32: P = 8 as well)
  qbuild_kernel 8 / 16 rows    mode 3, P = 64 (W = 32: 8, W = 64: 16)
  in-kernel fp64 chunk sum     test_chunks nchunk 3, 5 (and 9 but for mode 3 fp32 W = 64)
  slab_reduce, single step     test_chunks mode 3, fp32, W = 64, nchunk 9
  slab_reduce, quad (qgch > 4) test_quad_chunks nchunk 5, 9 (1, 3: summed in the kernels)
  qbuild_quad phase 1 / 2 lat  test_quad_chain P = 4, 32 (np 2 and 3)
  qbuild_quad phase 1 / 2 wide test_quad_chain P = 64 (np 2 and 3)
"""
import struct

import pytest
import torch

import _evd_ref as E

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SENTINEL = -7.25
SINGLE_P = (8, 16, 64)
QUAD_P = (4, 32, 64)
MX_ULPS = 4.0        # metric[0], fp32 ulps
SMAX_REL = 2.0 ** -16  # metric[4], see above
ULPS_F32, ULPS_F64 = 10.0, 2.0  # the one rotation of a 'single' case, see above
SCALE64 = 2.0 ** -29   # eps64 / eps32


def _metric(K, cuda):
    m = K.new_metric(cuda)
    m[2:4].view(torch.float64).fill_(E.FLOOR)
    return m


def _read_metric(m):
    h = m.cpu().tolist()
    f = lambda w: struct.unpack("<f", struct.pack("<i", w))[0]
    return {"mx": f(h[0]), "pairs": h[1] & 0xffffffff, "smax": f(h[4]), "ncols": h[5] & 0xffffffff}


def _count_ok(got, ref64, refd, what):
    """Counts of rotations against the fp64 reference's.  A decision can differ
    only where a coupling lies within the data precision's rounding of the
    threshold; the reference run in the data precision meets the same
    couplings, so its own departure from the fp64 count measures how many of
    them the case holds, and the kernel gets RATIO_MAX times that (exact for
    fp64 data and wherever the two reference counts agree)."""
    print(f"EVD_COUNT {what} kernel {got} ref64 {ref64} ref {refd}")
    assert abs(got - ref64) <= E.RATIO_MAX * abs(ref64 - refd), (what, got, ref64, refd)


@pytest.fixture(scope="module")
def single_refs():
    cache = {}

    def get(kind, W, dtype, mode, prec):
        key = (kind, W, dtype, 1 if (mode == 1 and kind == "graded") else E.ORDER[mode], prec)
        if key not in cache:
            c = E.single_case(kind, W, dtype, 64, full_dense=(mode == 1 and kind == "graded"))
            if prec == "f32 of f64":  # (fp64 run, fp32 run) on the Gram rounded to fp32
                g, t = c["G"].float(), E.tol_of(F32)
                cache[key] = (E.run_single(g.double(), t, c["max_inner"], mode, F64),
                              E.run_single(g, t, c["max_inner"], mode, F32))
            else:
                cache[key] = E.run_single(c["G"], c["tol"], c["max_inner"], mode, prec)
        return cache[key]
    return get


def _run_single(svdj, cuda, case, mode, P, slabs=None):
    K = svdj.ops.kernels
    W = case["W"]
    if slabs is None:
        slabs = (case["G"] if mode == 1 else case["C"])[:P, None]
    D = case["D"].clone().to(cuda)
    m = _metric(K, cuda)
    Q0 = torch.full((P, 2 * W, 2 * W), SENTINEL, dtype=slabs.dtype, device=cuda)
    Q, skip = K.evd_alone(slabs.contiguous().to(cuda), D, case["pairs"][:P], W, mode, case["tol"],
                          case["max_inner"], m, Q=Q0)
    torch.cuda.synchronize()
    return {"Q": Q.cpu(), "skip": skip.cpu(), "D": D.cpu(), "m": _read_metric(m)}


def _pair_d(D, pairs, W):
    return D.view(-1, W)[pairs.long()].reshape(pairs.shape[0], 2 * W)


def _check_single(tag, case, mode, P, out, r64, rd, dtype, scaled=None):
    W, G = case["W"], case["G"][:P]
    rot = r64["rot"][:P]
    assert torch.equal(out["skip"], (~rot).to(torch.int32)), tag
    assert out["m"]["pairs"] == int(rot.sum()), tag
    _count_ok(out["m"]["ncols"], int(r64["ncols"][:P].sum()), int(rd["ncols"][:P].sum()), tag)
    mx = E.maxconv(G, mode)
    print(f"EVD_MX {tag} {out['m']['mx']:.9e} {mx:.9e}")
    assert abs(out["m"]["mx"] - mx) <= MX_ULPS * 2.0 ** -23 * mx, tag
    if bool(rot.any()):
        sm = float(r64["smax"][:P].max())
        print(f"EVD_SMAX {tag} {out['m']['smax']:.9e} {sm:.9e} {out['m']['smax'] / sm - 1:.2e}")
        assert abs(out["m"]["smax"] - sm) <= SMAX_REL * sm, tag
    else:
        assert out["m"]["smax"] == 0.0 and out["m"]["ncols"] == 0, tag
    # D: untouched outside the launch's blocks and for skipped pairs (mode 1
    # re-measures it from the slab's diagonal: the same values here)
    Dp = _pair_d(out["D"], case["pairs"][:P], W)
    keep = torch.ones(case["D"].numel() // W, dtype=torch.bool)
    keep[case["pairs"][:P][rot].long().flatten()] = False
    assert torch.equal(out["D"].view(-1, W)[keep], case["D"].view(-1, W)[keep]), tag
    if not bool(rot.any()):
        return {}
    Q = out["Q"][rot]
    assert not bool(torch.isnan(Q).any()) and not bool((Q == SENTINEL).any()), tag
    res = {"orth": E.ratio(tag + " orth", E.orth(Q), E.orth(rd["Q"][:P][rot])),
           "D": E.ratio(tag + " D", E.d_measure(Dp[rot], Q, G[rot]),
                        E.d_measure(rd["lam"][:P][rot], rd["Q"][:P][rot], G[rot]))}
    q64 = r64["Q"][:P][rot]
    if dtype == F32:
        e_off, e_ent = E.off_measure(rd["Q"][:P][rot], G[rot], q64), E.entry(rd["Q"][:P][rot], q64)
    else:  # the fp32 reference's, scaled (see the module's text)
        a, b = scaled
        e_off = SCALE64 * E.off_measure(b["Q"][:P][rot], G[rot].float(), a["Q"][:P][rot])
        e_ent = SCALE64 * E.entry(b["Q"][:P][rot], a["Q"][:P][rot])
    # the rounding of c and s to the output type alone moves a rotated coupling by
    # |c s| (d_p + d_q) 2u <= 2u ||G||_F: below that the measure is not resolved
    res["off"] = E.ratio(tag + " off", E.off_measure(Q, G[rot], q64),
                         max(e_off, torch.finfo(dtype).eps))
    if case["kind"] == "graded":
        res["entry"] = E.ratio(tag + " entry", E.entry(Q, q64), e_ent)
    for k, v in res.items():
        assert v <= E.RATIO_MAX, (tag, k, v)
    if case["kind"] == "single":  # exactly one column rotation per pair, at its place
        q64 = r64["Q"][:P]
        assert torch.equal(out["Q"] != 0, q64 != 0), tag
        assert int((out["Q"] != 0).sum()) == P * (2 * W + 2), tag
        u = max(E.ulps(out["Q"], q64, dtype), E.ulps(Dp, r64["lam"][:P], dtype))
        print(f"EVD_ULPS {tag} {u:.2f}")
        assert u <= (ULPS_F32 if dtype == F32 else ULPS_F64), (tag, u)
    return res


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype,W", [(F32, 32), (F32, 64), (F64, 32), (F64, 64)])
def test_single_step(svdj, cuda, single_refs, dtype, W, mode, kind):
    """Everything after the Gram of a single step at P = 8, 16, 64 (the pair
    counts at which the Q build's form changes), the smaller launches on the
    first pairs of the largest: every check of _evd_ref, and the variants
    agree on the pairs they share."""
    case = E.single_case(kind, W, dtype, 64, full_dense=(mode == 1 and kind == "graded"))
    r64 = single_refs(kind, W, dtype, mode, F64)
    rd = single_refs(kind, W, dtype, mode, dtype)
    scaled = single_refs(kind, W, dtype, mode, "f32 of f64") if dtype == F64 else None
    outs = {}
    for P in SINGLE_P:
        tag = f"single/{str(dtype)[6:]}/W{W}/mode{mode}/{kind}/P{P}"
        outs[P] = _run_single(svdj, cuda, case, mode, P)
        _check_single(tag, case, mode, P, outs[P], r64, rd, dtype, scaled)
    for P in SINGLE_P[:-1]:
        rot = outs[P]["skip"] == 0
        assert torch.equal(outs[P]["skip"], outs[64]["skip"][:P])
        d = float((outs[P]["Q"][rot].double() - outs[64]["Q"][:P][rot].double()).abs().max()) if bool(rot.any()) else 0.0
        print(f"EVD_VARIANT single/{str(dtype)[6:]}/W{W}/mode{mode}/{kind} P{P} vs P64: max |dQ| {d:.3e}"
              f" bitwise {d == 0.0}")
        assert d <= 4 * torch.finfo(dtype).eps


@pytest.mark.parametrize("cancel", [False, True])
@pytest.mark.parametrize("nchunk", [1, 3, 5, 9])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype,W", [(F32, 32), (F32, 64), (F64, 32), (F64, 64)])
def test_chunks(svdj, cuda, dtype, W, mode, nchunk, cancel):
    """The graded Gram cut into nchunk slabs whose fp64 sum is exact: the
    chain on the slabs gives bitwise what it gives on their sum in one slab
    (the sum is formed in fp64 and rounded once on every path: in the EVD
    kernels, and by slab_reduce_kernel from 9 chunks on in mode 3, fp32, W =
    64).  A dropped, doubled or misplaced chunk changes the Gram (cancel: by
    64 times its size)."""
    P = 8
    base = E.single_case("graded", W, dtype, 64, full_dense=(mode == 1))
    src = (base["G"] if mode == 1 else base["C"])[:P]
    slabs, total = E.split_chunks(src, nchunk, cancel, 31 * nchunk + W)
    case = dict(base)
    a = _run_single(svdj, cuda, case, mode, P, slabs=slabs)
    b = _run_single(svdj, cuda, case, mode, P, slabs=total[:, None])
    assert torch.equal(a["skip"], b["skip"]) and int(a["skip"].sum()) == 0
    assert torch.equal(a["Q"], b["Q"]) and torch.equal(a["D"], b["D"]) and a["m"] == b["m"]
    assert not bool((a["Q"] == SENTINEL).any())


# ---------------------------------------------------------------- quad chain
@pytest.fixture(scope="module")
def quad_refs():
    cache = {}

    def get(kind, prec):
        if (kind, prec) not in cache:
            c = E.quad_case(kind)
            cache[kind, prec] = E.run_quad(c["slabs"], c["Dq"], c["tol"], c["max_inner"], prec)
        return cache[kind, prec]
    return get


def _quad_sel(case, P):
    nq = case["nq"]
    return torch.cat([case["slabs"][:P], case["slabs"][2 * nq:2 * nq + 2 * P]])


def _run_quad(svdj, cuda, case, P, np_, slabs=None):
    K = svdj.ops.kernels
    if slabs is None:
        slabs = _quad_sel(case, P)[:, None]
    D = case["D"].clone().to(cuda)
    m = _metric(K, cuda)
    o = K.quad_chain(slabs.contiguous().to(cuda), D, case["pairs0"][:P], case["pairs1"][:P],
                     case["tol"], case["max_inner"], m, np=np_)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in o.items()}
    out["D"], out["m"] = D.cpu(), _read_metric(m)
    return out


def _check_quad(tag, case, P, np_, out, r64, r32):
    nq = P // 2
    G, slabs = case["G"][:nq], _quad_sel(case, P)
    rot1, rot2 = r64["rot1"][:P], r64["rot2"][:P]
    assert torch.equal(out["skip1"], (~rot1).to(torch.int32)), tag
    assert torch.equal(out["skip2"], (~rot2).to(torch.int32)), tag
    assert out["m"]["pairs"] == int(rot1.sum() + rot2.sum()), tag
    _count_ok(out["m"]["ncols"], int(r64["ncols"][:nq].sum()), int(r32["ncols"][:nq].sum()), tag)
    mx = E.quad_maxconv(slabs, case["Dq"][:nq], out["upd"], r64["D1"][:nq])
    print(f"EVD_MX {tag} {out['m']['mx']:.9e} {mx:.9e}")
    assert abs(out["m"]["mx"] - mx) <= MX_ULPS * 2.0 ** -23 * mx, tag
    if bool(rot1.any() | rot2.any()):
        sm = float(r64["smax"][:nq].max())
        print(f"EVD_SMAX {tag} {out['m']['smax']:.9e} {sm:.9e} {out['m']['smax'] / sm - 1:.2e}")
        assert abs(out["m"]["smax"] - sm) <= SMAX_REL * sm, tag
    # T1: exactly the identity for a pair EVD 1 skipped
    eye = torch.eye(128, dtype=torch.float64)
    assert all(torch.equal(out["T1"][p], eye) for p in range(P) if not rot1[p]), tag
    Tk, parts = E.ts_to_t(out["Ts"], nq, np_)
    T64, T32 = r64["T"][:nq], r32["T"][:nq].float()
    # zero pattern: T touches only what the quad's four pair transforms touch
    assert not bool(((T64 - torch.eye(256, dtype=torch.float64)) == 0)[(Tk - torch.eye(256, dtype=torch.float64)) != 0].any()), tag
    # D: unchanged where neither EVD of the block's pairs rotated
    r1, r2 = rot1.view(nq, 2), rot2.view(nq, 2)
    touched = torch.stack([r1[:, 0] | r2[:, 0], r1[:, 1] | r2[:, 1], r1[:, 0] | r2[:, 1],
                           r1[:, 1] | r2[:, 0]], 1)  # a, b, c, d
    keep = torch.ones(case["D"].numel() // 64, dtype=torch.bool)
    keep[case["blk"][:nq][touched]] = False
    assert torch.equal(out["D"].view(-1, 64)[keep], case["D"].view(-1, 64)[keep]), tag
    Dk = E.quad_d_of(out["D"], case["blk"][:nq])
    # np 2: the two bf16 parts keep 16 mantissa bits of every entry of T - I, a
    # relative 2^-17 of entries <= 1 that the fp32 reference does not have
    split = 2.0 ** -17 if np_ == 2 else 0.0
    res = {"orthT1": E.ratio(tag + " orthT1", E.orth(out["T1"]), E.orth(r64["T1"][:P])),
           "upd": E.ratio(tag + " upd", E.upd_measure(out["upd"], out["T1"], slabs, nq),
                          E.upd_measure(r32["upd"][:P], r32["T1"][:P], slabs, nq)),
           "orthT": E.ratio(tag + " orthT", E.orth(Tk), E.orth(T32) + split),
           "D": E.ratio(tag + " D", E.d_measure(Dk, Tk, G), E.d_measure(r32["D"][:nq], T32, G) + split),
           "off": E.ratio(tag + " off", E.off_measure(Tk, G, T64),
                          max(E.off_measure(T32, G, T64), 2.0 ** -23) + split)}
    if case["kind"] == "graded":
        res["entryT1"] = E.ratio(tag + " entryT1", E.entry(out["T1"], r64["T1"][:P]),
                                 E.entry(r32["T1"][:P], r64["T1"][:P]))
        res["entryUpd"] = E.ratio(tag + " entryUpd", E.entry(out["upd"], r64["upd"][:P]),
                                  E.entry(r32["upd"][:P], r64["upd"][:P]))
        res["entryT"] = E.ratio(tag + " entryT", E.entry(Tk, T64), E.entry(T32, T64) + split)
    for k, v in res.items():
        assert v <= E.RATIO_MAX, (tag, k, v)
    if case["kind"] == "single" and np_ == 3:
        carry = torch.tensor([w == "carry" for w in case["which"][:nq]])
        for sel, bound, name in ((~carry, ULPS_F32, "one"), (carry, 3 * ULPS_F32, "carry")):
            if bool(sel.any()):
                u = max(E.ulps(Tk[sel], T64[sel], F32), E.ulps(Dk[sel], r64["D"][:nq][sel], F32))
                print(f"EVD_ULPS {tag} {name} {u:.2f}")
                assert u <= bound, (tag, name, u)
        for q in range(nq):  # C_ab / C_cd alone rotate nothing in either step
            if case["which"][q] in ("ab", "cd"):
                assert torch.equal(Tk[q], torch.eye(256, dtype=torch.float64)), (tag, q)
    return parts


@pytest.mark.parametrize("kind", E.KINDS)
def test_quad_chain(svdj, cuda, quad_refs, kind):
    """Everything between the Gram and the apply of a quad step at P = 4, 32
    (the two-rows-per-lane Q builds) and 64 (the wide ones), np 3 and 2."""
    case = E.quad_case(kind)
    r64, r32 = quad_refs(kind, F64), quad_refs(kind, F32)
    outs = {}
    for P in QUAD_P:
        o3 = _run_quad(svdj, cuda, case, P, 3)
        p3 = _check_quad(f"quad/{kind}/P{P}/np3", case, P, 3, o3, r64, r32)
        o2 = _run_quad(svdj, cuda, case, P, 2)
        p2 = _check_quad(f"quad/{kind}/P{P}/np2", case, P, 2, o2, r64, r32)
        # the 2-part Ts is the first two parts of the 3-part one, bitwise
        assert torch.equal(p2[0], p3[0]) and torch.equal(p2[1], p3[1])
        for k in ("T1", "upd", "skip1", "skip2", "D"):
            assert torch.equal(o2[k], o3[k]), k
        outs[P] = o3
    for P in QUAD_P[:-1]:
        for k in ("skip1", "skip2"):
            assert torch.equal(outs[P][k], outs[64][k][:P]), k
        d = float((outs[P]["T1"] - outs[64]["T1"][:P]).abs().max())
        nq = P // 2
        dt = float((E.ts_to_t(outs[P]["Ts"], nq, 3)[0] - E.ts_to_t(outs[64]["Ts"], 32, 3)[0][:nq]).abs().max())
        print(f"EVD_VARIANT quad/{kind} P{P} vs P64: max |dT1| {d:.3e} bitwise {d == 0.0},"
              f" max |dT| {dt:.3e} bitwise {dt == 0.0}")
        assert d <= 4 * 2.0 ** -52 and dt <= 4 * 2.0 ** -23


@pytest.mark.parametrize("cancel", [False, True])
@pytest.mark.parametrize("nchunk", [1, 3, 5, 9])
def test_quad_chunks(svdj, cuda, nchunk, cancel):
    """The graded quad Grams cut into nchunk slabs with an exact fp64 sum: the
    chain on the slabs (1, 3: summed by evd_cross_kernel and quad_update_kernel;
    5, 9: by slab_reduce_kernel first) gives bitwise what it gives on the sum."""
    case, P = E.quad_case("graded"), 4
    slabs, total = E.split_chunks(_quad_sel(case, P), nchunk, cancel, 77 * nchunk)
    a = _run_quad(svdj, cuda, case, P, 3, slabs=slabs)
    b = _run_quad(svdj, cuda, case, P, 3, slabs=total[:, None])
    for k in ("T1", "upd", "Ts", "skip1", "skip2", "D"):
        assert torch.equal(a[k], b[k]), k
    assert a["m"] == b["m"] and int(a["skip1"].sum()) == 0


def test_hooks_reject_bad_arguments(svdj, cuda):
    """-2 and no launch: null pointers, odd P, nchunk < 1, a short workspace."""
    import ctypes as C

    lib = svdj.ops.hip_lib()
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=cuda)
    p = C.c_void_p(buf.data_ptr())
    null = C.c_void_p(0)
    ev = lambda slabs=p, nchunk=1, P=2, ws=p, wsb=1 << 30, D=p: lib.svdj_evd_alone(
        0, 32, 3, slabs, nchunk, D, p, P, 1e-6, 0, 1, p, p, ws, wsb, p, null)
    assert ev(slabs=null) == -2 and ev(D=null) == -2 and ev(ws=null) == -2
    assert ev(nchunk=0) == -2 and ev(P=0) == -2 and ev(wsb=1024) == -2
    qc = lambda slabs=p, nchunk=1, P=2, wsb=1 << 30, np_=3, T1=p: lib.svdj_quad_chain(
        slabs, nchunk, p, p, P, 1e-6, 0, 1, np_, T1, p, p, p, p, p, wsb, p, null)
    assert qc(slabs=null) == -2 and qc(T1=null) == -2 and qc(P=3) == -2 and qc(P=0) == -2
    assert qc(nchunk=0) == -2 and qc(wsb=1024) == -2 and qc(np_=4) == -2
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0
