"""Cases, fp64 reference and checks of the tests of the EVD / Q-build chain
alone (tests/test_evd_ref_cpu.py, tests/test_gpu_evd.py).  Plain torch.

The chain of csrc/hip/block.hip between a step's Gram and its apply gets its
Gram as an input (kernels.evd_alone, kernels.quad_chain), so the kernels and
the reference (ops/reference.py jacobi_evd and the Gram-space algebra of
quad_step) start from bit-identical numbers: every Gram here is built in
fp64, rounded ONCE to the data type, and that value goes to both sides.

Every check is a function returning a measure.  A kernel passes a
rounding-level measure when it is at most RATIO_MAX x e_ref, e_ref the same
measure of the CPU reference run in the data precision on the same inputs.
"""
import functools
import math

import torch

import _apply_ref as A
import svdj

REF = svdj.ops.reference

RATIO_MAX = A.RATIO_MAX
FLOOR = 2.0 ** -20           # negligible-column floor of the cases (metric[2..3])
ORDER = {0: "ring", 1: "ring", 2: "bipartite", 3: "cross"}  # evd_kernel's own cyclic order
KINDS = ("single", "graded", "late", "mixed")


def tol_of(dtype):
    """sqrt(512) eps: the solver's default threshold at m = 512."""
    return math.sqrt(512.0) * torch.finfo(dtype).eps


def max_inner_of(kind):
    return {"single": 2, "graded": 1, "late": 3, "mixed": 2, "chunks": 1}[kind]


def ulps(x, ref64, dtype):
    """Largest distance of x from the fp64 values ref64 in units of the last
    place of ref64 rounded to dtype (0 where both are exactly equal)."""
    r = ref64.to(dtype).double()
    eps = torch.finfo(dtype).eps
    ulp = torch.where(r == 0, torch.full_like(r, torch.finfo(dtype).tiny),
                      2.0 ** torch.floor(torch.log2(r.abs().clamp(min=1e-300))) * eps)
    d = (x.double() - ref64).abs() / ulp
    return float(torch.where(x.double() == ref64, torch.zeros_like(d), d).max())


# ------------------------------------------------------------------ inputs
def graded_norms(n, seed, ratio=1.06):
    """n squared column norms ratio^k, k a random permutation of 0 .. n-1: no
    two closer than 5 %."""
    g = torch.Generator().manual_seed(seed)
    return ratio ** torch.randperm(n, generator=g).double()


def orth_blocks_gram(nblk, W, seed):
    """Gram X^T X (fp64) of nblk internally orthogonal W-column blocks in
    2 nblk W dimensions, squared column norms graded_norms: zero inside the
    blocks, dense relative couplings ~ 1 / sqrt(2 nblk W) between them."""
    g = torch.Generator().manual_seed(seed)
    n, m = nblk * W, 2 * nblk * W
    d = graded_norms(n, seed + 1)
    X = torch.empty(m, n, dtype=torch.float64)
    for b in range(nblk):
        q, _ = torch.linalg.qr(torch.randn(m, W, generator=g, dtype=torch.float64))
        X[:, b * W:(b + 1) * W] = q * d[b * W:(b + 1) * W].sqrt()
    G = X.t() @ X
    for b in range(nblk):
        blk = slice(b * W, (b + 1) * W)
        G[blk, blk] = torch.diag(d[blk])
    return G


def positions(W, count, seed):
    """(i, j) of the single couplings: the four corners, the two entries next
    to the centre, the main and the wrap-around diagonal, then random ones."""
    h = W // 2
    pos = [(0, 0), (0, W - 1), (W - 1, 0), (W - 1, W - 1), (h - 1, h), (h, h - 1),
           (1, 1), (h, h), (W - 2, W - 2), (1, 0), (h, h - 1), (0, W - 1), (h + 1, h), (W - 1, W - 2)]
    g = torch.Generator().manual_seed(seed)
    while len(pos) < count:
        pos.append((int(torch.randint(W, (1,), generator=g)), int(torch.randint(W, (1,), generator=g))))
    return pos[:count]


def pair_gram(C, Dp):
    """[[diag Dx, C], [C^T, diag Dy]] of every pair: C (P, W, W), Dp (P, 2W)."""
    P, W, _ = C.shape
    G = torch.diag_embed(Dp)
    G[:, :W, W:] = C
    G[:, W:, :W] = C.transpose(1, 2)
    return G


def block_perm(nblocks, seed):
    return torch.randperm(nblocks, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def single_case(kind, W, dtype, P=64, full_dense=False):
    """A single-step case of P pairs (pair p = blocks perm[2p], perm[2p+1]):
    'C' (P, W, W) and 'Dp' (P, 2W) in dtype (the values both sides get), 'G'
    (P, 2W, 2W) = pair_gram (full_dense: 'graded' with couplings inside the
    blocks as well, for the full-Gram mode), 'D' (2 P W,) by block id,
    'pairs', 'tol', 'max_inner', 'pos' (single: the coupling's (i, j))."""
    seed = 1000 * W + 17 * KINDS.index(kind)
    tol, pos = tol_of(dtype), None
    g = torch.Generator().manual_seed(seed)
    if kind in ("graded", "late") or kind == "mixed":
        G = torch.stack([orth_blocks_gram(2, W, seed + 10 * p) for p in range(P)])
        Dp = torch.diagonal(G, dim1=1, dim2=2).clone()
        C = G[:, :W, W:].clone()
        nrm = Dp[:, :W, None].sqrt() * Dp[:, None, W:].sqrt()
        if kind == "late":
            C = 1e-3 * nrm * (2 * torch.rand(P, W, W, generator=g, dtype=torch.float64) - 1)
        if kind == "mixed":
            sgn = torch.where(torch.rand(P, W, W, generator=g) < 0.5, -1.0, 1.0).double()
            small = 0.5 * tol * nrm * sgn
            late = 1e-3 * nrm * (2 * torch.rand(P, W, W, generator=g, dtype=torch.float64) - 1)
            pos = positions(W, P, seed + 3)
            for p in range(P):
                if p % 3 == 2:    # a column at the floor, one below it: never rotated
                    Dp[p, p % W] = FLOOR
                    Dp[p, W + (3 * p) % W] = FLOOR / 2
                    nr = Dp[p, :W, None].sqrt() * Dp[p, None, W:].sqrt()
                    C[p] = late[p] / nrm[p] * nr
                else:
                    C[p] = small[p]
                    if p % 3 == 1:  # exactly one coupling above the threshold
                        i, j = pos[p]
                        C[p, i, j] = 2 * tol * nrm[p, i, j]
        if full_dense:
            assert kind == "graded"
            X = torch.randn(P, 4 * W, 2 * W, generator=g, dtype=torch.float64) * Dp.sqrt()[:, None, :] / math.sqrt(4 * W)
            Gd = X.transpose(1, 2) @ X
            C, Dp = Gd[:, :W, W:].clone(), torch.diagonal(Gd, dim1=1, dim2=2).clone()
    else:  # single
        Dp = torch.stack([graded_norms(2 * W, seed + p) for p in range(P)])
        C = torch.zeros(P, W, W, dtype=torch.float64)
        pos = positions(W, P, seed + 3)
        for p, (i, j) in enumerate(pos):
            C[p, i, j] = 0.3 * math.sqrt(float(Dp[p, i] * Dp[p, W + j])) * (-1) ** p
    C, Dp = C.to(dtype), Dp.to(dtype)
    G = pair_gram(C, Dp)
    if full_dense:
        tri = torch.triu(Gd, 1).to(dtype)
        G = tri + tri.transpose(1, 2) + torch.diag_embed(Dp)
    perm = block_perm(2 * P, seed + 5)
    pairs = perm.view(P, 2).to(torch.int32)
    D = torch.empty(2 * P * W, dtype=dtype)
    D.view(2 * P, W)[perm] = Dp.reshape(2 * P, W)
    return {"C": C, "Dp": Dp, "G": G, "D": D, "pairs": pairs, "tol": tol,
            "max_inner": max_inner_of(kind), "pos": pos, "W": W, "P": P, "kind": kind}


def split_chunks(C, nchunk, cancel, seed):
    """C (..., W, W) cut into nchunk slabs (..., nchunk, W, W) of C's type whose
    fp64 sum, rounded to that type, is returned with them (the Gram both sides
    get).  Every slab holds fp32 values, so the fp64 sum is exact in any order.
    cancel: alternating slabs of +-64 |C| that cancel, so a dropped or doubled
    chunk shows."""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for k in range(nchunk - 1):
        if cancel:
            big = 64.0 * C.double().abs() * (1 + 0.01 * (k // 2))
            parts.append(((-1) ** k * big).float().double())
        else:
            parts.append((C.double() * (torch.rand(C.shape, generator=g, dtype=torch.float64) - 0.3)
                          ).float().double())
    rest = C.double() - sum(parts) if parts else C.double()
    parts.append(rest.float().double())
    slabs = torch.stack(parts, -3)
    return slabs.to(C.dtype), slabs.sum(-3).to(C.dtype)


# ------------------------------------------------------- single-step reference
def run_single(G, tol, max_inner, mode, dtype):
    """ops.reference.jacobi_evd with the kernels' ordering of `mode` on
    G.to(dtype): lam, Q, rot (pair rotated), smax / ncols per pair (the
    statistics of modes 0 - 2 with evd_kernel's look-ahead step: it solves
    every step one step ahead and counts what it solved; the cross EVD of
    mode 3 counts what it applied)."""
    st = {}
    lam, Q, rot = REF.jacobi_evd(G.to(dtype), tol, max_inner, 0, ORDER[mode], FLOOR, st,
                                 lookahead=mode != 3)
    P = G.shape[0]
    return {"lam": lam, "Q": Q, "rot": rot,
            "smax": st.get("smax_each", torch.zeros(P)).double(),
            "ncols": st.get("ncols_each", torch.zeros(P, dtype=torch.long))}


def maxconv(G, mode):
    """metric[0]: the largest |g| / sqrt(g_rr g_cc) over the entries the EVD
    assembles (cross block; mode 1: all off-diagonal), columns above the floor."""
    G = G.double()
    W = G.shape[-1] // 2
    d = torch.diagonal(G, dim1=1, dim2=2)
    den = d[:, :, None].sqrt() * d[:, None, :].sqrt()
    ok = (den > 0) & (d[:, :, None] > FLOOR) & (d[:, None, :] > FLOOR)
    R = torch.where(ok, G.abs() / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
    m = torch.triu(torch.ones_like(R[0]), 1).bool()
    if mode != 1:
        m = torch.zeros_like(m)
        m[:W, W:] = True
    return float(R[:, m].max())


# ------------------------------------------------------------------ checks
def orth(Q):
    """max |Q^T Q - I|."""
    Q = Q.double()
    return float((Q.transpose(-1, -2) @ Q - torch.eye(Q.shape[-1], dtype=torch.float64)).abs().max())


def d_measure(lam, Q, G):
    """max |lam - diag(Q^T G Q)| / diag(|Q|^T |G| |Q|)."""
    Q, G = Q.double(), G.double()
    num = (lam.double() - torch.diagonal(Q.transpose(-1, -2) @ G @ Q, dim1=-2, dim2=-1)).abs()
    den = torch.diagonal(Q.abs().transpose(-1, -2) @ G.abs() @ Q.abs(), dim1=-2, dim2=-1)
    return float((num / den).max())


def off_norm(Q, G):
    """Full off-diagonal Frobenius norm of Q^T G Q per matrix, over ||G||_F."""
    Q, G = Q.double(), G.double()
    H = Q.transpose(-1, -2) @ G @ Q
    off = H - torch.diag_embed(torch.diagonal(H, dim1=-2, dim2=-1))
    return off.flatten(-2).norm(dim=-1) / G.flatten(-2).norm(dim=-1)


def off_measure(Q, G, Q_ref64):
    """max over the matrices |off(Q) - off(Q_ref64)|: every Jacobi rotation
    removes 2 g^2 from the squared off-diagonal norm, so a result that applied
    other rotations than the reference leaves another norm."""
    return float((off_norm(Q, G) - off_norm(Q_ref64, G)).abs().max())


def entry(X, X_ref64):
    return float((X.double() - X_ref64.double()).abs().max())


def ratio(tag, e_k, e_ref, floor=0.0):
    """kernel / e_ref, printed; `floor`: a measure below it passes whatever
    e_ref (both are exact zeros or evaluation noise there)."""
    r = e_k / e_ref if e_ref > 0 else (0.0 if e_k <= floor else float("inf"))
    print(f"EVD_RATIO {tag} {e_k:.3e} {e_ref:.3e} {r:.2f}")
    return r


# ------------------------------------------------------------ quad reference
QN, QW = 256, 64
IA, IB, IC, ID = (torch.arange(QW) + k * QW for k in range(4))
BLOCKS = {"ac": (IA, IC), "bd": (IB, ID), "ad": (IA, ID), "bc": (IB, IC), "ab": (IA, IB), "cd": (IC, ID)}


def quad_slabs(G):
    """G (nq, 256, 256) -> (6 nq, 64, 64) in gram_quad's order: the pairs'
    Grams C_ac, C_bd of every quad, then C_ad, C_bc, C_ab, C_cd of every quad."""
    def blk(name):
        x, y = BLOCKS[name]
        return G[:, x][:, :, y]
    first = torch.stack([blk("ac"), blk("bd")], 1).flatten(0, 1)
    rest = torch.stack([blk("ad"), blk("bc"), blk("ab"), blk("cd")], 1).flatten(0, 1)
    return torch.cat([first, rest], 0).contiguous()


def quad_gram(slabs, Dq):
    """Inverse of quad_slabs: the quad's 256 x 256 Gram, D on the diagonal,
    the six slabs off it, zero inside the blocks."""
    nq = Dq.shape[0]
    G = torch.diag_embed(Dq.clone())
    first, rest = slabs[:2 * nq].view(nq, 2, QW, QW), slabs[2 * nq:].view(nq, 4, QW, QW)
    for k, name in enumerate(("ac", "bd")):
        x, y = BLOCKS[name]
        G[:, x[:, None], y[None, :]] = first[:, k]
    for k, name in enumerate(("ad", "bc", "ab", "cd")):
        x, y = BLOCKS[name]
        G[:, x[:, None], y[None, :]] = rest[:, k]
    iu = torch.triu(torch.ones(QN, QN), 1).bool()
    U = torch.where(iu, G, torch.zeros_like(G))
    return U + U.transpose(1, 2) + torch.diag_embed(Dq)


def place(qx, x, y):
    """(n, 128, 128) pair transforms on the rows / columns (x; y) of a 256 x
    256 identity."""
    T = torch.eye(QN, dtype=qx.dtype).repeat(qx.shape[0], 1, 1)
    i = torch.cat([x, y])
    T[:, i[:, None], i[None, :]] = qx
    return T


def cross_evd(C, Dx, Dy, tol, max_inner, dtype):
    """evd_cross_kernel of the pairs (C, Dx, Dy) in precision dtype."""
    r = run_single(pair_gram(C.to(dtype), torch.cat([Dx, Dy], 1).to(dtype)), tol, max_inner, 3, dtype)
    eye = torch.eye(2 * QW, dtype=dtype).expand_as(r["Q"])
    r["Q"] = torch.where(r["rot"][:, None, None], r["Q"], eye)
    r["lam"] = torch.where(r["rot"][:, None], r["lam"], torch.cat([Dx, Dy], 1).to(dtype))
    return r


def update_products(T1p, M, swap=False, transpose=False, emulate=False):
    """upd (2 nq, 64, 64) = L^T M R of every quad (block_quad.hpp
    quad_update_kernel): T1p (2 nq, 128, 128) the pairs' (a,c), (b,d)
    transforms, M (nq, 128, 128) = [[C_ab, C_ad], [C_cb, C_cd]] (rows a; c,
    columns b; d); j = 0: Q_ac[:, :64]^T M Q_bd[:, 64:] = C(a', d'), j = 1:
    Q_bd[:, :64]^T M^T Q_ac[:, 64:] = C(b', c').  emulate: operands rounded to
    fp32, products as an f32 MFMA chain (A.matmul_kblocked, depth 2).  swap /
    transpose: the wrong variants of the CPU tests."""
    nq = M.shape[0]
    Qac, Qbd = T1p[0::2], T1p[1::2]
    out = []
    for q in range(nq):
        for j in range(2):
            L = (Qac if j == 0 else Qbd)[q][:, :QW]
            Rm = (Qbd if j == 0 else Qac)[q][:, QW:]
            Mx = M[q] if (j == 0) != swap else M[q].t()
            if emulate:
                Y = A.matmul_kblocked(Mx.float(), Rm.float(), 2)
                o = A.matmul_kblocked(L.float().t().contiguous(), Y, 2).double()
            else:
                o = L.double().t() @ Mx.double() @ Rm.double()
            out.append(o.t() if transpose else o)
    return torch.stack(out)


def update_bound(T1p, M):
    """|L|^T |M| |R|: the denominator of the upd measure."""
    return update_products(T1p.abs(), M.abs())


def quad_m(slabs, nq):
    """M of every quad from the summed slabs (6 nq, 64, 64)."""
    r = slabs[2 * nq:].view(nq, 4, QW, QW).double()
    top = torch.cat([r[:, 2], r[:, 0]], 2)                    # C_ab, C_ad
    bot = torch.cat([r[:, 1].transpose(1, 2), r[:, 3]], 2)    # C_cb, C_cd
    return torch.cat([top, bot], 1)


def run_quad(slabs, Dq, tol, max_inner, dtype, order21=False, swap=False, transpose=False):
    """The quad chain on the summed slabs (6 nq, 64, 64) and Dq (nq, 256), EVDs
    in precision dtype (fp32: the update emulated in fp32 as well).  Returns
    T1 (2 nq, 128, 128), upd, T (nq, 256, 256) fp64, D (nq, 256), rot1 / rot2
    (2 nq) and the stop-test statistics.  order21 / swap / transpose: wrong
    variants."""
    nq = Dq.shape[0]
    Dq = Dq.clone().to(dtype)
    e1 = cross_evd(slabs[:2 * nq], torch.stack([Dq[:, IA], Dq[:, IB]], 1).flatten(0, 1),
                   torch.stack([Dq[:, IC], Dq[:, ID]], 1).flatten(0, 1), tol, max_inner, dtype)
    lam = e1["lam"].view(nq, 2, 2, QW)
    Dq[:, IA], Dq[:, IC], Dq[:, IB], Dq[:, ID] = lam[:, 0, 0], lam[:, 0, 1], lam[:, 1, 0], lam[:, 1, 1]
    T1p, D1 = e1["Q"].double(), Dq.clone()
    upd = update_products(T1p, quad_m(slabs, nq), swap=swap, transpose=transpose,
                          emulate=dtype == torch.float32)
    e2 = cross_evd(upd.to(dtype), torch.stack([Dq[:, IA], Dq[:, IB]], 1).flatten(0, 1),
                   torch.stack([Dq[:, ID], Dq[:, IC]], 1).flatten(0, 1), tol, max_inner, dtype)
    lam = e2["lam"].view(nq, 2, 2, QW)
    Dq[:, IA], Dq[:, ID], Dq[:, IB], Dq[:, IC] = lam[:, 0, 0], lam[:, 0, 1], lam[:, 1, 0], lam[:, 1, 1]
    T2p = e2["Q"].double()
    T1 = place(T1p[0::2], IA, IC) @ place(T1p[1::2], IB, ID)
    T2 = place(T2p[0::2], IA, ID) @ place(T2p[1::2], IB, IC)
    T = T2 @ T1 if order21 else T1 @ T2
    return {"T1": T1p, "upd": upd, "T": T, "D": Dq, "D1": D1, "rot1": e1["rot"], "rot2": e2["rot"],
            "ncols": e1["ncols"].view(nq, 2).sum(1) + e2["ncols"].view(nq, 2).sum(1),
            "smax": torch.maximum(e1["smax"].view(nq, 2).amax(1), e2["smax"].view(nq, 2).amax(1))}


def upd_measure(upd, T1p, slabs, nq):
    """max |upd - L^T M R| / (|L|^T |M| |R|), the products in fp64 from the
    given T1 and slabs: quad_update_kernel alone."""
    M = quad_m(slabs, nq)
    ref, den = update_products(T1p, M), update_bound(T1p, M)
    ok = den > 0
    return float(((upd.double() - ref).abs()[ok] / den[ok]).max()) if bool(ok.any()) else 0.0


def quad_maxconv(slabs, Dq, upd, D1):
    """metric[0] of a quad chain: both EVDs' input couplings."""
    nq = Dq.shape[0]
    g1 = pair_gram(slabs[:2 * nq].double(),
                   torch.cat([torch.stack([Dq[:, IA], Dq[:, IB]], 1).flatten(0, 1),
                              torch.stack([Dq[:, IC], Dq[:, ID]], 1).flatten(0, 1)], 1).double())
    g2 = pair_gram(upd.double(),
                   torch.cat([torch.stack([D1[:, IA], D1[:, IB]], 1).flatten(0, 1),
                              torch.stack([D1[:, ID], D1[:, IC]], 1).flatten(0, 1)], 1).double())
    return max(maxconv(g1, 3), maxconv(g2, 3))


def ts_to_t(ts, nq, np_):
    """I + the sum of the np_ parts of a split T - I (kernels.quad_chain's
    'Ts'), fp64, and the parts."""
    parts = A.unpack_ts(ts, nq, np_)
    return torch.eye(QN, dtype=torch.float64) + sum(p.double() for p in parts), parts


QUAD_SINGLE = ("ac", "bd", "ad", "bc", "ab", "cd", "carry")


@functools.lru_cache(maxsize=None)
def quad_case(kind, nq=32):
    """A quad-chain case of nq quads (quad q = blocks blk[q] = (a, b, c, d)):
    'slabs' (6 nq, 64, 64) fp32 (one chunk), 'Dq' (nq, 256) fp32, 'D' by block
    id, 'pairs0' / 'pairs1', 'G' (nq, 256, 256) fp32-valued (quad_gram), and
    for 'single' the 'which' block of every quad's coupling."""
    seed = 7000 + 13 * KINDS.index(kind)
    g = torch.Generator().manual_seed(seed)
    tol, which = tol_of(torch.float32), None
    if kind == "single":
        Dq = torch.stack([graded_norms(QN, seed + q) for q in range(nq)])
        G = torch.diag_embed(Dq)
        pos = positions(QW, 2 * nq, seed + 3)
        which = [QUAD_SINGLE[q % 7] for q in range(nq)]
        for q in range(nq):
            i, j = pos[q]
            names = ["ac", "ab"] if which[q] == "carry" else [which[q]]
            for n, name in enumerate(names):
                x, y = BLOCKS[name]
                jj = pos[nq + q][1] if n else j
                G[q, x[i], y[jj]] = 0.3 * math.sqrt(float(Dq[q, x[i]] * Dq[q, y[jj]])) * (-1) ** q
    else:
        G = torch.stack([orth_blocks_gram(4, QW, seed + 10 * q) for q in range(nq)])
        Dq = torch.diagonal(G, dim1=1, dim2=2).clone()
        nrm = Dq[:, :, None].sqrt() * Dq[:, None, :].sqrt()
        if kind == "late":
            G = 1e-3 * nrm * (2 * torch.rand(nq, QN, QN, generator=g, dtype=torch.float64) - 1)
        if kind == "mixed":
            sgn = torch.where(torch.rand(nq, QN, QN, generator=g) < 0.5, -1.0, 1.0).double()
            late = 1e-3 * nrm * (2 * torch.rand(nq, QN, QN, generator=g, dtype=torch.float64) - 1)
            G = 0.5 * tol * nrm * sgn
            pos = positions(QW, nq, seed + 3)
            which = [QUAD_SINGLE[(q // 3) % 6] for q in range(nq)]
            for q in range(nq):
                if q % 3 == 1:
                    x, y = BLOCKS[which[q]]
                    i, j = pos[q]
                    G[q, x[i], y[j]] = 2 * tol * nrm[q, x[i], y[j]]
                elif q % 3 == 2:
                    Dq[q, q % QN] = FLOOR
                    Dq[q, (97 * q + 64) % QN] = FLOOR / 2
                    nr = Dq[q, :, None].sqrt() * Dq[q, None, :].sqrt()
                    G[q] = late[q] / nrm[q] * nr
    Dq = Dq.float()
    slabs = quad_slabs(G).float()
    blk, pairs0 = A.quad_blocks(nq, seed + 5)
    pairs1 = torch.stack([blk[:, [0, 3]], blk[:, [1, 2]]], 1).reshape(2 * nq, 2).to(torch.int32)
    D = torch.empty(4 * nq * QW)
    D.view(4 * nq, QW)[blk.flatten()] = Dq.reshape(4 * nq, QW)
    return {"slabs": slabs, "Dq": Dq, "D": D, "blk": blk, "pairs0": pairs0, "pairs1": pairs1,
            "G": quad_gram(slabs, Dq), "tol": tol, "max_inner": max_inner_of(kind), "which": which,
            "nq": nq, "kind": kind}


def quad_d_of(D, blk):
    """D by block id -> (nq, 256) in [a b c d] order."""
    return D.view(-1, QW)[blk.flatten()].reshape(blk.shape[0], QN)
