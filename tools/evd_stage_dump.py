"""Everything the EVD stage writes, on seeded inputs, saved for a bitwise
comparison of two builds of the kernel library (dev aid).

    SVDJ_HIP_LIB=<build A> python tools/evd_stage_dump.py dump DIR_A
    SVDJ_HIP_LIB=<build B> python tools/evd_stage_dump.py dump DIR_B
    python tools/evd_stage_dump.py cmp DIR_A DIR_B

One process per build (the library is chosen when it is first loaded).

dump: kernels.evd_alone for modes 0-3, fp32 / fp64, W = 32 / 64, nchunk 1, 5,
9 at P = 8 and 64 (every Q-build row count), and kernels.quad_chain for
nchunk 1, 5, 9 (both sides of the pre-sum from 5 chunks on), 2 and 3 split
parts, P = 4 and 64 (both Q-build forms).  Per case one .npz: D, Q and the
skip flags, or T1, upd, Ts and both skip flags, and the metric words.
cmp: every array of every case bitwise; metric words 0 and 4 are atomic maxima
and word 5 an integer sum, so they do not depend on the order of the
workgroups and are compared like the rest.  Exit status 1 on any difference.
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

M_ROWS = 320  # rows of the synthetic data behind the Grams


def _blocks(nb, W, seed):
    """nb blocks of W mutually orthogonal columns with graded norms (what a
    cross step assumes of a block), random against each other: (nb, m, W) fp64."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(nb, M_ROWS, W, generator=g, dtype=torch.float64)
    Qm, _ = torch.linalg.qr(X)
    scale = torch.logspace(0, -3, W, dtype=torch.float64)
    return Qm * scale


def _chunked(X, Y, nchunk):
    """X^T Y per row chunk: (nchunk, cols of X, cols of Y)."""
    return torch.stack([x.T @ y for x, y in zip(X.tensor_split(nchunk), Y.tensor_split(nchunk))])


def _metric(K, dev, dtype):
    m = K.new_metric(dev)
    K.set_norm_floor(m, dtype, M_ROWS, 1.0)
    return m


def dump_single(K, dev, out):
    for dtype in (torch.float32, torch.float64):
        for W in (32, 64):
            for P in (8, 64):
                B = _blocks(2 * P, W, 1000 + W + P)
                pairs = torch.arange(2 * P, dtype=torch.int32).view(P, 2)
                D0 = (B * B).sum(1).reshape(-1).to(dtype)
                for mode in (0, 1, 2, 3):
                    for nchunk in (1, 5, 9):
                        if mode == 1:
                            S = torch.stack([_chunked(torch.cat([B[2 * p], B[2 * p + 1]], 1),
                                                      torch.cat([B[2 * p], B[2 * p + 1]], 1), nchunk)
                                             for p in range(P)])
                        else:
                            S = torch.stack([_chunked(B[2 * p], B[2 * p + 1], nchunk) for p in range(P)])
                        D = D0.clone().to(dev)
                        m = _metric(K, dev, dtype)
                        tol = 8 * torch.finfo(dtype).eps
                        Q, skip = K.evd_alone(S.to(dtype).contiguous().to(dev), D, pairs, W, mode, tol, 4, m)
                        torch.cuda.synchronize()
                        name = f"single_{str(dtype)[6:]}_W{W}_P{P}_mode{mode}_c{nchunk}"
                        np.savez(out / name, D=D.cpu().numpy(), Q=Q.cpu().numpy(),
                                 skip=skip.cpu().numpy(), metric=m.cpu().numpy())
                        print(name, "rotated pairs", int((skip == 0).sum()), flush=True)


def dump_quad(K, dev, out):
    W = 64
    for P in (4, 64):
        nq = P // 2
        B = _blocks(4 * nq, W, 2000 + P)  # quad q: blocks a, b, c, d = 4q .. 4q + 3
        a, b, c, d = (torch.arange(nq, dtype=torch.int32) * 4 + i for i in range(4))
        pairs0 = torch.stack([torch.stack([a, c], 1), torch.stack([b, d], 1)], 1).view(P, 2)
        pairs1 = torch.stack([torch.stack([a, d], 1), torch.stack([b, c], 1)], 1).view(P, 2)
        D0 = (B * B).sum(1).reshape(-1).float()
        for nchunk in (1, 5, 9):
            # gram_quad's order: C_ac, C_bd per quad, then per quad C_ad, C_bc, C_ab, C_cd
            first = [_chunked(B[x], B[y], nchunk) for q in range(nq)
                     for x, y in ((4 * q, 4 * q + 2), (4 * q + 1, 4 * q + 3))]
            rest = [_chunked(B[x], B[y], nchunk) for q in range(nq)
                    for x, y in ((4 * q, 4 * q + 3), (4 * q + 1, 4 * q + 2), (4 * q, 4 * q + 1),
                                 (4 * q + 2, 4 * q + 3))]
            S = torch.stack(first + rest).float().contiguous().to(dev)
            for parts in (2, 3):
                D = D0.clone().to(dev)
                m = _metric(K, dev, torch.float32)
                o = K.quad_chain(S, D, pairs0, pairs1, 8 * torch.finfo(torch.float32).eps, 4, m, np=parts)
                torch.cuda.synchronize()
                name = f"quad_P{P}_c{nchunk}_np{parts}"
                np.savez(out / name, D=D.cpu().numpy(), T1=o["T1"].cpu().numpy(),
                         upd=o["upd"].cpu().numpy(), Ts=o["Ts"].view(torch.int16).cpu().numpy(),
                         skip1=o["skip1"].cpu().numpy(), skip2=o["skip2"].cpu().numpy(),
                         metric=m.cpu().numpy())
                print(name, "rotated pairs", int((o["skip1"] == 0).sum()), int((o["skip2"] == 0).sum()),
                      flush=True)


def compare(da, db):
    fa, fb = sorted(p.name for p in da.glob("*.npz")), sorted(p.name for p in db.glob("*.npz"))
    bad = 0 if fa == fb and fa else 1
    if bad:
        print("different or empty sets of cases:", len(fa), len(fb))
    arrays = 0
    for f in sorted(set(fa) & set(fb)):
        A, Bz = np.load(da / f), np.load(db / f)
        for k in A.files:
            arrays += 1
            if A[k].tobytes() != Bz[k].tobytes():
                bad += 1
                print("DIFFERS", f, k, int((A[k] != Bz[k]).sum()), "entries")
    print(f"{len(fa)} cases, {arrays} arrays,", "all bitwise equal" if not bad else f"{bad} differences")
    return bad


def main():
    if sys.argv[1] == "cmp":
        sys.exit(1 if compare(Path(sys.argv[2]), Path(sys.argv[3])) else 0)
    import svdj

    out = Path(sys.argv[2])
    out.mkdir(parents=True, exist_ok=True)
    dev = torch.device("cuda:0")
    K = svdj.ops.kernels
    print("library", svdj.ops.hip_lib()._name)
    dump_single(K, dev, out)
    dump_quad(K, dev, out)


if __name__ == "__main__":
    main()
