"""Measure svd_batched's "block" engine on one GPU.

For each case: a warm-up solve, then repeated timed whole solves
(svd_batched(A, batched="block"): pack, the host sweep loop with its metric
copies, finalize), wall clock around a synchronised call, median and spread.
Two yardsticks on the same GPU in the same process: the engine the same call
takes without the opt-in ("loop": svd() per matrix), timed on a few matrices
and scaled to the batch, and torch.linalg.svd on the batched tensor.

    python tools/bench_batched_block.py --out profiles/batched_block/bench.jsonl

Needs a GPU; there is no CPU fall-back.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import svdj  # noqa: E402

CASES = [  # (batch, m, n, dtype, block)
    (1024, 128, 128, torch.float32, None),
    (256, 256, 256, torch.float32, None),
    (64, 512, 512, torch.float32, None),
    (256, 2048, 128, torch.float32, None),
    (256, 128, 128, torch.float64, None),
    (256, 256, 256, torch.float32, 64),
]


def timed(fn, warmup, repeats):
    """Median and (min, max) wall seconds of one synchronised call of ``fn``."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append JSON lines here")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loop-matrices", type=int, default=4)
    ap.add_argument("--cases", default=None, help="comma-separated case numbers (default: all)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batched_block needs a GPU")
    dev = torch.device("cuda:0")
    pick = [int(x) for x in args.cases.split(",")] if args.cases else range(len(CASES))
    for ci in pick:
        B, m, n, dtype, block = CASES[ci]
        g = torch.Generator().manual_seed(B + m + n)
        A = torch.rand(B, m, n, dtype=dtype, generator=g).to(dev)
        kw = {"batched": "block", **({"block": block} if block else {})}
        res = svdj.svd_batched(A, **kw)
        assert res.info["engine"] == "block" and bool(res.converged.all())
        med, lo, hi = timed(lambda: svdj.svd_batched(A, **kw), args.warmup, args.repeats)
        tm, tlo, thi = timed(lambda: torch.linalg.svd(A, full_matrices=False), 1, 3)
        k = min(args.loop_matrices, B)
        loop = svdj.svd_batched(A[:k])  # warm-up, and the route without the opt-in
        assert loop.info["engine"] == "loop"
        lm, llo, lhi = timed(lambda: svdj.svd_batched(A[:k]), 0, 3)
        rec = {"batch": B, "m": m, "n": n, "dtype": str(dtype).replace("torch.", ""),
               "block": res.info["block"], "mma": res.info["mma"],
               "blocks_per_matrix": res.info["blocks_per_matrix"],
               "pairs_per_step": res.info["pairs_per_step"], "chunks": res.info["chunks"],
               "sweeps_min": int(res.sweeps.min()), "sweeps_max": int(res.sweeps.max()),
               "block_s": med, "block_s_min": lo, "block_s_max": hi, "matrices_per_s": B / med,
               "torch_linalg_svd_s": tm, "torch_linalg_svd_s_min": tlo,
               "torch_linalg_svd_s_max": thi, "speedup_vs_torch": tm / med,
               "loop_matrices": k, "loop_s_per_matrix": lm / k, "loop_s_per_matrix_min": llo / k,
               "loop_s_per_matrix_max": lhi / k, "loop_s_scaled": lm / k * B,
               "speedup_vs_loop": lm / k * B / med}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
