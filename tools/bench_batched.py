"""Measure svd_batched (the LDS-resident batched kernel) on one GPU.

For each case: warm-up, then repeated timed calls of the kernel entry point
(device events around a launch batch), median and spread; matrices per second
and effective GB/s counting A read and U, S, V written.  Two yardsticks on the
same GPU in the same process: torch.linalg.svd on the batched tensor, and the
only route without the batched path, a Python loop of svd(A[i],
method="scalar"), timed on 64 matrices and scaled to the batch.

    python tools/bench_batched.py --out profiles/batched/bench.jsonl

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

CASES = [  # (batch, m, n, dtype)
    (16384, 16, 16, torch.float32),
    (16384, 32, 32, torch.float32),
    (4096, 64, 64, torch.float32),
    (1024, 256, 64, torch.float32),
    (4096, 32, 32, torch.float64),
    (1024, 64, 64, torch.float64),
]


def timed(fn, warmup, repeats, inner):
    """Median and (min, max) seconds of one call of ``fn`` over ``repeats``
    windows of ``inner`` calls each, device events around every window."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3 / inner)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append JSON lines here")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-matrices", type=int, default=64)
    ap.add_argument("--skip-loop", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batched needs a GPU")
    dev = torch.device("cuda:0")
    K = svdj.ops.kernels
    for B, m, n, dtype in CASES:
        g = torch.Generator().manual_seed(B + m + n)
        A = torch.rand(B, m, n, dtype=dtype, generator=g).to(dev)
        esize = A.element_size()
        nbytes = B * esize * (2 * m * n + n + n * n)  # A read; U, S, V written
        tol = svdj.models.BatchedJacobi().tolerance(dtype, m)
        res = svdj.svd_batched(A)
        assert res.info["engine"] == "kernel" and bool(res.converged.all())
        # a window of >= ~0.2 s of kernel time
        t1, _, _ = timed(lambda: K.batched_svd(A, tol), 1, 1, 1)
        inner = max(1, int(0.2 / max(t1, 1e-6)))
        med, lo, hi = timed(lambda: K.batched_svd(A, tol), args.warmup, args.repeats, inner)
        tm, tlo, thi = timed(lambda: torch.linalg.svd(A, full_matrices=False), 1,
                             max(3, args.repeats // 2), 1)
        rec = {"batch": B, "m": m, "n": n, "dtype": str(dtype).replace("torch.", ""),
               "threads": K.batched_threads(n), "lanes_per_pair": 8,
               "lds_bytes": K.batched_lds_bytes(dtype, m, n, True),
               "sweeps_max": int(res.sweeps.max()), "inner": inner,
               "kernel_s": med, "kernel_s_min": lo, "kernel_s_max": hi,
               "matrices_per_s": B / med, "effective_GBps": nbytes / med / 1e9,
               "torch_linalg_svd_s": tm, "torch_linalg_svd_s_min": tlo,
               "torch_linalg_svd_s_max": thi, "speedup_vs_torch": tm / med}
        if not args.skip_loop:
            k = min(args.loop_matrices, B)
            svdj.svd(A[0], method="scalar")  # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(k):
                svdj.svd(A[i], method="scalar")
            torch.cuda.synchronize()
            per = (time.perf_counter() - t0) / k
            rec.update({"scalar_loop_matrices": k, "scalar_loop_s_per_matrix": per,
                        "scalar_loop_s_scaled": per * B, "speedup_vs_scalar_loop": per * B / med})
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
