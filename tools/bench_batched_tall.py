"""Measure the tall batched engine (svd_batched(A, precondition="qr"),
csrc/hip/batched_tall.hip) on one GPU, by the method of tools/bench_batched.py:
per case 3 warm-up calls, then 7 windows of about 0.2 s of back-to-back kernel
entry-point calls between device events, median and spread.

Shapes the LDS kernel also takes are compared with it; shapes it rejects are
compared with the route they take today, the Python loop of svd(A[i]) timed on
16 matrices and scaled to the batch.  Every case is also compared with
torch.linalg.svd on a slice of the batch, scaled (it takes milliseconds per
matrix).  --panels adds one row per forced panel height for the first tall
fp32 case.

    python tools/bench_batched_tall.py --out profiles/batched_tall/bench.jsonl

Needs a GPU; there is no CPU fall-back.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import svdj  # noqa: E402
from bench_batched import timed  # noqa: E402

F32, F64 = torch.float32, torch.float64
CASES = [  # (batch, m, n, dtype)
    (1024, 256, 64, F32),
    (1024, 232, 64, F64),
    (1024, 2048, 64, F32),
    (4096, 4096, 32, F32),
    (4096, 1024, 16, F32),
    (256, 2048, 64, F64),
]


def window(fn, warmup, repeats):
    t1, _, _ = timed(fn, 1, 1, 1)
    inner = max(1, int(0.2 / max(t1, 1e-6)))
    return timed(fn, warmup, repeats, inner) + (inner,)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append JSON lines here")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-matrices", type=int, default=16)
    ap.add_argument("--torch-matrices", type=int, default=128)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--panels", type=int, nargs="*", default=[],
                    help="also time 1024 x 2048x64 fp32 at these forced panel heights")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batched_tall needs a GPU")
    dev = torch.device("cuda:0")
    K = svdj.ops.kernels

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for B, m, n, dtype in CASES:
        g = torch.Generator().manual_seed(B + m + n)
        A = torch.rand(B, m, n, dtype=dtype, generator=g).to(dev)
        nbytes = B * A.element_size() * (2 * m * n + n + n * n)  # A read; U, S, V written
        res = svdj.svd_batched(A, precondition="qr")
        assert res.info["engine"] == "qr_kernel" and bool(res.converged.all())
        tol, rows = res.info["tol"], res.info["panel_rows"]
        med, lo, hi, inner = window(lambda: K.batched_tall_svd(A, tol, panel_rows=rows),
                                    args.warmup, args.repeats)
        rec = {"batch": B, "m": m, "n": n, "dtype": str(dtype).replace("torch.", ""),
               "panel_rows": rows, "panels": res.info["panels"],
               "lds_bytes": res.info["lds_bytes"], "sweeps_max": int(res.sweeps.max()),
               "inner": inner, "qr_kernel_s": med, "qr_kernel_s_min": lo, "qr_kernel_s_max": hi,
               "matrices_per_s": B / med, "effective_GBps": nbytes / med / 1e9}
        fits = K.batched_lds_bytes(dtype, m, n, True) > 0
        if fits:
            ref = svdj.svd_batched(A)
            assert ref.info["engine"] == "kernel"
            ktol = ref.info["tol"]
            kmed, klo, khi, _ = window(lambda: K.batched_svd(A, ktol), args.warmup, args.repeats)
            rec.update({"kernel_s": kmed, "kernel_s_min": klo, "kernel_s_max": khi,
                        "kernel_sweeps_max": int(ref.sweeps.max()),
                        "speedup_vs_kernel": kmed / med})
        else:
            k = min(args.loop_matrices, B)
            assert svdj.svd_batched(A[:1]).info["engine"] == "loop"  # also the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            svdj.svd_batched(A[:k])
            torch.cuda.synchronize()
            per = (time.perf_counter() - t0) / k
            rec.update({"loop_matrices": k, "loop_s_per_matrix": per, "loop_s_scaled": per * B,
                        "speedup_vs_loop": per * B / med})
        if not args.skip_torch:
            # rocSOLVER takes milliseconds per matrix: a slice of the batch, scaled
            k = min(args.torch_matrices, B)
            At = A[:k]
            tm, tlo, thi = (t * B / k for t in timed(
                lambda: torch.linalg.svd(At, full_matrices=False), 1, 3, 1))
            rec.update({"torch_matrices": k, "torch_linalg_svd_s_scaled": tm,
                        "torch_linalg_svd_s_scaled_min": tlo,
                        "torch_linalg_svd_s_scaled_max": thi, "speedup_vs_torch": tm / med})
        emit(rec)
        if (B, m, n, dtype) == (1024, 2048, 64, F32):
            for rows in args.panels:
                if K.batched_tall_lds_bytes(dtype, n, True, rows) == 0:
                    continue
                med, lo, hi, inner = window(
                    lambda: K.batched_tall_svd(A, tol, panel_rows=rows), args.warmup, args.repeats)
                emit({"batch": B, "m": m, "n": n, "dtype": "float32", "panel_rows": rows,
                      "panels": -(-m // rows), "forced": True,
                      "lds_bytes": K.batched_tall_lds_bytes(dtype, n, True, rows),
                      "inner": inner, "qr_kernel_s": med, "qr_kernel_s_min": lo,
                      "qr_kernel_s_max": hi, "matrices_per_s": B / med})
        del A, res
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
