"""The native engine's host-only plan unit (csrc/distributed/dist_plan.cpp)
under AddressSanitizer + UBSan: tools/micro/dist_plan_check.cpp is built as a
stand-alone program and run once on the CPU (no Python in the process, no
preload).  It checks the plan of every rank, the pair lists, the placement
remap, moves_to_canonical, exposed_time, the id file, geometry and rules."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svd-jacobi-mpi-cuda_amd", "csrc")


def test_dist_plan_check_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "dist_plan_check")
    # The sanitizer runtime is linked into the program: ASan refuses to start
    # when any other preloaded library comes before a shared runtime.  Where the
    # runtime itself is preloaded (tools/asan_cpu_tests.sh), that one is used.
    static = [] if "asan" in os.environ.get("LD_PRELOAD", "") else ["-static-libasan", "-static-libubsan"]
    cmd = [os.environ.get("CXX", "g++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           *static, "-fno-omit-frame-pointer", "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
           "-I" + os.path.join(CSRC, "include"), "-I" + os.path.join(CSRC, "distributed"),
           os.path.join(ROOT, "tools", "micro", "dist_plan_check.cpp"),
           os.path.join(CSRC, "distributed", "dist_plan.cpp"),
           os.path.join(CSRC, "cpu", "schedule.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)  # no g++: raises, not skips
    assert b.returncode == 0, b.stdout + b.stderr
    env = {k: v for k, v in os.environ.items() if k != "SVDJ_DEBUG"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    m = re.search(r"(\d+) cases checked, 0 checks failed", out)
    assert m and int(m.group(1)) >= 600, out[-2000:]
