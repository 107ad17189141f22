"""Compare two device-only assembly listings kernel by kernel (dev aid).

    hipcc <project flags> --cuda-device-only -S csrc/hip/block.hip -o X.s
    python tools/asm_kernel_diff.py OLD.s NEW.s [TOUCHED_REGEX]

A kernel's text is everything from its `.type NAME,@function` line to its
`.size NAME` line: the instruction stream, its labels and the kernel
descriptor (`.amdhsa_kernel` block).  The function index inside local labels
(`.LBB12_3`, `.Lfunc_end12`) is dropped, since it only counts the functions
before this one in the file.  Prints one line per kernel and exits 1 when the
symbol sets differ or a kernel NOT matching TOUCHED_REGEX differs.
"""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, body = m.group(1), []
        if name is None:
            continue
        body.append(re.sub(r"(\.L|\b)(BB|func_end|func_begin)\d+", r"\1\2", line))
        if re.match(r"\s*\.size\s+" + re.escape(name) + ",", line):
            out[name] = "".join(body)
            name = None
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    touched = re.compile(sys.argv[3]) if len(sys.argv) > 3 else None
    bad = 0
    for n in sorted(set(old) ^ set(new)):
        print("only in", "old" if n in old else "new", n)
        bad += 1
    same = 0
    for n in sorted(set(old) & set(new)):
        if old[n] == new[n]:
            same += 1
            continue
        is_touched = bool(touched and touched.search(n))
        print(f"differs ({'touched' if is_touched else 'UNTOUCHED'}): {n} "
              f"{old[n].count(chr(10))} -> {new[n].count(chr(10))} lines")
        bad += 0 if is_touched else 1
    print(f"{len(old)} / {len(new)} kernels, {same} identical")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
