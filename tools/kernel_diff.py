#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libwipa.so function by function: the instruction text of every kernel of OLD (addresses
and padding stripped, branch targets by label) against the kernel of the same symbol in NEW, or -- when the symbol is gone, e.g. because
a template gained a defaulted parameter -- against every kernel of NEW that has no counterpart in OLD.  Prints which kernels are
identical, which were renamed with an identical body, which differ, and what is new.  Needs llvm-objdump of the ROCm toolchain; no GPU.
usage: python tools/kernel_diff.py OLD/libwipa.so NEW/libwipa.so"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump")


def kernels(lib):
    d = tempfile.mkdtemp()
    try:
        shutil.copy(lib, os.path.join(d, "lib.so"))  # the bundles are extracted next to the file
        subprocess.check_call([OBJDUMP, "--offloading", os.path.join(d, "lib.so")], cwd=d, stdout=subprocess.DEVNULL)
        out = {}
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            txt = subprocess.check_output([OBJDUMP, "-d", "--no-show-raw-insn", os.path.join(d, f)], text=True)
            cur = None
            for line in txt.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = m.group(1)
                    out.setdefault(cur, [])
                    continue
                if cur is None or not line.strip() or line.strip() == "...":
                    continue
                out[cur].append(re.sub(r"<[^>]*>", "<L>", line.split("//")[0].strip()))
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_new = {k: v for k, v in new.items() if k not in old}
    same = [k for k in old if k in new and old[k] == new[k]]
    differ = [k for k in old if k in new and old[k] != new[k]]
    renamed, gone = [], []
    for k in old:
        if k in new:
            continue
        twins = [n for n, v in only_new.items() if v == old[k]]
        (renamed if twins else gone).append((k, twins))
    taken = {n for _, t in renamed for n in t}
    print(f"kernels in OLD: {len(old)}; same symbol, identical instructions: {len(same)}; same symbol, different instructions: {len(differ)}; "
          f"renamed with identical instructions: {len(renamed)}; gone: {len(gone)}; new in NEW: {len(only_new) - len(taken)}")
    for k in differ:
        print("DIFFERENT ", k)
    for k, _ in gone:
        print("GONE      ", k)
    for k, t in renamed:
        print("RENAMED   ", k, "->", ", ".join(t))
    for n in sorted(only_new):
        if n not in taken:
            print("NEW       ", n, f"({len(only_new[n])} instructions)")
    return 1 if differ or gone else 0


if __name__ == "__main__":
    sys.exit(main())
