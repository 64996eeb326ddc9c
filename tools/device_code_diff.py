#!/usr/bin/env python3
"""Is the device code of the working tree the device code of a base revision?  (tools/device_code_diff.py [rev], default HEAD)

Both trees are copied into a scratch directory and every translation unit under conan_slam_amd/csrc is compiled to
gfx950 assembly (hipcc -S --cuda-device-only, as tools/kernel_resources.py does).  The comparison is per symbol, not
by position: the set of kernels must be the same, and for every function the instruction text and for every kernel the
metadata entry (VGPR / AGPR / SGPR / LDS / scratch, arguments) must be identical.  Labels are numbered by position in the
file and the __hip_cuid_<hash> lines change from compile to compile: both are normalised away."""
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("conan_slam_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only"]


def compile_tree(tree):
    srcs = sorted(f for f in os.listdir(os.path.join(tree, CSRC)) if f.endswith(".hip"))

    def one(src):
        out = os.path.join(tree, src + ".s")
        subprocess.run(["hipcc"] + FLAGS + ["-o", out, os.path.join(tree, CSRC, src)], check=True, stderr=subprocess.DEVNULL)
        return src, open(out).read()

    with concurrent.futures.ThreadPoolExecutor(max_workers=len(srcs)) as ex:
        return dict(ex.map(one, srcs))


def split(asm):
    """{symbol: text} for every function body and every kernel's descriptor + metadata entry"""
    asm = "\n".join(l for l in asm.split("\n") if "__hip_cuid_" not in l)
    asm = re.sub(r"\.LBB\d+_", ".LBB_", asm)
    asm = re.sub(r"\bBB\d+_", "BB_", asm)  # (the same labels in the loop comments: "in Loop: Header=BB44_4", "Child Loop BB57_7")
    asm = re.sub(r"[ \t]+;", " ;", asm)  # (comments are aligned with padding that depends on the label's width)
    asm = re.sub(r"\.L(func_end|func_begin|tmp)\d+", r".L\1", asm)
    parts = {}
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n(.*?)^\t\.size\t\1,[^\n]*\n", asm, flags=re.S | re.M):
        parts["text " + m.group(1)] = m.group(2)
    meta = asm[asm.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in asm else ""
    for blk in re.split(r"^  - (?=\.)", meta, flags=re.M)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        parts["meta " + name] = blk.split("amdhsa.target:")[0]
    return parts


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    scratch = tempfile.mkdtemp(prefix="cslam_devdiff_")
    base, new = os.path.join(scratch, "base"), os.path.join(scratch, "new")
    os.makedirs(base)
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC, "include"], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", base], input=tar, check=True)
    for d in (CSRC, "include"):
        shutil.copytree(os.path.join(ROOT, d), os.path.join(new, d), ignore=shutil.ignore_patterns("*.o", "*.so", "__pycache__"))
    with concurrent.futures.ThreadPoolExecutor(max_workers=2) as ex:
        a, b = ex.map(compile_tree, (base, new))
    bad = 0
    for src in sorted(set(a) | set(b)):
        pa, pb = split(a.get(src, "")), split(b.get(src, ""))
        kernels = sum(1 for k in pa if k.startswith("meta "))
        only = sorted(set(pa) ^ set(pb))
        differ = sorted(k for k in set(pa) & set(pb) if pa[k] != pb[k])
        print(f"{src:24s} {kernels:4d} kernels, {len(pa):4d} symbols: "
              + ("identical" if not only and not differ else f"{len(only)} only on one side, {len(differ)} differ"))
        for k in only + differ:
            print("    " + k)
        bad += len(only) + len(differ)
    shutil.rmtree(scratch)
    print("device code: " + ("IDENTICAL to " + rev if not bad else f"{bad} DIFFERENCES against " + rev))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
