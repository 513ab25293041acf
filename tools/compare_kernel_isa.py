#!/usr/bin/env python3
"""Are the kernels of one csrc/*.hip file the same machine code in two source trees?

    python tools/compare_kernel_isa.py OLD_CSRC NEW_CSRC FILE.hip [--pairs PAIRS.txt]

Compiles FILE.hip of both csrc directories to gfx950 device assembly with the flags of _build.py and
compares, kernel by kernel, the text from the kernel's label to its .Lfunc_end plus its .amdhsa_*
descriptor block (VGPRs, SGPRs, LDS, scratch, kernarg size).  Only the kernel's own mangled name and
the function index inside local labels (.LBB<i>_<n>, .Lfunc_end<i>) are normalised; everything else
is compared as text.  Kernels are paired by their demangled name; a kernel whose signature changed is
paired through PAIRS.txt, one `old name => new name` per line (names as this tool prints them, `#`
starts a comment).  Prints one line per kernel and exits non-zero if any kernel differs or stays
unpaired.  For a refactor that must leave the kernels alone this is the evidence, without a GPU.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
ARCH = os.environ.get("NXD_OFFLOAD_ARCH", "gfx950")
# _build.py: common flags and the per-file extras
FLAGS = ["-O3", "-fPIC", "-std=c++17", f"--offload-arch={ARCH}", "-fno-gpu-rdc", "-Wno-unused-result", "-Wno-unused-variable"]
EXTRA = {"flash_attn_bwd": ["-mllvm", "-amdgpu-mfma-vgpr-form"]}


def device_asm(csrc: Path, name: str, out: Path) -> str:
    src = csrc / name
    cmd = [os.path.join(ROCM, "bin", "hipcc"), *FLAGS, *EXTRA.get(src.stem, []), f"-I{csrc}", "--cuda-device-only", "-S",
           str(src), "-o", str(out)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.exit(f"compilation failed: {' '.join(cmd)}\n{r.stdout}")
    return out.read_text()


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or os.path.join(ROCM, "llvm", "bin", "llvm-cxxfilt")
    r = subprocess.run([tool], input="\n".join(names) + "\n", stdout=subprocess.PIPE,
                       text=True, check=True)
    # `void ns::kernel<...>(args)` -> `ns::kernel<...>`
    return [re.sub(r"^void ", "", re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", d.strip())) for d in r.stdout.splitlines()]


def kernels(asm: str) -> dict:
    """demangled name -> normalised text (body + descriptor) of every kernel of the assembly"""
    lines = asm.splitlines()
    mangled = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    out = {}
    for sym, nice in zip(mangled, demangle(mangled)):
        start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        d0 = next(i for i, l in enumerate(lines) if l.strip() == ".amdhsa_kernel " + sym)
        d1 = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        # this compiler puts the descriptor between the last instruction and .Lfunc_end; take it once
        block = lines[start:end + 1] + ([] if start < d0 < end else lines[d0:d1 + 1])
        text = "\n".join(block).replace(sym, "KERNEL")
        text = re.sub(r"(\.L|\b)BB\d+_", r"\1BB_", text)   # .LBB<i>_<n>, and BB<i>_<n> where a loop comment names a label
        text = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", text)
        text = re.sub(r"[ \t]+;", " ;", text)     # comments are aligned after the label, whose width has <i> in it
        out[nice] = text
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_csrc", type=Path)
    ap.add_argument("new_csrc", type=Path)
    ap.add_argument("file")
    ap.add_argument("--pairs", type=Path, help="lines `old name => new name` for kernels whose signature changed")
    a = ap.parse_args()
    pairs = {}
    if a.pairs:
        for line in a.pairs.read_text().splitlines():
            line = line.split("#")[0].strip()
            if line:
                o, n = (s.strip() for s in line.split("=>"))
                pairs[o] = n
    with tempfile.TemporaryDirectory() as tmp:
        old = kernels(device_asm(a.old_csrc, a.file, Path(tmp) / "old.s"))
        new = kernels(device_asm(a.new_csrc, a.file, Path(tmp) / "new.s"))
    bad = 0
    taken = set()
    for o, text in old.items():
        n = pairs.get(o, o)
        if n not in new:
            print(f"unpaired   {o}  (old only)")
            bad += 1
            continue
        taken.add(n)
        same = text == new[n]
        bad += not same
        print(f"{'identical' if same else 'differs  '}  {o}" + (f"  <->  {n}" if n != o else ""))
    for n in new:
        if n not in taken:
            print(f"unpaired   {n}  (new only)")
            bad += 1
    print(f"{a.file}: {len(old)} old / {len(new)} new kernels, {bad} not identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
