#!/usr/bin/env python3
"""Writes the kernel the host library chooses for every input its choice reads (scripts/kernel_choice.hip; no GPU needed).

    python scripts/kernel_choice.py [--csrc DIR] [--out FILE]

--csrc: the directory of mcbrat_api.hip (default: this tree's); --out: where to write (default: tests/golden/kernel_choice.txt).

The file has one line per kernel (or per refusal, "!text"): the name, then " | <block> <dynamic LDS>:" and the inputs that got it, as
base/mask pairs in hex -- every code base | m with m a subset of mask's bits (a bit in a mask: the choice did not depend on it
there).  Codes of trace_kernel and of trace_block_kernel are told apart by the kernel (the bit layouts: kernel_choice.hip)."""
import argparse
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cubes(codes):
    """a set of codes as a short list of (base, mask): disjoint; greedily, from the smallest code left, free every bit that can be freed"""
    left, out = set(codes), []
    while left:
        base, mask = min(left), 0
        for b in range(32):
            if base >> b & 1:
                continue
            m, sub, ok = mask | 1 << b, mask | 1 << b, True
            while ok:
                ok = base | sub in left
                if sub == 0:
                    break
                sub = (sub - 1) & m
            if ok:
                mask = m
        sub = mask
        while True:
            left.discard(base | sub)
            if sub == 0:
                break
            sub = (sub - 1) & mask
        out.append((base, mask))
    return out


def compact(text):
    """the program's lines (K index kernel; R index kernel block lds, or R index !refusal; T / B code result) -> the file"""
    kernels, results, by = {}, {}, {}
    for line in text.split("\n"):
        w = line.split(" ", 2)
        if w[0] == "K":
            kernels[w[1]] = w[2]
        elif w[0] == "R":
            f = w[2].split()
            results[w[1]] = (w[2], "") if w[2].startswith("!") else (kernels[f[0]], "%s %s" % (f[1], f[2]))
        elif w[0] in ("T", "B"):
            by.setdefault(results[w[2]], []).append(int(w[1], 16))
    names = []
    for name, _ in by:
        if name not in names:
            names.append(name)
    out = ["# kernel choice of the host library (scripts/kernel_choice.py explains the format, scripts/kernel_choice.hip the input codes)"]
    for name in names:
        out.append(name + "".join(" | %s: %s" % (how, " ".join("%x/%x" % c for c in cubes(codes))) for (n, how), codes in by.items() if n == name))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "mcbrat3d_amd", "csrc"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "kernel_choice.txt"))
    a = ap.parse_args()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory(prefix="kchoice") as tmp:
        exe = os.path.join(tmp, "kernel_choice")
        # host code only: the kernels' host stubs carry their names; the device image they would register is never built, so the
        # linker is told to leave that one symbol unresolved (nothing here launches a kernel)
        subprocess.check_call([hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-rdynamic", "-I", a.csrc, "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "scripts", "kernel_choice.hip"), os.path.join(a.csrc, "mcbrat_host.cpp"), "-ldl",
                               "-Wl,--unresolved-symbols=ignore-all", "-o", exe])
        text = compact(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    with open(a.out, "w") as f:
        f.write(text)
    print("%s: %d lines, %d bytes" % (a.out, text.count("\n"), len(text)))


if __name__ == "__main__":
    main()
