#!/usr/bin/env python3
"""Registers, scratch and LDS of every kernel instantiation in the library (compiles the device code to assembly;
no GPU needed).  usage: python scripts/kernel_resources.py [filter-substring] [-- extra hipcc flags]
       python scripts/kernel_resources.py --diff OTHER.s [--asm THIS.s]
--diff: compares this tree's device assembly (--asm: one compiled before, instead of compiling) with another, kernel symbol by
kernel symbol: the instruction text between the symbol's label and its end, and VGPRs, SGPRs, scratch, LDS and the spill counts
(both values of every symbol whose resources differ are printed).  Exit status 1 when a common symbol differs."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcbrat3d_amd", "csrc")


def kernels_of(path):
    """-> {symbol: (text from the label to the function's end, (vgpr, sgpr, scratch, lds, spilled sgpr, spilled vgpr))} of an assembly file"""
    text = open(path).read()
    res = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S):
        blk = m.group(0)
        g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        res[re.search(r"\.name:\s+(\S+)", blk).group(1)] = (g("vgpr_count"), g("sgpr_count"), g("private_segment_fixed_size"), g("group_segment_fixed_size"),
                                                            g("sgpr_spill_count"), g("vgpr_spill_count"))
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        if m.group(1) in res:
            # (local labels carry the function's number in the file, which moves with the order of instantiation; so do the
            # compiler's comments, which are not instruction text)
            body = re.sub(r"[ \t]*;[^\n]*", "", m.group(2))
            out[m.group(1)] = (re.sub(r"\.L([A-Za-z_]+)\d+_", r".L\1_", body), res[m.group(1)])
    return out


def diff(this, other):
    a, b = kernels_of(this), kernels_of(other)
    common = sorted(set(a) & set(b))
    differ = [k for k in common if a[k] != b[k]]
    dem = lambda names: subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    for title, names in (("only here", sorted(set(a) - set(b))), ("only in the other", sorted(set(b) - set(a))), ("differ", differ)):
        for n in dem(names) if names else []:
            if n:
                print("%s: %s" % (title, n))
    fmt = "vgpr %d sgpr %d scratch %d lds %d spill_sgpr %d spill_vgpr %d"
    changed = [k for k in differ if a[k][1] != b[k][1]]
    for k, n in zip(changed, dem(changed) if changed else []):
        print("resources: %s\n  here:  %s\n  other: %s" % (n, fmt % a[k][1], fmt % b[k][1]))
    print("kernels: %d here, %d in the other, %d common, %d of them differ, %d of those in resources" % (len(a), len(b), len(common), len(differ), len(changed)))
    return 1 if differ else 0


def main():
    argv = sys.argv[1:]
    if "--diff" in argv:
        other = argv[argv.index("--diff") + 1]
        this = argv[argv.index("--asm") + 1] if "--asm" in argv else None
        if this is None:
            this = os.path.join(os.environ.get("KRES_DIR") or tempfile.mkdtemp(prefix="kres"), "mcbrat_api.s")
            subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                                   "-o", this, os.path.join(CSRC, "mcbrat_api.hip")])
        sys.exit(diff(this, other))
    extra = []
    if "--" in argv:
        i = argv.index("--")
        argv, extra = argv[:i], argv[i + 1:]
    flt = argv[0] if argv else ""
    keep = os.environ.get("KRES_DIR")
    tmp = keep or tempfile.mkdtemp(prefix="kres")
    os.makedirs(tmp, exist_ok=True)
    asm = os.path.join(tmp, "mcbrat_api.s")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
           "-o", asm, os.path.join(CSRC, "mcbrat_api.hip")] + extra
    subprocess.check_call(cmd)
    text = open(asm).read()
    # the metadata block at the end lists every kernel
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        if flt and flt not in dem:
            continue
        g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        short = re.sub(r"mcbrat::|\(mcbrat::DevParams\)|\(mcbrat::FinishParams\)", "", dem)
        print("%-70s vgpr %3d sgpr %3d scratch %4d lds %6d spill_sgpr %3d spill_vgpr %3d" % (
            short[:70], g("vgpr_count"), g("sgpr_count"), g("private_segment_fixed_size"), g("group_segment_fixed_size"),
            g("sgpr_spill_count"), g("vgpr_spill_count")))
    print("assembly:", asm)


if __name__ == "__main__":
    main()
