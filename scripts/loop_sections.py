#!/usr/bin/env python3
"""Static instruction counts of the block walk's collision loop, section by section (no GPU needed).

Compiles the device code with -DMCBRAT_MARKS (each STAMP(i) of mcbrat_blockwalk.hip becomes an `@@mark i` comment in the
assembly), takes the step cloud's instantiation trace_block_kernel<768, true, false, false, 2, 0, true, 3> (or the one whose mangled name is given), keeps the basic blocks of its
inner loop and counts, per section between two marks, vector / scalar / LDS instructions, s_nop / s_waitcnt, and the classes
worth watching (moves, 64-bit address and multiply-add ops, SGPR spills into VGPR lanes, f32 <-> f64 conversions, kernel-argument
reloads, exec-mask saves).  Sections follow the layout of the code, so a section holds the rare branch that follows its mark.

    python scripts/loop_sections.py [assembly.s [mangled kernel name]]      (without an argument: compiles mcbrat_api.hip first,
    about a minute; "-" for the assembly compiles too)"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = sys.argv[2] if len(sys.argv) > 2 else "_ZN6mcbrat18trace_block_kernelILi768ELb1ELb0ELb0ELi2ELi0ELb1ELi3EEEvNS_9DevParamsE"
SECTIONS = {"7": "loop head + exits", "5": "launch", "0": "collision", "2": "scattering angle",
            "3": "next_direct", "4": "next_direct + drop test + leg set-up", "6": "crossings + exit test", "1": "move (loop end)"}
ORDER = ["loop head + exits", "launch", "collision", "scattering angle", "next_direct + drop test + leg set-up",
         "crossings + exit test", "move (loop end)"]
CLASSES = [("v_mov", "v_mov_b"), ("cndmask", "v_cndmask"), ("addr_u64", "v_lshl_add_u64"), ("mad_u64", "v_mad_u64_u32"),
           ("mul_lo", "v_mul_lo_u32"), ("readlane", "v_readlane"), ("writelane", "v_writelane"), ("rdfirstln", "v_readfirstlane"),
           ("cvt_f64", "v_cvt_f64_f32"), ("cvt_f32", "v_cvt_f32_f64"), ("s_load", "s_load"), ("saveexec", "s_and_saveexec")]


def assembly():
    if len(sys.argv) > 1 and sys.argv[1] != "-":
        return open(sys.argv[1]).read()
    out = os.path.join(tempfile.mkdtemp(prefix="loopsec"), "mcbrat_api.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
                           "-S", "-DMCBRAT_MARKS", "-o", out, os.path.join(ROOT, "mcbrat3d_amd", "csrc", "mcbrat_api.hip")])
    return open(out).read()


def main():
    txt = assembly()
    i = txt.index("\n" + KERNEL + ":")
    body = txt[i:txt.index(".Lfunc_end", i)].split("\n")
    # the iteration loop: the loop of depth 2 that holds the marks (an inner loop where no rare branch loops, as under RARE)
    hdrs = [re.match(r"\.LBB(\d+_\d+):", l).group(1) for k, l in enumerate(body)
            if re.match(r"\.LBB\d+_\d+:", l) and re.search(r"This (Inner )?Loop Header: Depth=2", body[k + 1])]
    marks = collections.Counter()
    cur = None
    for l in body:
        if re.match(r"(\.LBB\d+_\d+|; %bb\.\d+):", l):
            cur = next((h for h in hdrs if "Header=BB%s " % h in l or "Loop BB%s " % h in l or l.startswith(".LBB%s:" % h)), None)
        elif cur and "@@mark" in l:
            marks[cur] += 1
    hdr = marks.most_common(1)[0][0]
    inloop, sec, cnt = False, "move (loop end)", collections.defaultdict(collections.Counter)
    for l in body:
        if re.match(r"(\.LBB\d+_\d+|; %bb\.\d+):", l):  # a basic block: in the loop if it is its header or one of its blocks
            inloop = ("Header=BB%s " % hdr in l) or ("Loop BB%s " % hdr in l) or l.startswith(".LBB%s:" % hdr)
            continue
        t = l.strip()
        m = re.search(r"@@mark (\d+)", t)
        if m:
            sec = SECTIONS[m.group(1)]
            continue
        if not inloop or not t or t.startswith((";", ".")):
            continue
        op, c = t.split()[0], cnt[sec]
        c["all"] += 1
        c["s_nop" if op.startswith("s_nop") else "s_waitcnt" if op.startswith("s_waitcnt") else "S" if op.startswith("s_")
          else "V" if op.startswith("v_") else "DS" if op.startswith("ds_") else "other"] += 1
        for k, pfx in CLASSES:
            c[k] += op.startswith(pfx)
    keys = ["all", "V", "S", "DS", "s_nop", "s_waitcnt"] + [k for k, _ in CLASSES]
    print("%-38s" % "section" + "".join("%10s" % k for k in keys))
    tot = collections.Counter()
    for s in ORDER:
        tot.update(cnt[s])
        print("%-38s" % s + "".join("%10d" % cnt[s][k] for k in keys))
    print("%-38s" % "loop total" + "".join("%10d" % tot[k] for k in keys))


if __name__ == "__main__":
    main()
