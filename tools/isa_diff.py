#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, function by function (no GPU needed):
    python tools/isa_diff.py OLD_TREE NEW_TREE [-j N]
Every stratum-dsp_amd/csrc/*.hip of both trees is compiled to device assembly with its own
Makefile's HIPCC/HIPFLAGS (--cuda-device-only -S).  The assembly is split into functions by
mangled name and into .amdhsa_kernel descriptors, comments are stripped and the compiler's local
label numbers normalised, so a function may move between translation units and still compare
equal.  Prints same / differs / only in OLD / only in NEW per function and per descriptor, and
exits non-zero on any difference.  It compares for equality only.
"""
import argparse, collections, glob, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor


def tree_asm(tree, jobs, tmp):
    pkg = os.path.join(os.path.abspath(tree), "stratum-dsp_amd")
    cmd = subprocess.check_output(
        ["make", "-s", "-C", pkg, "--no-print-directory", "--eval",
         "isa-diff-cmd: ; @echo $(HIPCC) $(HIPFLAGS)", "isa-diff-cmd"], text=True).split()
    srcs = sorted(glob.glob(os.path.join(pkg, "csrc", "*.hip")))

    def one(src):
        out = os.path.join(tmp, os.path.basename(src)[:-4] + ".s")
        subprocess.check_call(cmd + ["--cuda-device-only", "-S", "-Wno-unused-command-line-argument",
                                     src, "-o", out], cwd=pkg)
        return open(out).read()
    with ThreadPoolExecutor(min(jobs, 16)) as ex:
        return list(ex.map(one, srcs))


def normalise(lines):
    tmps = {}
    text = "\n".join(l for l in (re.sub(r"\s*;.*", "", l).rstrip() for l in lines) if l)
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    return re.sub(r"\.Ltmp\d+", lambda m: tmps.setdefault(m.group(0), ".Ltmp%d" % len(tmps)), text)


def split(asms):
    """{("function"|"descriptor", name): sorted bodies} (a static name may recur across units)"""
    parts = collections.defaultdict(list)
    for asm in asms:
        fn = desc = None  # (name, lines) being collected; a kernel's descriptor sits inside its function
        for line in asm.splitlines():
            d = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
            if d:
                desc = (d.group(1), [])
            if desc:
                desc[1].append(line)
                if re.match(r"\s*\.end_amdhsa_kernel", line):
                    parts["descriptor", desc[0]].append(normalise(desc[1]))
                    desc = None
                continue
            m = re.match(r"\s*\.type\s+([^,\s]+),@function", line)
            if m and fn is None:
                fn = (m.group(1), [])
            if fn:
                fn[1].append(line)
                if re.match(r"\s*\.size\s+%s," % re.escape(fn[0]), line):
                    parts["function", fn[0]].append(normalise(fn[1]))
                    fn = None
    return {k: sorted(v) for k, v in parts.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old"), ap.add_argument("new"), ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new:
        old, new = split(tree_asm(a.old, a.j, t_old)), split(tree_asm(a.new, a.j, t_new))
    counts = collections.Counter()
    for key in sorted(set(old) | set(new)):
        verdict = ("only in NEW" if key not in old else "only in OLD" if key not in new
                   else "same" if old[key] == new[key] else "differs")
        counts[verdict] += 1
        print("%-11s %-10s %s" % (verdict, key[0], key[1]))
    print("total: " + ", ".join("%d %s" % (n, v) for v, n in sorted(counts.items())))
    return 0 if set(counts) <= {"same"} else 1


if __name__ == "__main__":
    sys.exit(main())
