#!/usr/bin/env python3
"""Did a refactor of a .hip file change what the compiler makes of it?

Compiles the same source file of two checkouts for gfx950 with the flags of dynfu_amd/build.py (product, and again
with -DDFA_DEV_AB), and prints two markdown tables per build: the kernels' resources as the compiler reports them
(-Rpass-analysis=kernel-resource-usage) and, per kernel, whether the gfx950 assembly (--save-temps) is identical
once comments, debug lines and symbol names are stripped.  No GPU needed.  Exit status 1 if any resource differs
or the sets of kernels differ (a differing ISA alone is reported, not failed).

    python tools/kernel_isa_diff.py PARENT_CHECKOUT BRANCH_CHECKOUT [--file solve.hip] [--drop-arg KERNEL:INDEX]

--drop-arg pcg_paired_kernel:1 matches kernels of the two sides whose template argument lists differ by the one
argument a change removed (index into the parent's list).
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dynfu_amd.build import FLAGS, hipcc  # noqa: E402

FIELDS = ["VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]",
          "Occupancy [waves/SIMD]"]


def compile_one(checkout, name, extra, out):
    os.makedirs(out, exist_ok=True)
    src = os.path.join(os.path.abspath(checkout), "dynfu_amd", "csrc", name)
    cmd = [hipcc()] + FLAGS + extra + ["-Rpass-analysis=kernel-resource-usage", "--save-temps", "-c", src, "-o", "x.o"]
    r = subprocess.run(cmd, cwd=out, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("hipcc failed:\n" + r.stderr)
    asm = [f for f in os.listdir(out) if f.endswith("gfx950.s")][0]
    return r.stderr, open(os.path.join(out, asm)).read()


def resources(remarks):
    res, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: .*?: +(.*?): (.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return res


def bodies(asm):
    """mangled name -> instruction text of the function, comments / debug lines / symbol names stripped"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M):
        lines = []
        for ln in m.group(2).splitlines():
            ln = ln.split(";")[0].rstrip()
            if not ln.strip() or re.match(r"\s*\.(loc|file|cfi_\w+)\b", ln):
                continue
            ln = re.sub(r"_Z\w+", "SYM", ln)
            ln = re.sub(r"\.L(BB|tmp|func_\w+?)\d+(_\d+)?", lambda g: ".L" + g.group(1) + (g.group(2) or ""), ln)
            lines.append(ln)
        out[m.group(1)] = "\n".join(lines)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, (re.sub(r"^(void )?dfa::", "", re.sub(r"\(.*", "", d)) for d in r.stdout.splitlines())))


def drop(name, rules):
    for kern, idx in rules:
        m = re.match(r"(%s)<(.*)>$" % re.escape(kern), name)
        if m:
            args = [a.strip() for a in m.group(2).split(",")]
            del args[idx]
            return "%s<%s>" % (m.group(1), ", ".join(args))
    return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--file", default="solve.hip")
    ap.add_argument("--drop-arg", action="append", default=[])
    a = ap.parse_args()
    rules = [(r.split(":")[0], int(r.split(":")[1])) for r in a.drop_arg]
    bad = False
    for label, extra in (("product", []), ("development (-DDFA_DEV_AB)", ["-DDFA_DEV_AB"])):
        with tempfile.TemporaryDirectory() as tmp:
            rp, ap_ = compile_one(a.parent, a.file, extra, os.path.join(tmp, "p"))
            rb, ab_ = compile_one(a.branch, a.file, extra, os.path.join(tmp, "b"))
        resp, resb, isap, isab = resources(rp), resources(rb), bodies(ap_), bodies(ab_)
        dp, db = demangle(list(resp)), demangle(list(resb))
        keyp = {drop(dp[n], rules): n for n in resp}
        keyb = {db[n]: n for n in resb}
        print("\n### %s build of %s: %d kernels (parent), %d (branch)\n" % (label, a.file, len(keyp), len(keyb)))
        for k in sorted(set(keyp) ^ set(keyb)):
            print("* only in %s: `%s`" % ("parent" if k in keyp else "branch", k))
            bad = True
        print("| kernel (branch name) | " + " | ".join(FIELDS) + " | resources | ISA |")
        print("|---|" + "---|" * (len(FIELDS) + 2))
        for k in sorted(set(keyp) & set(keyb)):
            p, b = resp[keyp[k]], resb[keyb[k]]
            same = all(p[f] == b[f] for f in FIELDS)
            bad |= not same
            cells = [b[f] if p[f] == b[f] else "%s -> %s" % (p[f], b[f]) for f in FIELDS]
            isa = "identical" if isap[keyp[k]] == isab[keyb[k]] else "differs"
            print("| `%s` | %s | %s | %s |" % (k, " | ".join(cells), "same" if same else "DIFFER", isa))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
