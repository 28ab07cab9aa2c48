#!/usr/bin/env python3
"""Did a refactor of .hip files change what the compiler makes of them?

Compiles source files of two checkouts for gfx950 with the flags of dynfu_amd/build.py (product, and again with
-DDFA_DEV_AB), and prints two markdown tables per build: the kernels' resources as the compiler reports them
(-Rpass-analysis=kernel-resource-usage) and, per kernel, whether the gfx950 assembly (--save-temps) is identical
once comments, debug lines and symbol names are stripped.  No GPU needed.  Exit status 1 if any resource differs,
the sets of kernels differ or a kernel appears twice on one side (a differing ISA alone is reported, not failed,
unless --require-identical).

    python tools/kernel_isa_diff.py PARENT_CHECKOUT BRANCH_CHECKOUT --file solve6_assemble.hip [--drop-arg KERNEL:INDEX]
    python tools/kernel_isa_diff.py PARENT_CHECKOUT BRANCH_CHECKOUT --parent-files solve.hip \
        --branch-files solve_graph.hip,solve_linearise.hip,... [--define NAME[=VALUE] ...] [--require-identical]

--file names one file, the same on both sides.  --parent-files / --branch-files name a comma-separated list per side
(code that moved between files): each side's kernels are the union over its files.
--define NAME or NAME=VALUE adds -DNAME / -DNAME=VALUE to every compilation (repeatable).
--drop-arg pcg_paired_kernel:1 matches kernels of the two sides whose template argument lists differ by the one
argument a change removed (index into the parent's list).
--drop-branch-arg s6_linearise_kernel:1:false does the same for an argument a change ADDED: the branch's instantiations
whose argument at that index has that value lose it before the names are matched (the others stay "only in branch").
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

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
            # (.section / .text: where the NEXT symbol of the file goes — it changes with what follows the kernel in its file)
            if not ln.strip() or re.match(r"\s*\.(loc|file|cfi_\w+|section|text)\b", ln):
                continue
            ln = re.sub(r"_Z\w+", "SYM", ln)
            ln = re.sub(r"\.L(BB|tmp|func_\w+?)\d+(_\d+)?", lambda g: ".L" + g.group(1) + (g.group(2) or ""), ln)
            lines.append(ln)
        out[m.group(1)] = "\n".join(lines)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    plain = (d.replace("(anonymous namespace)::", "") for d in r.stdout.splitlines())
    return dict(zip(names, (re.sub(r"^(void )?dfa::", "", re.sub(r"\(.*", "", d)) for d in plain)))


def compile_side(checkout, files, extra, out):
    """the union of the files' kernels: demangled name -> (resources, body); and the names met more than once"""
    with ThreadPoolExecutor(max_workers=4) as ex:
        outs = list(ex.map(lambda f: compile_one(checkout, f, extra, os.path.join(out, f)), files))
    kernels, twice = {}, []
    for remarks, asm in outs:
        res, isa = resources(remarks), bodies(asm)
        names = demangle(list(res))
        for n in res:
            if names[n] in kernels:
                twice.append(names[n])
            kernels[names[n]] = (res[n], isa[n])
    return kernels, twice


def drop(name, rules):
    for kern, idx, *value in rules:
        m = re.match(r"(%s)<(.*)>$" % re.escape(kern), name)
        if m:
            args = [a.strip() for a in m.group(2).split(",")]
            if value and args[idx] != value[0]:  # (a rule with a value only meets the instantiations that have it)
                continue
            del args[idx]
            # (a kernel that had no template arguments before the change added its first one keeps its bare name)
            return "%s<%s>" % (m.group(1), ", ".join(args)) if args else m.group(1)
    return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--file", help="one file of csrc/, the same on both sides")
    ap.add_argument("--parent-files", help="comma-separated; instead of --file for the parent")
    ap.add_argument("--branch-files", help="comma-separated; instead of --file for the branch")
    ap.add_argument("--define", action="append", default=[], metavar="NAME[=VALUE]")
    ap.add_argument("--drop-arg", action="append", default=[])
    ap.add_argument("--drop-branch-arg", action="append", default=[], metavar="KERNEL:INDEX:VALUE")
    ap.add_argument("--require-identical", action="store_true", help="a differing ISA fails too")
    a = ap.parse_args()
    rules = [(r.split(":")[0], int(r.split(":")[1])) for r in a.drop_arg]
    rules_b = [(r.split(":")[0], int(r.split(":")[1]), r.split(":")[2]) for r in a.drop_branch_arg]
    if not (a.file or (a.parent_files and a.branch_files)):
        ap.error("--file, or --parent-files and --branch-files")
    pfiles = (a.parent_files or a.file).split(",")
    bfiles = (a.branch_files or a.file).split(",")
    what = pfiles[0] if pfiles == bfiles else "%s -> %s" % (", ".join(pfiles), ", ".join(bfiles))
    defines = ["-D" + d for d in a.define]
    bad = False
    for label, extra in (("product", []), ("development (-DDFA_DEV_AB)", ["-DDFA_DEV_AB"])):
        with tempfile.TemporaryDirectory() as tmp:
            kp, twice_p = compile_side(a.parent, pfiles, defines + extra, os.path.join(tmp, "p"))
            kb, twice_b = compile_side(a.branch, bfiles, defines + extra, os.path.join(tmp, "b"))
        kp = {drop(k, rules): v for k, v in kp.items()}
        kb = {drop(k, rules_b): v for k, v in kb.items()}
        print("\n### %s build%s of %s: %d kernels (parent), %d (branch)\n" % (label, "".join(" " + d for d in defines), what, len(kp), len(kb)))
        for side, twice in (("parent", twice_p), ("branch", twice_b)):
            for k in twice:
                print("* twice in %s: `%s`" % (side, k))
                bad = True
        for k in sorted(set(kp) ^ set(kb)):
            print("* only in %s: `%s`" % ("parent" if k in kp else "branch", k))
            bad = True
        print("| kernel (branch name) | " + " | ".join(FIELDS) + " | resources | ISA |")
        print("|---|" + "---|" * (len(FIELDS) + 2))
        for k in sorted(set(kp) & set(kb)):
            (p, isap), (b, isab) = kp[k], kb[k]
            same = all(p[f] == b[f] for f in FIELDS)
            bad |= not same
            cells = [b[f] if p[f] == b[f] else "%s -> %s" % (p[f], b[f]) for f in FIELDS]
            bad |= a.require_identical and isap != isab
            print("| `%s` | %s | %s | %s |" % (k, " | ".join(cells), "same" if same else "DIFFER", "identical" if isap == isab else "differs"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
