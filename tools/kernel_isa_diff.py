#!/usr/bin/env python3
"""Did an edit change the machine code of a kernel it was not meant to touch?  CPU only: needs hipcc, no GPU.

  python tools/kernel_isa_diff.py <tree A> <tree B>     every kernel of every csrc/*.hip of A against the same kernel of B
  python tools/kernel_isa_diff.py --twins <tree>        passes.hip against passes_simple.hip of one tree: which ray kernels need their twin

A tree is a checkout of this repository (or its csrc directory); a directory that holds *.s files is taken as assembly already made
(--keep DIR leaves it there: compiling passes.hip takes minutes, so keep the parent's and pass the directory next time).  Each .hip file is
compiled with the command its Makefile prints for it, `-c` replaced by `--cuda-device-only -S` (the recipe of isa_by_function.py).  The
assembly is cut into kernels -- label to .Lfunc_end -- and what differs without meaning anything is dropped or renamed: comments, .loc /
.file / .cfi / debug directives, the numbers of local labels, the order of kernels within a file.  Per demangled kernel name:
  same | moved (file A -> file B), same | DIFFERS  (with both instruction counts and both kernel-descriptor rows)
Exit status 1 if a kernel differs, disappears or appears.
"""
import argparse
import concurrent.futures
import os
import re
import shlex
import subprocess
import sys
import tempfile

CSRC = os.path.join("sm64rt-legacy-renderer_amd", "csrc")
DESCRIPTOR = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")
MAX_JOBS = 16
DROPPED = (".loc", ".file", ".cfi_", ".cv_", ".ident", ".addrsig")
LOCAL_LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def compile_command(csrc, name):
    """The Makefile's own command for build/<name>.o (its per-object flags included), turned into a device-only -S run."""
    out = subprocess.run(["make", "-s", "-n", "-B", "build/%s.o" % name], cwd=csrc, check=True, capture_output=True, text=True).stdout
    line = next(l for l in out.splitlines() if " -c " in l and name + ".hip" in l)
    args = shlex.split(line)
    args = args[:args.index("-o")]
    args[args.index("-c")] = "-S"
    return args + ["--cuda-device-only"]


def assembly_of(tree, keep, jobs):
    """{file stem: assembly text} of a tree, or of a directory of *.s files."""
    tree = os.path.abspath(tree)
    listed = sorted(f for f in os.listdir(tree) if f.endswith(".s"))
    if listed:
        return {f[:-2]: open(os.path.join(tree, f), errors="replace").read() for f in listed}
    csrc = tree if os.path.exists(os.path.join(tree, "passes.hip")) else os.path.join(tree, CSRC)
    names = sorted(f[:-4] for f in os.listdir(csrc) if f.endswith(".hip"))
    outdir = os.path.abspath(keep) if keep else tempfile.mkdtemp(prefix="kernel_isa_")
    os.makedirs(outdir, exist_ok=True)

    def one(name):
        path = os.path.join(outdir, name + ".s")
        r = subprocess.run(compile_command(csrc, name) + ["-o", path], cwd=csrc, capture_output=True, text=True)
        if r.returncode:
            sys.exit("%s.hip of %s does not compile:\n%s" % (name, tree, r.stderr))
        return name, open(path, errors="replace").read()

    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as pool:
        return dict(pool.map(one, names))


def demangle(names):
    names = list(names)
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        return dict(zip(names, (o.replace("(anonymous namespace)::", "") for o in out)))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels_of(text):
    """{mangled name: (normalised body lines, instruction count, descriptor dict)}"""
    lines = text.splitlines()
    found, descriptor, current = {}, {}, None
    for l in lines:
        s = l.strip()
        if s.startswith(".amdhsa_kernel "):
            current = s.split()[1]
            descriptor[current] = {}
        elif s.startswith(".end_amdhsa_kernel"):
            current = None
        elif current and s.startswith(".amdhsa_"):
            key, _, value = s[len(".amdhsa_"):].partition(" ")
            descriptor[current][key] = value.strip()
    at = 0
    while at < len(lines):
        m = re.match(r"([A-Za-z_$][\w$.]*):", lines[at])
        if not m or m.group(1) not in descriptor:
            at += 1
            continue
        name, body, labels, count, in_text = m.group(1), [], {}, 0, True
        at += 1
        while at < len(lines) and not lines[at].startswith(".Lfunc_end"):
            s = " ".join(lines[at].split(";")[0].split())
            at += 1
            if s.startswith(".section"):           # the kernel descriptor sits in .rodata in front of .Lfunc_end: read above, no part of the code
                in_text = s.startswith(".section .text")
                continue
            if not s or not in_text or s.startswith(DROPPED):
                continue
            s = LOCAL_LABEL.sub(lambda k: labels.setdefault(k.group(0), ".L%d" % len(labels)), s)
            body.append(s)
            if not s.startswith(".") and not s.endswith(":"):
                count += 1
        found[name] = (body, count, descriptor[name])
    return found


def describe(entry):
    body, count, d = entry
    return "%6d instructions | " % count + "  ".join("%s %s" % (k, d.get(k, "-")) for k in DESCRIPTOR)


def load(tree, keep, jobs):
    per_file = {stem: kernels_of(text) for stem, text in assembly_of(tree, keep, jobs).items()}
    names = demangle({n for ks in per_file.values() for n in ks})
    return {stem: {names[n]: e for n, e in ks.items()} for stem, ks in per_file.items()}


def compare_trees(a, b):
    bad = moved = same = 0
    taken = set()                                  # (file, kernel) of B that some kernel of A was compared with
    rows = []
    for fa in sorted(a):
        for name in sorted(a[fa]):
            ea = a[fa][name]
            if name in b.get(fa, {}):
                fb = fa
            else:                                  # not where it was: the same kernel in another file, an identical copy first
                others = [f for f in sorted(b) if f != fa and name in b[f] and name not in a.get(f, {})]
                fb = next((f for f in others if b[f][name][0] == ea[0]), others[0] if others else None)
            if fb is None:
                rows.append("DISAPPEARED  %s.hip: %s\n      A: %s" % (fa, name, describe(ea)))
                bad += 1
                continue
            taken.add((fb, name))
            eb = b[fb][name]
            where = "" if fb == fa else "moved (%s.hip -> %s.hip), " % (fa, fb)
            if ea[0] == eb[0] and all(ea[2].get(k) == eb[2].get(k) for k in DESCRIPTOR):
                rows.append("%ssame  %s%s" % (where, "" if where else fa + ".hip: ", name))
                same += not where
                moved += bool(where)
            else:
                rows.append("%sDIFFERS  %s.hip: %s\n      A: %s\n      B: %s" % (where, fa, name, describe(ea), describe(eb)))
                bad += 1
    for fb in sorted(b):
        for name in sorted(b[fb]):
            if (fb, name) not in taken:
                rows.append("APPEARED  %s.hip: %s\n      B: %s" % (fb, name, describe(b[fb][name])))
                bad += 1
    print("\n".join(rows))
    print("%d kernels: %d same, %d moved and same, %d differ / appear / disappear" % (same + moved + bad, same, moved, bad))
    return 1 if bad else 0


def compare_twins(t):
    full, simple = t.get("passes", {}), t.get("passes_simple", {})
    identical = 0
    for name in sorted(set(full) | set(simple)):
        if name not in full or name not in simple:
            print("only in %s.hip  %s" % ("passes" if name in full else "passes_simple", name))
        elif full[name][0] == simple[name][0]:
            print("identical twins  %s" % name)
            identical += 1
        else:
            print("twins differ     %s   (%d / %d instructions)" % (name, full[name][1], simple[name][1]))
    print("%d kernels in passes.hip, %d in passes_simple.hip, %d identical in both" % (len(full), len(simple), identical))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("trees", nargs="+", help="two trees (or directories of *.s files); one with --twins")
    ap.add_argument("--twins", action="store_true", help="compare passes.hip with passes_simple.hip inside one tree")
    ap.add_argument("--keep", action="append", default=[], metavar="DIR", help="leave the assembly of the n-th tree in DIR (give it once per tree)")
    ap.add_argument("--jobs", type=int, default=min(MAX_JOBS, os.cpu_count() or 1), help="compile jobs at a time (at most %d)" % MAX_JOBS)
    o = ap.parse_args()
    if len(o.trees) != (1 if o.twins else 2):
        ap.error("--twins takes one tree, the comparison two")
    jobs = max(1, min(o.jobs, MAX_JOBS))
    loaded = [load(t, o.keep[k] if k < len(o.keep) else None, jobs) for k, t in enumerate(o.trees)]
    sys.exit(compare_twins(loaded[0]) if o.twins else compare_trees(loaded[0], loaded[1]))


if __name__ == "__main__":
    main()
