#!/usr/bin/env python3
"""Per-kernel code identity between two builds of the HIP sources (host only: needs hipcc, no GPU).

    tools/kernel_code_diff.py --old DIR_OR_COMMIT --new DIR_OR_COMMIT [--old-sources a.hip ...] [--new-sources a.hip b.hip ...]

Each side is either a directory of gfx950 assembly files (`hipcc --cuda-device-only -S`, one `.s` per source), or a git
commit (or `WORKTREE` for the checked-out tree), of which the named sources under csrc/ are compiled to assembly with the
Makefile's flags.  For every kernel symbol (`.amdhsa_kernel`) of the union of a side's files it compares
  * the instruction stream: the assembly text of the function with comments dropped and the position-dependent part of local
    labels (`.LBB<n>_<m>`, `.Lfunc_end<n>`, `.Ltmp<n>`: numbered by position in the file) normalised;
  * the kernel descriptor: every `.amdhsa_*` directive (VGPR / AGPR / SGPR counts, LDS bytes, scratch bytes among them).
It reports missing, extra and duplicate symbols and every kernel that differs, with the register / LDS / scratch figures of
both sides, and exits non-zero unless the two sides hold the same kernels with identical code.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "randomly-projected-additive-gps_amd/csrc"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-result", "--cuda-device-only", "-S"]
LABEL = re.compile(r"\.L(BB|func_end|tmp|JTI)\d+")
FIGURES = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def assemble(commit, sources, out_dir):
    """Compile `sources` of `commit` (or the working tree) to device assembly in out_dir."""
    tree = ROOT
    if commit != "WORKTREE":
        tree = os.path.join(out_dir, "tree")
        os.makedirs(tree)
        tar = subprocess.run(["git", "-C", ROOT, "archive", commit, CSRC, "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tree], input=tar, check=True)
    procs = []
    for s in sources:
        out = os.path.join(out_dir, os.path.splitext(s)[0] + ".s")
        procs.append(subprocess.Popen([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + [s, "-o", out],
                                      cwd=os.path.join(tree, CSRC), stderr=subprocess.PIPE, text=True))
    for s, p in zip(sources, procs):
        err = p.communicate()[1]
        if p.returncode:
            sys.exit("compiling %s at %s failed:\n%s" % (s, commit, err))
    return out_dir


def kernels_of(path):
    """{symbol: (instruction lines, descriptor lines)} of one assembly file."""
    lines = open(path).read().split("\n")
    desc, body = {}, {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = i + 1
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                j += 1
            desc[m.group(1)] = [l.strip() for l in lines[i + 1:j]]
            i = j
        i += 1
    starts = {l.split(":")[0]: n for n, l in enumerate(lines) if l[:1] == "_" and ":" in l}
    for sym in desc:
        text = []
        for n in range(starts[sym] + 1, len(lines)):
            if re.match(r"\s*\.(section|amdhsa_kernel)\b", lines[n]):
                break
            l = LABEL.sub(lambda q: ".L" + q.group(1), lines[n].split(";")[0]).strip()
            if l:
                text.append(l)
        body[sym] = text
    return {s: (body[s], desc[s]) for s in desc}


def side(spec, sources, tmp, name):
    d = spec if os.path.isdir(spec) else assemble(spec, sources, os.path.join(tmp, name))
    if not os.path.isdir(spec):
        os.makedirs(d, exist_ok=True)
    all_k, count = {}, collections.Counter()
    for f in sorted(os.listdir(d)):
        if f.endswith(".s") and (not sources or os.path.splitext(f)[0] + ".hip" in sources):
            ks = kernels_of(os.path.join(d, f))
            print("  %s %-24s %4d kernels" % (name, f, len(ks)))
            count.update(ks.keys())
            all_k.update(ks)
    return all_k, [s for s, n in count.items() if n > 1]


def figures(desc):
    vals = dict(l.replace(".amdhsa_", "").split(None, 1) for l in desc)
    return " ".join("%s=%s" % (k, vals.get(k, "?")) for k in FIGURES)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old", required=True)
    ap.add_argument("--new", required=True)
    ap.add_argument("--old-sources", nargs="*", default=[])
    ap.add_argument("--new-sources", nargs="*", default=[])
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        for n in ("old", "new"):
            os.makedirs(os.path.join(tmp, n))
        old, dup_old = side(a.old, a.old_sources, tmp, "old")
        new, dup_new = side(a.new, a.new_sources, tmp, "new")
    missing = sorted(set(old) - set(new))
    extra = sorted(set(new) - set(old))
    changed = []
    for s in sorted(set(old) & set(new)):
        code, d = old[s][0] != new[s][0], old[s][1] != new[s][1]
        if code or d:
            changed.append(s)
            print("DIFFERS %s (%s)\n    old: %s\n    new: %s" % (s, " + ".join(["code"] * code + ["descriptor"] * d),
                                                                figures(old[s][1]), figures(new[s][1])))
    for tag, syms in (("MISSING", missing), ("EXTRA", extra), ("DUPLICATE in old", dup_old), ("DUPLICATE in new", dup_new)):
        for s in syms:
            print("%s %s" % (tag, s))
    print("kernels: old %d, new %d; missing %d, extra %d, duplicate %d, differing %d, identical %d"
          % (len(old), len(new), len(missing), len(extra), len(dup_old) + len(dup_new), len(changed),
             len(set(old) & set(new)) - len(changed)))
    ok = not (missing or extra or dup_old or dup_new or changed)
    print("RESULT: %s" % ("IDENTICAL" if ok else "NOT IDENTICAL"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
