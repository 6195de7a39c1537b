#!/usr/bin/env python3
"""Are two versions of the library the same device code?  No GPU needed.

    tools/isa_diff.py <tree or directory of .s files> <tree or directory of .s files> [--jobs N] [--keep DIR] [--pair OLD=NEW]...

For a source tree, every file of csrc/Makefile's SRCS is compiled with the Makefile's flags plus `--offload-device-only -S`.
Functions are paired by DEMANGLED name with namespace qualifiers dropped (moving a tag type such as BF16 out of an anonymous
namespace renames every kernel instantiated on it and changes nothing else); comments, the `__hip_cuid_<hash of the source>`
lines and the function numbers inside local labels are dropped.  Per file: `identical`, or the first function that differs;
then, per kernel, the resource numbers of the code-object metadata on both sides (`a|b`, marked where they differ; `-`: the
kernel exists on one side only -- the functions both sides have are compared all the same).  A kernel that was renamed on
purpose is paired by hand: `--pair OLD=NEW` compares a's OLD with b's NEW, body and resource row, as if it had that name (plain
demangled names as the report prints them, or an unambiguous part of one); the report lists the pairs it applied, and a pair
that matches nothing is an error.
Text and numbers only.  Exit status 1 if anything differs.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join("peclr_amd", "csrc")
RESOURCES = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
             ".vgpr_spill_count", ".sgpr_spill_count")
MANGLED = re.compile(r"\b_Z\w+")


def makefile_vars(path):
    out = {}
    for line in open(path):
        m = re.match(r"(\w+)\s*[:?]?=\s*(.*)", line)
        if m:
            out[m.group(1)] = re.sub(r"\$\((\w+)\)", lambda v: out.get(v.group(1), ""), m.group(2).strip())
    return out


def compile_tree(tree, outdir, jobs):
    mk = makefile_vars(os.path.join(tree, CSRC, "Makefile"))
    def one(src):
        dst = os.path.join(outdir, src[:-4] + ".s")
        cmd = [mk["HIPCC"], *mk["FLAGS"].split(), "--offload-device-only", "-S", src, "-o", dst]
        r = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
        if r.returncode:
            sys.exit("%s: %s\n%s" % (tree, " ".join(cmd), r.stderr))
    with ThreadPoolExecutor(jobs) as pool:
        list(pool.map(one, mk["SRCS"].split()))


def cxxfilt(symbols):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    out = subprocess.run([tool], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout
    return dict(zip(symbols, out.splitlines()))


def plain_name(demangled):
    """Demangled name without namespace qualifiers: `void peclr::(anonymous namespace)::k<peclr::BF16>(...)` -> `void k<BF16>(...)`."""
    return re.sub(r"(\(anonymous namespace\)|\w+)::", "", demangled)


def parse(text, demangle=cxxfilt):
    """Assembly text -> ({function name: normalised body}, {kernel name: {resource: value}}), names as plain_name gives them."""
    text = "".join(l for l in text.splitlines(True) if "__hip_cuid_" not in l)
    names = {s: plain_name(d) for s, d in demangle(sorted(set(MANGLED.findall(text)))).items()}
    named = MANGLED.sub(lambda m: names[m.group(0)], text)
    funcs = {}
    for m in re.finditer(r"; -- Begin function ([^\n]*)\n(.*?); -- End function", named, re.S):
        body = re.sub(r"[ \t]*;.*", "", m.group(2))                       # comments (inline assembly here holds no `;`)
        body = re.sub(r"(\bBB|\.LBB|\.Lfunc_end)\d+", r"\1", body)          # the function's number inside local labels
        funcs[m.group(1).strip()] = body
    res = {}
    meta = text[text.find(".amdgpu_metadata"):]
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", entry)
        if name:
            res[names.get(name.group(1), name.group(1))] = {
                k: int(re.search(r"\n    \%s:\s+(\d+)" % k, "\n" + entry).group(1)) for k in RESOURCES}
    return funcs, res


def resolve(want, names, side):
    """The one name of `names` that is `want` or, failing that, contains it (None: there is none)."""
    hits = [n for n in names if n == want] or sorted(n for n in names if want in n)
    if len(hits) > 1:
        raise ValueError("--pair: %r is ambiguous in %s: %s" % (want, side, hits))
    return hits[0] if hits else None


def apply_pairs(fa, ra, fb, rb, pairs):
    """Gives a's function and resource row OLD the name of b's NEW for every (OLD, NEW) of `pairs` -> {pair applied: its report
    line}.  A pair that neither side has is left alone (another file's); one that a single side has is an error."""
    lines = {}
    for old, new in pairs:
        x, y = resolve(old, set(fa) | set(ra), "a"), resolve(new, set(fb) | set(rb), "b")
        if (x is None) != (y is None):
            raise ValueError("--pair %s=%s: %s" % (old, new, "a has no such function" if x is None else "b has no such function"))
        if x is None:
            continue
        if x != y and (y in fa or y in ra):
            raise ValueError("--pair %s=%s: a has %r as well" % (old, new, y))
        if x in fa:
            fa[y] = fa.pop(x).replace(x, y)                                 # (its own name: labels, .size, its LDS symbol)
        if x in ra:
            ra[y] = ra.pop(x)
        lines[(old, new)] = "  paired: a's %s = b's %s" % (x, y)
    return lines


def compare(a_text, b_text, demangle=cxxfilt, pairs=(), applied=None):
    """-> (verdict line, table rows, same?).  pairs: (OLD, NEW) names, a's OLD is compared with b's NEW as if it had that name;
    applied: a set that collects the pairs used here -- without one, a pair that matches nothing is an error."""
    (fa, ra), (fb, rb) = parse(a_text, demangle), parse(b_text, demangle)
    paired = apply_pairs(fa, ra, fb, rb, pairs)
    if applied is not None:
        applied.update(paired)
    elif len(paired) != len(pairs):
        raise ValueError("--pair: no such function on either side: %s" % ["%s=%s" % p for p in pairs if p not in paired])
    verdict = "identical (%d functions, %d kernels)" % (len(fa), len(ra))
    common = [name for name in fa if name in fb]
    changed = None
    for name in common:
        if fa[name] != fb[name]:
            la, lb = fa[name].splitlines(), fb[name].splitlines()
            at = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            changed = "DIFFERENT: %s, line %d of %d|%d:\n    a: %s\n    b: %s" % (
                name, at, len(la), len(lb), la[at].strip() if at < len(la) else "<end>", lb[at].strip() if at < len(lb) else "<end>")
            break
    if sorted(fa) != sorted(fb) or sorted(ra) != sorted(rb):
        # (a side that adds or drops functions: the ones both sides have are still compared, so that "N new kernels, every old
        # one untouched" can be read off the report)
        verdict = "DIFFERENT function lists: only in a %s, only in b %s\n  the %d functions both sides have: %s" % (
            sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa)), len(common), changed or "identical")
    elif changed:
        verdict = changed
    rows, same = list(paired.values()), verdict.startswith("identical")
    for name in sorted(set(ra) | set(rb)):
        x, y = ra.get(name), rb.get(name)
        cells = ["%s|%s" % (x[k] if x else "-", y[k] if y else "-") for k in RESOURCES]
        rows.append("  %s %s  %s" % ("  " if x == y else "!=", " ".join("%11s" % c for c in cells), name))
        same = same and x == y
    return verdict, rows, same


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", help="directory that keeps the .s files (a/ and b/); default: a temporary one")
    ap.add_argument("--pair", action="append", default=[], metavar="OLD=NEW",
                    help="compare a's function OLD with b's NEW (demangled names as the report prints them, or an unambiguous part)")
    args = ap.parse_args()
    pairs, applied = [tuple(p.split("=", 1)) for p in args.pair], set()
    if any(len(p) != 2 or not all(p) for p in pairs):
        ap.error("--pair takes OLD=NEW")
    keep = args.keep or tempfile.mkdtemp(prefix="isa_diff_")
    dirs = []
    for side, path in (("a", args.a), ("b", args.b)):
        if os.path.exists(os.path.join(path, CSRC, "Makefile")):
            out = os.path.join(keep, side)
            os.makedirs(out, exist_ok=True)
            compile_tree(path, out, args.jobs)
            path = out
        dirs.append(path)
    files = sorted(f for f in os.listdir(dirs[0]) if f.endswith(".s"))
    all_same = files == sorted(f for f in os.listdir(dirs[1]) if f.endswith(".s"))
    if not all_same:
        print("DIFFERENT file lists")
    print("resource columns (a|b): " + " ".join(k.lstrip(".") for k in RESOURCES))
    for f in files:
        if not os.path.exists(os.path.join(dirs[1], f)):
            continue
        try:
            verdict, rows, same = compare(*(open(os.path.join(d, f)).read() for d in dirs), pairs=pairs, applied=applied)
        except ValueError as e:
            sys.exit("%s: %s" % (f[:-2] + ".hip", e))
        print("%s: %s" % (f[:-2] + ".hip", verdict))
        print("\n".join(rows)) if rows else None
        all_same = all_same and same
    if not args.keep:
        shutil.rmtree(keep)
    if set(pairs) - applied:
        sys.exit("--pair: no such function in any file: %s" % sorted("%s=%s" % p for p in set(pairs) - applied))
    print("ALL IDENTICAL" if all_same else "DIFFERENCES FOUND")
    return 0 if all_same else 1


if __name__ == "__main__":
    sys.exit(main())
