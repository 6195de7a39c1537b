#!/usr/bin/env python3
"""Are two versions of the library the same device code?  No GPU needed.

    tools/isa_diff.py <tree or directory of .s files> <tree or directory of .s files> [--jobs N] [--keep DIR]

For a source tree, every file of csrc/Makefile's SRCS is compiled with the Makefile's flags plus `--offload-device-only -S`.
Functions are paired by DEMANGLED name with namespace qualifiers dropped (moving a tag type such as BF16 out of an anonymous
namespace renames every kernel instantiated on it and changes nothing else); comments, the `__hip_cuid_<hash of the source>`
lines and the function numbers inside local labels are dropped.  Per file: `identical`, or the first function that differs;
then, per kernel, the resource numbers of the code-object metadata on both sides (`a|b`, marked where they differ; `-`: the
kernel exists on one side only -- the functions both sides have are compared all the same).
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


def compare(a_text, b_text, demangle=cxxfilt):
    """-> (verdict line, table rows, same?)"""
    (fa, ra), (fb, rb) = parse(a_text, demangle), parse(b_text, demangle)
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
    rows, same = [], verdict.startswith("identical")
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
    args = ap.parse_args()
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
        verdict, rows, same = compare(*(open(os.path.join(d, f)).read() for d in dirs))
        print("%s: %s" % (f[:-2] + ".hip", verdict))
        print("\n".join(rows)) if rows else None
        all_same = all_same and same
    if not args.keep:
        shutil.rmtree(keep)
    print("ALL IDENTICAL" if all_same else "DIFFERENCES FOUND")
    return 0 if all_same else 1


if __name__ == "__main__":
    sys.exit(main())
