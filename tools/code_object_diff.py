"""Compare the gfx950 device code of object files kernel by kernel: the check that a refactor of host code, or a
move of kernels between translation units, left the generated code alone.

    python tools/code_object_diff.py [--rename REGEX REPL] OLD.o NEW.o [NEW2.o ...]   # exit 1 if a shared kernel differs

Kernels are matched by demangled name (a per-unit ".intern." / "__intern__" hash suffix stripped) between OLD and
the union of the NEW objects.  For every kernel on both sides the instruction streams (mnemonic, operands and
encoding words; the instruction's own address and the "<symbol+offset>" note of a branch are dropped) and the
resources of the code object's metadata (VGPRs, AGPRs, SGPRs, LDS, scratch, spills) must be identical.  Kernels on
one side only are listed.  --rename rewrites OLD's demangled names first (re.sub), for a kernel whose template
parameter list changed: --rename 'branch_merge_v2_kernel<(.*), 1>' 'branch_merge_v2_kernel<\\1>'.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
RES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
       ".vgpr_spill_count", ".sgpr_spill_count")


def _run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def _demangle(names):
    plain = [re.sub(r"(\.intern\.|__intern__)[0-9a-f]+", "", n) for n in names]
    filt = next((f for f in (os.path.join(LLVM, "llvm-cxxfilt"), shutil.which("c++filt")) if f and os.path.exists(f)), None)
    if filt is None:
        return dict(zip(names, plain))          # mangled names still match one to one
    out = subprocess.run([filt], input="\n".join(plain), check=True, capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels(obj):
    """{demangled kernel name: (resources dict, [instruction lines])} of the gfx950 code object inside obj."""
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, os.path.basename(obj))
        with open(obj, "rb") as src, open(local, "wb") as dst:
            dst.write(src.read())
        _run(os.path.join(LLVM, "llvm-objdump"), "--offloading", local, cwd=tmp)
        cos = [os.path.join(tmp, f) for f in sorted(os.listdir(tmp)) if f.endswith("gfx950")]
        if len(cos) != 1:
            raise SystemExit("%s: expected one gfx950 code object, found %d" % (obj, len(cos)))
        notes = _run(os.path.join(LLVM, "llvm-readelf"), "--notes", cos[0])
        dis = _run(os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", cos[0])
    res = {}
    for chunk in re.split(r"\n  - ", notes.split("amdhsa.kernels:")[1].split("\namdhsa.target")[0]):
        m = re.search(r"^\s+\.name:\s+(\S+)$", chunk, re.M)
        vals = {k: re.search(r"^\s*\%s:\s+(\S+)$" % re.escape(k), chunk, re.M) for k in RES}
        if m:
            res[m.group(1)] = {k: v.group(1) for k, v in vals.items() if v}
    code, cur = {}, None
    for line in dis.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = code.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t") and line.strip() != "...":   # (elided zero padding)
            text, _, enc = line.partition("//")
            enc = re.sub(r"<[^>]*>", "", enc.split(":", 1)[-1])
            cur.append(text.strip() + "  ; " + " ".join(enc.split()))
    names = _demangle(list(res))
    return {names[n]: (res[n], code.get(n, [])) for n in res}


def main(argv):
    rename = None
    if len(argv) > 3 and argv[1] == "--rename":
        rename, argv = (argv[2], argv[3]), argv[:1] + argv[4:]
    if len(argv) < 3:
        print(__doc__)
        return 2
    old, new = kernels(argv[1]), {}
    if rename:
        old = {re.sub(rename[0], rename[1], n): k for n, k in old.items()}
    for path in argv[2:]:
        for name, k in kernels(path).items():
            if name in new:
                raise SystemExit("kernel %s is in two of the new objects" % name)
            new[name] = k
    bad = 0
    for name in sorted(set(old) & set(new)):
        (r0, c0), (r1, c1) = old[name], new[name]
        if r0 != r1:
            bad += 1
            print("RESOURCES DIFFER  %s\n    old %s\n    new %s" % (name, r0, r1))
        if c0 != c1:
            bad += 1
            at = next((i for i, (x, y) in enumerate(zip(c0, c1)) if x != y), min(len(c0), len(c1)))
            print("CODE DIFFERS  %s: %d vs %d instructions, first at #%d\n    old %s\n    new %s" % (
                name, len(c0), len(c1), at, c0[at:at + 1], c1[at:at + 1]))
    shared = len(set(old) & set(new))
    print("%d kernels on both sides: %d identical in code and resources, %d differences" % (
        shared, shared - len({n for n in set(old) & set(new) if old[n] != new[n]}), bad))
    for title, only in (("only in the old object", set(old) - set(new)), ("only in the new objects", set(new) - set(old))):
        print("%d kernels %s" % (len(only), title))
        for name in sorted(only):
            print("    " + name)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
