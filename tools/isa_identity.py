"""Did a change to csrc/ change the generated code?  tools/isa_identity.py <tree A> <tree B> [--show]
Compiles every csrc/*.hip of both source trees to gfx950 assembly with the build's own flags (_build.FLAGS + _build.EXTRA, device side only),
cuts out every kernel's instruction stream and kernel descriptor, strips comments, normalises the function-local label numbers and compares
hashes by kernel name.  Prints the copy counts and the kernels that are new, gone or different (--show: a unified diff of the different ones).
A kernel that several units emit (a `static __global__` in a header) counts as unchanged when every copy in B equals some copy in A; the
units of A that hold the matching copy are printed.  Needs hipcc, no GPU.  Exit status 1 when anything is new, gone or different."""
import argparse
import difflib
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diverse_channel_vit_amd import _build  # noqa: E402

LABEL = re.compile(r"\.(LBB|Lfunc_end|Ltmp)\d+")


def kernels_of(src):
    """{kernel name: normalised text of its body + descriptor} of one translation unit"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        cmd = [_build.HIPCC] + _build.FLAGS + _build.EXTRA.get(os.path.basename(src), []) + ["--cuda-device-only", "-S", src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"hipcc failed for {src}:\n{r.stderr}")
        lines = [LABEL.sub(r".\1", ln.split(";")[0].rstrip()) for ln in open(out)]
    lines = [ln for ln in lines if ln.strip()]
    found = {}
    for name in [ln.split()[1] for ln in lines if ln.lstrip().startswith(".amdhsa_kernel ")]:
        body = lines[lines.index(name + ":"):]
        body = body[:next(i for i, ln in enumerate(body) if ln.startswith(".Lfunc_end")) + 1]
        desc = lines[lines.index("\t.amdhsa_kernel " + name):]
        desc = desc[:desc.index("\t.end_amdhsa_kernel") + 1]
        found[name] = "\n".join(body + desc)
    return found


def tree(root):
    """{kernel name: [(unit, text), ...]} of all units under root"""
    csrc = os.path.join(root, "diverse_channel_vit_amd", "csrc")
    units = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    with ThreadPoolExecutor(max_workers=8) as ex:
        per_unit = list(ex.map(lambda u: kernels_of(os.path.join(csrc, u)), units))
    table = {}
    for unit, found in zip(units, per_unit):
        for name, text in found.items():
            table.setdefault(name, []).append((unit, text))
    return table


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--show", action="store_true", help="print a unified diff of every kernel that differs")
    args = ap.parse_args()
    A, B = tree(args.a), tree(args.b)
    digest = lambda t: hashlib.sha256(t.encode()).hexdigest()
    for tag, T in (("A", A), ("B", B)):
        print(f"{tag}: {len(T)} kernel names, {sum(len(c) for c in T.values())} copies")
    new, gone, differ = sorted(set(B) - set(A)), sorted(set(A) - set(B)), []
    for name in sorted(set(A) & set(B)):
        in_a = {}
        for unit, text in A[name]:
            in_a.setdefault(digest(text), []).append(unit)
        if any(digest(text) not in in_a for _, text in B[name]):
            differ.append(name)
        elif len(in_a) > 1:
            print(f"{name}: {len(A[name])} copies in A with {len(in_a)} distinct bodies; B's equals that of", *in_a[digest(B[name][0][1])])
    for tag, names in (("new", new), ("gone", gone), ("different", differ)):
        print(f"{tag}: {len(names)}", *names)
    if args.show:
        for name in differ:
            (ua, ta), (ub, tb) = A[name][-1], B[name][-1]
            print("\n".join(difflib.unified_diff(ta.split("\n"), tb.split("\n"), f"A/{ua}:{name}", f"B/{ub}:{name}", lineterm="", n=2)))
    return 1 if new or gone or differ else 0


if __name__ == "__main__":
    sys.exit(main())
