"""Per-kernel text comparison of two sets of hipcc --save-temps device .s files.

usage: python scripts/isa_compare.py --a OLD.s [OLD2.s ...] --b NEW.s [NEW2.s ...]

For moves of kernels between translation units: every kernel symbol of set A must be in set B
and the reverse, and per kernel the text from its label to .end_amdhsa_kernel (instructions and
the .amdhsa_* descriptor, the resource comments behind it) and its .amdgpu_metadata record must
be equal. The one normalisation: what is numbered per translation unit is rewritten away — the
function index in local labels (.LBB<n>_<m>, .Lfunc_end<n>, BB<n>_<m> in loop notes) and the
comments that only name an LLVM IR value ("; %Flow1033"); every other comment is compared, with
the blanks in front of it collapsed (its column follows the label's length). Functions that
are not kernels (device code that was not inlined) are listed. Exit status 0 when both sets
are equal and hold only kernels."""
import argparse
import difflib
import re
import sys

LOCAL = re.compile(r"(?<![A-Za-z0-9_])(\.LBB|BB|\.Lfunc_end|\.Lfunc_begin)\d+")


def norm(lines):
    out = []
    for l in lines:
        parts = l.split(";")
        code = parts[0].rstrip()
        # comments stay, except the names of LLVM IR values ("; %Flow1033", "; %.lr.ph25.i"), which
        # are numbered per module; the column a comment starts in follows the label's length
        coms = [c.strip() for c in parts[1:]]
        coms = [c for c in coms if not (c.startswith("%") and not c.startswith("%bb."))]
        if coms:
            code += (" ; " if code else "; ") + " ; ".join(coms)
        out.append(LOCAL.sub(r"\1", code))
    return out


def parse(path):
    text = open(path).read().split("\n")
    kernels, functions, meta = {}, set(), {}
    label = {}
    for i, l in enumerate(text):
        m = re.match(r"\s+\.type\s+(\S+),@function", l)
        if m:
            functions.add(m.group(1))
        elif l and not l[0].isspace() and l.split(":")[0] in functions and l.split(":")[0] not in label:
            label[l.split(":")[0]] = i
    i = 0
    while i < len(text):
        m = re.match(r"\s+\.amdhsa_kernel\s+(\S+)", text[i])
        if m:
            sym = m.group(1)
            end = i
            while not text[end].strip().startswith(".end_amdhsa_kernel"):
                end += 1
            kernels[sym] = norm(text[label[sym]:end + 1])
            i = end
        i += 1
    # metadata: the records of amdhsa.kernels, each a YAML list item at two spaces
    try:
        b = next(i for i, l in enumerate(text) if l.strip() == ".amdgpu_metadata")
        e = next(i for i in range(b, len(text)) if text[i].strip() == ".end_amdgpu_metadata")
    except StopIteration:
        return kernels, functions, meta
    rec = None
    for l in text[b:e]:
        if l.startswith("  - "):
            rec = []
            l = "    " + l[4:]
        elif not l.startswith("    "):
            rec = None
        if rec is not None:
            rec.append(l.rstrip())
            m = re.match(r"\s+\.name:\s+(\S+)", l)
            if m and l.startswith("    .name:"):
                meta[m.group(1)] = rec
    return kernels, functions, meta


def load(paths):
    K, F, M = {}, set(), {}
    for p in paths:
        k, f, m = parse(p)
        dup = set(k) & set(K)
        if dup:
            sys.exit("kernel defined twice: %s" % sorted(dup)[:3])
        K.update(k)
        F |= f
        M.update(m)
    return K, F, M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", nargs="+", required=True)
    ap.add_argument("--b", nargs="+", required=True)
    ap.add_argument("--diff-lines", type=int, default=40)
    a = ap.parse_args()
    (ka, fa, ma), (kb, fb, mb) = load(a.a), load(a.b)
    bad = 0
    for name, k, f in (("A", ka, fa), ("B", kb, fb)):
        extra = sorted(f - set(k))
        print("%s: %d kernels, %d functions that are not kernels" % (name, len(k), len(extra)))
        for s in extra:
            print("  not a kernel:", s)
        bad += len(extra)
    for s in sorted(set(ka) - set(kb)):
        print("only in A:", s)
        bad += 1
    for s in sorted(set(kb) - set(ka)):
        print("only in B:", s)
        bad += 1
    same = 0
    for s in sorted(set(ka) & set(kb)):
        d = []
        if ka[s] != kb[s]:
            d += list(difflib.unified_diff(ka[s], kb[s], "A", "B", lineterm="", n=2))
        if ma.get(s) != mb.get(s):
            d += list(difflib.unified_diff(ma.get(s, []), mb.get(s, []), "A metadata", "B metadata", lineterm="", n=2))
        if d:
            bad += 1
            print("DIFFERS:", s)
            print("\n".join(d[:a.diff_lines]))
        else:
            same += 1
    print("%d kernels identical (code, descriptor, metadata); %d problems" % (same, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
