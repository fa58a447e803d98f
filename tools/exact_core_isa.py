"""Instruction-count comparison of fista_exact_kernel (and, where both builds have its listings, auto_lbda_kernel) between two
builds, from the ISA listings `make build/exact_5_32.s build/exact_10_32.s [build/auto_5_32.s build/auto_10_32.s]` leaves in
pybold_amd/csrc/build (hipcc for gfx950, no GPU needed):

    python tools/exact_core_isa.py <dir with the parent's exact_*.s / .res> <dir with this tree's> > profiles/exact_core_isa.txt
    python tools/exact_core_isa.py <parent's dir> <this tree's dir> exact_5_32 exactpp_10_32 autosplit_5_32 ...   (listings by name)

Per kernel: the resource report, the instruction count, the opcode histogram's differences, and whether the instruction
text is identical / identical up to register names / identical as a multiset (scheduling order only)."""
import collections
import os
import re
import sys


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        s = line.split(";")[0].strip()
        m = re.match(r"^(_ZN2pb\w+):", s)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
        if cur is None or not s or s.startswith(".") or s.endswith(":"):
            continue
        cur.append(re.sub(r"\s+", " ", s))
    return out


def resources(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass", line)
        if m and m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def anonymise(ins):
    return re.sub(r"\b[vsa]\[?\d+(:\d+)?\]?", "R", ins)


def main():
    old, new = sys.argv[1], sys.argv[2]
    names = sys.argv[3:]
    if names:
        print("tools/exact_core_isa.py: the kernels of %s of this tree against a build of the parent commit." % ", ".join(names))
        print("hipcc for gfx950, no GPU.\n")
    else:
        print("tools/exact_core_isa.py: fista_exact_kernel of this tree (pass body in exact_forward / exact_backward, shared with")
        print("auto_lbda_kernel) against a build of the parent commit.  hipcc for gfx950, no GPU.\n")
    for name in names or ("exact_5_32", "exact_10_32", "auto_5_32", "auto_10_32"):
        if name.startswith("auto") and not all(os.path.exists(os.path.join(d, name + ".s")) for d in (old, new)):
            continue
        ko, kn = kernels(os.path.join(old, name + ".s")), kernels(os.path.join(new, name + ".s"))
        ro, rn = resources(os.path.join(old, name + ".res")), resources(os.path.join(new, name + ".res"))
        assert sorted(ko) == sorted(kn), "symbols differ"
        for sym in sorted(kn):
            a, b = ko[sym], kn[sym]
            if a == b:
                verdict = "identical instruction text"
            elif [anonymise(i) for i in a] == [anonymise(i) for i in b]:
                verdict = "identical up to register names"
            elif collections.Counter(anonymise(i) for i in a) == collections.Counter(anonymise(i) for i in b):
                verdict = "same instructions, other order / registers"
            else:
                ha, hb = (collections.Counter(i.split(" ")[0] for i in x) for x in (a, b))
                moved = {k: hb[k] - ha[k] for k in sorted(set(ha) | set(hb)) if ha[k] != hb[k]}
                verdict = "differs: " + ", ".join("%s %+d" % kv for kv in moved.items())
            res = " ".join("%s %s->%s" % (k, ro[sym].get(k), v) if ro[sym].get(k) != v else "%s %s" % (k, v)
                           for k, v in rn[sym].items() if k in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]",
                                                                 "Occupancy [waves/SIMD]"))
            short = re.sub(r"^_ZN2pb\d+", "", sym).split("EEv")[0]
            print("%s %s: %d -> %d instructions | %s | %s" % (name, short, len(a), len(b), res, verdict))


if __name__ == "__main__":
    main()
