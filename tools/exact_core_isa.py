"""Instruction-level comparison of the float64 register-resident kernels (pybold_amd/csrc/fista_exact*.h, fista_auto*.h)
between two builds, from the ISA listings `make build/<name>.s` leaves in pybold_amd/csrc/build
(hipcc for gfx950, no GPU needed):

    python tools/exact_core_isa.py <dir with the parent's *.s / *.res> <dir with this tree's> > profiles/<file>.txt
    python tools/exact_core_isa.py <parent's dir> <this tree's dir> exact_5_32 exactpp_10_32 autosplit_5_32 ...   (listings by name)

With no names: every listing of the family -- the sixteen object prefixes on the pairs of their exact*_table.inc, 24 listings
and 96 kernels (`python tools/exact_core_isa.py --names` prints them).

Per kernel: the resource report, the instruction count, the opcode histogram's differences, and whether the instruction
text is identical / identical up to register names / identical as a multiset (scheduling order only)."""
import collections
import os
import re
import sys


CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pybold_amd", "csrc")
# table -> (its macro, the object prefixes built on its pairs)
FAMILY = (("exact_table.inc", "PB_EXACT", ("exact", "auto", "exactpp", "autopp")),
          ("exact_split_table.inc", "PB_EXACT_SPLIT", ("exactsplit", "autosplit", "exactsplitpp", "autosplitpp")),
          ("exact_long_table.inc", "PB_EXACT_LONG", ("exactlong", "autolong", "exactlongpp", "autolongpp")),
          ("exact_split_long_table.inc", "PB_EXACT_SPLIT_LONG",
           ("exactsplitlong", "autosplitlong", "exactsplitlongpp", "autosplitlongpp")))


def family_listings():
    names = []
    for table, macro, prefixes in FAMILY:
        pairs = re.findall(r"^%s\((\d+), *(\d+)\)" % macro, open(os.path.join(CSRC, table)).read(), re.M)
        names += ["%s_%s_%s" % (p, s, kt) for s, kt in pairs for p in prefixes]
    return names


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
    if sys.argv[1:] == ["--names"]:
        print(" ".join(family_listings()))
        return
    old, new = sys.argv[1], sys.argv[2]
    names = sys.argv[3:]
    if names:
        print("tools/exact_core_isa.py: the kernels of %s of this tree against a build of the parent commit." % ", ".join(names))
    else:
        names = family_listings()
        print("tools/exact_core_isa.py: every kernel of the float64 register-resident family (%d listings) of this tree against a"
              % len(names))
        print("build of the parent commit.")
    print("hipcc for gfx950, no GPU.\n")
    tally = collections.Counter()
    for name in names:
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
                                                                 "Occupancy [waves/SIMD]", "VGPRs Spill",
                                                                 "LDS Size [bytes/block]"))
            short = re.sub(r"^_ZN2pb\d+", "", sym).split("EEv")[0]
            print("%s %s: %d -> %d instructions | %s | %s" % (name, short, len(a), len(b), res, verdict))
            tally[verdict.split(":")[0]] += 1
    print("\n%d kernels: %s" % (sum(tally.values()), ", ".join("%d %s" % (n, v) for v, n in tally.most_common())))


if __name__ == "__main__":
    main()
