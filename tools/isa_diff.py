"""Compare the matrix-pipe objects of two builds kernel by kernel: what a refactor of csrc/mfma_core.h and the three
kernel headers owes (the objects are disassembled as tools/isa_spill_lint.py does, the resource reports are the
`build/mfma*.res` files the compile leaves beside them).

    python tools/isa_diff.py <build dir of the parent> <build dir of this tree> [object names ...]

Per kernel symbol:
  tier 1 (must hold): same symbols, resource report equal field by field (registers, scratch, LDS, occupancy), equal
          counts of matrix, barrier, LDS and global/buffer/flat memory instructions;
  tier 2: identical instruction text;
  tier 3: anything else that keeps tier 1 -- the counts of the instructions that moved are printed.
Exit code 1 if tier 1 fails anywhere."""
import collections
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_spill_lint import listing  # noqa: E402

WORK = (("mfma", r"v_mfma"), ("barrier", r"s_barrier"), ("lds", r"ds_"), ("mem", r"global_|buffer_|flat_"))


def kernels(obj):
    """{symbol: [instruction text, ...]} of an object file (addresses, encodings and labels dropped)."""
    out, cur = {}, None
    for line in listing(obj):
        s = line.strip()
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", s)
        if m:
            cur = out.setdefault(m.group(1), []) if m.group(1).startswith("_ZN2pb") else None
            continue
        if cur is None or not s or s.startswith("<") or re.match(r"^[0-9a-f]+ <", s):
            continue
        cur.append(re.sub(r"\s+", " ", s.split("//")[0]).strip())
    return out


def resources(res):
    """{symbol: {field: value}} of a kernel-resource-usage report."""
    out, cur = {}, None
    for line in open(res):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def main():
    old, new = sys.argv[1], sys.argv[2]
    names = sys.argv[3:] or sorted(os.path.basename(f) for f in glob.glob(os.path.join(new, "mfma*.o")))
    fails, tiers = 0, collections.Counter()
    for name in names:
        ko, kn = kernels(os.path.join(old, name)), kernels(os.path.join(new, name))
        ro, rn = (resources(os.path.join(d, name[:-2] + ".res")) for d in (old, new))
        if set(ko) != set(kn) or set(ro) != set(rn):
            fails += 1
            print("%s: TIER 1 FAILS: kernel symbols differ: %s" % (name, sorted(set(ko) ^ set(kn)) or sorted(set(ro) ^ set(rn))))
            continue
        for k in sorted(kn):
            ho, hn = (collections.Counter(i.split(" ")[0] for i in t[k]) for t in (ko, kn))
            work = ["%s %d" % (w, sum(c for op, c in hn.items() if re.match(rx, op))) for w, rx in WORK]
            bad = [f for f in rn[k] if ro[k].get(f) != rn[k][f]]
            bad += [w for w, rx in WORK if sum(c for op, c in ho.items() if re.match(rx, op)) != sum(c for op, c in hn.items() if re.match(rx, op))]
            res = "vgpr %s agpr %s sgpr %s scratch %s lds %s occ %s" % tuple(rn[k].get(f, "?") for f in (
                "VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"))
            if bad:
                fails += 1
                tier = "TIER 1 FAILS (%s)" % ", ".join(bad)
            elif ko[k] == kn[k]:
                tier = "tier 2"
            else:
                moved = ["%s %+d" % (op, hn[op] - ho[op]) for op in sorted(set(ho) | set(hn)) if ho[op] != hn[op]]
                tier = "tier 3 (%d -> %d instructions; %s)" % (len(ko[k]), len(kn[k]), ", ".join(moved) or "same opcode histogram")
            tiers[tier.split(" (")[0]] += 1
            print("%s %s: %s | %s | %s | %d instructions" % (name, k, tier, res, ", ".join(work), len(kn[k])))
    print("%d kernels: %s" % (sum(tiers.values()), ", ".join("%s: %d" % kv for kv in sorted(tiers.items()))))
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
