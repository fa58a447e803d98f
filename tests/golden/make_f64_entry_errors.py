"""Records tests/golden/f64_entry_errors.json from a build of libpybold_hip.so:

    python tests/golden/make_f64_entry_errors.py path/to/libpybold_hip.so [out.json]

The cases are those of tests/f64_entry_cases.py; nothing here needs a GPU (every call is refused before a launch, or has a
zero count).  Record from the build whose answers are the contract -- the commit BEFORE a change to the entry points -- and
reword a message on purpose by editing its one line of the "messages" table."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import f64_entry_cases as cases  # noqa: E402


def main(argv):
    lib = cases.bind(argv[1])
    out = argv[2] if len(argv) > 2 else os.path.join(HERE, "f64_entry_errors.json")
    rec = cases.record(lib)
    with open(out, "w") as f:
        f.write("{\n")
        f.write('"case_list_sha256": %s,\n' % json.dumps(rec["case_list_sha256"]))
        f.write('"faults": {\n"messages": [\n%s\n],\n' % ",\n".join(json.dumps(m) for m in rec["faults"]["messages"]))
        f.write('"results": {\n%s\n}\n},\n' % ",\n".join(
            "%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in rec["faults"]["results"].items()))
        f.write('"queries": {\n%s\n}\n}\n' % ",\n".join(
            "%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in rec["queries"].items()))
    n = sum(len(v) for v in rec["faults"]["results"].values())
    print("%d fault cases, %d distinct answers, %d bytes -> %s" % (n, len(rec["faults"]["messages"]), os.path.getsize(out), out))


if __name__ == "__main__":
    main(sys.argv)
