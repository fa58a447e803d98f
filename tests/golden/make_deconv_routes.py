"""Records tests/golden/deconv_routes.json from a tree whose libpybold_hip.so is built (no GPU needed):

    python tests/golden/make_deconv_routes.py [out.json]

The cases and the way a call is observed are those of tests/deconv_route_cases.py.  Record from the tree whose routing is
the contract -- the commit BEFORE a change to `deconv`, `deconv_auto` or the `force` switches -- and run it on the tree
after the change too: the two files must be byte-identical."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import deconv_route_cases as cases  # noqa: E402


def main(argv):
    out = argv[1] if len(argv) > 1 else os.path.join(HERE, "deconv_routes.json")
    rec = cases.record()
    with open(out, "w") as f:
        f.write("{\n")
        f.write('"case_list_sha256": %s,\n"n_cases": %d,\n' % (json.dumps(rec["case_list_sha256"]), rec["n_cases"]))
        f.write('"outcomes": [\n%s\n],\n' % ",\n".join(json.dumps(o) for o in rec["outcomes"]))
        f.write('"index": %s\n}\n' % json.dumps(rec["index"], separators=(",", ":")))
    print("%d cases, %d distinct outcomes, %d bytes -> %s" % (rec["n_cases"], len(rec["outcomes"]), os.path.getsize(out), out))


if __name__ == "__main__":
    main(sys.argv)
