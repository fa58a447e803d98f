"""CPU-only: the recorded contract of the float64 register family's entry points (tests/golden/f64_entry_errors.json, written by
tests/golden/make_f64_entry_errors.py from the build before the entry points were put behind one form table).  For every
call the library refuses -- eighteen call families, every single fault, every pair of faults, every fault beside P == 0 /
V == 0 -- the return code and the text of pb_last_error(); the pairs pin which check fires first, the zero counts which
checks precede the no-op.  For the family's queries, every answer on a grid around the limits of the four forms."""
import json
import os

import pytest

from tests import f64_entry_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    _lib.load()
    return cases.bind(_lib.LIB_PATH)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "f64_entry_errors.json")) as f:
        return json.load(f)


def test_the_case_list_is_the_recorded_one(golden):
    assert cases.case_list_hash() == golden["case_list_sha256"], "tests/f64_entry_cases.py drifted from the recording"
    assert len(cases.families()) == 18
    for name, over in cases.cases():                       # a fault, or no problems: nothing may reach a device
        assert over, name


def test_refused_calls_answer_as_recorded(lib, golden):
    fam = cases.families()
    table = golden["faults"]["messages"]
    seen = dict((name, 0) for name in fam)
    wrong = []
    for name, over in cases.cases():
        entry, kind, base = fam[name][:3]
        want_rc, want_msg = table[golden["faults"]["results"][name][seen[name]]]
        seen[name] += 1
        rc, msg, count = cases.call(lib, entry, kind, base, over)
        assert rc == -1 or (rc == 0 and count == 0), "%s %r passed validation with %d problems" % (name, over, count)
        if rc != want_rc or (rc != 0 and msg != want_msg.replace("@", entry, 1)):
            wrong.append((name, over, (rc, msg), (want_rc, want_msg)))
    assert not wrong, "%d calls answer otherwise than recorded, the first: %r" % (len(wrong), wrong[0])
    assert all(seen[name] == len(golden["faults"]["results"][name]) for name in fam)
    assert sum(seen.values()) >= 3000


def test_queries_answer_as_recorded(lib, golden):
    points = 0
    for name in cases.QUERIES_4 + cases.QUERIES_WHICH + cases.QUERIES_3:
        rec = golden["queries"][name]
        at = iter(rec["at"])
        for N in cases.GRID_N:
            for K in cases.GRID_K:
                want = rec["blocks"][next(at)]
                assert cases.query_block(lib, name, N, K) == want, (name, N, K)
                points += len(want)
    assert [lib.pb_auto_lbda_work_len(V) for V in cases.GRID_V] == golden["queries"]["pb_auto_lbda_work_len"]
    assert points >= 9000
