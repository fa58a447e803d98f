"""CPU-only: the recorded routing of `deconv` and `deconv_auto` (tests/golden/deconv_routes.json, written by
tests/golden/make_deconv_routes.py from the tree before the engines, switches and wrappers were put behind one form table).
For every case of tests/deconv_route_cases.py -- every engine name and AUTO_LBDA value, the three opt-in switches off and on,
1-D and batch `y`, one HRF or one per voxel, on a grid around the limits of the four float64 forms -- the solver function the
call ends in and the `force` it passes, or the exception it answers with, and the warnings beside either: exact, texts
included."""
import json
import os

import pytest

from tests import deconv_route_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "deconv_routes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    _lib.load()


def test_the_case_list_is_the_recorded_one(golden):
    assert cases.case_list_hash() == golden["case_list_sha256"], "tests/deconv_route_cases.py drifted from the recording"
    assert len(cases.cases()) == golden["n_cases"] == len(golden["index"]) and golden["n_cases"] >= 2000


def test_every_outcome_class_is_in_the_recording(golden):
    seen = [golden["outcomes"][i] for i in sorted(set(golden["index"]))]
    assert len(seen) == len(golden["outcomes"])
    reached = set(o[0] for o in seen)
    assert reached == set(cases.SEARCHES + cases.SOLVES + (None,))
    assert set(o[1] for o in seen if o[0] in cases.SOLVES) == {None, "split", "long_hrf", "split_long_hrf"}
    assert all(o[1] is None for o in seen if o[0] in cases.SEARCHES)
    assert all((o[0] is None) != (o[2] is None) for o in seen)          # a function reached, or an exception: never neither
    errors = [o[2] for o in seen if o[2]]
    for words in ("ValueError: deconv_auto: engine must be 'auto', 'device', 'host', 'device_split', 'device_split_pp', "
                  "'device_split_long_hrf' or 'device_long_hrf', got 'device_pp'",
                  "ValueError: deconv_auto(engine='device'): the device-resident lambda search carries series of up to 640 scans",
                  "ValueError: deconv_auto(engine='device_split'): the four-wave device-resident lambda search takes one HRF",
                  "ValueError: deconv_auto(engine='device_split'): the four-wave device-resident lambda search carries series",
                  "ValueError: deconv_auto(engine='device_split_pp'): the four-wave device-resident lambda search with one HRF",
                  "ValueError: deconv_auto(engine='device_split_pp'): the four-wave device-resident lambda search carries",
                  "ValueError: deconv_auto(engine='device_long_hrf'): the device-resident lambda search for long HRFs carries",
                  "ValueError: deconv_auto(engine='device_split_long_hrf'): the four-wave device-resident lambda search for long"):
        assert any(e.startswith(words) for e in errors), words
    warned = [o for o in seen if o[3]]
    assert warned and all(len(o[3]) == 1 and o[0] in ("fista_solve", "fista_solve_pp_d") for o in warned)
    assert all(o[3][0].startswith("RuntimeWarning: deconv_auto: the device-resident lambda search carries series of up to 640 "
                                  "scans") and o[3][0].endswith(": running the host loop. [deconv_route_cases.py]") for o in warned)


def test_every_call_goes_where_it_went(built, golden):
    wrong = []
    with cases.patched() as bold_signal:
        for case, i in zip(cases.cases(), golden["index"]):
            got = cases.run_case(bold_signal, case)
            if got != golden["outcomes"][i]:
                wrong.append((case, got, golden["outcomes"][i]))
    assert not wrong, "%d calls end otherwise than recorded, the first: %r" % (len(wrong), wrong[0])


def test_the_observation_leaves_the_modules_as_they_were(built):
    from pybold_amd import bold_signal, solver
    before = [(m, n, getattr(m, n)) for m in (solver, bold_signal) for n in dir(m) if not n.startswith("__")]
    with cases.patched():
        pass
    assert all(getattr(m, n) is v for m, n, v in before)
