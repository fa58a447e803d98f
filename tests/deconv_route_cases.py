"""The calls behind tests/golden/deconv_routes.json: where `deconv` and `deconv_auto` send a call -- which solver function,
with which `force` -- or what they refuse it with, observed without a GPU.  A plain helper module: the recorder
(tests/golden/make_deconv_routes.py) and the replay (tests/test_deconv_routes_host.py) both build and run their calls here.

How a call is observed (`patched`): `solver.device` answers the CPU, the two step estimates are constants, and every solver
function a route can end in -- the eight `solver.auto_lbda_solve*`, `solver.fista_solve`, `solver.fista_solve_pp_d` -- raises a
sentinel that carries its name and its `force` keyword.  Only public names and the private ones the tests already use are
replaced, so the same module runs on the tree before and after a change to the routing.  A call then ends in the sentinel or
in an exception of its own, with or without `warn_once` warnings (`solver._warned` is cleared before every call)."""
import contextlib
import hashlib
import itertools
import json
import os
import warnings

import numpy as np
import torch

# around the limits of the four forms: 640 / 1280 scans, 32 / 48 taps, wind = 6 (64 scans: the host loop's db3 noise estimate runs)
GRID_N = (64, 640, 641, 1280, 1281)
GRID_K = (1, 32, 33, 48, 49)
GRID_WIND = (6, 4)
ENGINES = ("auto", "device", "host", "device_split", "device_split_pp", "device_long_hrf", "device_split_long_hrf", "device_pp")
AUTO_LBDA = ("host", "device", "device_split", "device_split_pp", "device_long_hrf", "device_split_long_hrf", "device_pp")
SWITCHES = ("PER_VOXEL_SPLIT", "LONG_HRF", "SPLIT_LONG_HRF")
SEARCHES = ("auto_lbda_solve", "auto_lbda_solve_split", "auto_lbda_solve_long", "auto_lbda_solve_split_long",
            "auto_lbda_solve_pp", "auto_lbda_solve_split_pp", "auto_lbda_solve_long_pp", "auto_lbda_solve_split_long_pp")
SOLVES = ("fista_solve", "fista_solve_pp_d")
CARRIED = ((640, 32), (1280, 32), (640, 48), (1280, 48))       # one shape per form, for the 1-D calls of deconv_auto
V = 3


def cases():
    """Every case as a JSON-able list: ``[call, y kind, hrf kind, N, K, wind, *what the call adds]``."""
    out = []
    grid = list(itertools.product(GRID_N, GRID_K, GRID_WIND))
    for engine, (N, K, wind), hrf in itertools.product(ENGINES, grid, ("1d", "pv")):
        out.append(["deconv_auto", "2d", hrf, N, K, wind, engine])
    for engine, (N, K) in itertools.product(ENGINES, CARRIED):
        out.append(["deconv_auto", "1d", "1d", N, K, 6, engine])
    for mode, on, y, (N, K, wind), hrf in itertools.product(AUTO_LBDA, (0, 7), ("2d", "1d"), grid, ("1d", "pv")):
        out.append(["deconv_none", y, hrf, N, K, wind, mode, on])
    for on, (y, hrf), (N, K, wind), early in itertools.product(range(8), (("1d", "1d"), ("2d_f32", "1d"), ("2d", "pv")), grid,
                                                               (True, False)):
        out.append(["deconv_lbda", y, hrf, N, K, wind, on, early])
    return out


def case_list_hash():
    return hashlib.sha256(json.dumps(cases(), separators=(",", ":")).encode()).hexdigest()


class Reached(Exception):
    """A route's end: the solver function it called and the `force` it passed."""


@contextlib.contextmanager
def patched():
    """-> the `bold_signal` module with the observation points in place; everything is put back on exit."""
    from pybold_amd import bold_signal, solver

    def recorder(name):
        def record(*a, **k):
            raise Reached(name, k.get("force"))
        return record

    new = [(solver, "device", lambda dev=None: torch.device("cpu")),
           (bold_signal, "_pv_steps", lambda T, n: np.ones(T.shape[0])),
           (bold_signal, "spectral_radius_est", lambda *a, **k: 1.0),
           (bold_signal, "DISPATCH", "ctypes")]
    new += [(solver, name, recorder(name)) for name in SEARCHES + SOLVES]
    new += [(bold_signal, name, getattr(bold_signal, name)) for name in SWITCHES + ("AUTO_LBDA",)]     # (run_case sets them)
    old = [(mod, name, getattr(mod, name)) for mod, name, _ in new]
    try:
        for mod, name, value in new:
            setattr(mod, name, value)
        yield bold_signal
    finally:
        for mod, name, value in old:
            setattr(mod, name, value)


def run_case(bold_signal, case):
    """-> ``[function reached or None, its force, exception text or None, [warnings]]`` of one case, under `patched`."""
    from pybold_amd import solver
    call, ykind, hkind, N, K, wind = case[:6]
    y = np.zeros(N) if ykind == "1d" else np.zeros((V, N), dtype=np.float32 if ykind == "2d_f32" else np.float64)
    hrf = np.zeros((V, K)) if hkind == "pv" else np.zeros(K)
    on = 0
    if call == "deconv_auto":
        def go():
            return bold_signal.deconv_auto(y, 1.0, hrf, sigma=1.0, wind=wind, engine=case[6])
    elif call == "deconv_none":
        bold_signal.AUTO_LBDA, on = case[6], case[7]

        def go():
            return bold_signal.deconv(y, 1.0, hrf, wind=wind)
    else:
        on = case[6]

        def go():
            return bold_signal.deconv(y, 1.0, hrf, lbda=0.1, early_stopping=case[7], wind=wind)
    for bit, name in enumerate(SWITCHES):
        setattr(bold_signal, name, bool(on >> bit & 1))
    solver._warned.clear()
    fn = force = err = None
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        try:
            go()
            err = "returned"
        except Reached as r:
            fn, force = r.args
        except Exception as e:                                 # noqa: BLE001 -- whatever the call answers is the record
            err = "%s: %s" % (type(e).__name__, e)
    # (the file a warning points at: the caller of `deconv` / `deconv_auto`, this module, whatever the depth it is raised at)
    return [fn, force, err, ["%s: %s [%s]" % (w.category.__name__, w.message, os.path.basename(w.filename)) for w in caught]]


def record():
    """-> the recording: the case list's hash and count, the distinct outcomes, and each case's index into them."""
    outcomes, index = [], []
    with patched() as bold_signal:
        for case in cases():
            got = run_case(bold_signal, case)
            if got not in outcomes:
                outcomes.append(got)
            index.append(outcomes.index(got))
    return {"case_list_sha256": case_list_hash(), "n_cases": len(index), "outcomes": outcomes, "index": index}
