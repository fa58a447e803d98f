"""CPU-only checks of the four-wave float64 form (`fista_exact_split_kernel`, csrc/fista_exact_split.h): which shapes
`pb_fista_solve_d` hands to it, validation that never reaches a device, the register reports of the build.  The parity
tests are in tests/test_gpu_exact_split.py."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NONE, LOOPS, WINDOW = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not glob.glob(os.path.join(ROOT, "pybold_amd", "csrc", "build", "exactsplit_*.res")):
        ge.build()
    return _lib.load()


def test_which_float64_kernel(lib):
    """(N, K, cost trace, stop rule, wind) -> 7 one wave per series, 8 four waves, 0 the LDS kernel, -1 nothing."""
    for n, k, wj, stop, wind, want in ((640, 30, 0, NONE, 6, 7), (641, 30, 0, NONE, 6, 8), (1280, 32, 0, NONE, 6, 8),
                                       (1281, 30, 0, NONE, 6, 0), (1200, 33, 0, NONE, 6, 0), (1200, 28, 0, WINDOW, 4, 0),
                                       (1200, 28, 0, WINDOW, 6, 8), (1200, 28, 1, LOOPS, 6, 8), (1200, 28, 1, WINDOW, 6, 8),
                                       (300, 30, 1, WINDOW, 6, 7), (300, 30, 0, WINDOW, 8, 0), (1, 1, 0, NONE, 6, 7),
                                       (1200, 1, 0, NONE, 6, 8), (100000, 30, 0, NONE, 6, -1)):
        assert lib.pb_fista_which_kernel_d(n, k, wj, stop, wind) == want, (n, k, wj, stop, wind)


def test_solver_names_the_float64_kernels(lib):
    from pybold_amd import solver
    assert solver.KERNEL_NAMES[7].startswith("fista_exact_kernel") and solver.KERNEL_NAMES[8].startswith("fista_exact_split_kernel")
    assert solver.which_kernel_f64(640, 30) == solver.KERNEL_NAMES[7]
    assert solver.which_kernel_f64(641, 30) == solver.KERNEL_NAMES[8]
    assert solver.which_kernel_f64(1200, 28, want_J=True, stop="loops") == solver.KERNEL_NAMES[8]
    assert solver.which_kernel_f64(1200, 28, stop="window", wind=6) == solver.KERNEL_NAMES[8]
    assert solver.which_kernel_f64(1200, 28, stop="window", wind=4) == solver.KERNEL_NAMES[0]
    assert solver.which_kernel_f64(1281, 30) == solver.KERNEL_NAMES[0]
    with pytest.raises(ValueError):
        solver.which_kernel_f64(100000, 30)


def test_the_lambda_search_keeps_its_limit(lib):
    """exact_split_table.inc is a table of its own: the device-resident search still ends at 640 scans."""
    assert lib.pb_auto_lbda_supported(641, 30, 6) == 0 and lib.pb_auto_lbda_supported(640, 30, 6) == 1
    table = open(os.path.join(ROOT, "pybold_amd", "csrc", "exact_table.inc")).read()
    assert re.findall(r"^PB_EXACT\((\d+), *(\d+)\)", table, flags=re.M) == [("5", "32"), ("10", "32")]


def _solve_d(lib, N, K, P, flags, taps_dev, stop=NONE, wind=6):
    """pb_fista_solve_d on pointers that are never dereferenced (P = 0, or validation fails first)."""
    from pybold_amd import _lib
    fake = ctypes.c_void_p(4096)
    taps = np.ones(K)
    rc = lib.pb_fista_solve_d(fake, N, 1, fake, N, P, N, taps.ctypes.data, taps_dev, K, 1.0, 1.0, None, fake, 10, None, 0,
                              stop, 1e-3, wind, None, flags, None)
    return rc, lib.pb_last_error()


def test_dispatch_validation_does_not_reach_the_gpu(lib):
    from pybold_amd import _lib
    fake = ctypes.c_void_p(4096)
    # PB_FLAG_FORCE_FAST keeps its meaning -- the one-problem-per-wave form or an error --: it fails beyond 640 scans (four-wave
    # form or not), beyond 32 taps and for another window, and passes up to there (no problems: nothing is launched)
    for n, k, stop, wind in ((1281, 30, NONE, 6), (1200, 33, NONE, 6), (1200, 28, WINDOW, 4), (641, 28, NONE, 6), (700, 30, NONE, 6),
                             (1280, 32, NONE, 6)):
        rc, msg = _solve_d(lib, n, k, 0, _lib.PB_FLAG_FORCE_FAST, fake, stop, wind)
        assert rc == -1 and b"no register-resident float64 kernel" in msg, (n, k, stop, wind, rc, msg)
    assert _solve_d(lib, 640, 32, 0, _lib.PB_FLAG_FORCE_FAST, None)[0] == 0
    # the four-wave form reads the taps from the host copy: no device copy is needed for a shape it carries ...
    assert _solve_d(lib, 1200, 28, 0, 0, None)[0] == 0
    # ... while a call with problems that lands on the LDS kernel is still refused without one, before any launch
    for n, k, flags in ((1281, 28, 0), (1200, 33, 0), (1200, 28, _lib.PB_FLAG_FORCE_GENERIC)):
        rc, msg = _solve_d(lib, n, k, 1, flags, None)
        assert rc == -1 and b"NULL" in msg, (n, k, flags, rc, msg)


def test_no_instantiation_of_the_split_kernel_spills(lib):
    """Six kernels per table entry (cost trace x three stop rules), none of them with scratch."""
    table = open(os.path.join(ROOT, "pybold_amd", "csrc", "exact_split_table.inc")).read()
    pairs = re.findall(r"^PB_EXACT_SPLIT\((\d+), *(\d+)\)", table, flags=re.M)
    assert pairs == [("5", "32")]
    reports = glob.glob(os.path.join(ROOT, "pybold_amd", "csrc", "build", "exactsplit_*.res"))
    assert len(reports) == len(pairs)
    for s, kt in pairs:
        path = os.path.join(ROOT, "pybold_amd", "csrc", "build", "exactsplit_%s_%s.res" % (s, kt))
        assert os.path.exists(path), path
        text = open(path).read()
        names = re.findall(r"Function Name: (\S*fista_exact_split_kernel\S*)", text)
        scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
        assert len(set(names)) == 6 and len(scratch) == 6, (path, names)
        assert scratch == [0] * 6, (path, scratch)
