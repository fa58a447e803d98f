"""CPU-only checks of the device-resident lambda search with one voxel per workgroup of four waves
(`pb_auto_lbda_split_d`, `deconv_auto(engine="device_split")`, csrc/fista_auto_split.h): the support table, argument
validation that never reaches a device, the register report of the build, the exports.  The parity tests are in
tests/test_gpu_auto_lbda_split.py."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not glob.glob(os.path.join(ROOT, "pybold_amd", "csrc", "build", "autosplit_*.res")):
        ge.build()
    return _lib.load()


def test_supported_shapes(lib):
    """641 .. 1 280 scans, up to 32 taps, wind = 6 -- and the one-wave search keeps its limit."""
    for n, k, wind, want in ((641, 30, 6, 1), (700, 30, 6, 1), (1200, 28, 6, 1), (1280, 32, 6, 1), (1280, 1, 6, 1),
                             (640, 30, 6, 0), (1281, 30, 6, 0), (1200, 33, 6, 0), (1200, 28, 4, 0), (0, 30, 6, 0),
                             (1200, 0, 6, 0)):
        assert lib.pb_auto_lbda_split_supported(n, k, wind) == want, (n, k, wind)
    assert lib.pb_auto_lbda_supported(641, 30, 6) == 0
    from pybold_amd import solver
    assert solver.auto_lbda_split_supported(700, 30) and not solver.auto_lbda_split_supported(640, 30)
    assert not solver.auto_lbda_split_supported(1200, 28, wind=4) and not solver.auto_lbda_supported(641, 30)


def _auto_split(lib, **over):
    """pb_auto_lbda_split_d on pointers that are never dereferenced: validation must fail first."""
    fake = ctypes.c_void_p(4096)
    taps = np.ones(4)
    a = dict(y=fake, ldy=1200, w=fake, ldw=1200, cold=1, V=4, N=1200, taps=taps.ctypes.data, K=4, step=1.0, betas=fake,
             sigma=fake, early=1, tol=1e-6, wind=6, nb_iter=10, nb_sub_iter=10, chunk=0, R=None, G=None, J=None, ldt=0,
             alpha=fake, lbda=fake, n_outer=fake, n_inner=fake, work=fake, work_len=lib.pb_auto_lbda_work_len(4), stream=None)
    a.update(over)
    rc = lib.pb_auto_lbda_split_d(a["y"], a["ldy"], a["w"], a["ldw"], a["cold"], a["V"], a["N"], a["taps"], a["K"], a["step"],
                                  a["betas"], a["sigma"], a["early"], a["tol"], a["wind"], a["nb_iter"], a["nb_sub_iter"],
                                  a["chunk"], a["R"], a["G"], a["J"], a["ldt"], a["alpha"], a["lbda"], a["n_outer"],
                                  a["n_inner"], a["work"], a["work_len"], a["stream"])
    return rc, lib.pb_last_error()


def test_argument_errors_do_not_reach_the_gpu(lib):
    for over, word in ((dict(N=640, ldy=640, ldw=640), b"641..1280"), (dict(N=1281, ldy=1281, ldw=1281), b"641..1280"),
                       (dict(K=33), b"32 taps"), (dict(wind=4), b"wind"), (dict(nb_iter=0), b"nb_iter"),
                       (dict(y=None), b"NULL"), (dict(w=None), b"NULL"), (dict(sigma=None), b"NULL"), (dict(taps=None), b"NULL"),
                       (dict(betas=None), b"NULL"), (dict(work=None), b"NULL"),
                       (dict(work_len=lib.pb_auto_lbda_work_len(4) - 1), b"workspace"), (dict(ldy=1199), b"leading dimension"),
                       (dict(step=0.0), b"step"), (dict(R=ctypes.c_void_p(4096), ldt=9), b"ldt")):
        rc, msg = _auto_split(lib, **over)
        assert rc == -1 and word in msg and b"pb_auto_lbda_split_d" in msg, (over, rc, msg)
    # the same order as pb_auto_lbda_d: the window before the length before the taps
    assert b"wind" in _auto_split(lib, wind=4, N=640, K=33)[1] and b"641..1280" in _auto_split(lib, N=640, K=33)[1]
    from pybold_amd import _lib
    with pytest.raises(_lib.PyboldHipError):
        _lib.check(_auto_split(lib, wind=5)[0], "pb_auto_lbda_split_d")
    # zero voxels is a no-op, not an error
    assert _auto_split(lib, V=0, work_len=0)[0] == 0


def test_neither_instantiation_of_the_split_search_kernel_spills(lib):
    """One voxel lives in a workgroup for up to a million inner iterations: a spill there is paid every pass."""
    path = os.path.join(ROOT, "pybold_amd", "csrc", "build", "autosplit_5_32.res")
    assert os.path.exists(path), path
    text = open(path).read()
    names = re.findall(r"Function Name: (\S*auto_lbda_split_kernel\S*)", text)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(set(names)) == 2 and len(names) == 2 and len(scratch) == 2, (names, scratch)      # STOP = 0 and STOP = 2
    assert scratch == [0, 0], scratch
    # the report's name is read by no other test's pattern
    build = os.path.join(ROOT, "pybold_amd", "csrc", "build")
    assert path not in glob.glob(os.path.join(build, "auto_*.res")) + glob.glob(os.path.join(build, "exactsplit_*.res"))


def test_engine_refuses_other_shapes_by_name():
    """Shapes the four-wave engine does not carry are refused before anything touches a device."""
    import pybold_amd
    with pytest.raises(ValueError, match="300 scans"):
        pybold_amd.deconv_auto(np.zeros((2, 300)), 1.0, np.ones(30), sigma=1.0, engine="device_split")
    with pytest.raises(ValueError, match="641..1280 scans"):
        pybold_amd.deconv_auto(np.zeros((2, 1281)), 1.0, np.ones(30), sigma=1.0, engine="device_split")
    with pytest.raises(ValueError, match="33 taps"):
        pybold_amd.deconv_auto(np.zeros((2, 700)), 1.0, np.ones(33), sigma=1.0, engine="device_split")
    with pytest.raises(ValueError, match="wind = 4"):
        pybold_amd.deconv_auto(np.zeros((2, 700)), 1.0, np.ones(30), sigma=1.0, engine="device_split", wind=4)
    with pytest.raises(ValueError, match="engine"):
        pybold_amd.deconv_auto(np.zeros((2, 700)), 1.0, np.ones(30), engine="split")


def test_exports_and_operator(lib):
    import inspect
    from pybold_amd import solver, torch_ops
    assert callable(solver.auto_lbda_solve_split) and callable(solver.auto_lbda_split_supported)
    assert callable(torch_ops.auto_lbda_solve_split)
    assert inspect.signature(solver.auto_lbda_solve_split) == inspect.signature(solver.auto_lbda_solve)
    assert inspect.signature(torch_ops.auto_lbda_solve_split) == inspect.signature(torch_ops.auto_lbda_solve)
    ops = torch_ops.load()
    assert hasattr(ops, "auto_lbda_solve_split") and hasattr(ops, "auto_lbda_solve")


# ---- the inputs of the alpha-window test (tests/test_gpu_auto_lbda_split.py) --------------------------------------------
WINDOW_SCALES = (1.0, 1.5, 2.0, 3.0)
WINDOW_BUDGETS = ((40, 30, 1.0e-1), (12, 20, 1.0e-6))            # (nb_iter, nb_sub_iter, tol): every row fires / none does


def window_rows(g, case):
    """24 rows ``(Y (24, N), sigma (24,))`` of a case of auto_lbda_long.npz: sc * y and sc * y[::-1] for four scales, each
    with the case's three noise levels."""
    y, sig = g[case + "_y"], g[case + "_sigma"]
    rows = []
    for sc in WINDOW_SCALES:
        for base in (y, y[::-1].copy()):
            rows += [(sc * base, float(s)) for s in sig]
    assert len(rows) == 24
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows])


_oracle_runs = {}


def window_oracle(g, case, budget):
    """The C oracle's run of `window_rows` at a budget, computed once per session and shared."""
    key = (case,) + tuple(budget)
    if key not in _oracle_runs:
        from oracle import c_oracle
        Y, sigma = window_rows(g, case)
        nb_iter, nb_sub_iter, tol = budget
        _oracle_runs[key] = c_oracle.deconv_auto_lbda_batch(Y, g[case + "_hrf"], sigma, float(g[case + "_lipschitz"]), nb_iter=nb_iter,
                                                            nb_sub_iter=nb_sub_iter, tol=tol, threads=8)
    return _oracle_runs[key]


def oracle_alpha(R, n_outer, sigma, n):
    """The alpha trajectory of every row from the oracle's residuals: alpha_i = 1 + sum_{j <= i} 1e-4 (R_j - n sigma^2)."""
    return [1.0 + np.cumsum(1.0e-4 * (R[v, :n_outer[v]] - n * sigma[v] ** 2)) for v in range(len(sigma))]


@pytest.mark.parametrize("case,n_distinct", [("n700", 6), ("hcp", 4)])
def test_oracle_fires_the_alpha_window_on_every_comparison_row(golden, case, n_distinct):
    """The ground of the alpha-window test on the device: at (40, 30, tol 1e-1) the oracle's alpha window fires on all 24
    rows, at `n_distinct` different outer iterations, alpha stays away from the pole at 0 (|alpha| > 1e-2, so a
    rounding-level difference of a residual sum is not amplified beyond ~1e-12) and some rows take lambda negative; at
    (12, 20, tol 1e-6) it fires on none."""
    g = golden("auto_lbda_long")
    Y, sigma = window_rows(g, case)
    _, _, R, _, n_outer = window_oracle(g, case, WINDOW_BUDGETS[0])
    alphas = oracle_alpha(R, n_outer, sigma, Y.shape[1])
    print("%s: n_outer %s, min |alpha| %.4f, rows with alpha < 0: %d"
          % (case, sorted(set(n_outer.tolist())), min(np.abs(a).min() for a in alphas), sum(bool((a < 0).any()) for a in alphas)))
    assert (n_outer < WINDOW_BUDGETS[0][0]).all() and len(set(n_outer.tolist())) == n_distinct
    assert min(np.abs(a).min() for a in alphas) > 1.0e-2
    _, _, R, _, n_outer = window_oracle(g, case, WINDOW_BUDGETS[1])
    assert (n_outer == WINDOW_BUDGETS[1][0]).all()
    assert min(np.abs(a).min() for a in oracle_alpha(R, n_outer, sigma, Y.shape[1])) > 1.0e-2
