"""CPU-only checks of `deconv` with one HRF per voxel: the four entry points behind it are exported and bound, validate
their arguments before anything reaches a device, answer the form query; the register reports of the new objects; the
refusals of `deconv` / `deconv_auto` for mismatched `hrf` shapes.  The parity tests are in tests/test_gpu_per_voxel_hrf.py."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "pybold_amd", "csrc", "build")
NEW = ("pb_spectral_radius_pp", "pb_fista_solve_pp_d", "pb_fista_which_kernel_pp_d", "pb_auto_lbda_pp_d")
NONE, LOOPS, WINDOW = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not glob.glob(os.path.join(BUILD, "exactpp_*.res")):
        ge.build()
    return _lib.load()


def test_the_new_symbols_are_exported_and_bound(lib):
    from pybold_amd import _lib, solver
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pybold_hip.h")).read()
    for name in NEW:
        assert hasattr(raw, name), "missing export " + name
        assert name in _lib.SIGNATURES, "not bound: " + name
        assert re.search(r"\b%s\s*\(" % name, header), "not declared: " + name
    assert "fista_exact_pp_kernel" in solver.KERNEL_NAMES[9]
    for fn in ("spectral_radius_batch", "fista_solve_pp_d", "which_kernel_pp_f64", "auto_lbda_solve_pp"):
        assert callable(getattr(solver, fn))


def test_which_kernel_pp_d(lib):
    for args, want in (((640, 32, 1, WINDOW, 6), 9), ((641, 30, 1, WINDOW, 6), 0), ((300, 33, 1, WINDOW, 6), 0),
                       ((300, 30, 0, WINDOW, 4), 0), ((100000, 30, 1, WINDOW, 6), -1),
                       ((23, 3, 0, NONE, 6), 9), ((320, 32, 1, LOOPS, 6), 9), ((321, 17, 0, NONE, 4), 9), ((700, 30, 0, NONE, 6), 0)):
        assert lib.pb_fista_which_kernel_pp_d(*args) == want, args
    from pybold_amd import solver
    assert "fista_exact_pp_kernel" in solver.which_kernel_pp_f64(300, 30, want_J=True, stop="window")
    assert "LDS" in solver.which_kernel_pp_f64(700, 30)
    with pytest.raises(ValueError, match="exceeds LDS"):
        solver.which_kernel_pp_f64(100000, 30)


def _radius(lib, **over):
    fake = ctypes.c_void_p(4096)                     # never dereferenced: validation fails first
    a = dict(x0=fake, ldx=180, V=4, N=180, taps=fake, ldt=30, K=30, nb_iter=30, tol=1e-6, out=fake)
    a.update(over)
    rc = lib.pb_spectral_radius_pp(a["x0"], a["ldx"], a["V"], a["N"], a["taps"], a["ldt"], a["K"], a["nb_iter"], a["tol"], a["out"], None)
    return rc, lib.pb_last_error()


def _solve(lib, **over):
    fake = ctypes.c_void_p(4096)
    a = dict(y=fake, ldy=300, y_rep=1, w=fake, ldw=300, P=4, N=300, taps=fake, ldt=30, K=30, step=fake, lbda=1.0, lbda_dev=None,
             betas=fake, n_iter=10, J=None, ldj=0, stop=NONE, tol=0.0, wind=6, n_done=fake, flags=0)
    a.update(over)
    rc = lib.pb_fista_solve_pp_d(a["y"], a["ldy"], a["y_rep"], a["w"], a["ldw"], a["P"], a["N"], a["taps"], a["ldt"], a["K"],
                                 a["step"], a["lbda"], a["lbda_dev"], a["betas"], a["n_iter"], a["J"], a["ldj"], a["stop"],
                                 a["tol"], a["wind"], a["n_done"], a["flags"], None)
    return rc, lib.pb_last_error()


def _auto(lib, **over):
    fake = ctypes.c_void_p(4096)
    a = dict(y=fake, ldy=300, w=fake, ldw=300, cold=1, V=4, N=300, taps=fake, ldt=30, K=30, step=fake, betas=fake,
             sigma=fake, early=1, tol=1e-6, wind=6, nb_iter=10, nb_sub_iter=10, chunk=0, R=None, G=None, J=None, ldtr=0,
             alpha=fake, lbda=fake, n_outer=fake, n_inner=fake, work=fake, work_len=lib.pb_auto_lbda_work_len(4))
    a.update(over)
    rc = lib.pb_auto_lbda_pp_d(a["y"], a["ldy"], a["w"], a["ldw"], a["cold"], a["V"], a["N"], a["taps"], a["ldt"], a["K"],
                               a["step"], a["betas"], a["sigma"], a["early"], a["tol"], a["wind"], a["nb_iter"],
                               a["nb_sub_iter"], a["chunk"], a["R"], a["G"], a["J"], a["ldtr"], a["alpha"], a["lbda"],
                               a["n_outer"], a["n_inner"], a["work"], a["work_len"], None)
    return rc, lib.pb_last_error()


def test_argument_errors_do_not_reach_the_gpu(lib):
    fake = ctypes.c_void_p(4096)
    for call, name, cases in (
            (_radius, b"pb_spectral_radius_pp",
             ((dict(x0=None), b"NULL"), (dict(taps=None), b"NULL"), (dict(out=None), b"NULL"), (dict(ldt=29), b"ldt < K"),
              (dict(ldx=179), b"leading dimension"), (dict(N=7000, ldx=7000), b"exceeds LDS"), (dict(N=0), b"bad size"))),
            (_solve, b"pb_fista_solve_pp_d",
             ((dict(y=None), b"NULL"), (dict(w=None), b"NULL"), (dict(taps=None), b"NULL"), (dict(step=None), b"NULL"),
              (dict(betas=None), b"NULL"), (dict(ldt=29), b"ldt < K"), (dict(ldy=299), b"leading dimension"),
              (dict(ldw=299), b"leading dimension"), (dict(J=fake, ldj=9), b"leading dimension"), (dict(stop=7), b"stop_mode"),
              (dict(stop=-1), b"stop_mode"), (dict(N=100000, ldy=100000, ldw=100000), b"exceeds LDS"),
              (dict(N=700, ldy=700, ldw=700, flags=2), b"no register-resident"),          # PB_FLAG_FORCE_FAST beyond the register form
              (dict(K=33, ldt=33, flags=2), b"no register-resident"), (dict(N=0), b"bad size"))),
            (_auto, b"pb_auto_lbda_pp_d",
             ((dict(wind=4), b"wind"), (dict(N=641, ldy=641, ldw=641), b"640"), (dict(K=33, ldt=33), b"32 taps"),
              (dict(nb_iter=0), b"nb_iter"), (dict(y=None), b"NULL"), (dict(w=None), b"NULL"), (dict(taps=None), b"NULL"),
              (dict(step=None), b"NULL"), (dict(sigma=None), b"NULL"), (dict(betas=None), b"NULL"), (dict(work=None), b"NULL"),
              (dict(work_len=0), b"workspace"), (dict(ldy=299), b"leading dimension"), (dict(ldt=29), b"ldt < K"),
              (dict(R=fake, ldtr=9), b"leading dimension"), (dict(N=0), b"bad size")))):
        for over, word in cases:
            rc, msg = call(lib, **over)
            assert rc == -1 and word in msg and name in msg, (name, over, rc, msg)
    from pybold_amd import _lib
    assert _lib.PB_FLAG_FORCE_FAST == 2
    # zero problems / voxels: a no-op, not an error
    assert _radius(lib, V=0)[0] == 0
    assert _solve(lib, P=0)[0] == 0
    assert _auto(lib, V=0, work_len=0)[0] == 0


def test_register_reports_of_the_new_objects(lib):
    """One report per pair of exact_table.inc; six kernels of the solver (cost trace x stop rule), two of the search
    (window rule on / off); none of them may touch scratch -- a problem lives in a wave for its whole solve."""
    table = open(os.path.join(ROOT, "pybold_amd", "csrc", "exact_table.inc")).read()
    pairs = re.findall(r"^PB_EXACT\((\d+), *(\d+)\)", table, flags=re.M)
    assert len(pairs) >= 2
    for prefix, kernel, count in (("exactpp", "fista_exact_pp_kernel", 6), ("autopp", "auto_lbda_pp_kernel", 2)):
        assert len(glob.glob(os.path.join(BUILD, prefix + "_*.res"))) == len(pairs)
        for s, kt in pairs:
            path = os.path.join(BUILD, "%s_%s_%s.res" % (prefix, s, kt))
            assert os.path.exists(path), path
            text = open(path).read()
            names = re.findall(r"Function Name: (\S*%s\S*)" % kernel, text)
            scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
            assert len(set(names)) == count and len(names) == count and len(scratch) == count, (path, names)
            assert scratch == [0] * count, (path, scratch)


def test_mismatched_hrf_shapes_are_refused_without_a_gpu(lib):
    import pybold_amd
    y1, y2 = np.zeros(180), np.zeros((6, 180))
    for fn in (pybold_amd.deconv, pybold_amd.deconv_auto):
        for kw in ({}, {"sigma": 1.0}) if fn is pybold_amd.deconv_auto else ({"lbda": 1.0}, {"lbda": None}):
            for y, hrf in ((y1, np.zeros((6, 30))),          # one HRF per voxel, one series
                           (y2, np.zeros((5, 30))),          # five HRFs, six voxels
                           (y2, np.zeros((6, 2, 30)))):      # more than two dimensions
                with pytest.raises(ValueError, match="one HRF per voxel") as e:
                    fn(y, 1.0, hrf, **kw)
                assert str(tuple(np.shape(y))) in str(e.value) and str(tuple(np.shape(hrf))) in str(e.value)
    # the four-wave search takes one HRF for all voxels: refused by name for a 2-D hrf, before the device is asked
    with pytest.raises(ValueError, match="device_split.*one HRF"):
        pybold_amd.deconv_auto(np.zeros((6, 700)), 1.0, np.zeros((6, 30)), sigma=1.0, engine="device_split")
