"""CPU-only checks of the opt-in four-wave form with one HRF per voxel (series of 641 .. 1 280 scans): `PB_FLAG_PP_SPLIT` on
`pb_fista_solve_pp_d`, `pb_fista_pp_split_supported`, `pb_auto_lbda_split_pp_d` and the Python layers above them are
exported and bound, answer the shape query, validate their arguments before anything reaches a device; the register
reports of the new objects.  The parity tests are in tests/test_gpu_per_voxel_split.py."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "pybold_amd", "csrc", "build")
NEW = ("pb_fista_pp_split_supported", "pb_auto_lbda_split_pp_d")
NONE, LOOPS, WINDOW = 0, 1, 2
GENERIC, FAST, PP_SPLIT = 1, 2, 1048576


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not glob.glob(os.path.join(BUILD, "exactsplitpp_*.res")):
        ge.build()
    return _lib.load()


def test_the_new_symbols_are_exported_and_bound(lib):
    from pybold_amd import _lib, bold_signal, solver
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pybold_hip.h")).read()
    for name in NEW:
        assert hasattr(raw, name), "missing export " + name
        assert name in _lib.SIGNATURES, "not bound: " + name
        assert re.search(r"\b%s\s*\(" % name, header), "not declared: " + name
    assert _lib.PB_FLAG_PP_SPLIT == PP_SPLIT and re.search(r"#define\s+PB_FLAG_PP_SPLIT\s+%du\b" % PP_SPLIT, header)
    # a free bit: no other flag of the header carries it
    others = [int(v) for n, v in re.findall(r"#define\s+(PB_FLAG_\w+)\s+(\d+)u", header) if n != "PB_FLAG_PP_SPLIT"]
    assert others and all(v & PP_SPLIT == 0 for v in others)
    # the parameter list of pb_auto_lbda_pp_d
    assert _lib.SIGNATURES["pb_auto_lbda_split_pp_d"] == _lib.SIGNATURES["pb_auto_lbda_pp_d"]
    for fn in ("pp_split_supported", "auto_lbda_solve_split_pp", "fista_solve_pp_d"):
        assert callable(getattr(solver, fn))
    assert "split" not in solver._FORCE                   # no other function accepts it
    assert bold_signal.PER_VOXEL_SPLIT == (os.environ.get("PYBOLD_AMD_PP_SPLIT", "0") == "1")


def test_pp_split_supported_on_a_grid(lib):
    from pybold_amd import solver
    for N in (1, 300, 639, 640, 641, 642, 700, 960, 961, 1200, 1279, 1280, 1281, 2000, 100000):
        for K in (1, 2, 17, 30, 31, 32, 33, 40):
            want = int(641 <= N <= 1280 and K <= 32)
            for stop, wind, ok in ((NONE, 6, 1), (LOOPS, 6, 1), (WINDOW, 6, 1), (NONE, 4, 1), (LOOPS, 4, 1),
                                   (WINDOW, 4, 0), (WINDOW, 8, 0), (3, 6, 0), (-1, 6, 0)):
                assert lib.pb_fista_pp_split_supported(N, K, stop, wind) == want * ok, (N, K, stop, wind)
            # the queries of the existing forms are what they were
            assert lib.pb_fista_which_kernel_pp_d(N, K, 1, WINDOW, 6) in (0, 9, -1)
            assert lib.pb_fista_which_kernel_pp_d(N, K, 1, WINDOW, 6) != 9 or N <= 640
    for N, K in ((0, 30), (700, 0), (-5, 30)):
        assert lib.pb_fista_pp_split_supported(N, K, NONE, 6) == 0
    assert solver.pp_split_supported(700, 30, "window") and solver.pp_split_supported(1280, 32) and solver.pp_split_supported(641, 1, "loops")
    assert not solver.pp_split_supported(640, 30) and not solver.pp_split_supported(1281, 30) and not solver.pp_split_supported(700, 33)
    assert not solver.pp_split_supported(700, 30, "window", wind=4)
    # the search's shapes: pb_auto_lbda_split_supported answers for them
    assert lib.pb_auto_lbda_split_supported(700, 30, 6) == 1 and lib.pb_auto_lbda_split_supported(640, 30, 6) == 0


def _solve(lib, **over):
    fake = ctypes.c_void_p(4096)                     # never dereferenced: validation fails first
    a = dict(y=fake, ldy=700, y_rep=1, w=fake, ldw=700, P=4, N=700, taps=fake, ldt=30, K=30, step=fake, lbda=1.0, lbda_dev=None,
             betas=fake, n_iter=10, J=None, ldj=0, stop=NONE, tol=0.0, wind=6, n_done=fake, flags=PP_SPLIT)
    a.update(over)
    if "N" in over and "ldy" not in over:
        a["ldy"] = a["ldw"] = a["N"]
    if "K" in over and "ldt" not in over:
        a["ldt"] = a["K"]
    rc = lib.pb_fista_solve_pp_d(a["y"], a["ldy"], a["y_rep"], a["w"], a["ldw"], a["P"], a["N"], a["taps"], a["ldt"], a["K"],
                                 a["step"], a["lbda"], a["lbda_dev"], a["betas"], a["n_iter"], a["J"], a["ldj"], a["stop"],
                                 a["tol"], a["wind"], a["n_done"], a["flags"], None)
    return rc, lib.pb_last_error()


def _auto(lib, **over):
    fake = ctypes.c_void_p(4096)
    a = dict(y=fake, ldy=700, w=fake, ldw=700, cold=1, V=4, N=700, taps=fake, ldt=30, K=30, step=fake, betas=fake,
             sigma=fake, early=1, tol=1e-6, wind=6, nb_iter=10, nb_sub_iter=10, chunk=0, R=None, G=None, J=None, ldtr=0,
             alpha=fake, lbda=fake, n_outer=fake, n_inner=fake, work=fake, work_len=lib.pb_auto_lbda_work_len(4))
    a.update(over)
    if "N" in over and "ldy" not in over:
        a["ldy"] = a["ldw"] = a["N"]
    if "K" in over and "ldt" not in over:
        a["ldt"] = a["K"]
    rc = lib.pb_auto_lbda_split_pp_d(a["y"], a["ldy"], a["w"], a["ldw"], a["cold"], a["V"], a["N"], a["taps"], a["ldt"], a["K"],
                                     a["step"], a["betas"], a["sigma"], a["early"], a["tol"], a["wind"], a["nb_iter"],
                                     a["nb_sub_iter"], a["chunk"], a["R"], a["G"], a["J"], a["ldtr"], a["alpha"], a["lbda"],
                                     a["n_outer"], a["n_inner"], a["work"], a["work_len"], None)
    return rc, lib.pb_last_error()


def test_argument_errors_do_not_reach_the_gpu(lib):
    fake = ctypes.c_void_p(4096)
    for call, name, cases in (
            (_solve, b"pb_fista_solve_pp_d",
             ((dict(N=640), b"641..1280"), (dict(N=1281), b"641..1280"), (dict(N=300), b"641..1280"), (dict(K=33), b"32 taps"),
              (dict(stop=WINDOW, wind=4), b"wind"), (dict(flags=PP_SPLIT | GENERIC), b"PB_FLAG_FORCE_GENERIC"),
              (dict(flags=PP_SPLIT | FAST), b"PB_FLAG_FORCE_FAST"), (dict(flags=PP_SPLIT | FAST | GENERIC), b"PB_FLAG_PP_SPLIT"),
              # the checks the call has without the flag, in front of it
              (dict(y=None), b"NULL"), (dict(w=None), b"NULL"), (dict(taps=None), b"NULL"), (dict(step=None), b"NULL"),
              (dict(betas=None), b"NULL"), (dict(ldt=29), b"ldt < K"), (dict(ldy=699), b"leading dimension"),
              (dict(ldw=699), b"leading dimension"), (dict(J=fake, ldj=9), b"leading dimension"), (dict(stop=7), b"stop_mode"),
              (dict(N=0), b"bad size"))),
            (_auto, b"pb_auto_lbda_split_pp_d",
             ((dict(wind=4), b"wind"), (dict(N=640), b"641..1280"), (dict(N=1281), b"641..1280"), (dict(K=33), b"32 taps"),
              (dict(nb_iter=0), b"nb_iter"), (dict(nb_sub_iter=-1), b"nb_sub_iter"), (dict(chunk=-1), b"outer_chunk"),
              (dict(y=None), b"NULL"), (dict(w=None), b"NULL"), (dict(taps=None), b"NULL"),
              (dict(step=None), b"NULL"), (dict(sigma=None), b"NULL"), (dict(betas=None), b"NULL"), (dict(work=None), b"NULL"),
              (dict(work_len=0), b"workspace"), (dict(ldy=699), b"leading dimension"), (dict(ldw=699), b"leading dimension"),
              (dict(ldt=29), b"ldt < K"), (dict(R=fake, ldtr=9), b"leading dimension"), (dict(N=0), b"bad size")))):
        for over, word in cases:
            rc, msg = call(lib, **over)
            assert rc == -1 and word in msg and name in msg, (name, over, rc, msg)
    # without the flag the function is what it was: these are the pins of tests/test_per_voxel_hrf_host.py at 700 scans
    rc, msg = _solve(lib, flags=FAST)
    assert rc == -1 and b"no register-resident" in msg
    assert lib.pb_fista_which_kernel_pp_d(700, 30, 1, WINDOW, 6) == 0
    # zero problems / voxels: a no-op, not an error
    assert _solve(lib, P=0)[0] == 0
    assert _solve(lib, P=0, y=None, w=None)[0] == 0
    assert _auto(lib, V=0, work_len=0)[0] == 0


def test_register_reports_of_the_new_objects(lib):
    """One report per pair of exact_split_table.inc; six kernels of the solver (cost trace x stop rule), two of the search
    (window rule on / off); none of them may touch scratch -- a problem lives in its workgroup for the whole solve."""
    table = open(os.path.join(ROOT, "pybold_amd", "csrc", "exact_split_table.inc")).read()
    pairs = re.findall(r"^PB_EXACT_SPLIT\((\d+), *(\d+)\)", table, flags=re.M)
    assert len(pairs) >= 1
    for prefix, kernel, count in (("exactsplitpp", "fista_exact_split_pp_kernel", 6), ("autosplitpp", "auto_lbda_split_pp_kernel", 2)):
        assert len(glob.glob(os.path.join(BUILD, prefix + "_*.res"))) == len(pairs)
        for s, kt in pairs:
            path = os.path.join(BUILD, "%s_%s_%s.res" % (prefix, s, kt))
            assert os.path.exists(path), path
            text = open(path).read()
            names = re.findall(r"Function Name: (\S*%s\S*)" % kernel, text)
            scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
            vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", text)]
            assert len(set(names)) == count and len(names) == count and len(scratch) == count, (path, names)
            assert scratch == [0] * count, (path, scratch)
            # (the architectural vector registers alone: no instantiation leans on the accumulation file)
            assert len(vgprs) == count and max(vgprs) <= 256, (path, vgprs)


def test_python_refusals_come_before_any_device_call(lib, monkeypatch):
    import pybold_amd
    from pybold_amd import solver

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(solver, "device", no_device)
    # the new engine takes one HRF per voxel
    with pytest.raises(ValueError, match="device_split_pp.*'device_split'"):
        pybold_amd.deconv_auto(np.zeros((6, 700)), 1.0, np.zeros(30), sigma=1.0, engine="device_split_pp")
    with pytest.raises(ValueError, match="device_split_pp.*'device_split'"):
        pybold_amd.deconv_auto(np.zeros(700), 1.0, np.zeros(30), sigma=1.0, engine="device_split_pp")
    # ... at its shapes only
    for n, k, wind in ((640, 30, 6), (1281, 30, 6), (700, 33, 6), (700, 30, 4)):
        with pytest.raises(ValueError, match="device_split_pp.*641..1280"):
            pybold_amd.deconv_auto(np.zeros((6, n)), 1.0, np.zeros((6, k)), sigma=1.0, wind=wind, engine="device_split_pp")
    # the single-HRF four-wave engine keeps refusing a 2-D hrf, under the words it used
    with pytest.raises(ValueError, match="device_split.*one HRF"):
        pybold_amd.deconv_auto(np.zeros((6, 700)), 1.0, np.zeros((6, 30)), sigma=1.0, engine="device_split")
    with pytest.raises(ValueError, match="engine must be.*device_split_pp"):
        pybold_amd.deconv_auto(np.zeros((6, 700)), 1.0, np.zeros((6, 30)), sigma=1.0, engine="device_pp")
    # force="split" belongs to fista_solve_pp_d
    with pytest.raises(ValueError, match="split.*fista_solve_pp_d"):
        solver.fista_solve(np.zeros((2, 700)), np.ones(30), 1.0, 1.0, 10, force="split")
    with pytest.raises(KeyError):
        solver.launch_plan(700, 30, 4, force="split")
