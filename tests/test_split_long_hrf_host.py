"""CPU-only checks of the opt-in four-wave float64 register form for HRFs of up to 48 taps (series of 641 .. 1 280 scans, one
problem per workgroup of four waves, the taps in one VGPR pair of every wave: csrc/fista_exact_split_long.h):
`pb_fista_solve_split_long_d` / `pb_fista_solve_split_long_pp_d` (entry points of their own: every flag bit of the header is
taken up to `PB_FLAG_LONG_HRF`, which tests/test_long_hrf_host.py pins as the highest), `pb_fista_split_long_hrf_supported`,
`pb_auto_lbda_split_long_d`, `pb_auto_lbda_split_long_pp_d`, `pb_auto_lbda_split_long_supported` and the Python layers above
them are exported and bound, answer the shape queries, validate their arguments before anything reaches a device; the register
reports of the new objects; the queries and limits of the existing forms are what they were.  The parity tests are in
tests/test_gpu_split_long_hrf.py."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "pybold_amd", "csrc", "build")
NEW = ("pb_fista_split_long_hrf_supported", "pb_fista_solve_split_long_d", "pb_fista_solve_split_long_pp_d",
       "pb_auto_lbda_split_long_supported", "pb_auto_lbda_split_long_d", "pb_auto_lbda_split_long_pp_d")
NONE, LOOPS, WINDOW = 0, 1, 2
GENERIC, FAST, COLD, PP_SPLIT, LONG_HRF = 1, 2, 256, 1048576, 2097152


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not glob.glob(os.path.join(BUILD, "autosplitlongpp_*.res")):
        ge.build()
    return _lib.load()


def test_the_new_symbols_are_exported_and_bound(lib):
    import pybold_amd
    from pybold_amd import _lib, bold_signal, solver, torch_ops
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pybold_hip.h")).read()
    for name in NEW:
        assert hasattr(raw, name), "missing export " + name
        assert name in _lib.SIGNATURES, "not bound: " + name
        assert re.search(r"\b%s\s*\(" % name, header), "not declared: " + name
    # the form is named by its entry points, not by a flag: the header defines no flag beyond those it had, in any spelling
    assert not hasattr(_lib, "PB_FLAG_SPLIT_LONG_HRF") and "PB_FLAG_SPLIT_LONG_HRF" not in header
    flags = dict((n, int(v)) for n, v in re.findall(r"#define\s+(PB_FLAG_\w+)\s+(\d+)u", header))
    assert len(flags) == len(re.findall(r"#\s*define\s+PB_FLAG_", header)) and max(flags.values()) == LONG_HRF
    # the parameter lists of the solves they mirror
    assert _lib.SIGNATURES["pb_fista_solve_split_long_d"] == _lib.SIGNATURES["pb_fista_solve_d"]
    assert _lib.SIGNATURES["pb_fista_solve_split_long_pp_d"] == _lib.SIGNATURES["pb_fista_solve_pp_d"]
    # the parameter lists of the searches they mirror
    assert _lib.SIGNATURES["pb_auto_lbda_split_long_d"] == _lib.SIGNATURES["pb_auto_lbda_split_d"]
    assert _lib.SIGNATURES["pb_auto_lbda_split_long_pp_d"] == _lib.SIGNATURES["pb_auto_lbda_split_pp_d"]
    assert _lib.SIGNATURES["pb_auto_lbda_split_long_supported"] == _lib.SIGNATURES["pb_auto_lbda_split_supported"]
    assert _lib.SIGNATURES["pb_fista_split_long_hrf_supported"] == _lib.SIGNATURES["pb_fista_long_hrf_supported"]
    for fn in ("split_long_hrf_supported", "auto_lbda_split_long_supported", "auto_lbda_solve_split_long",
               "auto_lbda_solve_split_long_pp"):
        assert callable(getattr(solver, fn))
    assert callable(torch_ops.auto_lbda_solve_split_long) and hasattr(torch_ops.load(), "auto_lbda_solve_split_long")
    assert "split_long_hrf" not in solver._FORCE          # fista_solve (float64 y) and fista_solve_pp_d only
    # the switch: off unless the environment says "1", the pattern of LONG_HRF
    assert bold_signal.SPLIT_LONG_HRF == (os.environ.get("PYBOLD_AMD_SPLIT_LONG_HRF", "0") == "1")
    assert pybold_amd.bold_signal is bold_signal


def test_supported_queries_on_a_grid(lib):
    from pybold_amd import solver
    for N in (0, 1, 640, 641, 960, 1280, 1281):
        for K in (0, 1, 32, 33, 48, 49):
            shape = int(641 <= N <= 1280 and 1 <= K <= 48)
            for wind in (4, 6, 8):
                assert lib.pb_auto_lbda_split_long_supported(N, K, wind) == shape * int(wind == 6), (N, K, wind)
                for stop in (NONE, LOOPS, WINDOW):
                    want = shape * int(stop != WINDOW or wind == 6)
                    assert lib.pb_fista_split_long_hrf_supported(N, K, stop, wind) == want, (N, K, stop, wind)
                for stop in (-1, 3):
                    assert lib.pb_fista_split_long_hrf_supported(N, K, stop, wind) == 0
    assert solver.split_long_hrf_supported(1200, 42, "window") and solver.split_long_hrf_supported(1280, 48)
    assert solver.split_long_hrf_supported(641, 33, "loops") and solver.split_long_hrf_supported(700, 1)
    assert not solver.split_long_hrf_supported(640, 42) and not solver.split_long_hrf_supported(1281, 42)
    assert not solver.split_long_hrf_supported(1200, 49)
    assert not solver.split_long_hrf_supported(1200, 42, "window", wind=4) and solver.split_long_hrf_supported(1200, 42, "loops", wind=4)
    assert solver.auto_lbda_split_long_supported(1200, 42) and not solver.auto_lbda_split_long_supported(1200, 42, wind=4)
    assert not solver.auto_lbda_split_long_supported(640, 42) and not solver.auto_lbda_split_long_supported(1200, 49)


def test_the_existing_queries_keep_their_answers(lib):
    """Opt-in by name: nothing that describes a call without the flag moves."""
    for N in (641, 700, 1200, 1280):
        for K in (33, 42, 48):
            assert lib.pb_auto_lbda_supported(N, K, 6) == 0 and lib.pb_auto_lbda_split_supported(N, K, 6) == 0
            assert lib.pb_auto_lbda_long_supported(N, K, 6) == 0
            for stop in (NONE, LOOPS, WINDOW):
                assert lib.pb_fista_long_hrf_supported(N, K, stop, 6) == 0
                assert lib.pb_fista_pp_split_supported(N, K, stop, 6) == 0
                for wj in (0, 1):
                    assert lib.pb_fista_which_kernel_d(N, K, wj, stop, 6) == 0
                    assert lib.pb_fista_which_kernel_pp_d(N, K, wj, stop, 6) == 0
        assert lib.pb_auto_lbda_split_supported(N, 32, 6) == 1 and lib.pb_fista_pp_split_supported(N, 32, WINDOW, 6) == 1
        assert lib.pb_fista_which_kernel_d(N, 32, 0, WINDOW, 6) == 8 and lib.pb_fista_which_kernel_pp_d(N, 32, 0, WINDOW, 6) == 0
    assert lib.pb_auto_lbda_long_supported(640, 42, 6) == 1 and lib.pb_fista_long_hrf_supported(640, 48, WINDOW, 6) == 1
    table = open(os.path.join(ROOT, "pybold_amd", "csrc", "exact_split_table.inc")).read()
    assert re.findall(r"^PB_EXACT_SPLIT\((\d+), *(\d+)\)", table, flags=re.M) == [("5", "32")]
    long_table = open(os.path.join(ROOT, "pybold_amd", "csrc", "exact_long_table.inc")).read()
    assert re.findall(r"^PB_EXACT_LONG\((\d+), *(\d+)\)", long_table, flags=re.M) == [("5", "48"), ("10", "48")]
    new_table = open(os.path.join(ROOT, "pybold_amd", "csrc", "exact_split_long_table.inc")).read()
    assert re.findall(r"^PB_EXACT_SPLIT_LONG\((\d+), *(\d+)\)", new_table, flags=re.M) == [("5", "48")]


def _solve_d(lib, **over):
    fake = ctypes.c_void_p(4096)                     # never dereferenced: validation fails first
    a = dict(y=fake, ldy=1200, y_rep=1, w=fake, ldw=1200, P=4, N=1200, taps_host=fake, taps_dev=fake, K=42, step=1.0, lbda=1.0,
             lbda_dev=None, betas=fake, n_iter=10, J=None, ldj=0, stop=NONE, tol=0.0, wind=6, n_done=fake, flags=COLD, entry=None)
    a.update(over)
    if "N" in over and "ldy" not in over:
        a["ldy"] = a["ldw"] = a["N"]
    rc = getattr(lib, a["entry"] or "pb_fista_solve_split_long_d")(a["y"], a["ldy"], a["y_rep"], a["w"], a["ldw"], a["P"], a["N"], a["taps_host"], a["taps_dev"],
                              a["K"], a["step"], a["lbda"], a["lbda_dev"], a["betas"], a["n_iter"], a["J"], a["ldj"], a["stop"],
                              a["tol"], a["wind"], a["n_done"], a["flags"], None)
    return rc, lib.pb_last_error()


def _solve_pp(lib, **over):
    fake = ctypes.c_void_p(4096)
    a = dict(y=fake, ldy=1200, y_rep=1, w=fake, ldw=1200, P=4, N=1200, taps=fake, ldt=42, K=42, step=fake, lbda=1.0, lbda_dev=None,
             betas=fake, n_iter=10, J=None, ldj=0, stop=NONE, tol=0.0, wind=6, n_done=fake, flags=COLD, entry=None)
    a.update(over)
    if "N" in over and "ldy" not in over:
        a["ldy"] = a["ldw"] = a["N"]
    if "K" in over and "ldt" not in over:
        a["ldt"] = a["K"]
    rc = getattr(lib, a["entry"] or "pb_fista_solve_split_long_pp_d")(a["y"], a["ldy"], a["y_rep"], a["w"], a["ldw"], a["P"], a["N"], a["taps"], a["ldt"], a["K"],
                                 a["step"], a["lbda"], a["lbda_dev"], a["betas"], a["n_iter"], a["J"], a["ldj"], a["stop"],
                                 a["tol"], a["wind"], a["n_done"], a["flags"], None)
    return rc, lib.pb_last_error()


def _auto(lib, pp, **over):
    fake = ctypes.c_void_p(4096)
    a = dict(y=fake, ldy=1200, w=fake, ldw=1200, cold=1, V=4, N=1200, taps=fake, ldt=42, K=42, step=fake if pp else 1.0, betas=fake,
             sigma=fake, early=1, tol=1e-6, wind=6, nb_iter=10, nb_sub_iter=10, chunk=0, R=None, G=None, J=None, ldtr=0,
             alpha=fake, lbda=fake, n_outer=fake, n_inner=fake, work=fake, work_len=lib.pb_auto_lbda_work_len(4))
    a.update(over)
    if "N" in over and "ldy" not in over:
        a["ldy"] = a["ldw"] = a["N"]
    if "K" in over and "ldt" not in over:
        a["ldt"] = a["K"]
    head = (a["y"], a["ldy"], a["w"], a["ldw"], a["cold"], a["V"], a["N"])
    tail = (a["betas"], a["sigma"], a["early"], a["tol"], a["wind"], a["nb_iter"], a["nb_sub_iter"], a["chunk"], a["R"], a["G"],
            a["J"], a["ldtr"], a["alpha"], a["lbda"], a["n_outer"], a["n_inner"], a["work"], a["work_len"], None)
    if pp:
        rc = lib.pb_auto_lbda_split_long_pp_d(*head, a["taps"], a["ldt"], a["K"], a["step"], *tail)
    else:
        rc = lib.pb_auto_lbda_split_long_d(*head, a["taps"], a["K"], a["step"], *tail)
    return rc, lib.pb_last_error()


def test_argument_errors_do_not_reach_the_gpu(lib):
    fake = ctypes.c_void_p(4096)
    flag_cases = ((dict(N=640), b"641..1280"), (dict(N=300), b"641..1280"), (dict(N=1281), b"641..1280"), (dict(K=49), b"1..48"),
                  (dict(K=64), b"1..48"), (dict(stop=WINDOW, wind=4), b"wind"), (dict(stop=WINDOW, wind=8), b"wind"),
                  (dict(flags=GENERIC), b"PB_FLAG_FORCE_GENERIC"), (dict(flags=FAST), b"PB_FLAG_FORCE_FAST"),
                  (dict(flags=PP_SPLIT), b"PB_FLAG_PP_SPLIT"), (dict(flags=LONG_HRF), b"PB_FLAG_LONG_HRF"),
                  (dict(flags=LONG_HRF, N=600), b"four-wave 48-tap"), (dict(flags=COLD | FAST | GENERIC), b"four-wave 48-tap"),
                  (dict(N=0), b"bad size"), (dict(K=0), b"bad size"),
                  (dict(y=None), b"NULL"), (dict(w=None), b"NULL"), (dict(betas=None), b"NULL"),
                  (dict(ldy=1199), b"leading dimension"), (dict(ldw=1199), b"leading dimension"), (dict(stop=7), b"stop_mode"))
    auto_cases = ((dict(wind=4), b"wind"), (dict(wind=8), b"wind"), (dict(N=640), b"641..1280 scans"), (dict(N=1281), b"641..1280 scans"),
                  (dict(K=49), b"48 taps"), (dict(nb_iter=0), b"nb_iter"),
                  (dict(nb_sub_iter=-1), b"nb_sub_iter"), (dict(chunk=-1), b"outer_chunk"), (dict(y=None), b"NULL"),
                  (dict(w=None), b"NULL"), (dict(taps=None), b"NULL"), (dict(sigma=None), b"NULL"), (dict(betas=None), b"NULL"),
                  (dict(work=None), b"NULL"), (dict(work_len=0), b"workspace"), (dict(ldy=1199), b"leading dimension"),
                  (dict(ldw=1199), b"leading dimension"), (dict(R=fake, ldtr=9), b"nb_iter"), (dict(N=0), b"bad size"),
                  (dict(K=0), b"bad size"))
    for call, name, cases in (
            (_solve_d, b"pb_fista_solve_split_long_d", flag_cases + ((dict(taps_host=None), b"NULL"), (dict(J=fake, ldj=9), b"ldj"))),
            (_solve_pp, b"pb_fista_solve_split_long_pp_d", flag_cases + ((dict(taps=None), b"NULL"), (dict(step=None), b"NULL"),
                                                             (dict(ldt=41), b"ldt < K"), (dict(J=fake, ldj=9), b"ldj"))),
            (lambda l, **o: _auto(l, False, **o), b"pb_auto_lbda_split_long_d", auto_cases + ((dict(step=0.0), b"step"),)),
            (lambda l, **o: _auto(l, True, **o), b"pb_auto_lbda_split_long_pp_d", auto_cases + ((dict(step=None), b"NULL"),
                                                                                               (dict(ldt=41), b"ldt < K")))):
        for over, word in cases:
            rc, msg = call(lib, **over)
            assert rc == -1 and word in msg and name in msg, (name, over, rc, msg)
    # the existing entry points are what they were: PB_FLAG_LONG_HRF stops at 640 scans, 42 taps have no register form with one
    # problem per wave, and the four-wave searches stop at 32 taps
    rc, msg = _solve_d(lib, flags=LONG_HRF, entry="pb_fista_solve_d")
    assert rc == -1 and b"1..640" in msg and b"pb_fista_solve_d" in msg
    rc, msg = _solve_pp(lib, flags=LONG_HRF, entry="pb_fista_solve_pp_d")
    assert rc == -1 and b"1..640" in msg and b"pb_fista_solve_pp_d" in msg
    rc, msg = _solve_pp(lib, flags=PP_SPLIT, entry="pb_fista_solve_pp_d")
    assert rc == -1 and b"exceeds 32 taps" in msg
    rc, msg = _solve_d(lib, flags=FAST, entry="pb_fista_solve_d")
    assert rc == -1 and b"no register-resident" in msg
    a = (fake, 1200, fake, 1200, 1, 4, 1200)
    t = (fake, fake, 1, 1e-6, 6, 10, 10, 0, None, None, None, 0, fake, fake, fake, fake, fake, lib.pb_auto_lbda_work_len(4), None)
    assert lib.pb_auto_lbda_split_d(*a, fake, 42, 1.0, *t) == -1 and b"K=42 exceeds 32 taps" in lib.pb_last_error()
    assert lib.pb_auto_lbda_split_pp_d(*a, fake, 42, 42, fake, *t) == -1 and b"K=42 exceeds 32 taps" in lib.pb_last_error()
    assert lib.pb_auto_lbda_long_d(*a, fake, 42, 1.0, *t) == -1 and b"exceeds 640 scans" in lib.pb_last_error()
    # zero problems / voxels: a no-op, not an error
    assert _solve_d(lib, P=0)[0] == 0 and _solve_d(lib, P=0, y=None, w=None)[0] == 0
    assert _solve_pp(lib, P=0)[0] == 0
    assert _auto(lib, False, V=0, work_len=0)[0] == 0 and _auto(lib, True, V=0, work_len=0)[0] == 0


def test_register_reports_of_the_new_objects(lib):
    """One report per pair of exact_split_long_table.inc and kind of object: six kernels of each solver (cost trace x stop
    rule), two of each search (window rule on / off): 16 kernels.  None may touch scratch or spill a vector register -- a
    problem lives in its workgroup for the whole solve; the solvers hold SplitLds<48> (3 136 bytes) and nothing else in LDS,
    the searches add stat[2][4] (64 bytes)."""
    table = open(os.path.join(ROOT, "pybold_amd", "csrc", "exact_split_long_table.inc")).read()
    pairs = re.findall(r"^PB_EXACT_SPLIT_LONG\((\d+), *(\d+)\)", table, flags=re.M)
    assert pairs == [("5", "48")]
    total = 0
    for prefix, kernel, count, lds_bytes in (("exactsplitlong", "fista_exact_split_long_kernel", 6, 3136),
                                             ("exactsplitlongpp", "fista_exact_split_long_pp_kernel", 6, 3136),
                                             ("autosplitlong", "auto_lbda_split_long_kernel", 2, 3200),
                                             ("autosplitlongpp", "auto_lbda_split_long_pp_kernel", 2, 3200)):
        assert len(glob.glob(os.path.join(BUILD, prefix + "_*.res"))) == len(pairs)
        for s, kt in pairs:
            path = os.path.join(BUILD, "%s_%s_%s.res" % (prefix, s, kt))
            assert os.path.exists(path), path
            text = open(path).read()
            names = re.findall(r"Function Name: (\S*%s\S*)" % kernel, text)
            scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
            spill = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", text)]
            vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", text)]
            lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", text)]
            assert len(set(names)) == count and len(names) == count, (path, names)
            assert scratch == [0] * count, (path, scratch)
            assert spill == [0] * count, (path, spill)
            assert len(vgprs) == count and max(vgprs) <= 256, (path, vgprs)
            assert lds == [lds_bytes] * count, (path, lds)
            total += count
    assert total == 16


def test_python_refusals_come_before_any_device_call(lib, monkeypatch):
    import pybold_amd
    from pybold_amd import solver

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(solver, "device", no_device)
    # the new engine beyond what "device_split" carries: 33..48 taps, 641..1280 scans, wind = 6 -- one HRF or one per voxel
    for n, k, wind in ((640, 42, 6), (1281, 42, 6), (1200, 49, 6), (1200, 42, 4)):
        with pytest.raises(ValueError, match="device_split_long_hrf.*33..48 taps.*641..1280 scans"):
            pybold_amd.deconv_auto(np.zeros((6, n)), 1.0, np.zeros(k), sigma=1.0, wind=wind, engine="device_split_long_hrf")
        with pytest.raises(ValueError, match="device_split_long_hrf.*33..48 taps.*641..1280 scans"):
            pybold_amd.deconv_auto(np.zeros((6, n)), 1.0, np.zeros((6, k)), sigma=1.0, wind=wind, engine="device_split_long_hrf")
    # one HRF per voxel of up to 32 taps belongs to "device_split_pp"
    with pytest.raises(ValueError, match="device_split_long_hrf.*device_split_pp"):
        pybold_amd.deconv_auto(np.zeros((6, 1200)), 1.0, np.zeros((6, 32)), sigma=1.0, engine="device_split_long_hrf")
    # the list of engines names it, and still ends as it did
    with pytest.raises(ValueError, match="engine must be.*'device_split_long_hrf' or 'device_long_hrf', got"):
        pybold_amd.deconv_auto(np.zeros((6, 1200)), 1.0, np.zeros(42), sigma=1.0, engine="device_split_long")
    # the existing engines keep their limits and their words
    with pytest.raises(ValueError, match=r"engine='device_split'\): .*up to 32 taps"):
        pybold_amd.deconv_auto(np.zeros((6, 1200)), 1.0, np.zeros(42), sigma=1.0, engine="device_split")
    with pytest.raises(ValueError, match=r"engine='device_split_pp'\): .*up to 32 taps"):
        pybold_amd.deconv_auto(np.zeros((6, 1200)), 1.0, np.zeros((6, 42)), sigma=1.0, engine="device_split_pp")
    with pytest.raises(ValueError, match="device_long_hrf.*33..48 taps.*640 scans"):
        pybold_amd.deconv_auto(np.zeros((6, 1200)), 1.0, np.zeros(42), sigma=1.0, engine="device_long_hrf")
    with pytest.raises(ValueError, match=r"engine='device'\): .*up to 640 scans"):
        pybold_amd.deconv_auto(np.zeros((6, 1200)), 1.0, np.zeros(42), sigma=1.0, engine="device")
    # force="split_long_hrf" belongs to the float64 solves
    with pytest.raises(ValueError, match="split_long_hrf.*float64 Y only"):
        solver.fista_solve(np.zeros((2, 1200), dtype=np.float32), np.ones(42), 1.0, 1.0, 10, force="split_long_hrf")
    with pytest.raises(KeyError):
        solver.launch_plan(1200, 42, 4, force="split_long_hrf")


def test_the_switch_names_the_form_only_where_it_is_needed(lib, monkeypatch):
    from pybold_amd import bold_signal
    monkeypatch.setattr(bold_signal, "LONG_HRF", False)
    monkeypatch.setattr(bold_signal, "PER_VOXEL_SPLIT", False)
    monkeypatch.setattr(bold_signal, "SPLIT_LONG_HRF", False)
    assert bold_signal._long_hrf_force(1200, 42, "window", 6) is None and bold_signal._pv_force(1200, 42, "window", 6) is None
    monkeypatch.setattr(bold_signal, "SPLIT_LONG_HRF", True)
    assert bold_signal._long_hrf_force(1200, 42, "window", 6) == "split_long_hrf"
    assert bold_signal._long_hrf_force(1280, 48, None, 6) == "split_long_hrf"
    assert bold_signal._long_hrf_force(641, 33, "window", 6) == "split_long_hrf"
    assert bold_signal._pv_force(700, 33, None, 6) == "split_long_hrf"
    # up to 32 taps the existing four-wave forms carry the call; other shapes keep today's route
    for n, k, stop, wind in ((1200, 32, "window", 6), (1200, 20, None, 6), (640, 42, None, 6), (300, 42, None, 6), (1281, 42, None, 6),
                             (1200, 49, None, 6), (1200, 42, "window", 4)):
        assert bold_signal._long_hrf_force(n, k, stop, wind) is None, (n, k, stop, wind)
        assert bold_signal._pv_force(n, k, stop, wind) is None, (n, k, stop, wind)
    # the two switches carry disjoint lengths and do not replace each other; PER_VOXEL_SPLIT keeps its 32 taps
    monkeypatch.setattr(bold_signal, "LONG_HRF", True)
    monkeypatch.setattr(bold_signal, "PER_VOXEL_SPLIT", True)
    assert bold_signal._long_hrf_force(600, 42, None, 6) == "long_hrf" and bold_signal._long_hrf_force(700, 42, None, 6) == "split_long_hrf"
    assert bold_signal._pv_force(700, 32, None, 6) == "split" and bold_signal._pv_force(700, 33, None, 6) == "split_long_hrf"
    monkeypatch.setattr(bold_signal, "SPLIT_LONG_HRF", False)
    assert bold_signal._long_hrf_force(700, 42, None, 6) is None and bold_signal._pv_force(700, 42, None, 6) is None
