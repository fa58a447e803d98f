"""CPU-only: the host side of the conditioning guard for solves whose HRF lives in device memory (include/pybold_hip.h:
pb_fista_guard_work_len, pb_fista_guard_supported, pb_fista_pp_has_matrix_pipe, and the argument checks of
pb_conditioning_marks / pb_fista_solve_pp_guarded / pb_fista_solve_grouped_guarded, which fail before any launch)."""
import ctypes
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


COLD = 256


def test_work_len_grows_with_rows_and_shrinks_for_a_cold_start(lib):
    warm = [lib.pb_fista_guard_work_len(P, 300, 0) for P in (1, 64, 4096, 4097, 50000)]
    cold = [lib.pb_fista_guard_work_len(P, 300, COLD) for P in (1, 64, 4096, 4097, 50000)]
    assert all(b > a for a, b in zip(warm, warm[1:])) and all(b > a for a, b in zip(cold, cold[1:]))
    assert all(c < w for c, w in zip(cold, warm))
    # the warm start of up to P rows of N float64 is what a cold start leaves out; header, marks and two lists stay
    for P, w, c in zip((1, 64, 4096, 4097, 50000), warm, cold):
        assert w - c == 2 * P * 300 and c >= 8 + 3 * P + 2 * P
    assert lib.pb_fista_guard_work_len(64, 1200, 0) > lib.pb_fista_guard_work_len(64, 300, 0)
    assert lib.pb_fista_guard_work_len(64, 1200, COLD) == lib.pb_fista_guard_work_len(64, 300, COLD)
    assert lib.pb_fista_guard_work_len(-1, 300, 0) == 0 and lib.pb_fista_guard_work_len(0, 300, 0) > 0


def test_guard_supported_at_the_edges_of_the_float64_tables(lib):
    """1 one wave per row (up to 640 scans, 32 taps), 2 four waves (641 .. 1 280), 3 / 4 the same for 33 .. 48 taps, 5 the
    LDS kernel (49 .. 64 taps; 1 281 .. 1 344 scans), 0 no guard (65 taps: the marks pass holds 64; 1 345 scans)."""
    want = {(640, 32): 1, (640, 33): 3, (640, 48): 3, (640, 49): 5, (640, 64): 5, (640, 65): 0,
            (641, 32): 2, (641, 33): 4, (641, 48): 4, (641, 49): 5, (641, 64): 5, (641, 65): 0,
            (1280, 32): 2, (1280, 33): 4, (1280, 48): 4, (1280, 49): 5, (1280, 64): 5, (1280, 65): 0,
            (1281, 32): 5, (1281, 33): 5, (1281, 48): 5, (1281, 49): 5, (1281, 64): 5, (1281, 65): 0}
    for stop in (0, 1):
        got = {nk: lib.pb_fista_guard_supported(nk[0], nk[1], stop) for nk in want}
        assert got == want, stop
    assert lib.pb_fista_guard_supported(1344, 20, 0) == 5 and lib.pb_fista_guard_supported(1345, 20, 0) == 0
    assert lib.pb_fista_guard_supported(300, 20, 2) == 0          # the window rule is not a rule of pb_fista_solve_pp
    assert lib.pb_fista_guard_supported(0, 20, 0) == 0 and lib.pb_fista_guard_supported(300, 0, 0) == 0


def test_which_shared_hrf_calls_reach_the_matrix_pipe(lib):
    one_launch, force_mfma, force_mfma2, no_mfma = 32, 16384, 65536, 8192
    mfma = one_launch | force_mfma
    assert lib.pb_fista_pp_has_matrix_pipe(300, 20, 64, 1, 0, mfma) == 1
    assert lib.pb_fista_pp_has_matrix_pipe(300, 20, 64, 0, 0, mfma) == 0          # one HRF per row: vector forms
    assert lib.pb_fista_pp_has_matrix_pipe(300, 20, 64, 1, 1, mfma) == 0          # the _loops_deconv rule: vector forms
    assert lib.pb_fista_pp_has_matrix_pipe(300, 20, 64, 1, 0, no_mfma) == 0
    assert lib.pb_fista_pp_has_matrix_pipe(600, 28, 64, 1, 0, force_mfma2) == 1
    assert lib.pb_fista_pp_has_matrix_pipe(600, 28, 64, 1, 0, 0) == 0             # 64 rows without the pin: latency-bound forms
    assert lib.pb_fista_pp_has_matrix_pipe(1200, 28, 50000, 1, 0, 0) == 1
    assert lib.pb_fista_pp_has_matrix_pipe(300, 20, 50000, 1, 0, 0) == 1          # BASELINE config 4


def _pp_guarded(lib, y, w, taps, step, betas, n_done, work, work_len, P=4, N=300, K=20, ldt=0, stop=0, flags=0):
    return lib.pb_fista_solve_pp_guarded(y, N, w, N, P, N, taps, ldt, K, step, 1.0, None, betas, 10, stop, 0.0, n_done, work,
                                         work_len, flags, None)


def test_argument_errors_do_not_reach_the_gpu(lib):
    fake = ctypes.c_void_p(4096)          # never dereferenced: validation fails first
    need = lib.pb_fista_guard_work_len(4, 300, 0)
    name = b"pb_fista_solve_pp_guarded"
    rc = _pp_guarded(lib, fake, fake, fake, fake, fake, fake, None, need)
    assert rc == -1 and name in lib.pb_last_error() and b"work buffer" in lib.pb_last_error()
    rc = _pp_guarded(lib, fake, fake, fake, fake, fake, fake, fake, need - 1)
    assert rc == -1 and name in lib.pb_last_error() and b"pb_fista_guard_work_len" in lib.pb_last_error()
    rc = _pp_guarded(lib, fake, fake, fake, fake, fake, fake, ctypes.c_void_p(4100), need)      # not 8-byte aligned
    assert rc == -1 and name in lib.pb_last_error()
    rc = _pp_guarded(lib, fake, fake, fake, fake, fake, None, fake, need)
    assert rc == -1 and name in lib.pb_last_error() and b"n_done" in lib.pb_last_error()
    rc = _pp_guarded(lib, None, fake, fake, fake, fake, fake, fake, need)
    assert rc == -1 and name in lib.pb_last_error() and b"NULL" in lib.pb_last_error()
    rc = _pp_guarded(lib, fake, fake, fake, fake, fake, fake, fake, need, stop=2)
    assert rc == -1 and name in lib.pb_last_error() and b"stop_mode" in lib.pb_last_error()
    rc = _pp_guarded(lib, fake, fake, fake, fake, fake, fake, fake, need, ldt=5)
    assert rc == -1 and name in lib.pb_last_error() and b"leading dimension" in lib.pb_last_error()
    # a cold start needs the smaller buffer only
    cold_need = lib.pb_fista_guard_work_len(4, 300, COLD)
    rc = _pp_guarded(lib, fake, fake, fake, fake, fake, fake, fake, cold_need - 1, flags=COLD)
    assert rc == -1 and name in lib.pb_last_error()
    # zero problems is a no-op, whatever the pointers
    assert _pp_guarded(lib, None, None, None, None, None, None, None, 0, P=0) == 0

    # the grouped call: its own work buffer, then the guard's
    name = b"pb_fista_solve_grouped_guarded"
    off = np.array([0, 2, 4], dtype=np.int32)
    gneed = lib.pb_fista_grouped_work_len(4, 2, 20)

    def grouped(n_done=fake, work=fake, work_len=gneed, gwork=fake, gwork_len=need, offsets=off, flags=0):
        return lib.pb_fista_solve_grouped_guarded(fake, 300, fake, 300, 4, 300, fake, 20, 20, fake, 2, offsets.ctypes.data, fake, 1.0,
                                                  None, fake, 10, n_done, work, work_len, gwork, gwork_len, flags, None)
    assert grouped(gwork=None) == -1 and name in lib.pb_last_error() and b"guard work buffer" in lib.pb_last_error()
    assert grouped(gwork_len=need - 1) == -1 and name in lib.pb_last_error() and b"pb_fista_guard_work_len" in lib.pb_last_error()
    assert grouped(n_done=None) == -1 and name in lib.pb_last_error() and b"n_done" in lib.pb_last_error()
    assert grouped(work_len=gneed - 1) == -1 and name in lib.pb_last_error() and b"pb_fista_grouped_work_len" in lib.pb_last_error()
    assert grouped(work=None) == -1 and name in lib.pb_last_error() and b"NULL" in lib.pb_last_error()
    assert grouped(offsets=np.array([0, 3, 2], dtype=np.int32)) == -1 and name in lib.pb_last_error() and b"offsets" in lib.pb_last_error()
    # 1 200 scans without the opt-in of the split forms, the matrix pipe forced: refused like the plain call, before any launch
    rc = lib.pb_fista_solve_grouped_guarded(fake, 1200, fake, 1200, 4, 1200, fake, 20, 20, fake, 2, off.ctypes.data, fake, 1.0, None, fake,
                                            10, fake, fake, gneed, fake, lib.pb_fista_guard_work_len(4, 1200, 0), 16384 | 32, None)
    assert rc == -1 and name in lib.pb_last_error() and b"matrix-pipe" in lib.pb_last_error()

    # the marks pass on its own
    name = b"pb_conditioning_marks"
    assert lib.pb_conditioning_marks(fake, 300, 4, 300, fake, 0, 65, None, 0, fake, None) == -1 and name in lib.pb_last_error()
    assert lib.pb_conditioning_marks(fake, 300, 4, 1345, fake, 0, 20, None, 0, fake, None) == -1 and name in lib.pb_last_error()
    assert lib.pb_conditioning_marks(fake, 299, 4, 300, fake, 0, 20, None, 0, fake, None) == -1 and b"leading dimension" in lib.pb_last_error()
    assert lib.pb_conditioning_marks(fake, 300, 4, 300, fake, 19, 20, None, 0, fake, None) == -1 and b"leading dimension" in lib.pb_last_error()
    assert lib.pb_conditioning_marks(fake, 300, 4, 300, fake, 20, 20, fake, 0, fake, None) == -1 and b"offsets" in lib.pb_last_error()
    assert lib.pb_conditioning_marks(fake, 300, 4, 300, fake, 0, 20, None, 0, None, None) == -1 and b"NULL" in lib.pb_last_error()
    assert lib.pb_conditioning_marks(None, 300, 0, 300, None, 0, 20, None, 0, None, None) == 0


def test_python_switch_reads_the_environment_only_for_none(monkeypatch):
    from pybold_amd import solver
    monkeypatch.delenv("PYBOLD_AMD_PP_GUARD", raising=False)
    assert solver.pp_guard_opt_in(None) is False and solver.pp_guard_opt_in(True) is True
    monkeypatch.setenv("PYBOLD_AMD_PP_GUARD", "1")
    assert solver.pp_guard_opt_in(None) is True and solver.pp_guard_opt_in(False) is False
    monkeypatch.setenv("PYBOLD_AMD_PP_GUARD", "yes")
    assert solver.pp_guard_opt_in(None) is False
    import inspect
    import pybold_amd
    from pybold_amd import blind, distributed, parcels
    for fn in (blind.bd_batch, distributed.bd_shared, distributed.BdSharedGraph.__init__, distributed.HipOps.z_step, parcels.bd_parcels):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "guard" and last.default is None, fn
    for fn in (solver.fista_solve_pp, solver.fista_solve_grouped):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "guard" and last.default is False, fn
    assert "guard" not in inspect.signature(pybold_amd.bd).parameters       # the reference's signature
