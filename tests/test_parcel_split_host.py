"""CPU-only tests of the grouped z-step on the split matrix-pipe forms (PB_FLAG_GROUPED_SPLIT, 311 .. 1 280 scans): the
conditions the GPU cases rest on, by the float64 oracle; the routing decision `pb_fista_grouped_route` against the rules
restated in tests/parcel_split_cases.py (2 048 wave slots: what the library assumes without a device); what the build
leaves for the sixteen new objects; and the argument checks that never reach a GPU."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

from tests import parcel_cases as pc
from tests import parcel_split_cases as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "pybold_amd", "csrc", "build")
F, O, S, V = ps.FORCE_MFMA, ps.ONE_LAUNCH, ps.GROUPED_SPLIT, ps.NO_MFMA


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not glob.glob(os.path.join(BUILD, "mfma4g_*.res")):
        ge.build()
    return _lib.load()


# ---- 1: the conditions on the inputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,variant", ps.CASES)
def test_input_conditions_of_every_case(N, K, variant):
    """No zero reference row, every row four times inside the accuracy guard, a last tap that matters (parcel_cases)."""
    norm_min, ratio_max, tail_min = pc.input_conditions(ps.case(N, K, variant))
    assert norm_min > 0.0
    assert ratio_max <= pc.GUARD_RATIO_MAX, ratio_max
    assert tail_min >= pc.TAIL_SHARE_MIN, tail_min


@pytest.mark.parametrize("N,K", ps.HANDBACK_SHAPES)
def test_handback_case_sits_on_both_sides_of_the_accuracy_guard(N, K):
    ratio = ps.guard_ratios(ps.handback_case(N, K))
    even = np.arange(pc.ROWS) % 2 == 0
    print("hand-back case N=%d K=%d: lambda step / max|w| even rows <= %.2e, odd rows >= %.2e" % (N, K, ratio[even].max(), ratio[~even].min()))
    assert ratio[even].max() <= ps.HANDBACK_RATIO_EVEN_MAX
    assert ratio[~even].min() >= ps.HANDBACK_RATIO_ODD_MIN


def test_the_shapes_cover_every_instance():
    assert len(ps.TWO_WAVE) == 11 and len(ps.FOUR_WAVE) == 5
    assert sorted(ps.TWO_WAVE.values())[0] == (311, 320) and sorted(ps.TWO_WAVE.values())[-1] == (609, 640)
    for (a, b), (lo, hi) in ps.TWO_WAVE.items():
        assert b in (a, a + 1) and 32 * (a + b - 1) < lo <= hi == 32 * (a + b)
    assert sorted(ps.FOUR_WAVE.values()) == [(641, 768), (769, 896), (897, 1024), (1025, 1152), (1153, 1280)]
    assert len(ps.CASES) == 16 * 4 * 3


# ---- 2: the route ----------------------------------------------------------------------------------------------------------
def route(lib, sizes, N, K, flags):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    mu, rc = ctypes.c_int(-7), ctypes.c_int(-7)
    code = lib.pb_fista_grouped_route(off.ctypes.data, len(sizes), int(off[-1]), N, K, flags, ctypes.byref(mu), ctypes.byref(rc))
    return code, mu.value, rc.value


def check(lib, sizes, N, K, flags):
    got = route(lib, sizes, N, K, flags)
    assert got == ps.expected_route(sizes, N, K, flags), (sizes, N, K, flags, got, ps.expected_route(sizes, N, K, flags))
    return got


BIG = [20000, 1, 0, 15000]                          # 2 189 units


def test_route_without_the_flag_is_todays(lib):
    assert check(lib, BIG, 300, 27, 0)[0] == 4
    assert check(lib, pc.SIZES, 300, 27, 0) == (0, 0, 0)                # 84 rows: below 4 096
    assert check(lib, pc.SIZES, 300, 27, F | O) == (4, 9, 84)
    for N, K in ((600, 28), (1200, 28), (600, 40)):
        assert check(lib, BIG, N, K, 0) == (0, 0, 0)
        assert check(lib, BIG, N, K, F | O) == (-1, 0, 0)
    assert check(lib, BIG, 300, 27, V) == (0, 0, 0) and check(lib, BIG, 300, 27, V | F) == (-1, 0, 0)
    # whole rounds of 1 024 waves and the rows behind them (tests/test_gpu_parcels_variants.py)
    assert check(lib, [9000, 7384, 616], 150, 27, 0) == (4, 1024, 16376)
    assert check(lib, [10000, 10584, 300], 150, 27, 0) == (4, 1306, 20884)
    assert check(lib, [9000, 7384, 616], 150, 27, O) == (4, 1064, 17000)


def test_route_with_the_flag_serves_311_to_1280_scans_up_to_48_taps(lib):
    for N, code in ((311, 5), (640, 5), (641, 6), (1280, 6)):
        for K in (1, 28, 33, 34, 48):
            assert check(lib, BIG, N, K, S)[0] == code
            assert check(lib, pc.SIZES, N, K, S | F | O) == (code, 9, 84)   # forced: every unit in one launch, whatever the size
    assert check(lib, BIG, 310, 28, S) == check(lib, BIG, 310, 28, 0) and check(lib, BIG, 310, 28, S)[0] == 4
    for N, K in ((1281, 28), (600, 49), (300, 40), (128, 20)):
        assert check(lib, BIG, N, K, S) == (0, 0, 0)
        assert check(lib, BIG, N, K, S | F | O) == (-1, 0, 0)
    assert check(lib, BIG, 600, 28, S | V) == (0, 0, 0) and check(lib, BIG, 600, 28, S | V | F) == (-1, 0, 0)


def test_two_wave_minimum_counts_slot_rows(lib):
    """16 x units against mfma2_long_min_p(K): 5 120 up to 33 taps, 2 048 from 34 on.  Parcels of one row make a unit each."""
    for K, units in ((28, 320), (40, 128)):
        assert check(lib, [16] * (units - 1), 600, K, S) == (0, 0, 0)                       # 5 104 / 2 032 slot rows
        assert check(lib, [16] * units, 600, K, S) == (5, units, 16 * units)               # 5 120 / 2 048
        assert check(lib, [1] * (units - 1), 600, K, S) == (0, 0, 0)                        # the same units with 319 / 127 rows
        assert check(lib, [1] * units, 600, K, S) == (5, units, units)
    assert check(lib, [16] * 100, 1200, 28, S) == (0, 0, 0)                                  # four waves: the remainder rule alone
    assert check(lib, [16] * 161, 1200, 28, S) == (6, 161, 16 * 161)


@pytest.mark.parametrize("N,pass_units", [(600, 512), (1200, 256)])
def test_remainders_of_160_and_161_units_beside_one_whole_pass(lib, N, pass_units):
    """5/16 of 512 units and 10/16 of 256 are both 160: that many go behind the cut, one more stays.  The cut falls inside
    the second parcel, on a unit boundary."""
    first = 16 * (pass_units - 100) - 3                                  # pass_units - 100 units, the last one short
    for rem, stays in ((160, False), (161, True)):
        sizes = [first, 16 * (100 + rem) - 5, 0]
        got = check(lib, sizes, N, 28, S)
        units = pass_units + rem
        assert sum(ps.units_of(sizes)) == units
        if stays:
            assert got == (5 if N <= 640 else 6, units, sum(sizes))
        else:
            assert got == (5 if N <= 640 else 6, pass_units, first + 16 * 100)
        assert check(lib, sizes, N, 28, S | O)[1] == units                # one launch: everything
    # a cut exactly on a parcel boundary, empty parcels around it
    sizes = [0, 16 * pass_units - 7, 0, 0, 90, 5]
    assert check(lib, sizes, N, 28, S) == (5 if N <= 640 else 6, pass_units, 16 * pass_units - 7)


def test_route_of_bad_input_is_minus_one(lib):
    off = np.array([0, 10, 5], dtype=np.int32)
    assert lib.pb_fista_grouped_route(off.ctypes.data, 2, 5, 600, 28, S, None, None) == -1
    ok = np.array([0, 0], dtype=np.int32)
    assert lib.pb_fista_grouped_route(ok.ctypes.data, 1, 0, 600, 28, S, None, None) == -1


def test_python_wrapper_and_force_names(lib):
    from pybold_amd import _lib, solver
    assert _lib.PB_FLAG_GROUPED_SPLIT == S == 8388608
    assert solver._FORCE["gsplit"] == S and solver._FORCE["gsplit_mfma"] == S | F | O
    assert solver._FORCE["gsplit_mfmaonly"] == S | F | O | ps.NO_RESOLVE
    off = np.concatenate([[0], np.cumsum(BIG)])
    assert solver.grouped_route(off, 600, 28, "gsplit") == ps.expected_route(BIG, 600, 28, S)
    assert solver.grouped_route(off, 600, 28) == (0, 0, 0)
    assert solver.grouped_route(pc.OFFSETS, 1200, 48, "gsplit_mfmaonly") == (6, 9, 84)
    assert solver.grouped_route(pc.OFFSETS, 1200, 48, "mfma") == (-1, 0, 0)
    header = open(os.path.join(ROOT, "include", "pybold_hip.h")).read()
    assert re.search(r"\bPB_FLAG_GROUPED_SPLIT = 8388608\b", header)              # (an enumerator, like PB_FLAG_MFMA_DENSE_TILES)


# ---- 3: what the build leaves ------------------------------------------------------------------------------------------------
def test_build_outputs_of_the_sixteen_objects(lib):
    names = (["mfma2g_%d_%d" % ab for ab in ps.TWO_WAVE] + ["mfma4g_%d" % a for a in ps.FOUR_WAVE])
    assert len(names) == 16
    for name in names:
        assert os.path.exists(os.path.join(BUILD, name + ".o")), name
        blocks = open(os.path.join(BUILD, name + ".res")).read().split("Function Name: ")[1:]
        kernels = {b.split()[0]: b for b in blocks}
        tiles = set()
        for sym, b in kernels.items():
            m = re.search(r"fista_mfma[24]_kernelI.*Lb1ELb0ELb0ELb0ELi([23])ELb1EEE", sym)      # TAPS_DEV, plain, NT, GROUPED
            assert m, sym
            tiles.add(int(m.group(1)))
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, sym
            assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, sym
        assert tiles == {2, 3}, (name, sorted(kernels))


# ---- 4: argument checks that never reach the GPU --------------------------------------------------------------------------------
def test_forcing_a_shape_the_split_forms_lack_is_invalid(lib):
    fake = ctypes.c_void_p(4096)                                        # never dereferenced: validation fails first
    ok = np.array([0, 2, 5], dtype=np.int32)
    for N, K in ((1281, 28), (600, 49)):
        rc = lib.pb_fista_solve_grouped(fake, N, fake, N, 5, N, fake, K, K, fake, 2, ok.ctypes.data, fake, 1.0, None, fake, 10,
                                        fake, fake, 1 << 30, F | S, None)
        assert rc == -1 and b"matrix-pipe" in lib.pb_last_error() and b"GROUPED_SPLIT" in lib.pb_last_error()
    rc = lib.pb_fista_solve_grouped(fake, 600, fake, 600, 5, 600, fake, 28, 28, fake, 2, ok.ctypes.data, fake, 1.0, None, fake, 10,
                                    fake, fake, 1 << 30, F, None)      # without the flag: today's error and text
    assert rc == -1 and b"(129 .. 310 scans, K <= 33, n_done_dev given)" in lib.pb_last_error()
