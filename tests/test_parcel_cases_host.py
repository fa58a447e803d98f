"""CPU-only checks of tests/parcel_cases.py, the inputs behind tests/test_gpu_parcels_variants.py: the parcel layout, the
conditions every grouped z-step case must meet -- properties of the float64 oracle's output, so that a row the matrix
pipe hands back or misses is the kernel's doing --, the shape lists against the ranges of the compiled instances, and the
two host rules of the grouped normal equations restated there against the library's own queries.  No kernel is launched."""
import ctypes
import os

import numpy as np
import pytest

from oracle import c_oracle
from tests import parcel_cases as pc


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_layout_has_empty_parcels_first_last_and_as_neighbours(lib):
    from pybold_amd import solver
    assert len(pc.SIZES) == 10 and pc.ROWS == 84
    assert pc.SIZES[0] == 0 and pc.SIZES[-1] == 0 and pc.SIZES[3] == pc.SIZES[4] == 0
    assert len(pc.NONEMPTY) == len(pc.THETAS) == len(pc.GAINS) == 6
    table, first = solver.grouped_wave_table(pc.OFFSETS)
    assert len(table) == 9                                               # 1 + 1 + 1 + 2 + 3 + 1 waves
    assert sorted(set(int(g) for g in table[:, 2])) == pc.NONEMPTY
    assert list(first) == [0, 0, 1, 2, 2, 2, 3, 5, 8, 9, 9]


def test_shape_lists_sit_on_the_edges_of_the_compiled_instances(lib):
    """31 (NB - 1) < N <= 31 NB for NB = 5 .. 10 (pick_mfma_grouped, csrc/dispatch.h); the shapes listed as having no
    matrix-pipe form are refused when forced, before anything is launched."""
    assert sorted(pc.NB_RANGE) == [5, 6, 7, 8, 9, 10]
    for nb, (lo, hi) in pc.NB_RANGE.items():
        assert lo == 31 * (nb - 1) + 1 + (4 if nb == 5 else 0) and hi == 31 * nb       # (NB = 5 starts at 129 scans)
    assert len(pc.INSTANCE_SHAPES) == 40 and len(set(pc.INSTANCE_SHAPES)) == 40
    assert len(pc.BIT_SHAPES) == 24 and len(pc.LAYOUT_SHAPES) == 6      # the twelve edge lengths at 32 and at 33 taps
    assert [k for _, k in pc.LAYOUT_SHAPES] == [33, 32, 33, 32, 33, 32]
    fake = ctypes.c_void_p(4096)                                         # never dereferenced: the shape is refused first
    off = pc.OFFSETS.astype(np.int32)
    force_mfma = 16384                                                   # PB_FLAG_FORCE_MFMA
    from pybold_amd import _lib
    assert _lib.PB_FLAG_FORCE_MFMA == force_mfma
    for n, k in pc.VECTOR_SHAPES:
        rc = lib.pb_fista_solve_grouped(fake, n, fake, n, pc.ROWS, n, fake, k, k, fake, len(pc.SIZES), off.ctypes.data, fake, 1.0,
                                        None, fake, 10, fake, fake, 1 << 30, force_mfma, None)
        assert rc == -1 and b"matrix-pipe" in lib.pb_last_error(), (n, k)


@pytest.mark.parametrize("N,K", [(150, 27), (129, 1), (31, 4), (310, 33)])
def test_taps_steps_and_gains(N, K):
    taps, steps, gains = pc.parcel_taps(K, N)
    assert taps.shape == (10, K) and steps.shape == gains.shape == (10,)
    empty = [g for g in range(10) if g not in pc.NONEMPTY]
    assert np.isnan(taps[empty]).all() and np.isnan(steps[empty]).all()   # nothing may read them
    assert np.isfinite(taps[pc.NONEMPTY]).all() and (steps[pc.NONEMPTY] > 0).all()
    assert list(gains[pc.NONEMPTY]) == pc.GAINS
    peak = np.abs(taps[pc.NONEMPTY]).max(axis=1)
    assert peak.max() / peak.min() > 1e5                                  # gains over five orders of magnitude ...
    assert min(pc.GAINS) < 0.0 < max(pc.GAINS)                            # ... and of either sign


@pytest.mark.parametrize("variant", pc.VARIANTS)
@pytest.mark.parametrize("N,K", pc.ALL_Z_SHAPES)
def test_input_conditions_of_every_z_step_case(N, K, variant):
    """Every reference row is non-zero; lambda_row x step <= 0.005 max|w_ref| on every row (a quarter of the accuracy
    guard's MFMA_RHO_MAX = 0.02); |h[K - 1]| >= 0.01 max|h| for every HRF of two taps or more."""
    case = pc.z_step_case(N, K, variant)
    assert case["Y"].dtype == np.float32 and case["Y"].shape == case["ref"].shape == (pc.ROWS, N)
    assert (case["W0"] is None) == (variant == "cold") and (np.ndim(case["lbda"]) == 0) == (variant == "cold")
    smallest_norm, guard_ratio, tail_share = pc.input_conditions(case)
    assert np.isfinite(case["ref"]).all() and smallest_norm > 0.0
    assert guard_ratio <= pc.GUARD_RATIO_MAX, guard_ratio
    if K >= 2:
        assert tail_share >= pc.TAIL_SHARE_MIN, tail_share


@pytest.mark.parametrize("N,K", [s for s in pc.BIT_SHAPES if s[0] in (129, 310)] + [(155, 2), (156, 17)])
def test_the_last_tap_moves_the_oracle(N, K):
    """A tap loop that ends one short must show: with the last tap zeroed (same steps, same lambda) the oracle's iterate
    moves by more than 1e-4 relative on every row, ten times the bound the GPU tests assert."""
    case = pc.z_step_case(N, K, "warm")
    off = pc.OFFSETS
    for g in pc.NONEMPTY:
        r0, r1 = int(off[g]), int(off[g + 1])
        h = case["taps"][g].copy()
        h[-1] = 0.0
        cut = c_oracle.fista_batch(case["Y"][r0:r1].astype(np.float64), h, case["lbda_rows"][r0:r1].copy(), float(case["steps"][g]),
                                   case["n_iter"], W0=case["W0"][r0:r1], threads=1)[0]
        ref = case["ref"][r0:r1]
        moved = np.linalg.norm(cut - ref, axis=1) / np.linalg.norm(ref, axis=1)
        assert moved.min() > 1e-4, (g, moved.min())


# ---- the grouped normal equations ----------------------------------------------------------------------------------
def test_rows_per_unit_restated(lib):
    """`ne_rows_per_unit` against the library: the work buffer pb_hrf_normal_eq_w_grouped asks for is sized from the
    units of that rule, and the planner's table for those units fits the bound."""
    from pybold_amd import solver
    assert [pc.ne_rows_per_unit(v) for v in (0, 84, 16384, 16385, 17408, 17409, 20000)] == [16, 16, 16, 17, 17, 18, 20]
    for sizes, K in [(pc.SIZES, 27), ([16384], 5), ([16385], 5), (pc.NE_UNIT20_SIZES, 5), (pc.ne_raised_sizes(), 27), ([40000, 0, 3], 2)]:
        V, G = int(sum(sizes)), len(sizes)
        assert lib.pb_hrf_normal_eq_w_grouped_work_len(V, G, K) == pc.ne_work_len(V, G, K), (sizes, K)
        off = np.concatenate([[0], np.cumsum(sizes)])
        per = pc.ne_rows_per_unit(V)
        table, first = solver.grouped_wave_table(off, per=per)
        assert len(table) == sum(-(-n // per) for n in sizes) <= V // per + G
    assert pc.ne_case_e_log2(pc.NE_UNIT20_SIZES, 5)[2] == 20
    assert all(pc.ne_case_e_log2(sizes, K)[2] == 16 for name, sizes, N, K in pc.NE_REDUCE_CASES if name != "unit20")


def test_reduce_cases_land_on_every_width():
    """The second stage's entries per workgroup: the cases of the GPU test reach 2^8, 2^6, 2^4, 2^2 and 2^0, both sides
    of every threshold in units of the largest parcel, and the value raised for the grid's sake."""
    seen = {}
    for name, sizes, N, K in pc.NE_REDUCE_CASES:
        seen[name] = pc.ne_case_e_log2(sizes, K)
    assert [seen["ladder-%d" % b][1] for b in pc.NE_LADDER] == [6, 6, 6, 4, 4, 2, 2, 0]      # (the 70-row parcel: 5 units at least)
    assert seen["raised"][:2] == (0, 1)                                  # 100 parcels x 758 entries > 65 536 workgroups
    assert seen["unit20"][:2] == (0, 0)                                  # 500 units of 20 rows
    assert pc.ne_case_e_log2(pc.SIZES, 27)[:2] == (8, 8)                 # the layout of the kernel-selection cases: 3 units
    widths = {v[1] for v in seen.values()} | {pc.ne_case_e_log2(pc.SIZES, 27)[1]}
    assert widths == {8, 6, 4, 2, 1, 0}
    assert pc.reduce_e_log2(4, 1, 32) == 8 and pc.reduce_e_log2(5, 1, 32) == 6 and pc.reduce_e_log2(257, 65536, 1) == 0
    assert pc.reduce_e_log2(257, 86, 758) == 0 and pc.reduce_e_log2(257, 87, 758) == 1 and pc.reduce_e_log2(257, 70000, 758) == 8


def test_kernel_selection_shapes():
    """The three kernels of pb_hrf_normal_eq_w_grouped: the register form, the generic wave form on either side of each
    of its limits (K^2 <= 768, N <= 320), the sum form for 33 taps and -- 2 069 scans at 32 taps, the first length whose
    wave-form LDS (20 002 doubles) exceeds the 20 000 allowed -- below 33 taps."""
    assert [pc.ne_kernel(n, k) for n, k in pc.NE_KERNEL_SHAPES] == ["register", "wave", "wave", "wave", "sum", "register", "sum"]
    assert pc.NE_SUM_BELOW_33 == (2069, 32)
    assert pc.ne_wave_lds_doubles(2068, 32) <= pc.NE_LDS_DOUBLES_MAX < pc.ne_wave_lds_doubles(2069, 32)
    assert pc.ne_sum_lds_doubles(2069, 32) <= pc.NE_LDS_DOUBLES_MAX       # ... and the sum form carries it
    assert pc.ne_kernel(320, 27) == "register" and pc.ne_kernel(150, 33) == "sum"
