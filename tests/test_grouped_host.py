"""CPU-only: the unit table of the grouped calls (one HRF per parcel, rows contiguous by parcel) from the HOST build of
its planner -- csrc/plan.h: grouped_fill / grouped_table behind pb_fista_grouped_plan, the very functions the device
runs in grouped_table_kernel -- and the argument checks of the grouped entry points (no kernel is launched here)."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def check_table(sizes, per, table, first):
    """Every unit inside one parcel, every row exactly once and in order, short units only at the end of a parcel."""
    off = offsets_of(sizes)
    assert first.shape == (len(sizes) + 1,) and first[0] == 0 and first[-1] == len(table)
    assert len(table) == sum(-(-int(n) // per) for n in sizes)
    seen = np.zeros(int(off[-1]), dtype=np.int64)
    for u, (row0, rows, g) in enumerate(table):
        assert 0 <= g < len(sizes) and first[g] <= u < first[g + 1]
        assert 1 <= rows <= per
        assert off[g] <= row0 and row0 + rows <= off[g + 1]            # the unit's rows lie in ONE parcel
        seen[row0:row0 + rows] += 1
        if rows < per:                                                   # dead slots: only behind a parcel's last rows
            assert u == first[g + 1] - 1 and row0 + rows == off[g + 1]
        if u > first[g]:                                                 # a parcel's units follow one another
            assert row0 == table[u - 1][0] + per and table[u - 1][1] == per
        else:
            assert row0 == off[g]
    assert (seen == 1).all()                                             # every row exactly once


def test_wave_table_of_the_edge_sizes(lib):
    """Parcels of 1, 15, 16, 17 and 33 rows -- a lone problem, one short of a wave, exact, one over, two waves plus
    one -- are 1 + 1 + 1 + 2 + 3 = 8 waves."""
    from pybold_amd import solver
    sizes = [1, 15, 16, 17, 33]
    table, first = solver.grouped_wave_table(offsets_of(sizes))
    assert len(table) == 8 and list(first) == [0, 1, 2, 3, 5, 8]
    check_table(sizes, 16, table, first)
    assert [tuple(r) for r in table] == [(0, 1, 0), (1, 15, 1), (16, 16, 2), (32, 16, 3), (48, 1, 3), (49, 16, 4), (65, 16, 4),
                                         (81, 1, 4)]
    off = offsets_of(sizes).astype(np.int32)
    assert lib.pb_fista_grouped_waves(off.ctypes.data, 5, 82) == 8


def test_wave_table_empty_input_and_one_large_parcel(lib):
    from pybold_amd import solver
    table, first = solver.grouped_wave_table([0])                       # no parcel, no row
    assert table.shape == (0, 3) and list(first) == [0]
    table, first = solver.grouped_wave_table([0, 16384])
    assert len(table) == 1024 and list(first) == [0, 1024]
    check_table([16384], 16, table, first)
    table, first = solver.grouped_wave_table([0, 0, 5, 5])              # empty parcels have no unit
    assert [tuple(r) for r in table] == [(0, 5, 1)] and list(first) == [0, 0, 1, 1]


@pytest.mark.parametrize("per", [16, 49, 1])
def test_unit_tables_of_random_parcels(lib, per):
    """The same properties for uneven parcels and for the unit sizes the grouped normal equations use."""
    from pybold_amd import solver
    rng = np.random.RandomState(per)
    for trial in range(20):
        sizes = list(rng.randint(0, 70, size=rng.randint(1, 40)))
        table, first = solver.grouped_wave_table(offsets_of(sizes), per=per)
        check_table(sizes, per, table, first)
        assert len(table) <= int(sum(sizes)) // per + len(sizes)        # the bound the work buffers are sized with


def test_offsets_are_checked_before_anything_runs(lib):
    from pybold_amd import solver
    for bad in ([1, 5], [0, 5, 3], []):
        with pytest.raises(ValueError):
            solver.grouped_wave_table(bad)
    fake = ctypes.c_void_p(4096)                                        # never dereferenced: validation fails first
    off = np.array([0, 10, 5], dtype=np.int32)
    rc = lib.pb_fista_solve_grouped(fake, 150, fake, 150, 5, 150, fake, 27, 27, fake, 2, off.ctypes.data, fake, 1.0, None, fake, 10,
                                    fake, fake, 1 << 30, 0, None)
    assert rc == -1 and b"offsets" in lib.pb_last_error()
    rc = lib.pb_hrf_normal_eq_w_grouped(fake, 150, fake, 150, 5, 150, 27, 2, off.ctypes.data, fake, fake, 1 << 30, fake, 1000, None)
    assert rc == -1 and b"offsets" in lib.pb_last_error()
    ok = np.array([0, 2, 5], dtype=np.int32)
    rc = lib.pb_fista_solve_grouped(fake, 150, fake, 150, 5, 150, fake, 27, 27, fake, 2, ok.ctypes.data, fake, 1.0, None, fake, 10,
                                    fake, fake, 8, 0, None)
    assert rc == -1 and b"work buffer" in lib.pb_last_error()
    rc = lib.pb_fista_solve_grouped(fake, 128, fake, 128, 5, 128, fake, 27, 27, fake, 2, ok.ctypes.data, fake, 1.0, None, fake, 10,
                                    fake, fake, 1 << 30, 16384, None)   # PB_FLAG_FORCE_MFMA on 128 scans
    assert rc == -1 and b"matrix-pipe" in lib.pb_last_error()
    assert lib.pb_fista_grouped_work_len(82, 5, 27) >= 2 * 82 * 27 + 2 * 82 + 6 + 3 * 8
    assert lib.pb_hrf_normal_eq_w_grouped_work_len(82, 5, 27) >= 8 * (27 * 27 + 27 + 2)


def test_rows_are_sorted_by_label_once():
    from pybold_amd.parcels import sort_by_label
    labels = np.array([7, -2, 7, 100, -2, 7])
    distinct, order, offsets = sort_by_label(labels)
    assert list(distinct) == [-2, 7, 100] and list(offsets) == [0, 2, 5, 6]
    assert list(order) == [1, 4, 0, 2, 5, 3]                            # stable inside a parcel
