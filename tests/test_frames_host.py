"""CPU-only part of the layout tests: the framed-buffer helper (tests/frames.py) on host tensors -- its own self-test:
a bit flipped anywhere outside the window is caught and named -- and the refusal of leading dimensions smaller than
the row, on pointers that are never dereferenced.  The device part is tests/test_gpu_layout.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import frames
from frames import Frame1D, Frame2D

CPU = torch.device("cpu")


# ---- the helper ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int32, torch.int64])
def test_window_shape_stride_offset_and_sentinel(dtype):
    data = np.arange(5 * 7).reshape(5, 7)
    f = Frame2D(5, 7, dtype, CPU, left=3, right=18, guard_rows=2, fill=data)
    assert tuple(f.view.shape) == (5, 7) and f.view.stride() == (28, 1) and f.ld == 28
    assert tuple(f.buf.shape) == (9, 28)
    assert f.view.storage_offset() == 2 * 28 + 3
    assert f.ptr == f.buf.data_ptr() + (2 * 28 + 3) * f.buf.element_size()
    assert torch.equal(f.view, torch.from_numpy(data).to(dtype))
    assert torch.equal(f.contiguous(), torch.from_numpy(data).to(dtype)) and f.contiguous().is_contiguous()
    # everything outside the window is the sentinel; a float sentinel is a NaN
    outside = f.ibuf[~f._mask]
    assert (outside == frames._signed(frames.SENTINEL_BITS[dtype], dtype)).all() and outside.numel() == 9 * 28 - 35
    if dtype.is_floating_point:
        assert torch.isnan(f.buf[~f._mask]).all()
    # an output window is the sentinel too
    out = Frame2D(5, 7, dtype, CPU, left=1, right=4, guard_rows=2)
    assert bool(out.is_sentinel().all()) and tuple(out.is_sentinel().shape) == (5, 7)
    g = Frame1D(11, dtype, CPU, guard=64, fill=np.arange(11))
    assert tuple(g.view.shape) == (11,) and g.view.storage_offset() == 64 and g.buf.numel() == 11 + 128
    assert g.ptr == g.buf.data_ptr() + 64 * g.buf.element_size()
    assert torch.equal(g.contiguous(), torch.arange(11).to(dtype))


def test_layout_constants():
    """y: an offset that is no multiple of 4 elements and an odd total pad (row starts alternate in alignment); the
    guard of a vector keeps an int32 workspace 8-byte aligned."""
    left, right = frames.LAYOUT["y"]
    assert left % 4 != 0 and (left + right) % 2 == 1
    y = frames.frame2d("y", 4, 300, torch.float32, CPU, fill=np.zeros((4, 300)))
    starts = [(y.ptr + r * y.ld * 4) % 16 for r in range(4)]
    assert len(set(starts)) == 4 and all(s % 4 == 0 for s in starts)        # every alignment a float32 row can have
    assert frames.LAYOUT["W"] == (1, 4) and frames.LAYOUT["J"] == (1, 2) and frames.LAYOUT["taps_pp"] == (1, 2)
    assert frames.GUARD_ROWS == 2 and frames.GUARD_1D == 64 and frames.GUARD_1D % 2 == 0
    w = frames.frame1d("work", 10, torch.int32, CPU)
    assert (w.ptr - w.buf.data_ptr()) % 8 == 0
    p = frames.frame2d("W", 3, 5, torch.float64, CPU, packed=True)
    assert p.ld == 5 and tuple(p.buf.shape) == (3, 5) and p.ptr == p.buf.data_ptr()


def _flip(f, *cell):
    f.ibuf[cell] = f.ibuf[cell] ^ 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int32])
@pytest.mark.parametrize("cell,region,named", [((4, 2), "left pad", "(row 2, column -1)"), ((2, 10), "right pad", "(row 0, column 7)"),
                                               ((1, 5), "guard row", "(row -1, column 2)"), ((7, 0), "guard row", "(row 5, column -3)"),
                                               ((6, 27), "right pad", "(row 4, column 24)")])
def test_one_flipped_bit_outside_the_window_is_caught_and_named(dtype, cell, region, named):
    f = Frame2D(5, 7, dtype, CPU, left=3, right=18, guard_rows=2).snapshot()
    f.assert_outside_untouched()
    f.assert_untouched()
    _flip(f, *cell)
    for check in (f.assert_outside_untouched, f.assert_untouched):
        with pytest.raises(AssertionError) as e:
            check()
        assert named in str(e.value) and region in str(e.value), str(e.value)


@pytest.mark.parametrize("dtype", [torch.float64, torch.int32, torch.int64])
def test_one_flipped_bit_in_a_vector_guard_is_caught_and_named(dtype):
    for pos, named in ((63, "element -1"), (64 + 11, "element 11"), (0, "element -64")):
        f = Frame1D(11, dtype, CPU, guard=64).snapshot()
        _flip(f, pos)
        with pytest.raises(AssertionError) as e:
            f.assert_outside_untouched()
        assert named in str(e.value) and "guard" in str(e.value), str(e.value)


def test_a_write_inside_the_window_is_an_output_not_an_offence():
    f = Frame2D(5, 7, torch.float64, CPU, left=1, right=4, guard_rows=2).snapshot()
    f.view[:] = 1.5
    f.view[4, 6] = float("nan")
    f.assert_outside_untouched()
    assert not bool(f.is_sentinel().any())
    with pytest.raises(AssertionError) as e:                # ... but an input must not change even there
        f.assert_untouched()
    assert "(row 0, column 0)" in str(e.value) and "inside the window" in str(e.value)
    g = Frame1D(3, torch.int32, CPU, guard=64).snapshot()
    g.view[2] = 7
    g.assert_outside_untouched()
    with pytest.raises(AssertionError, match="element 2"):
        g.assert_untouched()
    # NaN to the SAME NaN is no change; NaN with another payload is one (value comparison would see neither)
    h = Frame2D(2, 2, torch.float32, CPU, left=1, right=1, guard_rows=1).snapshot()
    h.ibuf[0, 0] = frames._signed(frames.SENTINEL_BITS[torch.float32], torch.float32)
    h.assert_untouched()
    h.ibuf[0, 0] = 0x7FC00000
    with pytest.raises(AssertionError, match="guard row"):
        h.assert_untouched()


# ---- leading dimensions smaller than the row are refused before anything touches a device ------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


N, K, P, NI = 300, 30, 8, 40
FAKE = ctypes.c_void_p(4096)            # never dereferenced: validation must fail first


def _refused(lib, rc, word):
    msg = lib.pb_last_error()
    assert rc == -1 and word in msg, (rc, msg)


def test_small_leading_dimensions_are_refused(lib):
    """ldy = N - 1, ldw = N - 1, ldj = n_iter - 1, ldt = K - 1: PB_ERR_INVALID from every solver entry point that takes
    them.  Every one of these entry points validates its sizes before its first HIP call (pb_fista_solve_ex and
    pb_fista_solve_path in solve_impl, whose first device query is the route's; the others in their own bodies), so the
    fake pointers are never read and no check had to be left out."""
    taps = np.ones(K)
    th = taps.ctypes.data

    def ex(ldy=N, ldw=N, ldj=NI, J=FAKE):
        return lib.pb_fista_solve_ex(FAKE, ldy, 1, FAKE, ldw, P, N, th, FAKE, K, 1.0, 1.0, None, FAKE, NI, J, ldj, 0, 0.0, 6,
                                     FAKE, 0, None, None, 0.0, None, 0)

    def d(ldy=N, ldw=N, ldj=NI, J=FAKE):
        return lib.pb_fista_solve_d(FAKE, ldy, 1, FAKE, ldw, P, N, th, FAKE, K, 1.0, 1.0, None, FAKE, NI, J, ldj, 0, 0.0, 6,
                                    FAKE, 0, None)

    def pp(ldy=N, ldw=N, ldt=K):
        return lib.pb_fista_solve_pp(FAKE, ldy, FAKE, ldw, P, N, FAKE, ldt, K, FAKE, 1.0, None, FAKE, NI, 0, 0.0, FAKE, 0, None)

    def path(ldy=N, ldw=N):
        return lib.pb_fista_solve_path(FAKE, ldy, 1, FAKE, ldw, P, N, th, FAKE, K, 1.0, FAKE, FAKE, 0.0, FAKE, NI, FAKE, None, 0,
                                       0, None)

    def bt(ldy=N, ldw=N):
        return lib.pb_fista_solve_backtrack_d(FAKE, ldy, 1, FAKE, ldw, P, N, FAKE, K, 1.0, 0.5, 40, 1.0, None, FAKE, NI, None,
                                              None, None, 0, None)

    for fn in (ex, d, pp, path, bt):
        _refused(lib, fn(ldy=N - 1), b"leading dimension")
        _refused(lib, fn(ldw=N - 1), b"leading dimension")
        _refused(lib, fn(ldy=0), b"leading dimension")
    for fn in (ex, d):                                       # the entry points with a cost trace
        _refused(lib, fn(ldj=NI - 1), b"ldj")
        _refused(lib, fn(ldj=0), b"ldj")
        _refused(lib, fn(ldy=N - 1, J=None, ldj=0), b"leading dimension")
    _refused(lib, pp(ldt=K - 1), b"leading dimension")      # (ldt = 0 means ONE shared HRF: only a non-zero ldt < K is wrong)
    _refused(lib, pp(ldt=1), b"leading dimension")
    _refused(lib, pp(ldt=-1), b"leading dimension")
    from pybold_amd import _lib
    with pytest.raises(_lib.PyboldHipError, match="leading dimension"):
        _lib.check(ex(ldw=N - 1), "pb_fista_solve_ex")
