"""CPU-only checks of the 2:4-sparse near tiles of the plain one-wave matrix-pipe solve (csrc/mfma_sparse_tiles.h, through
`pb_mfma_sparse_tile`): the compressed values and position words decompress to exactly the split dense tile [C0 | -E] in
the column order the kernel's operands have; positions are ascending and distinct in every group of four; in float64 the
form  x_q = C0 w_q - E w_{q-1} + S sum_{b <= q-1} w_b  and its adjoint equal T_c w and T_c^T r; 33 taps are refused.
The parity tests of the kernel are in tests/test_gpu_sparse_tiles.py."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAN, SHIFT = 31, 9
NS = (129, 155, 156, 300, 310)
KS = (1, 2, 17, 30, 32)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not hasattr(ctypes.CDLL(_lib.LIB_PATH), "pb_mfma_sparse_tile"):
        ge.build()
    return _lib.load()


def taps_for(K):
    rng = np.random.RandomState(100 + K)
    h = rng.randn(K)
    if K == 17:
        h[0] = 0.0                       # an HRF that starts at zero: c[0] = 0, a structural nonzero that is numerically zero
    return h


def tile(lib, taps, pass_, par, r):
    hi = np.zeros((16, 32), np.uint16)
    lo = np.zeros((16, 32), np.uint16)
    idx = np.zeros((16, 4), np.uint16)
    c = np.zeros(64, np.float32)
    rc = lib.pb_mfma_sparse_tile(taps.ctypes.data, len(taps), pass_, par, r, hi.ctypes.data, lo.ctypes.data, idx.ctypes.data,
                                 c.ctypes.data)
    assert rc == 0, lib.pb_last_error()
    return hi.view(np.float16), lo.view(np.float16), idx, c


def rtz16(x):
    """float32 -> float16 rounded towards zero (v_cvt_pkrtz_f16_f32)."""
    h = np.float32(x).astype(np.float16)
    out = np.abs(h.astype(np.float32)) > np.abs(np.float32(x))
    bits = h.view(np.uint16).copy()
    bits[out] -= 1
    return bits.view(np.float16)


def dense_entry(c, pass_, own, ko, ki):
    """[C0 | -E] as csrc/mfma_sparse_tiles.h states it, in float32 like the builder."""
    S = np.float32(c[63])
    d = ko - ki if pass_ == 0 else ki - ko
    if own:
        if ko == 31:
            return np.float32(1.0) if ki == 31 else np.float32(2.0 ** -SHIFT)
        if ki == 31:
            return np.float32(S * np.float32(2.0 ** SHIFT))
        return np.float32(c[d]) if d >= 0 else np.float32(0.0)
    if ko == 31 or ki == 31:
        return np.float32(0.0)
    return np.float32(np.float32(c[min(31 + d, 63)]) - S)


def decompress(hi, lo, idx, par):
    """-> (own, other): two [16][32] float64 tiles (tile row, input slot) of hi + lo, the positions of every group, and
    the split parts laid out densely: [16][lane group][t][position]."""
    dh = np.zeros((16, 4, 4, 4), np.float16)
    dl = np.zeros((16, 4, 4, 4), np.float16)
    pos = np.zeros((16, 4, 4, 2), int)
    for rho in range(16):
        for kg in range(4):
            for p in range(4):
                gb, t = 2 * (kg & 1) + (p >> 1), 2 * (kg >> 1) + (p & 1)
                nib = (int(idx[rho, kg]) >> (4 * p)) & 15
                i0, i1 = nib & 3, nib >> 2
                pos[rho, gb, t] = (i0, i1)
                for i, j in ((i0, 2 * p), (i1, 2 * p + 1)):
                    dh[rho, gb, t, i] = hi[rho, 8 * kg + j]
                    dl[rho, gb, t, i] = lo[rho, 8 * kg + j]
    full = dh.astype(np.float64) + dl.astype(np.float64)
    own = np.zeros((16, 32))
    other = np.zeros((16, 32))
    for gb in range(4):
        for t in range(4):
            for s in range(2):
                own[:, 8 * gb + 2 * t + s] = full[:, gb, t, 2 * par + s]
                other[:, 8 * gb + 2 * t + s] = full[:, gb, t, 2 * (1 - par) + s]
    return own, other, pos, dh, dl


@pytest.mark.parametrize("K", KS)
def test_tiles_decompress_to_the_split_dense_tile(lib, K):
    taps = taps_for(K)
    for pass_ in (0, 1):
        for par in (0, 1):
            for r in (0, 1):
                hi, lo, idx, c = tile(lib, taps, pass_, par, r)
                assert (idx >> 16 == 0).all()
                _, _, pos, dh, dl = decompress(hi, lo, idx, par)
                assert (pos[..., 0] < pos[..., 1]).all(), "positions ascending and distinct in every group"
                want = np.zeros((16, 4, 4, 4), np.float32)
                for rho in range(16):
                    ko = 8 * (rho >> 2) + 4 * r + (rho & 3)
                    for gb in range(4):
                        for t in range(4):
                            for p4 in range(4):
                                want[rho, gb, t, p4] = dense_entry(c, pass_, (p4 >> 1) == par, ko, 8 * gb + 2 * t + (p4 & 1))
                wh = rtz16(want)
                wl = (want - wh.astype(np.float32)).astype(np.float16)
                assert (dh.view(np.uint16) == wh.view(np.uint16)).all() or (dh == wh).all(), "hi parts (round towards zero)"
                assert (dl == wl).all(), "lo parts (round to nearest of the exact rest)"
                assert (np.count_nonzero(want, axis=3) <= 2).all()


def full_tiles(lib, taps):
    """[pass][parity] -> (own, other) as [32][32] float64 (output slot, input slot)."""
    out = {}
    for pass_ in (0, 1):
        for par in (0, 1):
            own = np.zeros((32, 32))
            oth = np.zeros((32, 32))
            for r in (0, 1):
                hi, lo, idx, c = tile(lib, taps, pass_, par, r)
                o, x, _, _, _ = decompress(hi, lo, idx, par)
                for rho in range(16):
                    ko = 8 * (rho >> 2) + 4 * r + (rho & 3)
                    own[ko], oth[ko] = o[rho], x[rho]
            out[pass_, par] = (own, oth)
    return out, c.astype(np.float64)


@pytest.mark.parametrize("K", KS)
def test_the_form_equals_the_toeplitz_operator_in_float64(lib, K):
    """Blocks of 31 samples + sum slot, as the kernel walks them.  Every tile entry carries 22 bits (hi: 11 bits towards
    zero, lo: 11 bits to nearest of the rest: at most 2^-21 of the entry off, and E = S - c[.] is rounded once more in
    float32, 2^-24 of S); the float64 arithmetic of this test is far below that.  Bound: 2^-20 sum |entry| |input| per
    output, sums over the blocks before (behind) included."""
    taps = taps_for(K)
    tiles, c = full_tiles(lib, taps)
    for N in NS:
        nb = (N + SPAN - 1) // SPAN
        rng = np.random.RandomState(N + K)
        lag = np.subtract.outer(np.arange(N), np.arange(N))
        T = np.where(lag >= 0, c[np.clip(lag, 0, 63)], 0.0)
        for pass_ in (0, 1):
            v = rng.randn(N)
            vp = np.zeros(nb * SPAN)
            vp[:N] = v
            blocks = vp.reshape(nb, SPAN)
            want = T @ v if pass_ == 0 else T.T @ v
            bound_op = np.abs(T) @ np.abs(v) if pass_ == 0 else np.abs(T).T @ np.abs(v)
            got = np.zeros(nb * SPAN)
            run = 0.0                                    # the sum slot: 2^-9 times the sum of the blocks before (behind)
            order = range(nb) if pass_ == 0 else range(nb - 1, -1, -1)
            prev = np.zeros(32)
            for q in order:
                own, oth = tiles[pass_, q & 1]
                cur = np.concatenate([blocks[q], [run]])
                out = own @ cur + oth @ prev
                got[q * SPAN:(q + 1) * SPAN] = out[:SPAN]
                run = out[31]
                prev = cur
            err = np.abs(got[:N] - want)
            bound = 2.0 ** -20 * (bound_op + 2.0 * abs(c[63]) * np.abs(v).sum())
            assert (err <= bound).all(), "pass %d N=%d K=%d: %.3e above the bound by %.3e" % (pass_, N, K, err.max(), (err - bound).max())
            assert err.max() < 1e-5 * np.abs(want).max()


def test_33_taps_and_bad_arguments_are_refused(lib):
    buf = np.zeros(16 * 32, np.uint16)
    idx = np.zeros(64, np.uint16)
    for K in (33, 34, 64):
        taps = np.random.RandomState(K).randn(K)
        rc = lib.pb_mfma_sparse_tile(taps.ctypes.data, K, 0, 0, 0, buf.ctypes.data, buf.ctypes.data, idx.ctypes.data, None)
        assert rc == -1 and b"1..32" in lib.pb_last_error()
    taps = np.ones(4)
    assert lib.pb_mfma_sparse_tile(taps.ctypes.data, 0, 0, 0, 0, buf.ctypes.data, buf.ctypes.data, idx.ctypes.data, None) == -1
    assert lib.pb_mfma_sparse_tile(taps.ctypes.data, 4, 2, 0, 0, buf.ctypes.data, buf.ctypes.data, idx.ctypes.data, None) == -1
    assert lib.pb_mfma_sparse_tile(taps.ctypes.data, 4, 0, 0, 0, None, buf.ctypes.data, idx.ctypes.data, None) == -1
    assert lib.pb_mfma_sparse_tile(taps.ctypes.data, 4, 1, 1, 1, buf.ctypes.data, buf.ctypes.data, idx.ctypes.data, None) == 0


def test_the_flag_and_the_force_names(lib):
    from pybold_amd import _lib, solver
    header = open(os.path.join(ROOT, "include", "pybold_hip.h")).read()
    assert _lib.PB_FLAG_MFMA_DENSE_TILES == 1 << 22 and "PB_FLAG_MFMA_DENSE_TILES = %d" % (1 << 22) in header
    taken = [getattr(_lib, n) for n in dir(_lib) if n.startswith("PB_FLAG_") and n != "PB_FLAG_MFMA_DENSE_TILES"]
    assert all(v & (1 << 22) == 0 for v in taken)
    assert solver._FORCE["dense_tiles"] == _lib.PB_FLAG_MFMA_DENSE_TILES
    assert solver._FORCE["mfma_dense"] == solver._FORCE["mfma"] | _lib.PB_FLAG_MFMA_DENSE_TILES
    # the form code and its name do not tell the two kernels apart (callers key on them)
    assert lib.pb_fista_which_kernel(300, 30, 100000, 0, 0, 6) == 4
