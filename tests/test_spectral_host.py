"""CPU: the padding of the spectral operators (pybold/padding.py) against the reference's outputs
(tests/golden/spectral.npz), the divergence rule, a NumPy statement of the direct circular form the
device evaluates, and the argument checks of pb_spectral_conv / pb_spectral_corr (no kernel launch)."""
import ctypes
import os

import numpy as np
import pytest

from pybold_amd import convolution, padding

LENGTHS = (1, 2, 60, 99, 100, 300, 341, 342, 400, 405, 511, 513, 600, 995, 996, 1023, 1024, 1025, 2048, 2049)


@pytest.fixture(scope="module")
def g(golden):
    return golden("spectral")


def direct_form(c, x, retro):
    """out[i] = sum_{m<T} c[m] xp[(p_l + i -/+ m) mod L] over the padding's index map."""
    N = len(x)
    idx, p_l = padding.custom_padd_layout(N)
    L = idx.size
    xp = np.where(idx >= 0, x[np.maximum(idx, 0)], 0.0)
    i = np.arange(N)[:, None]
    m = np.arange(len(c))[None, :]
    return (c[None, :] * xp[(p_l + i + (m if retro else -m)) % L]).sum(axis=1)


def filt(k, N, deconvolve):
    L = padding.custom_padd_layout(N)[0].size
    return np.fft.irfft(1.0 / np.fft.rfft(k, L), L) if deconvolve else np.asarray(k)[:L]


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("N", LENGTHS)
def test_custom_padd_matches_reference(g, N):
    want = g["padidx_%d" % N]
    p_want = tuple(int(v) for v in g["padp_%d" % N])
    a, p = padding.custom_padd(np.arange(1, N + 1, dtype=np.float64))
    np.testing.assert_array_equal(a, want)
    assert (p if p != 0 else (0, 0)) == p_want
    x = g["x_%d" % N]
    xp, p = padding.custom_padd(x)
    assert np.log2(len(xp)).is_integer() and len(xp) >= 1024
    np.testing.assert_array_equal(padding.unpadd(xp, p), x)
    # the index map is the layout both custom_padd and the device path read
    idx, p_l = padding.custom_padd_layout(N)
    assert idx.dtype == np.int32 and idx.size == want.size
    np.testing.assert_array_equal(np.where(idx >= 0, idx + 1, 0), want)
    assert p_l == p_want[0]
    np.testing.assert_array_equal(idx[p_l:p_l + N], np.arange(N))


def test_custom_padd_list_and_arguments():
    arrays = [np.arange(300.0), np.arange(300.0) * 2.0]
    padded, p = padding.custom_padd(arrays)
    assert isinstance(padded, list) and p == padding.custom_padd(arrays[0])[1]
    np.testing.assert_array_equal(padded[1], 2.0 * padded[0])
    np.testing.assert_array_equal(padding.unpadd(padded, p)[1], arrays[1])
    # larger power of two, other zero runs
    a, p = padding.custom_padd(np.arange(1.0, 301.0), min_power_of_2=2048, min_zero_padd=10, zero_padd_ratio=0.1)
    assert len(a) == 2048 and p == (874, 874)
    np.testing.assert_array_equal(padding.unpadd(a, p), np.arange(1.0, 301.0))
    a, p = padding.custom_padd(np.ones(1024))
    assert p == 0 and len(a) == 1024
    with pytest.raises(ValueError, match="power of two"):
        padding.custom_padd(np.ones(10), min_power_of_2=1000)
    with pytest.raises(ValueError, match="512 samples padded to 1024"):
        padding.custom_padd(np.ones(512))
    with pytest.raises(ValueError):
        padding.custom_padd_layout(0)


def test_padd_unpadd_round_trips_and_errors():
    """The reference's own round trips (pybold/tests/test_padd.py) and its ValueErrors."""
    rng = np.random.RandomState(0)
    for N in (100, 128, 200, 256, 250, 300, 500, 600, 1000):
        s = rng.randn(N)
        for p in (10, 20, 214):
            for paddtype in ("left", "right", "center"):
                ps = padding.padd(s, p=p, paddtype=paddtype)
                assert len(ps) == N + p
                np.testing.assert_array_equal(padding.unpadd(ps, p=p, paddtype=paddtype), s)
        for p in ((5, 10), (20, 20), (214, 145), (3, 0)):
            ps = padding.padd(s, p=p, paddtype="center")
            assert (ps[:p[0]] == 0).all() and len(ps) == N + sum(p)
            np.testing.assert_array_equal(padding.unpadd(ps, p=p), s)
        ps, p = padding.custom_padd(s)
        np.testing.assert_array_equal(padding.unpadd(ps, p), s)
    s = np.arange(4.0)
    np.testing.assert_array_equal(padding.padd(s, 3, c=7.0), [7.0, 0, 1, 2, 3, 7, 7])
    assert padding.padd(s, 0) is s and padding.unpadd(s, 0) is s
    lst = padding.padd([s, s], 2, paddtype="left")
    assert isinstance(lst, list) and list(lst[1]) == [0, 0, 0, 1, 2, 3]
    for bad in ("middle", None):
        with pytest.raises(ValueError, match="paddtype"):
            padding.padd(s, 2, paddtype=bad)
        with pytest.raises(ValueError, match="paddtype"):
            padding.unpadd(s, 2, paddtype=bad)
    for side in ("left", "right"):
        with pytest.raises(ValueError, match="center"):
            padding.padd(s, (1, 2), paddtype=side)
        with pytest.raises(ValueError, match="center"):
            padding.unpadd(s, (1, 2), paddtype=side)


def test_divergence_rule_matches_reference(g):
    n, ks, want = g["div_n"], g["div_k"], g["div_matches"]
    got = np.array([[convolution.spectral_matches_causal(int(N), int(K)) for N in n] for K in ks])
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first disagreements (K, N): %s" % [(int(ks[a]), int(n[b])) for a, b in bad[:10]]
    # the rule as the documents state it (K >= 2)
    for K in (2, 30, 48, 64):
        for N in range(1, 4201):
            L = max(1024, 1 << (N - 1).bit_length())
            diverges = 342 <= N <= 512 or L - K + 1 < N <= L
            assert convolution.spectral_matches_causal(N, K) == (not diverges), (N, K)
    assert not convolution.spectral_matches_causal(512, 1) and convolution.spectral_matches_causal(400, 1)
    with pytest.raises(ValueError):
        convolution.spectral_matches_causal(300, 0)


@pytest.mark.parametrize("N", LENGTHS)
def test_direct_form_matches_reference(g, N):
    x = g["x_%d" % N]
    for K in (1, 30, 64):
        if "conv_%d_%d" % (N, K) not in g:
            continue
        k = g["k_%d" % K]
        assert rel(direct_form(filt(k, N, False), x, False), g["conv_%d_%d" % (N, K)]) < 1e-13
        assert rel(direct_form(filt(k, N, False), x, True), g["retro_%d_%d" % (N, K)]) < 1e-13


def test_direct_form_long_filters_and_deconvolution(g):
    for N, K in g["long_cases"]:
        x, k = g["x_%d" % N], g["k_%d" % K]
        assert K > N
        assert rel(direct_form(filt(k, N, False), x, False), g["conv_%d_%d" % (N, K)]) < 1e-13
        assert rel(direct_form(filt(k, N, False), x, True), g["retro_%d_%d" % (N, K)]) < 1e-13
    for f in ("hrf", "mild"):
        h = g["filt_" + f]
        for N in (2, 60, 300, 400, 405, 600, 996, 1024, 2049):
            x = g["x_%d" % N]
            assert rel(direct_form(filt(h, N, True), x, False), g["deconv_%d_%s" % (N, f)]) < 1e-12
            assert rel(direct_form(filt(h, N, True), x, True), g["rdeconv_%d_%s" % (N, f)]) < 1e-12


def test_spectral_operator_class_and_conv_and_linear_contract():
    """The spectral form of the reference's ConvAndLinear is SpectralConvAndLinear; ConvAndLinear keeps
    rejecting spectral_conv=True and names it."""
    import pybold_amd
    with pytest.raises(NotImplementedError, match="SpectralConvAndLinear"):
        pybold_amd.ConvAndLinear(pybold_amd.DiscretInteg(), np.ones(3), 10, spectral_conv=True)
    H = pybold_amd.SpectralConvAndLinear(pybold_amd.DiscretInteg(), [1.0, 0.5], 10)
    assert isinstance(H.M, pybold_amd.DiscretInteg) and H.k.dtype == np.float64 and list(H.k) == [1.0, 0.5]


# ---- C ABI argument checks: validation fails before anything reaches a device ----------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


@pytest.mark.parametrize("name", ["pb_spectral_conv", "pb_spectral_corr"])
def test_spectral_abi_rejects_bad_arguments(lib, name):
    fn = getattr(lib, name)
    fake = ctypes.c_void_p(4096)        # never dereferenced: validation fails first
    cases = [
        ((fake, 300, fake, 300, 4, 1100, fake, 1024, 0, fake, 30), b"N=1100"),    # N > L
        ((fake, 300, fake, 300, 4, 300, fake, 1024, 800, fake, 30), b"pad_left=800"),
        ((fake, 300, fake, 300, 4, 300, fake, 1024, -1, fake, 30), b"pad_left=-1"),
        ((fake, 300, fake, 300, 4, 300, fake, 1024, 362, fake, 0), b"T=0"),
        ((fake, 300, fake, 300, 4, 300, fake, 1024, 362, fake, 2000), b"T=2000"),  # T > L
        ((fake, 299, fake, 300, 4, 300, fake, 1024, 362, fake, 30), b"leading dimension"),
        ((fake, 9000, fake, 9000, 4, 9000, fake, 16384, 3692, fake, 8192), b"N=9000 with T=8192"),   # LDS
        ((None, 300, fake, 300, 4, 300, fake, 1024, 362, fake, 30), b"NULL"),
        ((fake, 300, fake, 300, 4, 300, None, 1024, 362, fake, 30), b"NULL"),
        ((fake, 300, fake, 300, 4, 300, fake, 1024, 362, None, 30), b"NULL"),
    ]
    for args, msg in cases:
        rc = fn(*args, None)
        assert rc == -1, (args, msg)
        assert msg in lib.pb_last_error(), (msg, lib.pb_last_error())
    # an empty batch is a no-op whatever the pointers are
    assert fn(None, 300, None, 300, 0, 300, None, 1024, 362, None, 30, None) == 0
