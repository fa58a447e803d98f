"""GPU: the spectral operators (pb_spectral_conv / pb_spectral_corr) against the reference's padded-FFT
functions (tests/golden/spectral.npz, operators.npz), SpectralConvAndLinear, the reference's
deconv output x at lengths where it is not the causal FIR, and a large batch against torch.fft."""
import numpy as np
import pytest
import torch

import pybold_amd
from pybold_amd import _lib, padding, solver

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 60, 99, 100, 300, 341, 342, 400, 405, 511, 513, 600, 995, 996, 1023, 1024, 1025, 2048, 2049)
CONV_TOL, DECONV_TOL = 1e-12, 1e-11


@pytest.fixture(scope="module")
def g(golden):
    assert torch.cuda.is_available()
    return golden("spectral")


def rel(a, b):
    return np.abs(np.asarray(a) - b).max() / np.abs(b).max()


@pytest.mark.parametrize("N", LENGTHS)
def test_convolve_forms_match_reference(g, N):
    x = g["x_%d" % N]
    for K in (1, 30, 64):
        if "conv_%d_%d" % (N, K) in g:
            k = g["k_%d" % K]
            assert rel(pybold_amd.spectral_convolve(k, x), g["conv_%d_%d" % (N, K)]) <= CONV_TOL
            assert rel(pybold_amd.spectral_retro_convolve(k, x), g["retro_%d_%d" % (N, K)]) <= CONV_TOL
    for N2, K in g["long_cases"]:                       # filters longer than the series (and than L)
        x2, k = g["x_%d" % N2], g["k_%d" % K]
        assert rel(pybold_amd.spectral_convolve(k, x2), g["conv_%d_%d" % (N2, K)]) <= CONV_TOL
        assert rel(pybold_amd.spectral_retro_convolve(k, x2), g["retro_%d_%d" % (N2, K)]) <= CONV_TOL


@pytest.mark.parametrize("f", ["hrf", "mild"])
def test_deconvolve_forms_match_reference(g, f):
    h = g["filt_" + f]
    for N in (2, 60, 300, 400, 405, 600, 996, 1024, 2049):
        x = g["x_%d" % N]
        assert rel(pybold_amd.spectral_deconvolve(h, x), g["deconv_%d_%s" % (N, f)]) <= DECONV_TOL, N
        assert rel(pybold_amd.spectral_retro_deconvolve(h, x), g["rdeconv_%d_%s" % (N, f)]) <= DECONV_TOL, N


def test_operators_fixture_spectral_keys(golden):
    """The five _spec cases of operators.npz (97-600 scans, one of them wrapping: 600 taps at 600 scans)."""
    o = golden("operators")
    for tag in "abcde":
        k, x = o[tag + "_k"], o[tag + "_x"]
        assert rel(pybold_amd.spectral_convolve(k, x), o[tag + "_spec"]) <= CONV_TOL
        assert rel(pybold_amd.spectral_retro_convolve(k, x), o[tag + "_spec_retro"]) <= CONV_TOL


def test_batches_equal_row_calls_and_stay_on_device(g):
    k, h = g["k_30"], g["filt_hrf"]
    for N in (300, 405, 1024):
        X = np.stack([g["x_%d" % N], -0.5 * g["x_%d" % N], np.linspace(-1, 1, N)])
        Xd = torch.from_numpy(X).cuda()
        for fn, c in ((pybold_amd.spectral_convolve, k), (pybold_amd.spectral_retro_convolve, k),
                      (pybold_amd.spectral_deconvolve, h), (pybold_amd.spectral_retro_deconvolve, h)):
            B = fn(c, X)
            assert isinstance(B, np.ndarray) and B.shape == X.shape and B.dtype == np.float64
            for r in range(len(X)):
                np.testing.assert_array_equal(B[r], fn(c, X[r]))
            T = fn(c, Xd)
            assert torch.is_tensor(T) and T.is_cuda and T.dtype == torch.float64 and T.shape == Xd.shape
            np.testing.assert_array_equal(T.cpu().numpy(), B)
            t1 = fn(c, Xd[1])
            assert torch.is_tensor(t1) and t1.is_cuda and t1.dim() == 1
    # a strided view of rows is accepted
    Xd = torch.from_numpy(np.stack([g["x_400"]] * 4)).cuda()[::2]
    np.testing.assert_array_equal(pybold_amd.spectral_convolve(k, Xd).cpu().numpy()[1],
                                  pybold_amd.spectral_convolve(k, g["x_400"]))


def test_spectral_conv_and_linear(g):
    """op = spectral_convolve(k, M.op(x)), adj = M.adj(spectral_retro_convolve(k, x)): the reference's
    ConvAndLinear(..., spectral_conv=True) (pybold/linear.py:88-89,108-109); the output keeps the input's length,
    dim_in / dim_out unused."""
    h = g["dc_405_hrf"]
    for N in (300, 405, 996):
        x = g["x_%d" % N]
        H = pybold_amd.SpectralConvAndLinear(pybold_amd.DiscretInteg(), h, dim_in=N, dim_out=N)
        want_op = pybold_amd.spectral_convolve(h, np.cumsum(x))
        want_adj = np.cumsum(pybold_amd.spectral_retro_convolve(h, x)[::-1])[::-1]
        assert rel(H.op(x), want_op) <= CONV_TOL and rel(H.adj(x), want_adj) <= CONV_TOL
        assert H.op(x).shape == (N,)
        # dimensions unused, tensors in / tensors out
        Hm = pybold_amd.SpectralConvAndLinear(pybold_amd.DiscretInteg(), h, dim_in=7)
        Xd = torch.from_numpy(np.stack([x, 2 * x])).cuda()
        T = Hm.op(Xd)
        assert torch.is_tensor(T) and T.is_cuda and T.shape == Xd.shape
        assert rel(T.cpu().numpy()[1], 2 * want_op) <= CONV_TOL
        # the causal operator where the divergence rule says the two agree, a different one elsewhere
        Hc = pybold_amd.ConvAndLinear(pybold_amd.DiscretInteg(), h, dim_in=N, dim_out=N)
        if pybold_amd.spectral_matches_causal(N, len(h)):
            assert rel(H.op(x), Hc.op(x)) < 1e-12 and rel(H.adj(x), Hc.adj(x)) < 1e-12
        else:
            assert rel(H.op(x), Hc.op(x)) > 1e-6
    np.random.seed(3)
    H = pybold_amd.SpectralConvAndLinear(pybold_amd.DiscretInteg(), h, dim_in=405)
    rho = pybold_amd.spectral_radius_est(H, (405,))
    assert np.isfinite(rho) and rho > 0


@pytest.mark.parametrize("N", [400, 405])
def test_reference_deconv_x_reproduced(g, N):
    """The reference's deconv returns x = spectral_convolve(hrf, z) (bold_signal.py:75): at 400 / 405 scans
    that is not the causal FIR of z.  Reproduced from the reference's z and from pybold_amd.deconv's own z."""
    pre = "dc_%d_" % N
    y, h, z, x = g[pre + "y"], g[pre + "hrf"], g[pre + "z"], g[pre + "x"]
    assert not pybold_amd.spectral_matches_causal(N, len(h))
    assert np.linalg.norm(pybold_amd.simple_convolve(h, z) - x) / np.linalg.norm(x) > 1e-2
    xs = pybold_amd.spectral_convolve(h, z)
    assert np.linalg.norm(xs - x) / np.linalg.norm(x) <= 1e-12
    np.random.seed(int(g[pre + "seed"]))
    _, z_own, _, _, _, _ = pybold_amd.deconv(y, float(g[pre + "tr"]), h, lbda=1.0, nb_iter=200, early_stopping=False)
    x_own = pybold_amd.spectral_convolve(h, z_own)
    assert np.linalg.norm(x_own - x) / np.linalg.norm(x) <= 1e-5


def test_large_batch_against_torch_fft():
    """V = 100 000 rows of 400 scans (a divergent length): sampled rows against a float64 torch.fft
    statement of the reference (gather-pad, rfft, multiply, irfft, slice)."""
    V, N = 100_000, 400
    gen = torch.Generator(device="cuda").manual_seed(11)
    X = torch.randn((V, N), dtype=torch.float64, device="cuda", generator=gen)
    k = np.random.RandomState(5).randn(30)
    idx, p_l = padding.custom_padd_layout(N)
    L = idx.size
    rows = torch.tensor([0, 1, 17, 4095, 4096, 65535, 77777, V - 1], device="cuda")
    idx_d = torch.from_numpy(idx.astype(np.int64)).cuda()
    xp = torch.where(idx_d >= 0, X[rows][:, idx_d.clamp(min=0)], torch.zeros((), dtype=torch.float64, device="cuda"))
    K = torch.fft.rfft(torch.from_numpy(k).cuda(), n=L)
    Xf = torch.fft.rfft(xp, n=L)
    for fn, spec in ((pybold_amd.spectral_convolve, K), (pybold_amd.spectral_retro_convolve, K.conj())):
        out = fn(k, X)
        assert out.shape == (V, N) and bool(torch.isfinite(out).all())
        want = torch.fft.irfft(Xf * spec, n=L)[:, p_l:p_l + N]
        err = ((out[rows] - want).abs().max() / want.abs().max()).item()
        assert err <= CONV_TOL, err


def test_bad_arguments_raise():
    x = torch.zeros((2, 300), dtype=torch.float64, device="cuda")
    idx, p_l = padding.custom_padd_layout(300)
    with pytest.raises(_lib.PyboldHipError, match="pad_left"):
        solver.spectral(x, idx, 1000, np.ones(30))
    with pytest.raises(_lib.PyboldHipError, match="T=2000"):
        solver.spectral(x, idx, p_l, np.ones(2000))
    with pytest.raises(_lib.PyboldHipError, match="N=300"):
        solver.spectral(x, idx[:200], 0, np.ones(3), corr=True)
    big = torch.zeros((1, 9000), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.PyboldHipError, match="exceeds LDS"):
        pybold_amd.spectral_deconvolve(np.ones(3), big)
    with pytest.raises(ValueError, match="512 samples"):
        pybold_amd.spectral_convolve(np.ones(3), np.ones(512))
    with pytest.raises(ValueError, match="empty kernel"):
        pybold_amd.spectral_convolve(np.ones(0), np.ones(300))
    with pytest.raises(TypeError):
        solver.spectral(x.float(), idx, p_l, np.ones(3))
    # a map with entries outside [0, N) reads them as zeros
    bad = idx.copy()
    bad[bad < 0] = 10 ** 6
    bad[:5] = -7
    xr = torch.from_numpy(np.random.RandomState(1).randn(1, 300)).cuda()
    np.testing.assert_array_equal(solver.spectral(xr, bad, p_l, np.ones(30)).cpu().numpy(),
                                  solver.spectral(xr, idx, p_l, np.ones(30)).cpu().numpy())
    # a zero bin of the filter spectrum gives non-finite output, as in the reference (1 / rfft(k, L))
    with np.errstate(divide="ignore", invalid="ignore"):
        assert not np.isfinite(pybold_amd.spectral_deconvolve(np.array([1.0, 1.0]), np.ones(300))).all()
