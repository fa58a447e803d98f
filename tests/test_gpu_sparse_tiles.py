"""GPU tests of the plain one-wave matrix-pipe solve on 2:4-sparse near tiles (fista_mfma_sparse_kernel: both near tiles of
a block in one v_smfmac_f32_16x16x64_f16, K <= 32 taps), through the Python layer: the float64 oracle at every shape where
the kernel takes another path, what still runs the dense tiles, the guards, and the two kernels side by side.
force="mfma" / "mfmaonly" reach the sparse kernel, force="mfma_dense" / "mfma_denseonly" fista_mfma_kernel."""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle import pybold_oracle as orc

pytestmark = pytest.mark.gpu

EPS = 1.0e-5                 # tests/test_gpu_mfma.py
N_ITER = 60


def rel_rows(a, b):
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    return (np.linalg.norm(a - b, axis=1) / (np.linalg.norm(b, axis=1) + 1e-300)).max()


def hrf_for(K):
    from tests.adversarial_data import hrf_for as f      # (imports the package: not at collection time)
    return f(K)


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


@pytest.fixture(scope="module")
def solver():
    from pybold_amd import solver
    assert torch.cuda.is_available()
    return solver


# N: five blocks (odd parity of the last one), exactly 5 x 31, the first sample of a sixth block, an even block count,
# the flagship, ten full blocks.  K: the edges of the tap range and the flagship's 30.
@pytest.mark.parametrize("K", [1, 2, 17, 30, 32])
@pytest.mark.parametrize("N", [129, 155, 156, 186, 300, 310])
def test_against_the_float64_oracle(solver, N, K):
    """P = 1, 17 and 48 (a partial wave, one dead lane group, three waves), cold and warm start, 60 iterations: every
    problem within EPS of the float64 oracle, none handed back."""
    rng = np.random.RandomState(1000 * N + K)
    hrf = hrf_for(K)
    lip = orc.gram_lipschitz(hrf, N)
    Y = rng.randn(48, N)
    Yh = Y.astype(np.float32).astype(np.float64)
    lmax = solver.lambda_max(dev32(Y), hrf).cpu().numpy()
    lam = 0.01 * float(lmax.min())               # dense solutions: the accuracy guard (threshold / max|w| > 0.02) stays quiet
    W0 = 0.01 * rng.randn(48, N)
    ref = {False: c_oracle.fista_batch(Yh, hrf, lam, 1.0 / lip, N_ITER, threads=4)[0],
           True: c_oracle.fista_batch(Yh, hrf, lam, 1.0 / lip, N_ITER, W0=W0, threads=4)[0]}
    assert solver.which_kernel(N, K, 100000).startswith("fista_mfma")
    for warm in (False, True):
        for P in (1, 17, 48):
            W, _, nd = solver.fista_solve(dev32(Y[:P]), hrf, lam, 1.0 / lip, N_ITER, W0=dev64(W0[:P]) if warm else None,
                                          force="mfmaonly")
            err = rel_rows(W.cpu().numpy(), ref[warm][:P])
            print("N=%d K=%d P=%d warm=%d: rel err %.3e" % (N, K, P, warm, err))
            assert (nd.cpu().numpy() == N_ITER).all(), (N, K, P, warm, nd.cpu().numpy())
            assert err < EPS, (N, K, P, warm, err)


def test_33_taps_and_the_cost_trace_stay_on_the_dense_tiles(solver):
    """Reported alike and bit for bit what force="mfma_dense" gives."""
    rng = np.random.RandomState(7)
    Y, W0 = rng.randn(40, 300), 0.01 * rng.randn(40, 300)
    for K, want_J in ((33, False), (30, True), (33, True)):
        hrf = orc.spm_hrf(1.0, 1.0, float(K), False)[0][:K]
        lip = orc.gram_lipschitz(hrf, 300)
        assert solver.which_kernel(300, K, 100000, want_J=want_J) == solver.which_kernel(300, 30, 100000, want_J=want_J)
        a = solver.fista_solve(dev32(Y), hrf, 0.3, 1.0 / lip, N_ITER, W0=dev64(W0), want_J=want_J, force="mfma")
        b = solver.fista_solve(dev32(Y), hrf, 0.3, 1.0 / lip, N_ITER, W0=dev64(W0), want_J=want_J, force="mfma_dense")
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and int(a[2].min()) == N_ITER
        if want_J:
            assert torch.equal(a[1], b[1])


def test_guards_hand_back_what_the_dense_kernel_hands_back(solver):
    """A warm start far outside the float16 range of the scaled series, non-finite input, an all-zero series with a warm
    start, sparse solutions (threshold > 0.02 max|w|): the same problems come back marked from both kernels, and the
    default call re-solves them to the oracle's answer."""
    from pybold_amd import data
    hrf = hrf_for(30)
    lip = orc.gram_lipschitz(hrf, 300)
    Y, _, _ = data.gen_rnd_bloc_bold_batch(40, dur=5.0, tr=1.0, hrf=hrf, nb_events=5, avg_dur=12.0, std_dur=1.0, snr=1.0, seed=5)
    Y[7] = 0.0
    Y[11] *= 1.0e30                                         # the series itself far out of range: scaled back by its own sigma
    Yh = Y.cpu().numpy().astype(np.float64)
    rng = np.random.RandomState(1)
    W0 = 1e-3 * rng.randn(40, 300)
    W0[3] *= 1e9                                            # sigma w far beyond 65504
    W0[21] = np.nan
    lmax = solver.lambda_max(Y, hrf).cpu().numpy()
    lam = np.where(np.arange(40) % 2 == 0, 1.0, 0.7 * lmax)
    lam[7] = 1.0
    lam[11] = 0.01 * lmax[11]
    nds = solver.fista_solve(Y, hrf, lam, 1.0 / lip, 120, W0=dev64(W0), force="mfmaonly")[2].cpu().numpy()
    ndd = solver.fista_solve(Y, hrf, lam, 1.0 / lip, 120, W0=dev64(W0), force="mfma_denseonly")[2].cpu().numpy()
    print("handed back: sparse tiles %s, dense tiles %s" % (np.flatnonzero(nds == -1), np.flatnonzero(ndd == -1)))
    assert (nds == ndd).all()
    caught = np.flatnonzero(nds == -1)
    assert 3 in caught and 21 in caught and 7 in caught and len(caught) >= 8 and (nds[[0, 2, 6, 8]] == 120).all()
    Wo, _, _ = c_oracle.fista_batch(Yh, hrf, lam, 1.0 / lip, 120, W0=W0, threads=8)
    ok = (np.arange(40) != 21) & (np.linalg.norm(Wo, axis=1) > 0)
    for force in ("mfma", "mfma_dense"):
        W, _, nd = solver.fista_solve(Y, hrf, lam, 1.0 / lip, 120, W0=dev64(W0), force=force)
        assert (nd.cpu().numpy() == 120).all()
        assert rel_rows(W.cpu().numpy()[ok], Wo[ok]) < EPS, force
        assert np.isnan(W.cpu().numpy()[21]).all()


def test_sparse_against_dense_tiles_at_the_flagship_shape(solver):
    """N = 300, K = 30, 500 iterations, 64 problems: both within EPS of the oracle.  The two distances and their ratio are
    printed for profiles/sparse_tiles_ab.txt; no bound on the ratio (the far field and E cancel where C1 added)."""
    from pybold_amd import data
    hrf = orc.spm_hrf(1.0, 1.0, 30.0, False)[0][:30]
    lip = orc.gram_lipschitz(hrf, 300)
    Y, _, _ = data.gen_rnd_bloc_bold_batch(64, dur=5.0, tr=1.0, hrf=hrf, nb_events=5, avg_dur=12.0, std_dur=1.0, snr=1.0, seed=11)
    Yh = Y.cpu().numpy().astype(np.float64)
    Wo, _, _ = c_oracle.fista_batch(Yh, hrf, 1.0, 1.0 / lip, 500, threads=8)
    err = {}
    for force in ("mfmaonly", "mfma_denseonly"):
        W, _, nd = solver.fista_solve(Y, hrf, 1.0, 1.0 / lip, 500, force=force)
        assert (nd.cpu().numpy() == 500).all()
        err[force] = rel_rows(W.cpu().numpy(), Wo)
    print("sparse tiles vs oracle %.3e, dense tiles vs oracle %.3e, ratio %.3f" % (err["mfmaonly"], err["mfma_denseonly"],
                                                                                err["mfmaonly"] / err["mfma_denseonly"]))
    assert err["mfmaonly"] < EPS and err["mfma_denseonly"] < EPS


def test_shared_taps_in_device_memory_compute_what_host_taps_compute(solver):
    """pb_fista_solve_pp with ONE HRF and its step in device memory (the z-step of the shared-HRF blind loop) runs the same
    kernel with the taps read on the device: whole rounds bit for bit what the host-taps solve gives, both within EPS of
    the oracle; with the dense tiles pinned the two agree bit for bit too."""
    rng = np.random.RandomState(4)
    N, P = 300, 16384 + 40
    h = hrf_for(27)
    lip = orc.gram_lipschitz(h, N)
    Y = dev32(rng.randn(P, N))
    taps, stepc = dev64(h), dev64(np.array([1.0 / lip]))
    W, nd = solver.fista_solve_pp(Y, taps, stepc, 0.5, N_ITER)
    Wh, _, ndh = solver.fista_solve(Y, h, 0.5, 1.0 / lip, N_ITER, force="nopart")
    assert int(nd.min()) == N_ITER and int(ndh.min()) == N_ITER
    assert torch.equal(W[:16384], Wh[:16384])
    idx = np.r_[0, 15, 16, 16383, rng.choice(16384, 12, replace=False)]
    Wo = c_oracle.fista_batch(Y.cpu().numpy()[idx].astype(np.float64), h, 0.5, 1.0 / lip, N_ITER, threads=4)[0]
    assert rel_rows(W.cpu().numpy()[idx], Wo) < EPS
    Wd, _ = solver.fista_solve_pp(Y, taps, stepc, 0.5, N_ITER, force="dense_tiles")
    assert not torch.equal(Wd[:16384], W[:16384])           # (the flag reaches the shared-taps call: another kernel ran)
    assert rel_rows(Wd.cpu().numpy()[idx], Wo) < EPS
