"""GPU tests of the matrix-pipe form of the solver (fista_mfma_kernel: both operators as float16 split
products on v_mfma_f32_16x16x32_f16, scans folded into the Toeplitz tiles), through the C ABI:
parity with the reference goldens and the float64 oracle, the cost trace, every series length it
serves, and its two guards (float16 range, accuracy of sparse solutions) with their exact re-solve."""
import numpy as np
import pytest
import torch

import stop_rule_cases as sc
from oracle import c_oracle
from oracle import pybold_oracle as orc

pytestmark = pytest.mark.gpu

EPS = 1.0e-5


def rel_rows(a, b):
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    return (np.linalg.norm(a - b, axis=1) / (np.linalg.norm(b, axis=1) + 1e-300)).max()


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


@pytest.fixture(scope="module")
def solver():
    from pybold_amd import solver
    assert torch.cuda.is_available()
    return solver


def test_golden_grid_on_the_matrix_pipe(solver, golden):
    """lambda x seed x iterations {1, 2, 3, 10, 500} of the reference (tests/golden/grid.npz): iterate
    and cost trace; the k = 0 and aliasing cases are in the 1/2/3-iteration goldens."""
    g = golden("grid")
    hrf = g["hrf"]
    assert "matrix pipe" in solver.which_kernel(300, len(hrf), 100000)
    worst = 0.0
    for s in range(4):
        y, lip = g["y_s%d" % s], float(g["lip_s%d" % s])
        Y = dev32(np.stack([y] * 19))                       # a ragged wave: 19 problems
        for lb in ("0.1", "1", "10"):
            for n in (1, 2, 3, 10, 500):
                W, J, nd = solver.fista_solve(Y, hrf, float(lb), 1.0 / lip, n, want_J=True, force="mfma")
                assert int(nd.min()) == n
                ref, Jref = g["dz_s%d_l%s_n%d" % (s, lb, n)], g["J_s%d_l%s_n%d" % (s, lb, n)]
                err = rel_rows(W.cpu().numpy(), np.stack([ref] * 19))
                worst = max(worst, err)
                assert err < EPS, (s, lb, n, err)
                Jn = J.cpu().numpy().astype(np.float64)
                np.testing.assert_allclose(Jn[0] / Jn[0, 0], Jref, rtol=3e-5)
                assert torch.equal(W[0], W[18]) and torch.equal(J[0], J[18])   # every column of a wave alike
    print("matrix-pipe kernel vs reference goldens: worst rel L2 %.2e" % worst)
    assert worst < 3e-6


@pytest.mark.parametrize("n,k", [(129, 16), (155, 27), (156, 27), (160, 27), (186, 30), (187, 30), (200, 30), (217, 27), (218, 27),
                                 (224, 27), (225, 27), (240, 27), (248, 33), (249, 20), (256, 33), (257, 20), (279, 28), (280, 27),
                                 (284, 28), (288, 27), (289, 27), (300, 30), (304, 33), (310, 33), (310, 32), (311, 30), (320, 32)])
def test_series_lengths_and_tap_counts(solver, n, k):
    """129..310 scans on the one-wave form (5..10 blocks of 31 samples + one sum slot, padding in the last block only:
    every block boundary is in the list), 311..320 on the split form; up to 33 taps;
    one lambda per problem, shared series (y_rep), warm start; vs the float64 C oracle."""
    rng = np.random.RandomState(n)
    hrf = orc.spm_hrf(1.0, 1.0, float(k), False)[0][:k]
    lip = orc.gram_lipschitz(hrf, n)
    Yv = rng.randn(7, n)
    lam = np.tile(np.array([0.05, 0.3, 1.0]), 7)
    W0 = 0.01 * rng.randn(21, n)
    Yh = np.repeat(Yv.astype(np.float32).astype(np.float64), 3, axis=0)
    Wo, Jo, _ = c_oracle.fista_batch(Yh, hrf, lam, 1.0 / lip, 150, W0=W0, want_J=True, threads=4)
    assert solver.which_kernel(n, k, 100000).startswith("fista_mfma")      # every shape of the list is served by it
    W, J, nd = solver.fista_solve(dev32(Yv), hrf, lam, 1.0 / lip, 150, W0=dev64(W0), want_J=True, y_rep=3, force="mfma")
    assert rel_rows(W.cpu().numpy(), Wo) < EPS and int(nd.min()) == 150
    np.testing.assert_allclose(J.cpu().numpy(), Jo, rtol=3e-5)
    W2, _, _ = solver.fista_solve(dev32(Yv), hrf, lam, 1.0 / lip, 150, W0=dev64(W0), y_rep=3, force="mfma")
    assert rel_rows(W2.cpu().numpy(), Wo) < EPS
    # and through the default dispatch (per-problem lambdas: the vector forms)
    W3, _, _ = solver.fista_solve(dev32(Yv), hrf, lam, 1.0 / lip, 150, W0=dev64(W0), y_rep=3)
    assert rel_rows(W3.cpu().numpy(), Wo) < EPS


@pytest.mark.parametrize("n,k", [(300, 34), (300, 40), (300, 48), (225, 41), (160, 34), (129, 48), (304, 47),
                                 (200, 40), (260, 36)])      # (seven and nine blocks: profiles/table_entries.txt)
def test_three_near_tiles_for_hrfs_of_34_to_48_taps(solver, n, k):
    """HRFs of 34..48 taps (short TR): the matrix-pipe form with a third near tile (lags up to 95, far
    field from lag 65 on); plain solves and the cost trace (the window-rule certificate of such
    shapes: the split form's from 225 scans on, round 5; the single-row form below).  Every problem is solved there (none handed back on ordinary data), equal to the float64 C oracle
    and to the vector forms; the library's own dispatch (whole rounds + remainder) too."""
    rng = np.random.RandomState(n + k)
    hrf = orc.spm_hrf(1.0, 30.0 / k, 30.0, False)[0][:k]
    assert len(hrf) == k
    lip = orc.gram_lipschitz(hrf, n)
    assert solver.which_kernel(n, k, 100000).startswith("fista_mfma")
    assert solver.which_kernel(n, k, 100000, want_J=True).startswith("fista_mfma")
    # (round 5: from 225 scans on the window rule rides the SPLIT form's certificate -- this form has none beside three tiles)
    assert solver.which_kernel(n, k, 100000, want_J=True, stop="window").startswith("fista_mfma2" if n > 224 else "fista_fast")
    Yv = rng.randn(40, n)
    W0 = 0.01 * rng.randn(40, n)
    Yh = Yv.astype(np.float32).astype(np.float64)
    Wo, Jo, _ = c_oracle.fista_batch(Yh, hrf, 0.3, 1.0 / lip, 200, W0=W0, want_J=True, threads=4)
    W, _, nd = solver.fista_solve(dev32(Yv), hrf, 0.3, 1.0 / lip, 200, W0=dev64(W0), force="mfmaonly")
    assert int(nd.min()) == 200                                     # nothing handed back
    assert rel_rows(W.cpu().numpy(), Wo) < 3e-6
    Wv, _, _ = solver.fista_solve(dev32(Yv), hrf, 0.3, 1.0 / lip, 200, W0=dev64(W0), force="valu")
    assert rel_rows(W.cpu().numpy(), Wv.cpu().numpy()) < 3e-6
    # with the cost trace (rotated loop), on the matrix pipe too
    Wj, J, ndj = solver.fista_solve(dev32(Yv), hrf, 0.3, 1.0 / lip, 200, W0=dev64(W0), want_J=True, force="mfmaonly")
    assert int(ndj.min()) == 200 and rel_rows(Wj.cpu().numpy(), Wo) < 3e-6
    np.testing.assert_allclose(J.cpu().numpy(), Jo, rtol=3e-5)
    # the default deconv call (window rule + cost trace): the split form's certificate, or the exact rule on the single-row form
    Ww, Jw, ndw = solver.fista_solve(dev32(Yv), hrf, 0.3, 1.0 / lip, 200, W0=dev64(W0), want_J=True, stop="window", tol=1e-6)
    assert int(ndw.min()) == 200 and rel_rows(Ww.cpu().numpy(), Wo) < EPS
    if (n, k) == (300, 48):                                         # whole round + remainder, cold start
        Y = dev32(rng.randn(16384 + 300, n))
        Wl, _, ndl = solver.fista_solve(Y, hrf, 1.0, 1.0 / lip, 60)
        assert solver.launch_plan(n, k, 16384 + 300)[0] == 16384 and int(ndl.min()) == 60
        idx = np.r_[0, 15, 16383, 16384, 16683, rng.choice(16384, 8, replace=False)]
        Wo2, _, _ = c_oracle.fista_batch(Y.cpu().numpy()[idx].astype(np.float64), hrf, 1.0, 1.0 / lip, 60, threads=4)
        assert rel_rows(Wl.cpu().numpy()[idx], Wo2) < EPS


def test_matrix_pipe_batch_properties(solver, golden):
    """Batch independence (bitwise, any position in a wave), power-of-two homogeneity (bitwise: the
    per-series scale absorbs it), agreement with the vector forms, the library's own dispatch."""
    from pybold_amd import data
    g = golden("case1")
    hrf, lip = g["hrf"], float(g["lipschitz"])
    Y, _, _ = data.gen_rnd_bloc_bold_batch(20011, dur=5.0, tr=1.0, hrf=hrf, nb_events=5, avg_dur=12.0, std_dur=1.0,
                                           snr=1.0, seed=21)
    W, _, nd = solver.fista_solve(Y, hrf, 1.0, 1.0 / lip, 80)            # 16 384 on the matrix pipe + a remainder
    assert solver.launch_plan(300, 30, 20011)[0] == 16384 and int(nd.min()) == 80
    Wm, _, _ = solver.fista_solve(Y, hrf, 1.0, 1.0 / lip, 80, force="mfma")
    assert torch.equal(W[:16384], Wm[:16384])
    lo, hi = 7003, 7003 + 4099
    Ws, _, _ = solver.fista_solve(Y[lo:hi].contiguous(), hrf, 1.0, 1.0 / lip, 80, force="mfma")
    assert torch.equal(Ws, Wm[lo:hi])
    Wh, _, _ = solver.fista_solve(Y * 8.0, hrf, 8.0, 1.0 / lip, 80, force="mfma")
    assert torch.equal(Wh, 8.0 * Wm)
    Wv, _, _ = solver.fista_solve(Y, hrf, 1.0, 1.0 / lip, 80, force="valu")
    assert float(((Wm - Wv).norm(dim=1) / Wv.norm(dim=1)).max()) < 2e-6
    idx = np.random.RandomState(0).choice(20011, 48, replace=False)
    Wo, _, _ = c_oracle.fista_batch(Y.cpu().numpy()[idx].astype(np.float64), hrf, 1.0, 1.0 / lip, 80, threads=8)
    assert rel_rows(W.cpu().numpy()[idx], Wo) < EPS


def test_guards_hand_problems_back_to_the_float32_operators(solver, golden):
    """(a) a warm start far outside the float16 range of the scaled series, (b) sparse solutions
    (lambda close to lambda_max: the accuracy guard), (c) an all-zero series (scale 1, warm start decaying): each is solved -- by the
    re-solve on the single-row form where a guard fired -- to the oracle's answer, n_done = n_iter."""
    from pybold_amd import data
    g = golden("case1")
    hrf, lip = g["hrf"], float(g["lipschitz"])
    Y, _, _ = data.gen_rnd_bloc_bold_batch(40, dur=5.0, tr=1.0, hrf=hrf, nb_events=5, avg_dur=12.0, std_dur=1.0,
                                           snr=1.0, seed=5)
    Y[7] = 0.0
    Yh = Y.cpu().numpy().astype(np.float64)
    rng = np.random.RandomState(1)
    W0 = 1e-3 * rng.randn(40, 300)
    W0[3] *= 1e9                                            # sigma w far beyond 65504
    W0[21] = np.nan                                         # garbage in: the guard must not swallow it silently
    lmax = solver.lambda_max(Y, hrf).cpu().numpy()
    lam = np.where(np.arange(40) % 2 == 0, 1.0, 0.7 * lmax)
    lam[7] = 1.0
    Wo, _, _ = c_oracle.fista_batch(Yh, hrf, lam, 1.0 / lip, 120, W0=W0, threads=8)
    W, _, nd = solver.fista_solve(Y, hrf, lam, 1.0 / lip, 120, W0=dev64(W0), force="mfma")
    Wn = W.cpu().numpy()
    ok = np.arange(40) != 21
    assert (nd.cpu().numpy() == 120).all()
    assert rel_rows(Wn[ok & (np.linalg.norm(Wo, axis=1) > 0)], Wo[ok & (np.linalg.norm(Wo, axis=1) > 0)]) < EPS
    assert np.isnan(Wn[21]).all()
    # without the re-solve (diagnostic flag) the problems a guard caught come back marked ...
    _, _, ndc = solver.fista_solve(Y, hrf, lam, 1.0 / lip, 120, W0=dev64(W0), force="mfmaonly")
    ndc = ndc.cpu().numpy()
    caught = np.flatnonzero(ndc == -1)
    assert 3 in caught and 21 in caught and (ndc[[0, 2, 6, 8]] == 120).all()
    assert np.isin(caught, np.r_[3, 21, np.arange(1, 40, 2)]).all() and len(caught) >= 8     # sparse solutions
    # ... and their final values are the single-row kernel's, bit for bit
    Wf, _, _ = solver.fista_solve(Y, hrf, lam, 1.0 / lip, 120, W0=dev64(W0), force="fast1")
    sel = torch.from_numpy(caught[caught != 21]).cuda()
    assert torch.equal(W[sel], Wf[sel])


def test_shared_hrf_z_step_on_the_matrix_pipe(solver):
    """pb_fista_solve_pp with ONE HRF and its step in device memory (the z-step of the shared-HRF blind
    loop): whole rounds on the matrix-pipe form reading the taps from the device, vs the oracle."""
    rng = np.random.RandomState(0)
    t_r, dur, n = 0.75, 20.0, 300
    h = orc.spm_hrf(0.9, t_r, dur, False)[0]
    lip = orc.gram_lipschitz(h, n)
    Y = dev32(rng.randn(16384 + 40, n))
    taps, stepc = dev64(h), dev64(np.array([1.0 / lip]))
    W, nd = solver.fista_solve_pp(Y, taps, stepc, 1.7, 60)
    assert int(nd.min()) == 60
    idx = np.r_[0, 15, 16, 16383, 16384, 16423, rng.choice(16384, 10, replace=False)]
    Wo = orc.fista_batch(Y.cpu().numpy()[idx].astype(np.float64), h, 1.7, 1.0 / lip, 60)
    assert rel_rows(W.cpu().numpy()[idx], Wo) < EPS
    Wv, _ = solver.fista_solve_pp(Y, taps, stepc, 1.7, 60, force="valu")
    assert float(((W - Wv).norm(dim=1) / Wv.norm(dim=1)).max()) < 2e-6


@pytest.mark.parametrize("theta", [0.5, 0.7, 1.08, 1.3, 2.0])
def test_tap_scale_does_not_eat_the_float16_range(solver, theta):
    """HRFs of different gain (dilations 0.5 .. 2.0 of the reference's model: max |cumsum h| from 2.5
    down to 0.63, tap scales 2^1 .. 2^3): the series' scale accounts for the tap scale, so ordinary
    data fitted with a WRONG HRF (the first z-steps of the blind loop: residuals as large as the
    series) stays on the matrix-pipe form -- nothing handed back -- for the plain solve and for the
    shared-HRF z-step, both equal to the oracle."""
    from pybold_amd import data
    t_r, dur, n = 0.75, 20.0, 300
    h_true = orc.spm_hrf(0.7, t_r, dur, False)[0]
    h = orc.spm_hrf(theta, t_r, dur, False)[0]
    lip = orc.gram_lipschitz(h, n)
    Y, _, _ = data.gen_rnd_bloc_bold_batch(16384 + 48, dur=n * t_r / 60.0, tr=t_r, hrf=h_true, nb_events=5, avg_dur=12.0,
                                           std_dur=1.0, snr=10.0, seed=41)
    _, _, nd = solver.fista_solve(Y, h, 1.7, 1.0 / lip, 100, force="mfmaonly")
    assert int((nd < 0).sum()) == 0
    taps, stepc = dev64(h), dev64(np.array([1.0 / lip]))
    W, nd = solver.fista_solve_pp(Y, taps, stepc, 1.7, 100, force="intermediate_noresolve")
    assert int((nd < 0).sum()) == 0 and int(nd.min()) == 100
    rng = np.random.RandomState(2)
    idx = np.r_[0, 16383, 16384, 16431, rng.choice(16384, 12, replace=False)]
    Wo = orc.fista_batch(Y.cpu().numpy()[idx].astype(np.float64), h, 1.7, 1.0 / lip, 100)
    assert rel_rows(W.cpu().numpy()[idx], Wo) < EPS


def test_window_rule_certificate_on_the_matrix_pipe(solver, golden):
    """The reference-default deconv call (window rule, wind = 6, cost trace) on the matrix-pipe form:
    (a) default tolerance, nothing fires: n_done = n_iter, iterate and trace equal the plain solve of
    the same kernel form bit for bit; the golden default run (1000 iterations) is reproduced;
    (b) a tolerance at which about half of the series stop early: stop iterations and iterates of the
    float64 oracle (the uncleared problems are re-solved with the full rule);
    (c) the certificate clears a realistic batch at the default tol = 1e-6 and all but a few problems at 2e-5."""
    from pybold_amd import data
    g = golden("early_stop")
    hrf, lip = g["hrf"], float(g["lipschitz"])
    assert "matrix pipe" in solver.which_kernel(300, 30, 40000, want_J=True, stop="window", wind=6)
    Y, _, _ = data.gen_rnd_bloc_bold_batch(16384 + 700, dur=5.0, tr=1.0, hrf=hrf, nb_events=5, avg_dur=12.0, std_dur=1.0,
                                           snr=1.0, seed=31)
    W, J, nd = solver.fista_solve(Y, hrf, 1.0, 1.0 / lip, 200, want_J=True, stop="window", tol=1e-6, wind=6)
    Wp, Jp, _ = solver.fista_solve(Y, hrf, 1.0, 1.0 / lip, 200, want_J=True)
    assert int(nd.min()) == 200 and torch.equal(W[:16384], Wp[:16384]) and torch.equal(J[:16384], Jp[:16384])
    Wg, _, ndg = solver.fista_solve(dev32(np.stack([g["y"]] * 20)), hrf, 1.0, 1.0 / lip, 1000, want_J=True,
                                    stop="window", tol=1e-6, wind=6, force="mfma")
    assert (ndg.cpu().numpy() == int(g["n_default"])).all()
    assert rel_rows(Wg.cpu().numpy(), np.stack([g["dz_default"]] * 20)) < EPS
    # (b)
    Ys = Y[:43].clone()
    Ys[20] = torch.from_numpy(g["y"]).float().cuda()
    Yh = Ys.cpu().numpy().astype(np.float64)
    tol = 0.01
    n_fire = np.array([orc.deconv_fixed_lbda(Yh[v], hrf, 1.0, nb_iter=400, tol=tol, lipschitz=lip, dense=False)[4]
                       for v in range(43)])
    n_iter = int(np.median(n_fire))
    out = [orc.deconv_fixed_lbda(Yh[v], hrf, 1.0, nb_iter=n_iter, tol=tol, lipschitz=lip, dense=False) for v in range(43)]
    Wr, nr = np.stack([o[2] for o in out]), np.array([o[4] for o in out])
    assert n_fire[20] == 191 and 10 <= (n_fire < n_iter).sum() <= 33
    Wm, Jm, ndm = solver.fista_solve(Ys, hrf, 1.0, 1.0 / lip, n_iter, want_J=True, stop="window", tol=tol, wind=6,
                                     force="mfmacert")
    assert (ndm.cpu().numpy() == nr).all()
    assert rel_rows(Wm.cpu().numpy(), Wr) < EPS
    Jn = Jm.cpu().numpy()
    for v in range(43):
        assert np.isfinite(Jn[v, :nr[v]]).all() and np.isnan(Jn[v, nr[v]:]).all(), v
    # (c) four tracked samples per problem: the bound clears a realistic batch up to tol ~ 2e-5 at 1000
    # iterations (the library keeps closer calls, tol * n_iter >= 0.02, on the pair form's sixteen)
    _, _, ndc = solver.fista_solve(Y[:2048], hrf, 1.0, 1.0 / lip, 1000, want_J=True, stop="window", tol=2e-5, wind=6,
                                   force="mfmacertonly")
    assert int((ndc < 0).sum()) <= 40                    # a few unlucky samples at most (2 %): re-solved
    _, _, ndc = solver.fista_solve(Y[:2048], hrf, 1.0, 1.0 / lip, 1000, want_J=True, stop="window", tol=1e-6, wind=6,
                                   force="mfmacertonly")
    assert int((ndc < 0).sum()) == 0                     # the reference default: nothing handed back


@pytest.mark.parametrize("n,k", [(150, 27), (180, 30), (210, 27), (240, 30), (270, 27)])
def test_rule_certificate_and_device_taps_at_every_block_count(solver, n, k):
    """`fista_mfma_kernel<NB, ...>` at 5 .. 9 blocks (ten: the 300-scan tests above and in tests/test_gpu_round4.py) in the
    three instances no series length of the other tests runs: the window rule as a certificate (stop iterations and iterates
    of the exact rule, the flagged rows re-solved; what the certificate alone clears ran every iteration), the _loops_deconv
    rule inside the kernel (+-1 on 3 % at most, as tests/test_gpu_round5.py allows the split forms), the shared-HRF z-step
    with the taps in device memory -- against the float64 oracles."""
    rng = np.random.RandomState(n * 3 + k)
    hrf = orc.spm_hrf(1.0, 1.0, float(k), False)[0][:k]
    lip = orc.gram_lipschitz(hrf, n)
    assert solver.launch_plan(n, k, 100000, stop="loops")[1].startswith("fista_mfma_kernel")
    assert "matrix pipe" in solver.which_kernel(n, k, 40000, want_J=True, stop="window", wind=6)
    # the certificate
    Yv = rng.randn(24, n)
    Y32 = Yv.astype(np.float32).astype(np.float64)
    Yd = dev32(Yv)
    tol = 0.01
    n_fire = np.array([orc.deconv_fixed_lbda(Y32[v], hrf, 0.7, nb_iter=400, tol=tol, lipschitz=lip, dense=False)[4] for v in range(24)])
    n_iter = int(np.median(n_fire))
    out = [orc.deconv_fixed_lbda(Y32[v], hrf, 0.7, nb_iter=n_iter, tol=tol, lipschitz=lip, dense=False) for v in range(24)]
    Wr, nr = np.stack([o[2] for o in out]), np.array([o[4] for o in out])
    assert 0 < (nr < n_iter).sum() < 24
    Ww, Jw, ndw = solver.fista_solve(Yd, hrf, 0.7, 1.0 / lip, n_iter, want_J=True, stop="window", tol=tol, wind=6, force="mfmacert")
    assert (ndw.cpu().numpy() == nr).all(), (ndw.cpu().numpy(), nr)
    assert rel_rows(Ww.cpu().numpy(), Wr) < EPS
    _, _, ndc = solver.fista_solve(Yd, hrf, 0.7, 1.0 / lip, n_iter, want_J=True, stop="window", tol=tol, wind=6, force="mfmacertonly")
    ndc = ndc.cpu().numpy()
    assert ((ndc == -1) | (ndc == n_iter)).all() and (ndc[nr < n_iter] == -1).all()
    Wp, Jp, _ = solver.fista_solve(Yd, hrf, 0.7, 1.0 / lip, 200, want_J=True, force="mfmaonly")
    Wd, Jd, ndd = solver.fista_solve(Yd, hrf, 0.7, 1.0 / lip, 200, want_J=True, stop="window", tol=1e-6, wind=6, force="mfmacertonly")
    assert int(ndd.min()) == 200 and torch.equal(Wd, Wp) and torch.equal(Jd, Jp)      # nothing fires: the plain solve, bit for bit
    # the _loops_deconv rule: series whose stops spread over the run
    V = 48
    Z = np.zeros((V, n))
    for v in range(V):
        for _ in range(5):
            o = rng.randint(0, n - 20)
            Z[v, o:o + rng.randint(8, 16)] = 1.0
    X = orc.causal_conv(hrf, Z)
    noise = rng.randn(V, n)
    noise *= (np.linalg.norm(X, axis=1) / np.linalg.norm(noise, axis=1) / np.sqrt(10 ** (np.linspace(-5, 20, V) / 10)))[:, None]
    Yl = dev32(X + noise)
    Yh = Yl.cpu().numpy().astype(np.float64)
    lbda = 0.003 * float(np.median(orc.lambda_max(Yh, hrf)))
    Wo, ndo = orc.loops_batch(Yh, hrf, lbda, 1.0 / lip, 300, 1e-3)
    W, _, nd = solver.fista_solve(Yl, hrf, lbda, 1.0 / lip, 300, stop="loops", tol=1e-3, force="mfma")
    ndn = nd.cpu().numpy()
    same = ndn == ndo
    assert np.abs(ndn - ndo).max() <= 1 and same.mean() >= 0.97, (ndn, ndo)
    # no row left out: one that stops an iteration apart holds the oracle's iterate of THAT iteration
    sc.judge(sc.sweep_case(Yh, hrf, lbda, 1.0 / lip, 300, ndo, W=Wo), W.cpu().numpy(), ndn)
    assert len(set(ndo.tolist())) > 5 and ndo.min() < 300
    # taps and step in device memory: everything on the matrix-pipe form in one launch
    taps, stepc = dev64(hrf), dev64(np.array([1.0 / lip]))
    Wt, ndt = solver.fista_solve_pp(Yd, taps, stepc, 0.7, 60, force="one")
    assert int(ndt.min()) == 60
    Wot, _, _ = c_oracle.fista_batch(Y32, hrf, 0.7, 1.0 / lip, 60, threads=4)
    assert rel_rows(Wt.cpu().numpy(), Wot) < EPS
    Wv, _ = solver.fista_solve_pp(Yd, taps, stepc, 0.7, 60, force="valu")
    d = ((Wt - Wv).norm(dim=1) / Wv.norm(dim=1)).cpu().numpy()
    assert d.max() < 4e-6 and d.max() > 0.0                 # (and it is not a vector form that ran)
