"""The four-wave float64 form (`fista_exact_split_kernel`, csrc/fista_exact_split.h): series of 641 .. 1 280 scans, one
series over the four waves of a workgroup, float64 end to end -- what `pb_fista_solve_d` runs for the 1-D calls of the
API, for `deconv(lbda=None)` and for the ill-conditioned class of a partitioned float32 call at HCP run lengths.

Bounds.  Iterates against the float64 oracle: 1e-11 relative, the bound tests/test_gpu_round5.py holds the one-wave kernel
to (`test_negative_lambda_is_the_float64_path_only`).  On the CPU, changing only the summation order of the two scans
(blocks of 5 and of 320 samples) moved a 500-iteration solve of the 1 200-scan fixture by 8e-16 relative at lambda in
{0.5, 2, -0.7}: four orders of margin for FMA contraction and the order of the trees.  The LDS kernel (the form these calls
ran on before) is held to the same bound on the same inputs: the inputs are fair.

Cases.  The full product of the sizes below with {cold, warm} x four lambdas x {60, 500} iterations would be ~1 700 oracle
solves; what can go wrong depends on them as follows, and every value appears where it matters:
  N (layout: which wave holds the last sample, which are padding, halo across a wave boundary) and K (halo length, lanes that
    read LDS): every (N, K) pair, three series, both starts, all four lambdas, both iteration counts;
  P (one workgroup per problem: indexing, y_rep, isolation): 1 and 257 at every N -- K cycling so that every K meets both --
    both starts, all four lambdas, 60 iterations, plus the determinism / isolation test on 257 rows."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle import pybold_oracle as orc

pytestmark = pytest.mark.gpu

SIZES = (641, 700, 897, 960, 961, 1024, 1200, 1279, 1280)
TAPS = (2, 16, 28, 32)
LAMBDAS = (0.5, 2.0, -0.7)
BOUND = 1e-11


@pytest.fixture(scope="module")
def solver():
    from pybold_amd import solver as s
    return s


def rel_rows(a, b):
    return np.linalg.norm(a - b, axis=1) / (np.linalg.norm(b, axis=1) + 1e-300)


def hrf_for(K):
    """SPM HRFs (h[0] = 0, as every HRF of the reference) where they have a shape, a short bump otherwise."""
    if K >= 20:
        return orc.spm_hrf(1.0, 1.0, float(K), False)[0][:K].copy()
    return np.array([0.0, 0.7]) if K == 2 else np.r_[0.0, np.hanning(K + 1)[1:-1] * 0.3]


_cache = {}


def block_signals(V, N, K, seed):
    """Block signals at SNR 1 dB from the package's generator, as float64 rows (host), their HRF and a step 1 / L."""
    key = (V, N, K, seed)
    if key not in _cache:
        from pybold_amd import data
        hrf = hrf_for(K)
        assert len(hrf) == K and hrf[0] == 0.0
        Y = data.gen_rnd_bloc_bold_batch(V, dur=(N + 0.5) / 60.0, tr=1.0, hrf=hrf, nb_events=5, avg_dur=12.0, std_dur=1.0,
                                         snr=1.0, seed=seed)[0]
        Y = Y[:, :N].double().cpu().numpy().copy()
        assert Y.shape == (V, N)
        Y.setflags(write=False)
        lip = 0.9 * orc.spectral_radius_est(orc._MatrixFreeH(hrf), np.random.RandomState(0).randn(N))
        _cache[key] = (Y, hrf, 1.0 / lip)
    return _cache[key]


def _plain(solver, V, N, K, iters, seed):
    Y, hrf, step = block_signals(V, N, K, seed)
    Yd = torch.tensor(Y, device="cuda")
    rng = np.random.RandomState(seed + 1)
    lam_vec = np.tile(np.array([0.5, -0.7, 2.0]), V) * rng.uniform(0.5, 1.5, 3 * V)        # y_rep = 3: problem p -> series p // 3
    assert solver.which_kernel_f64(N, K) == solver.KERNEL_NAMES[8]
    worst = {None: 0.0, "generic": 0.0}
    for n_iter in iters:
        for lam, y_rep in [(l, 1) for l in LAMBDAS] + [(lam_vec, 3)]:
            Yo = np.repeat(Y, y_rep, axis=0)
            for warm in (False, True):
                W0 = 0.01 * rng.randn(V * y_rep, N) if warm else None
                ref, _, _ = c_oracle.fista_batch(Yo, hrf, lam, step, n_iter, W0=W0, threads=16)
                for force in (None, "generic"):
                    W, _, nd = solver.fista_solve(Yd, hrf, lam, step, n_iter, W0=torch.from_numpy(W0).cuda() if warm else None,
                                                  y_rep=y_rep, force=force)
                    e = rel_rows(W.cpu().numpy(), ref).max()
                    worst[force] = max(worst[force], e)
                    assert int(nd.min()) == int(nd.max()) == n_iter
                    assert e <= BOUND, (N, K, V, n_iter, "vector" if y_rep == 3 else lam, warm, force, e)
                    neg = np.broadcast_to(np.asarray(lam) < 0, (V * y_rep,))
                    if neg.any():
                        # anti-shrinkage: the gradient at the last sample is exactly 0 (h[0] = 0), and stays so across waves
                        if not warm:
                            assert (ref[neg, -1] == 0.0).all()
                            assert (W[:, -1].cpu().numpy()[neg] == 0.0).all(), (N, K, force)
    return worst


@pytest.mark.parametrize("K", TAPS)
@pytest.mark.parametrize("N", SIZES)
def test_plain_solves_every_layout(solver, N, K):
    worst = _plain(solver, 3, N, K, (60, 500), seed=N + K)
    print("N %d K %d: four-wave form %.1e, LDS kernel %.1e" % (N, K, worst[None], worst["generic"]))


@pytest.mark.parametrize("i,N", list(enumerate(SIZES)))
@pytest.mark.parametrize("V", [1, 257])
def test_plain_solves_batch_sizes(solver, i, N, V):
    K = TAPS[(i + (V == 257)) % 4]
    worst = _plain(solver, V, N, K, (60,), seed=3 * N + V)
    print("N %d K %d V %d: four-wave form %.1e, LDS kernel %.1e" % (N, K, V, worst[None], worst["generic"]))


# --------------------------------------------------------------------------------------------
# cost trace and both stop rules
def _oracle_with_rule(Y, hrf, lam, step, n_iter, rule, tol):
    """The recurrence of oracle.pybold_oracle (fista_batch / loops_batch / deconv_fixed_lbda: its operators, prox and
    momentum sequence) for every row, with the cost trace, the criterion trace of `rule` and the iterate each row stops
    at.  "loops": ||w_{k+1} - u_k|| / (||w_{k+1}|| + 1e-10) from j > 2 (loops_batch); "window": `_window_stop` on the last
    six stored iterates [u_{k-4} .. u_k, w_{k+1}] from k > 6 (deconv_fixed_lbda)."""
    V, n = Y.shape
    H = orc._MatrixFreeH(hrf)
    betas = orc.momentum_sequence(n_iter)
    W = np.zeros((V, n))
    J = np.full((V, n_iter), np.nan)
    crit = np.full((V, n_iter), np.nan)
    n_done = np.full(V, n_iter)
    out = np.zeros((V, n))
    active = np.ones(V, dtype=bool)
    hist = []
    for k in range(n_iter):
        U = W - step * H.adj(H.op(W) - Y)
        if k > 0 and hist:
            hist[-1] = U
        P = orc.soft_threshold(U, lam * step)
        W = P + betas[k] * (P - (U if k > 0 else 0.0))
        J[:, k] = 0.5 * np.sum(np.square(H.op(W) - Y), axis=1) + lam * np.sum(np.abs(W), axis=1)
        hist = (hist + [W])[-6:]
        if rule == "loops" and k > 2:
            crit[:, k] = np.linalg.norm(W - U, axis=1) / (np.linalg.norm(W, axis=1) + 1.0e-10)
        if rule == "window" and k > 6:
            old, new = np.mean(hist[:-3], axis=0), np.mean(hist[-3:], axis=0)
            crit[:, k] = np.linalg.norm(new - old, axis=1) / (np.linalg.norm(new, axis=1) + 1.0e-10)
        fire = active & (crit[:, k] < tol)
        out[fire], n_done[fire] = W[fire], k + 1
        active &= ~fire
    out[active] = W[active]
    return out, J, crit, n_done


# (tol, lambda) per case: on these inputs the criterion of the window rule tends to a constant of 5e-3 .. 7e-3 (it compares
# iterates with gradient points, pybold/bold_signal.py:65/:72), so of the two tolerances only 1e-2 can fire there; the
# _loops_deconv criterion tends to a constant proportional to lambda, so 1e-3 needs lambda = 0.1 with the longer HRFs.
@pytest.mark.parametrize("rule,N,K,tol,lam", [
    ("loops", 641, 28, 1e-2, 0.5), ("loops", 960, 32, 1e-3, 0.1), ("loops", 1200, 28, 1e-2, 0.5), ("loops", 1280, 16, 1e-3, 0.5),
    ("loops", 897, 2, 1e-3, 0.1), ("window", 641, 28, 1e-2, 0.1), ("window", 960, 32, 1e-2, 0.1), ("window", 1200, 28, 1e-2, 0.1),
    ("window", 1280, 16, 1e-2, 0.1), ("window", 897, 2, 1e-2, 0.1)])
def test_cost_trace_and_stop_rules(solver, rule, N, K, tol, lam):
    V, n_iter = 37, 300
    Y, hrf, step = block_signals(V, N, K, seed=N + 7)
    Wo, Jo, crit, ndo = _oracle_with_rule(Y, hrf, lam, step, n_iter, rule, tol)
    # a condition on the INPUTS: no row's criterion comes within 1e-6 relative of tol at or before its stop
    for v in range(V):
        c = crit[v, :ndo[v]]
        c = c[~np.isnan(c)]
        assert (np.abs(c - tol) > 1e-6 * tol).all(), (v, c[np.abs(c - tol) <= 1e-6 * tol])
    assert ndo.min() < n_iter, "the rule fires nowhere: the test would show nothing"
    assert solver.which_kernel_f64(N, K, want_J=True, stop=rule, wind=6) == solver.KERNEL_NAMES[8]
    Yd = torch.tensor(Y, device="cuda")
    for want_J in (True, False):
        W, J, nd = solver.fista_solve(Yd, hrf, lam, step, n_iter, want_J=want_J, stop=rule, tol=tol, wind=6)
        nd = nd.cpu().numpy()
        print(rule, N, K, "stops", sorted(set(ndo.tolist()))[:8], "rows differing", int((nd != ndo).sum()))
        assert (nd == ndo).all(), (rule, N, K, np.nonzero(nd != ndo)[0], nd[nd != ndo], ndo[nd != ndo])
        assert rel_rows(W.cpu().numpy(), Wo).max() <= BOUND
        if want_J:
            Jn = J.cpu().numpy()
            for v in range(V):
                np.testing.assert_allclose(Jn[v, :ndo[v]], Jo[v, :ndo[v]], rtol=1e-10)
                assert np.isnan(Jn[v, ndo[v]:]).all()
    # no stop rule: the whole trace
    W, J, nd = solver.fista_solve(Yd, hrf, lam, step, n_iter, want_J=True)
    np.testing.assert_allclose(J.cpu().numpy(), Jo, rtol=1e-10)
    assert int(nd.min()) == n_iter


# --------------------------------------------------------------------------------------------
# determinism and isolation: where a missing barrier shows
@pytest.mark.parametrize("N,K", [(641, 32), (1200, 28), (1280, 32)])
def test_same_bits_twice_and_alone(solver, N, K):
    V = 257
    Y, hrf, step = block_signals(V, N, K, seed=5 * N)
    Yd = torch.tensor(Y, device="cuda")
    for kw in (dict(), dict(want_J=True, stop="window", tol=1e-3, wind=6), dict(stop="loops", tol=1e-2)):
        W1, J1, nd1 = solver.fista_solve(Yd, hrf, 0.5, step, 120, **kw)
        W2, J2, nd2 = solver.fista_solve(Yd, hrf, 0.5, step, 120, **kw)
        assert torch.equal(W1, W2) and torch.equal(nd1, nd2)
        if J1 is not None:
            assert torch.equal(torch.nan_to_num(J1), torch.nan_to_num(J2))
        for i in (0, 100, 256):
            Wi, Ji, ndi = solver.fista_solve(Yd[i:i + 1].contiguous(), hrf, 0.5, step, 120, **kw)
            assert torch.equal(Wi[0], W1[i]) and int(ndi[0]) == int(nd1[i]), (N, K, kw, i)
            if J1 is not None:
                assert torch.equal(torch.nan_to_num(Ji[0]), torch.nan_to_num(J1[i]))


# --------------------------------------------------------------------------------------------
# the reference itself
def test_one_dimensional_deconv_against_the_reference(solver, golden):
    """1-D `deconv(y, t_r, hrf, lbda)` on the 1 200-scan fixture of the REAL reference (tests/golden/make_golden_r5_long.py)."""
    import pybold_amd
    g = golden("long_series")
    y, hrf, t_r = g["hcp_y"], g["hcp_hrf"], float(g["hcp_t_r"])
    assert solver.which_kernel_f64(len(y), len(hrf), want_J=True, stop="window") == solver.KERNEL_NAMES[8]
    for lbda in (0.5, 2.0):
        for nb_iter, es in ((100, False), (400, True)):
            tag = "hcp_l%g_n%d%s" % (lbda, nb_iter, "_es" if es else "")
            np.random.seed(0)                       # spectral_radius_est draws from the global RNG, as the fixture did
            x, z, dz, J, _, _ = pybold_amd.deconv(y, t_r, hrf, lbda=lbda, nb_iter=nb_iter, early_stopping=es, tol=1.0e-2, wind=6)
            assert len(J) == len(g["J_" + tag]), (tag, len(J), len(g["J_" + tag]))
            assert (not es) or len(J) < nb_iter
            for got, key in ((x, "x_"), (z, "z_"), (dz, "dz_")):
                e = np.linalg.norm(np.asarray(got) - g[key + tag]) / np.linalg.norm(g[key + tag])
                assert e <= 1e-10, (tag, key, e)
            np.testing.assert_allclose(np.asarray(J), g["J_" + tag], rtol=1e-9)


def _deconv_with_sigma(monkeypatch, y, t_r, hrf, sigma, **kw):
    """`pybold_amd.deconv(lbda=None)` with the noise estimate replaced by the value the fixture's reference run was given
    (as tests/test_gpu_round5.py does)."""
    import pybold_amd
    from pybold_amd import bold_signal
    monkeypatch.setattr(bold_signal, "mad_daub_noise_est", lambda x: sigma)
    np.random.seed(0)
    return pybold_amd.deconv(y, t_r, hrf, lbda=None, **kw)


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - b) / (np.linalg.norm(b) + 1e-300)


@pytest.mark.parametrize("case", ["hcp", "n700"])
def test_deconv_auto_lambda_on_long_series_against_the_reference(solver, golden, monkeypatch, case):
    """`deconv(lbda=None)` at 1 200 and 700 scans against the REAL reference's runs (tests/golden/make_golden_auto_long.py):
    three noise levels x three budgets, the 1-D call and the three sigma as the rows of one batch.  alpha stays away from 0
    in every run (min |alpha| 0.26 .. 3.1): none is exempt; the 2 sigma runs take lambda negative."""
    g = golden("auto_lbda_long")
    y, hrf, t_r, sig = g[case + "_y"], g[case + "_hrf"], float(g[case + "_t_r"]), g[case + "_sigma"]
    assert solver.which_kernel_f64(len(y), len(hrf), stop="window") == solver.KERNEL_NAMES[8]
    neg = 0
    for o, i, tol in ((20, 50, 1e-6), (60, 300, 1e-2), (60, 300, 1e-3)):
        tags = ["%s_s%d_o%d_i%d_t%g" % (case, s, o, i, tol) for s in range(3)]
        kw = dict(nb_iter=o, nb_sub_iter=i, early_stopping=True, tol=tol, wind=6)
        for s, tag in enumerate(tags):
            x, z, dz, J, R, G = _deconv_with_sigma(monkeypatch, y, t_r, hrf, float(sig[s]), **kw)
            assert len(J) == len(g["J_" + tag]), (tag, len(J), len(g["J_" + tag]))
            errs = [rel(dz, g["dz_" + tag]), rel(z, g["z_" + tag]), rel(x, g["x_" + tag]),
                    rel(J, g["J_" + tag]), rel(R, g["R_" + tag]), rel(G, g["G_" + tag])]
            print(tag, "1-D", ["%.1e" % e for e in errs])
            assert max(errs) <= 1e-6, (tag, errs)
            neg += bool((g["alpha_" + tag] < 0).any())
        X, Z, W, J, R, G = _deconv_with_sigma(monkeypatch, np.repeat(y[None, :], 3, axis=0), t_r, hrf, sig.copy(), **kw)
        n_ref = [len(g["J_" + t]) for t in tags]
        assert J.shape == (max(n_ref), 3)
        for s, tag in enumerate(tags):
            n = n_ref[s]
            assert np.isnan(J[n:, s]).all() and not np.isnan(J[:n, s]).any(), tag
            errs = [rel(W[s], g["dz_" + tag]), rel(Z[s], g["z_" + tag]), rel(X[s], g["x_" + tag]),
                    rel(J[:n, s], g["J_" + tag]), rel(R[:n, s], g["R_" + tag]), rel(G[:n, s], g["G_" + tag])]
            print(tag, "batch", ["%.1e" % e for e in errs])
            assert max(errs) <= 1e-6, (tag, errs)
    assert neg >= 3


# --------------------------------------------------------------------------------------------
# the ill-conditioned class of a partitioned float32 call
def _ill_families(N, ordinary):
    """The 16 families tests/test_gpu_round5.py::test_ill_conditioned_series_are_solved_in_float64 uses at 300 scans, at N."""
    t = np.arange(N)
    rng = np.random.RandomState(1)
    alt = np.where(t % 2 == 0, 1.0, -1.0)
    hp = rng.randn(N)
    return np.stack([ordinary, rng.randn(N), alt, np.sin(2 * np.pi * t / 3), np.sin(2 * np.pi * t / 4), np.sin(2 * np.pi * t / 6),
                     np.sin(2 * np.pi * t / 10), np.diff(np.r_[0.0, hp]), np.diff(np.r_[0.0, 0.0, hp], n=2), alt + 1e-3 * ordinary,
                     alt + 1e-2 * ordinary, alt + 0.1 * ordinary, alt * (1 + np.sin(2 * np.pi * t / 100)), np.ones(N), 37.0 * alt,
                     1e-3 * alt])


@pytest.mark.parametrize("N,K", [(700, 30), (1200, 28)])
def test_ill_conditioned_class_of_a_partitioned_call(solver, N, K):
    """The default float32 `fista_solve` on >= 4 096 rows: the series its lambda_max pass marks run in float64 -- on the
    four-wave form at these lengths -- and every family is within 1e-5 of the oracle on diff_z, z and x; the same through
    `pb_fista_solve_ex` with NO device copy of the taps (the guard no longer needs one for these shapes)."""
    from pybold_amd import _lib
    Yb, hrf, _ = block_signals(3, N, K, seed=N + K)
    step = 1.0 / orc.gram_lipschitz(hrf, N)
    fams = _ill_families(N, Yb[0])
    nf, n_iter = len(fams), 500
    assert nf == 16
    Yd = torch.from_numpy(np.tile(fams, (4096 // nf + 1, 1)).astype(np.float32)).cuda()
    P = Yd.shape[0]
    Yo = Yd[:nf].cpu().numpy().astype(np.float64)
    lmax = solver.lambda_max(Yd, hrf)
    lib = _lib.load()
    taps = np.ascontiguousarray(hrf, dtype=np.float64)
    betas = torch.from_numpy(orc.momentum_sequence(n_iter)).cuda()
    for lam in (0.0, 0.05 * lmax, 1.0):
        lam_o = lam[:nf].cpu().numpy() if torch.is_tensor(lam) else lam
        ref, _, _ = c_oracle.fista_batch(Yo, hrf, lam_o, step, n_iter, threads=16)
        xr, zr = orc.fista_outputs(ref, hrf)
        W, _, nd = solver.fista_solve(Yd, hrf, lam, step, n_iter)
        # the same call without a device copy of the taps
        W2 = torch.empty_like(W)
        nd2 = torch.empty_like(nd)
        work = torch.empty((int(lib.pb_fista_work_len(P, 1)),), dtype=torch.int32, device="cuda")
        lam_dev = lam.contiguous() if torch.is_tensor(lam) else None
        rc = lib.pb_fista_solve_ex(Yd.data_ptr(), N, 1, W2.data_ptr(), N, P, N, taps.ctypes.data, None, K, step,
                                   0.0 if lam_dev is not None else float(lam), lam_dev.data_ptr() if lam_dev is not None else None,
                                   betas.data_ptr(), n_iter, None, 0, 0, 0.0, 6, nd2.data_ptr(), _lib.PB_FLAG_COLD_START,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), None, 0.0, work.data_ptr(), work.numel())
        _lib.check(rc, "pb_fista_solve_ex")
        torch.cuda.synchronize()
        for Wg, ndg, what in ((W, nd, "default"), (W2, nd2, "no device taps")):
            assert int(ndg.min()) == n_iter
            X, Z = solver.fista_outputs(Wg[:nf].contiguous(), hrf)
            errs = np.stack([rel_rows(Wg[:nf].cpu().numpy(), ref), rel_rows(Z.cpu().numpy(), zr), rel_rows(X.cpu().numpy(), xr)])
            print(N, what, "lambda", "0.05 lmax" if torch.is_tensor(lam) else lam, "worst family errors", errs.max(axis=0).round(8).tolist())
            assert errs.max() <= 1e-5, (N, what, np.nonzero(errs.max(axis=0) > 1e-5)[0], errs.max())
            assert torch.equal(Wg[:nf], Wg[nf:2 * nf])
