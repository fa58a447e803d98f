"""The noise-driven lambda search of `deconv(lbda=None)` (pybold/bold_signal.py:99-214) resident on the device:
`deconv_auto(engine="device")` / `solver.auto_lbda_solve` / `pb_auto_lbda_d` against the reference's own runs
(tests/golden/auto_lbda.npz, auto_lbda_wind6.npz), against the host-driven loop on the same inputs, against the NumPy
oracle over the shapes the kernel serves; the noise level on the device (`pb_mad_daub_noise_est(_d)`) against the host
function it restates."""
import time
import warnings

import numpy as np
import pytest
import torch

from oracle import pybold_oracle as orc
from test_auto_lbda_host import DEVICE_VS_HOST_BUDGETS, device_vs_host_rows
from test_oracle_golden import AUTO_LBDA_CHAOTIC_AFTER, auto_lbda_runs

pytestmark = pytest.mark.gpu


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - b) / (np.linalg.norm(b) + 1e-300)


def _auto(y, hrf, sigma, **kw):
    import pybold_amd
    np.random.seed(0)                       # spectral_radius_est draws from the global RNG (:52), as the fixtures did
    return pybold_amd.deconv_auto(y, 1.0, hrf, sigma=sigma, **kw)


def _groups(runs):
    """The runs that share (case, kwargs) as the rows of one call: {(case, kwargs): [(tag, sigma)]}."""
    groups = {}
    for tag, case, sigma, kw in runs:
        groups.setdefault((case,) + tuple(sorted(kw.items())), []).append((tag, sigma))
    return groups


def _check_group(g, case, kw, members, tol_f, engine="device"):
    """One batched call for the rows of a group; every row against the reference's run of that row.  Returns the worst
    relative error and the outputs."""
    Y = np.repeat(g[case + "_y"][None, :], len(members), axis=0)
    X, Z, W, J, R, G, info = _auto(Y, g[case + "_hrf"], np.array([s for _, s in members]), engine=engine, **kw)
    assert info["engine"] == engine
    n_ref = [len(g["J_" + tag]) for tag, _ in members]
    assert J.shape == R.shape == G.shape == (max(n_ref), len(members)), (J.shape, n_ref)
    worst = 0.0
    for v, (tag, _) in enumerate(members):
        n = n_ref[v]
        assert int(info["n_outer"][v]) == n, (tag, int(info["n_outer"][v]), n)
        for T in (J, R, G):                  # NaN from the row's stop on, as the batch of the host loop
            assert np.isnan(T[n:, v]).all() and not np.isnan(T[:n, v]).any(), tag
        upto = AUTO_LBDA_CHAOTIC_AFTER.get(tag, n)
        errs = [rel(J[:upto, v], g["J_" + tag][:upto]), rel(R[:upto, v], g["R_" + tag][:upto]), rel(G[:upto, v], g["G_" + tag][:upto])]
        if tag not in AUTO_LBDA_CHAOTIC_AFTER:
            errs += [rel(W[v], g["dz_" + tag]), rel(Z[v], g["z_" + tag]), rel(X[v], g["x_" + tag])]
        else:
            assert np.isfinite(W[v]).all()
        print("%-32s n_outer %4d n_inner %7d  worst rel. error %.2e" % (tag, n, int(info["n_inner"][v]), max(errs)))
        assert max(errs) < tol_f, (tag, errs)
        worst = max(worst, max(errs))
    return worst, info


def test_device_search_against_the_reference_runs(golden):
    """Every non-default run of auto_lbda.npz with wind == 6 (96 runs; the rows of one case and budget batched into one
    call), and the 12 runs of auto_lbda_wind6.npz, against the reference: diff_z, z, x and the rows of J, R, G to
    1e-7 (the bound of the host-loop tests on the same fixtures, tests/test_gpu_round5.py), n_outer equal to the
    reference's, NaN padding as the batch of the host loop.

    auto_lbda.npz alone holds TWO runs with wind == 6 in which the alpha window fires (c1_s1 at tol 1e-2 and 1e-3;
    its other firing runs use wind = 4, which the device engine does not carry), short of the four this test must see:
    auto_lbda_wind6.npz (tests/golden/make_golden_auto_wind6.py, the same recipe with the real reference) adds runs at
    wind = 6 in which it fires on every row, at another outer iteration per row.  Nothing of auto_lbda.npz is left out."""
    neg = fired = n_runs = 0
    worst = 0.0
    for name in ("auto_lbda", "auto_lbda_wind6"):
        g = golden(name)
        runs = [r for r in auto_lbda_runs(g, default=False) if r[3]["wind"] == 6]
        assert len(runs) == (96 if name == "auto_lbda" else 12)
        assert name != "auto_lbda" or len(runs) == sum(1 for r in auto_lbda_runs(g, default=False) if r[3]["wind"] == 6)
        for key, members in _groups(runs).items():
            case, kw = key[0], dict(key[1:])
            w, _ = _check_group(g, case, kw, members, 1e-7)
            worst = max(worst, w)
            for tag, _ in members:
                neg += bool((g["alpha_" + tag] < 0).any())
                fired += len(g["J_" + tag]) < kw["nb_iter"]
                n_runs += 1
    print("device-resident search vs the reference: %d runs, worst rel. error %.2e; lambda < 0 in %d, alpha window fired in %d"
          % (n_runs, worst, neg, fired))
    assert n_runs == 108 and neg >= 10 and fired >= 4


def test_device_search_reference_default_call(golden):
    """`deconv(y, t_r, hrf)` -- lbda=None, 1000 x 1000, tol 1e-6, wind 6 -- on the device engine against the reference's
    run of that call: the three noise levels of case 1 as one batch, case 2 (another HRF: one HRF per call) as a call
    of its own.  1e-6 throughout; c1_s1 over the outer iterations before alpha passes through 7e-4
    (AUTO_LBDA_CHAOTIC_AFTER, exactly as tests/test_gpu_round5.py uses it), nothing else excluded."""
    g = golden("auto_lbda")
    runs = auto_lbda_runs(g, default=True)
    assert len(runs) == 4
    for key, members in _groups(runs).items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, info = _check_group(g, key[0], dict(key[1:]), members, 1e-6)
        print("%s default call, %d row(s): %.2f s wall clock, n_inner %s (%.3g inner iterations in all)"
              % (key[0], len(members), time.perf_counter() - t0, info["n_inner"].tolist(), float(info["n_inner"].sum())))


def test_device_engine_against_host_engine_on_the_same_inputs(golden):
    """64 rows (test_auto_lbda_host.device_vs_host_rows) at three budgets: n_outer equal on every row, R, G, J, diff_z
    within 1e-9 relative.  Same float64 operations in both engines, only the reduction order of r differs (one wave's
    DPP tree against a workgroup's); tests/test_auto_lbda_host.py checks that the oracle keeps |alpha| > 1e-2 on every
    row, so no row is near the alpha = 0 pole that would amplify it.  No row is routed elsewhere."""
    g = golden("auto_lbda")
    Y, sigma = device_vs_host_rows(g)
    hrf = g["c1_hrf"]
    for nb_iter, nb_sub_iter, tol in DEVICE_VS_HOST_BUDGETS:
        out = {}
        for engine in ("device", "host"):
            t0 = time.perf_counter()
            out[engine] = _auto(Y, hrf, sigma, nb_iter=nb_iter, nb_sub_iter=nb_sub_iter, tol=tol, engine=engine)
            print("(%d, %d) %s engine: %.2f s" % (nb_iter, nb_sub_iter, engine, time.perf_counter() - t0))
        d, h = out["device"], out["host"]
        assert d[6]["engine"] == "device" and h[6]["engine"] == "host"
        assert np.array_equal(d[6]["n_outer"], h[6]["n_outer"]), np.where(d[6]["n_outer"] != h[6]["n_outer"])
        print("rows whose summed inner iterations differ: %d" % int((d[6]["n_inner"] != h[6]["n_inner"]).sum()))
        assert d[3].shape == h[3].shape
        worst = 0.0
        for v in range(Y.shape[0]):
            n = int(h[6]["n_outer"][v])
            errs = [rel(d[2][v], h[2][v])] + [rel(d[k][:n, v], h[k][:n, v]) for k in (3, 4, 5)]
            assert np.isnan(d[3][n:, v]).all() and np.isnan(h[3][n:, v]).all()
            assert max(errs) < 1e-9, (nb_iter, nb_sub_iter, v, errs)
            worst = max(worst, max(errs))
        assert rel(d[6]["alpha"], h[6]["alpha"]) < 1e-9 and rel(d[6]["lbda"], h[6]["lbda"]) < 1e-9
        print("(%d, %d): device vs host worst rel. error %.2e, n_outer %d..%d" % (nb_iter, nb_sub_iter, worst,
                                                                                 h[6]["n_outer"].min(), h[6]["n_outer"].max()))


def test_chunking_is_invisible(golden):
    """outer_chunk in {1, 7, nb_iter} (and the library's choice): bit-identical W, alpha, lbda, R, G, J, n_outer, n_inner."""
    from pybold_amd import solver
    g = golden("auto_lbda")
    Y, sigma = device_vs_host_rows(g)
    Yd = torch.from_numpy(Y).cuda()
    step = 1.0 / float(g["c1_lipschitz"])
    for nb_iter, nb_sub_iter, tol in ((20, 10, 1e-6), (60, 300, 1e-2)):
        ref = None
        for chunk in (1, 7, nb_iter, 0):
            W, res = solver.auto_lbda_solve(Yd, g["c1_hrf"], step, sigma, tol=tol, nb_iter=nb_iter, nb_sub_iter=nb_sub_iter,
                                            outer_chunk=chunk)
            if ref is None:
                ref = (W, res)
                assert int(res["n_outer"].min()) < int(res["n_outer"].max()) or nb_iter == 20
                continue
            assert torch.equal(W, ref[0]), chunk
            for k in ("alpha", "lbda", "n_outer", "n_inner"):
                assert torch.equal(res[k], ref[1][k]), (chunk, k)
            for k in ("R", "G", "J"):
                assert torch.equal(torch.nan_to_num(res[k], nan=-7.0), torch.nan_to_num(ref[1][k], nan=-7.0)), (chunk, k)
                assert torch.equal(torch.isnan(res[k]), torch.isnan(ref[1][k])), (chunk, k)
    # a warm start is read, not modified, and the traces are optional
    W0 = ref[0].clone()
    W1, res1 = solver.auto_lbda_solve(Yd, g["c1_hrf"], step, sigma, nb_iter=3, nb_sub_iter=10, W0=W0, want_trace=False)
    assert torch.equal(W0, ref[0]) and res1["R"] is None and not torch.equal(W1, W0)


def test_early_stopping_off(golden):
    """early_stopping=False (no window rule in the inner solves, no alpha window) against the oracle at (8, 40)."""
    g = golden("auto_lbda")
    for case in ("c1", "c2"):
        y, hrf, sig = g[case + "_y"], g[case + "_hrf"], g[case + "_sigma"]
        np.random.seed(0)
        from pybold_amd.linear import ConvAndLinear, DiscretInteg
        from pybold_amd.utils import spectral_radius_est
        lip = 0.9 * spectral_radius_est(ConvAndLinear(DiscretInteg(), hrf, dim_in=len(y), dim_out=len(y)), (len(y),))
        X, Z, W, J, R, G, info = _auto(np.repeat(y[None, :], 3, axis=0), hrf, sig, nb_iter=8, nb_sub_iter=40,
                                       early_stopping=False, engine="device")
        assert (info["n_outer"] == 8).all() and (info["n_inner"] == 9 * 40).all() and J.shape == (8, 3)
        for v in range(3):
            xo, zo, wo, Jo, Ro, Go = orc.deconv_auto_lbda(y, hrf, float(sig[v]), lip, early_stopping=False, nb_iter=8, nb_sub_iter=40)
            errs = [rel(W[v], wo), rel(Z[v], zo), rel(X[v], xo), rel(J[:, v], Jo), rel(R[:, v], Ro), rel(G[:, v], Go)]
            assert max(errs) < 1e-9, (case, v, errs)


def _block_signal(n, hrf, rng):
    z = np.zeros(n)
    for start in range(3, n, max(n // 6, 8)):
        z[start:start + max(n // 14, 3)] = rng.uniform(0.5, 1.5)
    x = orc.causal_conv(hrf, z)
    return x + 0.4 * np.std(x) * rng.standard_normal(n)


@pytest.mark.parametrize("n", [64, 240, 320, 321, 600, 640])
@pytest.mark.parametrize("k", [1, 27, 32])
def test_shapes_against_the_oracle(n, k):
    """Both instantiations (5 and 10 samples per lane) at their edges, HRFs of 1, 27 and 32 taps: three rows at a
    (6, 40) budget against orc.deconv_auto_lbda, 1e-9."""
    from pybold_amd import utils
    from pybold_amd.linear import ConvAndLinear, DiscretInteg
    rng = np.random.default_rng(1000 * n + k)
    hrf = np.array([1.0]) if k == 1 else orc.spm_hrf(1.0, t_r=30.0 / k, dur=30.0, normalized_hrf=False)[0][:k]
    assert len(hrf) == k
    Y = np.stack([_block_signal(n, hrf, rng) for _ in range(3)])
    sigma = utils.mad_daub_noise_est(Y) * np.array([0.5, 1.0, 1.5])
    np.random.seed(0)
    lip = 0.9 * utils.spectral_radius_est(ConvAndLinear(DiscretInteg(), hrf, dim_in=n, dim_out=n), (n,))
    X, Z, W, J, R, G, info = _auto(Y, hrf, sigma, nb_iter=6, nb_sub_iter=40, engine="device")
    for v in range(3):
        xo, zo, wo, Jo, Ro, Go = orc.deconv_auto_lbda(Y[v], hrf, float(sigma[v]), lip, nb_iter=6, nb_sub_iter=40)
        assert int(info["n_outer"][v]) == len(Jo)
        errs = [rel(W[v], wo), rel(Z[v], zo), rel(X[v], xo), rel(J[:, v], Jo), rel(R[:, v], Ro), rel(G[:, v], Go)]
        assert max(errs) < 1e-9, (n, k, v, errs)


def test_unsupported_shapes_are_refused_or_run_on_the_host(golden):
    g = golden("auto_lbda")
    rng = np.random.default_rng(5)
    hrf30 = g["c1_hrf"]
    hrf33 = orc.spm_hrf(1.0, t_r=30.0 / 33, dur=30.0, normalized_hrf=False)[0][:33]
    from pybold_amd import solver
    for y, hrf, kw, word in ((np.stack([_block_signal(641, hrf30, rng)] * 2), hrf30, dict(), "641 scans"),
                             (np.stack([_block_signal(300, hrf33, rng)] * 2), hrf33, dict(), "33 taps"),
                             (np.stack([g["c1_y"]] * 2), hrf30, dict(wind=4), "wind = 4")):
        with pytest.raises(ValueError, match=word):
            _auto(y, hrf, 1.0, nb_iter=3, nb_sub_iter=10, engine="device", **kw)
        solver._warned.clear()
        with pytest.warns(RuntimeWarning, match="running the host loop"):
            out = _auto(y, hrf, np.array([1.0, 1.0]), nb_iter=3, nb_sub_iter=10, engine="auto", **kw)
        ref = _auto(y, hrf, np.array([1.0, 1.0]), nb_iter=3, nb_sub_iter=10, engine="host", **kw)
        assert out[6]["engine"] == "host" and np.array_equal(out[2], ref[2]) and np.array_equal(out[3], ref[3])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert _auto(np.stack([g["c1_y"]] * 2), hrf30, 1.0, nb_iter=2, nb_sub_iter=5, engine="auto")[6]["engine"] == "device"


def test_the_switch(golden, monkeypatch):
    """bold_signal.AUTO_LBDA = "device": a 2-D deconv(lbda=None) returns what deconv_auto(engine="device") returns, NumPy
    in or CUDA in; a 1-D call keeps the host loop."""
    import pybold_amd
    from pybold_amd import bold_signal
    g = golden("auto_lbda")
    y, hrf, sig = g["c1_y"], g["c1_hrf"], g["c1_sigma"]
    Y = np.repeat(y[None, :], 3, axis=0) * np.array([1.0, 1.5, 2.0])[:, None]
    kw = dict(nb_iter=12, nb_sub_iter=30)
    np.random.seed(0)
    host = pybold_amd.deconv(Y, 1.0, hrf, lbda=None, **kw)
    np.random.seed(0)
    one_d_before = pybold_amd.deconv(y, 1.0, hrf, lbda=None, **kw)
    monkeypatch.setattr(bold_signal, "AUTO_LBDA", "device")
    calls = []
    real = bold_signal.solver.auto_lbda_solve
    monkeypatch.setattr(bold_signal.solver, "auto_lbda_solve", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for to_dev in (False, True):
        Yin = torch.from_numpy(Y).cuda() if to_dev else Y
        np.random.seed(0)
        got = pybold_amd.deconv(Yin, 1.0, hrf, lbda=None, **kw)
        want = _auto(Yin, hrf, None, engine="device", **kw)
        assert len(got) == 6 and len(calls) == (4 if to_dev else 2)
        for a, b in zip(got, want[:6]):
            assert type(a) is type(b)
            if torch.is_tensor(a):
                assert a.is_cuda and torch.equal(a, b)
            else:
                assert np.array_equal(a, b, equal_nan=True)
        # ... and follows the host loop's answer for the same call (same sigma: estimated from the same rows)
        for a, b in zip(got, host):
            a = a.cpu().numpy() if torch.is_tensor(a) else a
            assert a.shape == b.shape and rel(a, b) < 1e-9
    n_calls = len(calls)
    np.random.seed(0)
    one_d = pybold_amd.deconv(y, 1.0, hrf, lbda=None, **kw)
    assert len(calls) == n_calls and isinstance(one_d[3], list)
    for a, b in zip(one_d, one_d_before):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    del sig


SIGMA_LENGTHS = [5, 6, 7, 64, 240, 284, 300, 301, 600, 1200, 2432, 8192]


@pytest.mark.parametrize("n", SIGMA_LENGTHS)
def test_noise_level_on_the_device(n):
    """solver.mad_daub_noise_est against utils.mad_daub_noise_est on 257 rows: noise, constant rows (sigma = 0),
    integer-quantised rows (ties in both medians), rows with a DC offset of 1e3.  |delta sigma| <= 1e-13 max|y_row|:
    six rounded products of 2^-53 relative size with a ~50x margin (with contraction off the two should agree exactly).
    The float32-row entry equals the float64 one on the widened data."""
    from pybold_amd import solver, utils
    rng = np.random.default_rng(n)
    Y = rng.standard_normal((257, n)) * rng.uniform(0.1, 30.0, size=(257, 1))
    Y[0:8] = rng.uniform(-5, 5, size=(8, 1))                               # constant rows
    Y[8:40] = np.round(rng.standard_normal((32, n)) * 2.0)                 # integer-quantised: ties
    Y[40:72] += 1.0e3                                                      # DC offset
    Y[72:80] = np.round(rng.standard_normal((8, n))) + 1.0e3
    want = utils.mad_daub_noise_est(Y)
    got = solver.mad_daub_noise_est(torch.from_numpy(Y).cuda()).cpu().numpy()
    bound = 1.0e-13 * np.abs(Y).max(axis=1)
    assert got.shape == want.shape == (257,)
    assert (want[0:8] == 0.0).all() and (got[0:8] == 0.0).all()
    print("N = %d: max |delta sigma| %.3e (%d rows differ at all)" % (n, np.abs(got - want).max(), int((got != want).sum())))
    assert (np.abs(got - want) <= bound).all(), np.abs(got - want).max()
    Y32 = Y.astype(np.float32)
    got32 = solver.mad_daub_noise_est(torch.from_numpy(Y32).cuda())
    wide = solver.mad_daub_noise_est(torch.from_numpy(Y32.astype(np.float64)).cuda())
    assert torch.equal(got32, wide)
    # the same through the registered operator, and a strided view (leading dimension > N)
    from pybold_amd import torch_ops
    assert torch.equal(torch_ops.mad_daub_noise_est(torch.from_numpy(Y).cuda()), torch.from_numpy(got).cuda())
    pad = torch.zeros((257, n + 3), dtype=torch.float64, device="cuda")
    pad[:, :n] = torch.from_numpy(Y).cuda()
    assert torch.equal(solver.mad_daub_noise_est(pad[:, :n]), torch.from_numpy(got).cuda())


def test_noise_level_limits_and_default_sigma(golden):
    from pybold_amd import _lib, solver
    with pytest.raises(_lib.PyboldHipError, match="8192"):
        solver.mad_daub_noise_est(torch.zeros((2, 8193), dtype=torch.float64, device="cuda"))
    with pytest.raises(_lib.PyboldHipError):
        solver.mad_daub_noise_est(torch.zeros((2, 4), dtype=torch.float64, device="cuda"))
    # sigma=None: on the device for CUDA input, the host function otherwise -- the same numbers, hence the same search
    g = golden("auto_lbda")
    Y = np.stack([g["c1_y"], 2.0 * g["c1_y"]])
    a = _auto(Y, g["c1_hrf"], None, nb_iter=4, nb_sub_iter=20, engine="device")
    b = _auto(torch.from_numpy(Y).cuda(), g["c1_hrf"], None, nb_iter=4, nb_sub_iter=20, engine="device")
    from pybold_amd import utils
    assert np.array_equal(a[6]["sigma"], utils.mad_daub_noise_est(Y)) and np.allclose(b[6]["sigma"], a[6]["sigma"], rtol=0, atol=1e-13 * np.abs(Y).max())
    assert b[2].is_cuda and rel(b[2].cpu().numpy(), a[2]) < 1e-9 and np.array_equal(a[6]["n_outer"], b[6]["n_outer"])


def test_registered_operator_matches_ctypes(golden):
    from pybold_amd import solver, torch_ops
    g = golden("auto_lbda")
    Yd = torch.from_numpy(np.repeat(g["c1_y"][None, :], 3, axis=0)).cuda()
    step = 1.0 / float(g["c1_lipschitz"])
    W, res = solver.auto_lbda_solve(Yd, g["c1_hrf"], step, g["c1_sigma"], nb_iter=5, nb_sub_iter=50)
    W2, res2 = torch_ops.auto_lbda_solve(Yd, g["c1_hrf"], step, g["c1_sigma"], nb_iter=5, nb_sub_iter=50)
    assert torch.equal(W, W2)
    for k in ("alpha", "lbda", "n_outer", "n_inner", "R", "G", "J"):
        assert torch.equal(res[k], res2[k]), k


def test_search_is_capturable(golden):
    """No host synchronisation, no allocation inside pb_auto_lbda_d: its launches replay from a captured graph."""
    from pybold_amd import solver
    g = golden("auto_lbda")
    Yd = torch.from_numpy(np.repeat(g["c1_y"][None, :], 3, axis=0)).cuda()
    sig = torch.from_numpy(g["c1_sigma"]).cuda()
    step = 1.0 / float(g["c1_lipschitz"])
    kw = dict(nb_iter=6, nb_sub_iter=20, outer_chunk=2)
    W, res = solver.auto_lbda_solve(Yd, g["c1_hrf"], step, sig, **kw)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        solver.auto_lbda_solve(Yd, g["c1_hrf"], step, sig, **kw)                # warm the capture stream
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            Wg, resg = solver.auto_lbda_solve(Yd, g["c1_hrf"], step, sig, **kw)
    Wg.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(Wg, W) and torch.equal(resg["alpha"], res["alpha"]) and torch.equal(resg["n_inner"], res["n_inner"])
