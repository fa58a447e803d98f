"""The noise-driven lambda search of `deconv(lbda=None)` resident on the device for series of 641 .. 1 280 scans:
`deconv_auto(engine="device_split")` / `solver.auto_lbda_solve_split` / `pb_auto_lbda_split_d` (one voxel per workgroup of
four waves, csrc/fista_auto_split.h) against the reference's own runs (tests/golden/auto_lbda_long.npz), against the C
oracle and the host-driven loop where the alpha window fires, against the NumPy oracle at the edges of the layout."""
import numpy as np
import pytest
import torch

from oracle import pybold_oracle as orc
from test_auto_lbda_split_host import WINDOW_BUDGETS, oracle_alpha, window_oracle, window_rows

pytestmark = pytest.mark.gpu

ENGINE = "device_split"


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - b) / (np.linalg.norm(b) + 1e-300)


def _auto(y, hrf, sigma, **kw):
    import pybold_amd
    np.random.seed(0)                       # spectral_radius_est draws from the global RNG, as the fixtures did
    return pybold_amd.deconv_auto(y, 1.0, hrf, sigma=sigma, **kw)


@pytest.mark.parametrize("case", ["hcp", "n700"])
def test_split_search_against_the_reference_runs(golden, case):
    """All 18 runs of auto_lbda_long.npz (the REAL reference at 1 200 and 700 scans; 9 per case), the three sigma of a budget
    as the rows of one call: n_outer equal to the reference's, NaN padding as the host loop's batch, diff_z, z, x, J, R, G
    within 1e-6 -- the bound tests/test_gpu_exact_split.py holds the host loop to on the same fixture; min |alpha| is
    0.26 .. 3.1 in every run, none is exempt.  The 2 sigma runs take lambda negative (three per case)."""
    g = golden("auto_lbda_long")
    y, hrf, sig = g[case + "_y"], g[case + "_hrf"], g[case + "_sigma"]
    neg = n_runs = 0
    for o, i, tol in ((20, 50, 1e-6), (60, 300, 1e-2), (60, 300, 1e-3)):
        tags = ["%s_s%d_o%d_i%d_t%g" % (case, s, o, i, tol) for s in range(3)]
        X, Z, W, J, R, G, info = _auto(np.repeat(y[None, :], 3, axis=0), hrf, sig.copy(), nb_iter=o, nb_sub_iter=i,
                                       early_stopping=True, tol=tol, wind=6, engine=ENGINE)
        assert info["engine"] == ENGINE
        n_ref = [len(g["J_" + t]) for t in tags]
        assert J.shape == R.shape == G.shape == (max(n_ref), 3)
        for s, tag in enumerate(tags):
            n = n_ref[s]
            assert int(info["n_outer"][s]) == n, (tag, int(info["n_outer"][s]), n)
            for T in (J, R, G):
                assert np.isnan(T[n:, s]).all() and not np.isnan(T[:n, s]).any(), tag
            errs = [rel(W[s], g["dz_" + tag]), rel(Z[s], g["z_" + tag]), rel(X[s], g["x_" + tag]),
                    rel(J[:n, s], g["J_" + tag]), rel(R[:n, s], g["R_" + tag]), rel(G[:n, s], g["G_" + tag])]
            print(tag, "n_outer %d n_inner %d" % (n, int(info["n_inner"][s])), ["%.1e" % e for e in errs])
            assert max(errs) <= 1e-6, (tag, errs)
            neg += bool((g["alpha_" + tag] < 0).any())
            n_runs += 1
    assert n_runs == 9 and neg >= 3       # (6 of the 18 runs: three per case; the issue's floor of 3 holds for each case alone)


@pytest.mark.parametrize("case", ["n700", "hcp"])
@pytest.mark.parametrize("budget", WINDOW_BUDGETS)
def test_alpha_window_against_the_oracle_and_the_host_engine(golden, case, budget):
    """24 rows per case (test_auto_lbda_split_host.window_rows).  At (40, 30, tol 1e-1) the alpha window fires on every row,
    at several outer iterations; at (12, 20, 1e-6) on none.  n_outer equal to the C oracle's and to the host engine's on
    every row; R, G, J, diff_z, alpha, lbda within 1e-9 of the host engine: the same float64 operations in both, only the
    reduction order of r differs, and the oracle keeps |alpha| > 1e-2 on every row (asserted here on the oracle's run), so
    no row is near the pole alpha = 0 that would amplify it."""
    g = golden("auto_lbda_long")
    Y, sigma = window_rows(g, case)
    hrf = g[case + "_hrf"]
    nb_iter, nb_sub_iter, tol = budget
    _, _, Ro, _, n_oracle = window_oracle(g, case, budget)
    alphas = oracle_alpha(Ro, n_oracle, sigma, Y.shape[1])
    assert min(np.abs(a).min() for a in alphas) > 1.0e-2
    if tol == 1.0e-1:
        assert (n_oracle < nb_iter).all() and len(set(n_oracle.tolist())) >= 4
    else:
        assert (n_oracle == nb_iter).all()
    out = {e: _auto(Y, hrf, sigma, nb_iter=nb_iter, nb_sub_iter=nb_sub_iter, tol=tol, engine=e) for e in (ENGINE, "host")}
    d, h = out[ENGINE], out["host"]
    assert d[6]["engine"] == ENGINE and h[6]["engine"] == "host"
    assert np.array_equal(d[6]["n_outer"], n_oracle), (d[6]["n_outer"], n_oracle)
    assert np.array_equal(d[6]["n_outer"], h[6]["n_outer"]), np.where(d[6]["n_outer"] != h[6]["n_outer"])
    diff = np.nonzero(d[6]["n_inner"] != h[6]["n_inner"])[0]
    print("rows whose summed inner iterations differ: %d %s" % (len(diff), diff.tolist()))
    assert d[3].shape == h[3].shape
    worst = 0.0
    for v in range(Y.shape[0]):
        n = int(h[6]["n_outer"][v])
        errs = [rel(d[2][v], h[2][v])] + [rel(d[k][:n, v], h[k][:n, v]) for k in (3, 4, 5)]
        assert np.isnan(d[3][n:, v]).all() and np.isnan(h[3][n:, v]).all()
        assert max(errs) < 1e-9, (case, budget, v, errs)
        worst = max(worst, max(errs))
    assert rel(d[6]["alpha"], h[6]["alpha"]) < 1e-9 and rel(d[6]["lbda"], h[6]["lbda"]) < 1e-9
    print("%s %s: four-wave engine vs host worst rel. error %.2e, n_outer %d..%d, rows with alpha < 0: %d"
          % (case, budget, worst, n_oracle.min(), n_oracle.max(), sum(bool((a < 0).any()) for a in alphas)))


def _block_signal(n, hrf, rng):
    z = np.zeros(n)
    for start in range(3, n, max(n // 6, 8)):
        z[start:start + max(n // 14, 3)] = rng.uniform(0.5, 1.5)
    x = orc.causal_conv(hrf, z)
    return x + 0.4 * np.std(x) * rng.standard_normal(n)


@pytest.mark.parametrize("n", [641, 960, 961, 1280])
@pytest.mark.parametrize("k", [1, 27, 32])
def test_edge_layouts_against_the_oracle(n, k):
    """641: one live sample in wave 2, wave 3 all padding; 960 / 961: the boundary of wave 3; 1 280: full.  HRFs of 1, 27
    and 32 taps (no halo, a halo, the longest).  Three rows at a (6, 40) budget against orc.deconv_auto_lbda, 1e-9 on all
    six outputs (alpha stays in 1.006 .. 1.035 on these rows)."""
    from pybold_amd import utils
    from pybold_amd.linear import ConvAndLinear, DiscretInteg
    rng = np.random.default_rng(1000 * n + k)
    hrf = np.array([1.0]) if k == 1 else orc.spm_hrf(1.0, t_r=30.0 / k, dur=30.0, normalized_hrf=False)[0][:k]
    assert len(hrf) == k
    Y = np.stack([_block_signal(n, hrf, rng) for _ in range(3)])
    sigma = utils.mad_daub_noise_est(Y) * np.array([0.5, 1.0, 1.5])
    np.random.seed(0)
    lip = 0.9 * utils.spectral_radius_est(ConvAndLinear(DiscretInteg(), hrf, dim_in=n, dim_out=n), (n,))
    X, Z, W, J, R, G, info = _auto(Y, hrf, sigma, nb_iter=6, nb_sub_iter=40, engine=ENGINE)
    for v in range(3):
        xo, zo, wo, Jo, Ro, Go = orc.deconv_auto_lbda(Y[v], hrf, float(sigma[v]), lip, nb_iter=6, nb_sub_iter=40)
        assert int(info["n_outer"][v]) == len(Jo)
        errs = [rel(W[v], wo), rel(Z[v], zo), rel(X[v], xo), rel(J[:, v], Jo), rel(R[:, v], Ro), rel(G[:, v], Go)]
        assert max(errs) < 1e-9, (n, k, v, errs)


def _same(res, ref, what):
    for k in ("alpha", "lbda", "n_outer", "n_inner"):
        assert torch.equal(res[k], ref[k]), (what, k)
    for k in ("R", "G", "J"):
        assert torch.equal(torch.nan_to_num(res[k], nan=-7.0), torch.nan_to_num(ref[k], nan=-7.0)), (what, k)
        assert torch.equal(torch.isnan(res[k]), torch.isnan(ref[k])), (what, k)


def test_chunking_is_invisible_and_a_voxel_is_alone_in_its_batch(golden):
    """outer_chunk in {1, 7, nb_iter} and the library's choice: bit-identical W, alpha, lbda, R, G, J, n_outer, n_inner on
    the 24 rows of n700, with and without the alpha window firing.  Row 5 solved alone equals its row of the batch.  A warm
    start is read and not modified; the traces are optional."""
    from pybold_amd import solver
    g = golden("auto_lbda_long")
    Y, sigma = window_rows(g, "n700")
    hrf = g["n700_hrf"]
    Yd = torch.from_numpy(Y).cuda()
    step = 1.0 / float(g["n700_lipschitz"])
    for nb_iter, nb_sub_iter, tol in ((20, 10, 1e-6), (40, 30, 1e-1)):
        kw = dict(tol=tol, nb_iter=nb_iter, nb_sub_iter=nb_sub_iter)
        ref = None
        for chunk in (1, 7, nb_iter, 0):
            W, res = solver.auto_lbda_solve_split(Yd, hrf, step, sigma, outer_chunk=chunk, **kw)
            if ref is None:
                ref = (W, res)
                assert int(res["n_outer"].min()) < int(res["n_outer"].max()) or nb_iter == 20
                continue
            assert torch.equal(W, ref[0]), chunk
            _same(res, ref[1], chunk)
        W1, res1 = solver.auto_lbda_solve_split(Yd[5:6].contiguous(), hrf, step, sigma[5:6], **kw)
        assert torch.equal(W1[0], ref[0][5])
        _same(res1, {k: t[5:6] for k, t in ref[1].items()}, "alone")
    W0 = ref[0].clone()
    W1, res1 = solver.auto_lbda_solve_split(Yd, hrf, step, sigma, nb_iter=3, nb_sub_iter=10, W0=W0, want_trace=False)
    assert torch.equal(W0, ref[0]) and res1["R"] is None and res1["G"] is None and res1["J"] is None and not torch.equal(W1, W0)


def test_early_stopping_off(golden):
    """early_stopping=False (no window rule in the inner solves, no alpha window) against the oracle at (8, 40)."""
    g = golden("auto_lbda_long")
    y, hrf, sig = g["hcp_y"], g["hcp_hrf"], g["hcp_sigma"]
    X, Z, W, J, R, G, info = _auto(np.repeat(y[None, :], 3, axis=0), hrf, sig, nb_iter=8, nb_sub_iter=40,
                                   early_stopping=False, engine=ENGINE)
    assert (info["n_outer"] == 8).all() and (info["n_inner"] == 9 * 40).all() and J.shape == (8, 3)
    np.random.seed(0)
    from pybold_amd.linear import ConvAndLinear, DiscretInteg
    from pybold_amd.utils import spectral_radius_est
    lip = 0.9 * spectral_radius_est(ConvAndLinear(DiscretInteg(), hrf, dim_in=len(y), dim_out=len(y)), (len(y),))
    for v in range(3):
        xo, zo, wo, Jo, Ro, Go = orc.deconv_auto_lbda(y, hrf, float(sig[v]), lip, early_stopping=False, nb_iter=8, nb_sub_iter=40)
        errs = [rel(W[v], wo), rel(Z[v], zo), rel(X[v], xo), rel(J[:, v], Jo), rel(R[:, v], Ro), rel(G[:, v], Go)]
        assert max(errs) < 1e-9, (v, errs)


def test_registered_operator_matches_ctypes(golden):
    from pybold_amd import solver, torch_ops
    g = golden("auto_lbda_long")
    Yd = torch.from_numpy(np.repeat(g["n700_y"][None, :], 3, axis=0)).cuda()
    step = 1.0 / float(g["n700_lipschitz"])
    W, res = solver.auto_lbda_solve_split(Yd, g["n700_hrf"], step, g["n700_sigma"], nb_iter=5, nb_sub_iter=50)
    W2, res2 = torch_ops.auto_lbda_solve_split(Yd, g["n700_hrf"], step, g["n700_sigma"], nb_iter=5, nb_sub_iter=50)
    assert torch.equal(W, W2)
    for k in ("alpha", "lbda", "n_outer", "n_inner", "R", "G", "J"):
        assert torch.equal(res[k], res2[k]), k


def test_search_is_capturable(golden):
    """No host synchronisation, no allocation inside pb_auto_lbda_split_d: its launches replay from a captured graph."""
    from pybold_amd import solver
    g = golden("auto_lbda_long")
    Yd = torch.from_numpy(np.repeat(g["n700_y"][None, :], 3, axis=0)).cuda()
    sig = torch.from_numpy(g["n700_sigma"]).cuda()
    step = 1.0 / float(g["n700_lipschitz"])
    kw = dict(nb_iter=6, nb_sub_iter=20, outer_chunk=2)
    W, res = solver.auto_lbda_solve_split(Yd, g["n700_hrf"], step, sig, **kw)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        solver.auto_lbda_solve_split(Yd, g["n700_hrf"], step, sig, **kw)                # warm the capture stream
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            Wg, resg = solver.auto_lbda_solve_split(Yd, g["n700_hrf"], step, sig, **kw)
    Wg.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(Wg, W) and torch.equal(resg["alpha"], res["alpha"]) and torch.equal(resg["n_inner"], res["n_inner"])


def test_the_switch(golden, monkeypatch):
    """bold_signal.AUTO_LBDA = "device_split": a 2-D deconv(lbda=None) at 700 scans returns what
    deconv_auto(engine="device_split") returns (NumPy in, or CUDA in -> CUDA x, z, diff_z); one at 300 scans goes to the
    one-wave engine; a 1-D call keeps the host loop."""
    import pybold_amd
    from pybold_amd import bold_signal
    g = golden("auto_lbda_long")
    y, hrf = g["n700_y"], g["n700_hrf"]
    Y = np.repeat(y[None, :], 3, axis=0) * np.array([1.0, 1.5, 2.0])[:, None]
    kw = dict(nb_iter=8, nb_sub_iter=20)
    np.random.seed(0)
    one_d_before = pybold_amd.deconv(y, 1.0, hrf, lbda=None, **kw)
    monkeypatch.setattr(bold_signal, "AUTO_LBDA", "device_split")
    calls = {"split": 0, "one": 0}
    real_split, real_one = bold_signal.solver.auto_lbda_solve_split, bold_signal.solver.auto_lbda_solve
    monkeypatch.setattr(bold_signal.solver, "auto_lbda_solve_split",
                        lambda *a, **k: (calls.__setitem__("split", calls["split"] + 1), real_split(*a, **k))[1])
    monkeypatch.setattr(bold_signal.solver, "auto_lbda_solve",
                        lambda *a, **k: (calls.__setitem__("one", calls["one"] + 1), real_one(*a, **k))[1])
    for to_dev in (False, True):
        Yin = torch.from_numpy(Y).cuda() if to_dev else Y
        np.random.seed(0)
        got = pybold_amd.deconv(Yin, 1.0, hrf, lbda=None, **kw)
        want = _auto(Yin, hrf, None, engine=ENGINE, **kw)
        assert want[6]["engine"] == ENGINE
        assert len(got) == 6 and calls == {"split": 4 if to_dev else 2, "one": 0}
        for a, b in zip(got, want[:6]):
            assert type(a) is type(b)
            if torch.is_tensor(a):
                assert a.is_cuda and torch.equal(a, b)
            else:
                assert np.array_equal(a, b, equal_nan=True)
        assert all(torch.is_tensor(a) and a.is_cuda for a in got[:3]) == to_dev
    # 300 scans: the one-wave engine
    np.random.seed(0)
    got = pybold_amd.deconv(Y[:, :300].copy(), 1.0, hrf, lbda=None, **kw)
    assert calls == {"split": 4, "one": 1}
    want = _auto(Y[:, :300].copy(), hrf, None, engine="device", **kw)
    for a, b in zip(got, want[:6]):
        assert np.array_equal(a, b, equal_nan=True)
    # a 1-D call: the host loop, as before
    n_calls = dict(calls)
    np.random.seed(0)
    one_d = pybold_amd.deconv(y, 1.0, hrf, lbda=None, **kw)
    assert calls == n_calls and isinstance(one_d[3], list)
    for a, b in zip(one_d, one_d_before):
        assert np.array_equal(np.asarray(a), np.asarray(b))
