"""The opt-in four-wave float64 register form for HRFs of up to 48 taps (csrc/fista_exact_split_long.h: one problem per
workgroup of four waves, series of 641 .. 1 280 scans, the taps in one VGPR pair of every wave) on the GPU:
`pb_fista_solve_split_long_d` / `pb_fista_solve_split_long_pp_d`, `pb_auto_lbda_split_long_d` /
`pb_auto_lbda_split_long_pp_d`, `deconv` under `bold_signal.SPLIT_LONG_HRF` and `deconv_auto(engine="device_split_long_hrf")`.

1. Up to 32 taps the form must return the BITS of the existing KT = 32 four-wave kernels (the same pass, the extra taps add
   exact zeros; the wider halo only moves lanes from a DPP shift to an LDS read of the same value).
2. At 33 .. 48 taps: the float64 oracles under oracle/ with the float64 bounds of tests/test_gpu_long_hrf.py (1e-10 per row
   and on the cost trace), and the same call without the flag -- the LDS kernel, today's answer -- within 1e-9 with equal
   n_done.  641 scans leave one sample in wave 1 and two waves of padding; at 688 / 689 wave 1 first holds a full 47-sample
   halo and one more; 960 / 961 are the boundary of waves 2 and 3.
3. The search: n_outer of the host engine and of the C oracle on rows whose alpha window fires at different outer
   iterations, 1e-9 against the host engine; chunking and batch position change no bit; early stopping off; graph capture;
   the registered operator.
4. The REAL reference's runs (tests/golden/split_long_hrf.npz) within 1e-6, n_outer and trace lengths equal.
5. Padded leading dimensions and sentinel guards (tests/frames.py) at N = 961, K = 42.
6. The form is refused outside its shapes; a call that does not name it at (700, 42) is the LDS kernel's, bit for bit."""
import functools

import numpy as np
import pytest
import torch

import frames
import table_shapes as ts
from oracle import c_oracle

pytestmark = pytest.mark.gpu

V = 6                       # one workgroup per voxel
N_ITER = 60
EPS, RTOL_J = 1.0e-10, 1.0e-10          # tests/test_gpu_long_hrf.py
VS_LDS = 1.0e-9
FORCE = "split_long_hrf"


@pytest.fixture(scope="module")
def solver():
    from pybold_amd import solver
    return solver


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def rel_rows(a, b):
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    return float((np.linalg.norm(a - b, axis=1) / (np.linalg.norm(b, axis=1) + 1e-300)).max())


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - b) / (np.linalg.norm(b) + 1e-300)


def same(a, b):
    """Bit equality that sees NaN padding."""
    if a is None or b is None:
        return a is None and b is None
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


@functools.lru_cache(maxsize=None)
def problems(N, K):
    """V rows: noise, one HRF (first tap 0, as every SPM HRF) and its step, V HRFs with their own steps (gains of the first:
    the spectral norm scales with the gain), a warm start, one lambda per row with a NEGATIVE one in row 1."""
    rng = np.random.RandomState(977 * N + K)
    hrf = 0.3 * rng.randn(K)
    if K > 1:
        hrf[0] = 0.0
    else:
        hrf[0] = 1.0
    lip = ts.lipschitz(hrf, N)
    Y = rng.randn(V, N)
    W0 = 0.01 * rng.randn(V, N)
    lam = 0.5 * (0.5 + rng.rand(V))
    lam[1] = -0.02
    taps_pp, steps = ts.scaled_taps(hrf, lip, V)
    for a in (hrf, Y, W0, lam, taps_pp, steps):
        a.setflags(write=False)
    return dict(hrf=hrf, step=1.0 / lip, Y=Y, W0=W0, lam=lam, taps_pp=np.ascontiguousarray(taps_pp), steps=np.asarray(steps))


VARIANTS = (dict(), dict(want_J=True), dict(want_J=True, warm=True, lam=True), dict(stop="loops", tol=2e-2, want_J=True),
            dict(stop="window", tol=2e-2, want_J=True), dict(stop="window", tol=2e-2, warm=True, lam=True))


def run(solver, p, force, pp=False, want_J=False, warm=False, lam=False, stop=None, tol=0.0, n_iter=N_ITER):
    Y = dev(p["Y"])
    lbda = p["lam"] if lam else 0.5
    W0 = dev(p["W0"]) if warm else None
    if pp:
        return solver.fista_solve_pp_d(Y, dev(p["taps_pp"]), p["steps"], lbda, n_iter, W0=W0, want_J=want_J, stop=stop, tol=tol, force=force)
    return solver.fista_solve(Y, p["hrf"], lbda, p["step"], n_iter, W0=W0, want_J=want_J, stop=stop, tol=tol, force=force)


# ---- 1. the bits of the existing four-wave forms where both exist ---------------------------------------------------------
@pytest.mark.parametrize("N", [641, 960, 961, 1280])
@pytest.mark.parametrize("K", [1, 30, 32])
def test_up_to_32_taps_the_bits_of_the_existing_four_wave_kernels(solver, N, K):
    """force="split_long_hrf" against the default fista_solve (pb_fista_which_kernel_d says 8: fista_exact_split_kernel) and
    against fista_solve_pp_d(force="split") (fista_exact_split_pp_kernel), KT = 32: plain, cost trace, warm start with one
    lambda per row (one of them negative), both stop rules -- W, n_done and J with torch.equal.  Then the search against
    auto_lbda_solve_split / auto_lbda_solve_split_pp: w, n_outer, n_inner, alpha, lbda, R, G, J."""
    from pybold_amd import _lib
    assert _lib.load().pb_fista_which_kernel_d(N, K, 1, 2, 6) == 8
    p = problems(N, K)
    fired = set()
    for pp in (False, True):
        for kw in VARIANTS:
            a, b = run(solver, p, FORCE, pp, **kw), run(solver, p, "split" if pp else None, pp, **kw)
            assert torch.equal(a[0], b[0]), (N, K, pp, kw, float((a[0] - b[0]).abs().max()))
            assert torch.equal(a[2], b[2]), (N, K, pp, kw, a[2].tolist(), b[2].tolist())
            assert same(a[1], b[1]), (N, K, pp, kw)
            assert bool(torch.isfinite(a[0]).all())
            if kw.get("stop"):
                fired |= set(a[2].tolist())
    print("N=%d K=%d: stop rules left at %s" % (N, K, sorted(fired)))
    Y, sigma = dev(p["Y"]), 0.8 + 0.1 * np.arange(V)
    for nb_iter, nb_sub, tol in ((12, 25, 1e-1), (5, 30, 1e-6)):
        kw = dict(tol=tol, nb_iter=nb_iter, nb_sub_iter=nb_sub)
        for long_fn, ref_fn, args in ((solver.auto_lbda_solve_split_long, solver.auto_lbda_solve_split, (p["hrf"], p["step"])),
                                      (solver.auto_lbda_solve_split_long_pp, solver.auto_lbda_solve_split_pp,
                                       (dev(p["taps_pp"]), p["steps"]))):
            (Wa, ra), (Wb, rb) = long_fn(Y, *args, sigma, **kw), ref_fn(Y, *args, sigma, **kw)
            assert torch.equal(Wa, Wb), (N, K, kw, long_fn.__name__)
            for k in ("n_outer", "n_inner", "alpha", "lbda", "R", "G", "J"):
                assert same(ra[k], rb[k]), (N, K, kw, long_fn.__name__, k)


# ---- 2. the new ground: 33 .. 48 taps -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_runs(N, K):
    p = problems(N, K)
    out = {"cold": c_oracle.fista_batch(p["Y"], p["hrf"], 0.5, p["step"], N_ITER, want_J=True, threads=4)[:2],
           "warm": c_oracle.fista_batch(p["Y"], p["hrf"], p["lam"], p["step"], N_ITER, W0=p["W0"], want_J=True, threads=4)[:2]}
    res = [c_oracle.fista_batch(p["Y"][v:v + 1], p["taps_pp"][v], float(p["lam"][v]), float(p["steps"][v]), N_ITER,
                                W0=p["W0"][v:v + 1], want_J=True, threads=1) for v in range(V)]
    out["pp_warm"] = (np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res]))
    return out


@pytest.mark.parametrize("N", [641, 688, 689, 960, 961, 1279, 1280])
@pytest.mark.parametrize("K", [33, 42, 47, 48])
def test_33_to_48_taps_against_the_oracle_and_the_lds_kernel(solver, N, K):
    """Every variant through force="split_long_hrf": the iterate and the cost trace of the variants without a stop rule
    against the C oracle (1e-10), every variant against the same call without the flag (pb_fista_which_kernel_d says 0: the
    LDS kernel) within 1e-9 with n_done equal."""
    from pybold_amd import _lib
    lib = _lib.load()
    p, o = problems(N, K), oracle_runs(N, K)
    assert lib.pb_fista_which_kernel_d(N, K, 1, 2, 6) == 0 and lib.pb_fista_which_kernel_pp_d(N, K, 1, 2, 6) == 0
    assert lib.pb_fista_split_long_hrf_supported(N, K, 2, 6) == 1
    worst = {"oracle": 0.0, "J": 0.0, "lds": 0.0}
    for pp in (False, True):
        for kw in VARIANTS:
            W, J, nd = run(solver, p, FORCE, pp, **kw)
            Wl, Jl, ndl = run(solver, p, None, pp, **kw)
            Wn, Wln = W.cpu().numpy(), Wl.cpu().numpy()
            assert torch.equal(nd, ndl), (N, K, pp, kw, nd.tolist(), ndl.tolist())
            live = np.linalg.norm(Wln, axis=1) > 0
            e = rel_rows(Wn[live], Wln[live]) if live.any() else 0.0
            worst["lds"] = max(worst["lds"], e)
            assert e < VS_LDS, (N, K, pp, kw, e)
            assert np.abs(Wn[~live]).max(initial=0.0) == 0.0
            if J is not None:
                Jn, Jln = J.cpu().numpy(), Jl.cpu().numpy()
                assert np.array_equal(np.isnan(Jn), np.isnan(Jln)), (N, K, pp, kw)
                np.testing.assert_allclose(Jn, Jln, rtol=VS_LDS)
            key = None
            if not kw.get("stop"):
                key = ("pp_warm" if pp else "warm") if kw.get("warm") else (None if pp else "cold")
            if key:
                Wr, Jr = o[key]
                e = rel_rows(Wn, Wr)
                worst["oracle"] = max(worst["oracle"], e)
                assert (nd.cpu().numpy() == N_ITER).all() and e < EPS, (N, K, pp, kw, e)
                if J is not None:
                    worst["J"] = max(worst["J"], float(np.abs(J.cpu().numpy() / Jr - 1.0).max()))
                    np.testing.assert_allclose(J.cpu().numpy(), Jr, rtol=RTOL_J)
    # lambda < 0 on every row: the last sample has no gradient (h[0] = 0) and stays exactly 0 from a cold start
    Wneg = solver.fista_solve(dev(p["Y"]), p["hrf"], -0.02, p["step"], N_ITER, force=FORCE)[0]
    assert bool((Wneg[:, N - 1] == 0.0).all()) and bool(torch.isfinite(Wneg).all())
    Wc = run(solver, p, FORCE, False)[0]
    assert bool((Wc[:, N - 1] == 0.0).all())
    print("N=%d K=%d worst: vs oracle %.2e (cost trace %.2e), vs LDS kernel %.2e" % (N, K, worst["oracle"], worst["J"], worst["lds"]))


# ---- 6. refusals, and nothing changes without the flag ---------------------------------------------------------------------
def test_the_flag_is_refused_outside_its_shapes_and_changes_nothing_without_it(solver):
    p = problems(700, 42)
    Y = dev(p["Y"])
    with pytest.raises(Exception, match="641..1280"):
        solver.fista_solve(dev(np.zeros((2, 640))), p["hrf"], 1.0, p["step"], 10, force=FORCE)
    with pytest.raises(Exception, match="641..1280"):
        solver.fista_solve(dev(np.zeros((2, 1281))), p["hrf"], 1.0, p["step"], 10, force=FORCE)
    with pytest.raises(Exception, match="1..48"):
        solver.fista_solve(Y, np.ones(49), 1.0, p["step"], 10, force=FORCE)
    with pytest.raises(Exception, match="wind"):
        solver.fista_solve(Y, p["hrf"], 1.0, p["step"], 10, stop="window", wind=4, force=FORCE)
    with pytest.raises(Exception, match="wind"):
        solver.fista_solve_pp_d(Y, dev(p["taps_pp"]), p["steps"], 1.0, 10, stop="window", wind=8, force=FORCE)
    with pytest.raises(Exception, match="1..640"):                      # PB_FLAG_LONG_HRF keeps its limit
        solver.fista_solve(Y, p["hrf"], 1.0, p["step"], 10, force="long_hrf")
    # switch off, no flag: a 42-tap call of 700 scans is the LDS kernel, bit for bit what force="generic" returns
    for pp in (False, True):
        a = run(solver, p, None, pp, want_J=True, stop="window", tol=2e-2)
        b = run(solver, p, "generic", pp, want_J=True, stop="window", tol=2e-2)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and same(a[1], b[1])


# ---- 3. the search ------------------------------------------------------------------------------------------------------
SEARCH_CASES = ("k33_n700", "k42_n1200", "k48_n1280")
SCALES = (1.0, 1.5, 2.0, 3.0)
BUDGETS = ((40, 30, 1.0e-1), (12, 20, 1.0e-6))            # (nb_iter, nb_sub_iter, tol): the alpha window fires / does not


def search_rows(g, case):
    """24 rows of a case of split_long_hrf.npz: sc * y and sc * y[::-1] for four scales, each with the case's three noise levels."""
    y, sig = g[case + "_y"], g[case + "_sigma"]
    rows = [(sc * base, float(s)) for sc in SCALES for base in (y, y[::-1].copy()) for s in sig]
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows])


def _auto(y, hrf, sigma, **kw):
    import pybold_amd
    np.random.seed(0)                       # spectral_radius_est draws from the global RNG, as the fixtures did
    return pybold_amd.deconv_auto(y, 1.0, hrf, sigma=sigma, **kw)


@pytest.mark.parametrize("case", SEARCH_CASES)
@pytest.mark.parametrize("budget", BUDGETS)
def test_alpha_window_against_the_oracle_and_the_host_engine(golden, case, budget):
    """n_outer equal to the C oracle's and to the host engine's on every row; R, G, J, diff_z, alpha, lbda within 1e-9 of
    the host engine (the host loop's inner solves run on the LDS kernel: the same float64 operations, other reduction
    orders).  The oracle keeps |alpha| > 1e-2 on every row (asserted on its run; 0.115 at the least), so no row is near the
    pole alpha = 0."""
    g = golden("split_long_hrf")
    Y, sigma = search_rows(g, case)
    hrf = g[case + "_hrf"]
    nb_iter, nb_sub_iter, tol = budget
    _, _, Ro, _, n_oracle = c_oracle.deconv_auto_lbda_batch(Y, hrf, sigma, float(g[case + "_lipschitz"]), nb_iter=nb_iter,
                                                            nb_sub_iter=nb_sub_iter, tol=tol, threads=8)
    alphas = [1.0 + np.cumsum(1.0e-4 * (Ro[v, :n_oracle[v]] - Y.shape[1] * sigma[v] ** 2)) for v in range(len(sigma))]
    assert min(np.abs(a).min() for a in alphas) > 1.0e-2
    if tol == 1.0e-1:
        print("oracle n_outer:", sorted(set(n_oracle.tolist())))
        assert (n_oracle < nb_iter).any() and len(set(n_oracle.tolist())) >= 3
    else:
        assert (n_oracle == nb_iter).all()
    out = {e: _auto(Y, hrf, sigma, nb_iter=nb_iter, nb_sub_iter=nb_sub_iter, tol=tol, engine=e) for e in ("device_split_long_hrf", "host")}
    d, h = out["device_split_long_hrf"], out["host"]
    assert d[6]["engine"] == "device_split_long_hrf" and h[6]["engine"] == "host"
    assert np.array_equal(d[6]["n_outer"], n_oracle), (d[6]["n_outer"], n_oracle)
    assert np.array_equal(d[6]["n_outer"], h[6]["n_outer"])
    assert d[3].shape == h[3].shape
    worst = 0.0
    for v in range(Y.shape[0]):
        n = int(h[6]["n_outer"][v])
        errs = [rel(d[2][v], h[2][v])] + [rel(d[k][:n, v], h[k][:n, v]) for k in (3, 4, 5)]
        assert np.isnan(d[3][n:, v]).all() and np.isnan(h[3][n:, v]).all()
        assert max(errs) < 1e-9, (case, budget, v, errs)
        worst = max(worst, max(errs))
    assert rel(d[6]["alpha"], h[6]["alpha"]) < 1e-9 and rel(d[6]["lbda"], h[6]["lbda"]) < 1e-9
    print("%s %s: device_split_long_hrf vs host worst rel. error %.2e over %d rows, n_outer %d..%d, rows with alpha < 0: %d"
          % (case, budget, worst, Y.shape[0], n_oracle.min(), n_oracle.max(), sum(bool((a < 0).any()) for a in alphas)))


def _same_search(res, ref, what):
    for k in ("alpha", "lbda", "n_outer", "n_inner", "R", "G", "J"):
        assert same(res[k], ref[k]), (what, k)


@pytest.mark.parametrize("pp", [False, True])
def test_chunking_is_invisible_and_a_voxel_is_alone_in_its_batch(golden, solver, pp):
    """outer_chunk in {1, 7, nb_iter} and the library's choice: bit-identical outputs on the 24 rows of k42_n1200, with the
    alpha window firing, without it, and with early stopping off.  Row 5 solved alone equals its row of the batch.  A warm
    start is read and not modified; the traces are optional.  With one HRF per voxel (the shared one under a gain per row)
    likewise."""
    g = golden("split_long_hrf")
    Y, sigma = search_rows(g, "k42_n1200")
    hrf, lip = g["k42_n1200_hrf"], float(g["k42_n1200_lipschitz"])
    Yd = torch.from_numpy(Y).cuda()
    if pp:
        T, steps = ts.scaled_taps(hrf, lip, Y.shape[0])
        Td, steps = dev(T), np.asarray(steps)

        def solve(rows, **kw):
            return solver.auto_lbda_solve_split_long_pp(Yd[rows].contiguous(), Td[rows].contiguous(), steps[rows], sigma[rows], **kw)
    else:
        def solve(rows, **kw):
            return solver.auto_lbda_solve_split_long(Yd[rows].contiguous(), hrf, 1.0 / lip, sigma[rows], **kw)
    every = slice(0, Y.shape[0])
    for nb_iter, nb_sub_iter, tol, es in ((20, 10, 1e-6, True), (40, 30, 1e-1, True), (9, 12, 1e-1, False)):
        kw = dict(tol=tol, nb_iter=nb_iter, nb_sub_iter=nb_sub_iter, early_stopping=es)
        ref = None
        for chunk in (1, 7, nb_iter, 0):
            W, res = solve(every, outer_chunk=chunk, **kw)
            if ref is None:
                ref = (W, res)
                if not es:          # early stopping off: every outer and every inner iteration runs
                    assert bool((res["n_outer"] == nb_iter).all()) and bool((res["n_inner"] == (nb_iter + 1) * nb_sub_iter).all())
                elif nb_iter == 40:
                    assert int(res["n_outer"].min()) < int(res["n_outer"].max())
                continue
            assert torch.equal(W, ref[0]), chunk
            _same_search(res, ref[1], chunk)
        W1, res1 = solve(slice(5, 6), **kw)
        assert torch.equal(W1[0], ref[0][5])
        _same_search(res1, {k: t[5:6] for k, t in ref[1].items()}, "alone")
    W0 = ref[0].clone()
    W1, res1 = solve(every, nb_iter=3, nb_sub_iter=10, W0=W0, want_trace=False)
    assert torch.equal(W0, ref[0]) and res1["R"] is None and res1["G"] is None and res1["J"] is None and not torch.equal(W1, W0)


def test_registered_operator_matches_ctypes_and_the_search_is_capturable(golden, solver):
    """torch.ops.pybold_hip.auto_lbda_solve_split_long is the ctypes call; no host synchronisation and no allocation inside
    pb_auto_lbda_split_long_d: its launches replay from a captured graph."""
    from pybold_amd import torch_ops
    g = golden("split_long_hrf")
    hrf, step = g["k42_n1200_hrf"], 1.0 / float(g["k42_n1200_lipschitz"])
    Yd = torch.from_numpy(np.repeat(g["k42_n1200_y"][None, :], 3, axis=0)).cuda()
    sig = torch.from_numpy(g["k42_n1200_sigma"]).cuda()
    kw = dict(nb_iter=6, nb_sub_iter=20, outer_chunk=2)
    W, res = solver.auto_lbda_solve_split_long(Yd, hrf, step, sig, **kw)
    W2, res2 = torch_ops.auto_lbda_solve_split_long(Yd, hrf, step, sig, **kw)
    assert torch.equal(W, W2)
    _same_search(res2, res, "operator")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        solver.auto_lbda_solve_split_long(Yd, hrf, step, sig, **kw)                # warm the capture stream
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            Wg, resg = solver.auto_lbda_solve_split_long(Yd, hrf, step, sig, **kw)
    Wg.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(Wg, W) and torch.equal(resg["alpha"], res["alpha"]) and torch.equal(resg["n_inner"], res["n_inner"])


# ---- 4. the reference's own runs ----------------------------------------------------------------------------------------
REF_CASES = ("k42_n1200", "k33_n700", "k48_n1280")
REF_BUDGETS = ((20, 50, 1e-6), (60, 300, 1e-3))


@pytest.mark.parametrize("case", REF_CASES)
def test_reference_runs_through_deconv_with_the_switch_on(golden, case, monkeypatch):
    """Fixed lambda (early stopping on / off) and every kept lbda=None run (the host loop) of split_long_hrf.npz through
    `deconv` under bold_signal.SPLIT_LONG_HRF, as 1-D calls and with the HRF tiled to (V, K): x, z, diff_z, J (R, G) within
    1e-6, the number of iterations equal.  Every solve must have gone through force="split_long_hrf".

    Worst figure measured on an MI355X: 4.0e-14 (k33_n700; 2.3e-14 on the HCP run k42_n1200, 3.8e-14 on k48_n1280)."""
    import pybold_amd
    from pybold_amd import bold_signal
    g = golden("split_long_hrf")
    y, hrf, t_r, sig = g[case + "_y"], g[case + "_hrf"], float(g[case + "_t_r"]), g[case + "_sigma"]
    kept = set(g["auto_tags"].tolist())
    monkeypatch.setattr(bold_signal, "SPLIT_LONG_HRF", True)
    forces = []
    real, real_pp = bold_signal.solver.fista_solve, bold_signal.solver.fista_solve_pp_d
    monkeypatch.setattr(bold_signal.solver, "fista_solve", lambda *a, **k: (forces.append(k.get("force")), real(*a, **k))[1])
    monkeypatch.setattr(bold_signal.solver, "fista_solve_pp_d", lambda *a, **k: (forces.append(k.get("force")), real_pp(*a, **k))[1])
    worst = 0.0
    for es in (1, 0):
        tag = "%s_fix_es%d" % (case, es)
        for tiled in (False, True):
            np.random.seed(0)
            if tiled:
                x, z, dz, J, _, _ = pybold_amd.deconv(np.repeat(y[None, :], 2, axis=0), t_r, np.repeat(hrf[None, :], 2, axis=0), lbda=1.0,
                                                      nb_iter=200, early_stopping=bool(es), tol=1e-6, wind=6)
                x, z, dz, J = x[1], z[1], dz[1], J[1][~np.isnan(J[1])]
            else:
                x, z, dz, J, _, _ = pybold_amd.deconv(y, t_r, hrf, lbda=1.0, nb_iter=200, early_stopping=bool(es), tol=1e-6, wind=6)
            assert len(J) == len(g["J_" + tag]), (tag, tiled, len(J), len(g["J_" + tag]))
            errs = [rel(dz, g["dz_" + tag]), rel(z, g["z_" + tag]), rel(x, g["x_" + tag]), rel(J, g["J_" + tag])]
            worst = max(worst, max(errs))
            assert max(errs) <= 1e-6, (tag, tiled, errs)
    real_mad = bold_signal.mad_daub_noise_est
    n_auto = 0
    for si in range(3):
        monkeypatch.setattr(bold_signal, "mad_daub_noise_est", lambda x, s=float(sig[si]): np.full(np.atleast_2d(x).shape[0], s))
        for o, i, tol in REF_BUDGETS:
            tag = "%s_s%d_o%d_i%d_t%g" % (case, si, o, i, tol)
            if tag not in kept:
                continue
            n_auto += 1
            np.random.seed(0)
            x, z, dz, J, R, G = pybold_amd.deconv(y, t_r, hrf, lbda=None, nb_iter=o, nb_sub_iter=i, early_stopping=True, tol=tol, wind=6)
            assert len(J) == len(g["J_" + tag]) and len(R) == len(g["R_" + tag]) and len(G) == len(g["G_" + tag]), (tag, len(J))
            errs = [rel(dz, g["dz_" + tag]), rel(z, g["z_" + tag]), rel(x, g["x_" + tag]), rel(J, g["J_" + tag]),
                    rel(R, g["R_" + tag]), rel(G, g["G_" + tag])]
            worst = max(worst, max(errs))
            assert max(errs) <= 1e-6, (tag, errs)
    monkeypatch.setattr(bold_signal, "mad_daub_noise_est", real_mad)
    assert n_auto >= 3, (case, n_auto)
    assert forces and set(forces) == {"split_long_hrf"}, forces
    print("%s through deconv (SPLIT_LONG_HRF on): worst rel. error %.2e over %d solves" % (case, worst, len(forces)))


@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("case", REF_CASES)
def test_reference_runs_through_the_device_engine(golden, case, tiled):
    """The kept lbda=None runs of a case (the sigmas as the rows of one call per budget) through
    deconv_auto(engine="device_split_long_hrf"), with a shared HRF and with the HRF tiled to (V, K): n_outer equal to the
    reference's, x, z, diff_z, J, R, G within 1e-6."""
    g = golden("split_long_hrf")
    y, hrf, t_r, sig = g[case + "_y"], g[case + "_hrf"], float(g[case + "_t_r"]), g[case + "_sigma"]
    kept = set(g["auto_tags"].tolist())
    worst, n_runs = 0.0, 0
    for o, i, tol in REF_BUDGETS:
        rows = [s for s in range(3) if "%s_s%d_o%d_i%d_t%g" % (case, s, o, i, tol) in kept]
        if not rows:
            continue
        tags = ["%s_s%d_o%d_i%d_t%g" % (case, s, o, i, tol) for s in rows]
        H = np.repeat(hrf[None, :], len(rows), axis=0) if tiled else hrf
        X, Z, W, J, R, G, info = _auto(np.repeat(y[None, :], len(rows), axis=0), H, sig[rows].copy(), nb_iter=o, nb_sub_iter=i,
                                       early_stopping=True, tol=tol, wind=6, engine="device_split_long_hrf")
        assert info["engine"] == "device_split_long_hrf"
        n_ref = [len(g["J_" + t]) for t in tags]
        assert J.shape == R.shape == G.shape == (max(n_ref), len(rows))
        for s, tag in enumerate(tags):
            n = n_ref[s]
            assert int(info["n_outer"][s]) == n, (tag, int(info["n_outer"][s]), n)
            for T in (J, R, G):
                assert np.isnan(T[n:, s]).all() and not np.isnan(T[:n, s]).any(), tag
            errs = [rel(W[s], g["dz_" + tag]), rel(Z[s], g["z_" + tag]), rel(X[s], g["x_" + tag]),
                    rel(J[:n, s], g["J_" + tag]), rel(R[:n, s], g["R_" + tag]), rel(G[:n, s], g["G_" + tag])]
            worst = max(worst, max(errs))
            assert max(errs) <= 1e-6, (tag, tiled, errs)
            n_runs += 1
    assert n_runs >= 3, (case, n_runs)
    print("%s tiled=%s through the device engine: worst rel. error %.2e over %d runs" % (case, tiled, worst, n_runs))


def test_the_switch_for_the_search(golden, monkeypatch):
    """bold_signal.AUTO_LBDA = "device_split_long_hrf": a 2-D deconv(lbda=None) with 42 taps at 1 200 scans returns what
    deconv_auto(engine="device_split_long_hrf") returns; one with 30 taps goes to the existing four-wave engine;
    "device_split" keeps the host loop for 42 taps."""
    import pybold_amd
    from pybold_amd import bold_signal
    g = golden("split_long_hrf")
    y, hrf = g["k42_n1200_y"], g["k42_n1200_hrf"]
    Y = np.repeat(y[None, :], 3, axis=0) * np.array([1.0, 1.5, 2.0])[:, None]
    kw = dict(nb_iter=8, nb_sub_iter=20)
    calls = {"long": 0, "split": 0}
    real_long, real_split = bold_signal.solver.auto_lbda_solve_split_long, bold_signal.solver.auto_lbda_solve_split
    monkeypatch.setattr(bold_signal.solver, "auto_lbda_solve_split_long",
                        lambda *a, **k: (calls.__setitem__("long", calls["long"] + 1), real_long(*a, **k))[1])
    monkeypatch.setattr(bold_signal.solver, "auto_lbda_solve_split",
                        lambda *a, **k: (calls.__setitem__("split", calls["split"] + 1), real_split(*a, **k))[1])
    monkeypatch.setattr(bold_signal, "AUTO_LBDA", "device_split")
    np.random.seed(0)
    host = pybold_amd.deconv(Y, 1.0, hrf, lbda=None, **kw)
    assert calls == {"long": 0, "split": 0}
    monkeypatch.setattr(bold_signal, "AUTO_LBDA", "device_split_long_hrf")
    np.random.seed(0)
    got = pybold_amd.deconv(Y, 1.0, hrf, lbda=None, **kw)
    want = _auto(Y, hrf, None, engine="device_split_long_hrf", **kw)
    assert calls == {"long": 2, "split": 0} and len(got) == 6
    for a, b, c in zip(got, want[:6], host):
        assert np.array_equal(a, b, equal_nan=True)
        assert np.asarray(a).shape == np.asarray(c).shape
    np.random.seed(0)
    pybold_amd.deconv(Y, 1.0, hrf[:30].copy(), lbda=None, **kw)
    assert calls == {"long": 2, "split": 1}
    # deconv_auto with the engine named and 30 taps: what "device_split" does
    info = _auto(Y, hrf[:30].copy(), None, engine="device_split_long_hrf", **kw)[6]
    assert info["engine"] == "device_split" and calls == {"long": 2, "split": 2}


# ---- 5. layout ----------------------------------------------------------------------------------------------------------
def test_padded_leading_dimensions_and_guards(solver):
    """N = 961, K = 42 through the frames of tests/frames.py: y, W, J, taps_pp and the traces as windows of larger
    allocations (pads left and right of every row, guard rows, guards around every vector).  Inputs come back untouched,
    nothing outside an output's window changes, and the windows hold the bits of the packed calls."""
    from pybold_amd import _lib
    lib = _lib.load()
    N, K = 961, 42
    p = problems(N, K)
    d = torch.device("cuda", torch.cuda.current_device())
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    flags = 0
    n_iter, tol = N_ITER, 2e-2
    for pp in (False, True):
        y = frames.frame2d("y", V, N, f64, d, fill=p["Y"]).snapshot()
        w = frames.frame2d("W", V, N, f64, d, fill=p["W0"])
        J = frames.frame2d("J", V, n_iter, f64, d).snapshot()
        n_done = frames.frame1d("n_done", V, i32, d).snapshot()
        lam = frames.frame1d("lbda", V, f64, d, fill=p["lam"]).snapshot()
        betas = frames.betas_frame(d, n_iter)
        w.snapshot()
        if pp:
            taps = frames.frame2d("taps_pp", V, K, f64, d, fill=p["taps_pp"]).snapshot()
            steps = frames.frame1d("steps", V, f64, d, fill=p["steps"]).snapshot()
            rc = lib.pb_fista_solve_split_long_pp_d(y.ptr, y.ld, 1, w.ptr, w.ld, V, N, taps.ptr, taps.ld, K, steps.ptr, 0.0, lam.ptr,
                                                    betas.ptr, n_iter, J.ptr, J.ld, 2, tol, 6, n_done.ptr, flags, solver._stream_ptr(d))
            _lib.check(rc, "pb_fista_solve_split_long_pp_d")
        else:
            hrf = np.ascontiguousarray(p["hrf"])
            rc = lib.pb_fista_solve_split_long_d(y.ptr, y.ld, 1, w.ptr, w.ld, V, N, hrf.ctypes.data, None, K, float(p["step"]), 0.0,
                                                 lam.ptr, betas.ptr, n_iter, J.ptr, J.ld, 2, tol, 6, n_done.ptr, flags,
                                                 solver._stream_ptr(d))
            _lib.check(rc, "pb_fista_solve_split_long_d")
        torch.cuda.synchronize()
        for f in (y, lam, betas) + ((taps, steps) if pp else ()):
            f.assert_untouched()
        for f in (w, J, n_done):
            f.assert_outside_untouched()
        Wp, Jp, ndp = run(solver, p, FORCE, pp, want_J=True, warm=True, lam=True, stop="window", tol=tol)
        assert torch.equal(w.contiguous(), Wp) and torch.equal(n_done.contiguous(), ndp)
        nd = ndp.cpu().numpy()
        for v in range(V):           # the trace up to a row's last iteration; beyond it the sentinel is still there
            assert torch.equal(J.view[v, :nd[v]], Jp[v, :nd[v]]) and bool(J.is_sentinel()[v, nd[v]:].all())
        # the search on framed buffers
        nb_iter, nb_sub = 9, 20
        sigma = frames.frame1d("sigma", V, f64, d, fill=0.8 + 0.1 * np.arange(V)).snapshot()
        w = frames.frame2d("W", V, N, f64, d).snapshot()
        tr = [frames.frame2d("trace", V, nb_iter, f64, d).snapshot() for _ in range(3)]
        alpha, lbda = (frames.frame1d(n, V, f64, d).snapshot() for n in ("alpha", "lbda"))
        n_outer, n_inner = frames.frame1d("n_outer", V, i32, d).snapshot(), frames.frame1d("n_inner", V, i64, d).snapshot()
        work = frames.frame1d("work", int(lib.pb_auto_lbda_work_len(V)), f64, d).snapshot()
        betas = frames.betas_frame(d, nb_sub)
        tail = (betas.ptr, sigma.ptr, 1, 1e-1, 6, nb_iter, nb_sub, 4, tr[0].ptr, tr[1].ptr, tr[2].ptr, tr[0].ld, alpha.ptr, lbda.ptr,
                n_outer.ptr, n_inner.ptr, work.ptr, work.n, solver._stream_ptr(d))
        if pp:
            rc = lib.pb_auto_lbda_split_long_pp_d(y.ptr, y.ld, w.ptr, w.ld, 1, V, N, taps.ptr, taps.ld, K, steps.ptr, *tail)
        else:
            rc = lib.pb_auto_lbda_split_long_d(y.ptr, y.ld, w.ptr, w.ld, 1, V, N, hrf.ctypes.data, K, float(p["step"]), *tail)
        _lib.check(rc, "pb_auto_lbda_split_long")
        torch.cuda.synchronize()
        for f in (y, sigma, betas) + ((taps, steps) if pp else ()):
            f.assert_untouched()
        for f in [w, alpha, lbda, n_outer, n_inner, work] + tr:
            f.assert_outside_untouched()
        kw = dict(tol=1e-1, nb_iter=nb_iter, nb_sub_iter=nb_sub)
        if pp:
            Wp, res = solver.auto_lbda_solve_split_long_pp(dev(p["Y"]), dev(p["taps_pp"]), p["steps"], 0.8 + 0.1 * np.arange(V), **kw)
        else:
            Wp, res = solver.auto_lbda_solve_split_long(dev(p["Y"]), p["hrf"], p["step"], 0.8 + 0.1 * np.arange(V), **kw)
        assert torch.equal(w.contiguous(), Wp) and torch.equal(n_outer.contiguous(), res["n_outer"])
        assert torch.equal(alpha.contiguous(), res["alpha"]) and torch.equal(n_inner.contiguous(), res["n_inner"])
        no = res["n_outer"].cpu().numpy()
        for t, k in zip(tr, ("R", "G", "J")):
            for v in range(V):
                assert torch.equal(t.view[v, :no[v]], res[k][v, :no[v]]) and bool(t.is_sentinel()[v, no[v]:].all()), (k, v)
