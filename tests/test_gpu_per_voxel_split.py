"""The opt-in four-wave form with one HRF per voxel on the GPU (series of 641 .. 1 280 scans): `fista_exact_split_pp_kernel`
behind `pb_fista_solve_pp_d | PB_FLAG_PP_SPLIT`, `auto_lbda_split_pp_kernel` behind `pb_auto_lbda_split_pp_d`, and the
switches above them (`force="split"`, `PER_VOXEL_SPLIT`, `engine="device_split_pp"`, `AUTO_LBDA="device_split_pp"`).

Bounds.
  * Row v of a per-voxel call against the single-HRF four-wave call of that row (`pb_fista_solve_d`, code 8 of
    `pb_fista_which_kernel_d`; `pb_auto_lbda_split_d`): BIT FOR BIT on every output.  Both kernels run the same pass
    halves (csrc/fista_exact_split.h: split_forward / split_backward) on the same inputs; only the place the taps and
    the step are read from differs -- as tests/test_gpu_per_voxel_hrf.py holds the one-wave form to.
  * `deconv` with `PER_VOXEL_SPLIT` against the reference's 1 200-scan fixture: 1e-10 relative on x, z, diff_z, rtol 1e-9
    on J (tests/test_gpu_exact_split.py::test_one_dimensional_deconv_against_the_reference holds the 1-D call to it).
  * The lambda search against the reference's runs: equal n_outer, 1e-6 (tests/test_gpu_auto_lbda_split.py); against the
    host engine on per-voxel taps: 1e-9 (the same file).
"""
import numpy as np
import pytest
import torch

from oracle import pybold_oracle as orc

pytestmark = pytest.mark.gpu

NAN = float("nan")
V3 = 3
# 641: one live sample in wave 2, wave 3 all padding; 960 / 961: the boundary of wave 3; 1 280: full.
# 32 taps: the full halo; 17; 2: a halo of one sample.
SHAPES = [(641, 32), (960, 17), (961, 2), (1280, 32)]
N_ITER, TOL = 300, 1.0e-2
# lambdas of the three rows under each stop rule at tol = 1e-2, chosen with the CPU oracle (oracle_n_done below, printed
# beside the GPU's counts) so that at every shape the rows stop at two or more different iterations below N_ITER, cold and
# warm: the oracle's counts are 101 .. 184 under the window rule and 4 .. 100 under the _loops_deconv rule, whose
# criterion -- the size of the prox step against the iterate's -- grows with lambda (at lambdas of 30 and more it does
# not fire within 300 iterations on these series).
LBDA = {"window": (0.2, 0.3, 0.4), "loops": (2.0, 6.0, 12.0)}
# the warm start: small against the solution (both stop criteria are relative to the iterate's norm: from a start of the
# solution's size they fire at their first test on every row)
W0_AMPLITUDE = 2.0e-3
LBDA_NO_RULE = (0.3, -0.2, 0.5)               # one negative: the reference's prox grows every non-zero entry by |th|


@pytest.fixture(scope="module")
def solver():
    from pybold_amd import solver as s
    return s


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - b) / (np.linalg.norm(b) + 1e-300)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def taps_for(V, K):
    """V different causal bumps of K taps with h[0] = 0 (as every HRF of the reference): shape and amplitude vary by row."""
    t = np.arange(K, dtype=np.float64)
    H = np.stack([t ** (1.0 + 0.3 * v) * np.exp(-t / (0.8 + 0.25 * v)) for v in range(V)])
    return H / H.sum(axis=1, keepdims=True) * (0.8 + 0.1 * np.arange(V))[:, None]


_cache = {}


def problems(N, K):
    """Block signals (random on/off blocks convolved with the row's HRF, noise), one HRF and one step 1 / (0.9 rho) per
    row, a warm start whose last sample is 0, as every iterate of the reference's (h[0] = 0): host float64 arrays."""
    key = (N, K)
    if key not in _cache:
        rng = np.random.RandomState(1000 * N + K)
        H = taps_for(V3, K)
        Y = np.empty((V3, N))
        for v in range(V3):
            z = np.repeat(rng.randint(0, 2, size=N // 6 + 1).astype(np.float64), 6)[:N] * (2.0 + v)
            Y[v] = np.convolve(z, H[v])[:N] + 0.3 * rng.randn(N)
        steps = np.array([1.0 / (0.9 * orc.spectral_radius_est(orc._MatrixFreeH(H[v]), rng.randn(N))) for v in range(V3)])
        W0 = W0_AMPLITUDE * rng.randn(V3, N)
        W0[:, -1] = 0.0
        _cache[key] = (Y, H, steps, W0)
    return _cache[key]


def oracle_n_done(N, K, stop, warm):
    """Iterations the CPU oracle runs on the three rows under a stop rule (float64 NumPy, matrix-free operator)."""
    Y, H, steps, W0 = problems(N, K)
    out = []
    for v in range(V3):
        lb = LBDA[stop][v]
        w0 = W0[v] if warm else None
        if stop == "loops":
            out.append(int(orc.loops_batch(Y[v:v + 1], H[v], lb, steps[v], N_ITER, TOL, W0=None if w0 is None else w0[None])[1][0]))
        else:
            out.append(int(orc.deconv_fixed_lbda(Y[v], H[v], lb, nb_iter=N_ITER, early_stopping=True, tol=TOL, wind=6,
                                                 lipschitz=1.0 / steps[v], w0=w0, dense=False)[4]))
    return out


def padded(a, pad, dtype=torch.float64):
    """(buffer, view): the rows of `a` in a CUDA buffer whose rows are `pad` elements longer, the guard band NaN."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), NAN, dtype=dtype, device="cuda")
    buf[:, :a.shape[1]] = torch.as_tensor(a, dtype=dtype)
    return buf, buf[:, :a.shape[1]]


def solve_padded(solver, Y, H, steps, lbda, n_iter, W0, want_J, stop, tol):
    """pb_fista_solve_pp_d | PB_FLAG_PP_SPLIT on buffers whose leading dimensions ldy, ldw, ldt, ldj are all padded, the
    guard bands (the tap slots K .. ldt-1 included) NaN; asserts that the guard bands come back untouched.
    -> (W, J, n_done) on the host."""
    from pybold_amd import _lib
    lib = _lib.load()
    V, N = Y.shape
    Yb, Yv = padded(Y, 5)
    Tb, Tv = padded(H, 3)
    Wb, Wv = padded(W0 if W0 is not None else np.zeros((V, N)), 7)
    Jb = torch.full((V, n_iter + 4), NAN, dtype=torch.float64, device="cuda")
    st = torch.as_tensor(steps, dtype=torch.float64).cuda()
    lb = torch.as_tensor(np.broadcast_to(lbda, (V,)).copy(), dtype=torch.float64).cuda()
    betas = solver._betas_on(Yb.device, n_iter)
    n_done = torch.full((V,), -7, dtype=torch.int32, device="cuda")
    flags = _lib.PB_FLAG_PP_SPLIT | (_lib.PB_FLAG_COLD_START if W0 is None else 0)
    rc = lib.pb_fista_solve_pp_d(Yv.data_ptr(), Yb.stride(0), 1, Wv.data_ptr(), Wb.stride(0), V, N, Tv.data_ptr(), Tb.stride(0),
                                 H.shape[1], st.data_ptr(), 0.0, lb.data_ptr(), betas.data_ptr(), n_iter,
                                 Jb.data_ptr() if want_J else None, Jb.stride(0) if want_J else 0, solver._STOP[stop], tol, 6,
                                 n_done.data_ptr(), flags, solver._stream_ptr(Yb.device))
    _lib.check(rc, "pb_fista_solve_pp_d")
    torch.cuda.synchronize()
    assert torch.isnan(Wb[:, N:]).all() and torch.isnan(Jb[:, n_iter:]).all(), "guard band written"
    assert torch.isnan(Yb[:, N:]).all() and torch.isnan(Tb[:, H.shape[1]:]).all()
    assert torch.equal(Yv, torch.as_tensor(Y).cuda()) and torch.equal(Tv, torch.as_tensor(H).cuda())
    if not want_J:
        assert torch.isnan(Jb).all()
    return Wv.cpu().numpy(), (Jb[:, :n_iter].cpu().numpy() if want_J else None), n_done.cpu().numpy()


def solve_rows(solver, Y, H, steps, lbda, n_iter, W0, want_J, stop, tol):
    """The same problems one by one through the single-HRF entry point (pb_fista_solve_d: the four-wave kernel with the
    taps by value)."""
    Yd = torch.as_tensor(Y).cuda()
    W0d = torch.as_tensor(W0).cuda() if W0 is not None else None
    lb = np.broadcast_to(lbda, (Y.shape[0],))
    Ws, Js, nd = [], [], []
    for v in range(Y.shape[0]):
        W, J, n = solver.fista_solve(Yd[v:v + 1], H[v], float(lb[v]), float(steps[v]), n_iter,
                                     W0=None if W0d is None else W0d[v:v + 1], want_J=want_J, stop=stop, tol=tol, wind=6)
        Ws.append(W.cpu().numpy()[0])
        Js.append(J.cpu().numpy()[0] if want_J else None)
        nd.append(int(n[0]))
    return np.stack(Ws), (np.stack(Js) if want_J else None), np.array(nd)


# ---- 1. solver ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", SHAPES)
def test_solver_equals_the_single_hrf_four_wave_kernel_row_by_row(solver, N, K):
    """Three rows with different HRFs, steps and lambdas, every leading dimension padded: stop rules none / loops / window
    x cost trace on / off x cold / warm, W, J and n_done bit for bit against the single-HRF call of each row."""
    from pybold_amd import _lib
    lib = _lib.load()
    Y, H, steps, W0 = problems(N, K)
    assert (H[:, 0] == 0.0).all() and len({tuple(h) for h in H}) == V3 and len(set(steps.tolist())) == V3
    for stop in (None, "loops", "window"):
        assert lib.pb_fista_which_kernel_d(N, K, 1, solver._STOP[stop], 6) == 8
        assert lib.pb_fista_which_kernel_pp_d(N, K, 1, solver._STOP[stop], 6) == 0          # the default is what it was
        assert lib.pb_fista_pp_split_supported(N, K, solver._STOP[stop], 6) == 1
        n_iter, tol = (N_ITER, TOL) if stop else (40, 0.0)
        lbda = np.array(LBDA[stop] if stop else LBDA_NO_RULE)
        for warm in (False, True):
            for want_J in (True, False):
                args = (Y, H, steps, lbda, n_iter, W0 if warm else None, want_J, stop, tol)
                W, J, nd = solve_padded(solver, *args)
                Wr, Jr, ndr = solve_rows(solver, *args)
                what = (N, K, stop, want_J, warm)
                print(what, "n_done", nd.tolist(), "oracle", oracle_n_done(N, K, stop, warm) if stop and want_J else "-",
                      "max |W - W_row|", float(np.abs(W - Wr).max()))
                assert np.array_equal(nd, ndr), (what, nd, ndr)
                assert same_bits(W, Wr), (what, float(np.abs(W - Wr).max()))
                if want_J:
                    assert same_bits(J, Jr), what                  # (NaN beyond a row's n_done in both)
                    for v in range(V3):
                        assert not np.isnan(J[v, :nd[v]]).any() and np.isnan(J[v, nd[v]:]).all(), what
                if stop:            # the workgroups leave at different times, all before the iteration count
                    assert (nd < n_iter).all() and len(set(nd.tolist())) >= 2, (what, nd)
                else:
                    assert (nd == n_iter).all()
                    # lambda < 0 (row 1): sign(u) |th| is discontinuous at 0; the last sample has no gradient (h[0] = 0) and
                    # above it the suffix sum is exactly 0 in every layout -- wave 3 all padding at 641, one sample at 961
                    assert lbda[1] < 0 and (W[:, N - 1] == 0.0).all(), (what, W[:, N - 1])
    # a row alone equals that row inside the batch
    W1, J1, nd1 = solve_padded(solver, Y[1:2], H[1:2], steps[1:2], np.array(LBDA["window"][1:2]), N_ITER, W0[1:2], True, "window", TOL)
    Wb, Jb, ndb = solve_padded(solver, Y, H, steps, np.array(LBDA["window"]), N_ITER, W0, True, "window", TOL)
    assert same_bits(W1[0], Wb[1]) and same_bits(J1[0], Jb[1]) and nd1[0] == ndb[1]
    # the Python entry point is that call (contiguous buffers of its own)
    Wp, Jp, ndp = solver.fista_solve_pp_d(torch.as_tensor(Y).cuda(), torch.as_tensor(H).cuda(), steps, np.array(LBDA["window"]),
                                          N_ITER, W0=torch.as_tensor(W0).cuda(), want_J=True, stop="window", tol=TOL, force="split")
    assert same_bits(Wp.cpu().numpy(), Wb) and same_bits(Jp.cpu().numpy(), Jb) and np.array_equal(ndp.cpu().numpy(), ndb)


def test_the_flag_is_refused_outside_its_shapes_and_changes_nothing_without_it(solver):
    Y, H, steps, _ = problems(641, 32)
    Yd, Hd = torch.as_tensor(Y).cuda(), torch.as_tensor(H).cuda()
    with pytest.raises(Exception, match="641..1280"):
        solver.fista_solve_pp_d(Yd[:, :640].contiguous(), Hd, steps, 1.0, 10, force="split")
    with pytest.raises(Exception, match="wind"):
        solver.fista_solve_pp_d(Yd, Hd, steps, 1.0, 10, stop="window", wind=4, force="split")
    with pytest.raises(ValueError, match="force"):
        solver.fista_solve_pp_d(Yd, Hd, steps, 1.0, 10, force="wide")
    # without the flag: the LDS kernel, bit for bit what force="generic" returns
    a = solver.fista_solve_pp_d(Yd, Hd, steps, 0.5, 30, want_J=True, stop="window", tol=TOL)
    b = solver.fista_solve_pp_d(Yd, Hd, steps, 0.5, 30, want_J=True, stop="window", tol=TOL, force="generic")
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(torch.nan_to_num(a[1], nan=-7.0), torch.nan_to_num(b[1], nan=-7.0))


# ---- 2. lambda search ---------------------------------------------------------------------------------------------------
def _same(res, ref, what):
    for k in ("alpha", "lbda", "n_outer", "n_inner"):
        assert torch.equal(res[k], ref[k]), (what, k, res[k], ref[k])
    for k in ("R", "G", "J"):
        assert torch.equal(torch.isnan(res[k]), torch.isnan(ref[k])), (what, k)
        assert torch.equal(torch.nan_to_num(res[k], nan=-7.0), torch.nan_to_num(ref[k], nan=-7.0)), (what, k)


@pytest.mark.parametrize("N,K", [(641, 32), (961, 2), (1280, 32)])
def test_search_equals_the_single_hrf_four_wave_search_row_by_row(solver, N, K):
    """pb_auto_lbda_split_pp_d (taps and traces in padded buffers) against pb_auto_lbda_split_d on each row, 10 outer x 50
    inner iterations, early stopping on (the inner window rule fires at tol = 1e-2) and off: every output bit for bit;
    outer_chunk = 1 changes no bit."""
    from pybold_amd import utils
    Y, H, steps, _ = problems(N, K)
    sigma = utils.mad_daub_noise_est(Y) * np.array([0.5, 1.0, 2.0])
    Yb, Yv = padded(Y, 5)
    Tb, Tv = padded(H, 3)
    for es in (True, False):
        kw = dict(early_stopping=es, tol=TOL, nb_iter=10, nb_sub_iter=50)
        W, res = solver.auto_lbda_solve_split_pp(Yv, Tv, steps, sigma, **kw)
        torch.cuda.synchronize()
        assert torch.isnan(Yb[:, N:]).all() and torch.isnan(Tb[:, K:]).all()
        print((N, K, es), "n_outer", res["n_outer"].tolist(), "n_inner", res["n_inner"].tolist(), "lbda", res["lbda"].tolist())
        if not es:
            assert (res["n_outer"] == 10).all() and (res["n_inner"] == 11 * 50).all()
        for v in range(V3):
            W1, res1 = solver.auto_lbda_solve_split(Yv[v:v + 1], H[v], float(steps[v]), sigma[v:v + 1], **kw)
            assert torch.equal(W1[0], W[v]), (N, K, es, v, float((W1[0] - W[v]).abs().max()))
            _same(res1, {k: t[v:v + 1] for k, t in res.items()}, (N, K, es, v))
        Wc, resc = solver.auto_lbda_solve_split_pp(Yv, Tv, steps, sigma, outer_chunk=1, **kw)
        assert torch.equal(Wc, W)
        _same(resc, res, (N, K, es, "outer_chunk=1"))


# ---- 3. deconv with a 2-D hrf, fixed lambda, on the reference's 1 200-scan fixture ---------------------------------------
def _second_hrf(hrf):
    """A different HRF of the same length (h[0] = 0): the reference's, delayed by one sample and rescaled."""
    other = np.zeros_like(hrf)
    other[1:] = 0.8 * hrf[:-1]
    return other


def test_deconv_fixed_lambda_against_the_reference(golden, monkeypatch):
    import pybold_amd
    from pybold_amd import bold_signal
    g = golden("long_series")
    y, hrf, t_r = g["hcp_y"], g["hcp_hrf"], float(g["hcp_t_r"])
    Y = np.stack([y, 0.7 * y[::-1]])
    Hh = np.stack([hrf, _second_hrf(hrf)])
    calls = []
    real = bold_signal.solver.fista_solve_pp_d
    monkeypatch.setattr(bold_signal.solver, "fista_solve_pp_d", lambda *a, **k: (calls.append(k.get("force")), real(*a, **k))[1])
    monkeypatch.setattr(bold_signal, "PER_VOXEL_SPLIT", True)
    for lbda in (0.5, 2.0):
        for nb_iter, es in ((100, False), (400, True)):
            tag = "hcp_l%g_n%d%s" % (lbda, nb_iter, "_es" if es else "")
            np.random.seed(0)          # row 0 of the randn(2, N) draw is the draw of the reference's call
            x, z, dz, J, _, _ = pybold_amd.deconv(Y, t_r, Hh, lbda=lbda, nb_iter=nb_iter, early_stopping=es, tol=1.0e-2, wind=6)
            assert calls[-1] == "split"
            n = int(np.sum(~np.isnan(J[0])))
            assert n == len(g["J_" + tag]), (tag, n, len(g["J_" + tag]))
            assert (not es) or n < nb_iter
            for got, key in ((x, "x_"), (z, "z_"), (dz, "dz_")):
                e = rel(got[0], g[key + tag])
                print(tag, key, "%.2e" % e)
                assert e <= 1e-10, (tag, key, e)
            np.testing.assert_allclose(J[0, :n], g["J_" + tag], rtol=1e-9)


# ---- 4. lambda search on the reference's fixtures -------------------------------------------------------------------------
def _step_of(hrf, n):
    from pybold_amd.linear import ConvAndLinear, DiscretInteg
    from pybold_amd.utils import spectral_radius_est
    np.random.seed(0)                     # the draw of the reference's 1-D call
    return 1.0 / (0.9 * spectral_radius_est(ConvAndLinear(DiscretInteg(), hrf, dim_in=n, dim_out=n), (n,)))


@pytest.mark.parametrize("case", ["n700", "hcp"])
def test_search_against_the_reference_runs(solver, golden, monkeypatch, case):
    """The nine runs of a case of auto_lbda_long.npz, the three sigma of a budget as the rows of one call with the HRF
    tiled and every step the 1-D step: n_outer equal to the reference's, diff_z, J, R, G within 1e-6; within 1e-9 of the
    host engine on the same per-voxel taps and steps."""
    import pybold_amd
    from pybold_amd import bold_signal
    g = golden("auto_lbda_long")
    y, hrf, sig = g[case + "_y"], g[case + "_hrf"], g[case + "_sigma"]
    n = len(y)
    Y = np.repeat(y[None, :], 3, axis=0)
    Hh = np.repeat(hrf[None, :], 3, axis=0)
    steps = np.full(3, _step_of(hrf, n))
    monkeypatch.setattr(bold_signal, "_pv_steps", lambda T, n_: steps.copy())
    Yd, Td = torch.from_numpy(Y).cuda(), torch.from_numpy(Hh).cuda()
    for o, i, tol in ((20, 50, 1e-6), (60, 300, 1e-2), (60, 300, 1e-3)):
        tags = ["%s_s%d_o%d_i%d_t%g" % (case, s, o, i, tol) for s in range(3)]
        kw = dict(nb_iter=o, nb_sub_iter=i, early_stopping=True, tol=tol, wind=6)
        W, res = solver.auto_lbda_solve_split_pp(Yd, Td, steps, sig.copy(), **kw)
        W = W.cpu().numpy()
        n_outer = res["n_outer"].cpu().numpy()
        J, R, G = (res[k].cpu().numpy() for k in ("J", "R", "G"))
        host = pybold_amd.deconv_auto(Y, 1.0, Hh, sigma=sig.copy(), engine="host", **kw)
        assert host[6]["engine"] == "host"
        for s, tag in enumerate(tags):
            m = len(g["J_" + tag])
            assert int(n_outer[s]) == m, (tag, int(n_outer[s]), m)
            errs = [rel(W[s], g["dz_" + tag]), rel(J[s, :m], g["J_" + tag]), rel(R[s, :m], g["R_" + tag]), rel(G[s, :m], g["G_" + tag])]
            assert np.isnan(J[s, m:]).all()
            assert int(host[6]["n_outer"][s]) == m
            errs_h = [rel(W[s], host[2][s]), rel(J[s, :m], host[3][:m, s]), rel(R[s, :m], host[4][:m, s]), rel(G[s, :m], host[5][:m, s])]
            print(tag, "n_outer %d" % m, "reference", ["%.1e" % e for e in errs], "host engine", ["%.1e" % e for e in errs_h])
            assert max(errs) <= 1e-6, (tag, errs)
            assert max(errs_h) < 1e-9, (tag, errs_h)


# ---- 5. switches --------------------------------------------------------------------------------------------------------
def test_the_engine_and_the_switches(solver, golden, monkeypatch):
    import pybold_amd
    from pybold_amd import bold_signal
    g = golden("auto_lbda_long")
    y, hrf, sig = g["n700_y"], g["n700_hrf"], g["n700_sigma"]
    Y = np.repeat(y[None, :], 3, axis=0) * np.array([1.0, 1.5, 2.0])[:, None]
    Hh = np.stack([hrf, _second_hrf(hrf), 1.1 * hrf])
    kw = dict(nb_iter=8, nb_sub_iter=20)
    # deconv_auto(engine="device_split_pp") is the solver call on the steps deconv draws
    np.random.seed(0)
    steps = bold_signal._pv_steps(torch.from_numpy(Hh).cuda(), 700)
    W, res = solver.auto_lbda_solve_split_pp(torch.from_numpy(Y).cuda(), torch.from_numpy(Hh).cuda(), steps, sig, **kw)
    np.random.seed(0)
    out = pybold_amd.deconv_auto(Y, 1.0, Hh, sigma=sig, engine="device_split_pp", **kw)
    assert out[6]["engine"] == "device_split_pp"
    assert np.array_equal(out[2], W.cpu().numpy()) and np.array_equal(out[6]["n_outer"], res["n_outer"].cpu().numpy())
    assert np.array_equal(out[3], res["J"][:, :int(res["n_outer"].max())].t().cpu().numpy(), equal_nan=True)
    assert np.array_equal(out[6]["lbda"], res["lbda"].cpu().numpy()) and np.array_equal(out[6]["n_inner"], res["n_inner"].cpu().numpy())
    with pytest.raises(ValueError, match="device_split.*one HRF"):
        pybold_amd.deconv_auto(Y, 1.0, Hh, sigma=sig, engine="device_split", **kw)
    # AUTO_LBDA = "device_split_pp" reaches it from deconv(lbda=None); "device_split" keeps the host loop for a 2-D hrf
    monkeypatch.setattr(bold_signal, "mad_daub_noise_est", lambda x: sig)
    calls = []
    real = bold_signal.solver.auto_lbda_solve_split_pp
    monkeypatch.setattr(bold_signal.solver, "auto_lbda_solve_split_pp", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(bold_signal, "AUTO_LBDA", "device_split_pp")
    np.random.seed(0)
    got = pybold_amd.deconv(Y, 1.0, Hh, lbda=None, **kw)
    assert len(calls) == 1 and len(got) == 6
    for a, b in zip(got, out[:6]):
        assert np.array_equal(a, b, equal_nan=True)
    monkeypatch.setattr(bold_signal, "AUTO_LBDA", "device_split")
    np.random.seed(0)
    host = pybold_amd.deconv(Y, 1.0, Hh, lbda=None, **kw)
    assert len(calls) == 1 and rel(host[2], got[2]) < 1e-9
    # a single HRF under "device_split_pp": everything "device_split" does
    monkeypatch.setattr(bold_signal, "AUTO_LBDA", "device_split_pp")
    np.random.seed(0)
    one = pybold_amd.deconv(Y, 1.0, hrf, lbda=None, **kw)
    np.random.seed(0)
    want = pybold_amd.deconv_auto(Y, 1.0, hrf, sigma=sig, engine="device_split", **kw)
    assert len(calls) == 1
    for a, b in zip(one, want[:6]):
        assert np.array_equal(a, b, equal_nan=True)
    # PER_VOXEL_SPLIT off (the default): deconv on a 2-D hrf at 700 scans is the call without a forced form, bit for bit
    monkeypatch.setattr(bold_signal, "AUTO_LBDA", "host")
    forces = []
    real_solve = bold_signal.solver.fista_solve_pp_d
    monkeypatch.setattr(bold_signal.solver, "fista_solve_pp_d", lambda *a, **k: (forces.append(k.get("force")), real_solve(*a, **k))[1])
    monkeypatch.setattr(bold_signal, "PER_VOXEL_SPLIT", False)
    np.random.seed(0)
    off = pybold_amd.deconv(Y, 1.0, Hh, lbda=0.5, nb_iter=60, early_stopping=False)
    assert forces == [None]
    Wn, Jn, ndn = real_solve(torch.from_numpy(Y).cuda(), torch.from_numpy(Hh).cuda(), steps, 0.5, 60, want_J=True, force=None)
    Wg, _, ndg = real_solve(torch.from_numpy(Y).cuda(), torch.from_numpy(Hh).cuda(), steps, 0.5, 60, want_J=True, force="generic")
    assert np.array_equal(off[2], Wn.cpu().numpy()) and torch.equal(Wn, Wg) and torch.equal(ndn, ndg)
    # ... and on: the four-wave form, in the fixed-lambda call and in the inner solves of the host-loop search
    monkeypatch.setattr(bold_signal, "PER_VOXEL_SPLIT", True)
    np.random.seed(0)
    on = pybold_amd.deconv(Y, 1.0, Hh, lbda=0.5, nb_iter=60, early_stopping=False)
    assert forces[-1] == "split" and rel(on[2], off[2]) < 1e-9
    np.random.seed(0)
    host_on = pybold_amd.deconv(Y, 1.0, Hh, lbda=None, **kw)
    assert set(forces[2:]) == {"split"} and len(forces) >= 2 + 2
    assert rel(host_on[2], got[2]) < 1e-9
    # shapes the four-wave form does not carry keep their kernel with the switch on
    np.random.seed(0)
    pybold_amd.deconv(Y[:, :300].copy(), 1.0, Hh, lbda=0.5, nb_iter=20, early_stopping=False)
    assert forces[-1] is None
