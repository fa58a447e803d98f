"""`deconv` with one HRF per voxel on the GPU: the batched power iteration, `fista_exact_pp_kernel` and the LDS fallback
behind `pb_fista_solve_pp_d`, `auto_lbda_pp_kernel` behind `pb_auto_lbda_pp_d`, and the API calls on the fixture of the
REAL reference (tests/golden/make_golden_pv.py: six voxels, six HRFs, six consecutive reference calls per run).

Bounds.
  * Row v of a per-voxel call against the single-HRF call of that row: BIT FOR BIT (`W`, `J`, `n_done`, `rho`).  Both
    kernels run the same pass body (csrc/fista_exact.h: exact_forward / exact_backward) on the same inputs; only the
    place the taps are read from differs.
  * `deconv` against the reference: 1e-10 relative on x, z, diff_z and J (tests/test_gpu_exact_split.py::
    test_one_dimensional_deconv_against_the_reference holds the 1-D call to it).
  * `lbda=None` against the reference: 1e-7 (tests/test_gpu_round5.py / test_gpu_auto_lbda_device.py for this branch);
    device engine against host engine: 1e-9 with equal n_outer (tests/test_gpu_auto_lbda_device.py).
  * The six step constants against the fixture: 1e-10 relative (tests/test_gpu_parity.py::
    test_spectral_radius_matches_golden holds `spectral_radius_est` to it against a fixture's `lipschitz`).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
STOPS = (None, "loops", "window")
V7 = 7                                        # two workgroups of four waves, the last wave of the second one idle


@pytest.fixture(scope="module")
def solver():
    from pybold_amd import solver as s
    return s


@pytest.fixture(scope="module")
def pv(golden):
    return golden("per_voxel_hrf")


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - b) / (np.linalg.norm(b) + 1e-300)


def taps_for(V, K):
    """V different causal bumps of K taps with h[0] = 0 (as every HRF of the reference): shape and amplitude vary by row."""
    t = np.arange(K, dtype=np.float64)
    H = np.stack([t ** (1.0 + 0.3 * v) * np.exp(-t / (0.8 + 0.25 * v)) for v in range(V)])
    return H / H.sum(axis=1, keepdims=True) * (0.8 + 0.1 * np.arange(V))[:, None]


_cache = {}


def problems(V, N, K):
    """Block signals (random on/off blocks convolved with the row's HRF, unit-variance noise), one HRF and one step
    1 / (0.9 rho) per row, a warm start: host float64 arrays."""
    key = (V, N, K)
    if key not in _cache:
        from oracle import pybold_oracle as orc
        rng = np.random.RandomState(1000 * N + K)
        H = taps_for(V, K)
        Y = np.empty((V, N))
        for v in range(V):
            z = np.repeat(rng.randint(0, 2, size=N // 6 + 1).astype(np.float64), 6)[:N] * (2.0 + v)
            Y[v] = np.convolve(z, H[v])[:N] + 0.3 * rng.randn(N)
        steps = np.array([1.0 / (0.9 * orc.spectral_radius_est(orc._MatrixFreeH(H[v]), rng.randn(N))) for v in range(V)])
        W0 = 0.05 * rng.randn(V, N)
        _cache[key] = (Y, H, steps, W0)
    return _cache[key]


def padded(a, pad, dtype=torch.float64):
    """(buffer, view): the rows of `a` in a CUDA buffer whose rows are `pad` elements longer, the guard band NaN."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), NAN, dtype=dtype, device="cuda")
    buf[:, :a.shape[1]] = torch.as_tensor(a, dtype=dtype)
    return buf, buf[:, :a.shape[1]]


def solve_padded(solver, Y, H, steps, lbda, n_iter, W0, want_J, stop, tol, wind, force=None):
    """pb_fista_solve_pp_d on buffers whose leading dimensions ldy, ldw, ldt, ldj are all padded, the guard bands (the
    tap slots K .. ldt-1 included) NaN; asserts that the guard bands come back untouched.  -> (W, J, n_done) on the host."""
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
    flags = solver._FORCE[force] | (_lib.PB_FLAG_COLD_START if W0 is None else 0)
    rc = lib.pb_fista_solve_pp_d(Yv.data_ptr(), Yb.stride(0), 1, Wv.data_ptr(), Wb.stride(0), V, N, Tv.data_ptr(), Tb.stride(0),
                                 H.shape[1], st.data_ptr(), 0.0, lb.data_ptr(), betas.data_ptr(), n_iter,
                                 Jb.data_ptr() if want_J else None, Jb.stride(0) if want_J else 0, solver._STOP[stop], tol, wind,
                                 n_done.data_ptr(), flags, solver._stream_ptr(Yb.device))
    _lib.check(rc, "pb_fista_solve_pp_d")
    torch.cuda.synchronize()
    assert torch.isnan(Wb[:, N:]).all() and torch.isnan(Jb[:, n_iter:]).all(), "guard band written"
    assert torch.isnan(Yb[:, N:]).all() and torch.isnan(Tb[:, H.shape[1]:]).all()
    assert torch.equal(Yv, torch.as_tensor(Y).cuda()) and torch.equal(Tv, torch.as_tensor(H).cuda())
    return Wv.cpu().numpy(), (Jb[:, :n_iter].cpu().numpy() if want_J else None), n_done.cpu().numpy()


def solve_rows(solver, Y, H, steps, lbda, n_iter, W0, want_J, stop, tol, wind, force=None):
    """The same problems one by one through the single-HRF entry point (pb_fista_solve_d: taps by value)."""
    Yd = torch.as_tensor(Y).cuda()
    W0d = torch.as_tensor(W0).cuda() if W0 is not None else None
    lb = np.broadcast_to(lbda, (Y.shape[0],))
    Ws, Js, nd = [], [], []
    for v in range(Y.shape[0]):
        W, J, n = solver.fista_solve(Yd[v:v + 1], H[v], float(lb[v]), float(steps[v]), n_iter,
                                     W0=None if W0d is None else W0d[v:v + 1], want_J=want_J, stop=stop, tol=tol, wind=wind, force=force)
        Ws.append(W.cpu().numpy()[0])
        Js.append(J.cpu().numpy()[0] if want_J else None)
        nd.append(int(n[0]))
    return np.stack(Ws), (np.stack(Js) if want_J else None), np.array(nd)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_against_rows(solver, N, K, wind, force_rows, kernel_code, stops=STOPS):
    """Every (stop rule, cost trace, start) of a shape: the padded per-voxel call against single-row calls, bit for bit.
    -> {stop rule: the values of n_done below the iteration count}."""
    from pybold_amd import _lib
    Y, H, steps, W0 = problems(V7, N, K)
    varied = {}
    for stop in stops:
        assert _lib.load().pb_fista_which_kernel_pp_d(N, K, 1, solver._STOP[stop], wind) == kernel_code
        n_iter, tol = (300, 1.0e-2) if stop else (40, 0.0)
        # (the _loops_deconv criterion is the size of the prox step against the iterate's, i.e. proportional to lambda: at
        # the lambdas of the other cases it is below 1e-2 at its first test on every series of 180 scans or more)
        lbda = (0.2 + 0.1 * np.arange(V7)) * ((1 if N < 100 else 10 if N < 640 else 30) if stop == "loops" else 1)
        for want_J in (True, False):
            for warm in (False, True):
                args = (Y, H, steps, lbda, n_iter, W0 if warm else None, want_J, stop, tol, wind)
                W, J, nd = solve_padded(solver, *args)
                Wr, Jr, ndr = solve_rows(solver, *args, force=force_rows)
                what = (N, K, stop, want_J, warm)
                print(what, "n_done", nd.tolist(), "max |W - W_row|", float(np.abs(W - Wr).max()))
                assert np.array_equal(nd, ndr), (what, nd, ndr)
                assert same_bits(W, Wr), (what, float(np.abs(W - Wr).max()))
                if want_J:
                    assert same_bits(J, Jr), what                  # (NaN beyond a row's n_done in both)
                    for v in range(V7):
                        assert not np.isnan(J[v, :nd[v]]).any() and np.isnan(J[v, nd[v]:]).all(), what
                if stop:
                    varied[stop] = varied.get(stop, set()) | set(int(n) for n in nd if n < n_iter)
    return varied


# ---- 1. power iteration -----------------------------------------------------------------------------------------------
def test_batched_power_iteration_equals_single_launches(solver, pv):
    V, N, K = 7, 180, 30
    rng = np.random.RandomState(5)
    H = taps_for(V, K)
    H[:6] = pv["hrf"]
    Xb, Xv = padded(rng.randn(V, N), 5)
    Tb, Tv = padded(H, 3)
    rho, n_it = solver.spectral_radius_batch(Xv, Tv)
    assert rho.shape == (V,) and n_it.shape == (V,)
    assert torch.isnan(Xb[:, N:]).all() and torch.isnan(Tb[:, K:]).all()
    x_host = Xv.cpu().numpy()
    for v in range(V):
        r1, n1 = solver.spectral_radius(x_host[v], H[v])
        assert np.float64(r1).view(np.uint64) == rho[v:v + 1].view(np.uint64)[0] and n1 == n_it[v], (v, r1, rho[v], n1, n_it[v])
    # the fixture's six constants, from the start vectors the six reference calls drew
    rho6, _ = solver.spectral_radius_batch(pv["x0"], pv["hrf"])
    err = np.abs(0.9 * rho6 - pv["lipschitz"]) / pv["lipschitz"]
    print("0.9 rho against the fixture:", err)
    assert (err <= 1e-10).all(), err


# ---- 2. solver, register form -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(23, 3), (180, 30), (320, 32), (321, 17), (640, 32)])
def test_register_form_equals_the_single_hrf_kernel_row_by_row(solver, N, K):
    """Both S (5 up to 320 scans, 10 beyond), a partial last lane, a halo of 1 to 7 neighbour lanes, full width; seven
    rows (a workgroup with one idle wave), a different HRF, step and lambda per row, every leading dimension padded."""
    assert "fista_exact_pp_kernel" in solver.which_kernel_pp_f64(N, K, want_J=True, stop="window")
    assert solver.which_kernel_f64(N, K, want_J=True, stop="window") == solver.KERNEL_NAMES[7]
    varied = check_against_rows(solver, N, K, 6, None, 9)
    for stop in ("loops", "window"):          # waves leave at different times
        assert len(varied[stop]) >= 2, (N, K, stop, varied)
    # the Python entry point is that call (contiguous buffers of its own)
    Y, H, steps, W0 = problems(V7, N, K)
    lbda = 0.2 + 0.1 * np.arange(V7)
    W, J, nd = solver.fista_solve_pp_d(torch.as_tensor(Y).cuda(), torch.as_tensor(H).cuda(), steps, lbda, 300, W0=torch.as_tensor(W0).cuda(),
                                       want_J=True, stop="window", tol=1.0e-2, force="fast")
    Wp, Jp, ndp = solve_padded(solver, Y, H, steps, lbda, 300, W0, True, "window", 1.0e-2, 6)
    assert same_bits(W.cpu().numpy(), Wp) and same_bits(J.cpu().numpy(), Jp) and np.array_equal(nd.cpu().numpy(), ndp)


def test_register_form_scalar_and_negative_lambda(solver):
    """A scalar lambda for all rows, and a negative one (the reference's prox, as pb_fista_solve_d): row by row as above."""
    Y, H, steps, W0 = problems(V7, 180, 30)
    Yd, Hd = torch.as_tensor(Y).cuda(), torch.as_tensor(H).cuda()
    for lbda in (0.7, -0.3):
        W, _, nd = solver.fista_solve_pp_d(Yd, Hd, steps, lbda, 60)
        Wr, _, ndr = solve_rows(solver, Y, H, steps, lbda, 60, None, False, None, 0.0, 6)
        assert same_bits(W.cpu().numpy(), Wr) and np.array_equal(nd.cpu().numpy(), ndr), lbda


# ---- 3. solver, LDS fallback ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,wind", [(700, 30, 6), (300, 40, 6), (300, 30, 4)])
def test_lds_fallback_equals_the_single_hrf_lds_kernel_row_by_row(solver, N, K, wind):
    # (wind = 4: only the window rule leaves the register form, whose other rules do not read wind)
    stops = STOPS if wind == 6 else ("window",)
    varied = check_against_rows(solver, N, K, wind, "generic", 0, stops)
    for stop in stops[1:] if wind == 6 else stops:
        assert len(varied[stop]) >= 2, (N, K, stop, varied)
    Y, H, steps, _ = problems(V7, N, K)
    with pytest.raises(Exception, match="no register-resident"):
        solver.fista_solve_pp_d(torch.as_tensor(Y).cuda(), torch.as_tensor(H).cuda(), steps, 1.0, 10, stop="window", wind=wind, force="fast")


# ---- 4. deconv with a 2-D hrf, fixed lambda ---------------------------------------------------------------------------
@pytest.mark.parametrize("run", ["a", "b", "c"])
def test_deconv_fixed_lambda_against_the_reference(pv, run):
    import pybold_amd
    lbda, nb_iter, es, tol, wind = pv[run + "_kw"]
    kw = dict(lbda=float(lbda), nb_iter=int(nb_iter), early_stopping=bool(es), tol=float(tol), wind=int(wind))
    y, hrf = pv["y"], pv["hrf"]
    np.random.seed(0)
    x, z, dz, J, _, _ = pybold_amd.deconv(y, 1.0, hrf, **kw)
    n_ref = pv[run + "_n"]
    assert J.shape == (6, int(n_ref.max()))
    got_n = np.array([int(np.sum(~np.isnan(J[v]))) for v in range(6)])
    print("run", run, "trace lengths", got_n.tolist(), "reference", n_ref.tolist())
    assert np.array_equal(got_n, n_ref)
    np.random.seed(0)
    for v in range(6):                        # the same six calls, one by one, under the same seed
        n = int(n_ref[v])
        assert np.isnan(J[v, n:]).all()
        errs = [rel(x[v], pv[run + "_x"][v]), rel(z[v], pv[run + "_z"][v]), rel(dz[v], pv[run + "_dz"][v]), rel(J[v, :n], pv[run + "_J"][v, :n])]
        x1, z1, dz1, J1, _, _ = pybold_amd.deconv(y[v], 1.0, hrf[v], **kw)
        assert len(J1) == n
        errs1 = [rel(x[v], x1), rel(z[v], z1), rel(dz[v], dz1), rel(J[v, :n], J1)]
        print("run %s voxel %d: against the reference %.2e, against the 1-D call %.2e" % (run, v, max(errs), max(errs1)))
        assert max(errs) <= 1e-10, (run, v, errs)
        assert max(errs1) <= 1e-10, (run, v, errs1)
    # lbda as a (V,) array: the same call
    np.random.seed(0)
    xa, _, dza, Ja, _, _ = pybold_amd.deconv(y, 1.0, hrf, **dict(kw, lbda=np.full(6, kw["lbda"])))
    assert np.array_equal(dza, dz) and np.array_equal(xa, x) and np.array_equal(np.isnan(Ja), np.isnan(J))


# ---- 5. lbda = None ---------------------------------------------------------------------------------------------------
def _auto(pv, run, engine, **extra):
    import pybold_amd
    nb_iter, nb_sub_iter, es, tol, wind = pv[run + "_kw"]
    np.random.seed(0)
    return pybold_amd.deconv_auto(pv["y"], 1.0, pv["hrf"], sigma=pv["sigma"], nb_iter=int(nb_iter), nb_sub_iter=int(nb_sub_iter),
                                  early_stopping=bool(es), tol=float(tol), wind=int(wind), engine=engine, **extra)


@pytest.mark.parametrize("run", ["d", "e"])
def test_lambda_search_against_the_reference(pv, run):
    n_ref = pv[run + "_n"]
    out = {}
    for engine in ("host", "device"):
        x, z, dz, J, R, G, info = out[engine] = _auto(pv, run, engine)
        assert info["engine"] == engine
        assert np.array_equal(info["n_outer"], n_ref), (engine, info["n_outer"], n_ref)
        assert J.shape == R.shape == G.shape == (int(n_ref.max()), 6)
        for v in range(6):
            n = int(n_ref[v])
            for T in (J, R, G):
                assert np.isnan(T[n:, v]).all() and not np.isnan(T[:n, v]).any()
            errs = [rel(J[:n, v], pv[run + "_J"][v, :n]), rel(R[:n, v], pv[run + "_R"][v, :n]), rel(G[:n, v], pv[run + "_G"][v, :n]),
                    rel(dz[v], pv[run + "_dz"][v]), rel(z[v], pv[run + "_z"][v]), rel(x[v], pv[run + "_x"][v])]
            print("run %s %-6s voxel %d: n_outer %2d, worst rel. error %.2e" % (run, engine, v, n, max(errs)))
            assert max(errs) < 1e-7, (run, engine, v, errs)
    h, d = out["host"], out["device"]
    assert np.array_equal(h[6]["n_outer"], d[6]["n_outer"])
    for v in range(6):
        n = int(n_ref[v])
        errs = [rel(d[k][:n, v], h[k][:n, v]) for k in (3, 4, 5)] + [rel(d[k][v], h[k][v]) for k in (0, 1, 2)]
        assert max(errs) < 1e-9, (run, v, errs)
    assert rel(d[6]["alpha"], h[6]["alpha"]) < 1e-9 and rel(d[6]["lbda"], h[6]["lbda"]) < 1e-9
    # chunking changes no bit
    c = _auto(pv, run, "device", outer_chunk=1)
    for k in range(6):
        assert np.array_equal(c[k], d[k], equal_nan=True), k
    for k in ("alpha", "lbda", "n_outer", "n_inner"):
        assert np.array_equal(c[6][k], d[6][k]), k


def test_lambda_search_switch_and_limits(pv, monkeypatch):
    """`deconv(lbda=None)` with a 2-D hrf honours PYBOLD_AMD_AUTO_LBDA's module switch; shapes the device-resident search
    does not carry are refused by engine='device' before any launch."""
    import pybold_amd
    from pybold_amd import bold_signal
    monkeypatch.setattr(bold_signal, "mad_daub_noise_est", lambda x: pv["sigma"])
    outs = {}
    for mode in ("host", "device"):
        monkeypatch.setattr(bold_signal, "AUTO_LBDA", mode)
        np.random.seed(0)
        outs[mode] = pybold_amd.deconv(pv["y"], 1.0, pv["hrf"], lbda=None, nb_iter=5, nb_sub_iter=50, early_stopping=False)
    for v in range(6):
        assert rel(outs["host"][2][v], pv["e_dz"][v]) < 1e-7 and rel(outs["device"][2][v], pv["e_dz"][v]) < 1e-7
    assert rel(outs["device"][3], outs["host"][3]) < 1e-9
    with pytest.raises(ValueError, match="640 scans"):
        pybold_amd.deconv_auto(np.zeros((2, 700)), 1.0, np.ones((2, 30)), sigma=1.0, engine="device")


# ---- 6. CUDA in -> CUDA out; a 1-D hrf is untouched --------------------------------------------------------------------
def test_cuda_in_cuda_out_and_the_single_hrf_call_is_unchanged(pv):
    import pybold_amd
    y, hrf = pv["y"], pv["hrf"]

    def single():
        np.random.seed(0)
        return pybold_amd.deconv(y, 1.0, hrf[2], lbda=0.5, nb_iter=60, early_stopping=False)
    before = single()
    np.random.seed(0)
    host = pybold_amd.deconv(y, 1.0, hrf, lbda=0.5, nb_iter=60, early_stopping=False)
    yd, hd = torch.from_numpy(y).cuda(), torch.from_numpy(hrf).cuda()
    np.random.seed(0)
    dev = pybold_amd.deconv(yd, 1.0, hd, lbda=0.5, nb_iter=60, early_stopping=False)
    for k in range(4):
        assert torch.is_tensor(dev[k]) and dev[k].is_cuda and dev[k].dtype == torch.float64
        assert np.array_equal(dev[k].cpu().numpy(), host[k], equal_nan=True), k
    np.random.seed(0)
    a_host = pybold_amd.deconv_auto(y, 1.0, hrf, sigma=pv["sigma"], nb_iter=5, nb_sub_iter=50, early_stopping=False, engine="device")
    np.random.seed(0)
    a_dev = pybold_amd.deconv_auto(yd, 1.0, hd, sigma=torch.from_numpy(pv["sigma"]).cuda(), nb_iter=5, nb_sub_iter=50,
                                   early_stopping=False, engine="device")
    for k in range(3):
        assert a_dev[k].is_cuda and np.array_equal(a_dev[k].cpu().numpy(), a_host[k]), k
    for k in range(3, 6):
        assert np.array_equal(np.asarray(a_dev[k]), a_host[k], equal_nan=True), k
    after = single()
    for k in range(4):
        assert np.array_equal(before[k], after[k], equal_nan=True), k
