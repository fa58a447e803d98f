"""Padded leading dimensions and guard bands on every solver form (include/pybold_hip.h, "Conventions": row-major
matrices with a leading dimension in elements, no alignment beyond the element's own).

Every case runs the same call twice -- on FRAMED buffers (tests/frames.py: pad columns on both sides of every row, an
unaligned and alternating row start for y, guard rows, guard elements around every vector, all holding a NaN / integer
sentinel) and on PACKED copies of the same data -- and asserts
  (a) W, J, the traces, n_done and the scalar outputs are BIT-equal between the two calls;
  (b) every output frame is untouched outside its window (W, J, traces, n_done, alpha / lbda / n_outer / n_inner, z / x,
      the guard behind the workspace);
  (c) every input frame is untouched as a whole (y, lbda, betas, taps_pp, step_vec, sigma, lmax);
  (d) the framed result equals the float64 oracle row by row, at the project's bounds: 1e-5 relative L2 for the float32
      forms (EPS of the GPU tests), 1e-11 for the float64 forms (BOUND of tests/test_gpu_exact_split.py), rtol 3e-5 on a
      float32 cost trace (tests/test_gpu_mfma.py) and 1e-11 on a float64 one (tests/test_gpu_round2.py), 1e-9 for the
      lambda search (tests/test_gpu_auto_lbda_device.py);
  (e) the intended kernel did the work: for the forms whose guards hand problems back, one more framed call with the
      no-re-solve variant of the flag -- at most 2 % of the rows come back (n_done = -1), those hold their warm start bit
      for bit, all others meet (d).
Every problem has its own series, its own lambda, its own warm start (0.01 randn) and, where the form takes it,
y_rep = 3: a misplaced row is an O(1) error.  The stop rules run with a tolerance they cannot meet in 40 iterations, so
every problem runs them all and the oracle of the plain recurrence applies (the rules' own tests are elsewhere)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import frames
from oracle import c_oracle
from oracle import pybold_oracle as orc

pytestmark = pytest.mark.gpu

EPS, BOUND, AUTO_BOUND = 1.0e-5, 1.0e-11, 1.0e-9
J_RTOL, J64_RTOL = 3.0e-5, 1.0e-11
NI, ROWS, Y_REP = 40, 37, 3
HANDED_BACK = 0.02
TOL = {None: 0.0, "window": 1.0e-6, "loops": 1.0e-9}       # never met in 40 iterations (window: ~0.9 / k)
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64

_worst = {}


def note(group, err):
    _worst[group] = max(_worst.get(group, 0.0), float(err))
    print("%s: worst error against the oracle so far %.2e (this case %.2e)" % (group, _worst[group], err))


@pytest.fixture(scope="module")
def solver():
    from pybold_amd import solver as s
    assert torch.cuda.is_available()
    return s


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def rel_rows(a, b):
    return np.linalg.norm(a - b, axis=1) / (np.linalg.norm(b, axis=1) + 1e-300)


def bits(t):
    return t.contiguous().view(frames._INT_VIEW[t.dtype])


_hrf, _lip = {}, {}


def hrf_for(K):
    """The HRFs of tests/test_gpu_mfma.py: SPM at TR 1 s cut to K taps; 34+ taps: a short TR."""
    if K not in _hrf:
        h = orc.spm_hrf(1.0, 1.0, float(K), False)[0][:K] if K <= 33 else orc.spm_hrf(1.0, 30.0 / K, 30.0, False)[0][:K]
        assert len(h) == K
        _hrf[K] = np.ascontiguousarray(h)
    return _hrf[K]


def step_for(N, K):
    if (N, K) not in _lip:
        _lip[(N, K)] = orc.gram_lipschitz(hrf_for(K), N)
    return 1.0 / _lip[(N, K)]


def block_rows(V, N, K, seed):
    """Block signals at SNR 1 dB from the package's generator (tests/test_gpu_exact_split.py), float32 CUDA (V, N)."""
    from pybold_amd import data
    Y = data.gen_rnd_bloc_bold_batch(V, dur=(N + 0.5) / 60.0, tr=1.0, hrf=hrf_for(K), nb_events=5, avg_dur=12.0, std_dur=1.0,
                                     snr=1.0, seed=seed)[0]
    return Y[:, :N].contiguous()


# ---- one problem set per (shape, data kind): series, lambdas, warm starts and the oracle, computed once ----------------
_problems = {}


def problem(N, K, kind, P=ROWS, y_rep=Y_REP):
    key = (N, K, kind, P, y_rep)
    if key in _problems:
        return _problems[key]
    rng = np.random.RandomState(1000 * N + 10 * K + len(kind))
    V = (P + y_rep - 1) // y_rep
    pr = SimpleNamespace(N=N, K=K, P=P, V=V, y_rep=y_rep, hrf=hrf_for(K), step=step_for(N, K), f64=kind == "block64")
    if kind == "randn":            # float32 forms: randn rows, lambda in {0.05, 0.3, 1.0} x a scale of the problem's own
        pr.Y = rng.randn(V, N).astype(np.float32)
        pr.lam = np.tile([0.05, 0.3, 1.0], P)[:P] * rng.uniform(0.8, 1.25, P)
    else:                          # float64 forms: block signals, lambdas of both signs (tests/test_gpu_exact_split.py)
        pr.Y = block_rows(V, N, K, seed=N + K).double().cpu().numpy()
        pr.lam = np.tile([0.5, -0.7, 2.0], P)[:P] * rng.uniform(0.5, 1.5, P)
    pr.W0 = 0.01 * rng.randn(P, N)
    pr.Yo = np.repeat(pr.Y.astype(np.float64), y_rep, axis=0)[:P]          # the series of problem p, as the kernels read it
    pr.Wo, pr.Jo, _ = c_oracle.fista_batch(pr.Yo, pr.hrf, pr.lam, pr.step, NI, W0=pr.W0, want_J=True, threads=16)
    for a in (pr.Y, pr.lam, pr.W0, pr.Yo, pr.Wo, pr.Jo):
        a.setflags(write=False)
    _problems[key] = pr
    return pr


def run_solve(pr, packed, force=None, want_J=False, stop=None, work=False):
    """pb_fista_solve_ex (float32 y) or pb_fista_solve_d (float64 y) on framed or packed buffers."""
    from pybold_amd import _lib
    d = dev()
    r = SimpleNamespace()
    r.y = frames.frame2d("y", pr.V, pr.N, F64 if pr.f64 else F32, d, fill=pr.Y, packed=packed)
    r.w = frames.frame2d("W", pr.P, pr.N, F64, d, fill=pr.W0, packed=packed)
    r.lam = frames.frame1d("lbda", pr.P, F64, d, fill=pr.lam, packed=packed)
    r.J = frames.frame2d("J", pr.P, NI, F64 if pr.f64 else F32, d, packed=packed) if want_J else None
    r.nd = frames.frame1d("n_done", pr.P, I32, d, packed=packed)
    r.work = frames.frame1d("work", int(_lib.load().pb_fista_work_len(pr.P, pr.y_rep)), I32, d, packed=packed) if work else None
    r.outs = [f for f in (r.w, r.J, r.nd, r.work) if f is not None]
    r.ins = [r.y, r.lam]
    for f in r.outs + r.ins:
        f.snapshot()
    kw = dict(lbda_v=r.lam, J=r.J, n_done=r.nd, stop=stop, tol=TOL[stop], wind=6, y_rep=pr.y_rep, force=force)
    if pr.f64:
        r.ins.append(frames.fista_solve_d(r.y, r.w, pr.hrf, pr.step, NI, **kw))
    else:
        r.ins.append(frames.fista_solve_ex(r.y, r.w, pr.hrf, pr.step, NI, work=r.work, **kw))
    torch.cuda.synchronize()
    return r


def check_layout(fr, pk, equal=("w", "J", "nd")):
    for name in equal:                                   # (a) bit equality, NaNs and unwritten cells included
        a, b = getattr(fr, name), getattr(pk, name)
        if a is not None:
            assert torch.equal(a.window_bits(), b.window_bits()), "%s differs between the framed and the packed call" % name
    for f in fr.outs:                                    # (b)
        f.assert_outside_untouched()
    for f in fr.ins:                                     # (c)
        f.assert_untouched()


def check_oracle(pr, r, group, bound, rows=None, n_iter=NI):
    """(d) on the rows of `rows` (default: all): iterate, cost trace, n_done = n_iter."""
    rows = np.arange(pr.P) if rows is None else np.asarray(rows)
    W = r.w.contiguous().cpu().numpy()
    assert np.isfinite(W[rows]).all(), "a NaN in the iterate: a sentinel was read, or a cell of W never written"
    err = rel_rows(W[rows], pr.Wo[rows]).max() if len(rows) else 0.0
    note(group, err)
    assert err < bound, (group, err)
    nd = r.nd.contiguous().cpu().numpy()
    assert (nd[rows] == n_iter).all(), nd
    if r.J is not None and len(rows):
        J = r.J.contiguous().cpu().numpy().astype(np.float64)
        assert np.isfinite(J[rows]).all()
        np.testing.assert_allclose(J[rows], pr.Jo[rows], rtol=J64_RTOL if pr.f64 else J_RTOL)


def check_no_resolve(pr, r, group, bound, W0_bits, rows=None):
    """(e): the no-re-solve variant -- what came back is marked, few, and untouched; the rest is the intended kernel's."""
    nd = r.nd.contiguous()
    back = nd == -1
    n_back = int(back.sum())
    print("%s: %d of %d problems handed back" % (group, n_back, pr.P))
    assert n_back <= int(HANDED_BACK * pr.P), (group, n_back)
    assert torch.equal(r.w.window_bits()[back], W0_bits[back])
    for f in r.outs:
        f.assert_outside_untouched()
    for f in r.ins:
        f.assert_untouched()
    kept = np.flatnonzero(~back.cpu().numpy())
    check_oracle(pr, r, group, bound, rows=kept if rows is None else np.intersect1d(kept, rows))


# ---- the float32 forms through pb_fista_solve_ex, one form per launch ------------------------------------------------------
def _ex_cases():
    c = []
    for force, variants in (("fast1", "pJwl"), ("fast2", "pJ"), ("fast2d", "pJ"), ("wide", "pJwl"), ("generic", "pJwl"), (None, "pJwl")):
        for v in variants:
            c.append((300, 30, force, v in "Jw", {"w": "window", "l": "loops"}.get(v), None))
    c.append((300, 30, "cert2", True, "window", "certonly"))                       # pair certificate plus re-solve
    c += [(600, 30, "fast2", False, None, None), (600, 30, "fast2", True, None, None),        # split pair
          (600, 30, "cert2", True, "window", "certonly")]
    for N, K in ((300, 30), (129, 16), (300, 40)):                                      # one-wave matrix pipe
        c += [(N, K, "mfma", False, None, "mfmaonly"), (N, K, "mfma", True, None, "mfmaonly")]
        if K <= 33:                                       # (beside three near tiles the one-wave form carries no stop rule)
            c += [(N, K, "mfmacert", True, "window", "mfmacertonly"), (N, K, "mfma", False, "loops", "mfmaonly")]
    c.append((300, 30, "mfma2", False, None, "mfma2only"))                            # a short series over two waves
    for N, K in ((600, 30), (311, 30), (600, 42), (1200, 28), (641, 30)):             # two waves; four beyond 640 scans
        c += [(N, K, "mfma2", False, None, "mfma2only"), (N, K, "mfma2", False, "loops", "mfma2only")]
        # 311..320 scans: the exact form behind the certificate would be the single-row entry of 24 samples per lane, which
        # cannot hold the window rule's ring (csrc/dispatch.h: ring_fits), so route() keeps such a call off the two-wave form --
        # it runs the rule in full, one problem per wave, whatever the flag (the plan query answers otherwise for this cell).
        # The case stays as a layout check of that form; 321 scans is the shortest series that reaches the certificate.
        c.append((N, K, "mfma2cert", True, "window", "mfma2certonly" if N != 311 else None))
    c.append((321, 30, "mfma2cert", True, "window", "mfma2certonly"))
    c.append((600, 30, "mfma2", True, None, "mfma2only"))
    c.append((1200, 28, "mfma2", True, None, "mfma2only"))
    return c


def _id(case):
    N, K, force, want_J, stop, _ = case
    return "N%d-K%d-%s%s%s" % (N, K, force or "default", "-J" if want_J else "", "-" + stop if stop else "")


@pytest.mark.parametrize("case", _ex_cases(), ids=_id)
def test_float32_forms(solver, case):
    N, K, force, want_J, stop, only = case
    pr = problem(N, K, "randn")
    fr = run_solve(pr, False, force, want_J, stop)
    pk = run_solve(pr, True, force, want_J, stop)
    check_layout(fr, pk)
    check_oracle(pr, fr, "float32 forms", EPS)
    if only:
        # the plan of THIS call (its count, stop rule and flag): one launch of the form the flag stands for at this length
        want = "fista_mfma4_kernel" if N > 640 else "fista_mfma2_kernel" if force.startswith("mfma2") else "fista_mfma_kernel"
        if force.startswith("mfma"):
            plan = solver.launch_plan(N, K, ROWS, stop=stop, force=force)
            assert plan[0] == 0 and plan[2].startswith(want + " "), plan
        no = run_solve(pr, False, only, want_J, stop)
        check_no_resolve(pr, no, "float32 forms, no re-solve", EPS, bits(torch.from_numpy(pr.W0).to(dev())))


# ---- float64 end to end: one wave, four waves, the LDS kernel ---------------------------------------------------------------
@pytest.mark.parametrize("stop", [None, "window", "loops"])
@pytest.mark.parametrize("N,force,form", [(300, None, 7), (1200, None, 8), (1200, "generic", 0)])
def test_float64_forms(solver, N, force, form, stop):
    K = 28
    pr = problem(N, K, "block64")
    assert (pr.lam < 0).any()
    if force is None:
        assert solver.which_kernel_f64(N, K, want_J=True, stop=stop) == solver.KERNEL_NAMES[form]
    fr = run_solve(pr, False, force, True, stop)
    pk = run_solve(pr, True, force, True, stop)
    assert fr.J.ld > NI
    check_layout(fr, pk)
    check_oracle(pr, fr, "float64 forms", BOUND)


# ---- the device-resident lambda search ---------------------------------------------------------------------------------------
def _block_signal(n, hrf, rng):
    """The rows of tests/test_gpu_auto_lbda_device.py::test_shapes_against_the_oracle."""
    z = np.zeros(n)
    for start in range(3, n, max(n // 6, 8)):
        z[start:start + max(n // 14, 3)] = rng.uniform(0.5, 1.5)
    x = orc.causal_conv(hrf, z)
    return x + 0.4 * np.std(x) * rng.standard_normal(n)


def _run_auto(a, packed):
    from pybold_amd import _lib
    d = dev()
    V, N = a.Y.shape
    r = SimpleNamespace()
    r.y = frames.frame2d("y", V, N, F64, d, fill=a.Y, packed=packed)
    r.w = frames.frame2d("W", V, N, F64, d, packed=packed)                  # cold: output only
    r.sigma = frames.frame1d("sigma", V, F64, d, fill=a.sigma, packed=packed)
    r.R, r.G, r.J = (frames.frame2d("trace", V, a.nb_iter, F64, d, packed=packed) for _ in range(3))
    r.alpha, r.lbda = frames.frame1d("alpha", V, F64, d, packed=packed), frames.frame1d("lbda", V, F64, d, packed=packed)
    r.n_outer = frames.frame1d("n_outer", V, I32, d, packed=packed)
    r.n_inner = frames.frame1d("n_inner", V, I64, d, packed=packed)
    r.work = frames.frame1d("work", int(_lib.load().pb_auto_lbda_work_len(V)), F64, d, packed=packed)
    r.outs = [r.w, r.R, r.G, r.J, r.alpha, r.lbda, r.n_outer, r.n_inner, r.work]
    r.ins = [r.y, r.sigma]
    for f in r.outs + r.ins:
        f.snapshot()
    r.ins.append(frames.auto_lbda_d(r.y, r.w, a.hrf, a.step, r.sigma, a.nb_iter, a.nb_sub_iter, R=r.R, G=r.G, J=r.J, alpha=r.alpha,
                                    lbda=r.lbda, n_outer=r.n_outer, n_inner=r.n_inner, work=r.work, cold=True))
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("N", [300, 640])
def test_device_lambda_search(solver, N):
    from pybold_amd import utils
    from pybold_amd.linear import ConvAndLinear, DiscretInteg
    K, V = 30, 5
    rng = np.random.default_rng(1000 * N + K)
    hrf = orc.spm_hrf(1.0, t_r=30.0 / K, dur=30.0, normalized_hrf=False)[0][:K]
    Y = np.stack([_block_signal(N, hrf, rng) for _ in range(V)])
    sigma = utils.mad_daub_noise_est(Y) * np.array([0.5, 1.0, 1.5, 0.75, 1.25])
    np.random.seed(0)
    lip = 0.9 * utils.spectral_radius_est(ConvAndLinear(DiscretInteg(), hrf, dim_in=N, dim_out=N), (N,))
    a = SimpleNamespace(Y=Y, hrf=hrf, sigma=sigma, step=1.0 / lip, nb_iter=6, nb_sub_iter=40)
    assert solver.auto_lbda_supported(N, K)
    fr, pk = _run_auto(a, False), _run_auto(a, True)
    assert fr.R.ld > a.nb_iter
    check_layout(fr, pk, equal=("w", "R", "G", "J", "alpha", "lbda", "n_outer", "n_inner"))
    Wo, Jo, Ro, Go, n_outer = c_oracle.deconv_auto_lbda_batch(Y, hrf, sigma, lip, nb_iter=a.nb_iter, nb_sub_iter=a.nb_sub_iter,
                                                             threads=16)
    assert (fr.n_outer.contiguous().cpu().numpy() == n_outer).all()
    W = fr.w.contiguous().cpu().numpy()
    worst = rel_rows(W, Wo).max()
    for T, To in ((fr.R, Ro), (fr.G, Go), (fr.J, Jo)):
        Tn, unwritten = T.contiguous().cpu().numpy(), T.is_sentinel().cpu().numpy()
        for v in range(V):
            n = int(n_outer[v])
            assert unwritten[v, n:].all() and not unwritten[v, :n].any()       # entries from n_outer on are left untouched
            worst = max(worst, np.linalg.norm(Tn[v, :n] - To[v, :n]) / np.linalg.norm(To[v, :n]))
    note("device lambda search", worst)
    assert worst < AUTO_BOUND
    lb = fr.lbda.contiguous().cpu().numpy()
    np.testing.assert_array_equal(lb, 1.0 / (2.0 * fr.alpha.contiguous().cpu().numpy()))
    assert (fr.n_inner.contiguous().cpu().numpy() > 0).all()


# ---- the backtracked step ------------------------------------------------------------------------------------------------------
def test_backtracked_step(solver):
    N, K, P = 300, 30, ROWS
    d = dev()
    V = (P + Y_REP - 1) // Y_REP
    hrf, step0 = hrf_for(K), 8.0 * step_for(N, K)
    rng = np.random.RandomState(5)
    Y = block_rows(V, N, K, seed=77).double().cpu().numpy()
    lam = np.linspace(0.05, 5.0, P)
    W0 = 0.01 * rng.randn(P, N)

    def run(packed):
        r = SimpleNamespace()
        r.y = frames.frame2d("y", V, N, F64, d, fill=Y, packed=packed)
        r.w = frames.frame2d("W", P, N, F64, d, fill=W0, packed=packed)
        r.lam = frames.frame1d("lbda", P, F64, d, fill=lam, packed=packed)
        r.nd, r.halv = frames.frame1d("n_done", P, I32, d, packed=packed), frames.frame1d("halvings", P, I32, d, packed=packed)
        r.step = frames.frame1d("step", P, F64, d, packed=packed)
        r.outs, r.ins = [r.w, r.nd, r.halv, r.step], [r.y, r.lam]
        for f in r.outs + r.ins:
            f.snapshot()
        r.ins.append(frames.fista_solve_backtrack_d(r.y, r.w, hrf, step0, NI, lbda_v=r.lam, n_done=r.nd, step_out=r.step,
                                                    halvings=r.halv, y_rep=Y_REP))
        torch.cuda.synchronize()
        return r

    fr, pk = run(False), run(True)
    check_layout(fr, pk, equal=("w", "nd", "halv", "step"))
    Wo, so, ho, margin = orc.fista_backtrack_batch(np.repeat(Y, Y_REP, axis=0)[:P], hrf, lam, step0, NI, W0=W0)
    robust = margin > 1e-9                                # (tests/test_gpu_round5.py: decisions away from equality)
    assert robust.sum() >= P - 2, margin
    assert (fr.halv.contiguous().cpu().numpy()[robust] == ho[robust]).all() and int(fr.halv.contiguous().max()) >= 1
    assert (fr.step.contiguous().cpu().numpy()[robust] == so[robust]).all()
    err = rel_rows(fr.w.contiguous().cpu().numpy()[robust], Wo[robust]).max()
    note("backtracked step", err)
    assert err < 1e-10                                    # the bound of test_backtracked_step_opt_in_mode
    assert (fr.nd.contiguous().cpu().numpy() == NI).all()


# ---- pb_fista_solve_pp ----------------------------------------------------------------------------------------------------------
_pp = {}


def pp_problem(N, shared):
    if (N, shared) in _pp:
        return _pp[(N, shared)]
    rng = np.random.RandomState(7 * N + shared)
    P = ROWS
    pr = SimpleNamespace(N=N, P=P, f64=False)
    pr.Y = rng.randn(P, N).astype(np.float32)
    pr.lam = np.tile([0.05, 0.3, 1.0], P)[:P] * rng.uniform(0.8, 1.25, P)
    pr.W0 = 0.01 * rng.randn(P, N)
    if shared:
        pr.K = 28 if N > 640 else 30
        pr.taps = hrf_for(pr.K)[None, :]
        pr.steps = np.array([step_for(N, pr.K)])
    else:                                                 # one dilation of the reference's model per problem
        pr.taps = np.stack([orc.spm_hrf(th, 1.0, 30.0, False)[0] for th in np.linspace(0.7, 1.3, P)])
        pr.K = pr.taps.shape[1]
        pr.steps = np.array([1.0 / orc.gram_lipschitz(h, N) for h in pr.taps])
    Yo = pr.Y.astype(np.float64)
    pr.Wo = np.stack([c_oracle.fista_batch(Yo[p:p + 1], pr.taps[0 if shared else p], pr.lam[p], pr.steps[0 if shared else p], NI,
                                           W0=pr.W0[p:p + 1], threads=1)[0][0] for p in range(P)])
    _pp[(N, shared)] = pr
    return pr


def run_pp(pr, shared, packed, force, stop):
    d = dev()
    r = SimpleNamespace(J=None)
    r.y = frames.frame2d("y", pr.P, pr.N, F32, d, fill=pr.Y, packed=packed)
    r.w = frames.frame2d("W", pr.P, pr.N, F64, d, fill=pr.W0, packed=packed)          # iterated in place
    r.lam = frames.frame1d("lbda", pr.P, F64, d, fill=pr.lam, packed=packed)
    if shared:
        r.taps = frames.frame1d("taps", pr.K, F64, d, fill=pr.taps[0], packed=packed)
    else:
        r.taps = frames.frame2d("taps_pp", pr.P, pr.K, F64, d, fill=pr.taps, packed=packed)
    r.steps = frames.frame1d("step_vec", len(pr.steps), F64, d, fill=pr.steps, packed=packed)
    r.nd = frames.frame1d("n_done", pr.P, I32, d, packed=packed)
    r.outs, r.ins = [r.w, r.nd], [r.y, r.lam, r.taps, r.steps]
    for f in r.outs + r.ins:
        f.snapshot()
    r.ins.append(frames.fista_solve_pp(r.y, r.w, r.taps, r.steps, NI, pr.K, lbda_v=r.lam, n_done=r.nd, stop=stop, tol=TOL[stop],
                                       force=force))
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("stop", [None, "loops"])
@pytest.mark.parametrize("force", ["fast1", None, "generic"])
def test_per_problem_hrfs(solver, force, stop):
    pr = pp_problem(300, False)
    fr, pk = run_pp(pr, False, False, force, stop), run_pp(pr, False, True, force, stop)
    assert fr.taps.ld > pr.K
    check_layout(fr, pk, equal=("w", "nd"))
    check_oracle(pr, fr, "per-problem HRFs", EPS)


@pytest.mark.parametrize("N,force,only", [(300, "fast2", None), (300, "mfma", "mfmaonly"), (600, "mfma2", "mfma2only"),
                                          (1200, "mfma2", "mfma2only")])
def test_one_shared_hrf_in_device_memory(solver, N, force, only):
    pr = pp_problem(N, True)
    fr, pk = run_pp(pr, True, False, force, None), run_pp(pr, True, True, force, None)
    check_layout(fr, pk, equal=("w", "nd"))
    check_oracle(pr, fr, "one shared HRF in device memory", EPS)
    if only:
        if force == "mfma":                               # one launch of the one-wave form over every problem
            assert solver.launch_plan(N, pr.K, pr.P, force="mfma")[2].startswith("fista_mfma_kernel ")
        else:                                             # (the plan of a pb_fista_solve_ex call of this shape: route_pp takes the same split forms)
            assert solver.launch_plan(N, pr.K, pr.P, force=force)[2].startswith("fista_mfma4_kernel " if N > 640 else "fista_mfma2_kernel ")
        no = run_pp(pr, True, False, only, None)
        check_no_resolve(pr, no, "one shared HRF, no re-solve", EPS, bits(torch.from_numpy(pr.W0).to(dev())))


# ---- outputs and statistics ---------------------------------------------------------------------------------------------------
def test_outputs_and_statistics(solver):
    N, K, P = 300, 30, ROWS
    d = dev()
    V = (P + Y_REP - 1) // Y_REP
    hrf = hrf_for(K)
    rng = np.random.RandomState(3)
    Wn = rng.randn(P, N) * (rng.rand(P, N) < 0.1)
    Yn = rng.randn(V, N)
    taps_pp = np.stack([orc.spm_hrf(th, 1.0, 30.0, False)[0] for th in np.linspace(0.7, 1.3, P)])
    Yrep = np.repeat(Yn, Y_REP, axis=0)[:P]
    Zo = np.cumsum(Wn, axis=1)

    def run(packed):
        r = SimpleNamespace()
        mk2 = lambda kind, rows, cols, dt, fill=None: frames.frame2d(kind, rows, cols, dt, d, fill=fill, packed=packed)
        mk1 = lambda name, n, dt=F64, fill=None: frames.frame1d(name, n, dt, d, fill=fill, packed=packed)
        r.w, r.y32, r.y64 = mk2("W", P, N, F64, Wn), mk2("y", V, N, F32, Yn), mk2("y", V, N, F64, Yn)
        r.yv32 = mk2("y", P, N, F32, Yrep)                # one series per row: pb_lambda_max, pb_hrf_normal_eq_w
        r.taps = mk2("taps_pp", P, K, F64, taps_pp)
        r.z, r.x, r.zp, r.xp = (mk2("out", P, N, F64) for _ in range(4))
        r.r2, r.l1, r.r2d, r.l1d = (mk1(n, P) for n in ("r2", "l1", "r2_d", "l1_d"))
        r.lm, r.lmd = mk1("lambda_max", V), mk1("lambda_max_d", V)
        ne = K * K + K + 2
        r.ne, r.ne_work = mk1("normal_eq_w", ne), mk1("normal_eq_work", 64 * ne)
        r.outs = [r.z, r.x, r.zp, r.xp, r.r2, r.l1, r.r2d, r.l1d, r.lm, r.lmd, r.ne, r.ne_work]
        r.ins = [r.w, r.y32, r.y64, r.yv32, r.taps]
        for f in r.outs + r.ins:
            f.snapshot()
        frames.fista_outputs(r.w, hrf, z=r.z, x=r.x)
        frames.fista_outputs_pp(r.w, r.taps, K, z=r.zp, x=r.xp)
        frames.fista_stats(r.w, r.y32, hrf, r.r2, r.l1, y_rep=Y_REP)
        frames.fista_stats(r.w, r.y64, hrf, r.r2d, r.l1d, y_rep=Y_REP)
        frames.lambda_max(r.y32, hrf, r.lm)
        frames.lambda_max(r.y64, hrf, r.lmd)
        frames.hrf_normal_eq_w(r.w, r.yv32, K, r.ne_work, r.ne)
        torch.cuda.synchronize()
        return r

    fr, pk = run(False), run(True)
    assert fr.z.ld > N and fr.x.ld > N and fr.taps.ld > K
    check_layout(fr, pk, equal=("z", "x", "zp", "xp", "r2", "l1", "r2d", "l1d", "lm", "lmd", "ne"))
    get = lambda f: f.contiguous().cpu().numpy()
    # the tolerances of tests/test_gpu_round2.py: 1e-12 on z = cumsum(w), x, the statistics and lambda_max
    np.testing.assert_allclose(get(fr.z), Zo, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(get(fr.x), orc.causal_conv(hrf, Zo), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(get(fr.zp), Zo, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(get(fr.xp), np.stack([orc.causal_conv(taps_pp[p], Zo[p]) for p in range(P)]), rtol=1e-12, atol=1e-12)
    for y, r2, l1 in ((Yrep.astype(np.float32).astype(np.float64), fr.r2, fr.l1), (Yrep, fr.r2d, fr.l1d)):
        np.testing.assert_allclose(get(r2), np.sum(np.square(orc.causal_conv(hrf, Zo) - y), axis=1), rtol=1e-12)
        np.testing.assert_allclose(get(l1), np.abs(Wn).sum(axis=1), rtol=1e-12)
    np.testing.assert_allclose(get(fr.lm), orc.lambda_max(Yn.astype(np.float32), hrf), rtol=1e-12)
    np.testing.assert_allclose(get(fr.lmd), orc.lambda_max(Yn, hrf), rtol=1e-12)
    # the normal equations of hrf_fit_err from w: G[m][m'] = sum z[i-m] z[i-m'], b[m] = sum z[i-m] y[i], yy, sum ||w||_1;
    # sums of P * N ~ 1e4 products: n eps ~ 1e-12 of the largest sum of absolute terms (a diagonal entry of G)
    y = Yrep.astype(np.float32).astype(np.float64)
    S = np.stack([np.concatenate([np.zeros((P, m)), Zo[:, :N - m]], axis=1) for m in range(K)])      # (K, P, N): z shifted by m
    G = np.einsum("apn,bpn->ab", S, S)
    ne_o = np.r_[G.ravel(), np.einsum("apn,pn->a", S, y), np.sum(y * y), np.abs(Wn).sum()]
    np.testing.assert_allclose(get(fr.ne), ne_o, rtol=1e-12, atol=1e-12 * G.max())


# ---- calls partitioned on the device: perm, range, grid_slots, the workspace and only_flagged meet padded rows ------------------
def ill_families(N, y):
    """The ill-conditioned families of tests/test_gpu_round5.py::test_ill_conditioned_series_are_solved_in_float64 at any
    length (`y`: an ordinary series to mix in)."""
    t = np.arange(N)
    alt = np.where(t % 2 == 0, 1.0, -1.0)
    return [alt, np.sin(2 * np.pi * t / 3), np.sin(2 * np.pi * t / 4), alt + 1e-3 * y, 37.0 * alt, 1e-3 * alt]


_big = {}


def big_problem(solver, N, K, P, mixed, seed):
    """P block signals on the device.  `mixed` (partitioned calls): every 16th series from an ill-conditioned family,
    lambda_p = c_p lambda_max,p with c_p alternating 0.02 (dense class) and 0.9 (sparse class); else ONE lambda for the
    call (what the matrix-pipe forms of an unpartitioned call take).  The oracle runs on 256 sampled rows."""
    key = (N, K, P, mixed)
    if key in _big:
        return _big[key]
    d = dev()
    pr = SimpleNamespace(N=N, K=K, P=P, V=P, y_rep=1, hrf=hrf_for(K), step=step_for(N, K), f64=False)
    Y = block_rows(P, N, K, seed)
    gen = torch.Generator(device=d).manual_seed(seed + 1)
    pr.planted = np.arange(0, P, 16)
    if mixed:
        fams = ill_families(N, Y[1].double().cpu().numpy())
        Y[torch.from_numpy(pr.planted).to(d)] = torch.from_numpy(np.stack([fams[i % len(fams)] for i in range(len(pr.planted))])).to(d, F32)
        c = torch.where(torch.arange(P, device=d) % 2 == 0, 0.02, 0.9).double()
        pr.lam = (c * solver.lambda_max(Y, pr.hrf)).cpu().numpy()
    else:
        pr.lam = None
        pr.lam_scalar = 1.0
    pr.Y = Y
    pr.W0 = 0.01 * torch.randn((P, N), generator=gen, device=d, dtype=F64)
    rng = np.random.RandomState(seed)
    pr.rows = np.unique(np.r_[0, P - 1, pr.planted[:24], rng.choice(P, 230, replace=False)])       # 256 rows at most
    sel = torch.from_numpy(pr.rows).to(d)
    lam_o = pr.lam[pr.rows] if mixed else pr.lam_scalar
    Wo, Jo, _ = c_oracle.fista_batch(Y[sel].double().cpu().numpy(), pr.hrf, lam_o, pr.step, NI, W0=pr.W0[sel].cpu().numpy(),
                                     want_J=True, threads=16)
    pr.Wo, pr.Jo = np.zeros((P, N)), np.zeros((P, NI))
    pr.Wo[pr.rows], pr.Jo[pr.rows] = Wo, Jo
    _big[key] = pr
    return pr


def run_big(pr, packed, force, want_J, stop, work, cold=False):
    from pybold_amd import _lib
    d = dev()
    r = SimpleNamespace()
    r.y = frames.frame2d("y", pr.P, pr.N, F32, d, fill=pr.Y, packed=packed)
    r.w = frames.frame2d("W", pr.P, pr.N, F64, d, fill=None if cold else pr.W0, packed=packed)
    r.lam = frames.frame1d("lbda", pr.P, F64, d, fill=pr.lam, packed=packed) if pr.lam is not None else None
    r.J = frames.frame2d("J", pr.P, NI, F32, d, packed=packed) if want_J else None
    r.nd = frames.frame1d("n_done", pr.P, I32, d, packed=packed)
    r.work = frames.frame1d("work", int(_lib.load().pb_fista_work_len(pr.P, 1)), I32, d, packed=packed) if work else None
    r.outs = [f for f in (r.w, r.J, r.nd, r.work) if f is not None]
    r.ins = [f for f in (r.y, r.lam) if f is not None]
    for f in r.outs + r.ins:
        f.snapshot()
    r.ins.append(frames.fista_solve_ex(r.y, r.w, pr.hrf, pr.step, NI, lbda=0.0 if r.lam is not None else pr.lam_scalar, lbda_v=r.lam,
                                       J=r.J, n_done=r.nd, stop=stop, tol=TOL[stop], wind=6, force=force, cold=cold, work=r.work))
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("variant", ["plain", "window-J"])
@pytest.mark.parametrize("N,K,P,matrix_pipe", [(300, 30, 4112, False), (600, 30, 5136, False), (1200, 28, 4112, False),
                                               (300, 30, 10752, True), (300, 30, 19200, True), (600, 30, 6144, True),
                                               (1200, 28, 6144, True)])
def test_partitioned_calls(solver, N, K, P, matrix_pipe, variant):
    """The caller's workspace framed, n_done given.  P just above the thresholds of csrc/dispatch.h (PART_MIN_P = 4 096,
    MFMA2_LONG_MIN_P = 5 120): the call is partitioned -- lambda_max pass, index lists, device-side plan, perm / range /
    grid_slots in every launch, the float64 list -- but its dense class (7/16 of the problems) is too small to earn a pass
    of a matrix-pipe form (csrc/plan.h: plan_partitioned wants more than MFMA2_MIN_R = 4 608 dense problems at 300 scans,
    5/16 of a pass of 8 192 at 600, 10/16 of a pass of 4 096 at 1 200) and joins the sparse class on the vector forms.  The
    larger counts are the smallest at which the dense class runs where it is meant to: the two-wave form (300 scans,
    4 704 dense), the one-wave form (300 scans, 8 400 dense: above half a round), a pass of the two-wave / four-wave form
    (600 / 1 200 scans, 2 688 dense)."""
    want_J, stop = (False, None) if variant == "plain" else (True, "window")
    pr = big_problem(solver, N, K, P, True, seed=N)
    fr, pk = run_big(pr, False, None, want_J, stop, True), run_big(pr, True, None, want_J, stop, True)
    check_layout(fr, pk)                                  # (a) on all rows
    check_oracle(pr, fr, "partitioned calls", EPS, rows=pr.rows)
    assert (fr.nd.contiguous() == NI).all()
    # (e) both classes and the float64 list were non-empty: the measurement aids solve one class each, on a cold W
    written = {}
    for aid in ("path_dense", "path_sparse"):
        r = run_big(pr, False, aid, want_J, stop, True, cold=True)
        for f in r.outs:
            f.assert_outside_untouched()
        for f in r.ins:
            f.assert_untouched()
        unwritten = r.w.is_sentinel()
        in_class, done = ~r.nd.is_sentinel(), r.nd.contiguous() == NI            # (n_done = -1: handed back, iterate untouched)
        assert not bool(unwritten[done].any()) and bool(unwritten[~in_class].all())  # the other class's rows are left alone
        assert bool((done | (r.nd.contiguous() == -1))[in_class].all())
        written[aid] = in_class.cpu().numpy()
    dense, sparse = written["path_dense"], written["path_sparse"]
    ill = ~(dense | sparse)
    print("N %d, %s: %d dense, %d sparse, %d ill-conditioned of %d" % (N, variant, dense.sum(), sparse.sum(), ill.sum(), P))
    assert not (dense & sparse).any() and sparse.sum() > 0 and ill.sum() > 0
    assert np.isin(np.flatnonzero(ill), pr.planted).all()                     # the float64 list: planted series only
    odd = np.arange(P) % 2 == 1
    assert sparse[odd].all() and not dense[odd].any()                         # lambda = 0.9 lambda_max: never on the matrix pipe
    if matrix_pipe:                                       # path_dense runs the matrix-pipe candidates only
        assert dense.sum() > 0.8 * (7 * P // 16), dense.sum()
    else:               # the dense class is there (lambda = 0.02 lambda_max) but earns no matrix-pipe pass: every ordinary row on a vector form
        assert dense.sum() == 0 and sparse[~np.isin(np.arange(P), pr.planted)].all()


# ---- host-side plans with several pieces (run_pieces), whole passes plus remainder (run_passes) ---------------------------------
def _pieces_sizes(solver):
    # one round plus 300; plus just under half a round; plus half a round and 1.3 sixteenths: the left-overs of the two-wave
    # pass as one-problem waves beside it (csrc/plan.h: R in (half, half + beside_chunks * round / 16], two chunks)
    rnd = solver.round_size(300, 30)
    return [rnd + 300, rnd + rnd // 2 - 37, rnd + rnd // 2 + rnd // 16 + 300]


def _several_forms(solver, N, K, P, stop, force):
    n_main, main, tail = solver.launch_plan(N, K, P, stop=stop, force=force)
    if not (n_main > 0 and main != tail):
        pytest.skip("this device plans one form for N=%d, P=%d: %r" % (N, P, (n_main, main, tail)))
    return n_main


def _big_case(solver, pr, force, only, want_J, stop, group):
    fr, pk = run_big(pr, False, force, want_J, stop, False), run_big(pr, True, force, want_J, stop, False)
    check_layout(fr, pk)
    check_oracle(pr, fr, group, EPS, rows=pr.rows)
    assert (fr.nd.contiguous() == NI).all()
    no = run_big(pr, False, only, want_J, stop, False)
    check_no_resolve(pr, no, group + ", no re-solve", EPS, bits(pr.W0), rows=pr.rows)


@pytest.mark.parametrize("variant", ["plain", "window-J"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_host_side_plans_with_several_pieces(solver, which, variant):
    want_J, stop = (False, None) if variant == "plain" else (True, "window")
    P = _pieces_sizes(solver)[which]
    _several_forms(solver, 300, 30, P, stop, "nopart")
    pr = big_problem(solver, 300, 30, P, False, seed=11 + which)
    _big_case(solver, pr, "nopart", "noresolve", want_J, stop, "host-side plans")


@pytest.mark.parametrize("variant", ["plain", "window-J"])
@pytest.mark.parametrize("N,K,per_cu", [(600, 30, 32), (1200, 28, 16)])
def test_whole_pass_plus_remainder(solver, N, K, per_cu, variant):
    want_J, stop = (False, None) if variant == "plain" else (True, "window")
    npass = torch.cuda.get_device_properties(dev()).multi_processor_count * per_cu
    P = npass + ROWS
    assert _several_forms(solver, N, K, P, stop, "nopart") == npass
    pr = big_problem(solver, N, K, P, False, seed=N + 1)
    _big_case(solver, pr, "nopart", "noresolve", want_J, stop, "whole pass plus remainder")


@pytest.mark.parametrize("which", [0, 1, 2])
def test_shared_hrf_plan_with_several_pieces(solver, which):
    """pb_fista_solve_pp with ONE HRF in device memory: run_pieces on one stream (route_pp), where the third count puts
    the left-overs of the two-wave pass on one launch of one-problem waves behind it."""
    P = _pieces_sizes(solver)[which]
    base = big_problem(solver, 300, 30, P, False, seed=11 + which)
    d = dev()
    lam = np.random.RandomState(which).uniform(0.5, 1.5, P)
    Wo, _, _ = c_oracle.fista_batch(base.Y[torch.from_numpy(base.rows).to(d)].double().cpu().numpy(), base.hrf, lam[base.rows], base.step, NI,
                                    W0=base.W0[torch.from_numpy(base.rows).to(d)].cpu().numpy(), threads=16)
    pr = SimpleNamespace(N=300, K=30, P=P, Y=base.Y, W0=base.W0, lam=lam, taps=base.hrf[None, :], steps=np.array([base.step]), f64=False,
                         Wo=np.zeros((P, 300)))
    pr.Wo[base.rows] = Wo
    fr, pk = run_pp(pr, True, False, None, None), run_pp(pr, True, True, None, None)
    check_layout(fr, pk, equal=("w", "nd"))
    check_oracle(pr, fr, "shared-HRF plan with several pieces", EPS, rows=base.rows)
    assert (fr.nd.contiguous() == NI).all()
    no = run_pp(pr, True, False, "noresolve", None)
    check_no_resolve(pr, no, "shared-HRF plan, no re-solve", EPS, bits(pr.W0), rows=base.rows)


def test_regularisation_path_entry_point(solver):
    """pb_fista_solve_path (pb_fista_solve_ex with per-problem lambdas, the caller's lambda_max and workspace): lmax framed
    too, workspace of pb_fista_path_work_len entries."""
    from pybold_amd import _lib
    N, K, P = 300, 30, 4112
    pr = big_problem(solver, N, K, P, True, seed=N)
    d = dev()
    lmax = solver.lambda_max(pr.Y, pr.hrf)

    def run(packed):
        r = SimpleNamespace(J=None)
        r.y = frames.frame2d("y", P, N, F32, d, fill=pr.Y, packed=packed)
        r.w = frames.frame2d("W", P, N, F64, d, fill=pr.W0, packed=packed)
        r.lam = frames.frame1d("lbda", P, F64, d, fill=pr.lam, packed=packed)
        r.lmax = frames.frame1d("lmax", P, F64, d, fill=lmax, packed=packed)
        r.nd = frames.frame1d("n_done", P, I32, d, packed=packed)
        r.work = frames.frame1d("work", int(_lib.load().pb_fista_path_work_len(P)), I32, d, packed=packed)
        r.outs, r.ins = [r.w, r.nd, r.work], [r.y, r.lam, r.lmax]
        for f in r.outs + r.ins:
            f.snapshot()
        r.ins.append(frames.fista_solve_path(r.y, r.w, pr.hrf, pr.step, NI, r.lam, r.lmax, r.nd, r.work))
        torch.cuda.synchronize()
        return r

    fr, pk = run(False), run(True)
    check_layout(fr, pk, equal=("w", "nd"))
    check_oracle(pr, fr, "regularisation path entry point", EPS, rows=pr.rows)
    assert (fr.nd.contiguous() == NI).all()
    plain = run_big(pr, True, None, False, None, True)               # the same call through pb_fista_solve_ex: the same bits
    assert torch.equal(plain.w.window_bits(), fr.w.window_bits())
