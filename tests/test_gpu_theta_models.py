"""The theta-step kernels at every model branch, tap count and bracket edge: `theta_fit_kernel` (csrc/blind.h) through
`solver.theta_fit` / `solver.theta_fit_step`, `spm_hrf_kernel` (csrc/generic.h) through `solver.spm_hrf_batch`, on the
fixed problems of tests/theta_model_cases.py.  The minimiser, its cost and taps come from the mp run stored in
tests/golden/theta_models.npz; everything else is float64 scipy / NumPy at run time (tests/test_theta_models_host.py
shows how far those sit inside the tolerances used here).  The tolerances are the project's: theta 2e-7 (n_refine 3 on a
bracket of 1.3; 2e-3 and 2e-6 for one and two levels), taps rtol 1e-10 / atol 1e-14, cost rel 1e-8, HRF values rtol
1e-12 / atol 1e-15, ||A^T A||_F rtol 1e-11.

Each case launches a handful of one-workgroup kernels on series of 40 to 135 scans."""
import numpy as np
import pytest
import torch

from oracle import pybold_oracle as orc
from tests import theta_model_cases as cases

pytestmark = pytest.mark.gpu


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def ids(cs):
    return [c.name for c in cs]


@pytest.fixture(scope="module")
def solver():
    from pybold_amd import solver
    assert torch.cuda.is_available()
    return solver


@pytest.fixture(scope="module")
def fx(golden):
    return golden("theta_models")


class Problem:
    """One case on the host and on the device; the references are computed once and never written again."""

    def __init__(self, solver, fx, case):
        self.case, self.model = case, cases.MODELS[case.model]
        self.W, self.Y = fx[case.name + "/W"], fx[case.name + "/Y"]
        self.Z = np.cumsum(self.W, axis=1)
        self.yy = float(np.sum(self.Y * self.Y))
        self.theta_star, self.F_star = float(fx[case.name + "/theta_star"]), float(fx[case.name + "/F_star"])
        self.Zd, self.Yd = dev64(self.Z), dev64(self.Y)
        self.ne = solver.hrf_normal_eq(self.Zd, self.Yd, case.K)
        for a in (self.W, self.Y, self.Z):
            a.setflags(write=False)

    def hrf(self, theta):
        return orc.spm_hrf(float(theta), self.case.t_r, self.case.dur, False, **self.model)[0]

    def direct(self, theta, Z=None, Y=None):
        return cases.direct_cost(self.hrf(theta), self.Z if Z is None else Z, self.Y if Y is None else Y)

    def check_fit(self, theta, cost, taps, Z=None, Y=None):
        """Taps and cost of a returned dilation against scipy and the direct cost (one set)."""
        th = float(theta)
        np.testing.assert_allclose(taps.cpu().numpy().reshape(-1), self.hrf(th), rtol=1e-10, atol=1e-14)
        direct = self.direct(th, Z, Y)
        print("%s: theta %.12f cost %.15e direct %.15e" % (self.case.name, th, float(cost), direct))
        assert float(cost) == pytest.approx(direct, rel=1e-8)


@pytest.fixture(scope="module")
def problem(solver, fx):
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = Problem(solver, fx, case)
        return cache[case.name]
    return get


# ---- spm_hrf_kernel with every model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model,K", [(m, K) for m, taps in cases.HRF_BATCH_TAPS.items() for K in taps])
def test_spm_hrf_batch_with_model(solver, model, K):
    t_r, dur = cases.TAPS[K] if K in cases.TAPS else cases.POW_TAPS
    d = cases.hrf_batch_deltas(model, K)
    out = solver.spm_hrf_batch(dev64(d), t_r, dur, **cases.MODELS[model])
    assert tuple(out.shape) == cases.HRF_BATCH_SHAPE + (K,) and (d.size * K) % 256 != 0
    out = out.cpu().numpy()
    t = cases.sample_times(t_r, dur)
    for idx in np.ndindex(*d.shape):
        if d[idx] == cases.TINY_DELTA:
            ref = cases.ref_hrf(d[idx], t, model)                # (below the range orc.spm_hrf accepts)
            assert out[idx][0] == 0.0 and out[idx][1] == 0.0 and ref[1] == 0.0      # at or below the location: exact
        else:
            ref = orc.spm_hrf(d[idx], t_r, dur, False, **cases.MODELS[model])[0]
        np.testing.assert_allclose(out[idx], ref, rtol=1e-12, atol=1e-15, err_msg=str(idx))


# ---- the theta-step on every model and tap count ---------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.FITTED, ids=ids(cases.FITTED))
def test_theta_fit_finds_the_minimiser(solver, problem, case):
    p = problem(case)
    theta, cost, taps = solver.theta_fit(p.ne, case.t_r, case.dur, case.bounds, **p.model)
    assert theta.shape == (1,) and cost.shape == (1,) and taps.shape == (1, case.K)
    print("%s: |device - mp| = %.2e" % (case.name, abs(float(theta) - p.theta_star)))
    assert float(theta) == pytest.approx(p.theta_star, abs=cases.THETA_TOL[3])
    p.check_fit(theta, cost, taps)
    assert float(cost) <= p.F_star * (1 + 1e-9)


@pytest.mark.parametrize("case", cases.STEP_CASES, ids=ids(cases.STEP_CASES))
def test_theta_fit_step_against_independent_references(solver, problem, case):
    """theta, cost and taps equal pb_theta_fit on the same message bit for bit; the step and the normalised cost against
    NumPy's ||A^T A||_F and the direct cost."""
    p = problem(case)
    msg = solver.hrf_normal_eq_w(dev64(p.W), dev32(p.Y), case.K)
    theta, cost, taps = solver.theta_fit(msg[:-1], case.t_r, case.dur, case.bounds, **p.model)
    th2, f2, taps2, step, jc = solver.theta_fit_step(msg, case.t_r, case.dur, case.bounds, case.N, cases.LBDA, **p.model)
    assert torch.equal(theta, th2) and torch.equal(cost, f2) and torch.equal(taps[0], taps2)
    th = float(th2)
    direct = p.direct(th)
    jc_ref = (2.0 * direct + cases.LBDA * float(np.abs(p.W).sum())) / p.yy
    fro = orc.gram_lipschitz(p.hrf(th), case.N)
    print("%s: 1/step %.15e fro %.15e jcost %.15e ref %.15e" % (case.name, 1.0 / float(step), fro, float(jc), jc_ref))
    assert float(jc) == pytest.approx(jc_ref, rel=1e-8)
    if case.kind == "constant":
        assert th == case.bounds[0] and fro == 0.0 and 1.0 / float(step) == 0.0
    else:
        assert th == pytest.approx(p.theta_star, abs=cases.THETA_TOL[3])
        np.testing.assert_allclose(1.0 / float(step), fro, rtol=1e-11)


@pytest.mark.parametrize("case", [c for c in cases.CASES if c.kind == "constant"],
                         ids=ids([c for c in cases.CASES if c.kind == "constant"]))
def test_constant_cost_returns_the_lower_bound(solver, problem, case):
    """K = 1: t[0] = 0, every candidate prices h == 0 and the first minimum wins at every level."""
    p = problem(case)
    for n_refine in cases.N_REFINE:
        theta, cost, taps = solver.theta_fit(p.ne, case.t_r, case.dur, case.bounds, n_refine=n_refine, **p.model)
        assert float(theta) == case.bounds[0], n_refine
        assert float(cost) == pytest.approx(0.5 * p.yy, rel=1e-14)
        assert float(taps.abs().max()) == 0.0 and taps.shape == (1, 1)


# ---- bracket edges at K = 27 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", cases.BRACKET_NAMES)
@pytest.mark.parametrize("case", cases.BRACKET_CASES, ids=ids(cases.BRACKET_CASES))
def test_bracket_edges(solver, problem, case, variant):
    p = problem(case)
    name, bounds, kind = [v for v in cases.bracket_variants(p.theta_star) if v[0] == variant][0]
    theta, cost, taps = solver.theta_fit(p.ne, case.t_r, case.dur, bounds, **p.model)
    th = float(theta)
    print("%s %s: bounds (%.12f, %.12f) theta %.12f mp %.12f" % (case.name, name, bounds[0], bounds[1], th, p.theta_star))
    if kind == "interior":
        assert th == pytest.approx(p.theta_star, abs=cases.THETA_TOL[3])
        assert float(cost) <= p.F_star * (1 + 1e-9)
    elif kind == "point":
        assert th == 1.0
    else:
        bound = bounds[0] if kind == "lo" else bounds[1]
        assert th == pytest.approx(bound, abs=1e-12)
        assert float(cost) == pytest.approx(p.direct(bound), rel=1e-8)
    p.check_fit(theta, cost, taps)
    if name.endswith("cell-0.8"):
        # one level on a minimiser in the second / last-but-one cell: the parabola of the first scan through the bound
        th1, f1, taps1 = solver.theta_fit(p.ne, case.t_r, case.dur, bounds, n_refine=1, **p.model)
        assert float(th1) == pytest.approx(p.theta_star, abs=cases.THETA_TOL[1])
        p.check_fit(th1, f1, taps1)


@pytest.mark.parametrize("n_refine", cases.N_REFINE)
@pytest.mark.parametrize("case", cases.BRACKET_CASES, ids=ids(cases.BRACKET_CASES))
def test_refinement_levels(solver, problem, case, n_refine):
    p = problem(case)
    theta, cost, taps = solver.theta_fit(p.ne, case.t_r, case.dur, case.bounds, n_refine=n_refine, **p.model)
    print("%s n_refine %d: |device - mp| = %.2e" % (case.name, n_refine, abs(float(theta) - p.theta_star)))
    assert float(theta) == pytest.approx(p.theta_star, abs=cases.THETA_TOL[n_refine])
    assert float(cost) >= p.F_star * (1 - 1e-9)
    p.check_fit(theta, cost, taps)


# ---- layouts of the normal-equation sets -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.BRACKET_CASES, ids=ids(cases.BRACKET_CASES))
def test_layouts_of_the_sets(solver, problem, case):
    p = problem(case)
    K, ne_len = case.K, case.K * case.K + case.K + 1
    kw = dict(p.model)
    pv = solver.hrf_normal_eq(p.Zd, p.Yd, K, per_voxel=True)
    assert pv.shape == (cases.N_VOX, ne_len) and p.ne.shape == (ne_len,)
    th, f, taps = solver.theta_fit(pv, case.t_r, case.dur, case.bounds, **kw)
    assert th.shape == (3,) and taps.shape == (3, K)
    # every set against the restated search on its own normal equations and the direct cost of its voxel
    for v in range(cases.N_VOX):
        G, b, yy = orc.hrf_normal_eq(p.Z[v], p.Y[v], K)
        th_o = orc.theta_fit_normal_eq(G, b, yy, case.t_r, case.dur, case.bounds, n_refine=3, schedule="kernel", **kw)[0]
        assert float(th[v]) == pytest.approx(th_o, abs=cases.THETA_TOL[3]), v
        p.check_fit(th[v], f[v], taps[v], p.Z[v:v + 1], p.Y[v:v + 1])
    # the same sets as rows of a wider buffer, the pad full of NaN: bit-equal to the contiguous call
    buf = torch.full((cases.N_VOX, ne_len + 5), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :ne_len] = pv
    view = buf[:, :ne_len]
    assert view.stride(0) == ne_len + 5 and not view.is_contiguous()
    th_w, f_w, taps_w = solver.theta_fit(view, case.t_r, case.dur, case.bounds, **kw)
    assert torch.equal(th_w, th) and torch.equal(f_w, f) and torch.equal(taps_w, taps)
    # a single row taken as a view of that buffer, 1-D and 2-D
    for row in (buf[1, :ne_len], buf[1:2, :ne_len]):
        th_1, f_1, taps_1 = solver.theta_fit(row, case.t_r, case.dur, case.bounds, **kw)
        assert torch.equal(th_1, th[1:2]) and torch.equal(f_1, f[1:2]) and torch.equal(taps_1, taps[1:2])
    assert bool(torch.isnan(buf[:, ne_len:]).all())


# ---- which density formula ran ---------------------------------------------------------------------------------------
def _taps_and_kernel_values(solver, p):
    case = p.case
    theta, _, taps = solver.theta_fit(p.ne, case.t_r, case.dur, case.bounds, **p.model)
    return taps[0], solver.spm_hrf_batch(theta, case.t_r, case.dur, **p.model)[0]


@pytest.mark.parametrize("name", ["nonint-K27", "nonint-K127"])
def test_exp_log_densities_are_spm_hrf_kernels_formula(solver, problem, name):
    """A shape without an integer power up to 64 is priced by exp((a-1) log v - v - lgamma a), the formula of
    spm_hrf_kernel: the taps of the fit equal that kernel's values at the returned dilation bit for bit."""
    taps, ref = _taps_and_kernel_values(solver, problem(cases.BY_NAME[name]))
    assert cases.model_path(cases.BY_NAME[name].model) == "explog+explog"
    assert torch.equal(taps, ref)


def test_power_65_is_priced_by_exp_log(solver, problem):
    """pow65: the peak takes its integer power, the undershoot (a - 1 = 65) the exp/log formula.  With lo == hi the fit
    returns h(theta) itself, and h = peak - 0.5 * undershoot is one rounding of two values the library also gives alone:
    the peak from the same fit with ratio 0, and 0.5 * undershoot by spm_hrf_kernel's exp/log formula with the peak's
    location moved past the window (a density is exactly 0 at or below its location; the product by 0.5 is exact)."""
    p = problem(cases.BY_NAME["pow65-K30"])
    case, m = p.case, p.model
    assert cases.model_path(case.model) == "int+explog" and m["p_u_ratio"] == 0.5
    th = 1.45
    full = solver.theta_fit(p.ne, case.t_r, case.dur, (th, th), **m)[2][0].cpu().numpy()
    peak = solver.theta_fit(p.ne, case.t_r, case.dur, (th, th), **dict(m, p_u_ratio=0.0))[2][0].cpu().numpy()
    late = dict(m, p_delay=6.0e-6, p_disp=1.0e-6)                  # location 1000 s
    assert cases.DT / late["p_disp"] > th * case.dur
    half_under = -solver.spm_hrf_batch(dev64([th]), case.t_r, case.dur, **late)[0].cpu().numpy()
    assert half_under.max() >= 0.1 * np.abs(full).max() and (half_under >= 0.0).all()
    assert np.array_equal(full, peak - half_under)


@pytest.mark.parametrize("name", ["default-K27", "int_locs_differ-K27", "pow64-K30"])
def test_integer_powers_are_not_priced_by_exp_log(solver, problem, name):
    """Integer a - 1 up to 64 takes the power by repeated squaring: the same values as spm_hrf_kernel's exp/log formula to
    rounding, but not its bits on all of 27 (30) taps."""
    taps, ref = _taps_and_kernel_values(solver, problem(cases.BY_NAME[name]))
    assert "explog" not in cases.model_path(cases.BY_NAME[name].model)
    np.testing.assert_allclose(taps.cpu().numpy(), ref.cpu().numpy(), rtol=1e-12, atol=1e-15)
    differ = int((taps != ref).sum())
    print("%s: %d of %d taps differ in bits from the exp/log formula" % (name, differ, taps.numel()))
    assert differ > 0


# ---- refusals happen on the host, before any launch ------------------------------------------------------------------
def test_refusals_launch_nothing(solver):
    from pybold_amd import _lib
    lib = _lib.load()
    t_r, dur = cases.K_TOO_MANY
    K = len(solver.hrf_sample_times(t_r, dur))
    assert K == cases.K_MAX + 1
    ne = torch.zeros((K * K + K + 1,), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.PyboldHipError, match="pb_theta_fit: bad argument"):
        solver.theta_fit(ne, t_r, dur, cases.BOUNDS)
    msg = torch.zeros((K * K + K + 2,), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.PyboldHipError, match="pb_theta_fit_step: bad argument"):
        solver.theta_fit_step(msg, t_r, dur, cases.BOUNDS, 200, cases.LBDA)
    t27 = cases.TAPS[27]
    ne27 = torch.zeros((27 * 27 + 27 + 1,), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.PyboldHipError, match="pb_theta_fit: bad argument"):
        solver.theta_fit(ne27, t27[0], t27[1], (1.9, 0.6))
    # the outputs of a refused call keep what they held
    t_dev = solver._sample_times_on(ne.device, t_r, dur)
    out = torch.full((2 + K,), float("nan"), dtype=torch.float64, device="cuda")
    a1, loc1, a2, loc2, ratio = cases.model_doubles("default")
    for k, sets, lo, hi in ((K, ne, 0.6, 1.9), (27, ne27, 1.9, 0.6)):
        rc = lib.pb_theta_fit(sets.data_ptr(), sets.numel(), 1, k, t_dev.data_ptr(), a1, loc1, a2, loc2, ratio, lo, hi, 3,
                              out[0:1].data_ptr(), out[1:2].data_ptr(), out[2:].data_ptr(), k, None)
        assert rc != 0 and b"pb_theta_fit: bad argument" in lib.pb_last_error()
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
