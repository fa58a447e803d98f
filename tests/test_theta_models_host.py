"""CPU-only checks of tests/golden/theta_models.npz against the float64 oracle: every tolerance that
tests/test_gpu_theta_models.py holds the device to is shown here to hold, with room, for the reference alone -- the
restated section search against the high-precision minimiser, scipy's HRF against the mp taps, NumPy's ||A^T A||_F
against the mp one -- and the conditions on the cases (one local minimum, a cost away from the cancellation floor, a
minimiser away from the bounds, an undershoot that shows) are re-asserted from the stored series."""
import numpy as np
import pytest

from oracle import pybold_oracle as orc
from tests import theta_model_cases as cases

IDS = [c.name for c in cases.CASES]


@pytest.fixture(scope="module")
def fx(golden):
    return golden("theta_models")


@pytest.fixture(scope="module")
def problem(fx):
    """`(Z, Y, t, G, b, yy)` of a case, computed once."""
    cache = {}

    def get(case):
        if case.name not in cache:
            W, Y = fx[case.name + "/W"], fx[case.name + "/Y"]
            Z = np.cumsum(W, axis=1)
            cache[case.name] = (Z, Y, cases.sample_times(case.t_r, case.dur)) + orc.hrf_normal_eq(Z, Y, case.K)
        return cache[case.name]
    return get


def test_case_table_reaches_every_path_and_tap_count():
    assert [cases.model_path(m) for m in cases.MODELS] == ["fused", "int+int", "explog+explog", "int+explog", "fused",
                                                            "fused", "int+explog"]
    assert cases.MODELS["pow64"]["undershoot"] - 1 == cases.INT_POWER_MAX == cases.MODELS["pow65"]["undershoot"] - 2
    for K, (t_r, dur) in cases.TAPS.items():
        assert len(cases.sample_times(t_r, dur)) == K
    assert len(cases.sample_times(*cases.POW_TAPS)) == 30
    assert len(cases.sample_times(*cases.K_TOO_MANY)) == cases.K_MAX + 1
    assert sorted(cases.TAPS) == [1, 3, 16, 17, 27, 42, 60, cases.K_MAX]
    names = set(IDS)
    for K in (3, 17, 27):
        assert {"%s-K%d" % (m, K) for m in cases.GENERAL_MODELS} <= names
    for K in cases.TAPS:
        assert {"%s-K%d" % (m, K) for m in cases.WIDE_K_MODELS} <= names
    assert {c.kind for c in cases.CASES} == {"interior", "constant", "short", "square"}
    assert all(c.N == max(c.K + 8, 40) for c in cases.CASES if c.kind in ("interior", "constant"))
    assert [(c.K, c.N) for c in cases.CASES if c.kind in ("short", "square")] == [(27, 20), (27, 27)]
    for m, taps in cases.HRF_BATCH_TAPS.items():
        for K in taps:
            assert (np.prod(cases.HRF_BATCH_SHAPE) * K) % 256 != 0


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_fixture_holds_the_case_as_the_table_draws_it(fx, case):
    """The stored series are what `cases.draw` gives for the stored seed, Z is exact, Y is float32."""
    W, Y = cases.draw(case, int(fx[case.name + "/seed_bump"]))
    assert np.array_equal(W, fx[case.name + "/W"]) and np.array_equal(Y, fx[case.name + "/Y"])
    assert np.array_equal(W * 64.0, np.round(W * 64.0)) and np.abs(np.cumsum(W, axis=1)).max() < 2.0 ** 20
    assert np.array_equal(Y, Y.astype(np.float32).astype(np.float64))
    assert np.array_equal(fx[case.name + "/model"], cases.model_doubles(case.model))
    assert (float(fx[case.name + "/t_r"]), float(fx[case.name + "/dur"])) == (case.t_r, case.dur)
    assert tuple(fx[case.name + "/bounds"]) == case.bounds


@pytest.mark.parametrize("case", cases.FITTED, ids=[c.name for c in cases.FITTED])
def test_conditions_on_the_cost(fx, problem, case):
    Z, Y, t, G, b, yy = problem(case)
    lo, hi = case.bounds
    th_star, F_star = float(fx[case.name + "/theta_star"]), float(fx[case.name + "/F_star"])
    grid = np.linspace(lo, hi, 2601)
    f = np.array([cases.quad_cost(cases.ref_hrf(th, t, case.model), G, b, yy) for th in grid])
    assert cases.count_local_minima(f) == 1 == int(fx[case.name + "/n_minima"])
    assert abs(grid[int(np.argmin(f))] - th_star) <= (hi - lo) / 2600.0
    assert F_star >= 1e-3 * 0.5 * yy
    cell = (hi - lo) / 63.0
    assert lo + 2 * cell <= th_star <= hi - 2 * cell
    # the quadratic form and the direct cost are the same number in float64, far inside the device's rel=1e-8
    h = cases.ref_hrf(th_star, t, case.model)
    assert cases.quad_cost(h, G, b, yy) == pytest.approx(F_star, rel=1e-11)
    assert cases.direct_cost(h, Z, Y) == pytest.approx(F_star, rel=1e-11)
    if case.model in cases.POW_MODELS:
        assert min(cases.undershoot_share(th, t, case.model) for th in grid[::10]) >= 0.1


@pytest.mark.parametrize("case", cases.FITTED, ids=[c.name for c in cases.FITTED])
def test_restated_algorithm_finds_the_high_precision_minimiser(fx, problem, case):
    _, _, _, G, b, yy = problem(case)
    th, f, h = orc.theta_fit_normal_eq(G, b, yy, case.t_r, case.dur, case.bounds, n_refine=3, schedule="kernel",
                                       **cases.MODELS[case.model])
    th_star = float(fx[case.name + "/theta_star"])
    print("%s: |restated - mp| = %.2e (stored %.2e)" % (case.name, abs(th - th_star), float(fx[case.name + "/restated_gap"])))
    assert th == pytest.approx(th_star, abs=cases.HOST_THETA_TOL[3])
    assert f <= float(fx[case.name + "/F_star"]) * (1 + 1e-11)


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_oracle_hrf_and_gram_match_the_high_precision_values(fx, case):
    """scipy's taps at a fifth of the device's (rtol 1e-12, atol 1e-15), NumPy's norm at a tenth of its rtol 1e-11."""
    th_star, h_star = float(fx[case.name + "/theta_star"]), fx[case.name + "/h_star"]
    h = orc.spm_hrf(th_star, case.t_r, case.dur, False, **cases.MODELS[case.model])[0]
    assert h.shape == (case.K,)
    assert np.array_equal(h, cases.ref_hrf(th_star, cases.sample_times(case.t_r, case.dur), case.model))
    gap = np.abs(h - h_star).max()
    print("%s: max |scipy h - mp h| = %.2e (stored %.2e), max |h| = %.3f" % (case.name, gap, float(fx[case.name + "/h_gap"]),
                                                                             np.abs(h_star).max()))
    np.testing.assert_allclose(h, h_star, rtol=2e-13, atol=2e-16)
    gram = float(fx[case.name + "/gram_star"])
    if case.kind == "constant":
        assert np.all(h_star == 0.0) and gram == 0.0 and th_star == case.bounds[0]
    else:
        assert orc.gram_lipschitz(h_star, case.N) == pytest.approx(gram, rel=1e-12)


def test_kernel_schedule_is_an_option_and_the_default_is_unchanged(fx, problem):
    """`schedule="uniform"` (the default) is the search the existing callers get; the model keywords are spm_hrf's."""
    case = cases.BY_NAME["default-K27"]
    _, _, _, G, b, yy = problem(case)
    th_u = orc.theta_fit_normal_eq(G, b, yy, case.t_r, case.dur, case.bounds)[0]
    th_d = orc.theta_fit_normal_eq(G, b, yy, case.t_r, case.dur, case.bounds, n_refine=3, n_grid=64, schedule="uniform",
                                   **cases.MODELS["default"])[0]
    assert th_u == th_d == pytest.approx(float(fx[case.name + "/theta_star"]), abs=1e-8)
    with pytest.raises(ValueError):
        orc.theta_fit_normal_eq(G, b, yy, case.t_r, case.dur, case.bounds, schedule="other")


@pytest.mark.parametrize("case", cases.BRACKET_CASES, ids=[c.name for c in cases.BRACKET_CASES])
def test_bracket_cases_hold_for_the_restated_algorithm(fx, problem, case):
    _, _, t, G, b, yy = problem(case)
    th_star = float(fx[case.name + "/theta_star"])
    kw = dict(schedule="kernel", **cases.MODELS[case.model])
    variants = cases.bracket_variants(th_star)
    assert [v[0] for v in variants] == cases.BRACKET_NAMES
    for name, bounds, kind in variants:
        assert cases.BOUNDS[0] <= bounds[0] <= bounds[1] <= cases.BOUNDS[1], name
        th = orc.theta_fit_normal_eq(G, b, yy, case.t_r, case.dur, bounds, n_refine=3, **kw)[0]
        want = {"interior": th_star, "lo": bounds[0], "hi": bounds[1], "point": 1.0}[kind]
        assert th == pytest.approx(want, abs=cases.HOST_THETA_TOL[3] if kind == "interior" else 1e-12), name
        if name.endswith("cell-0.3") or name.endswith("cell-0.8"):
            # the minimiser sits in the named cell of the first scan, on the named side of its middle
            pos = (th_star - bounds[0]) / ((bounds[1] - bounds[0]) / 63.0)
            place = float(name[-3:])
            assert pos == pytest.approx(place if name.startswith("first") else 63.0 - place, abs=1e-6), name
        if name.endswith("cell-0.8"):
            # nearest candidate 1 / 62: one level closes with the parabola through the candidate on the bound
            th1 = orc.theta_fit_normal_eq(G, b, yy, case.t_r, case.dur, bounds, n_refine=1, **kw)[0]
            assert th1 == pytest.approx(th_star, abs=cases.HOST_THETA_TOL[1]), name
    for n_refine in cases.N_REFINE:
        th = orc.theta_fit_normal_eq(G, b, yy, case.t_r, case.dur, case.bounds, n_refine=n_refine, **kw)[0]
        print("%s n_refine %d: |restated - mp| = %.2e" % (case.name, n_refine, abs(th - th_star)))
        assert th == pytest.approx(th_star, abs=cases.HOST_THETA_TOL[n_refine]), n_refine
        assert 2 * cases.HOST_THETA_TOL[n_refine] <= cases.THETA_TOL[n_refine]


def test_tiny_dilation_leaves_tap_one_at_or_below_every_location():
    for model, taps in cases.HRF_BATCH_TAPS.items():
        for K in taps:
            t_r, dur = cases.TAPS[K] if K in cases.TAPS else cases.POW_TAPS
            t = cases.sample_times(t_r, dur)
            _, loc1, _, loc2, _ = cases.model_doubles(model)
            assert cases.TINY_DELTA * t[1] <= min(loc1, loc2)
            h = cases.ref_hrf(cases.TINY_DELTA, t, model)
            assert h[0] == 0.0 and h[1] == 0.0
            d = cases.hrf_batch_deltas(model, K)
            assert d.shape == cases.HRF_BATCH_SHAPE and d[1, 2] == cases.TINY_DELTA
