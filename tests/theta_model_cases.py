"""The case table of the theta-step and HRF-model tests (tests/golden/make_golden_theta_models.py,
tests/test_theta_models_host.py, tests/test_gpu_theta_models.py): HRF models that reach each of the three code paths of
`spm_hrf_value` / `gamma_pdf` (csrc/blind.h), tap counts around the ways `theta_fit_kernel` deals its work, brackets at
the edges of its section search, and the layouts of the normal-equation sets.

A case is one small problem -- 3 voxels of N scans, `Z = cumsum(W)` of a sparse innovation on a 2^-6 grid (so that every
summation order gives the same Z), `Y = h(theta_0) * Z` + white noise at 10 % of the signal norm, rounded through
float32 (so that the float32 and float64 entry points see the same series).  The data, the high-precision minimiser and
its values live in tests/golden/theta_models.npz; the conditions every case must meet are asserted by the generator and,
for the float64 oracle alone, by tests/test_theta_models_host.py.

A plain helper module: no fixtures, no pytest configuration.  Nothing here touches the library under test."""
import collections

import numpy as np
from scipy.stats import gamma

DT = 0.001

# ---- HRF models: (p_delay, p_disp, undershoot, u_disp, p_u_ratio); shapes a = delay / disp, locations dt / disp -------
MODELS = collections.OrderedDict([
    ("default", dict(p_delay=6, p_disp=1.0, undershoot=16.0, u_disp=1.0, p_u_ratio=0.167)),          # fused path (control)
    ("int_locs_differ", dict(p_delay=6, p_disp=1.5, undershoot=16.0, u_disp=2.0, p_u_ratio=0.167)),  # a = 4, 8: a power each
    ("nonint", dict(p_delay=5.5, p_disp=1.0, undershoot=14.5, u_disp=1.0, p_u_ratio=0.25)),          # exp/log twice
    ("mixed", dict(p_delay=6, p_disp=1.0, undershoot=16.0, u_disp=1.3, p_u_ratio=0.167)),            # a power and an exp/log
    ("a_is_1", dict(p_delay=1, p_disp=1.0, undershoot=16.0, u_disp=1.0, p_u_ratio=0.1)),             # power 0
    ("pow64", dict(p_delay=6, p_disp=1.0, undershoot=65.0, u_disp=1.0, p_u_ratio=0.5)),              # the last integer power
    ("pow65", dict(p_delay=6, p_disp=1.0, undershoot=66.0, u_disp=1.0, p_u_ratio=0.5)),              # the first sent to exp/log
])
GENERAL_MODELS = ("default", "int_locs_differ", "nonint", "mixed", "a_is_1")
WIDE_K_MODELS = ("default", "nonint", "int_locs_differ")
POW_MODELS = ("pow64", "pow65")
INT_POWER_MAX = 64                                   # hrf_int_power (csrc/blind.h): integer a - 1 up to here


def model_path(name):
    """Which path `spm_hrf_value` takes: "fused", or one of "int" / "explog" per density."""
    m = MODELS[name]
    a = (m["p_delay"] / m["p_disp"], m["undershoot"] / m["u_disp"])
    kind = ["int" if (e >= 0.0 and e <= INT_POWER_MAX and e == int(e)) else "explog" for e in (a[0] - 1.0, a[1] - 1.0)]
    if kind == ["int", "int"] and DT / m["p_disp"] == DT / m["u_disp"]:
        return "fused"
    return "+".join(kind)


# ---- tap counts: (t_r, dur) -> K through hrf_sample_times -------------------------------------------------------------
TAPS = collections.OrderedDict([(1, (1.0, 1.0)), (3, (2.0, 6.0)), (16, (1.0, 16.0)), (17, (1.0, 17.0)), (27, (0.75, 20.0)),
                                (42, (0.72, 30.0)), (60, (0.5, 30.0)), (127, (0.25, 31.75))])
POW_TAPS = (2.0, 60.0)                               # K = 30
K_TOO_MANY = (0.25, 32.0)                            # K = 128: refused
K_MAX = 127
N_VOX = 3
BOUNDS = (0.6, 1.9)
# The undershoot of the pow models peaks at x = a - 1 = 64, 65: for the window theta * t <= theta * 58 to hold it at
# EVERY theta of the bracket (the generator asserts a share of 10 % of max|h|) the bracket starts where 58 theta
# reaches the peak's flank
POW_BOUNDS = (1.1, 1.9)
THETA_0 = {1: 1.0, 3: 1.15, 16: 1.1, 17: 0.95, 27: 1.2, 30: 1.45, 42: 1.3, 60: 1.0, 127: 1.25}
NOISE_SHARE = 0.10
LBDA = 0.7                                           # of the jcost check of theta_fit_step
N_REFINE = (1, 2, 3, 5)
THETA_TOL = {1: 2e-3, 2: 2e-6, 3: 2e-7, 4: 2e-7, 5: 2e-7}        # device vs the high-precision minimiser
HOST_THETA_TOL = {1: 1e-3, 2: 1e-6, 3: 1e-8, 5: 1e-7}             # the restated algorithm vs the same (float64 NumPy alone)
BRACKET_MODELS = ("default", "nonint")
EDGE_WIDTH = 0.441                                   # bracket of the first-cell / last-cell cases: cells of 0.007
EDGE_PLACES = (0.3, 0.8)                             # the minimiser's place inside the edge cell, in cells from the bound


def sample_times(t_r, dur, dt=DT):
    """hrf_sample_times of pybold_amd/solver.py restated (the library is not imported here)."""
    return np.ascontiguousarray(np.linspace(0, dur, int(float(dur) / dt))[::int(t_r / dt)])


def n_scans(K):
    return max(K + 8, 40)


Case = collections.namedtuple("Case", "name model t_r dur K N bounds theta_0 kind")
# kind: "interior" (a minimiser inside the bracket), "constant" (K = 1: h == 0), "short" (N < K: theta_fit only),
# "square" (N == K)


def _cases():
    out = []
    for K, (t_r, dur) in TAPS.items():
        models = GENERAL_MODELS if K in (3, 17, 27) else WIDE_K_MODELS
        for m in models:
            out.append(Case("%s-K%d" % (m, K), m, t_r, dur, K, n_scans(K), BOUNDS, THETA_0[K],
                            "constant" if K == 1 else "interior"))
    for m in POW_MODELS:
        out.append(Case("%s-K30" % m, m, POW_TAPS[0], POW_TAPS[1], 30, n_scans(30), POW_BOUNDS, THETA_0[30], "interior"))
    t_r, dur = TAPS[27]
    out.append(Case("default-K27-N20", "default", t_r, dur, 27, 20, BOUNDS, THETA_0[27], "short"))
    out.append(Case("nonint-K27-N27", "nonint", t_r, dur, 27, 27, BOUNDS, THETA_0[27], "square"))
    return out


CASES = _cases()
BY_NAME = collections.OrderedDict((c.name, c) for c in CASES)
FITTED = [c for c in CASES if c.kind != "constant"]             # cases with a minimiser to find
STEP_CASES = [c for c in CASES if c.N >= c.K]                   # pb_theta_fit_step takes N >= K
BRACKET_CASES = [BY_NAME["%s-K27" % m] for m in BRACKET_MODELS]


def case_seed(case, bump=0):
    return 104729 * list(MODELS).index(case.model) + 7919 * case.K + 31 * case.N + bump


def draw(case, bump=0):
    """`(W, Y)` of a case, float64 (3, N); Y holds float32 values.  The HRF of the signal comes from :func:`ref_hrf`."""
    rng = np.random.RandomState(case_seed(case, bump))
    V, N = N_VOX, case.N
    W = np.round(64.0 * (rng.rand(V, N) < 0.15) * rng.randn(V, N)) / 64.0
    W[:, 0] = np.round(64.0 * rng.randn(V)) / 64.0               # no all-zero series
    Z = np.cumsum(W, axis=1)
    h = ref_hrf(case.theta_0, sample_times(case.t_r, case.dur), case.model)
    X = np.stack([np.convolve(h, z)[:N] for z in Z])
    E = rng.randn(V, N)
    scale = NOISE_SHARE * np.linalg.norm(X) / np.linalg.norm(E) if np.linalg.norm(X) > 0 else 1.0
    Y = (X + scale * E).astype(np.float32).astype(np.float64)
    return W, Y


def model_doubles(name, dt=DT):
    """`(a1, loc1, a2, loc2, ratio)` as the wrappers of pybold_amd/solver.py hand them to the library."""
    m = MODELS[name]
    return (m["p_delay"] / m["p_disp"], dt / m["p_disp"], m["undershoot"] / m["u_disp"], dt / m["u_disp"], m["p_u_ratio"])


def ref_hrf(delta, t, model):
    """The un-normalised two-gamma HRF at the sample times `t`, float64 scipy: what `orc.spm_hrf(delta, t_r, dur, False,
    **MODELS[model])[0]` computes (tests/test_theta_models_host.py asserts bit equality), without its range check on
    `delta` and without building the fine grid."""
    a1, loc1, a2, loc2, ratio = model_doubles(model)
    ts = float(delta) * np.asarray(t, dtype=np.float64)
    return gamma.pdf(ts, a1, loc=loc1) - ratio * gamma.pdf(ts, a2, loc=loc2)


def undershoot_share(delta, t, model):
    """max |ratio * undershoot density| / max |h| over the window at one dilation."""
    a1, loc1, a2, loc2, ratio = model_doubles(model)
    ts = float(delta) * np.asarray(t, dtype=np.float64)
    return float(np.abs(ratio * gamma.pdf(ts, a2, loc=loc2)).max() / np.abs(ref_hrf(delta, t, model)).max())


def pack_normal_eq(G, b, yy):
    return np.concatenate([np.asarray(G).ravel(), np.asarray(b), [yy]])


def quad_cost(h, G, b, yy):
    return 0.5 * yy - h.dot(b) + 0.5 * h.dot(G.dot(h))


def direct_cost(h, Z, Y):
    """`0.5 sum_v || y_v - h * z_v ||^2`: the cost without the normal equations."""
    N = Z.shape[1]
    return float(sum(0.5 * np.sum(np.square(y - np.convolve(h, z)[:N])) for z, y in zip(Z, Y)))


def count_local_minima(f):
    """Local minima of a sampled function, plateaus counted once, the ends included."""
    f = np.asarray(f, dtype=np.float64)
    keep = np.concatenate([[True], f[1:] != f[:-1]])
    g = f[keep]
    if len(g) == 1:
        return 1
    left = np.concatenate([[True], g[1:] < g[:-1]])
    right = np.concatenate([g[:-1] < g[1:], [True]])
    return int(np.sum(left & right))


def edge_bounds(theta_star, side, place):
    """A bracket of EDGE_WIDTH with `theta_star` inside its first (`side` = "first") or last 64-grid cell, `place` cells
    from that bound."""
    cell = EDGE_WIDTH / 63.0
    if side == "first":
        lo = theta_star - place * cell
        return (lo, lo + EDGE_WIDTH)
    hi = theta_star + place * cell
    return (hi - EDGE_WIDTH, hi)


def bracket_variants(theta_star):
    """`(name, bounds, kind)` of the bracket cases of one K = 27 problem; kind "interior": the minimiser is inside,
    "lo" / "hi": the bound is the answer, "point": lo == hi."""
    out = [("full", BOUNDS, "interior"),
           ("min-on-lo", (theta_star + 0.05, BOUNDS[1]), "lo"),
           ("min-on-hi", (BOUNDS[0], theta_star - 0.05), "hi")]
    for side in ("first", "last"):
        for place in EDGE_PLACES:
            out.append(("%s-cell-%.1f" % (side, place), edge_bounds(theta_star, side, place), "interior"))
    out.append(("lo-eq-hi", (1.0, 1.0), "point"))
    return out


BRACKET_NAMES = [v[0] for v in bracket_variants(1.2)]

# ---- spm_hrf_batch: deltas (C, V), C V K no multiple of 256; the last delta leaves tap 1 at or below every location ---
HRF_BATCH_SHAPE = (3, 5)
HRF_BATCH_TAPS = {m: ((3, 17, 27) if m in GENERAL_MODELS else (30,)) for m in MODELS}
TINY_DELTA = 1.0e-4                                  # TINY_DELTA * t[1] <= 0.0005 = the smallest location, for t_r <= 2


def hrf_batch_deltas(model, K):
    rng = np.random.RandomState(17 + 31 * K + list(MODELS).index(model))
    d = rng.uniform(0.6, 1.9, size=HRF_BATCH_SHAPE)
    d[0, 0], d[-1, -1] = 0.6, 1.9
    d[1, 2] = TINY_DELTA
    return d
