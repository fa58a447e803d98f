"""Golden fixture ``theta_models.npz``: the cases of tests/theta_model_cases.py with a high-precision minimiser.

    python tests/golden/make_golden_theta_models.py

CPU only; needs ``mpmath`` (50 digits here).  The tests that read the fixture need ``numpy`` / ``scipy`` alone.

For every case of ``theta_model_cases.CASES`` the script draws ``(W, Y)`` (``cases.draw``; ``Z = cumsum(W)`` is exact),
forms the normal equations ``G, b, yy`` of ``0.5 sum_v ||y_v - h * z_v||^2`` in mp and minimises

    F(theta) = 0.5 yy - h(theta)^T b + 0.5 h(theta)^T G h(theta)

over the case's bounds: a float64 scan of 2 601 dilations brackets the minimum, a golden-section search in mp closes the
bracket to 1e-20.  ``h(theta)`` is the two-gamma model at the float64 shapes, locations and sample times the library
receives (``cases.model_doubles``, ``cases.sample_times``), each density ``exp((a-1) log v - v - loggamma a)`` in mp.

Keys, ``<case>/`` in front of each:
  W, Y (3, N)     the innovation and the series (float32 values in float64)
  model (5,)      a_peak, loc_peak, a_under, loc_under, ratio;  t_r, dur, bounds (2,), seed_bump
  theta_star      the minimiser, rounded to float64 (a K = 1 case has h == 0: the lower bound)
  F_star, h_star (K,), gram_star    F, h and ||A^T A||_F (A = toeplitz(h) tril(1) on N scans) at that float64 dilation
  n_minima        local minima of F on the 2 601-point scan
  h_gap           max |scipy h - mp h| at theta_star
  restated_gap    |theta of orc.theta_fit_normal_eq(schedule="kernel", n_refine=3) - theta_star|

Conditions asserted before anything is written (a case that misses one is redrawn with the next ``seed_bump``):
one local minimum on the scan; ``F_star >= 1e-3 * 0.5 yy``; the minimiser at least two first-scan cells from either
bound; for the K = 27 problems of the bracket cases a minimiser that leaves room for the edge brackets inside
(0.6, 1.9); for the ``pow`` models an undershoot of at least 10 % of max|h| inside the window at every dilation of the
bounds; the restated algorithm within 1e-8 of the minimiser.
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import theta_model_cases as cases  # noqa: E402
from oracle import pybold_oracle as orc  # noqa: E402

mp.mp.dps = 50
N_SCAN = 2601
MAX_BUMPS = 40


def mp_hrf(theta, t_mp, model):
    a1, loc1, a2, loc2, ratio = [mp.mpf(x) for x in cases.model_doubles(model)]

    def pdf(x, a, loc, lg):
        v = x - loc
        return mp.mpf(0) if v <= 0 else mp.exp((a - 1) * mp.log(v) - v - lg)
    lg1, lg2 = mp.loggamma(a1), mp.loggamma(a2)
    return [pdf(theta * t, a1, loc1, lg1) - ratio * pdf(theta * t, a2, loc2, lg2) for t in t_mp]


def mp_normal_eq(Z, Y, K):
    """G (K x K nested lists), b, yy in mp from the Toeplitz structure: G[m][m + d] = R_d(N - 1 - m - d)."""
    V, N = Z.shape
    G = [[mp.mpf(0)] * K for _ in range(K)]
    b = [mp.mpf(0)] * K
    yy = mp.mpf(0)
    for v in range(V):
        z = [mp.mpf(float(x)) for x in Z[v]]
        y = [mp.mpf(float(x)) for x in Y[v]]
        yy += mp.fsum(x * x for x in y)
        for m in range(min(K, N)):
            b[m] += mp.fsum(z[i - m] * y[i] for i in range(m, N))
        for d in range(min(K, N)):
            run = mp.mpf(0)
            at = {}
            for j in range(N - d):
                run += z[j] * z[j + d]
                at[j] = run
            for m in range(K - d):
                T = N - 1 - m - d
                if T >= 0:
                    G[m][m + d] += at[T]
                    if d:
                        G[m + d][m] += at[T]
    return G, b, yy


def mp_cost(h, G, b, yy):
    K = len(h)
    Gh = [mp.fsum(G[m][k] * h[k] for k in range(K)) for m in range(K)]
    return yy / 2 - mp.fsum(h[m] * b[m] for m in range(K)) + mp.fsum(h[m] * Gh[m] for m in range(K)) / 2


def mp_gram(h, N):
    """||A^T A||_F, A = toeplitz(h, N, N) tril(1): (A^T A)[j, j + d] = R_d(N - 1 - j - d) of c = cumsum(h)."""
    K = len(h)
    c, run = [], mp.mpf(0)
    for i in range(N):
        if i < K:
            run += h[i]
        c.append(run)
    tot = mp.mpf(0)
    for d in range(N):
        r, acc = mp.mpf(0), mp.mpf(0)
        for t in range(N - d):
            r += c[t] * c[t + d]
            acc += r * r
        tot += (1 if d == 0 else 2) * acc
    return mp.sqrt(tot)


def golden_section(f, a, c, width):
    inv = (mp.sqrt(5) - 1) / 2
    x1, x2 = c - inv * (c - a), a + inv * (c - a)
    f1, f2 = f(x1), f(x2)
    while c - a > width:
        if f1 <= f2:
            c, x2, f2 = x2, x1, f1
            x1 = c - inv * (c - a)
            f1 = f(x1)
        else:
            a, x1, f1 = x1, x2, f2
            x2 = a + inv * (c - a)
            f2 = f(x2)
    return (a + c) / 2


def solve(case, bump):
    """The record of one draw, or the name of the condition it misses."""
    W, Y = cases.draw(case, bump)
    Z = np.cumsum(W, axis=1)
    K, N = case.K, case.N
    t = cases.sample_times(case.t_r, case.dur)
    assert len(t) == K, (case.name, len(t))
    t_mp = [mp.mpf(float(x)) for x in t]
    G, b, yy = mp_normal_eq(Z, Y, K)
    Gf, bf, yyf = orc.hrf_normal_eq(Z, Y, K)
    assert np.allclose(Gf, np.array([[float(x) for x in row] for row in G]), rtol=1e-12, atol=1e-12 * np.abs(Gf).max())
    assert np.allclose(bf, [float(x) for x in b], rtol=1e-10, atol=1e-12 * np.abs(bf).max())
    lo, hi = case.bounds
    rec = {"W": W, "Y": Y, "model": np.array(cases.model_doubles(case.model)), "t_r": case.t_r, "dur": case.dur,
           "bounds": np.array(case.bounds), "seed_bump": bump}
    if case.kind == "constant":
        assert K == 1 and t[0] == 0.0
        theta_star, n_min, restated_gap = lo, 1, 0.0
    else:
        grid = np.linspace(lo, hi, N_SCAN)
        f = np.array([cases.quad_cost(cases.ref_hrf(th, t, case.model), Gf, bf, yyf) for th in grid])
        n_min = cases.count_local_minima(f)
        if n_min != 1:
            return "%d local minima" % n_min
        m = int(np.argmin(f))
        cell = (hi - lo) / 63.0
        if not (lo + 2 * cell <= grid[m] <= hi - 2 * cell):
            return "minimiser %.4f within two cells of a bound" % grid[m]
        a, c = mp.mpf(float(grid[max(m - 1, 0)])), mp.mpf(float(grid[min(m + 1, N_SCAN - 1)]))
        theta_star = float(golden_section(lambda th: mp_cost(mp_hrf(th, t_mp, case.model), G, b, yy), a, c, mp.mpf(10) ** -20))
        if case in cases.BRACKET_CASES:
            for _, bnd, kind in cases.bracket_variants(theta_star):
                if not (cases.BOUNDS[0] <= bnd[0] <= bnd[1] <= cases.BOUNDS[1]):
                    return "bracket %s leaves (0.6, 1.9)" % (bnd,)
        if case.model in cases.POW_MODELS:
            share = min(cases.undershoot_share(th, t, case.model) for th in grid[::10])
            if share < 0.1:
                return "undershoot share %.3f" % share
        th_o = orc.theta_fit_normal_eq(Gf, bf, yyf, case.t_r, case.dur, case.bounds, n_refine=3, schedule="kernel",
                                       **cases.MODELS[case.model])[0]
        restated_gap = abs(th_o - theta_star)
        if restated_gap > 1e-8:
            return "restated algorithm %.3e from the minimiser" % restated_gap
    h_star = mp_hrf(mp.mpf(theta_star), t_mp, case.model)
    F_star = mp_cost(h_star, G, b, yy)
    if case.kind != "constant" and F_star < mp.mpf("1e-3") * yy / 2:
        return "F_star / (0.5 yy) = %.3e" % float(F_star / (yy / 2))
    h64 = np.array([float(x) for x in h_star])
    h_gap = max(abs(float(mp.mpf(float(s)) - x)) for s, x in zip(cases.ref_hrf(theta_star, t, case.model), h_star))
    gram = float(mp_gram(h_star, N))
    rec.update({"theta_star": theta_star, "F_star": float(F_star), "h_star": h64, "gram_star": gram, "n_minima": n_min,
                "h_gap": h_gap, "restated_gap": restated_gap})
    return rec


def main():
    out = {}
    for case in cases.CASES:
        for bump in range(MAX_BUMPS):
            rec = solve(case, bump)
            if isinstance(rec, dict):
                break
            print("  %-24s seed_bump %d: %s -- redrawn" % (case.name, bump, rec), flush=True)
        else:
            raise AssertionError("%s: no draw meets the conditions" % case.name)
        print("%-24s K %3d N %3d theta* %.12f |restated - mp| %.2e |scipy h - mp h| %.2e minima %d F*/(yy/2) %.3f"
              % (case.name, case.K, case.N, rec["theta_star"], rec["restated_gap"], rec["h_gap"], rec["n_minima"],
                 rec["F_star"] / (0.5 * float(np.sum(rec["Y"] ** 2)))), flush=True)
        for k, v in rec.items():
            out["%s/%s" % (case.name, k)] = np.asarray(v)
    np.savez_compressed(os.path.join(HERE, "theta_models.npz"), **out)
    print("theta_models.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(os.path.join(HERE, "theta_models.npz"))))


if __name__ == "__main__":
    main()
