"""The device-resident lambda searches as test data (tests/test_search_cases_host.py, tests/test_gpu_search_entries.py):
`auto_lbda_kernel` and its four-wave, 48-tap and one-HRF-per-voxel kin are compiled once per line of exact_table.inc,
exact_split_table.inc, exact_long_table.inc and exact_split_long_table.inc, with the taps on the host and with one HRF per
voxel ("pp"), each with STOP == 2 and STOP == 0, behind the eight `solver.auto_lbda_solve*` entry points.  This module

  * lists the instances and their edge shapes (`instances`, `shapes`, `cases`): the last length of an instance (no sample of
    the last strip masked) and its first (one sample in the last strip or wave; five scans, the shortest series
    mad_daub_noise_est accepts, on the first one-wave instance), with one tap, all the taps of the instance and, on the
    48-tap forms, 33;
  * draws the rows of a case (`case`): block signals plus noise at different scales and noise levels, one row whose lambda
    goes negative, redrawn until every stop decision of the search is taken somewhere and none of them is close to the
    tolerance, and the two float64 oracles agree on it (`check`);
  * restates `orc.deconv_auto_lbda` / `orc._inner_fista` in float64, line for line (`search`), with a warm start, the sum of
    inner iterations, the alpha trajectory and every criterion value that is compared with the tolerance.

A plain helper module: no fixtures, no pytest configuration.  Nothing here touches the library under test."""
import collections
import functools

import numpy as np

import table_shapes as ts
from oracle import c_oracle
from oracle import pybold_oracle as orc

WIND = 6
MIN_SCANS = 5                                       # the shortest series mad_daub_noise_est accepts
ALPHA_MIN = 1.0e-2                                  # tests/test_auto_lbda_host.py: the ground of the 1e-9 bound
CLEAR = 1.0e-4                                      # every criterion stays this far (x tol) from tol
ORACLES = 1.0e-12                                   # the two float64 oracles agree this closely on every row that is kept: a row
                                                    # on which they do not (alpha passing close to 0) is no ground for a 1e-9 bound
REDRAWS = 20

# budget -> (nb_iter, nb_sub_iter, tol, early_stopping)
BUDGETS = collections.OrderedDict((("FIRE", (40, 30, 1.0e-1, True)), ("QUIET", (12, 20, 1.0e-6, True)),
                                   ("OFF", (8, 40, 1.0e-6, False))))

Form = collections.namedtuple("Form", "name table entry entry_pp supported short")
# `short`: the 32-tap form of the same lengths, whose bits a 48-tap form promises for K <= 32
FORMS = collections.OrderedDict((f.name, f) for f in (
    Form("one_wave", "exact", "auto_lbda_solve", "auto_lbda_solve_pp", "pb_auto_lbda_supported", None),
    Form("four_waves", "exact_split", "auto_lbda_solve_split", "auto_lbda_solve_split_pp", "pb_auto_lbda_split_supported", None),
    Form("long", "exact_long", "auto_lbda_solve_long", "auto_lbda_solve_long_pp", "pb_auto_lbda_long_supported", "one_wave"),
    Form("four_waves_long", "exact_split_long", "auto_lbda_solve_split_long", "auto_lbda_solve_split_long_pp",
         "pb_auto_lbda_split_long_supported", "four_waves")))
ONE_WAVE_OF = {"four_waves": "one_wave", "four_waves_long": "long"}      # the form that serves the lengths below a four-wave form

Case = collections.namedtuple("Case", "form pp entry corner N K")


def four_waves(form):
    return form in ONE_WAVE_OF


def n_rows(form):
    """Six rows on the one-wave forms (four voxels per workgroup: the second workgroup is half empty), three on the others."""
    return 3 if four_waves(form) else 6


def first_length(form):
    """The first length a form serves: five scans, or one past the last length of the one-wave form below it."""
    if not four_waves(form):
        return MIN_SCANS
    below = FORMS[ONE_WAVE_OF[form]].table
    return ts.per_lane(below) * max(s for s, _ in ts.entries(below)) + 1


@functools.lru_cache(maxsize=None)
def instances(form):
    """[(entry, first length, last length)] of a form, by S: an instance (S, KT) serves the lengths from the previous
    instance's last + 1 (or the form's first) to S x the scans per unit of S."""
    table = FORMS[form].table
    out, first = [], first_length(form)
    for entry in sorted(ts.entries(table)):
        last = entry[0] * ts.per_lane(table)
        out.append((entry, first, last))
        first = last + 1
    return tuple(out)


def shapes(form):
    """[(entry, corner, N, K)]: the full and the masked corner of every instance; K = 1, KT and, on the 48-tap forms, 33."""
    out = []
    for entry, first, last in instances(form):
        taps = sorted({1, entry[1]} | ({33} if entry[1] > 33 else set()))
        out += [(entry, corner, n, k) for corner, n in (("full", last), ("masked", first)) for k in taps]
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(Case(form, pp, entry, corner, N, K) for form in FORMS for pp in (False, True)
                 for entry, corner, N, K in shapes(form))


def case_id(c, budget=None):
    f = FORMS[c.form]
    name = "%s-%s_%d_%d-%s_%dx%d" % (f.entry_pp if c.pp else f.entry, f.table, c.entry[0], c.entry[1], c.corner, c.N, c.K)
    return name if budget is None else name + "-" + budget


# ---- the reference: orc.deconv_auto_lbda / orc._inner_fista restated ------------------------------------------------------
class _H:
    def __init__(self, kernel):
        self.k = np.asarray(kernel, dtype=np.float64)

    def op(self, x):
        return orc.causal_conv(self.k, orc.integ_op(x))

    def adj(self, r):
        return orc.integ_adj(orc.causal_corr(self.k, r))


def _inner(w, H, H_adj_y, step, th, nb_sub_iter, early_stopping, wind, tol, crit):
    """orc._inner_fista; returns (w, inner iterations run) and appends every window criterion it compares with tol."""
    hist = []
    t_old = 1.0
    n = 0
    for j in range(nb_sub_iter):
        u = w - step * (H.adj(H.op(w)) - H_adj_y)
        if j > 0 and hist:
            hist[-1] = u
        prev = u if j > 0 else 0.0
        p = orc.soft_threshold(u, th)
        t = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t_old ** 2))
        w = p + (t_old - 1.0) / t * (p - prev)
        t_old = t
        hist.append(w)
        if len(hist) > wind:
            hist = hist[1:]
        n = j + 1
        if early_stopping and j > wind:
            half = int(wind / 2)
            old = np.mean(hist[:-half], axis=0)
            new = np.mean(hist[-half:], axis=0)
            c = np.linalg.norm(new - old) / (np.linalg.norm(new) + 1.0e-10)
            crit.append(c)
            if c < tol:
                break
    return w, n


Run = collections.namedtuple("Run", "W R G J alpha lbda n_outer n_inner crit_alpha crit_inner")


def search(y, hrf, sigma, lipschitz, early_stopping=True, tol=1.0e-6, wind=WIND, nb_iter=1000, nb_sub_iter=1000, w0=None):
    """orc.deconv_auto_lbda with an optional warm start `w0`.  Returns Run(W, R, G, J (n_outer,), alpha (n_outer,): the
    trajectory, lbda: the last one, n_outer, n_inner: inner iterations summed over every inner solve, the last one included,
    crit_alpha / crit_inner: every value of the alpha window's / the inner window rule's criterion that was compared with tol)."""
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    hrf = np.asarray(hrf, dtype=np.float64)
    H = _H(hrf)
    H_adj_y = H.adj(y)
    step = 1.0 / lipschitz
    w = np.zeros(n) if w0 is None else np.array(w0, dtype=np.float64)
    alpha, mu = 1.0, 1.0e-4
    lbda = 1.0 / (2.0 * alpha)
    l_alpha, alphas, J, R, G = [], [], [], [], []
    crit_alpha, crit_inner = [], []
    n_inner = 0
    for i in range(nb_iter):
        w, it = _inner(w, H, H_adj_y, step, lbda / lipschitz, nb_sub_iter, early_stopping, wind, tol, crit_inner)
        n_inner += it
        z = np.cumsum(w)
        x = orc.causal_conv(hrf, z)
        grad = np.sum(np.square(x - y)) - n * sigma ** 2
        alpha += mu * grad
        lbda = 1.0 / (2.0 * alpha)
        l_alpha.append(alpha)
        alphas.append(alpha)
        if len(l_alpha) > wind:
            l_alpha = l_alpha[1:]
        r = np.sum(np.square(x - y))
        g = np.sum(np.abs(w))
        R.append(r)
        G.append(g)
        J.append(0.5 * r + lbda * g)
        if early_stopping and i > wind:
            half = int(wind / 2)
            old = np.mean(l_alpha[:-half])
            new = np.mean(l_alpha[-half:])
            c = np.abs(new - old) / np.abs(new)
            crit_alpha.append(c)
            if c < tol:
                break
    w, it = _inner(w, H, H_adj_y, step, lbda / lipschitz, nb_sub_iter, early_stopping, wind, tol, crit_inner)
    n_inner += it
    out = Run(w, np.array(R), np.array(G), np.array(J), np.array(alphas), float(lbda), len(J), n_inner, np.array(crit_alpha),
              np.array(crit_inner))
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def run_budget(y, hrf, sigma, lipschitz, budget, w0=None):
    nb_iter, nb_sub_iter, tol, early = BUDGETS[budget]
    return search(y, hrf, sigma, lipschitz, early_stopping=early, tol=tol, nb_iter=nb_iter, nb_sub_iter=nb_sub_iter, w0=w0)


# ---- the rows of a case ------------------------------------------------------------------------------------------------------
SCALES = (1.0, 1.5, 2.0, 3.0, 0.7)


def _rng(c, *more):
    return np.random.default_rng((c.N, c.K, list(FORMS).index(c.form), int(c.pp)) + tuple(int(m) for m in more))


def _short(c):
    """The short masked corner: the first five taps of the spm HRFs give a zero response there."""
    return c.corner == "masked" and not four_waves(c.form) and c.entry == instances(c.form)[0][0]


@functools.lru_cache(maxsize=None)
def _operator(c, N):
    """`(base HRF (K,), its Lipschitz constant at N scans)`: [1.0] at K = 1, else the spm HRF of the existing shape tests --
    or, at the short corner, 0.3 randn(K) taps as tests/test_gpu_table_entries.py draws them."""
    if c.K == 1:
        hrf = np.array([1.0])
    elif _short(c):
        hrf = 0.3 * _rng(c, 0).standard_normal(c.K)
    else:
        hrf = orc.spm_hrf(1.0, t_r=30.0 / c.K, dur=30.0, normalized_hrf=False)[0][:c.K]
    assert len(hrf) == c.K
    hrf.setflags(write=False)
    return hrf, ts.lipschitz(hrf, N)


def _block_signal(n, hrf, rng):
    """tests/test_gpu_auto_lbda_device.py: blocks of random height under the HRF plus noise at 0.4 of its standard deviation."""
    z = np.zeros(n)
    for start in range(3, n, max(n // 6, 8)):
        z[start:start + max(n // 14, 3)] = rng.uniform(0.5, 1.5)
    x = orc.causal_conv(hrf, z)
    return x + 0.4 * np.std(x) * rng.standard_normal(n)


def _draw(c, N, v, attempt, negative):
    """Row v of a case, draw number `attempt`: `(y, sigma)`.  The first draw takes the scale and the noise factor from a
    fixed ladder (scales 1, 1.5, 2, 3, 0.7; sigma = 0.5 .. 2 x the estimated noise level), a redraw draws both; the
    negative-lambda row is scaled to 10 standard deviations and searched at 3 x its estimated noise level."""
    rng = _rng(c, N, 1 + v, attempt)
    s = _block_signal(N, _operator(c, N)[0], rng)
    if negative:
        y = 10.0 * s / np.std(s)
        return y, 3.0 * orc.mad_daub_noise_est(y)
    regular = n_rows(c.form) - 1
    if attempt == 0:
        scale, factor = SCALES[v % len(SCALES)], 0.5 + 1.5 * v / max(regular - 1, 1)
    else:
        scale, factor = 10.0 ** rng.uniform(-0.3, 1.5 if _short(c) else 0.7), rng.uniform(0.5, 2.0)
    y = scale * s
    return y, factor * orc.mad_daub_noise_est(y)


def _row_taps(c, N, V):
    """hrf (K,) and the Lipschitz constant (host taps), or taps (V, K) and one constant per row (pp: the base HRF under a
    gain and a sign per row, exact steps)."""
    hrf, lip = _operator(c, N)
    if not c.pp:
        return hrf, np.full(V, lip)
    taps, steps = ts.scaled_taps(hrf, lip, V)
    return taps, 1.0 / steps


def clearance(run, tol):
    """The smallest distance, in units of tol, of any criterion the run compared with tol."""
    crit = np.concatenate([run.crit_alpha, run.crit_inner])
    return float(np.abs(crit - tol).min() / tol) if crit.size else np.inf


def c_oracle_distance(y, hrf, sigma, lipschitz, budget, run):
    """The largest relative distance of W, R, G, J of the C oracle's search from `run` (inf: another n_outer)."""
    nb_iter, nb_sub_iter, tol, early = BUDGETS[budget]
    W, J, R, G, n = c_oracle.deconv_auto_lbda_batch(y[None, :], hrf, np.array([sigma]), float(lipschitz), early_stopping=early, tol=tol,
                                                    nb_iter=nb_iter, nb_sub_iter=nb_sub_iter, threads=1)
    if int(n[0]) != run.n_outer:
        return np.inf
    m = run.n_outer
    return max(float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))
               for a, b in ((W[0], run.W), (R[0, :m], run.R), (G[0, :m], run.G), (J[0, :m], run.J)))


def row_faults(runs, negative):
    """What keeps a row from being used, as a list of words (empty: the row meets the per-row conditions).  `runs`: budget ->
    Run, and "WARM" -> the warm QUIET run at a full corner."""
    bad = []
    for name, run in runs.items():
        nb_iter, nb_sub_iter, tol, early = BUDGETS["QUIET" if name == "WARM" else name]
        if not (np.isfinite(run.alpha).all() and np.isfinite(run.W).all()):
            bad.append(name + ": not finite")
            continue
        if not np.abs(run.alpha).min() > ALPHA_MIN:
            bad.append("%s: |alpha| %.2e" % (name, np.abs(run.alpha).min()))
        if early and clearance(run, tol) < CLEAR:
            bad.append("%s: a criterion %.1e tol from tol" % (name, clearance(run, tol)))
        if name in ("QUIET", "WARM") and (run.n_outer, run.n_inner) != (nb_iter, (nb_iter + 1) * nb_sub_iter):
            bad.append("%s: stops (%d, %d)" % (name, run.n_outer, run.n_inner))
        if name == "FIRE" and not negative and not run.n_inner < (run.n_outer + 1) * nb_sub_iter:
            bad.append("FIRE: the inner rule never fires")
        if name == "FIRE" and negative and run.n_outer != nb_iter:
            bad.append("FIRE: the negative-lambda row stops at %d" % run.n_outer)
        if name in ("FIRE", "QUIET") and negative and not (run.alpha < 0).any():
            bad.append(name + ": alpha stays positive")
    return bad


def case_faults(N, fire):
    """The conditions on the rows of a case together, on their FIRE runs."""
    nb_iter = BUDGETS["FIRE"][0]
    stops = [r.n_outer for r in fire]
    fired = sorted({n for n in stops if n < nb_iter})
    bad = []
    if not fired:
        bad.append("no row fires before nb_iter")
    if nb_iter not in stops:
        bad.append("no row runs all of nb_iter")
    if N >= 320 and len(fired) < 2:
        bad.append("fewer than two distinct firing iterations: %s" % stops)
    return bad


class NoRows(Exception):
    """No draw of this shape meets the conditions of a search case."""


def _build(c, N):
    V = n_rows(c.form)
    neg = V - 1 if four_waves(c.form) else 2            # (one-wave forms: inside the first workgroup, among rows that stop earlier)
    taps, lips = _row_taps(c, N, V)
    full = c.corner == "full"
    W0 = 0.01 * _rng(c, N, 0, 7).standard_normal((V, N)) if full else None

    def evaluate(v, attempt):
        y, sigma = _draw(c, N, v, attempt, v == neg)
        hrf = taps[v] if c.pp else taps
        runs, faults = collections.OrderedDict(), []
        for name in list(BUDGETS) + (["WARM"] if full else []):              # (a draw is dropped at its first run that fails)
            warm = name == "WARM"
            runs[name] = run_budget(y, hrf, sigma, lips[v], "QUIET" if warm else name, w0=W0[v] if warm else None)
            faults = row_faults({name: runs[name]}, v == neg)
            if not faults and not warm:
                e = c_oracle_distance(y, hrf, sigma, lips[v], name, runs[name])
                faults = [] if e <= ORACLES else ["%s: %.1e from the C oracle" % (name, e)]
            if faults:
                break
        return y, sigma, runs, faults

    rows, attempts = [None] * V, [0] * V

    def redraw(v):
        """The next draw of row v that meets the per-row conditions."""
        while attempts[v] <= REDRAWS:
            y, sigma, runs, faults = evaluate(v, attempts[v])
            attempts[v] += 1
            if not faults:
                rows[v] = (y, sigma, runs)
                return
        raise NoRows("%s: row %d at %d scans: %s" % (case_id(c), v, N, faults))

    for v in range(V):
        redraw(v)
    regular = [v for v in range(V) if v != neg]
    for turn in range(REDRAWS + 1):
        faults = case_faults(N, [r[2]["FIRE"] for r in rows])
        if not faults:
            break
        if turn == REDRAWS:
            raise NoRows("%s at %d scans: %s" % (case_id(c), N, faults))
        # redraw, in turn, a regular row that shares its stop with another one: a row that stops alone is kept
        stops = [rows[v][2]["FIRE"].n_outer for v in range(V)]
        shared = [v for v in regular if stops.count(stops[v]) > 1] or regular
        redraw(shared[turn % len(shared)])
    Y, sigma = np.stack([r[0] for r in rows]), np.array([r[1] for r in rows])
    ref = collections.OrderedDict((b, tuple(r[2][b] for r in rows)) for b in list(BUDGETS) + (["WARM"] if full else []))
    steps = 1.0 / lips
    for a in (Y, sigma, taps, lips, steps) + ((W0,) if full else ()):
        a.setflags(write=False)
    return dict(case=c, N=N, K=c.K, V=V, Y=Y, sigma=sigma, taps=taps, lips=lips, steps=steps, negative=neg, W0=W0, ref=ref,
                draws=tuple(attempts))


@functools.lru_cache(maxsize=None)
def case(c):
    """The rows and references of a case: dict(N: the length used, K, V, Y (V, N), sigma (V,), taps: (K,) or, pp, (V, K),
    lips / steps (V,), negative: the negative-lambda row, W0: the warm start of the full corners, ref: budget -> one Run per
    row ("WARM": the QUIET budget from W0), draws: draws used per row).  At the short corner, where no draw of five scans
    meets the conditions, the next length of table_shapes.LADDER is taken."""
    lengths = (c.N,)
    if _short(c):
        last = [i for i in instances(c.form) if i[0] == c.entry][0][2]
        lengths += tuple(n for n in ts.LADDER if c.N < n <= last)
    why = None
    for N in lengths:
        try:
            return _build(c, N)
        except NoRows as e:
            why = why or e
    raise why


def check(data):
    """Every condition of a case on its stored references; AssertionError names the first that fails."""
    neg, ref = data["negative"], data["ref"]
    for v in range(data["V"]):
        faults = row_faults({b: ref[b][v] for b in ref}, v == neg)
        assert not faults, (case_id(data["case"]), v, faults)
    faults = case_faults(data["N"], ref["FIRE"])
    assert not faults, (case_id(data["case"]), faults)
