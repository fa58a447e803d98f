"""The stop rules of the matrix-pipe kernels as test data (tests/test_stop_rule_cases_host.py, tests/test_gpu_mfma_stop_rules.py):
`fista_mfma_kernel`, `fista_mfma2_kernel` and `fista_mfma4_kernel` carry the _loops_deconv rule in full (LOOPS) and the window
rule (wind = 6) as a no-fire certificate (CERT), one compiled instance per block count and number of near tiles
(table_shapes.mfma_instance).  This module

  * lists the cases: every rule instance a pinned call reaches, at the corners of the region of shapes that reach it
    (`cases`; `reaches` restates the part of route() in pybold_amd/csrc/dispatch.h that `force="mfma"` / `"mfma2"` take);
  * draws the inputs of a case (`loops_inputs`, `window_inputs`): rows that stay clear of the tolerance, dense enough for the
    matrix pipe to keep them, firing at different iterations, one whole group of 16 rows firing only;
  * judges a result row by row (`judge`): the stop iteration against the oracle's criterion, the iterate against the float64
    C oracle after THAT ROW'S OWN number of iterations -- no row is left out of the comparison.

A plain helper module: no fixtures, no pytest configuration."""
import collections
import functools

import numpy as np

import table_shapes as ts

WIND = 6
N_LO, N_HI, K_HI = 129, 1280, 65        # the scans the three forms serve; the taps their pickers accept (pick_mfma2 / pick_mfma4)
V_ROWS, POOL, BUDGET = 37, 148, 120     # rows of a batch (16 + 16 + 5), rows drawn, most iterations
EPS, RTOL_J = 1.0e-5, 3.0e-5            # the project's bounds for float32-storage forms: iterate (relative row norm), cost trace
BAND = 0.01                             # table_shapes.fire_iteration: a clear row's criterion stays 1 % of tol away from tol
RHO = 0.5 * 0.02                        # MFMA_RHO_MAX of pybold_amd/csrc/mfma_core.h with a factor 2 to spare
TOL_MIN = 1.0e-3

FORMS = ("mfma", "mfma2", "mfma4")
RULES = ("loops", "window")
# form -> the pins of solver.fista_solve: (re-solve, no re-solve, certificate, certificate without re-solve)
PINS = {"mfma": ("mfma", "mfmaonly", "mfmacert", "mfmacertonly"),
        "mfma2": ("mfma2", "mfma2only", "mfma2cert", "mfma2certonly"),
        "mfma4": ("mfma2", "mfma2only", "mfma2cert", "mfma2certonly")}

Case = collections.namedtuple("Case", "form instance corner N K rule")


def case_id(c):
    return "%s-%s_%dx%d-%s" % (c.instance.replace("<", "_").replace(">", "").replace(",", "_").replace(" ", "_"), c.corner, c.N, c.K,
                               c.rule)


# ---- which shapes reach a rule instance under its pin ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vector_entries(N, K):
    return ts.pick("fast", N, K), ts.pick("wide", N, K)


def reaches(form, N, K, rule):
    """A small pinned call (`PINS[form]`, one lambda, n_done asked for, fewer than 1 024 problems) of this shape and rule runs
    the rule variant of `ts.mfma_instance(form, N, K)`.  Restates route() of dispatch.h for these pins:

    one wave (`force="mfma"`): the piece of a single-row entry's plan -- the entry must exist (none at 305..310 scans beyond
    32 taps) and, for the window rule, hold the increment ring (S <= 20) and have the pair certificate (KT <= 32) the
    matrix-pipe certificate is planned beside; `pick_mfma(.., stop_rule=true)`: two near tiles only.
    two / four waves (`force="mfma2"`): PATH_SPLIT_LONG -- `pick_mfma2` (three near tiles from 225 scans on) or
    `mfma4_serves`, and a backup form for the re-solve: the single-row entry up to 320 scans where there is one, else one
    problem per wave, with the ring for the window rule."""
    if ts.mfma_instance(form, N, K) is None:
        return False
    fe, we = _vector_entries(N, K)
    if form == "mfma":
        if K > 33 or fe is None:
            return False
        return rule == "loops" or (ts.ring_fits(fe[0], "window", WIND) and ts.has_pair(fe))
    if form == "mfma4" and we is None:
        return False
    backup = we if (we is not None and (fe is None or N > 320)) else fe
    return backup is not None and ts.ring_fits(backup[0], rule, WIND)


@functools.lru_cache(maxsize=None)
def regions():
    """{(form, instance, rule): sorted [(N, K)]} over N_LO .. N_HI scans and 1 .. K_HI taps: the shapes that reach each rule
    instance.  (The forms overlap: 129 .. 640 scans reach the two-wave form through its pin whatever the one-wave form serves.)"""
    out = collections.OrderedDict()
    for form in FORMS:
        for N in range(N_LO, N_HI + 1):
            for K in range(1, K_HI + 1):
                inst = ts.mfma_instance(form, N, K)
                if inst is None:
                    continue
                for rule in RULES:
                    if reaches(form, N, K, rule):
                        out.setdefault((form, inst, rule), []).append((N, K))
    return out


def max_taps():
    """The largest tap count a pinned rule call accepts on any form (the backup forms end it, not the pickers)."""
    return max(k for shapes in regions().values() for _, k in shapes)


def corners(shapes):
    """[(name, N, K)] of a region: `masked` -- the smallest N and the fewest taps there (the last block partly filled, or
    one sample into a new block; taps zero-padded); `full` -- the largest N and the most taps there (the last block as
    full as it gets); `taps` -- the largest N among the shapes with the most taps of the region, where that is another shape
    (regions are no rectangles: a backup form may end the taps earlier at the longest series)."""
    n_min, n_max = min(s[0] for s in shapes), max(s[0] for s in shapes)
    k_max = max(s[1] for s in shapes)
    masked = (n_min, min(s[1] for s in shapes if s[0] == n_min))
    full = (n_max, max(s[1] for s in shapes if s[0] == n_max))
    out = [("masked",) + masked, ("full",) + full]
    if full[1] < k_max:
        out.append(("taps", max(s[0] for s in shapes if s[1] == k_max), k_max))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(Case(form, inst, name, N, K, rule) for (form, inst, rule), shapes in regions().items()
                 for name, N, K in corners(shapes))


# ---- the operator as a Gram matrix: criteria of a pool of rows at the price of one matrix product per iteration ---------
@functools.lru_cache(maxsize=2)
def operator(N, K, seed=0):
    """`(taps, A, G, step)`: a random HRF of K taps (as table_shapes.stop_rule_inputs draws it), A = toeplitz(taps) . cumsum
    as an (N, N) matrix, G = A^T A and the step 1 / (1.05 ||A||_2^2 + 1e-9) of table_shapes.lipschitz."""
    rng = np.random.RandomState(3000017 * (seed + 1) + 1009 * N + K)
    taps = 0.3 * rng.randn(K)
    c = np.cumsum(taps)
    lag = np.arange(N)[:, None] - np.arange(N)[None, :]
    A = np.where(lag >= 0, c[np.clip(lag, 0, K - 1)], 0.0)
    G = A.T.dot(A)
    step = 1.0 / (1.05 * float(np.linalg.eigvalsh(G)[-1]) + 1e-9)
    for a in (taps, A, G):
        a.setflags(write=False)
    return taps, A, G, step


def criteria(Y, A, G, lbda, step, n_iter, W0=None):
    """table_shapes.trajectory with the operator as a matrix (tests/test_stop_rule_cases_host.py holds the two together):
    `(crit_loops, crit_window, wmax)`, each (V, n_iter) -- the _loops_deconv criterion of iteration j (NaN for j <= 2), the
    window criterion at wind = 6 (NaN for k <= 6), and max |w| of the iterate after iteration j."""
    from oracle import pybold_oracle as orc
    V, n = Y.shape
    th = lbda * step
    B = Y.dot(A)
    W = np.zeros((V, n)) if W0 is None else np.array(W0, dtype=np.float64)
    betas = orc.momentum_sequence(n_iter)
    crit_l, crit_w, wmax = (np.full((V, n_iter), np.nan) for _ in range(3))
    hist = []
    half = WIND // 2
    for k in range(n_iter):
        U = W - step * (W.dot(G) - B)
        if k > 0 and hist:
            hist[-1] = U                                   # (the stored alias of w_k was overwritten: deconv_fixed_lbda)
        P = orc.soft_threshold(U, th)
        W = P + betas[k] * (P - (U if k > 0 else 0.0))
        wmax[:, k] = np.abs(W).max(axis=1)
        if k > 2:
            crit_l[:, k] = np.linalg.norm(W - U, axis=1) / (np.linalg.norm(W, axis=1) + 1.0e-10)
        hist = (hist + [W])[-WIND:]
        if k > WIND:
            old, new = np.mean(hist[:-half], axis=0), np.mean(hist[-half:], axis=0)
            crit_w[:, k] = np.linalg.norm(new - old, axis=1) / (np.linalg.norm(new, axis=1) + 1.0e-10)
    return crit_l, crit_w, wmax


# ---- selection -----------------------------------------------------------------------------------------------------------
def _spread(items, n):
    """n of the sorted list `items`, evenly spaced, the first and the last among them."""
    if n >= len(items):
        return list(items)
    return [items[int(round(j * (len(items) - 1) / max(n - 1, 1)))] for j in range(n)]


def select(n_done, fired, ok, V):
    """V rows of a pool in the order of a case, or None.  `ok`: the rows that are clear and dense.  At least half of the rows
    fire, at three or more different iterations, one of them after iteration 8 (past the first periodic range check of the
    kernels); at least one never fires.  Rows 0 .. 15 fire, all of them (a whole wave / workgroup finishes early); the rows
    that never fire alternate with the other firing rows behind them, and the batch ends in a partial group."""
    assert V > 16 and V % 16 != 0
    never = [i for i in np.flatnonzero(ok) if not fired[i]]
    fire = sorted((i for i in np.flatnonzero(ok) if fired[i]), key=lambda i: (n_done[i], i))
    n_fire = min(len(fire), V - min(len(never), (V - 16) * 3 // 5))      # (12 of 37 never fire where the pool has 25 that do)
    n_never = V - n_fire
    if n_never < 1 or n_never > len(never) or 2 * n_fire < V:
        return None
    picks = _spread(fire, n_fire)
    if len(set(picks)) < n_fire:
        picks = fire[:n_fire - 1] + [fire[-1]]
    stops = {n_done[i] for i in picks}
    if len(stops) < 3 or max(stops) <= 8:
        return None
    first = _spread(picks, 16)
    if len(set(first)) < 16 or len({n_done[i] for i in first}) < 3:
        return None
    rest_fire, rest = [i for i in picks if i not in first], []
    for j in range(max(n_never, len(rest_fire))):
        rest += never[j:j + 1] if j < n_never else []
        rest += rest_fire[j:j + 1]
    return np.array(first + rest)


def check_selection(inp):
    """The conditions every case's inputs meet (asserted on the CPU: the host test, and the GPU test when it builds a case)."""
    V, n_iter, tol = len(inp["n_done"]), inp["n_iter"], inp["tol"]
    nd, fired = inp["n_done"], inp["fired"]
    assert inp["Y"].shape == (V, inp["N"]) and V % 16 != 0 and n_iter <= BUDGET and tol >= TOL_MIN
    assert inp["clear"].all() and inp["dense"].all()
    assert (fired == (nd < n_iter)).all() and 2 * fired.sum() >= V and (~fired).any()
    assert len(set(nd[fired].tolist())) >= 3 and nd[fired].max() > 8
    assert fired[:16].all(), "no whole group of 16 firing rows"
    assert (~fired[16:32]).any() and len(set(nd[:16].tolist())) >= 3


HORIZONS = (40, BUDGET)                 # iterations of the pool's trajectory: the short one first, it serves most cases


def _budgets(crit, tol, first_test):
    """Iteration budgets to try: where 40 % .. 90 % of the rows that fire within the horizon have fired, then the horizon."""
    horizon = crit.shape[1]
    n_done, fired, _ = ts.fire_iteration(crit, tol, horizon)
    out = []
    if fired.any():
        at = np.sort(n_done[fired])
        out = [int(at[min(len(at) - 1, int(q * len(at)))]) + 1 for q in (0.6, 0.75, 0.5, 0.9, 0.4)]
    seen = []
    for n in out + [horizon]:
        if first_test + 6 <= n <= horizon and n not in seen:
            seen.append(n)
    return seen


def _finish(N, K, Y, W0, taps, step, lbda, tol, n, crit, wmax, V):
    """The rows of a pool for (tol, budget n), as the dict of a case -- or None."""
    n_done, fired, clear = ts.fire_iteration(crit[:, :n], tol, n)
    dense = lbda * step <= RHO * wmax[np.arange(len(n_done)), n_done - 1]
    rows = select(n_done, fired, clear & dense, V)
    if rows is None:
        return None
    inp = dict(N=N, K=K, Y=Y[rows], taps=taps, step=step, lbda=lbda, tol=tol, n_iter=n, n_done=n_done[rows], fired=fired[rows],
               clear=clear[rows], dense=dense[rows], W0=None if W0 is None else W0[rows], crit=crit[rows, :n])
    check_selection(inp)
    return inp


def loops_inputs(N, K, V=V_ROWS, pool=POOL, seed=0):
    """Inputs of a _loops_deconv case: block signals under the HRF plus noise at -5 .. 20 dB (the batches of
    tests/test_gpu_round5.py), cold start, lambda = 0.003 .. 0.01 of the pool's median lambda_max (the rule compares
    (1 + beta) ||clamp(u, +-th)|| with ||w'||: it fires where lambda is small against the signal)."""
    taps, A, G, step = operator(N, K, seed)
    rng = np.random.RandomState(4000037 * (seed + 1) + 1009 * N + K)
    Z = np.zeros((pool, N))
    for v in range(pool):
        for _ in range(max(5, N // 60)):
            o = rng.randint(0, N - 20)
            Z[v, o:o + rng.randint(8, 16)] = 1.0
    X = ts.op_forward_rows(np.atleast_2d(taps), np.diff(Z, axis=1, prepend=0.0))
    noise = rng.randn(pool, N)
    noise *= (np.linalg.norm(X, axis=1) / np.linalg.norm(noise, axis=1) / np.sqrt(10 ** (np.linspace(-5, 20, pool) / 10)))[:, None]
    Y = (X + noise).astype(np.float32).astype(np.float64)
    lmed = float(np.median(np.abs(Y.dot(A)).max(axis=1)))
    for horizon in HORIZONS:
        for frac in (0.003, 0.006, 0.01):
            lbda = frac * lmed
            crit, _, wmax = criteria(Y, A, G, lbda, step, horizon)
            for tol in (1e-3, 2e-3, 5e-3, 1e-2):
                for n in _budgets(crit, tol, 3):
                    inp = _finish(N, K, Y, None, taps, step, lbda, tol, n, crit, wmax, V)
                    if inp is not None:
                        return dict(inp, rule="loops")
    raise ts.NoInputs("no _loops_deconv inputs for N=%d K=%d V=%d" % (N, K, V))


def window_inputs(N, K, V=V_ROWS, pool=POOL, seed=0):
    """Inputs of a window-rule case (wind = 6), as table_shapes.certificate_inputs draws them: half of the pool is warm-started
    next to its solution (200 iterations, perturbed by 1e-5 .. 1 of its size: these fire at the first tests and, the larger
    the perturbation, later), half is cold and dense (lambda_max / lambda 5 .. 100)."""
    from oracle import pybold_oracle as orc
    taps, A, G, step = operator(N, K, seed)
    rng = np.random.RandomState(5000011 * (seed + 1) + 1009 * N + K)
    lbda = 0.5
    Gs = rng.randn(pool, N)
    lmax = np.abs(Gs.dot(A)).max(axis=1)
    Y = Gs * (lbda * 10.0 ** rng.uniform(0.7, 2.0, pool) / lmax)[:, None]
    Y = Y.astype(np.float32).astype(np.float64)
    warm = np.arange(pool) % 2 == 0
    n_warm = int(warm.sum())
    th, B = lbda * step, Y[warm].dot(A)
    near = np.zeros((n_warm, N))
    for k, beta in enumerate(orc.momentum_sequence(200)):
        U = near - step * (near.dot(G) - B)
        P = orc.soft_threshold(U, th)
        near = P + beta * (P - (U if k > 0 else 0.0))
    size = np.linalg.norm(near, axis=1, keepdims=True) / np.sqrt(N)
    W0 = np.zeros((pool, N))
    W0[warm] = near + 10.0 ** rng.uniform(-5.0, 0.0, size=(n_warm, 1)) * size * rng.randn(n_warm, N)
    for horizon in HORIZONS:
        _, crit, wmax = criteria(Y, A, G, lbda, step, horizon, W0=W0)
        for tol in (0.005, 0.01, 0.02, 0.05, 0.1):
            for n in (16, 20, 24, 32, 40, 60, BUDGET):
                if n > horizon or (horizon > HORIZONS[0] and n <= HORIZONS[0]):
                    continue
                inp = _finish(N, K, Y, W0, taps, step, lbda, tol, n, crit, wmax, V)
                if inp is not None:
                    return dict(inp, rule="window")
    raise ts.NoInputs("no window-rule inputs for N=%d K=%d V=%d" % (N, K, V))


def inputs(case, V=V_ROWS, pool=POOL):
    return (loops_inputs if case.rule == "loops" else window_inputs)(case.N, case.K, V, pool)


# ---- the oracle's side of a case, and the judge --------------------------------------------------------------------------
def iterates_at(case, n_done, rows=None):
    """The float64 C oracle's iterate of every row (of `rows`) after that row's own `n_done[v]` iterations, rule off, same warm
    start."""
    from oracle import c_oracle
    rows = np.arange(len(case["Y"])) if rows is None else np.asarray(rows)
    n_done = np.asarray(n_done)[rows]
    W = np.empty((len(rows), case["Y"].shape[1]))
    for n in np.unique(n_done):
        at = rows[n_done == n]
        W0 = None if case.get("W0") is None else case["W0"][at]
        W[n_done == n] = c_oracle.fista_batch(case["Y"][at], case["taps"], case["lbda"], case["step"], int(n), W0=W0, threads=0)[0]
    return W


def trace(case):
    """The C oracle's cost trace of every row over the whole budget (computed once per case)."""
    from oracle import c_oracle
    if case.get("J") is None:
        case["J"] = c_oracle.fista_batch(case["Y"], case["taps"], case["lbda"], case["step"], case["n_iter"], W0=case.get("W0"),
                                         want_J=True, threads=0)[1]
    return case["J"]


def sweep_case(Y, taps, lbda, step, n_iter, n_done, clear=None, W0=None, W=None):
    """The dict `judge` reads, for a batch that was not selected: `n_done` the oracle's stop iterations, `clear` the rows
    known to stay clear of the tolerance (none, if not given: every row may then stop one iteration apart), `W` the float64
    oracle's iterates at ITS stop iterations where the caller has them (pybold_oracle.loops_batch; else the C oracle's are
    computed) -- a row that stops elsewhere is compared with the C oracle's iterate of its own iteration either way."""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    n_done = np.asarray(n_done, dtype=np.int64)
    return dict(N=Y.shape[1], Y=Y, taps=np.asarray(taps, dtype=np.float64), step=float(step), lbda=float(lbda), n_iter=int(n_iter),
                n_done=n_done, clear=np.zeros(len(n_done), dtype=bool) if clear is None else np.asarray(clear, dtype=bool),
                W0=None if W0 is None else np.asarray(W0, dtype=np.float64), W=None if W is None else np.asarray(W, dtype=np.float64))


Verdict = collections.namedtuple("Verdict", "err differed jerr")


def judge(case, W, n_done, J=None):
    """Every row of a result against the oracle; AssertionError names the first row that fails.

      * n_done lies in [1, n_iter]; on a clear row it equals the oracle's, on any other it is at most one apart;
      * the iterate of EVERY row is within EPS (relative row norm) of the C oracle's iterate after that row's own n_done
        iterations; where the oracle's iterate is all zero the row is all zero;
      * with a cost trace: the entries before n_done within RTOL_J of the C oracle's trace, NaN from n_done on.

    Returns Verdict(worst row error, rows whose n_done differs from the oracle's, worst trace error or None)."""
    W, n_done = np.asarray(W, dtype=np.float64), np.asarray(n_done).astype(np.int64)
    ref_nd, n_iter = case["n_done"], case["n_iter"]
    assert W.shape == case["Y"].shape and n_done.shape == ref_nd.shape
    assert ((n_done >= 1) & (n_done <= n_iter)).all(), "n_done outside [1, %d]: %s" % (n_iter, n_done.tolist())
    apart = np.abs(n_done - ref_nd)
    bad = np.flatnonzero(case["clear"] & (apart > 0))
    assert bad.size == 0, "clear rows %s stop at %s, the oracle at %s" % (bad.tolist(), n_done[bad].tolist(), ref_nd[bad].tolist())
    assert apart.max() <= 1, "rows %s stop more than one iteration from the oracle" % np.flatnonzero(apart > 1).tolist()
    if case.get("W") is None:
        case["W"] = iterates_at(case, ref_nd)              # (the oracle's own result: computed once per case)
    Wr = case["W"]
    if apart.any():                                        # a row that stops elsewhere: the oracle's iterate of THAT iteration
        Wr = Wr.copy()
        Wr[apart > 0] = iterates_at(case, n_done, np.flatnonzero(apart > 0))
    assert np.isfinite(W).all(), "rows %s hold non-finite values" % np.flatnonzero(~np.isfinite(W).all(axis=1)).tolist()
    norm = np.linalg.norm(Wr, axis=1)
    live = norm > 0
    err = np.zeros(len(norm))
    err[live] = np.linalg.norm(W[live] - Wr[live], axis=1) / norm[live]
    err[~live] = np.where(np.abs(W[~live]).max(axis=1, initial=0.0) == 0.0, 0.0, np.inf)
    worst = int(err.argmax())
    assert err[worst] < EPS, "row %d (n_done %d, oracle %d): %.3e from the oracle's iterate after %d iterations" % (
        worst, n_done[worst], ref_nd[worst], err[worst], n_done[worst])
    jerr = None
    if J is not None:
        J, Jr = np.asarray(J, dtype=np.float64), trace(case)
        assert J.shape == Jr.shape
        jerr = 0.0
        for v in range(len(n_done)):
            head, tail = J[v, :n_done[v]], J[v, n_done[v]:]
            assert np.isnan(tail).all(), "row %d: the trace holds a value past its last iteration (%d)" % (v, n_done[v])
            e = float(np.abs(head / Jr[v, :n_done[v]] - 1.0).max())
            assert e <= RTOL_J, "row %d: trace %.3e from the oracle's" % (v, e)      # (NaN fails too)
            jerr = max(jerr, e)
    return Verdict(float(err.max()), int((apart > 0).sum()), jerr)
