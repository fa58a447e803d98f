"""The kernel tables as test data (tests/test_table_shapes_host.py, tests/test_gpu_table_entries.py): every line of
pybold_amd/csrc/fast_table.inc, wide_table.inc, exact_table.inc and exact_split_table.inc is a translation unit of its own
with its own family of kernels, and a shape (N scans, K taps) reaches exactly one line of a table.  This module parses the
tables, restates the pickers of pybold_amd/csrc/dispatch.h (`pick_cheapest`, `pick_split`, `ring_fits`) and the part of
`route()` / `route_pp()` that a small pinned call takes, finds by brute force the region of shapes that select each entry,
and yields the edge shapes of that region.  A line added to a table later is picked up without an edit here.

It also draws the inputs of the stop-rule cases: a batch whose rows fire at different iterations, some of them never, none
of them close to the tolerance (`stop_rule_inputs`).

A plain helper module: no fixtures, no pytest configuration.  tests/test_table_shapes_host.py pins the restatement to
the library's own queries."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pybold_amd", "csrc")

# table -> (file, macro, scans per unit of S); the two 48-tap tables are read by tests/search_cases.py
TABLES = {"fast": ("fast_table.inc", "PB_FAST", 16), "wide": ("wide_table.inc", "PB_WIDE", 64),
          "exact": ("exact_table.inc", "PB_EXACT", 64), "exact_split": ("exact_split_table.inc", "PB_EXACT_SPLIT", 256),
          "exact_long": ("exact_long_table.inc", "PB_EXACT_LONG", 64),
          "exact_split_long": ("exact_split_long_table.inc", "PB_EXACT_SPLIT_LONG", 256)}
N_GRID, K_GRID = 2500, 50          # the brute-force grid: 1 <= N <= N_GRID, 1 <= K <= K_GRID
WINDS = (4, 6, 8)                  # window lengths the register-resident forms carry
TOLS = (0.1, 0.02, 0.005)          # the tolerances of test_window_rule_other_window_lengths


@functools.lru_cache(maxsize=None)
def entries(table):
    """The (S, KT) lines of a table, in file order."""
    fname, macro, _ = TABLES[table]
    text = open(os.path.join(CSRC, fname)).read()
    return tuple((int(s), int(kt)) for s, kt in re.findall(r"^%s\((\d+), *(\d+)\)" % macro, text, flags=re.M))


def per_lane(table):
    return TABLES[table][2]


# ---- the pickers of dispatch.h ---------------------------------------------------------------------------------------
def pick_cheapest(tab, N, K, lane):
    """Smallest S * KT among the entries with S >= ceil(N / lane) and KT >= K; the first entry wins a tie."""
    best = None
    s_need = (N + lane - 1) // lane
    for e in tab:
        if e[0] < s_need or e[1] < K:
            continue
        if best is None or e[0] * e[1] < best[0] * best[1]:
            best = e
    return best


def pick(table, N, K):
    """The entry of `table` that carries (N, K), or None.  The four-wave float64 table serves only what the one-wave
    table does not (the scan ranges of kF64 in csrc/dispatch.h)."""
    if N < 1 or K < 1:
        return None
    if table == "exact_split" and pick_cheapest(entries("exact"), N, K, per_lane("exact")):
        return None
    return pick_cheapest(entries(table), N, K, per_lane(table))


def has_pair(entry):
    """The entries that carry the pair forms (pair_or_null and its kin)."""
    return entry[0] <= 20 and entry[1] <= 32


def pick_split(N, K):
    """One series of 16 S < N <= 32 S scans over the two slots of a row: only where no whole-series pair entry fits."""
    whole = pick("fast", N, K)
    if whole and has_pair(whole):
        return None
    best = None
    for e in entries("fast"):
        if not has_pair(e) or e[1] < K or N <= 16 * e[0] or N > 32 * e[0]:
            continue
        if best is None or e[0] * e[1] < best[0] * best[1]:
            best = e
    return best


def ring_fits(S, stop, wind, float64=False):
    """An entry of S samples per lane carries the call's stop rule: the window rule needs its increment ring (S <= 20,
    wind in {4, 6, 8}); the float64 forms carry wind = 6 only, on every entry."""
    if stop != "window":
        return True
    if float64:
        return wind == 6
    return wind in WINDS and S <= 20


# ---- regions and edge shapes -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _choice(table):
    """index of the picked entry (-1: none) for every (N, K) of the grid, as an (N_GRID + 1, K_GRID + 1) array."""
    tab, lane = entries(table), per_lane(table)
    n = np.arange(N_GRID + 1)[:, None]
    k = np.arange(K_GRID + 1)[None, :]
    s_need = (n + lane - 1) // lane
    best_cost = np.full((N_GRID + 1, K_GRID + 1), np.iinfo(np.int64).max)
    best = np.full((N_GRID + 1, K_GRID + 1), -1)
    for i, (s, kt) in enumerate(tab):
        better = (s >= s_need) & (kt >= k) & (s * kt < best_cost)          # strict: the first entry keeps a tie
        best[better] = i
        best_cost[better] = s * kt
    best[0, :] = -1
    best[:, 0] = -1
    if table == "exact_split":
        best[_choice("exact") >= 0] = -1
    return best


def covered(table):
    """Boolean (N_GRID + 1, K_GRID + 1): the shapes some entry of the table carries."""
    return _choice(table) >= 0


def region(table, entry):
    """Sorted list of the (N, K) of the grid that select `entry`."""
    i = entries(table).index(entry)
    nn, kk = np.nonzero(_choice(table) == i)
    return list(zip(nn.tolist(), kk.tolist()))


def _corners(shapes, kt):
    """(full, masked) of an enumerated region: largest N at K = KT; smallest N, then the smallest K there."""
    if not shapes:
        return []
    at_kt = [s for s in shapes if s[1] == kt]
    full = max(at_kt) if at_kt else max(shapes)
    n_min = min(s[0] for s in shapes)
    masked = (n_min, min(s[1] for s in shapes if s[0] == n_min))
    return [("full", full[0], full[1]), ("masked", masked[0], masked[1])]


def edge_shapes(table, entry):
    """[(corner name, N, K)] of an entry: the full corner (largest N, K = KT) and the masked corner (smallest N and
    smallest K of the region), taken from the enumerated set -- regions need not be rectangles.  Empty for a dead line."""
    return _corners(region(table, entry), entry[1])


@functools.lru_cache(maxsize=None)
def _split_regions():
    out = {}
    pairs = [e for e in entries("fast") if has_pair(e)]
    for N in range(1, min(N_GRID, 32 * max(e[0] for e in pairs)) + 1):
        for K in range(1, min(K_GRID, max(e[1] for e in pairs)) + 1):
            e = pick_split(N, K)
            if e:
                out.setdefault(e, []).append((N, K))
    return out


def split_region(entry):
    return _split_regions().get(entry, [])


def split_edge_shapes(entry):
    """Edge shapes of the pair-split family of an entry: 16 S + 1 and 32 S scans at K = KT where pick_split selects the
    entry there, and the corners of the enumerated region (they coincide where the region is the whole band)."""
    shapes = split_region(entry)
    out = []
    for name, n in (("lo", 16 * entry[0] + 1), ("hi", 32 * entry[0])):
        if (n, entry[1]) in shapes:
            out.append((name, n, entry[1]))
    for c in _corners(shapes, entry[1]):
        if (c[1], c[2]) not in [(o[1], o[2]) for o in out]:
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def edge_shapes_pp_wide(entry, P):
    """Edge shapes of `launch_wide_pp` of a wide entry: route_pp() has no pin for one problem per wave and hands a shape to
    the single-row entry wherever one exists (short entries apart), so the corners are those of the part of the region that
    does reach the wide form -- the full corner, and the shortest HRF at the shortest series that has it."""
    shapes = region("wide", entry)
    own = [s for s in shapes if forced_form_pp(s[0], s[1], P, False, None, "fast")[:2] == (WIDE, entry)]
    if own == shapes or not own:
        return _corners(shapes, entry[1])
    k_min = min(s[1] for s in own)
    masked = (min(s[0] for s in own if s[1] == k_min), k_min)
    return [_corners(own, entry[1])[0], ("masked", masked[0], masked[1])]


# ---- the matrix-pipe block counts (fista_mfma.h, fista_mfma2.h, fista_mfma4.h: the audit of profiles/table_entries.txt) ----
MFMA2_PAIRS = ((2, 3), (3, 3), (3, 4), (4, 4), (4, 5), (5, 5), (5, 6), (6, 6), (6, 7), (7, 7), (7, 8), (8, 8), (8, 9), (9, 9),
               (9, 10), (10, 10))


def mfma_instance(form, N, K):
    """The compiled block count a shape lands in, as "mfma<9> 2t" / "mfma2<6,7> 3t" / "mfma4<8> 2t" (2t / 3t: two near
    tiles for up to 33 taps, three beyond), or None where the form does not carry the shape: pick_mfma / pick_mfma2 /
    pick_mfma4 of dispatch.h."""
    tiles = "2t" if K <= 33 else "3t"
    if form == "mfma":
        nb = (N + 30) // 31
        return "mfma<%d> %s" % (nb, tiles) if 129 <= N and nb <= 10 and 1 <= K <= 64 else None
    if form == "mfma2":
        nb = (N + 31) // 32
        if not (5 <= nb <= 20 and 1 <= K <= 65) or (K > 33 and N <= 224):
            return None
        return "mfma2<%d,%d> %s" % (MFMA2_PAIRS[nb - 5] + (tiles,))
    if form == "mfma4":
        return "mfma4<%d> %s" % ((N + 127) // 128, tiles) if 640 < N <= 1280 and 1 <= K <= 65 else None
    raise ValueError(form)


# ---- what a small pinned call runs: route() / route_pp() of dispatch.h for P < 1024 without a workspace -----------------
SINGLE_ROW, PAIR, WIDE, GENERIC = "single row", "pair", "one per wave", "generic"


def forced_form(N, K, P, stop=None, wind=6, force=None):
    """The form `solver.fista_solve(..., force=force)` runs a float32 call of P < 1024 problems on, with the reason when
    it is not what the pin asks for: `(form, entry, why)`.  Restates route(): the split pair form under a pair pin, the
    single-row entry unless its ring does not fit, then one problem per wave, then the LDS kernel."""
    assert P < 1024 and force in ("fast1", "fast2", "fast2d", "cert2", "certonly", "wide")
    plain, window6 = stop is None, (stop == "window" and wind == 6)
    fe, we = pick("fast", N, K), pick("wide", N, K)
    pair_pin = force in ("fast2", "cert2", "certonly")
    se = pick_split(N, K)
    if pair_pin and se and (plain or (window6 and force != "fast2" and we and ring_fits(we[0], stop, wind))):
        return PAIR + " split", se, ""
    if force != "wide" and fe:
        if not ring_fits(fe[0], stop, wind):
            fe = None
    elif force == "wide":
        fe = None
    if fe:
        if force == "fast1":
            return SINGLE_ROW, fe, ""
        cert = window6 and has_pair(fe) and P >= 2 and force in ("cert2", "certonly")
        if cert or (has_pair(fe) and P >= 2 and plain):
            return PAIR, fe, ""
        return SINGLE_ROW, fe, "no pair form on this entry for this call"
    if we and ring_fits(we[0], stop, wind):
        return WIDE, we, "" if force == "wide" else "no single-row entry carries this call"
    return GENERIC, None, "no register-resident entry carries this call"


def forced_form_pp(N, K, P, shared, stop=None, force=None):
    """The same for `solver.fista_solve_pp` (route_pp(); P small enough that one problem per wave finishes first where
    the entry is a short one): force in ("fast1", "fast2", "fast").

    Like `forced_form` this is a restatement by hand of dispatch.h / plan.h and nothing in the library reports a pinned
    form (pb_fista_plan_ex ignores the pins), so a later change of route() / route_pp() -- SPLIT_MIN_P, the cost constants
    of best_form, pick_wide_small -- has to be restated here too: until then the pair and per-problem-taps families of
    tests/test_gpu_table_entries.py could run another kernel of the same entry with every test green.  The unpinned
    queries do not help: `which_kernel` / `launch_plan` name the cheapest form for the batch (the single-row form for one
    problem and for 37 alike), so tests/test_table_shapes_host.py can pin "register-resident or not" only.  What does
    discriminate is the result: the mutation record of profiles/table_entries.txt shows it for the single-row and the
    one-problem-per-wave families, whose kernels differ in their host-side tap handling; the pair forms differ from the
    single-row form in their rounding (fast FIRs), which the 1e-5 bound does not resolve."""
    assert P <= 64 and force in ("fast1", "fast2", "fast")
    fe, we = pick("fast", N, K), pick("wide", N, K)
    if fe:
        if shared and stop is None and has_pair(fe) and P >= 2 and force == "fast2":
            return PAIR, fe, ""
        if force == "fast" and we and we[0] <= 8 and not (shared and stop is None and has_pair(fe) and P >= 2):
            return WIDE, we, ""
        return SINGLE_ROW, fe, ""
    if we:
        return WIDE, we, ""
    return GENERIC, None, "no register-resident entry carries this call"


# ---- inputs ----------------------------------------------------------------------------------------------------------
def lipschitz(hrf, N):
    """1.05 ||A||_2^2 + 1e-9 with A = toeplitz(hrf) . cumsum, from the exact spectral norm (the largest eigenvalue of
    A^T A) as tests/test_gpu_random_shapes.py takes it."""
    from oracle import pybold_oracle as orc
    A = orc.toeplitz_from_kernel(np.asarray(hrf, dtype=np.float64), N, N).dot(np.tril(np.ones((N, N))))
    if N <= 700:
        nrm2 = np.linalg.norm(A, 2) ** 2
    else:
        nrm2 = float(np.linalg.eigvalsh(A.T.dot(A))[-1])
    return 1.05 * nrm2 + 1e-9


def scaled_taps(base, lip, V):
    """One HRF and one step per problem at the price of one spectral norm: the base HRF under a different gain and sign
    per row -- ||A||_2^2 scales with the square of the gain, so every row's step is 1 / (1.05 ||A_v||_2^2 + 1e-9) exactly.
    Returns `(taps (V, K), steps (V,))`; `lip` = lipschitz(base, N)."""
    gain = np.linspace(0.6, 1.4, V) * np.where(np.arange(V) % 2 == 0, 1.0, -1.0)
    return gain[:, None] * np.asarray(base)[None, :], 1.0 / (gain ** 2 * (lip - 1e-9) + 1e-9)


def op_forward_rows(taps, W):
    """h_v * cumsum(w_v) for every row: orc.causal_conv . orc.integ_op with one HRF per row, `taps` (1, K) or (V, K)."""
    Z = np.cumsum(W, axis=-1)
    n = Z.shape[-1]
    out = np.zeros_like(Z)
    for m in range(min(taps.shape[1], n)):
        out[:, m:] += taps[:, m:m + 1] * Z[:, :n - m]
    return out


def op_adjoint_rows(taps, R):
    """The adjoint of `op_forward_rows`: orc.integ_adj . orc.causal_corr."""
    n = R.shape[-1]
    out = np.zeros_like(R)
    for m in range(min(taps.shape[1], n)):
        out[:, :n - m] += taps[:, m:m + 1] * R[:, m:]
    return np.flip(np.cumsum(np.flip(out, axis=-1), axis=-1), axis=-1)


def trajectory(Y, taps, lbda, steps, n_iter, W0=None):
    """The oracle's recurrence (oracle/pybold_oracle.py: fista_batch, loops_batch, deconv_fixed_lbda) for every row, with
    the criteria of both stop rules at every iteration: returns `(crit_loops, crit_window)` with crit_loops (V, n_iter) the
    _loops_deconv criterion of iteration j (NaN for j <= 2) and crit_window {wind: (V, n_iter)} the window criterion
    (NaN for k <= wind).  `taps` (K,) or (V, K), `steps` scalar or (V,).  Only the selection of inputs reads this: what a
    kernel is compared with comes from the oracles themselves."""
    from oracle import pybold_oracle as orc
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    V, n = Y.shape
    taps = np.atleast_2d(np.asarray(taps, dtype=np.float64))           # (1, K) shared or (V, K)
    step = np.broadcast_to(np.asarray(steps, dtype=np.float64), (V,))[:, None]
    th = np.broadcast_to(np.asarray(lbda, dtype=np.float64), (V,))[:, None] * step
    W = np.zeros((V, n)) if W0 is None else np.array(W0, dtype=np.float64)
    betas = orc.momentum_sequence(n_iter)
    crit_l = np.full((V, n_iter), np.nan)
    crit_w = {w: np.full((V, n_iter), np.nan) for w in WINDS}
    hist = []
    for k in range(n_iter):
        U = W - step * op_adjoint_rows(taps, op_forward_rows(taps, W) - Y)
        if k > 0 and hist:
            hist[-1] = U                                   # (the stored alias of w_k was overwritten: deconv_fixed_lbda)
        P = orc.soft_threshold(U, th)
        W = P + betas[k] * (P - (U if k > 0 else 0.0))
        if k > 2:
            crit_l[:, k] = np.linalg.norm(W - U, axis=1) / (np.linalg.norm(W, axis=1) + 1.0e-10)
        hist.append(W)
        hist = hist[-max(WINDS):]
        for w in WINDS:
            if k > w:
                h = hist[-w:]
                half = w // 2
                old, new = np.mean(h[:-half], axis=0), np.mean(h[-half:], axis=0)
                crit_w[w][:, k] = np.linalg.norm(new - old, axis=1) / (np.linalg.norm(new, axis=1) + 1.0e-10)
    return crit_l, crit_w


def fire_iteration(crit, tol, n_iter):
    """n_done of every row under a rule with criterion `crit` (V, n_iter): first k with crit < tol, plus one; n_iter where
    none.  `clear`: the criterion stays 1 % of tol away from tol at every test up to and including the firing one."""
    below = np.nan_to_num(crit, nan=np.inf) < tol
    fired = below.any(axis=1)
    first = np.where(fired, below.argmax(axis=1), n_iter - 1)
    n_done = np.where(fired, first + 1, n_iter)
    fired = fired & (n_done < n_iter)                      # (a row that meets the rule at the last iteration ran them all)
    idx = np.arange(crit.shape[1])[None, :]
    tested = np.isfinite(crit) & (idx <= first[:, None])
    clear = ~(tested & (np.abs(crit - tol) < 0.01 * tol)).any(axis=1)
    return n_done, fired, clear


def _select(n_done, fired, clear, V, never_ok=None):
    """V rows of a pool that meet the conditions of a stop-rule case, or None: at least a third of the rows fire, at two
    or more different iterations; at least one row never fires; every row is clear of the tolerance.  `never_ok`: boolean,
    the rows that may be kept as never-firing ones."""
    ok = np.flatnonzero(clear)
    never = [i for i in ok if not fired[i] and (never_ok is None or never_ok[i])]
    fire = [i for i in ok if fired[i]]
    if not never or len({n_done[i] for i in fire}) < 2:
        return None
    n_fire = max((V + 2) // 3, min(V - 1, (V + 1) // 2))
    if len(fire) < n_fire:
        return None
    # firing rows spread over the iterations that occur (sorted by iteration, evenly spaced picks); the rest never fire --
    # or, where the pool has too few of those, fire too
    fire.sort(key=lambda i: (n_done[i], i))
    n_never = min(len(never), V - n_fire)
    n_fire = V - n_never
    if len(fire) < n_fire:
        return None
    picks = [fire[int(round(j * (len(fire) - 1) / max(n_fire - 1, 1)))] for j in range(n_fire)]
    if len(set(picks)) < n_fire:
        picks = fire[:n_fire - 1] + [fire[-1]]
    if len({n_done[i] for i in picks}) < 2:
        return None
    rows = sorted(picks + never[:n_never])
    return np.array(rows)


class NoInputs(Exception):
    """No batch of this shape meets the conditions of a stop-rule case."""


def _budgets(crit, tol, horizon, first_test):
    """Iteration budgets to try for a tolerance: the horizon, then where the middle of the pool fires (the existing
    stop-rule tests take the median of the firing iterations: half of the rows fire, half do not)."""
    n_done, fired, _ = fire_iteration(crit, tol, horizon)
    out = [horizon]
    if fired.any():
        at = np.sort(n_done[fired])
        out += [int(at[min(len(at) - 1, int(q * len(at)))]) for q in (0.5, 0.35, 0.65, 0.2, 0.8)]
    seen = []
    for n in out:
        if n >= first_test + 3 and n not in seen:
            seen.append(n)
    return seen


def stop_rule_inputs(N, K, V, rule, wind=6, seed=0, float32=True, per_problem_taps=False, n_iter=60):
    """Inputs of a stop-rule case: `dict(Y, taps, steps, lbda, tol, n_iter, n_done)` with Y (V, N).  Rows of different
    amplitude (so that the rule fires at different iterations) are drawn into a pool; V of them are kept such that, for
    one tol of TOLS and a budget of at most `n_iter` iterations, the conditions of `_select` hold; the budget is doubled
    (twice at most) where no tol does, and NoInputs is raised where that fails too.  Deterministic."""
    rng = np.random.RandomState(1000003 * seed + 1009 * N + K)
    base = 0.3 * rng.randn(K)
    lip = lipschitz(base, N)
    first_test = 3 if rule == "loops" else wind + 1
    horizon = n_iter
    for attempt in range(3):
        pool = max(4 * V, 24)
        Y = rng.randn(pool, N) * (10.0 ** rng.uniform(-1.5, 1.0, size=(pool, 1)))
        if float32:
            Y = Y.astype(np.float32).astype(np.float64)
        taps, steps = (scaled_taps(base, lip, pool) if per_problem_taps else (base, 1.0 / lip))
        # one lambda for the batch, a tenth of the pool's median lambda_max = ||A^T y||_inf: with amplitudes over 2.5 decades
        # some rows are all zero, some sparse, some dense
        lbda = 0.1 * float(np.median(np.abs(op_adjoint_rows(np.atleast_2d(taps), Y)).max(axis=1)))
        crit_l, crit_w = trajectory(Y, taps, lbda, steps, horizon)
        crit = crit_l if rule == "loops" else crit_w[wind]
        for tol in TOLS:
            for n in _budgets(crit, tol, horizon, first_test):
                n_done, fired, clear = fire_iteration(crit[:, :n], tol, n)
                rows = _select(n_done, fired, clear, V)
                if rows is not None:
                    if per_problem_taps:
                        taps, steps = taps[rows], steps[rows]
                    return dict(N=N, Y=Y[rows], taps=taps, steps=steps, lbda=lbda, tol=tol, n_iter=n, n_done=n_done[rows])
        horizon *= 2
    raise NoInputs("no stop-rule inputs for N=%d K=%d V=%d %s wind=%d" % (N, K, V, rule, wind))


def certificate_reach(N, S, split):
    """How far above tol the window criterion of a row must stay for the no-fire certificate of the pair form to be able
    to clear it, from the bound the kernel documents (fista_pair_ffa.h): it compares the numerator of the criterion on ONE
    tracked sample per lane (sample S / 2 of each lane's strip of S; a split series has a second set in its other half)
    with tol^2 (||w_k||^2 / 0.3133 + 4 ||w_{k+1}||^2 / 0.6467) ~ 9.4 tol^2 ||w||^2.  With the increments spread evenly over
    the N samples the tracked ones carry n_tracked / N of ||3 (new - old)||^2, so the criterion has to exceed
    tol sqrt(1.04 N / n_tracked); twice that is asked here, for a spread that is not even.  None: fewer than eight tracked
    samples lie inside the series -- with none the certificate cannot clear any row, and the share of a handful is not
    predictable (measured at 6 scans, one tracked sample: 10 to 14 of 18 rows that stay 5 tol away were flagged; from eight
    tracked samples on, 161 scans at S = 19, none was)."""
    first = min(N, 16 * S)
    tracked = sum(1 for lane in range(16) if lane * S + S // 2 < first)
    if split:
        tracked += sum(1 for lane in range(16) if 16 * S + lane * S + S // 2 < N)
    return 2.0 * np.sqrt(1.04 * N / tracked) if tracked >= 8 else None


def certificate_inputs(N, K, V, S, split=False, seed=0, n_iter=60):
    """Inputs of a window-rule (wind = 6) case for the certificate families: the conditions of `stop_rule_inputs`, and the
    rows that never fire stay `certificate_reach` times tol above tol at every test, so that a sound certificate clears
    them and `force="certonly"` flags only rows whose rule fires.  A cold batch cannot be both (rows that fire within a
    few iterations at a tol the dense rows are that far from do not exist: the criterion starts near 0.9 / 7), so half of
    the pool is WARM-started next to its solution -- 600 oracle iterations, perturbed by 1e-4 .. 0.3 of its size: these
    fire at the first tests, at different iterations -- and half is cold and dense (lambda_max / lambda 5 .. 100).  Returns
    the dict of `stop_rule_inputs` with `W0` (V, N) added (rows of zeros: cold); budgets of 16 .. 24 iterations first."""
    from oracle import c_oracle
    reach = certificate_reach(N, S, split)
    if reach is None:
        raise NoInputs("fewer than eight tracked samples of the certificate inside %d scans at S = %d" % (N, S))
    rng = np.random.RandomState(2000003 * (seed + 1) + 1009 * N + K)
    taps = 0.3 * rng.randn(K)
    step = 1.0 / lipschitz(taps, N)
    lbda = 0.5
    pool = max(4 * V, 24)
    G = rng.randn(pool, N)
    lmax = np.abs(op_adjoint_rows(np.atleast_2d(taps), G)).max(axis=1)
    Y = G * (lbda * 10.0 ** rng.uniform(0.7, 2.0, pool) / lmax)[:, None]
    Y = Y.astype(np.float32).astype(np.float64)
    warm = np.arange(pool) % 2 == 0
    W0 = np.zeros((pool, N))
    near = c_oracle.fista_batch(Y[warm], taps, lbda, step, 600, threads=4)[0]
    size = np.linalg.norm(near, axis=1, keepdims=True) / np.sqrt(N)
    W0[warm] = near + 10.0 ** rng.uniform(-4.0, -0.5, size=(int(warm.sum()), 1)) * size * rng.randn(int(warm.sum()), N)
    crit = trajectory(Y, taps, lbda, step, n_iter, W0=W0)[1][6]
    for tol in sorted(TOLS):
        for n in (16, 20, 24, 12, 32, 40, n_iter):
            n_done, fired, clear = fire_iteration(crit[:, :n], tol, n)
            far = ~warm & (np.nanmin(crit[:, 7:n], axis=1) >= reach * tol)
            rows = _select(n_done, fired, clear, V, far)
            if rows is not None:
                return dict(N=N, Y=Y[rows], taps=taps, steps=step, lbda=lbda, tol=tol, n_iter=n, n_done=n_done[rows], W0=W0[rows],
                            reach=reach)
    raise NoInputs("no certificate inputs for N=%d K=%d V=%d S=%d" % (N, K, V, S))


LADDER = (2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128)


@functools.lru_cache(maxsize=None)
def _region_set(table, entry, split):
    return frozenset(split_region(entry) if split else region(table, entry))


def stop_rule_inputs_near(table, entry, N, K, V, rule, split=False, **kw):
    """`stop_rule_inputs` at the edge shape (N, K) -- or, where no batch of that shape can meet the conditions (a series of
    one scan converges at once: its rule fires at the first test or never), at the next length of LADDER that the same
    entry carries with the same K.  The dict names the length used (`N`).  `certificate=True`: `certificate_inputs`."""
    shapes = _region_set(table, entry, split)
    certificate = kw.pop("certificate", False)
    for n in (N,) + tuple(n for n in LADDER if n > N and (n, K) in shapes):
        try:
            if certificate:
                return certificate_inputs(n, K, V, entry[0], split=split, seed=kw.get("seed", 0), n_iter=kw.get("n_iter", 60))
            return stop_rule_inputs(n, K, V, rule, **kw)
        except NoInputs:
            continue
    raise NoInputs("no stop-rule inputs for %s %s at K=%d from N=%d on" % (table, entry, K, N))
