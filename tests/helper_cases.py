"""Cases, inputs, references and error bounds for the row-in-LDS helper kernels of csrc/generic.h (launchers: csrc/capi.hip):
the operator surface (pb_integ_op, pb_integ_adj, pb_conv, pb_corr, pb_op_forward, pb_op_adjoint), the outputs
(pb_fista_outputs, pb_fista_outputs_pp), the statistics (pb_fista_stats[_d], pb_lambda_max[_d], pb_hrf_cost[_d],
pb_hrf_cost_pv[_d]), the Lipschitz constants (pb_gram_frobenius, pb_spectral_radius[_pp]) and pb_inf_norm -- at the edges
of the five block primitives they rest on (block_cumsum, block_conv, block_corr, block_sum, block_max).  NumPy only: no
torch, no GPU.  tests/test_helper_cases_host.py checks this module, tests/test_gpu_helper_kernels.py runs the kernels.

Two input families per case, three rows each, seeded from the case:

* integer: samples and taps are small integers, the magnitude chosen per case such that the sum of the ABSOLUTE values of
  the terms of every sum of the operation stays below 2^53 (asserted on int64 arithmetic).  Every partial sum in every
  order is then an exactly representable integer, with or without fused multiply-add: the kernel must return the bits of
  the int64 result whatever its chunking.
* real: (0) amplitudes spread over 1e-6 .. 1e6, (1) an alternating +-1e6 carrier with 1e-9 relative jitter (the cumulative
  sums cancel nine digits), (2) a DC offset of 1e8.  Reference in np.longdouble (63-bit mantissa required: `LD_OK`).  The
  bound of every output element is derived, not measured: a sum of m terms in any order, fused or not, errs by at most
  (m + 8) 2^-53 sum|terms| (the 8 covers the subtract-and-re-add steps of the chunked scan); a stage fed by a stage carries
  the inner bound through its own linear map (|taps| for the Toeplitz products, ones for the scans) and adds its own bound
  on the perturbed magnitudes.  The GPU test compares |got - ref| <= bound element by element and adds no tolerance."""
import collections
import functools
import zlib

import numpy as np

LD = np.longdouble
LD_NMANT = int(np.finfo(LD).nmant)
LD_OK = LD_NMANT >= 63
U = LD(2.0) ** -53
TWO53 = 2 ** 53
THREADS, WAVE = 256, 64
LDS_DOUBLES_MAX = 20000                      # csrc/capi.hip
LIMIT_K = 30

EDGE_N = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000)
RECT = ((1, 300), (300, 1), (255, 257), (257, 255), (513, 100), (100, 513))      # (n_in, n_out)

GROUPS = collections.OrderedDict((
    ("operators", ("integ_op", "integ_adj", "conv", "corr", "op_forward", "op_adjoint")),
    ("outputs", ("outputs", "outputs_pp")),
    ("statistics", ("stats", "stats_d", "lambda_max", "lambda_max_d", "hrf_cost", "hrf_cost_d", "hrf_cost_pv",
                    "hrf_cost_pv_d")),
    ("lipschitz", ("gram_frobenius", "spectral_radius", "spectral_radius_pp")),
    ("inf_norm", ("inf_norm",)),
))
ENTRY_POINT = {"integ_op": "pb_integ_op", "integ_adj": "pb_integ_adj", "conv": "pb_conv", "corr": "pb_corr",
               "op_forward": "pb_op_forward", "op_adjoint": "pb_op_adjoint", "outputs": "pb_fista_outputs",
               "outputs_pp": "pb_fista_outputs_pp", "stats": "pb_fista_stats", "stats_d": "pb_fista_stats_d",
               "lambda_max": "pb_lambda_max", "lambda_max_d": "pb_lambda_max_d", "hrf_cost": "pb_hrf_cost",
               "hrf_cost_d": "pb_hrf_cost_d", "hrf_cost_pv": "pb_hrf_cost_pv", "hrf_cost_pv_d": "pb_hrf_cost_pv_d",
               "gram_frobenius": "pb_gram_frobenius", "spectral_radius": "pb_spectral_radius",
               "spectral_radius_pp": "pb_spectral_radius_pp", "inf_norm": "pb_inf_norm"}
ROW_ENTRIES = GROUPS["operators"] + GROUPS["outputs"] + GROUPS["statistics"]       # one row staged per workgroup
RECT_ENTRIES = ("conv", "corr", "op_forward", "op_adjoint")
INTEG = ("integ_op", "integ_adj")
F32_Y = ("stats", "lambda_max", "hrf_cost", "hrf_cost_pv")                          # y is float32; the _d twin takes float64
HAS_Y = F32_Y + tuple(e + "_d" for e in F32_Y)
CUMSUM_ON_ROW = ("integ_op", "integ_adj", "op_forward", "outputs", "outputs_pp", "stats", "stats_d")

# entry, samples in / out as the C entry point names them, taps, option (outputs: which of z / x; stats: y_rep;
# hrf_cost*: candidates)
Case = collections.namedtuple("Case", "entry n_in n_out K opt")


def case_id(c):
    shape = "%d" % c.n_in if c.n_in == c.n_out else "%dto%d" % (c.n_in, c.n_out)
    return "%s-%s-K%d%s" % (c.entry, shape, c.K, "" if c.opt is None else "-%s" % (c.opt,))


def tap_counts(n):
    """At most four of {1, 2, n-1, n, n+1, 2n, 30, 127}: n and n+1 always (n >= 2), two more that rotate with the length."""
    idx = EDGE_N.index(n) if n in EDGE_N else 0
    extras = [1, 30, 2 * n, n - 1, 2, 127]
    rot = (2 * idx) % len(extras)
    out = []
    for k in ([n, n + 1] if n >= 2 else [1, 2]) + extras[rot:] + extras[:rot]:
        if k >= 1 and k not in out and len(out) < 4:
            out.append(k)
    return tuple(out)


def _opt(entry, j):
    if entry.startswith("outputs"):
        return ("zx", "z", "x", "zx")[j % 4]
    if entry.startswith("stats"):
        return 1 + j % 2                           # y_rep: 2 on three problems leaves the last series with one problem
    if entry.startswith("hrf_cost"):
        return (1, 3)[j % 2]                       # candidate HRFs
    return None


@functools.lru_cache(maxsize=None)
def row_cases(group):
    out = []
    for entry in GROUPS[group]:
        for n in EDGE_N:
            for j, K in enumerate((0,) if entry in INTEG else tap_counts(n)):
                out.append(Case(entry, n, n, K, _opt(entry, j)))
        if entry in RECT_ENTRIES:
            for n_in, n_out in RECT:
                for K in (1, 30, max(n_in, n_out) + 1):
                    out.append(Case(entry, n_in, n_out, K, None))
    return tuple(out)


# ---- LDS of every launcher, in doubles (csrc/capi.hip) -----------------------------------------------------------------
def lds_doubles(entry, n, K, n_other=None):
    nmax = n if n_other is None else max(n, n_other)
    if entry in INTEG:
        return 2 * nmax + 8
    if entry in RECT_ENTRIES:
        return 2 * nmax + K + 8
    if entry in ("outputs", "outputs_pp", "stats", "stats_d", "lambda_max", "lambda_max_d"):
        return 2 * n + K + 8
    if entry.startswith("hrf_cost"):
        return n + K + 8
    if entry.startswith("spectral_radius"):
        return 3 * n + K + 8
    if entry == "gram_frobenius":
        return n + 8                               # the launcher's check; the closed form itself stages 3 K <= 3072
    raise KeyError(entry)


def limit_shape(entry):
    """(N, K): the longest row with K = 30 taps (none for the two scans) that the launcher's own check admits."""
    K = 0 if entry in INTEG else LIMIT_K
    n = LDS_DOUBLES_MAX
    while lds_doubles(entry, n, K) > LDS_DOUBLES_MAX:
        n -= 1
    assert lds_doubles(entry, n + 1, K) > LDS_DOUBLES_MAX >= lds_doubles(entry, n, K)
    return n, K


def over_shape(entry):
    n, K = limit_shape(entry)
    return n + 1, K


def limit_case(entry):
    n, K = limit_shape(entry)
    return Case(entry, n, n, K, {"outputs": "zx", "outputs_pp": "zx"}.get(entry, 2 if entry.startswith("stats") else
                                                                        3 if entry.startswith("hrf_cost") else None))


# ---- block primitives in the kernels' own order (float64 NumPy; products and sums rounded separately) --------------------
def emu_block_cumsum(x, reverse=False, mutant=None):
    """block_cumsum<REVERSE> of csrc/generic.h on every row of x: 256 threads own ceil(n / 256) consecutive elements, the
    chunk totals are scanned inside each wave of 64 (Hillis-Steele) and across the four waves, and every thread re-adds its
    elements to (wave offset + inclusive total - own total).  mutant = "drop_last": the chunk totals miss the chunk's last
    element (a one-off in `hi`)."""
    x = np.asarray(x)
    R, n = x.shape
    src = x[:, ::-1] if reverse else x
    chunk = (n + THREADS - 1) // THREADS
    pad = np.zeros((R, THREADS * chunk), dtype=x.dtype)
    pad[:, :n] = src
    own = pad.reshape(R, THREADS, chunk)
    owned = np.minimum(np.maximum(n - np.arange(THREADS) * chunk, 0), chunk)           # elements of every thread
    local = np.zeros((R, THREADS), dtype=x.dtype)
    for j in range(chunk):
        take = (j < owned - 1) if mutant == "drop_last" else (j < owned)
        local = np.where(take[None, :], local + own[:, :, j], local)
    incl = local.reshape(R, THREADS // WAVE, WAVE).copy()
    o = 1
    while o < WAVE:
        up = np.zeros_like(incl)
        up[:, :, o:] = incl[:, :, :-o]
        incl[:, :, o:] = incl[:, :, o:] + up[:, :, o:]
        o <<= 1
    red = incl[:, :, WAVE - 1]
    woff = np.zeros((R, THREADS // WAVE), dtype=x.dtype)
    for w in range(1, THREADS // WAVE):
        woff[:, w] = woff[:, w - 1] + red[:, w - 1]
    if mutant == "subtract":
        run = (woff[:, :, None] + incl).reshape(R, THREADS) - local
    else:
        excl = np.zeros_like(incl)
        excl[:, :, 1:] = incl[:, :, :-1]
        run = (woff[:, :, None] + excl).reshape(R, THREADS)
    out = np.zeros_like(own)
    for j in range(chunk):
        run = np.where((j < owned)[None, :], run + own[:, :, j], run)
        out[:, :, j] = run
    out = out.reshape(R, THREADS * chunk)[:, :n]
    return out[:, ::-1] if reverse else out


def emu_block_conv(k, x, n_out, mutant=None):
    """block_conv: out[i] = sum_{m = m0 .. m1} k[m] x[i - m], m ascending.  mutant = "m1_short": m1 one tap short."""
    k, x = np.atleast_2d(k), np.asarray(x)
    R, n_in = x.shape
    K = k.shape[1]
    out = np.zeros((R, n_out), dtype=x.dtype)
    for i in range(n_out):
        m0, m1 = max(0, i - n_in + 1), min(K - 1, i) - (1 if mutant == "m1_short" else 0)
        for m in range(m0, m1 + 1):
            out[:, i] = out[:, i] + k[:, m] * x[:, i - m]
    return out


# ---- the operations, generic in the working type (int64: exact; longdouble: reference; float64: plain NumPy) ----------------
class Track:
    """real: carry an error bound with every value; integer: collect sum|terms| of every sum."""

    def __init__(self, real):
        self.real, self.mags = real, []


def _flip(a, reverse):
    return a[:, ::-1] if reverse else a


def _cumsum(x, e, reverse, tr, emu=False):
    val = emu_block_cumsum(x, reverse, emu if isinstance(emu, str) else None) if emu else _flip(np.cumsum(_flip(x, reverse), axis=1), reverse)
    if tr is None:
        return val, None
    ax = np.abs(x)
    if not tr.real:
        tr.mags.append(int(ax.sum(axis=1).max()))
        return val, None
    n = x.shape[1]
    m = (np.arange(n, 0, -1) if reverse else np.arange(1, n + 1)).astype(LD)[None, :]
    scan = lambda a: _flip(np.cumsum(_flip(a, reverse), axis=1), reverse)
    return val, scan(e) + (m + 8) * U * scan(ax + e)


def _toeplitz(k, x, e, n_out, tr, corr, rev_taps=False):
    """corr = False: out[i] = sum_m k[m] x[i - m] (0 <= i - m < n_in); corr = True: out[j] = sum_m k[m] x[j + m] (j + m < n_in)."""
    R, n_in = x.shape
    k = np.atleast_2d(k)
    K = k.shape[1]
    val = np.zeros((max(R, k.shape[0]), n_out), dtype=x.dtype)
    track = tr is not None
    if track:
        S = np.zeros(val.shape, dtype=x.dtype if not tr.real else LD)
        E = np.zeros(val.shape, dtype=LD)
        cnt = np.zeros(n_out, dtype=np.int64)
        ak, ax = np.abs(k), np.abs(x) + (e if tr.real else 0)
    ms = range(min(K, n_in if corr else n_out))
    for m in (reversed(ms) if rev_taps else ms):
        if corr:
            lo, hi, s0 = 0, min(n_out, n_in - m), m
        else:
            lo, hi, s0 = m, min(n_out, n_in + m), 0
        if hi <= lo:
            continue
        w = hi - lo
        val[:, lo:hi] += k[:, m:m + 1] * x[:, s0:s0 + w]
        if track:
            S[:, lo:hi] += ak[:, m:m + 1] * ax[:, s0:s0 + w]
            cnt[lo:hi] += 1
            if tr.real:
                E[:, lo:hi] += ak[:, m:m + 1] * e[:, s0:s0 + w]
    if not track:
        return val, None
    if not tr.real:
        tr.mags.append(int(S.max()) if S.size else 0)
        return val, None
    return val, E + (cnt.astype(LD)[None, :] + 8) * U * S


def _sqsum(d, e, tr):
    """sum_i d_i^2 per row (the fma chain and block_sum)."""
    val = (d * d).sum(axis=1)
    if tr is None:
        return val, None
    if not tr.real:
        tr.mags.append(int(val.max()))
        return val, None
    n = d.shape[1]
    ad = np.abs(d)
    return val, (2 * ad * e + e * e).sum(axis=1) + (n + 8) * U * ((ad + e) ** 2).sum(axis=1)


def _diff(a, ea, y, tr):
    """a - y, one rounding on values known to ea."""
    d = a - y
    if tr is None or not tr.real:
        return d, None
    return d, ea + (2 + 8) * U * (np.abs(a) + ea + np.abs(y))


def evaluate(case, inp, W, tr=None, emu=False, rev_taps=False):
    """The operation of `case` on the inputs in working type W.  {name: (value, bound or None)}."""
    x = inp["x"].astype(W)
    k = inp["taps"].astype(W) if inp.get("taps") is not None else None
    y = inp["y"].astype(W) if inp.get("y") is not None else None
    e0 = np.zeros(x.shape, dtype=LD) if tr is not None and tr.real else None
    N = case.n_in
    entry = case.entry[:-2] if case.entry.endswith("_d") else case.entry
    if entry == "integ_op":
        return {"out": _cumsum(x, e0, False, tr, emu)}
    if entry == "integ_adj":
        return {"out": _cumsum(x, e0, True, tr, emu)}
    if entry == "conv":
        return {"out": _toeplitz(k, x, e0, case.n_out, tr, False, rev_taps)}
    if entry == "corr":                                   # r has n_out samples, the result n_in
        return {"out": _toeplitz(k, x, e0, case.n_in, tr, True, rev_taps)}
    if entry == "op_forward":
        a, ea = _cumsum(x, e0, False, tr, emu)
        return {"out": _toeplitz(k, a, ea, case.n_out, tr, False, rev_taps)}
    if entry == "op_adjoint":
        a, ea = _toeplitz(k, x, e0, case.n_in, tr, True, rev_taps)
        return {"out": _cumsum(a, ea, True, tr, emu)}
    if entry in ("outputs", "outputs_pp"):
        z, ez = _cumsum(x, e0, False, tr, emu)
        return {"z": (z, ez), "x": _toeplitz(k, z, ez, N, tr, False, rev_taps)}
    if entry == "stats":
        a, ea = _cumsum(x, e0, False, tr, emu)
        b, eb = _toeplitz(k, a, ea, N, tr, False, rev_taps)
        d, ed = _diff(b, eb, y[np.arange(x.shape[0]) // case.opt], tr)
        ax = np.abs(x)
        l1 = ax.sum(axis=1)
        if tr is not None and not tr.real:
            tr.mags.append(int(l1.max()))
        return {"r2": _sqsum(d, ed, tr), "l1": (l1, (N + 8) * U * l1 if tr is not None and tr.real else None)}
    if entry == "lambda_max":
        b, eb = _toeplitz(k, y, e0, N, tr, True, rev_taps)
        b, eb = _cumsum(b, eb, True, tr, emu)
        return {"out": (np.abs(b).max(axis=1), eb.max(axis=1) if eb is not None else None)}
    if entry in ("hrf_cost", "hrf_cost_pv"):
        vals, errs = [], []
        for c in range(case.opt):                          # taps [C][K] or [C][V][K]
            acc, ea = _toeplitz(k[c], x, e0, N, tr, False, rev_taps)
            d, ed = _diff(acc, ea, y, tr)
            v, ev = _sqsum(d, ed, tr)
            vals.append(v / 2 if W is not np.int64 else v)  # (integers: the halving is done in float64, exactly)
            errs.append(ev / 2 if ev is not None else None)
        return {"cost": (np.stack(vals), np.stack(errs) if errs[0] is not None else None)}
    raise KeyError(case.entry)


# ---- inputs -------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def real_rows(rng, rows, n):
    """(0) amplitudes over 1e-6 .. 1e6, (1) alternating +-1e6 carrier with 1e-9 relative jitter, (2) DC offset 1e8."""
    out = np.empty((3, n))
    out[0] = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6.0, 6.0, n)
    out[1] = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * 1.0e6 * (1.0 + 1.0e-9 * rng.standard_normal(n))
    out[2] = 1.0e8 + rng.standard_normal(n)
    return out[np.arange(rows) % 3]


def _taps_shape(case, rows):
    if case.entry in INTEG:
        return None
    if case.entry == "outputs_pp":
        return (rows, case.K)
    if case.entry.startswith("hrf_cost_pv"):
        return (case.opt, rows, case.K)
    if case.entry.startswith("hrf_cost"):
        return (case.opt, case.K)
    return (case.K,)


def _n_src(case):
    return case.n_out if case.entry in ("corr", "op_adjoint") else case.n_in


def make_inputs(case, family, rows=3, M=None):
    """x: the rows the entry stages (w, z, x or r; for lambda_max the series is y and x aliases it); taps; y."""
    rng = _rng(case.entry[:-2] if case.entry.endswith("_d") else case.entry, case.n_in, case.n_out, case.K, family)
    n, ts = _n_src(case), _taps_shape(case, rows)
    y_rows = -(-rows // case.opt) if case.entry.startswith("stats") else rows
    inp = {"taps": None, "y": None}
    if family == "integer":
        mk = min(M, 3)
        inp["x"] = rng.integers(-M, M + 1, (rows, n)).astype(np.float64)
        if ts is not None:
            inp["taps"] = rng.integers(-mk, mk + 1, ts).astype(np.float64)
        if case.entry in HAS_Y:
            inp["y"] = rng.integers(-100 * M, 100 * M + 1, (y_rows, n)).astype(np.float64)
    else:
        inp["x"] = real_rows(rng, rows, n)
        if ts is not None:
            inp["taps"] = rng.standard_normal(ts)
        if case.entry in HAS_Y:
            inp["y"] = real_rows(rng, y_rows, n)
    if case.entry in F32_Y:
        inp["y"] = inp["y"].astype(np.float32)             # the reference is computed on the widened data
    if case.entry.startswith("lambda_max"):
        inp["x"] = inp["y"]
    return inp


@functools.lru_cache(maxsize=8)
def reference(case, family, rows=3):
    """{"inputs": ..., "outs": {name: (float64 or longdouble reference, longdouble bound per element or None = exact)},
    "mags": sum|terms| of every sum (integer family)}."""
    if family == "integer":
        for M in (9, 5, 3, 2, 1):
            inp = make_inputs(case, family, rows, M)
            tr = Track(False)
            outs = evaluate(case, inp, np.int64, tr)
            if max(tr.mags) < TWO53:
                break
        assert max(tr.mags) < TWO53, (case, max(tr.mags))     # the precondition of bit equality
        ref = {}
        for name, (v, _) in outs.items():
            f = v.astype(np.float64)
            assert (f.astype(np.int64) == v).all()
            ref[name] = (f / 2 if name == "cost" else f, None)
        return {"inputs": inp, "outs": ref, "mags": tuple(tr.mags), "M": M}
    assert LD_OK, "np.longdouble has a %d-bit mantissa here" % LD_NMANT
    inp = make_inputs(case, family, rows)
    return {"inputs": inp, "outs": evaluate(case, inp, LD, Track(True)), "mags": None, "M": None}


def cancellation(case, rows=3):
    """max over the elements of the carrier row of sum|terms| / |result| in the scan that acts on the row itself."""
    x = make_inputs(case, "real", rows)["x"][1:2].astype(LD)
    rev = case.entry == "integ_adj"
    s, a = _cumsum(x, None, rev, None)[0], _cumsum(np.abs(x), None, rev, None)[0]
    return float((a / np.maximum(np.abs(s), LD(1e-300))).max())


def ratio(got, ref, bound):
    """Worst |got - ref| / bound over the elements (bound None: 0 if the bits agree, else inf)."""
    got = np.asarray(got, dtype=np.float64)
    if bound is None:
        return 0.0 if np.array_equal(got.view(np.int64), np.asarray(ref, dtype=np.float64).view(np.int64)) else float("inf")
    err = np.abs(got.astype(LD) - ref)
    if not np.isfinite(got).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / bound)
    return float(r.max())


# ---- pb_gram_frobenius ---------------------------------------------------------------------------------------------
GRAM_RTOL = 1.0e-11                                  # tests/test_gpu_blind_batch.py
GRAM_LIMIT_N = LDS_DOUBLES_MAX - 8
GRAM_CASES = ((1024, 1100), (1025, 1100), (2, 2), (3, 2), (65, 65), (66, 65), (257, 257), (258, 257), (1, 1))   # (K, N)
GRAM_LIMIT_CASES = ((2000, GRAM_LIMIT_N), (LIMIT_K, GRAM_LIMIT_N))


def hrf_like(rng, rows, K):
    """A positive bump with 5 % noise, another dilation per row: what the Lipschitz helpers are given."""
    t = np.arange(K)[None, :] / max(K - 1, 1)
    width = rng.uniform(0.15, 0.35, (rows, 1))
    return np.exp(-0.5 * ((t - 0.3) / width) ** 2) * (1.0 + 0.05 * rng.standard_normal((rows, K))) + 0.01


def gram_taps(K, N, rows=2):
    """One HRF per row.  At the limit length the second row is TWICE the first: its constant is four times the first's, bit
    for bit (powers of two), so that the reference -- five seconds of longdouble per row there -- is computed once."""
    taps = hrf_like(_rng("gram", K, N), rows, K)
    if N >= GRAM_LIMIT_N:
        taps[1:] = 2.0 * taps[0]
    return taps


def gram_reference(taps, N):
    """|| A^T A ||_F, A = toeplitz(h) tril(1), by the diagonal recurrence in longdouble: with c = cumsum(h),
    (A^T A)[j, j + d] = R_d(N - 1 - j - d), R_d(T) = sum_{t <= T} c[t] c[t + d]; step T updates every diagonal d <= N - 1 - T.
    O(N) vector steps, no dense matrix."""
    taps = np.atleast_2d(taps)
    if N >= GRAM_LIMIT_N and len(taps) > 1 and (taps[1:] == 2.0 * taps[0]).all():
        return gram_reference(taps[:1], N) * np.array([1.0] + [4.0] * (len(taps) - 1), dtype=LD)
    P, K = taps.shape
    h = np.zeros((P, N), dtype=LD)
    h[:, :min(K, N)] = taps[:, :N]
    c = np.cumsum(h, axis=1)
    r = np.zeros((P, N), dtype=LD)
    acc = np.zeros((P, N), dtype=LD)
    tmp = np.empty((P, N), dtype=LD)
    for T in range(N):
        L = N - T
        np.multiply(c[:, T:T + 1], c[:, T:], out=tmp[:, :L])
        np.add(r[:, :L], tmp[:, :L], out=r[:, :L])
        np.multiply(r[:, :L], r[:, :L], out=tmp[:, :L])
        np.add(acc[:, :L], tmp[:, :L], out=acc[:, :L])
    return np.sqrt(acc[:, 0] + 2 * acc[:, 1:].sum(axis=1))


# ---- pb_spectral_radius, pb_spectral_radius_pp ------------------------------------------------------------------------
RHO_RTOL = 1.0e-12                                   # test_fused_power_iteration_equals_host_loop
SPECTRAL_N = (1, 2, 65, 257, 513)
SPECTRAL_ITERS = (0, 2, 30)
TOL_MARGIN = 0.01
Spectral = collections.namedtuple("Spectral", "N K nb_iter")


def spectral_cases():
    out = []
    for N in SPECTRAL_N:
        for K in sorted({1, N, N + 3}):
            for it in SPECTRAL_ITERS:
                out.append(Spectral(N, K, it))
    return tuple(out)


def power_trace(x0, taps, nb_iter):
    """The recurrence of power_iter_kernel in longdouble WITHOUT the stop: norms[0] = ||x0||, norms[i] = ||x_i||."""
    x = np.asarray(x0, dtype=LD)[None, :]
    k = np.asarray(taps, dtype=LD)[None, :]
    N = x.shape[1]
    norms = [np.sqrt((x * x).sum())]
    for _ in range(nb_iter):
        a = _cumsum(x, None, False, None)[0]
        b = _toeplitz(k, a, None, N, None, False)[0]
        a = _toeplitz(k, b, None, N, None, True)[0]
        a = _cumsum(a, None, True, None)[0]
        x = a / norms[-1]
        norms.append(np.sqrt((x * x).sum()))
    return norms


def power_result(norms, tol):
    """(rho, steps) of the kernel's loop on a trace."""
    for i in range(1, len(norms)):
        if abs(norms[i] - norms[i - 1]) < tol:
            return norms[i], i
    return norms[-1], len(norms) - 1


def _tol_ok(traces, tol):
    """The reference's criterion stays TOL_MARGIN * tol away from tol at every iteration it evaluates, and tol is far above
    the float64 noise of a norm."""
    for norms in traces:
        if tol < 1.0e-9 * float(max(norms)):
            return False
        for i in range(1, len(norms)):
            d = abs(norms[i] - norms[i - 1])
            if abs(d - tol) < TOL_MARGIN * tol:
                return False
            if d < tol:
                break
    return True


@functools.lru_cache(maxsize=None)
def spectral_reference(case, rows=3):
    """Three start vectors and three HRFs, one tol for the call: {"x0", "taps", "tol", "rho" [rows], "steps" [rows]}."""
    rng = _rng("spectral", case.N, case.K)
    x0 = rng.standard_normal((rows, case.N))
    taps = hrf_like(rng, rows, case.K)
    traces = [power_trace(x0[r], taps[r], case.nb_iter) for r in range(rows)]
    cands = []
    for norms in traces:
        d = [abs(norms[i] - norms[i - 1]) for i in range(1, len(norms))]
        cands += [float(np.sqrt(d[j] * max(d[j + 1], LD(1e-6) * d[j]))) for j in range(len(d) - 1)]
    scale = float(max(max(t) for t in traces))
    cands = sorted(c for c in cands if c > 0) + [1.0e-6 * scale, 1.0e-8 * scale]     # the smallest first: the latest stop
    tol = next((c for c in cands if _tol_ok(traces, c)), None)
    assert tol is not None, case                     # (the host test runs every case)
    res = [power_result(t, tol) for t in traces]
    return {"x0": x0, "taps": taps, "tol": tol, "rho": np.array([r[0] for r in res], dtype=LD),
            "steps": np.array([r[1] for r in res]), "traces": traces}


# ---- pb_inf_norm ---------------------------------------------------------------------------------------------------
INF_NORM_N = (1, 255, 256, 257, 100003)


def inf_norm_inputs(n):
    x = real_rows(_rng("inf_norm", n), 3, n)
    x[1] = 0.0                                           # an all-zero row: 0 / 1e-12
    return x


def inf_norm_reference(x):
    """x / (max|x| + 1e-12): one correctly rounded division per element, so float64 NumPy gives the kernel's bits."""
    return x / (np.abs(x).max(axis=1, keepdims=True) + 1.0e-12)
