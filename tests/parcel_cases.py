"""Inputs and float64 references of the parcel tests at every compiled variant (tests/test_parcel_cases_host.py,
tests/test_gpu_parcels_variants.py): one layout of parcels with empty ones at every kind of place, one HRF per parcel
with gains that differ by orders of magnitude and in sign, the grouped z-step's cold and warm cases with the oracle's
iterate per parcel, the parcel layouts of the grouped normal equations, and the two host rules of
pb_hrf_normal_eq_w_grouped restated.

The conditions the z-step cases must meet -- no zero reference row, every row four times inside the matrix pipe's
accuracy guard, a last tap that matters -- are properties of the ORACLE's output; tests/test_parcel_cases_host.py
asserts them for every shape listed here, without a GPU.  If a shape misses one, give it another seed (`SEED_BUMP`);
the conditions stay.

A plain helper module: no fixtures, no pytest configuration.  Nothing here touches the library under test."""
import functools

import numpy as np

from oracle import c_oracle
from oracle import pybold_oracle as orc

# ---- the parcel layout: G = 10, 84 rows, 9 waves; empty parcels first, last and as two neighbours in the middle ------
SIZES = [0, 1, 15, 0, 0, 16, 17, 33, 2, 0]
OFFSETS = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
ROWS = int(OFFSETS[-1])
NONEMPTY = [g for g, n in enumerate(SIZES) if n > 0]
THETAS = [0.7, 1.0, 1.3, 1.6, 2.0, 0.85]             # one dilation and one gain per non-empty parcel, in their order
GAINS = [1.0, -1.0, 2.0 ** -10, 300.0, 0.37, 5.0]
SHORT_BASE = [0.0, 0.6, 0.3, 0.1, 0.05, 0.02, 0.01]    # K < 8: its first K entries ([0.8] for K = 1)
N_ITER = 60
LBDA_FRACTION = 0.01                                 # of lambda_max
GUARD_RATIO_MAX = 0.005                              # lambda step / max|w_ref|: a quarter of MFMA_RHO_MAX = 0.02 (csrc/mfma_core.h)
TAIL_SHARE_MIN = 0.01                                # |h[K - 1]| / max|h|
SEED_BUMP = {}                                       # (N, K) -> added to the seed, for a shape that misses a condition

# ---- the shapes of tests/test_gpu_parcels_variants.py ----------------------------------------------------------------
NB_RANGE = {5: (129, 155), 6: (156, 186), 7: (187, 217), 8: (218, 248), 9: (249, 279), 10: (280, 310)}      # 31 (NB - 1) < N <= 31 NB
INSTANCE_SHAPES = ([(n, k) for nb in sorted(NB_RANGE) for n in NB_RANGE[nb] for k in (1, 32, 33)]
                   + [(155, 2), (156, 2), (155, 17), (156, 17)])
BIT_SHAPES = [(n, k) for nb in sorted(NB_RANGE) for n in NB_RANGE[nb] for k in (32, 33)]
RECORDED_SHAPE = (150, 27)                            # where profiles/bd_parcels.txt records equality with the shared form
LAYOUT_SHAPES = [(NB_RANGE[nb][1], 33 if nb % 2 else 32) for nb in sorted(NB_RANGE)]
ROUTE_SHAPES = [(129, 1), (155, 33), (310, 32)]
VECTOR_SHAPES = [(128, 33), (311, 33), (150, 34), (31, 4), (600, 40)]      # no matrix-pipe form
ALL_Z_SHAPES = sorted(set(INSTANCE_SHAPES + BIT_SHAPES + [RECORDED_SHAPE] + LAYOUT_SHAPES + ROUTE_SHAPES + VECTOR_SHAPES))
VARIANTS = ("cold", "warm")


def row_parcel():
    """The parcel of every row."""
    return np.repeat(np.arange(len(SIZES)), SIZES)


@functools.lru_cache(maxsize=None)
def parcel_taps(K, N):
    """`(taps (G, K), steps (G,), gains (G,))`, float64: one HRF per non-empty parcel -- a two-gamma HRF of K seconds at
    TR 1 s for K >= 8, the first K of SHORT_BASE below --, a ramp of 5 % of its peak added with the parcel's sign so that
    the last tap matters, times the parcel's gain; the step 1 / ||A^T A||_F in float64 NumPy (what
    pybold/bold_signal.py:249-254 computes; `orc.gram_lipschitz`), independent of the library's gram_frobenius_batch.
    Empty parcels hold NaN everywhere: nothing may read them."""
    G = len(SIZES)
    taps = np.full((G, K), np.nan)
    steps = np.full((G,), np.nan)
    gains = np.full((G,), np.nan)
    for j, g in enumerate(NONEMPTY):
        if K >= 8:
            base = orc.spm_hrf(THETAS[j], 1.0, float(K), False)[0][:K]
        else:
            base = np.array([0.8] if K == 1 else SHORT_BASE[:K])
        assert base.shape == (K,)
        h = base + 0.05 * np.abs(base).max() * (-1.0) ** g * np.linspace(0.0, 1.0, K)
        taps[g] = GAINS[j] * h
        gains[g] = GAINS[j]
        steps[g] = 1.0 / orc.gram_lipschitz(taps[g], N)
    for a in (taps, steps, gains):
        a.setflags(write=False)
    return taps, steps, gains


@functools.lru_cache(maxsize=None)
def z_step_case(N, K, variant):
    """A grouped z-step on the layout SIZES with the oracle's iterate after N_ITER iterations.  Y: 84 x N standard
    normal rounded through float32.  "cold": one lambda, 0.01 x the smallest lambda_max of the rows (every row with its
    parcel's HRF), no start values.  "warm": lambda per row, 0.01 x its own lambda_max, start values
    0.01 randn / |gain of the row's parcel|.  The reference: `c_oracle.fista_batch` parcel by parcel."""
    assert variant in VARIANTS
    taps, steps, gains = parcel_taps(K, N)
    rng = np.random.RandomState(7919 * N + 31 * K + SEED_BUMP.get((N, K), 0))
    Y = rng.randn(ROWS, N).astype(np.float32)
    W0_all = 0.01 * rng.randn(ROWS, N) / np.abs(gains[row_parcel()])[:, None]
    Yd = Y.astype(np.float64)
    lmax = np.empty(ROWS)
    for g in NONEMPTY:
        r0, r1 = int(OFFSETS[g]), int(OFFSETS[g + 1])
        lmax[r0:r1] = orc.lambda_max(Yd[r0:r1], taps[g])
    if variant == "cold":
        lbda, W0 = LBDA_FRACTION * float(lmax.min()), None
    else:
        lbda, W0 = LBDA_FRACTION * lmax, W0_all
    lbda_rows = np.broadcast_to(np.asarray(lbda, dtype=np.float64), (ROWS,))
    ref = np.empty((ROWS, N))
    for g in NONEMPTY:
        r0, r1 = int(OFFSETS[g]), int(OFFSETS[g + 1])
        ref[r0:r1] = c_oracle.fista_batch(Yd[r0:r1], taps[g], float(lbda) if variant == "cold" else lbda_rows[r0:r1].copy(),
                                          float(steps[g]), N_ITER, W0=None if W0 is None else W0[r0:r1], threads=1)[0]
    for a in (Y, ref, lmax) + (() if W0 is None else (W0,)) + (() if variant == "cold" else (lbda,)):
        a.setflags(write=False)
    return dict(N=N, K=K, variant=variant, Y=Y, taps=taps, steps=steps, gains=gains, offsets=OFFSETS, lbda=lbda,
                lbda_rows=lbda_rows, W0=W0, ref=ref, n_iter=N_ITER)


def input_conditions(case):
    """The three figures the conditions are on: `(smallest row norm of the reference, largest lambda step / max|w_ref|
    over the rows, smallest |h[K - 1]| / max|h| over the HRFs)`."""
    rp = row_parcel()
    ref = case["ref"]
    norms = np.linalg.norm(ref, axis=1)
    ratio = case["lbda_rows"] * case["steps"][rp] / np.maximum(np.abs(ref).max(axis=1), 1e-300)
    h = case["taps"][NONEMPTY]
    tail = np.abs(h[:, -1]) / np.abs(h).max(axis=1)
    return float(norms.min()), float(ratio.max()), float(tail.min())


# ---- the grouped normal equations: host rules restated, parcel layouts -----------------------------------------------
NE_UNITS, NE_MIN_ROWS = 1024, 16                     # NE_GROUPED_UNITS, NE_GROUPED_MIN_ROWS (csrc/capi.hip)
NE_LDS_DOUBLES_MAX = 20000                           # LDS_DOUBLES_MAX (csrc/capi.hip)


def ne_len(K):
    """Entries of one set as pb_hrf_normal_eq_w_grouped stores it: G [K][K], b [K], yy, ||w||_1."""
    return K * K + K + 2


def ne_rows_per_unit(V):
    """ne_grouped_rows of csrc/capi.hip: about 1 024 workgroups, 16 rows at least each."""
    return max(NE_MIN_ROWS, -(-V // NE_UNITS))


def ne_work_len(V, G, K):
    """ne_grouped_work of csrc/capi.hip (doubles), with grouped_max_units of csrc/plan.h:339."""
    max_units = V // ne_rows_per_unit(V) + G
    return (G + 2 + 3 * max_units + 1) // 2 + max_units * ne_len(K)


def reduce_e_log2(max_units, G, ne):
    """e_log2 in pb_hrf_normal_eq_w_grouped, csrc/capi.hip: entries per workgroup of the second stage from the largest
    parcel's units, raised until the grid stays within 2^16 workgroups."""
    e = 8 if max_units <= 4 else (6 if max_units <= 16 else (4 if max_units <= 64 else (2 if max_units <= 256 else 0)))
    while e < 8 and G * ((ne + (1 << e) - 1) >> e) > 65536:
        e += 1
    return e


def _ne_sk(i):
    return i + (i >> 3)                              # csrc/blind.h:125


def ne_wave_lds_doubles(N, K):
    """csrc/blind.h:346-351 (four waves per workgroup, NE_LB = NE_JB = 8)."""
    return 4 * (_ne_sk(N + 16) + 1 + _ne_sk(N + K + 16) + 1) + K * K + 2 * K + 2


def ne_sum_lds_doubles(N, K):
    """csrc/blind.h:127-129."""
    return _ne_sk(N + 16) + 1 + _ne_sk(N + K + 16) + 1 + K * K + 2 * 8 * 16 + 2 * K + 16


def ne_kernel(N, K):
    """Which of the three kernels pb_hrf_normal_eq_w_grouped launches (its `wave_form` and the launch below it in csrc/capi.hip; ne_wave_form)."""
    if K <= 32 and ne_wave_lds_doubles(N, K) <= NE_LDS_DOUBLES_MAX:
        return "register" if K * K <= 64 * 12 and N <= 64 * 5 else "wave"
    return "sum"


def smallest_sum_form_scans(K):
    """The first N at which K <= 32 taps leave the wave form because its LDS does not fit."""
    N = 1
    while ne_wave_lds_doubles(N, K) <= NE_LDS_DOUBLES_MAX:
        N += 1
    return N


NE_SUM_BELOW_33 = (smallest_sum_form_scans(32), 32)   # (2069, 32): 20 002 doubles; 2 068 scans take 19 994
NE_KERNEL_SHAPES = [(150, 27), (150, 28), (321, 27), (150, 32), (150, 33), (40, 1), NE_SUM_BELOW_33]
NE_FRAMED_SHAPES = [(150, 28), (150, 33)]
NE_LADDER = [64, 65, 256, 257, 1024, 1025, 4096, 4097]       # the largest parcel's rows, N = 40, K = 5


def ne_ladder_sizes(big):
    return [1, 0, big, 70]


def ne_raised_sizes():
    """One parcel of 4 097 rows (257 units: e_log2 = 0) and 99 of 1 .. 3 rows: G ne = 100 x 758 > 65 536 at K = 27."""
    return [4097] + [1 + (g % 3) for g in range(99)]


NE_UNIT20_SIZES = [9999, 1, 10000]                    # V = 20 000: units of 20 rows

# (name, sizes, N, K) of every reduce case of section 4
NE_REDUCE_CASES = ([("ladder-%d" % b, ne_ladder_sizes(b), 40, 5) for b in NE_LADDER]
                   + [("raised", ne_raised_sizes(), 150, 27), ("unit20", NE_UNIT20_SIZES, 40, 5)])


def ne_case_e_log2(sizes, K):
    """`(e_log2 before the raise, e_log2 launched, rows per unit)` of a layout."""
    per = ne_rows_per_unit(int(sum(sizes)))
    max_units = max(-(-int(n) // per) for n in sizes)
    return reduce_e_log2(max_units, 0, ne_len(K)), reduce_e_log2(max_units, len(sizes), ne_len(K)), per


@functools.lru_cache(maxsize=None)
def ne_case(sizes, N, K, seed=3):
    """`(W float64 (V, N) at 10 % density, Y float32 (V, N), ref (G, K K + K + 2))`: the reference from
    `orc.hrf_normal_eq(cumsum(W_g), Y_g, K)` and `abs(W_g).sum()` parcel by parcel, zeros for an empty parcel."""
    sizes = list(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    V = int(off[-1])
    rng = np.random.RandomState(seed + 7919 * N + 31 * K + V)
    W = (rng.rand(V, N) < 0.1) * rng.randn(V, N)
    Y = rng.randn(V, N).astype(np.float32)
    ref = np.zeros((len(sizes), ne_len(K)))
    for g in range(len(sizes)):
        r0, r1 = int(off[g]), int(off[g + 1])
        if r1 > r0:
            Gm, b, yy = orc.hrf_normal_eq(np.cumsum(W[r0:r1], axis=1), Y[r0:r1].astype(np.float64), K)
            ref[g] = np.concatenate([Gm.ravel(), b, [yy, np.abs(W[r0:r1]).sum()]])
    for a in (W, Y, ref):
        a.setflags(write=False)
    return W, Y, ref, off
