"""Inputs and float64 references of the parcel tests on the SPLIT matrix-pipe forms (tests/test_parcel_split_host.py,
tests/test_gpu_parcels_split.py): the grouped z-step with PB_FLAG_GROUPED_SPLIT at 311 .. 1 280 scans.

The layout (ten parcels, four of them empty with NaN taps, 84 rows), the HRFs with gains from 2^-10 to 300 and both
signs, the cold and warm cases and their oracle iterates are those of tests/parcel_cases.py (`z_step_case`); here are the
shapes -- the first and the last length of every compiled instance, at the edges of both tile counts --, the hand-back
case, and the routing rule of csrc/dispatch.h (`route_grouped`) restated.

A plain helper module: no fixtures, no pytest configuration.  Nothing here touches the library under test."""
import functools

import numpy as np

from oracle import c_oracle
from oracle import pybold_oracle as orc
from tests import parcel_cases as pc

# ---- the instances: (first, last) length of launch_mfma2_grouped<NBA, NBB> and launch_mfma4_grouped<A> ------------------
TWO_WAVE = {(5, 5): (311, 320)}                      # ten blocks of 32 samples: 289 .. 320 fit, the route sends 311+ here
TWO_WAVE.update({((nb) // 2, (nb + 1) // 2): (32 * (nb - 1) + 1, 32 * nb) for nb in range(11, 21)})
FOUR_WAVE = {a: (128 * (a - 1) + 1, 128 * a) for a in range(6, 11)}
TAPS = (1, 33, 34, 48)                               # two near tiles at both edges, three at both edges of what the route serves
LOWER = [r[0] for r in list(TWO_WAVE.values()) + list(FOUR_WAVE.values())]
UPPER = [r[1] for r in list(TWO_WAVE.values()) + list(FOUR_WAVE.values())]
# (N, K, variant): "cold" at both lengths, "warm" at the upper one
CASES = ([(n, k, "cold") for n in sorted(LOWER + UPPER) for k in TAPS] + [(n, k, "warm") for n in UPPER for k in TAPS])
BIT_SHAPES = [(n, k) for n in UPPER for k in (33, 48)]
LAYOUT_SHAPES = [(352, 33), (352, 48), (768, 33), (768, 48)]
HANDBACK_SHAPES = [(352, 27), (768, 27), (352, 40), (768, 40)]
HANDBACK_FRACTIONS = (0.01, 0.9)                     # of a row's own lambda_max: even rows, odd rows
HANDBACK_RATIO_EVEN_MAX, HANDBACK_RATIO_ODD_MIN = 0.005, 0.08      # MFMA_RHO_MAX = 0.02 (csrc/mfma_core.h): four times inside, four times outside


def case(N, K, variant):
    return pc.z_step_case(N, K, variant)


@functools.lru_cache(maxsize=None)
def handback_case(N, K):
    """The layout of parcel_cases with `parcel_taps`, Y standard normal from seed 7919 N + 31 K + 1, a cold start and one
    lambda per row: 0.01 x its own lambda_max on even rows (far inside the accuracy guard of the matrix pipe), 0.9 x on odd
    rows (far outside: the matrix-pipe forms hand those back).  The reference: `c_oracle.fista_batch` parcel by parcel."""
    taps, steps, gains = pc.parcel_taps(K, N)
    rng = np.random.RandomState(7919 * N + 31 * K + 1)
    Y = rng.randn(pc.ROWS, N).astype(np.float32)
    Yd = Y.astype(np.float64)
    lbda = np.empty(pc.ROWS)
    ref = np.empty((pc.ROWS, N))
    frac = np.where(np.arange(pc.ROWS) % 2 == 0, HANDBACK_FRACTIONS[0], HANDBACK_FRACTIONS[1])
    for g in pc.NONEMPTY:
        r0, r1 = int(pc.OFFSETS[g]), int(pc.OFFSETS[g + 1])
        lbda[r0:r1] = frac[r0:r1] * orc.lambda_max(Yd[r0:r1], taps[g])
        ref[r0:r1] = c_oracle.fista_batch(Yd[r0:r1], taps[g], lbda[r0:r1].copy(), float(steps[g]), pc.N_ITER, W0=None, threads=1)[0]
    for a in (Y, lbda, ref):
        a.setflags(write=False)
    return dict(N=N, K=K, variant="cold", Y=Y, taps=taps, steps=steps, gains=gains, offsets=pc.OFFSETS, lbda=lbda, lbda_rows=lbda,
                W0=None, ref=ref, n_iter=pc.N_ITER)


def guard_ratios(c):
    """lambda step / max|w_ref| of every row (what the accuracy guard of the matrix pipe compares with MFMA_RHO_MAX)."""
    return c["lbda_rows"] * c["steps"][pc.row_parcel()] / np.maximum(np.abs(c["ref"]).max(axis=1), 1e-300)


# ---- the route of pb_fista_solve_grouped restated (csrc/dispatch.h: route_grouped) ----------------------------------------
FORCE_MFMA, ONE_LAUNCH, NO_MFMA, GROUPED_SPLIT, NO_RESOLVE = 16384, 32, 8192, 8388608, 2048
HOST_WAVE_SLOTS = 2048                               # wave_slots() without a device: 256 compute units x 4 SIMDs x 2
ONE_WAVE_MIN_ROWS = 4096                             # GROUPED_MFMA_MIN_P
WIDE_TAPS_MAX = 48                                   # the one-problem-per-wave table ends here (csrc/wide_table.inc)


def units_of(sizes):
    return [-(-int(n) // 16) for n in sizes]


def row_of_unit(sizes, unit):
    """First row of unit `unit` of the table; the number of rows if there is no such unit."""
    off, u = 0, 0
    for n, k in zip(sizes, units_of(sizes)):
        if u + k > unit:
            return off + (unit - u) * 16
        off, u = off + int(n), u + k
    return off


def expected_route(sizes, N, K, flags, wave_slots=HOST_WAVE_SLOTS):
    """`(code, main_units, row_cut)` by the rules of the header and DESIGN 6, for flags out of FORCE_MFMA, ONE_LAUNCH,
    NO_MFMA, GROUPED_SPLIT, NO_RESOLVE."""
    P, units = int(sum(sizes)), sum(units_of(sizes))
    forced = bool(flags & FORCE_MFMA)
    one = forced or bool(flags & ONE_LAUNCH)
    split = bool(flags & GROUPED_SPLIT) and N > 310
    if flags & NO_MFMA:
        served = False
    elif not split:
        served = 129 <= N <= 310 and 1 <= K <= 33
    else:
        served = N <= 1280 and 1 <= K <= WIDE_TAPS_MAX
    if not served:
        return (-1 if forced else 0), 0, 0
    main = units
    if not split:
        if not forced and P < ONE_WAVE_MIN_ROWS:
            main = 0
        elif not one:
            rnd = wave_slots // 2
            whole = units // rnd * rnd
            if 0 < whole < units and P - row_of_unit(sizes, whole) <= ONE_WAVE_MIN_ROWS:
                main = whole
    elif not forced:
        four = N > 640
        pass_units = wave_slots // (8 if four else 4)
        whole = units // pass_units * pass_units
        rem = units - whole
        keep = one or (16 * rem > 10 * pass_units if four else 16 * rem > 5 * pass_units)     # above 10/16 or 5/16 of a pass
        if not four and 16 * units < (2048 if K > 33 else 5120):
            main = 0
        elif not four and whole == 0:
            main = units                             # meets the minimum, fills no pass: one partial pass
        else:
            main = units if keep else whole
    if main == 0:
        return 0, 0, 0
    return (4 if not split else 6 if N > 640 else 5), main, (P if main == units else row_of_unit(sizes, main))
