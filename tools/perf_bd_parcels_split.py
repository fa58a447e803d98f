"""Time `bd_parcels` (one HRF dilation per parcel) and its z-step at the lengths the split matrix-pipe forms serve by
opt-in (PB_FLAG_GROUPED_SPLIT, force="gsplit"), following the protocol of tools/perf_bd_parcels.py:

  (a) 50 000 voxels x 600 scans, TR 0.75 s, K = 27 (the two-wave form);
  (b) 32 768 voxels x 1 200 scans, TR 0.72 s, a 20 s HRF: K = 28 (an HCP-length run; the four-wave form);

each for G = 1, 100 and 400 parcels of equal size and 400 uneven ones, 20 outer x 100 inner iterations + the closing z-step:

  * `bd_parcels` without the opt-in: every row on the per-problem vector route -- the baseline;
  * `bd_parcels` with force="gsplit";
  * `distributed.bd_shared` (one dilation for all voxels): the floor;

then the z-step alone (`fista_solve_grouped`, 100 iterations, warm-started from zeros) with and without the flag at those
sizes and at 2 048, 4 096 and 8 192 rows (parcels of 128 rows), around the thresholds of the route, and the number of units a
z-step launches against V / 16.

Interleaved rounds in one process (every variant once per round, HIP events around each call after a warm-up); median,
minimum and maximum over the rounds.

    python tools/perf_bd_parcels_split.py [--rounds 5] [--workloads a,b] [--out profiles/parcels_split_timing.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pybold_amd  # noqa: E402
from pybold_amd import data, distributed, solver, spm_hrf  # noqa: E402

WORKLOADS = {"a": dict(V=50_000, N=600, t_r=0.75), "b": dict(V=32_768, N=1200, t_r=0.72)}
DUR, LBDA, NB_ITER, NB_INNER = 20.0, 1.7, 20, 100


def timed_rounds(variants, rounds):
    """{name: times in ms}: every variant once per round, after one warm-up call each."""
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(rounds):
        for name, fn in variants:
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            times[name].append(ev[0].elapsed_time(ev[1]))
    return {k: np.array(v) for k, v in times.items()}


def report(lines, times, per=1, unit="per outer iteration"):
    for name, t in times.items():
        lines.append("  %-44s median %9.3f ms  min %9.3f  max %9.3f  %s %8.3f ms" % (name, np.median(t), t.min(), t.max(), unit, np.median(t) / per))


def workload(tag, V, N, t_r, rounds, lines):
    h_true = spm_hrf(0.7, t_r, DUR, False)[0]
    K = len(h_true)
    Y, _, _ = data.gen_rnd_bloc_bold_batch(V, dur=N * t_r / 60.0, tr=t_r, hrf=h_true, nb_events=10, avg_dur=12.0, std_dur=1.0, snr=10.0, seed=44)
    assert Y.shape == (V, N)
    rng = np.random.RandomState(0)
    groupings = {"G=%d equal" % G: np.arange(V) * G // V for G in (1, 100, 400)}
    cuts = np.sort(rng.choice(np.arange(1, V), size=399, replace=False))
    groupings["G=400 uneven"] = np.searchsorted(cuts, np.arange(V), side="right")
    lines += ["", "workload (%s): V=%d N=%d TR=%.2f K=%d, %d outer x %d inner + closing z-step, %d interleaved rounds, HIP events"
              % (tag, V, N, t_r, K, NB_ITER, NB_INNER, rounds), ""]
    kw = dict(lbda=LBDA, theta_0=2.0, hrf_dur=DUR, nb_iter=NB_ITER, nb_inner=NB_INNER)
    variants = []
    for name, labels in groupings.items():
        sizes = np.bincount(labels)
        off = np.concatenate([[0], np.cumsum(sizes)])
        lines.append("  %-14s parcels of %d .. %d voxels: %d units per z-step (V / 16 = %d); route with the flag (code, main units, row cut): %s"
                     % (name, sizes.min(), sizes.max(), int(np.sum(-(-sizes // 16))), -(-V // 16), solver.grouped_route(off, N, K, "gsplit")))
        for force in (None, "gsplit"):
            variants.append(("bd_parcels %s%s" % (name, " force=gsplit" if force else ""),
                             lambda labels=labels, force=force: pybold_amd.bd_parcels(Y, labels, t_r, force=force, **kw)))
    variants.append(("bd_shared", lambda: distributed.bd_shared(Y, t_r, **kw)))
    lines.append("")
    times = timed_rounds(variants, rounds)
    report(lines, times, NB_ITER + 1)
    lines.append("")
    for name in groupings:
        base, opt = times["bd_parcels %s" % name], times["bd_parcels %s force=gsplit" % name]
        lines.append("  %-14s baseline / opt-in = %.2f (medians); spread of the baseline's rounds %.1f %%, of the opt-in's %.1f %%; opt-in / bd_shared = %.2f"
                     % (name, np.median(base) / np.median(opt), 100 * (base.max() - base.min()) / np.median(base),
                        100 * (opt.max() - opt.min()) / np.median(opt), np.median(opt) / np.median(times["bd_shared"])))
    # the z-step alone: taps of dilations spread over the parcels, 100 iterations from zeros
    lines += ["", "  z-step alone (fista_solve_grouped, %d iterations):" % NB_INNER]
    zvar = []
    cases = [(name, labels, V) for name, labels in groupings.items()]
    cases += [("%d rows, parcels of 128" % rows, np.arange(rows) // 128, rows) for rows in (2048, 4096, 8192)]
    for name, labels, rows in cases:
        sizes = np.bincount(labels)
        po = solver.ParcelOffsets(np.concatenate([[0], np.cumsum(sizes)]), Y.device)
        theta = torch.linspace(0.7, 1.6, po.G, dtype=torch.float64, device=Y.device)
        taps = solver.spm_hrf_batch(theta, t_r, DUR)
        steps = 1.0 / solver.gram_frobenius_batch(taps, N)
        Yr = Y[:rows].contiguous()
        W0 = torch.zeros((rows, N), dtype=torch.float64, device=Y.device)
        for force in (None, "gsplit"):
            zvar.append(("z-step %s%s %s" % (name, " force=gsplit" if force else "", solver.grouped_route(po, N, K, force) if force else ""),
                         lambda Yr=Yr, taps=taps, steps=steps, po=po, W0=W0, force=force: solver.fista_solve_grouped(
                             Yr, taps, steps, po, LBDA, NB_INNER, W0=W0, force=force)))
    ztimes = timed_rounds(zvar, rounds)
    for name, t in ztimes.items():
        lines.append("    %-62s median %8.3f ms  min %8.3f  max %8.3f" % (name, np.median(t), t.min(), t.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workloads", default="a,b")
    ap.add_argument("--out", default=os.path.join("profiles", "parcels_split_timing.txt"))
    args = ap.parse_args()
    dev = solver.device()
    lines = ["perf_bd_parcels_split: %s, %d compute units" % (torch.cuda.get_device_name(dev),
                                                            torch.cuda.get_device_properties(dev).multi_processor_count)]
    for tag in args.workloads.split(","):
        workload(tag, rounds=args.rounds, lines=lines, **WORKLOADS[tag])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
