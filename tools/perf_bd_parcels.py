"""Time `bd_parcels` (one HRF dilation per parcel) on BASELINE config 4's workload -- 50 000 voxels x 300 scans, TR 0.75 s,
K = 27, 20 outer x 100 inner iterations + the closing z-step -- for G = 1, 100, 400 and 3 125 parcels of equal size and
one run with uneven sizes, against

  * the same call with force="valu": every row on the per-problem vector route with its parcel's taps (what the library
    could do before the grouped z-step: the parcel's taps spread over its voxels into pb_fista_solve_pp);
  * `bd` on the 2-D batch (blind.bd_batch: one dilation per voxel); its `nb_iter` is the number of outer AND of inner
    iterations, so it runs 100 outer iterations of 100 and is compared per outer iteration;
  * `distributed.bd_shared` (one dilation for all voxels): the floor, G = 1 should sit near it.

Interleaved rounds in one process (every variant once per round, HIP events around each call after a warm-up); median
and min over the rounds, per call and per outer iteration (call / 21; bd: call / 101).  Also the number of matrix-pipe
waves a z-step launches against V / 16.

    python tools/perf_bd_parcels.py [--rounds 5] [--voxels 50000] [--out profiles/bd_parcels.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pybold_amd  # noqa: E402
from pybold_amd import blind, data, distributed, solver, spm_hrf  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--voxels", type=int, default=50_000)
    ap.add_argument("--out", default=os.path.join("profiles", "bd_parcels.txt"))
    args = ap.parse_args()
    dev = solver.device()
    V, t_r, dur, lbda, nb_iter, nb_inner = args.voxels, 0.75, 20.0, 1.7, 20, 100
    h_true = spm_hrf(0.7, t_r, dur, False)[0]
    Y, _, _ = data.gen_rnd_bloc_bold_batch(V, dur=3.75, tr=t_r, hrf=h_true, nb_events=5, avg_dur=12.0, std_dur=1.0, snr=10.0, seed=44)
    N = Y.shape[1]
    rng = np.random.RandomState(0)
    groupings = {}
    for G in (1, 100, 400, 3125):
        groupings["G=%d equal" % G] = np.arange(V) * G // V
    cuts = np.sort(rng.choice(np.arange(1, V), size=399, replace=False))            # 400 parcels, sizes drawn unevenly
    groupings["G=400 uneven"] = np.searchsorted(cuts, np.arange(V), side="right")
    variants = []
    waves = {}
    for name, labels in groupings.items():
        sizes = np.bincount(labels)
        waves[name] = (int(np.sum(-(-sizes // 16))), int(sizes.min()), int(sizes.max()))
        for force in (None, "valu"):
            variants.append(("bd_parcels %s%s" % (name, " force=valu" if force else ""), nb_iter + 1,
                             lambda labels=labels, force=force: pybold_amd.bd_parcels(Y, labels, t_r, lbda=lbda, theta_0=2.0, hrf_dur=dur,
                                                                                      nb_iter=nb_iter, nb_inner=nb_inner, force=force)))
    variants.append(("bd_shared", nb_iter + 1,
                     lambda: distributed.bd_shared(Y, t_r, lbda=lbda, theta_0=2.0, hrf_dur=dur, nb_iter=nb_iter, nb_inner=nb_inner)))
    variants.append(("bd 2-D (100 outer x 100)", 101, lambda: blind.bd_batch(Y, t_r, lbda=lbda, theta_0=2.0, hrf_dur=dur, nb_iter=100)))
    lines = ["perf_bd_parcels: V=%d N=%d K=%d, %d outer x %d inner + closing z-step, %d interleaved rounds, HIP events; %s"
             % (V, N, len(h_true), nb_iter, nb_inner, args.rounds, torch.cuda.get_device_name(dev)), ""]
    for name, (w, lo, hi) in waves.items():
        lines.append("  %-14s parcels of %d .. %d voxels: %d matrix-pipe waves per z-step (V / 16 = %d)" % (name, lo, hi, w, -(-V // 16)))
    lines.append("")
    for _, _, fn in variants:                     # warm-up: code objects, caches
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(args.rounds):
        for name, _, fn in variants:
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            times[name].append(ev[0].elapsed_time(ev[1]))
    med = {}
    for name, outer, _ in variants:
        t = np.array(times[name])
        med[name] = float(np.median(t)) / outer
        lines.append("  %-40s median %9.2f ms  min %9.2f ms  per outer iteration %8.3f ms" % (name, np.median(t), t.min(), med[name]))
    lines.append("")
    for name in groupings:
        a = med["bd_parcels %s" % name]
        lines.append("  %-14s per outer iteration: force=valu / default = %.2f, bd 2-D / default = %.2f, default / bd_shared = %.2f"
                     % (name, med["bd_parcels %s force=valu" % name] / a, med["bd 2-D (100 outer x 100)"] / a, a / med["bd_shared"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
