"""Rates of the opt-in four-wave float64 solver with one HRF per voxel (fista_exact_split_pp_kernel,
csrc/fista_exact_split_pp.h) beside the two kernels it is to be compared with, on the same data in the same process,
alternating, medians of `--rounds` rounds after a warm-up round, timed with device events around each call (the method of
tools/perf_per_voxel_hrf.py).  Needs a GPU.

    python tools/perf_per_voxel_split.py [--rounds 7] [--out profiles/per_voxel_split.txt]

Points: 1, 100, 1 024 and 16 384 voxels x 500 iterations at 700 and 1 200 scans, 30 taps, no stop rule, no cost trace:
  split    solver.fista_solve_pp_d(force="split")    fista_exact_split_pp_kernel: taps and step of every voxel from device memory
  lds      solver.fista_solve_pp_d(force="generic")  the LDS kernel with the same per-voxel taps: what serves the call without
           the opt-in
  shared   solver.fista_solve(float64 Y)             fista_exact_split_kernel: one HRF for all, taps by value -- the rows of `split`
           hold that same HRF, so both solve the same problems (the outputs are compared bit for bit)
and the per-voxel lambda search (`deconv_auto` with a 2-D hrf, a different HRF per voxel) at a (50, 200) budget, window rules on
at the default tol = 1e-6, 1 024 voxels: engine "device_split_pp" (auto_lbda_split_pp_kernel) against engine "host" (inner solves
on the LDS kernel) and against engine "host" with PER_VOXEL_SPLIT on (inner solves on fista_exact_split_pp_kernel).  "beyond
the spread" = the slower call's fastest round is slower than the faster call's slowest round.  The register reports of the
build (csrc/build/exactsplitpp_*.res, autosplitpp_*.res) are printed beside the rates."""
import argparse
import glob
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from perf_per_voxel_hrf import interleaved  # noqa: E402


def register_report():
    lines = []
    for path in sorted(glob.glob(os.path.join(ROOT, "pybold_amd", "csrc", "build", "*splitpp_*_*.res"))):
        text = open(path).read()
        for m in re.finditer(r"Function Name: (\S+).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                             r"Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", text, flags=re.S):
            t = re.search(r"(fista_exact_split_pp|auto_lbda_split_pp)_kernelILi(\d+)ELi(\d+)E(?:Lb([01])E)?Li(\d)E", m.group(1))
            if t:
                what = "%s<S=%s, KT=%s%s, STOP=%s>" % (t.group(1), t.group(2), t.group(3),
                                                       "" if t.group(4) is None else ", WITH_J=%s" % t.group(4), t.group(5))
                lines.append("  %-58s %3s VGPRs, %3s SGPRs, scratch %s, LDS %s B, %s waves/SIMD"
                             % (what, m.group(3), m.group(2), m.group(4), m.group(6), m.group(5)))
    return lines or ["  (no register reports in csrc/build)"]


def verdict(fast, slow):
    return "beyond the spread" if min(slow) > max(fast) else "WITHIN the spread of the rounds"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import warnings

    import torch
    import pybold_amd
    from oracle import pybold_oracle as orc
    from pybold_amd import bold_signal, data, solver
    warnings.simplefilter("ignore")
    K, n_iter = 30, 500
    lines = ["tools/perf_per_voxel_split.py: %d taps, %d iterations, one process, calls alternating, medians of %d rounds after one "
             "warm-up round [min .. max], 5 solves back to back per timed window (one search per window); rates in voxel-iterations "
             "per second." % (K, n_iter, args.rounds), ""]
    hrf = orc.spm_hrf(1.0, 1.0, float(K), False)[0][:K].copy()
    for n in (700, 1200):
        Yall = data.gen_rnd_bloc_bold_batch(16384, dur=(n + 0.5) / 60.0, tr=1.0, hrf=hrf, snr=1.0, seed=n)[0][:, :n].double().contiguous()
        step = 1.0 / orc.gram_lipschitz(hrf, n)
        for V in (1, 100, 1024, 16384):
            Y = Yall[:V].contiguous()
            T = torch.from_numpy(hrf).cuda().repeat(V, 1).contiguous()
            steps = torch.full((V,), step, dtype=torch.float64, device="cuda")
            calls = {"split": lambda: solver.fista_solve_pp_d(Y, T, steps, 0.5, n_iter, force="split")[0],
                     "lds": lambda: solver.fista_solve_pp_d(Y, T, steps, 0.5, n_iter, force="generic")[0],
                     "shared": lambda: solver.fista_solve(Y, hrf, 0.5, step, n_iter)[0]}
            times, outs = interleaved(calls, args.rounds, reps=5)
            same = bool(torch.equal(outs["split"], outs["shared"]))
            e_lds = float(((outs["lds"] - outs["split"]).norm(dim=1) / (outs["split"].norm(dim=1) + 1e-300)).max())
            med = {k: float(np.median(t)) for k, t in times.items()}
            for k, what in (("split", "fista_exact_split_pp_kernel"), ("lds", "LDS kernel, per-problem taps"),
                            ("shared", "fista_exact_split_kernel (taps by value)")):
                line = ("%4d scans x %5d voxels  %-42s %9.5f s [%.5f .. %.5f]  %.3e voxel-iterations/s"
                        % (n, V, what, med[k], min(times[k]), max(times[k]), V * n_iter / med[k]))
                print(line, flush=True)
                lines.append(line)
            line = ("%4d scans x %5d voxels  lds / split time %.2f (%s); split / shared time %.3f (%s); split equals shared bit for "
                    "bit: %s; lds against split, worst row %.1e"
                    % (n, V, med["lds"] / med["split"],
                       verdict(times["split"], times["lds"]) if med["lds"] > med["split"] else "split SLOWER, " + verdict(times["lds"], times["split"]),
                       med["split"] / med["shared"],
                       verdict(times["shared"], times["split"]) if med["split"] > med["shared"] else verdict(times["split"], times["shared"]),
                       same, e_lds))
            print(line, flush=True)
            lines += [line, ""]

    # the lambda search, one HRF per voxel
    V = 1024
    for n in (700, 1200):
        deltas = torch.linspace(0.6, 1.9, V, dtype=torch.float64, device="cuda")
        T = solver.spm_hrf_batch(deltas, 1.0, float(K))
        T = (T / T.abs().amax(dim=1, keepdim=True))[:, :K].contiguous()
        Y = data.gen_rnd_bloc_bold_batch(V, dur=(n + 0.5) / 60.0, tr=1.0, hrf=hrf, snr=1.0, seed=7)[0][:, :n].double().contiguous()
        sigma = solver.mad_daub_noise_est(Y)

        def search(engine, pp_split=False):
            np.random.seed(0)
            bold_signal.PER_VOXEL_SPLIT = pp_split
            try:
                return pybold_amd.deconv_auto(Y, 1.0, T, sigma=sigma, nb_iter=50, nb_sub_iter=200, engine=engine)
            finally:
                bold_signal.PER_VOXEL_SPLIT = False
        times, outs = interleaved({"device_split_pp": lambda: search("device_split_pp"), "host": lambda: search("host"),
                                   "host+split": lambda: search("host", True)}, min(args.rounds, 3))
        med = {k: float(np.median(t)) for k, t in times.items()}
        for k in ("device_split_pp", "host", "host+split"):
            line = ("deconv_auto, 2-D hrf, %d voxels x %d scans, budget (50, 200), tol 1e-6: engine %-15s %9.4f s [%.4f .. %.4f], %d inner "
                    "iterations" % (V, n, k, med[k], min(times[k]), max(times[k]), int(outs[k][6]["n_inner"].sum())))
            print(line, flush=True)
            lines.append(line)
        d = outs["device_split_pp"]
        for k in ("host", "host+split"):
            same_outer = bool(np.array_equal(d[6]["n_outer"], outs[k][6]["n_outer"]))
            e = float(((d[2] - outs[k][2]).norm(dim=1) / (outs[k][2].norm(dim=1) + 1e-300)).max())
            line = "%s / device_split_pp time %.2f (%s); n_outer equal on every voxel: %s; diff_z device against %s, worst voxel %.1e" % (
                k, med[k] / med["device_split_pp"],
                verdict(times["device_split_pp"], times[k]) if med[k] > med["device_split_pp"] else "device SLOWER, " + verdict(times[k], times["device_split_pp"]),
                same_outer, k, e)
            print(line, flush=True)
            lines.append(line)
        lines.append("")
    lines += ["register reports:"] + register_report()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
