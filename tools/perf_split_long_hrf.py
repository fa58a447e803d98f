"""The opt-in four-wave float64 register form for HRFs of up to 48 taps (csrc/fista_exact_split_long.h: 641 .. 1 280 scans)
against the route the same call takes without the flag -- the any-size LDS kernel, unchanged code: the yardstick.  Same box,
same process, same inputs, interleaved, medians of `--rounds` rounds after a warm-up round, every point with the spread
(min .. max) of its rounds.  Needs a GPU.

    python tools/perf_split_long_hrf.py [--rounds 5] [--out profiles/split_long_hrf.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/perf_split_long_hrf.py --trace-run
    python tools/perf_split_long_hrf.py --trace DIR --out profiles/split_long_hrf.txt       (appends the longest dispatches)

Points: (1) the fixed-lambda solve, 42 taps at 700 and 1 200 scans, 500 iterations, V in {1, 100, 1 024, 16 384}, one HRF and
one HRF per voxel; (2) the lambda search at a (50, 200) budget, the same V: deconv_auto(engine="device_split_long_hrf") against
the host loop with and without bold_signal.SPLIT_LONG_HRF; (3) the price of the holder and of 16 more taps: 30 taps through
the new form against fista_exact_split_kernel (the default route) / fista_exact_split_pp_kernel (force="split"), which return
the same bits.  A timed window is `reps` calls between two device synchronisations (more calls where one is short).
--trace-run: searches that run every inner iteration (early stopping off, 48 taps, 1 280 scans) at budgets that fill the
library's chunk, for the longest single dispatch."""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ITER = 500
BUDGET = (50, 200)
SCANS = (700, 1200)
VOXELS = (1, 100, 1024, 16384)


def hrf_of(n_taps):
    from pybold_amd.hrf_model import spm_hrf
    h = spm_hrf(1.0, t_r=30.0 / n_taps, dur=30.0)[0][:n_taps]
    assert len(h) == n_taps
    return h


def series(V, n_scans, hrf, seed):
    from pybold_amd import data
    Y, _, _ = data.gen_rnd_bloc_bold_batch(V, dur=(n_scans + 0.5) / 60.0, tr=1.0, hrf=hrf, snr=1.0, seed=seed)
    return Y[:, :n_scans].double().contiguous()


def interleaved(calls, rounds, reps):
    """{name: [seconds per call]} of `rounds` rounds after one warm-up round, the calls alternating within a round."""
    import torch
    times = {k: [] for k in calls}
    for r in range(rounds + 1):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            if r > 0:
                times[k].append((time.perf_counter() - t0) / reps)
    return times


def fmt(ts):
    return "%9.3f ms (%.3f .. %.3f)" % (1e3 * float(np.median(ts)), 1e3 * min(ts), 1e3 * max(ts))


def verdict(new, old):
    """`old / new` of the medians; beyond the spread only when the slowest round of one beats the fastest of the other."""
    ratio = float(np.median(old)) / float(np.median(new))
    if max(new) < min(old):
        return "%.2fx faster, beyond the spread" % ratio
    if max(old) < min(new):
        return "%.2fx: SLOWER, beyond the spread" % ratio
    return "%.2fx: within the spread of the rounds" % ratio


def step_of(hrf, n):
    from pybold_amd.linear import ConvAndLinear, DiscretInteg
    from pybold_amd.utils import spectral_radius_est
    np.random.seed(0)
    return 1.0 / (0.9 * spectral_radius_est(ConvAndLinear(DiscretInteg(), hrf, dim_in=n, dim_out=n), (n,)))


def solve_points(args, n_taps, other, other_pp, other_name):
    import torch
    from pybold_amd import solver
    hrf = hrf_of(n_taps)
    lines = []
    for n_scans in SCANS:
        step = step_of(hrf, n_scans)
        for V in (VOXELS if n_taps > 32 else (1024, 16384)):
            Y = series(V, n_scans, hrf, 4000 + V)
            T = torch.from_numpy(np.repeat(hrf[None, :], V, axis=0)).cuda()
            steps = np.full(V, step)
            reps = 20 if V <= 100 else (4 if V == 1024 else 1)
            for pp in (False, True):
                if pp:
                    def call(force):
                        return solver.fista_solve_pp_d(Y, T, steps, 1.0, N_ITER, force=force)
                else:
                    def call(force):
                        return solver.fista_solve(Y, hrf, 1.0, step, N_ITER, force=force)
                oth = other_pp if pp else other
                t = interleaved({"long": lambda: call("split_long_hrf"), "other": lambda: call(oth)}, args.rounds, reps)
                a, b = call("split_long_hrf")[0], call(oth)[0]
                err = float((torch.linalg.norm(a - b, dim=1) / (torch.linalg.norm(b, dim=1) + 1e-300)).max())
                line = ("N %4d K %2d V %6d %-11s %d iterations | split_long_hrf %s | %s %s | %s | worst rel. difference of W %.1e"
                        % (n_scans, n_taps, V, "per-voxel" if pp else "shared HRF", N_ITER, fmt(t["long"]), other_name,
                           fmt(t["other"]), verdict(t["long"], t["other"]), err))
                print(line, flush=True)
                lines.append(line)
            del Y, T
    return lines


def search_points(args):
    import torch
    import pybold_amd
    from pybold_amd import bold_signal, solver
    hrf = hrf_of(42)
    nb_iter, nb_sub_iter = BUDGET
    lines = []
    for n_scans in SCANS:
        for V in VOXELS:
            Y = series(V, n_scans, hrf, 5000 + V)
            sigma = solver.mad_daub_noise_est(Y)
            last = {}

            def run(engine, switch):
                bold_signal.SPLIT_LONG_HRF = switch
                try:
                    np.random.seed(0)
                    last[(engine, switch)] = pybold_amd.deconv_auto(Y, 1.0, hrf, sigma=sigma, nb_iter=nb_iter, nb_sub_iter=nb_sub_iter,
                                                                    engine=engine)
                finally:
                    bold_signal.SPLIT_LONG_HRF = False
            t = interleaved({"device": lambda: run("device_split_long_hrf", False), "host_long": lambda: run("host", True),
                             "host": lambda: run("host", False)}, args.rounds, 1)
            d, h = last[("device_split_long_hrf", False)], last[("host", False)]
            err = (torch.linalg.norm(d[2] - h[2], dim=1) / (torch.linalg.norm(h[2], dim=1) + 1e-300)).cpu().numpy()
            line = ("N %4d K 42 V %5d budget %d x %d | device_split_long_hrf %s | host loop, SPLIT_LONG_HRF on %s | host loop (today) %s | "
                    "device vs today: %s; host loop with the switch vs today: %s | sum n_inner %.4g, n_outer differs on %d voxel(s), rel. "
                    "difference of diff_z median %.1e, beyond 1e-9 on %d voxel(s)"
                    % (n_scans, V, nb_iter, nb_sub_iter, fmt(t["device"]), fmt(t["host_long"]), fmt(t["host"]),
                       verdict(t["device"], t["host"]), verdict(t["host_long"], t["host"]), int(d[6]["n_inner"].sum()),
                       int((d[6]["n_outer"] != h[6]["n_outer"]).sum()), float(np.median(err)), int((err >= 1e-9).sum())))
            print(line, flush=True)
            lines.append(line)
            del Y
    return lines


def trace_run():
    """Searches that fill the library's chunk: early stopping off, 48 taps, 1 280 scans, 330 x 200 inner iterations per voxel
    (12 x 200 at 16 384 voxels)."""
    import torch
    from pybold_amd import solver
    hrf = hrf_of(48)
    n_scans = 1280
    step = step_of(hrf, n_scans)
    for V in (100, 1024, 16384):
        Y = series(V, n_scans, hrf, 6000 + V)
        sigma = solver.mad_daub_noise_est(Y)
        nb_iter = 330 if V <= 1024 else 12
        solver.auto_lbda_solve_split_long(Y, hrf, step, sigma, early_stopping=False, nb_iter=nb_iter, nb_sub_iter=200, want_trace=False)
        T = torch.from_numpy(np.repeat(hrf[None, :], V, axis=0)).cuda()
        solver.auto_lbda_solve_split_long_pp(Y, T, np.full(V, step), sigma, early_stopping=False, nb_iter=nb_iter, nb_sub_iter=200,
                                             want_trace=False)
        torch.cuda.synchronize()
        print("traced N %d V %d" % (n_scans, V), flush=True)


def longest_kernels(trace_dir):
    """Longest single dispatch of the four-wave long-HRF search kernels per kernel and grid size, from a rocprofv3 kernel trace."""
    best = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            if "auto_lbda_split_long" not in name:
                continue
            kind = "auto_lbda_split_long_pp_kernel" if "auto_lbda_split_long_pp" in name else "auto_lbda_split_long_kernel"
            grid = int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r["Grid_Size"])
            dur = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            n, worst = best.get((kind, grid), (0, 0))
            best[(kind, grid)] = (n + 1, max(worst, dur))
    return ["longest %-30s dispatch at grid %8d (%6d voxels): %.4f s over %d dispatches" % (k, grid, grid // 256, w * 1e-9, n)
            for (k, grid), (n, w) in sorted(best.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--trace", default=None, help="rocprofv3 output directory of a --trace-run: append the longest dispatches")
    args = ap.parse_args()
    if args.trace_run:
        return trace_run()
    if args.trace:
        lines = ["", "rocprofv3 --kernel-trace --stats of one --trace-run (no counters): 48 taps, 1 280 scans, early stopping off, 330 x 200 "
                 "inner iterations per voxel (12 x 200 at 16 384 voxels), the library's own outer_chunk:"]
        lines += longest_kernels(args.trace)
        mode = "a"
    else:
        assert args.rounds >= 5, "medians of at least five rounds"
        lines = ["tools/perf_split_long_hrf.py: the four-wave float64 register form for HRFs of up to 48 taps (pb_fista_solve_split_long_d, "
                 "pb_auto_lbda_split_long_d) against the same call on the default entry point (the LDS kernel), block signals at SNR 1 dB, "
                 "interleaved, medians (min .. max) of %d rounds after one warm-up round, per call." % args.rounds, "",
                 "(1) fixed-lambda solve, 42 taps:"]
        lines += solve_points(args, 42, None, None, "no flag (LDS kernel)")
        lines += ["", "(2) lambda search, 42 taps:"]
        lines += search_points(args)
        lines += ["", "(3) the price of the holder and of 16 more taps: 30 taps through the new form against fista_exact_split_kernel "
                  "(no flag) / fista_exact_split_pp_kernel (force='split'), the same bits:"]
        lines += solve_points(args, 30, None, "split", "four-wave KT=32")
        mode = "w"
    if args.out:
        with open(args.out, mode) as f:
            f.write("\n".join(lines) + "\n")
    elif args.trace:
        print("\n".join(lines))


if __name__ == "__main__":
    main()
