"""The noise-driven lambda search of deconv(lbda=None): the host-driven loop (`deconv_auto(engine="host")`, the code
`deconv(lbda=None)` runs by default) against the device-resident engine (`engine="device"`), same box, same inputs,
same sigma, interleaved, medians of `--rounds` rounds after a warm-up.  Needs a GPU.

    python tools/perf_auto_lbda.py [--rounds 5] [--out profiles/auto_lbda_device.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/perf_auto_lbda.py --device-only --rounds 1
    python tools/perf_auto_lbda.py --trace DIR --out profiles/auto_lbda_device.txt      (appends the longest kernels)

Inputs: block signals as BASELINE config 3 draws them (`pybold_amd.data.gen_rnd_bloc_bold_batch`, 5 events, SNR 1 dB),
N = 300 scans, the canonical 30-tap HRF.  Points: V in {100, 1 024, 16 384, 100 000} at a (50, 200) budget, and the
full default call (1000 x 1000) at V <= 1 024 (the host loop at 100 000 x default is hours: not run).
Per point: both wall clocks (host clock around the call; the call ends in device->host copies, i.e. synchronised), the
inner iterations the search needed (sum of n_inner) and the voxel-iterations/s that gives, the kernel launches of the
library, and whether both engines agree."""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINTS = [(100, 50, 200), (1024, 50, 200), (16384, 50, 200), (100000, 50, 200), (100, 1000, 1000), (1024, 1000, 1000)]
N_SCANS = 300


def device_launches(V, nb_iter, nb_sub_iter):
    """Launches of pb_auto_lbda_d at its own choice of outer_chunk (include/pybold_hip.h), and that chunk."""
    chunk = max(1, 65536 // (max(nb_sub_iter, 1) * max(1, -(-V // 2048))))
    return -(-nb_iter // chunk) + 1, chunk


def run_points(args):
    import torch
    import pybold_amd
    from pybold_amd import data, solver
    from pybold_amd.hrf_model import spm_hrf
    hrf = spm_hrf(1.0, t_r=1.0, dur=30.0)[0]
    lines = []
    # clocks: half a second of solves before anything is timed
    Yw, _, _ = data.gen_rnd_bloc_bold_batch(16384, dur=N_SCANS / 60.0, tr=1.0, hrf=hrf, snr=1.0, seed=1)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:
        solver.fista_solve(Yw, hrf, 1.0, 1e-6, 200)
        torch.cuda.synchronize()
    for V, nb_iter, nb_sub_iter in POINTS:
        Y, _, _ = data.gen_rnd_bloc_bold_batch(V, dur=N_SCANS / 60.0, tr=1.0, hrf=hrf, snr=1.0, seed=3000 + V)
        sigma = solver.mad_daub_noise_est(Y)
        kw = dict(sigma=sigma, nb_iter=nb_iter, nb_sub_iter=nb_sub_iter)
        engines = ("device",) if args.device_only else ("device", "host")
        times = {e: [] for e in engines}
        last = {}
        for r in range(args.rounds + 1):                        # round 0 warms both engines up and is not counted
            for e in engines:
                np.random.seed(0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[e] = pybold_amd.deconv_auto(Y, 1.0, hrf, engine=e, **kw)
                torch.cuda.synchronize()
                if r > 0 or args.rounds == 0:
                    times[e].append(time.perf_counter() - t0)
        info = last["device"][6]
        n_inner = int(info["n_inner"].sum())
        launches, chunk = device_launches(V, nb_iter, nb_sub_iter)
        t_dev = float(np.median(times["device"]))
        line = ("V %6d  budget %4d x %4d | device %9.4f s (min %.4f max %.4f), %d launches (outer_chunk %d) + outputs, "
                "sum n_inner %.4g, %.3g voxel-iterations/s, n_outer %d..%d"
                % (V, nb_iter, nb_sub_iter, t_dev, min(times["device"]), max(times["device"]), launches, chunk, n_inner,
                   n_inner / t_dev, info["n_outer"].min(), info["n_outer"].max()))
        if not args.device_only:
            hinfo = last["host"][6]
            t_host = float(np.median(times["host"]))
            n_diff = int((info["n_outer"] != hinfo["n_outer"]).sum())
            err = (torch.linalg.norm(last["device"][2] - last["host"][2], dim=1)
                   / (torch.linalg.norm(last["host"][2], dim=1) + 1e-300)).cpu().numpy()
            near_pole = np.minimum(np.abs(info["alpha"]), np.abs(hinfo["alpha"])) < 1e-1
            line += (" | host %9.4f s (min %.4f max %.4f), %d launches (solve + statistics per outer iteration, final solve, "
                     "outputs) and %d synchronising copies, %.3g voxel-iterations/s | host / device %.2fx | agreement: n_outer "
                     "differs on %d voxel(s); rel. difference of diff_z median %.1e, below 1e-9 on %.2f %% of the voxels, worst "
                     "%.1e (final |alpha| < 0.1 on %d voxels; worst among the others %.1e)"
                     % (t_host, min(times["host"]), max(times["host"]), 2 * int(hinfo["n_outer"].max()) + 2,
                        2 * int(hinfo["n_outer"].max()), n_inner / t_host, t_host / t_dev, n_diff, float(np.median(err)),
                        100.0 * float((err < 1e-9).mean()), float(err.max()), int(near_pole.sum()),
                        float(err[~near_pole].max()) if (~near_pole).any() else 0.0))
        print(line, flush=True)
        lines.append(line)
        del Y, last
    return lines


def longest_kernels(trace_dir):
    """Longest single dispatch of auto_lbda_kernel per grid size, from a rocprofv3 kernel trace."""
    best = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "auto_lbda_kernel" not in r["Kernel_Name"]:
                continue
            grid = int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r["Grid_Size"])
            dur = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            n, worst = best.get(grid, (0, 0))
            best[grid] = (n + 1, max(worst, dur))
    return ["longest auto_lbda_kernel dispatch at grid %8d (about %6d voxels): %.4f s over %d dispatches"
            % (grid, grid // 64, worst * 1e-9, n) for grid, (n, worst) in sorted(best.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--trace", default=None, help="rocprofv3 output directory of a --device-only run: append the longest kernels")
    args = ap.parse_args()
    if args.trace:
        lines = ["", "rocprofv3 --kernel-trace --stats of one --device-only run (no counters), library's own outer_chunk:"]
        lines += longest_kernels(args.trace)
        mode = "a"
    else:
        lines = ["tools/perf_auto_lbda.py: deconv_auto(engine='host') -- the loop deconv(lbda=None) runs by default -- against "
                 "engine='device', N = %d, K = 30, block signals at SNR 1 dB, same sigma (computed on the device), "
                 "interleaved, medians of %d rounds after one warm-up round." % (N_SCANS, args.rounds), ""]
        lines += run_points(args)
        mode = "w"
    if args.out:
        with open(args.out, mode) as f:
            f.write("\n".join(lines) + "\n")
    elif args.trace:
        print("\n".join(lines))


if __name__ == "__main__":
    main()
