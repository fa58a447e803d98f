"""The noise-driven lambda search of deconv(lbda=None) on series of 641 .. 1 280 scans: the host-driven loop
(`deconv_auto(engine="host")`, unchanged code: the yardstick) against the device-resident engine with one voxel per
workgroup of four waves (`engine="device_split"`), same box, same inputs, same sigma, interleaved, medians of
`--rounds` rounds after a warm-up.  Needs a GPU.

    python tools/perf_auto_lbda_split.py [--rounds 5] [--out profiles/auto_lbda_split.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/perf_auto_lbda_split.py --device-only --rounds 1
    python tools/perf_auto_lbda_split.py --trace DIR --out profiles/auto_lbda_split.txt      (appends the longest kernels)

Inputs: block signals (`pybold_amd.data.gen_rnd_bloc_bold_batch`, 5 events, SNR 1 dB), 700 scans with the canonical
30-tap HRF and 1 200 scans with a 28-tap one, V in {100, 1 024, 16 384} at a (50, 200) budget.
Per point: both wall clocks (host clock around the call; the call ends in device->host copies, i.e. synchronised), the
inner iterations the search needed, the kernel launches of the library with its own outer_chunk, and whether both engines
agree (relative difference of diff_z per voxel: median, and the count beyond 1e-9)."""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(700, 30, 1.0), (1200, 28, 30.0 / 28)]            # (scans, taps, TR of the HRF)
BATCHES = [100, 1024, 16384]
BUDGET = (50, 200)


def split_launches(V, nb_iter, nb_sub_iter):
    """Launches of pb_auto_lbda_split_d at its own choice of outer_chunk (include/pybold_hip.h), and that chunk."""
    chunk = max(1, 32768 // (max(nb_sub_iter, 1) * max(1, -(-V // 512))))
    return -(-nb_iter // chunk) + 1, chunk


def run_points(args):
    import torch
    import pybold_amd
    from pybold_amd import data, solver
    from pybold_amd.hrf_model import spm_hrf
    lines = []
    nb_iter, nb_sub_iter = BUDGET
    for n_scans, n_taps, t_r in SHAPES:
        hrf = spm_hrf(1.0, t_r=t_r, dur=30.0)[0][:n_taps]
        assert len(hrf) == n_taps and solver.auto_lbda_split_supported(n_scans, n_taps)
        for V in BATCHES:
            Y, _, _ = data.gen_rnd_bloc_bold_batch(V, dur=(n_scans + 0.5) / 60.0, tr=1.0, hrf=hrf, snr=1.0, seed=3000 + V)
            Y = Y[:, :n_scans].double().contiguous()
            sigma = solver.mad_daub_noise_est(Y)
            kw = dict(sigma=sigma, nb_iter=nb_iter, nb_sub_iter=nb_sub_iter)
            engines = ("device_split",) if args.device_only else ("device_split", "host")
            times = {e: [] for e in engines}
            last = {}
            for r in range(args.rounds + 1):                    # round 0 warms both engines up and is not counted
                for e in engines:
                    np.random.seed(0)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[e] = pybold_amd.deconv_auto(Y, 1.0, hrf, engine=e, **kw)
                    torch.cuda.synchronize()
                    if r > 0 or args.rounds == 0:
                        times[e].append(time.perf_counter() - t0)
            info = last["device_split"][6]
            n_inner = int(info["n_inner"].sum())
            launches, chunk = split_launches(V, nb_iter, nb_sub_iter)
            t_dev = float(np.median(times["device_split"]))
            line = ("N %4d V %6d  budget %3d x %3d | device_split %9.4f s (min %.4f max %.4f), %d launches (outer_chunk %d) + "
                    "outputs, sum n_inner %.4g, %.3g voxel-iterations/s, n_outer %d..%d"
                    % (n_scans, V, nb_iter, nb_sub_iter, t_dev, min(times["device_split"]), max(times["device_split"]), launches,
                       chunk, n_inner, n_inner / t_dev, info["n_outer"].min(), info["n_outer"].max()))
            if not args.device_only:
                hinfo = last["host"][6]
                t_host = float(np.median(times["host"]))
                n_diff = int((info["n_outer"] != hinfo["n_outer"]).sum())
                err = (torch.linalg.norm(last["device_split"][2] - last["host"][2], dim=1)
                       / (torch.linalg.norm(last["host"][2], dim=1) + 1e-300)).cpu().numpy()
                near_pole = np.minimum(np.abs(info["alpha"]), np.abs(hinfo["alpha"])) < 1e-1
                line += (" | host %9.4f s (min %.4f max %.4f), %d launches (solve + statistics per outer iteration, final solve, "
                         "outputs) and %d synchronising copies | host / device_split %.2fx%s | agreement: n_outer differs on %d "
                         "voxel(s); rel. difference of diff_z median %.1e, beyond 1e-9 on %d voxel(s), worst %.1e (final |alpha| "
                         "< 0.1 on %d voxels; worst among the others %.1e)"
                         % (t_host, min(times["host"]), max(times["host"]), 2 * int(hinfo["n_outer"].max()) + 2,
                            2 * int(hinfo["n_outer"].max()), t_host / t_dev, "" if t_host >= t_dev else " (SLOWER than the host loop)",
                            n_diff, float(np.median(err)), int((err >= 1e-9).sum()), float(err.max()), int(near_pole.sum()),
                            float(err[~near_pole].max()) if (~near_pole).any() else 0.0))
            print(line, flush=True)
            lines.append(line)
            del Y, last
    return lines


def longest_kernels(trace_dir):
    """Longest single dispatch of auto_lbda_split_kernel per grid size, from a rocprofv3 kernel trace."""
    best = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "auto_lbda_split_kernel" not in r["Kernel_Name"]:
                continue
            grid = int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r["Grid_Size"])
            dur = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            n, worst = best.get(grid, (0, 0))
            best[grid] = (n + 1, max(worst, dur))
    return ["longest auto_lbda_split_kernel dispatch at grid %8d (%6d voxels, both lengths): %.4f s over %d dispatches"
            % (grid, grid // 256, worst * 1e-9, n) for grid, (n, worst) in sorted(best.items())]


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
        lines = ["tools/perf_auto_lbda_split.py: deconv_auto(engine='host') -- the loop deconv(lbda=None) runs by default -- against "
                 "engine='device_split' (one voxel per workgroup of four waves), block signals at SNR 1 dB, same sigma (computed on "
                 "the device), interleaved, medians of %d rounds after one warm-up round." % args.rounds, ""]
        lines += run_points(args)
        mode = "w"
    if args.out:
        with open(args.out, mode) as f:
            f.write("\n".join(lines) + "\n")
    elif args.trace:
        print("\n".join(lines))


if __name__ == "__main__":
    main()
