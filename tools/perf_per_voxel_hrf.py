"""Rates of the float64 solver with one HRF per voxel (fista_exact_pp_kernel, csrc/fista_exact_pp.h) beside the two kernels
it is to be compared with, on the same data in the same process, alternating, medians of `--rounds` rounds after a warm-up
round, timed with device events around each call.  Needs a GPU.

    python tools/perf_per_voxel_hrf.py [--rounds 7] [--voxels 16384] [--out profiles/per_voxel_hrf.txt]

Points: 16 384 voxels x 500 iterations at 300 and 600 scans, 30 taps, no stop rule, no cost trace:
  pp       solver.fista_solve_pp_d(force="fast")     fista_exact_pp_kernel: taps and step of every voxel from device memory
  shared   solver.fista_solve(float64 Y, force="fast")  fista_exact_kernel: one HRF for all, taps by value -- the rows of `pp` hold
           that same HRF, so both solve the same problems (the outputs are compared bit for bit)
  lds      solver.fista_solve_pp_d(force="generic")  the LDS kernel with per-problem taps, the only route that could have served
           this call before
and the per-voxel lambda search (`deconv_auto` with a 2-D hrf, a different HRF per voxel) at a (50, 200) budget, window rules on
at the default tol = 1e-6: engine "device" (auto_lbda_pp_kernel) against engine "host".  The register reports of the build
(csrc/build/exactpp_*.res, exact_*.res where `make build/exact_<S>_<KT>.s` has left them) are printed beside the rates."""
import argparse
import glob
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1.0e-3, out


def interleaved(calls, rounds, reps=1):
    """{name: [seconds per call and round]} after one warm-up round, the calls alternating within every round, `reps` calls
    back to back per timed window (a solve of a few milliseconds alone measures the clock ramp as much as the kernel); last outputs."""
    times, outs = {k: [] for k in calls}, {}
    for r in range(rounds + 1):
        for name, fn in calls.items():
            t, out = timed(lambda: [fn() for _ in range(reps)])
            outs[name] = out[-1]
            if r > 0:
                times[name].append(t / reps)
    return times, outs


def register_report():
    lines = []
    for path in sorted(glob.glob(os.path.join(ROOT, "pybold_amd", "csrc", "build", "exact*_*_*.res"))):
        if "exactsplit" in path:
            continue
        text = open(path).read()
        for m in re.finditer(r"Function Name: (\S+).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                             r"Occupancy \[waves/SIMD\]: (\d+)", text, flags=re.S):
            t = re.search(r"kernelILi(\d+)ELi(\d+)ELb([01])ELi(\d)E", m.group(1))
            if t and t.group(3) == "0" and t.group(4) == "0":          # the variant timed here: no cost trace, no stop rule
                lines.append("  %-22s S=%-2s KT=%s: %3s VGPRs, %3s SGPRs, scratch %s, %s waves/SIMD"
                             % (os.path.basename(path), t.group(1), t.group(2), m.group(3), m.group(2), m.group(4), m.group(5)))
    return lines or ["  (no register reports in csrc/build)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--voxels", type=int, default=16384)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import warnings

    import torch
    import pybold_amd
    from oracle import pybold_oracle as orc
    from pybold_amd import data, solver
    warnings.simplefilter("ignore")
    V, K, n_iter = args.voxels, 30, 500
    lines = ["tools/perf_per_voxel_hrf.py: %d voxels, %d taps, one process, calls alternating, medians of %d rounds after one warm-up "
             "round [min .. max], 20 solves back to back per timed window (one search per window); rates in voxel-iterations per "
             "second." % (V, K, args.rounds), ""]
    hrf = orc.spm_hrf(1.0, 1.0, float(K), False)[0][:K].copy()
    for n in (300, 600):
        Y = data.gen_rnd_bloc_bold_batch(V, dur=(n + 0.5) / 60.0, tr=1.0, hrf=hrf, snr=1.0, seed=n)[0][:, :n].double().contiguous()
        step = 1.0 / orc.gram_lipschitz(hrf, n)
        T = torch.from_numpy(hrf).cuda().repeat(V, 1).contiguous()
        steps = torch.full((V,), step, dtype=torch.float64, device="cuda")
        calls = {"pp": lambda: solver.fista_solve_pp_d(Y, T, steps, 0.5, n_iter, force="fast")[0],
                 "shared": lambda: solver.fista_solve(Y, hrf, 0.5, step, n_iter, force="fast")[0],
                 "lds": lambda: solver.fista_solve_pp_d(Y, T, steps, 0.5, n_iter, force="generic")[0]}
        times, outs = interleaved(calls, args.rounds, reps=20)
        same = bool(torch.equal(outs["pp"], outs["shared"]))
        e_lds = float(((outs["lds"] - outs["pp"]).norm(dim=1) / (outs["pp"].norm(dim=1) + 1e-300)).max())
        med = {k: float(np.median(t)) for k, t in times.items()}
        for k, what in (("pp", "fista_exact_pp_kernel"), ("shared", "fista_exact_kernel (taps by value)"), ("lds", "LDS kernel, per-problem taps")):
            line = ("%4d scans  %-36s %9.4f s [%.4f .. %.4f]  %.3e voxel-iterations/s"
                    % (n, what, med[k], min(times[k]), max(times[k]), V * n_iter / med[k]))
            print(line, flush=True)
            lines.append(line)
        line = ("%4d scans  pp / shared time %.3f; lds / pp time %.2f; pp equals shared bit for bit: %s; lds against pp, worst row %.1e"
                % (n, med["pp"] / med["shared"], med["lds"] / med["pp"], same, e_lds))
        print(line, flush=True)
        lines += [line, ""]

    # the lambda search, one HRF per voxel
    n = 300
    deltas = torch.linspace(0.6, 1.9, V, dtype=torch.float64, device="cuda")
    T = solver.spm_hrf_batch(deltas, 1.0, float(K))
    T = (T / T.abs().amax(dim=1, keepdim=True))[:, :K].contiguous()
    Y = data.gen_rnd_bloc_bold_batch(V, dur=(n + 0.5) / 60.0, tr=1.0, hrf=hrf, snr=1.0, seed=7)[0][:, :n].double().contiguous()
    sigma = solver.mad_daub_noise_est(Y)

    def search(engine):
        np.random.seed(0)
        return pybold_amd.deconv_auto(Y, 1.0, T, sigma=sigma, nb_iter=50, nb_sub_iter=200, engine=engine)
    times, outs = interleaved({"device": lambda: search("device"), "host": lambda: search("host")}, min(args.rounds, 3))
    med = {k: float(np.median(t)) for k, t in times.items()}
    same_outer = bool(np.array_equal(outs["device"][6]["n_outer"], outs["host"][6]["n_outer"]))
    e = float(((outs["device"][2] - outs["host"][2]).norm(dim=1) / (outs["host"][2].norm(dim=1) + 1e-300)).max())
    for k in ("device", "host"):
        line = ("deconv_auto, 2-D hrf, %d voxels x %d scans, budget (50, 200), tol 1e-6: engine %-6s %9.4f s [%.4f .. %.4f], %d inner iterations"
                % (V, n, k, med[k], min(times[k]), max(times[k]), int(outs[k][6]["n_inner"].sum())))
        print(line, flush=True)
        lines.append(line)
    line = "host / device time %.2f; n_outer equal on every voxel: %s; diff_z device against host, worst voxel %.1e" % (
        med["host"] / med["device"], same_outer, e)
    print(line, flush=True)
    lines += [line, "", "register reports (the variant timed above: no cost trace, no stop rule):"] + register_report()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
