"""A/B timing of alternative builds of libpybold_hip.so (PYBOLD_HIP_LIB).  Each build is timed in a fresh process per
round, the builds alternating, so that drift of the box hits them alike; per shape the script reports min and median
over several launches and a checksum of the result.

    python tools/ab_kernel.py [--rounds R] [--shapes config3,n600,n1200,l640,l1200,z300,z600,z1200] <lib A> <lib B> ...

Shapes: config3 = 100 000 x 300 scans x 500 iterations (PYBOLD_AB_FORCE picks the form, default "fast1");
n600 / n1200 = the matrix-pipe forms over two / four waves (32 768 / 16 384 series, 200 iterations);
l640 / l1200 = the same with the _loops_deconv rule (tol 1e-3; through fista_solve: its allocations are in the time);
z300 / z600 / z1200 = the shared-HRF z-step (fista_solve_pp, taps and step from device memory, 100 iterations, warm).
(These run without the re-solve of what a guard hands back: the matrix-pipe kernels alone are timed.)
At the end: per shape the per-round medians of every build, and -- the first build being the baseline -- whether each
other build's median of medians lies within the baseline's own spread (max - min of its per-round medians)."""
import argparse
import os
import subprocess
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--shapes", default="config3")
ap.add_argument("libs", nargs="+")
args = ap.parse_args()
code = r'''
import os, sys, time, numpy as np, torch
sys.path.insert(0, ".")
from pybold_amd import solver
from pybold_amd.hrf_model import spm_hrf
hrf = spm_hrf(1.0, t_r=1.0, dur=30.)[0]
def timed(launch, result, reps=12, warm=3):
    for _ in range(warm): launch()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); launch(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return "min %.3f ms  median %.3f ms  checksum %.10e" % (min(ts), float(np.median(ts)), float(result().abs().sum()))
for shape in sys.argv[1].split(","):
    torch.manual_seed(0)
    if shape == "config3":
        Y = torch.randn(100000, 300, device="cuda", dtype=torch.float32)
        plan = solver.FistaPlan(Y, hrf, 1.0, 1.0 / 723876.27, 500, force=os.environ.get("PYBOLD_AB_FORCE", "fast1"))
        out = timed(plan.run, lambda: plan.W)
    elif shape[0] == "n":
        N = int(shape[1:])
        Y = torch.randn(32768 if N <= 640 else 16384, N, device="cuda", dtype=torch.float32)
        plan = solver.FistaPlan(Y, hrf, 1.0, 1.0 / (8.1 * N * N), 200, force="mfma2only" if N <= 640 else "noresolve")
        out = timed(plan.run, lambda: plan.W)
    elif shape[0] == "l":
        N = int(shape[1:])
        Y = torch.randn(32768 if N <= 640 else 16384, N, device="cuda", dtype=torch.float32)
        res = [None]
        def launch():
            res[0] = solver.fista_solve(Y, hrf, 1.0, 1.0 / (8.1 * N * N), 200, stop="loops", tol=1.0e-3,
                                        force="mfma2only" if N <= 640 else "noresolve")[0]
        out = timed(launch, lambda: res[0])
    else:
        N = int(shape[1:])
        Y = torch.randn(32768 if N <= 640 else 16384, N, device="cuda", dtype=torch.float32)
        taps = torch.from_numpy(np.asarray(hrf, dtype=np.float64)).cuda()
        steps = torch.tensor([1.0 / (8.1 * N * N)], dtype=torch.float64, device="cuda")
        W = torch.zeros(Y.shape, dtype=torch.float64, device="cuda")
        def launch():
            solver.fista_solve_pp(Y, taps, steps, 1.0, 100, W0=W, inplace=True, force="intermediate_noresolve")
        out = timed(launch, lambda: W)
    print("%s: %s" % (shape, out), flush=True)
'''
medians = {}
for rnd in range(args.rounds):
    for lib in args.libs:
        env = dict(os.environ)
        if lib != "default":
            env["PYBOLD_HIP_LIB"] = os.path.abspath(lib)
        out = subprocess.run([sys.executable, "-c", code, args.shapes], env=env, capture_output=True, text=True)
        if out.returncode != 0:                      # nothing more is started on the GPU after a failure
            print("%-28s round %d: exit %d: %s" % (lib, rnd, out.returncode, out.stderr.strip()[-300:]), flush=True)
            sys.exit(1)
        for line in out.stdout.strip().splitlines():
            print("%-28s round %d: %s" % (lib, rnd, line), flush=True)
            medians.setdefault(line.split(":")[0], {}).setdefault(lib, []).append(float(line.split("median ")[1].split()[0]))
for shape, by_lib in medians.items():
    base = by_lib[args.libs[0]]
    spread = max(base) - min(base)
    for lib in args.libs:
        m = by_lib[lib]
        verdict = "" if lib == args.libs[0] else ("  within the baseline's median + spread: %s" % (
            "yes" if np.median(m) <= np.median(base) + spread else "NO"))
        print("%-8s %-28s medians %s  median %.3f  spread %.3f%s" % (
            shape, lib, " ".join("%.3f" % x for x in m), float(np.median(m)), max(m) - min(m), verdict))
