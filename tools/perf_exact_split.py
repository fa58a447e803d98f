"""The four-wave float64 form (fista_exact_split_kernel, 641 .. 1 280 scans) against the PARENT COMMIT's library, which ran
these calls on the any-size LDS kernel: same box, same inputs, both libraries timed in the same run, alternating, medians
of `--rounds` rounds after a warm-up round, with the spread.  Needs a GPU and a build of the parent commit's library:

    git worktree add /some/dir HEAD~1 && make -C /some/dir/pybold_amd/csrc      (or any other build of the parent)
    python tools/perf_exact_split.py --baseline /some/dir/pybold_amd/libpybold_hip.so [--rounds 5] [--out profiles/exact_split.txt]

The baseline is NOT this tree's `force="generic"`: it is the parent's own dispatch.  One worker process per library (a
fresh child each; `PYBOLD_HIP_LIB` selects the library), both alive for the whole run; the parent process hands out one
point and one round at a time, to one worker after the other.

Points: float64 `fista_solve`, 500 iterations, at 700 and 1 200 scans x {1, 100, 1 024, 16 384} voxels; the 1-D `deconv` of
the `hcp` series of tests/golden/long_series.npz (1 200 scans, 28 taps; 100 iterations, lambda 0.5); `deconv(lbda=None)` at a
(50, 200) budget on 1 024 voxels x 1 200 scans; the default float32 `fista_solve` on the 1 200-scan batch of sixteen
ill-conditioned families (tests/test_gpu_exact_split.py), 4 112 rows, 500 iterations."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

POINTS = ([("solve", n, v) for n in (700, 1200) for v in (1, 100, 1024, 16384)]
          + [("deconv1d", 1200, 1), ("auto", 1200, 1024), ("ill", 1200, 4112)])


def describe(p):
    kind, n, v = p
    return {"solve": "float64 fista_solve, 500 iterations, %4d scans x %5d voxels" % (n, v),
            "deconv1d": "1-D deconv of the hcp series (1 200 scans, 28 taps), 100 iterations",
            "auto": "deconv(lbda=None), budget (50, 200), 1 024 voxels x 1 200 scans",
            "ill": "float32 fista_solve (default dispatch), 16 ill-conditioned families, 4 112 rows x 1 200 scans, 500 iterations"}[kind]


def worker():
    """Reads point indices from stdin, one per line; times that point once; answers with one JSON line."""
    from pybold_amd import _lib
    if os.environ.get("PB_PERF_BASELINE"):
        _lib.SIGNATURES.pop("pb_fista_which_kernel_d", None)         # (the parent's library does not have the query)
    import torch
    import pybold_amd
    from oracle import pybold_oracle as orc
    from pybold_amd import data, solver
    prepared = {}

    def prepare(p):
        kind, n, v = p
        if kind == "solve":
            hrf = orc.spm_hrf(1.0, 1.0, 28.0, False)[0][:28].copy()
            Y = data.gen_rnd_bloc_bold_batch(v, dur=(n + 0.5) / 60.0, tr=1.0, hrf=hrf, snr=1.0, seed=n + v)[0][:, :n].double().contiguous()
            step = 1.0 / orc.gram_lipschitz(hrf, n)
            return lambda: solver.fista_solve(Y, hrf, 0.5, step, 500)
        g = np.load(os.path.join(ROOT, "tests", "golden", "long_series.npz"))
        y, hrf, t_r = g["hcp_y"], g["hcp_hrf"], float(g["hcp_t_r"])
        if kind == "deconv1d":
            return lambda: pybold_amd.deconv(y, t_r, hrf, lbda=0.5, nb_iter=100, early_stopping=False)
        if kind == "auto":
            Y = data.gen_rnd_bloc_bold_batch(v, dur=(n + 0.5) / 60.0, tr=t_r, hrf=hrf, snr=1.0, seed=7)[0][:, :n].double().contiguous()
            sigma = solver.mad_daub_noise_est(Y)
            return lambda: pybold_amd.deconv_auto(Y, t_r, hrf, sigma=sigma, nb_iter=50, nb_sub_iter=200, engine="host")
        from test_gpu_exact_split import _ill_families
        hrf = orc.spm_hrf(1.0, 1.0, 28.0, False)[0][:28].copy()
        ordinary = data.gen_rnd_bloc_bold_batch(1, dur=(n + 0.5) / 60.0, tr=1.0, hrf=hrf, snr=1.0, seed=3)[0][0, :n].double().cpu().numpy()
        fams = _ill_families(n, ordinary)
        Y = torch.from_numpy(np.tile(fams, (v // len(fams), 1)).astype(np.float32)).cuda()
        step = 1.0 / orc.gram_lipschitz(hrf, n)
        return lambda: solver.fista_solve(Y, hrf, 1.0, step, 500)

    import warnings
    warnings.simplefilter("ignore")
    print(json.dumps({"ready": _lib.LIB_PATH}), flush=True)
    for line in sys.stdin:
        i = int(line)
        if i not in prepared:
            prepared[i] = prepare(POINTS[i])
        np.random.seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prepared[i]()
        torch.cuda.synchronize()
        print(json.dumps({"point": i, "seconds": time.perf_counter() - t0}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", help="libpybold_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker()
    if not args.baseline or not os.path.exists(args.baseline):
        sys.exit("--baseline: a build of the parent commit's libpybold_hip.so is required")
    procs = {}
    for name, env in (("parent", dict(os.environ, PYBOLD_HIP_LIB=os.path.abspath(args.baseline), PB_PERF_BASELINE="1")),
                      ("this tree", {k: v for k, v in os.environ.items() if k != "PYBOLD_HIP_LIB"})):
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], env=env, stdin=subprocess.PIPE,
                                       stdout=subprocess.PIPE, text=True)
        print(name, json.loads(procs[name].stdout.readline())["ready"], flush=True)

    def once(name, i):
        procs[name].stdin.write("%d\n" % i)
        procs[name].stdin.flush()
        line = procs[name].stdout.readline()
        if not line:
            raise RuntimeError("the worker of %s ended (exit status %s)" % (name, procs[name].poll()))
        return json.loads(line)["seconds"]

    lines = ["tools/perf_exact_split.py: the parent commit's library (LDS kernel for float64 calls beyond 640 scans) against this "
             "tree's (fista_exact_split_kernel), one worker process each, alternating, medians of %d rounds after one warm-up "
             "round; min .. max in brackets." % args.rounds, ""]
    try:
        for i, p in enumerate(POINTS):
            times = {name: [] for name in procs}
            for r in range(args.rounds + 1):
                for name in procs:
                    t = once(name, i)
                    if r > 0:
                        times[name].append(t)
            med = {name: float(np.median(t)) for name, t in times.items()}
            sep = min(times["parent"]) > max(times["this tree"])
            line = ("%-110s | parent %9.4f s [%.4f .. %.4f] | this tree %9.4f s [%.4f .. %.4f] | parent / this tree %6.2fx | %s"
                    % (describe(p), med["parent"], min(times["parent"]), max(times["parent"]), med["this tree"],
                       min(times["this tree"]), max(times["this tree"]), med["parent"] / med["this tree"],
                       "faster beyond the spread" if sep else "NOT separated from the parent by the spread"))
            print(line, flush=True)
            lines.append(line)
    finally:
        for pr in procs.values():
            pr.stdin.close()
            pr.wait(timeout=60)
    lines += ["", "A layout of two waves x 10 samples per lane: not measured."]
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
