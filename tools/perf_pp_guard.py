"""Price of the opt-in conditioning guard on the solves whose HRF lives in device memory (profiles/pp_guard.txt).

Workloads: BASELINE config 4 (50 000 voxels x 300 scans, 100 inner iterations) -- one shared-HRF z-step, one grouped z-step
with 400 parcels, the loops bd_shared and bd_parcels (20 x 100) -- and one shared-HRF z-step of 32 768 x 1 200 scans.
Legs, interleaved round by round (one leg after the other inside a round, so that drift hits them alike):
  off    guard=False (what the entry points enqueue without the switch)
  on/b   guard=True, block signals at SNR 1 dB: nothing is marked -- the marks pass, the list build, the empty re-solves
  on/c   guard=True, pure white noise: the worst case
Medians and min .. max over the rounds, HIP events around each call; the marked counts of the guarded legs.

Leg (a), guard off against the PARENT commit: `--parent-lib PATH` names a build of the parent's library (its capi.hip
compiled as it was, linked with the same kernel objects).  A library is loaded once per process, so the off legs of both
builds run in child processes of this tool, alternating parent / this build round by round; each child reports the median
of its own repeats, the table shows the median and spread of those over the rounds for either build.

    python tools/perf_pp_guard.py [--rounds 7] [--loops] [--parent-lib libpybold_hip_parent.so] > profiles/pp_guard.txt
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pybold_oracle as orc  # noqa: E402
from pybold_amd import _lib  # noqa: E402

if os.environ.get("PYBOLD_HIP_LIB"):               # a child on the parent's build: bind what that build exports
    _have = ctypes.CDLL(_lib.LIB_PATH)
    for _name in [n for n in _lib.SIGNATURES if not hasattr(_have, n)]:
        del _lib.SIGNATURES[_name]

from pybold_amd import data, distributed, parcels, solver  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def report(name, legs, rounds):
    times = {k: [] for k in legs}
    counts = {}
    for k, fn in legs.items():                     # warm-up: caches, work buffers
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in legs.items():
            ms, out = timed(fn)
            times[k].append(ms)
            if out is not None:
                counts[k] = out()
    base = float(np.median(times["off"]))
    for k in legs:
        t = np.array(times[k])
        print("%-34s %-5s median %9.3f ms  (min %9.3f .. max %9.3f, %d rounds)  x %.3f of off  %s"
              % (name, k, np.median(t), t.min(), t.max(), rounds, np.median(t) / base, counts.get(k, "")))
    sys.stdout.flush()


def z_step_legs(Yb, Yn, hrf, n_iter, grouped=None):
    V, N = Yb.shape
    dev = Yb.device
    taps = torch.from_numpy(hrf).to(dev)
    step = torch.tensor([1.0 / orc.gram_lipschitz(hrf, N)], dtype=torch.float64, device=dev)
    W = torch.zeros((V, N), dtype=torch.float64, device=dev)
    work = torch.empty((solver.guard_work_len(V, N),), dtype=torch.int32, device=dev)
    if grouped is None:
        def run(Y, guard):
            solver.fista_solve_pp(Y, taps, step, 1.0, n_iter, W0=W, inplace=True, guard_work=work, guard=guard)
            return (lambda: solver.guard_counts(work)) if guard else None
    else:
        po = solver.ParcelOffsets(grouped, dev)
        tg, sg = taps.reshape(1, -1).repeat(po.G, 1).contiguous(), step.repeat(po.G).contiguous()
        gw = torch.empty((int(solver._lib.load().pb_fista_grouped_work_len(V, po.G, len(hrf))),), dtype=torch.int32, device=dev)

        def run(Y, guard):
            solver.fista_solve_grouped(Y, tg, sg, po, 1.0, n_iter, W0=W, inplace=True, work=gw, guard_work=work, guard=guard)
            return (lambda: solver.guard_counts(work)) if guard else None
    return {"off": lambda: run(Yb, False), "on/b": lambda: run(Yb, True), "off/c": lambda: run(Yn, False), "on/c": lambda: run(Yn, True)}


def off_legs(V, loops):
    """name -> callable of every workload's guard-off leg on block signals, through the calls without the keyword."""
    dev = solver.device()
    hrf = orc.spm_hrf(1.0, 1.0, 20.0, False)[0][:20].copy()
    hrf28 = orc.spm_hrf(1.0, 1.0, 28.0, False)[0][:28].copy()
    Yb, _, _ = data.gen_rnd_bloc_bold_batch(V, dur=300.5 / 60.0, tr=1.0, hrf=hrf, nb_events=5, avg_dur=12.0, std_dur=1.0, snr=1.0, seed=4,
                                            device=dev)
    Yl, _, _ = data.gen_rnd_bloc_bold_batch(32768, dur=1200.5 / 60.0, tr=1.0, hrf=hrf28, nb_events=5, avg_dur=12.0, std_dur=1.0, snr=1.0,
                                            seed=5, device=dev)
    legs = {}

    def z_shared(Y, h):
        taps = torch.from_numpy(h).to(dev)
        step = torch.tensor([1.0 / orc.gram_lipschitz(h, Y.shape[1])], dtype=torch.float64, device=dev)
        W = torch.zeros(Y.shape, dtype=torch.float64, device=dev)
        return lambda: solver.fista_solve_pp(Y, taps, step, 1.0, 100, W0=W, inplace=True)
    legs["z-step shared %d x 300 x 100" % V] = z_shared(Yb, hrf)
    po = solver.ParcelOffsets(np.linspace(0, V, 401).astype(np.int64), dev)
    tg = torch.from_numpy(hrf).to(dev).reshape(1, -1).repeat(po.G, 1).contiguous()
    sg = torch.full((po.G,), 1.0 / orc.gram_lipschitz(hrf, 300), dtype=torch.float64, device=dev)
    Wg = torch.zeros(Yb.shape, dtype=torch.float64, device=dev)
    gw = torch.empty((int(_lib.load().pb_fista_grouped_work_len(V, po.G, 20)),), dtype=torch.int32, device=dev)
    legs["z-step 400 parcels %d x 300 x 100" % V] = lambda: solver.fista_solve_grouped(Yb, tg, sg, po, 1.0, 100, W0=Wg, inplace=True, work=gw)
    legs["z-step shared 32768 x 1200 x 100"] = z_shared(Yl, hrf28)
    if loops:
        labels = np.repeat(np.arange(400), -(-V // 400))[:V]
        kw = dict(lbda=1.0, theta_0=2.0, hrf_dur=20.0, nb_iter=20, nb_inner=100)
        legs["bd_shared 20 x 100, %d x 300" % V] = lambda: distributed.bd_shared(Yb, 1.0, **kw)
        legs["bd_parcels 400 parcels 20 x 100, %d x 300" % V] = lambda: parcels.bd_parcels(Yb, labels, 1.0, **kw)
    return legs


def child_off(V, loops, repeats):
    out = {}
    for name, fn in off_legs(V, loops).items():
        fn()
        torch.cuda.synchronize()
        out[name] = float(np.median([timed(fn)[0] for _ in range(repeats)]))
    print("CHILD " + json.dumps(out))


def against_parent(parent_lib, V, loops, rounds):
    res = {"parent": {}, "this": {}}
    for _ in range(rounds):
        for which in ("parent", "this"):
            env = dict(os.environ)
            env.pop("PYBOLD_HIP_LIB", None)
            if which == "parent":
                env["PYBOLD_HIP_LIB"] = os.path.abspath(parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--child-off", "--voxels", str(V)] + (["--loops"] if loops else [])
            txt = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=300).stdout
            line = [ln for ln in txt.splitlines() if ln.startswith("CHILD ")][-1]
            for name, ms in json.loads(line[6:]).items():
                res[which].setdefault(name, []).append(ms)
    print("# (a) guard off against the parent commit's library: median of a process's repeats, then median (min .. max) over %d "
          "alternating processes per build" % rounds)
    for name in res["this"]:
        a, b = np.array(res["parent"][name]), np.array(res["this"][name])
        print("%-44s parent %9.3f ms (%9.3f .. %9.3f)   this, guard off %9.3f ms (%9.3f .. %9.3f)   x %.3f"
              % (name, np.median(a), a.min(), a.max(), np.median(b), b.min(), b.max(), np.median(b) / np.median(a)))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library: leg (a)")
    ap.add_argument("--child-off", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--loops", action="store_true", help="also the loops bd_shared and bd_parcels, 20 x 100")
    ap.add_argument("--voxels", type=int, default=50000)
    a = ap.parse_args()
    if a.child_off:
        return child_off(a.voxels, a.loops, 5)
    if a.parent_lib:
        against_parent(a.parent_lib, a.voxels, a.loops, max(3, a.rounds // 2))
    dev = solver.device()
    hrf = orc.spm_hrf(1.0, 1.0, 20.0, False)[0][:20].copy()
    V = a.voxels
    Yb, _, _ = data.gen_rnd_bloc_bold_batch(V, dur=300.5 / 60.0, tr=1.0, hrf=hrf, nb_events=5, avg_dur=12.0, std_dur=1.0, snr=1.0, seed=4,
                                            device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    Yn = torch.randn(Yb.shape, generator=gen, device=dev, dtype=torch.float32)
    print("# legs: off = guard off on block signals (SNR 1 dB), on/b = guard on, same input; off/c, on/c = pure white noise")
    report("z-step shared %d x 300 x 100" % V, z_step_legs(Yb, Yn, hrf, 100), a.rounds)
    offsets = np.linspace(0, V, 401).astype(np.int64)
    report("z-step 400 parcels %d x 300 x 100" % V, z_step_legs(Yb, Yn, hrf, 100, grouped=offsets), a.rounds)
    hrf28 = orc.spm_hrf(1.0, 1.0, 28.0, False)[0][:28].copy()
    Yl, _, _ = data.gen_rnd_bloc_bold_batch(32768, dur=1200.5 / 60.0, tr=1.0, hrf=hrf28, nb_events=5, avg_dur=12.0, std_dur=1.0, snr=1.0,
                                            seed=5, device=dev)
    Yln = torch.randn(Yl.shape, generator=gen, device=dev, dtype=torch.float32)
    report("z-step shared 32768 x 1200 x 100", z_step_legs(Yl, Yln, hrf28, 100), a.rounds)
    if a.loops:
        labels = np.repeat(np.arange(400), -(-V // 400))[:V]
        kw = dict(lbda=1.0, theta_0=2.0, hrf_dur=20.0, nb_iter=20, nb_inner=100)

        def shared(Y, guard):
            _, _, d = distributed.bd_shared(Y, 1.0, guard=guard, **kw)
            return (lambda: d["guard"]) if guard else None

        def parc(Y, guard):
            d = parcels.bd_parcels(Y, labels, 1.0, guard=guard, **kw)[4]
            return (lambda: d["guard"]) if guard else None
        for name, fn in (("bd_shared 20 x 100", shared), ("bd_parcels 400 parcels 20 x 100", parc)):
            report("%s, %d x 300" % (name, V), {"off": lambda: fn(Yb, False), "on/b": lambda: fn(Yb, True),
                                                "off/c": lambda: fn(Yn, False), "on/c": lambda: fn(Yn, True)}, max(3, a.rounds // 2))


if __name__ == "__main__":
    main()
