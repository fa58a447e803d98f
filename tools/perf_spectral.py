"""Time the spectral operator kernel (pb_spectral_conv) against pb_conv (the causal FIR over the same rows) and a
torch.fft statement of the reference's padded product (gather-pad, rfft, multiply, irfft, slice), float64,
V = 100 000 rows, K = 30 taps at 300 and 400 scans; and spectral_deconvolve at 400 scans (T = 1 024 taps).

Interleaved rounds in one process (every variant once per round, HIP events around each call after a
warm-up); median and min over the rounds.  Bytes and flops come from the shapes:
  direct kernels: rows read once and written once (8 B each); 2 N T flops per row (T taps per output)
  torch.fft route: gathered padded rows (L), spectra (L/2 + 1 complex) written and read per stage; flops are
  the nominal 2.5 L log2 L per real transform, twice, plus 6 per complex product (L/2 + 1 bins)

    python tools/perf_spectral.py [--rounds 20] [--out profiles/spectral_ops.txt]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pybold_amd import _lib, padding, solver  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--voxels", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join("profiles", "spectral_ops.txt"))
    args = ap.parse_args()
    dev = solver.device()
    lib = _lib.load()
    stream = solver._stream_ptr(dev)
    V, K = args.voxels, 30
    rng = np.random.RandomState(0)
    k = rng.randn(K)
    hrf = np.exp(-0.5 * ((np.arange(K) - 6.0) / 2.0) ** 2) - 0.2 * np.exp(-0.5 * ((np.arange(K) - 16.0) / 3.0) ** 2)
    gen = torch.Generator(device=dev).manual_seed(1)
    lines = ["perf_spectral: V=%d float64, %d interleaved rounds, HIP events; %s" % (V, args.rounds, torch.cuda.get_device_name(dev))]
    results = {}

    def case(N, deconvolve):
        X = torch.randn((V, N), dtype=torch.float64, device=dev, generator=gen)
        out = torch.empty_like(X)
        idx, p_l = padding.custom_padd_layout(N)
        L = idx.size
        c = np.fft.irfft(1.0 / np.fft.rfft(hrf, L), L) if deconvolve else k[:L]
        T = c.size
        m_d = torch.from_numpy(idx).to(dev)
        c_d = torch.from_numpy(np.ascontiguousarray(c)).to(dev)
        k_d = torch.from_numpy(k).to(dev)
        gidx = torch.from_numpy(idx.astype(np.int64)).to(dev)
        keep = (gidx >= 0).to(torch.float64)
        spec = torch.fft.rfft(torch.from_numpy(hrf if deconvolve else k).to(dev), n=L)
        spec = 1.0 / spec if deconvolve else spec

        def spectral():
            _lib.check(lib.pb_spectral_conv(X.data_ptr(), N, out.data_ptr(), N, V, N, m_d.data_ptr(), L, p_l,
                                            c_d.data_ptr(), T, stream), "pb_spectral_conv")

        def conv():
            _lib.check(lib.pb_conv(X.data_ptr(), N, out.data_ptr(), N, V, N, N, k_d.data_ptr(), K, stream), "pb_conv")

        def fft():
            xp = X[:, gidx.clamp(min=0)] * keep
            return torch.fft.irfft(torch.fft.rfft(xp, n=L) * spec, n=L)[:, p_l:p_l + N]

        variants = [("pb_spectral_conv", spectral)] + ([] if deconvolve else [("pb_conv", conv)]) + [("torch.fft", fft)]
        # the outputs agree before anything is timed
        spectral()
        ref = fft()
        err = ((out - ref).abs().max() / ref.abs().max()).item()
        for _, fn in variants:           # warm-up: code objects, FFT plans
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in variants}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(args.rounds):
            for name, fn in variants:
                ev[0].record()
                fn()
                ev[1].record()
                ev[1].synchronize()
                times[name].append(ev[0].elapsed_time(ev[1]))
        label = "N=%d %s T=%d L=%d" % (N, "spectral_deconvolve" if deconvolve else "K=%d" % K, T, L)
        lines.append("")
        lines.append("%s   (pb_spectral_conv vs torch.fft max-abs / max-abs %.1e)" % (label, err))
        direct_bytes = 2.0 * V * N * 8
        fft_bytes = V * (N * 8 + 3 * L * 8 + 4 * (L // 2 + 1) * 16 + N * 8)
        flops = {"pb_spectral_conv": 2.0 * V * N * T, "pb_conv": 2.0 * V * N * K - V * K * (K - 1),
                 "torch.fft": V * (2 * 2.5 * L * math.log2(L) + 6 * (L // 2 + 1))}
        nbytes = {"pb_spectral_conv": direct_bytes, "pb_conv": direct_bytes, "torch.fft": fft_bytes}
        for name, _ in variants:
            t = np.array(times[name])
            med = float(np.median(t))
            results[(label, name)] = med
            lines.append("  %-17s median %8.3f ms  min %8.3f ms   %7.1f GB/s  %8.1f GFLOP/s  (%.2e B, %.2e flop)"
                         % (name, med, t.min(), nbytes[name] / med * 1e-6, flops[name] / med * 1e-6,
                            nbytes[name], flops[name]))
        if not deconvolve:
            lines.append("  pb_spectral_conv / pb_conv = %.3f (median)"
                         % (results[(label, "pb_spectral_conv")] / results[(label, "pb_conv")]))
        lines.append("  torch.fft / pb_spectral_conv = %.3f (median)"
                     % (results[(label, "torch.fft")] / results[(label, "pb_spectral_conv")]))
        del X, out
        torch.cuda.empty_cache()

    with torch.cuda.device(dev):
        case(300, False)
        case(400, False)
        case(400, True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
