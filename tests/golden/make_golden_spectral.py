"""Generate ``spectral.npz`` (the spectral operators and their padding) from the REAL reference.

Needs the reference checkout (``PYBOLD_REFERENCE``, imported read-only as in make_golden.py); the tests read only the
``.npz``.  From any directory outside the reference:

    PYTHONDONTWRITEBYTECODE=1 python3 <repo>/tests/golden/make_golden_spectral.py

Data only: inputs and the reference's outputs, no reference source text.

Keys
  x_<N>, k_<K>                     inputs: one random series per length, one random filter per tap count
  conv_<N>_<K>, retro_<N>_<K>      spectral_convolve / spectral_retro_convolve(k_<K>, x_<N>) (one tap: below 995
                                   scans only, to keep the file small)
  long_cases                       (N, K) pairs with a filter longer than the series
  deconv_<N>_<f>, rdeconv_<N>_<f>  spectral_deconvolve / spectral_retro_deconvolve(filt_<f>, x_<N>), f in hrf / mild
  padidx_<N>, padp_<N>             custom_padd(arange(1, N + 1)): 0 = a padded zero, i + 1 = sample i; p as (left, right),
                                   (0, 0) where the reference returns p = 0
  div_n, div_k, div_matches        div_matches[k, n - 1]: both spectral forms equal the causal FIR / its adjoint (max-abs
                                   over max-abs <= 1e-9 on random input); False where the reference raises
  dc_<N>_{y,hrf,z,x,tr,seed}       fixed-lambda deconv (lbda = 1, 200 iterations, no early stop) on a block signal at
                                   SNR 1 dB; np.random.seed(seed) right before the call (spectral_radius_est draws from it)
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference  # noqa: E402

LENGTHS = (1, 2, 60, 99, 100, 300, 341, 342, 400, 405, 511, 513, 600, 995, 996, 1023, 1024, 1025, 2048, 2049)
TAPS = (1, 30, 64)
LONG = ((60, 100), (300, 1500))
DECONV_LENGTHS = (2, 60, 300, 400, 405, 600, 996, 1024, 2049)
DIV_K = (1, 2, 30, 48, 64)
DIV_N = 4200


def causal(k, x):
    return np.convolve(k, x)[:len(x)]


def causal_adj(k, x):
    return np.convolve(k, x[::-1])[:len(x)][::-1]


def main():
    bs, cv, data, hm, lin, ut = _import_reference()
    from pybold import padding
    rng = np.random.RandomState(20261016)
    out = {}
    ks = {K: rng.randn(K) for K in TAPS + tuple(k for _, k in LONG)}
    for K, k in ks.items():
        out["k_%d" % K] = k
    for N in LENGTHS + tuple(n for n, _ in LONG):
        if "x_%d" % N not in out:
            out["x_%d" % N] = rng.randn(N)
    for N, K in [(N, K) for N in LENGTHS for K in TAPS if K > 1 or N < 995] + list(LONG):
        out["conv_%d_%d" % (N, K)] = cv.spectral_convolve(ks[K], out["x_%d" % N])
        out["retro_%d_%d" % (N, K)] = cv.spectral_retro_convolve(ks[K], out["x_%d" % N])
    out["long_cases"] = np.array(LONG)

    filts = {"hrf": hm.spm_hrf(1.0, t_r=1.0, dur=30.0)[0], "mild": np.array([1.0, 0.5, 0.25])}
    for f, h in filts.items():
        out["filt_" + f] = h
        for N in DECONV_LENGTHS:
            out["deconv_%d_%s" % (N, f)] = cv.spectral_deconvolve(h, out["x_%d" % N])
            out["rdeconv_%d_%s" % (N, f)] = cv.spectral_retro_deconvolve(h, out["x_%d" % N])

    for N in LENGTHS:
        a, p = padding.custom_padd(np.arange(1, N + 1, dtype=np.float64))
        out["padidx_%d" % N] = a.astype(np.int32)
        out["padp_%d" % N] = np.array((0, 0) if p == 0 else p, dtype=np.int64)

    matches = np.zeros((len(DIV_K), DIV_N), dtype=bool)
    for a, K in enumerate(DIV_K):
        k = rng.randn(K)
        for N in range(1, DIV_N + 1):
            x = rng.randn(N)
            try:
                s, r = cv.spectral_convolve(k, x), cv.spectral_retro_convolve(k, x)
            except ValueError:
                continue
            c, ca = causal(k, x), causal_adj(k, x)
            matches[a, N - 1] = (np.abs(s - c).max() <= 1e-9 * np.abs(c).max()
                                 and np.abs(r - ca).max() <= 1e-9 * np.abs(ca).max())
    out["div_n"] = np.arange(1, DIV_N + 1)
    out["div_k"] = np.array(DIV_K)
    out["div_matches"] = matches

    for N, tr in ((400, 1.0), (405, 0.72)):
        hrf = hm.spm_hrf(1.0, t_r=tr, dur=20.0)[0]
        y = data.gen_regular_bloc_bold(dur=N * tr / 60.0 + 1.0, tr=tr, hrf=hrf, snr=1.0, random_state=0)[0][:N]
        assert len(y) == N
        np.random.seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            x, z, _, _, _, _ = bs.deconv(y, tr, hrf, lbda=1.0, nb_iter=200, early_stopping=False)
        pre = "dc_%d_" % N
        out.update({pre + "y": y, pre + "hrf": hrf, pre + "z": z, pre + "x": x, pre + "tr": tr, pre + "seed": 0})
        print("N=%d TR=%.2f taps=%d  ||x - causal(h, z)|| / ||x|| = %.2e"
              % (N, tr, len(hrf), np.linalg.norm(x - causal(hrf, z)) / np.linalg.norm(x)))

    path = os.path.join(HERE, "spectral.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d keys, %d bytes)" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
