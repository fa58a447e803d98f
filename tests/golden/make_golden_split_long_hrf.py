"""Golden fixture ``split_long_hrf.npz``: the reference's ``deconv`` -- fixed lambda (pybold/bold_signal.py:13-97) and the
``lbda=None`` branch (:99-214) -- run by the REAL reference with HRFs of 33, 42 and 48 taps on series of 700, 1 200 and 1 280
scans, the range of the opt-in four-wave float64 register form for long HRFs (csrc/fista_exact_split_long.h):

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_split_long_hrf.py

Same import recipe as ``make_golden_long_hrf.py`` (build container only; data only, no reference source): the reference is
imported with the numba / pywt shims of ``make_golden.py`` and the noise level ``sigma`` is injected after import.

Cases ``k<K>_n<N>``: the reference's ``spm_hrf`` over 30 s at TR 0.72 s (the HCP TR: 42 taps) on 1 200 scans (the HCP run),
at TR 0.91 s (33 taps) on 700 scans, at TR 0.625 s (48 taps) on 1 280 scans; ``gen_regular_bloc_bold`` at SNR 1 dB,
``random_state=1``, cut to length.  Every (N, K) satisfies ``pybold_amd.spectral_matches_causal`` (asserted): the reference's
``x`` is spectral.

Fixed-lambda runs (tags ``<case>_fix_es1`` / ``_fix_es0``): lbda = 1, ``nb_iter = 200``, ``tol = 1e-6``, ``wind = 6``, with and
without early stopping; keys ``x_``, ``z_``, ``dz_``, ``J_``.
Runs with ``lbda=None`` (tags ``<case>_s<sigma index>_o<nb_iter>_i<nb_sub_iter>_t<tol>``): sigma in {0.5, 1, 2} x the in-package
db3 MAD estimate rounded to 6 digits, budgets (20, 50, 1e-6) and (60, 300, 1e-3), window rules on, ``wind = 6``; keys ``kw_``,
``x_``, ``z_``, ``dz_``, ``J_``, ``R_``, ``G_``, ``alpha_`` (recomputed from R with the reference's own expression).  Only runs in
which alpha stays away from 0 (min |alpha| > ``ALPHA_FLOOR``, printed per run) are kept -- nearer the pole of
lambda = 1 / (2 alpha) a run is chaotic and pins nothing; ``auto_tags`` lists the kept ones.  Per case ``<case>_y``, ``_hrf``,
``_t_r``, ``_lipschitz``, ``_sigma``."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import _import_reference, quiet  # noqa: E402

BUDGETS = ((20, 50, 1.0e-6), (60, 300, 1.0e-3))
CASES = ((42, 0.72, 1200), (33, 0.91, 700), (48, 0.625, 1280))      # (taps, t_r, scans); HRFs over dur = 30 s
ALPHA_FLOOR = 1.0e-2


def main():
    bs, cv, data, hm, lin, ut = _import_reference()
    import pybold_amd
    from oracle import pybold_oracle as orc        # only for the size of sigma (a number we CHOOSE)
    out, kept, neg = {}, [], 0
    for k, t_r, n in CASES:
        hrf = hm.spm_hrf(1.0, t_r=t_r, dur=30.0)[0]
        assert len(hrf) == k, (len(hrf), k)
        case = "k%d_n%d" % (k, n)
        assert pybold_amd.spectral_matches_causal(n, k), case
        y_all = data.gen_regular_bloc_bold(dur=n * t_r / 60.0 + 1.0, tr=t_r, hrf=hrf, snr=1.0, random_state=1)[0]
        y = np.array(y_all[:n])
        assert len(y) == n, len(y)
        np.random.seed(0)
        H = lin.ConvAndLinear(lin.DiscretInteg(), hrf, dim_in=n, dim_out=n)
        lip = 0.9 * ut.spectral_radius_est(H, (n,))
        s_hat = float(orc.mad_daub_noise_est(y))
        sigmas = np.array([float("%.6g" % (f * s_hat)) for f in (0.5, 1.0, 2.0)])
        out.update({case + "_y": y, case + "_hrf": hrf, case + "_t_r": t_r, case + "_lipschitz": lip, case + "_sigma": sigmas})
        for es in (1, 0):
            tag = "%s_fix_es%d" % (case, es)
            np.random.seed(0)
            x, z, dz, J, _, _ = quiet(bs.deconv, y, t_r, hrf, lbda=1.0, nb_iter=200, early_stopping=bool(es), tol=1.0e-6, wind=6)
            out.update({"x_" + tag: x, "z_" + tag: z, "dz_" + tag: dz, "J_" + tag: np.array(J)})
            print("%-28s K %d iterations %3d  |dz| %.6g" % (tag, k, len(J), np.linalg.norm(dz)), flush=True)
        real = bs.mad_daub_noise_est
        try:
            for si, sigma in enumerate(sigmas):
                for o, i, tol in BUDGETS:
                    tag = "%s_s%d_o%d_i%d_t%g" % (case, si, o, i, tol)
                    bs.mad_daub_noise_est = lambda x, s=float(sigma): s      # bold_signal.py:10 bound the name at import
                    np.random.seed(0)
                    t0 = time.time()
                    x, z, dz, J, R, G = quiet(bs.deconv, y, t_r, hrf, lbda=None, nb_iter=o, nb_sub_iter=i, early_stopping=True,
                                              tol=tol, wind=6)
                    alpha, a = [], 1.0
                    for r in R:
                        a += 1.0e-4 * (r - n * float(sigma) ** 2)
                        alpha.append(a)
                    keep = np.abs(alpha).min() > ALPHA_FLOOR
                    print("%-28s K %d outer %3d  min|alpha| %.3g  lbda_end %.6g  |dz| %.6g  %.1f s  %s" % (
                        tag, k, len(J), np.abs(alpha).min(), 1.0 / (2.0 * alpha[-1]), np.linalg.norm(dz), time.time() - t0,
                        "kept" if keep else "DROPPED: alpha too close to 0"), flush=True)
                    if not keep:
                        continue
                    kept.append(tag)
                    neg += bool((np.array(alpha) < 0).any())
                    out["kw_" + tag] = np.array([o, i, 1.0, tol, 6])
                    out.update({"x_" + tag: x, "z_" + tag: z, "dz_" + tag: dz, "J_" + tag: np.array(J), "R_" + tag: np.array(R),
                                "G_" + tag: np.array(G), "alpha_" + tag: np.array(alpha)})
        finally:
            bs.mad_daub_noise_est = real
    out["auto_tags"] = np.array(kept)
    path = os.path.join(HERE, "split_long_hrf.npz")
    np.savez_compressed(path, **out)
    print("split_long_hrf.npz:", len(out), "arrays,", len(kept), "lbda=None runs kept,", neg, "with alpha < 0,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
