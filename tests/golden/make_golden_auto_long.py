"""Golden fixture ``auto_lbda_long.npz``: the reference's ``deconv(lbda=None)`` branch (pybold/bold_signal.py:99-214) run by the
REAL reference on series of 641 .. 1 280 scans, the range of the four-wave float64 kernel (csrc/fista_exact_split.h):

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_auto_long.py

Same import recipe as ``make_golden_r5.py`` (build container only; data only, no reference source): the reference is imported
with the numba / pywt shims of ``make_golden.py`` and the noise level ``sigma`` is injected after import.

Cases: ``hcp`` -- 1 200 scans at TR 0.72 s with a 20 s HRF (28 taps), the series of ``make_golden_r5_long.py`` -- and ``n700`` --
700 scans at TR 1 s with a 30 s HRF (30 taps), the same generator with ``random_state=1``.  sigma in {0.5, 1, 2} x the in-package
db3 MAD estimate, rounded to 6 digits; budgets ``(nb_iter, nb_sub_iter, tol)`` in {(20, 50, 1e-6), (60, 300, 1e-2),
(60, 300, 1e-3)}, window rules on, ``wind = 6``.  In every run alpha stays away from 0 (the printed min |alpha|), so none sits in
the chaotic regime; the 2 sigma runs drive alpha -- hence lambda -- negative.

Keys, per run tag ``<case>_s<sigma index>_o<nb_iter>_i<nb_sub_iter>_t<tol>``: ``kw_`` ([nb_iter, nb_sub_iter, early_stopping,
tol, wind]), ``x_``, ``z_``, ``dz_``, ``J_``, ``R_``, ``G_``, ``alpha_`` (recomputed from R with the reference's own expression, as in
``make_golden_r5.py``); per case ``<case>_y``, ``_hrf``, ``_t_r``, ``_lipschitz``, ``_x0``, ``_sigma``."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import _import_reference, quiet  # noqa: E402

BUDGETS = ((20, 50, 1.0e-6), (60, 300, 1.0e-2), (60, 300, 1.0e-3))


def main():
    bs, cv, data, hm, lin, ut = _import_reference()
    from oracle import pybold_oracle as orc        # only for the size of sigma (a number we CHOOSE)
    out = {}
    for case, n, t_r, dur in (("hcp", 1200, 0.72, 20.0), ("n700", 700, 1.0, 30.0)):
        hrf = hm.spm_hrf(1.0, t_r=t_r, dur=dur)[0]
        y = data.gen_regular_bloc_bold(dur=n * t_r / 60.0 + 1.0, tr=t_r, hrf=hrf, snr=1.0, random_state=1)[0][:n]
        assert len(y) == n, len(y)
        np.random.seed(0)
        x0 = np.random.randn(n)
        np.random.seed(0)
        H = lin.ConvAndLinear(lin.DiscretInteg(), hrf, dim_in=n, dim_out=n)
        lip = 0.9 * ut.spectral_radius_est(H, (n,))
        s_hat = float(orc.mad_daub_noise_est(y))
        sigmas = np.array([float("%.6g" % (f * s_hat)) for f in (0.5, 1.0, 2.0)])
        out.update({case + "_y": y, case + "_hrf": hrf, case + "_t_r": t_r, case + "_lipschitz": lip, case + "_x0": x0,
                    case + "_sigma": sigmas})
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
                    out["kw_" + tag] = np.array([o, i, 1.0, tol, 6])
                    out.update({"x_" + tag: x, "z_" + tag: z, "dz_" + tag: dz, "J_" + tag: np.array(J), "R_" + tag: np.array(R),
                                "G_" + tag: np.array(G), "alpha_" + tag: np.array(alpha)})
                    print("%-28s K %d outer %3d  min|alpha| %.3g  lbda_end %.6g  |dz| %.6g  %.1f s" % (
                        tag, len(hrf), len(J), np.abs(alpha).min(), 1.0 / (2.0 * alpha[-1]), np.linalg.norm(dz), time.time() - t0),
                        flush=True)
        finally:
            bs.mad_daub_noise_est = real
    np.savez_compressed(os.path.join(HERE, "auto_lbda_long.npz"), **out)
    print("auto_lbda_long.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
