"""``auto_lbda_wind6.npz``: more runs of the reference's ``deconv(lbda=None)`` branch (pybold/bold_signal.py:99-214) by
the REAL reference, same recipe, series, HRFs and injected noise levels as ``make_golden_r5.py`` (read from its
``auto_lbda.npz``), all with ``wind = 6`` -- the window the register-resident kernels carry -- and tolerances at which
the alpha window (:164-178) FIRES on every run, at a different outer iteration per noise level:

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 <repo>/tests/golden/make_golden_auto_wind6.py

``auto_lbda.npz`` has two such runs with ``wind = 6`` (its others use ``wind = 4``, which the device-resident search
does not carry).  Budget 60 x 100, ``tol`` in {5e-2, 1e-1}, the three noise levels of either case: 12 runs.
Keys as in ``auto_lbda.npz`` (``tests/test_oracle_golden.py::auto_lbda_runs`` reads either file)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference, quiet  # noqa: E402


def main():
    bs = _import_reference()[0]
    src = np.load(os.path.join(HERE, "auto_lbda.npz"))
    out = {}
    real = bs.mad_daub_noise_est
    try:
        for case in ("c1", "c2"):
            y, hrf, sigmas = src[case + "_y"], src[case + "_hrf"], src[case + "_sigma"]
            for k in ("_y", "_hrf", "_lipschitz", "_sigma"):
                out[case + k] = src[case + k]
            n = len(y)
            for si, sigma in enumerate(sigmas):
                for tol in (5.0e-2, 1.0e-1):
                    tag = "%s_s%d_o60_i100_e1_t%g_w6" % (case, si, tol)
                    bs.mad_daub_noise_est = lambda x, s=float(sigma): s      # bold_signal.py:10 bound the name at import
                    np.random.seed(0)
                    x, z, dz, J, R, G = quiet(bs.deconv, y, 1.0, hrf, lbda=None, nb_iter=60, nb_sub_iter=100,
                                              early_stopping=True, tol=tol, wind=6)
                    alpha, a = [], 1.0
                    for r in R:
                        a += 1.0e-4 * (r - n * float(sigma) ** 2)
                        alpha.append(a)
                    out["kw_" + tag] = np.array([60, 100, 1.0, tol, 6])
                    out.update({"x_" + tag: x, "z_" + tag: z, "dz_" + tag: dz, "J_" + tag: np.array(J),
                                "R_" + tag: np.array(R), "G_" + tag: np.array(G), "alpha_" + tag: np.array(alpha)})
                    print("%-28s outer %3d  min|alpha| %.4f" % (tag, len(J), np.abs(alpha).min()), flush=True)
    finally:
        bs.mad_daub_noise_est = real
    np.savez_compressed(os.path.join(HERE, "auto_lbda_wind6.npz"), **out)
    print("auto_lbda_wind6.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
