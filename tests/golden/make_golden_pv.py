"""Golden fixture ``per_voxel_hrf.npz``: ``deconv`` of six voxels, each with ITS OWN HRF, by the REAL reference --
six consecutive 1-D calls after one ``np.random.seed(0)``, the call pattern ``deconv(y2d, t_r, hrf2d)`` of this
package restates in one batch.

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 <repository>/tests/golden/make_golden_pv.py

Same import recipe as ``make_golden.py`` (build container only; data only, no reference source); the noise level of the
``lbda=None`` runs is injected as in ``make_golden_r5.py``.

Inputs: ``hrf_v = spm_hrf(delta_v, t_r=1.0, dur=30.)[0]`` for ``delta = 0.6, 0.8, 1.0, 1.2, 1.5, 1.9`` and
``y_v = gen_regular_bloc_bold(dur=3, tr=1.0, hrf=hrf_v, snr=1.0, random_state=v)[0]`` (180 scans).

Keys:
  y (6, 180), hrf (6, 30), delta (6,)
  x0 (6, 180)       ``np.random.randn(6, 180)`` under ``np.random.seed(0)``: row v is the start vector the v-th of the six
                    consecutive calls draws for its power iteration
  lipschitz (6,)    the six ``0.9 rho`` of those calls
  sigma (6,)        the in-package db3 MAD estimate of every series, rounded to 6 digits (injected into runs d, e)
  runs a, b, c (fixed lambda): ``<run>_kw`` = [lbda, nb_iter, early_stopping, tol, wind], ``<run>_x``, ``_z``, ``_dz``
                    (6, 180), ``<run>_J`` (6, longest trace) padded with NaN, ``<run>_n`` (6,) trace lengths
     a  lbda=0.5, nb_iter=300, tol=1e-2, wind=6, early_stopping=True
     b  the same with lbda=2.0
     c  lbda=0.5, nb_iter=60, early_stopping=False
  runs d, e (lbda=None): ``<run>_kw`` = [nb_iter, nb_sub_iter, early_stopping, tol, wind], ``_x``, ``_z``, ``_dz``,
                    ``<run>_J``, ``_R``, ``_G`` (6, longest) padded with NaN, ``<run>_n`` (6,) outer iterations
     d  nb_iter=20, nb_sub_iter=50, tol=1e-2
     e  nb_iter=5, nb_sub_iter=50, early_stopping=False

Before anything is written the script asserts, for runs a and b, that the repository's oracle in its other arithmetic
(``deconv_fixed_lbda(dense=False)``) stops every voxel at the reference's iteration: a fixture whose decisions sit on a
rounding edge is not written.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import _import_reference, quiet  # noqa: E402

DELTAS = (0.6, 0.8, 1.0, 1.2, 1.5, 1.9)


def pad(rows):
    n = max(len(r) for r in rows)
    out = np.full((len(rows), n), np.nan)
    for v, r in enumerate(rows):
        out[v, :len(r)] = r
    return out


def main():
    bs, cv, data, hm, lin, ut = _import_reference()
    from oracle import pybold_oracle as orc
    hrf = np.stack([hm.spm_hrf(d, t_r=1.0, dur=30.)[0] for d in DELTAS])
    y = np.stack([data.gen_regular_bloc_bold(dur=3, tr=1.0, hrf=hrf[v], snr=1.0, random_state=v)[0]
                  for v in range(len(DELTAS))])
    V, n = y.shape
    np.random.seed(0)
    x0 = np.random.randn(V, n)
    np.random.seed(0)
    lip = np.array([0.9 * ut.spectral_radius_est(lin.ConvAndLinear(lin.DiscretInteg(), hrf[v], dim_in=n, dim_out=n), (n,))
                    for v in range(V)])
    sigma = np.array([float("%.6g" % float(orc.mad_daub_noise_est(y[v]))) for v in range(V)])
    out = {"y": y, "hrf": hrf, "delta": np.array(DELTAS), "x0": x0, "lipschitz": lip, "sigma": sigma}

    for tag, kw in (("a", dict(lbda=0.5, nb_iter=300, tol=1.0e-2, wind=6, early_stopping=True)),
                    ("b", dict(lbda=2.0, nb_iter=300, tol=1.0e-2, wind=6, early_stopping=True)),
                    ("c", dict(lbda=0.5, nb_iter=60, tol=1.0e-6, wind=6, early_stopping=False))):
        np.random.seed(0)
        res = [quiet(bs.deconv, y[v], 1.0, hrf[v], **kw) for v in range(V)]
        n_ref = np.array([len(r[3]) for r in res])
        if kw["early_stopping"]:
            n_orc = np.array([orc.deconv_fixed_lbda(y[v], hrf[v], kw["lbda"], nb_iter=kw["nb_iter"], early_stopping=True,
                                                    tol=kw["tol"], wind=kw["wind"], lipschitz=lip[v], dense=False)[4]
                              for v in range(V)])
            assert (n_orc == n_ref).all(), "run %s: oracle stops at %s, reference at %s" % (tag, n_orc, n_ref)
            assert (n_ref < kw["nb_iter"]).all() and len(set(n_ref.tolist())) >= 2, n_ref
        out.update({tag + "_kw": np.array([kw["lbda"], kw["nb_iter"], float(kw["early_stopping"]), kw["tol"], kw["wind"]]),
                    tag + "_x": np.stack([r[0] for r in res]), tag + "_z": np.stack([r[1] for r in res]),
                    tag + "_dz": np.stack([r[2] for r in res]), tag + "_J": pad([np.asarray(r[3]) for r in res]),
                    tag + "_n": n_ref})
        print("run %s: iterations %s" % (tag, n_ref.tolist()), flush=True)

    real = bs.mad_daub_noise_est
    try:
        for tag, kw in (("d", dict(nb_iter=20, nb_sub_iter=50, tol=1.0e-2, wind=6, early_stopping=True)),
                        ("e", dict(nb_iter=5, nb_sub_iter=50, tol=1.0e-6, wind=6, early_stopping=False))):
            np.random.seed(0)
            res = []
            for v in range(V):
                bs.mad_daub_noise_est = lambda x, s=float(sigma[v]): s      # bold_signal.py:10 bound the name at import
                res.append(quiet(bs.deconv, y[v], 1.0, hrf[v], lbda=None, **kw))
            n_ref = np.array([len(r[3]) for r in res])
            out.update({tag + "_kw": np.array([kw["nb_iter"], kw["nb_sub_iter"], float(kw["early_stopping"]), kw["tol"], kw["wind"]]),
                        tag + "_x": np.stack([r[0] for r in res]), tag + "_z": np.stack([r[1] for r in res]),
                        tag + "_dz": np.stack([r[2] for r in res]), tag + "_J": pad([np.asarray(r[3]) for r in res]),
                        tag + "_R": pad([np.asarray(r[4]) for r in res]), tag + "_G": pad([np.asarray(r[5]) for r in res]),
                        tag + "_n": n_ref})
            print("run %s: outer iterations %s" % (tag, n_ref.tolist()), flush=True)
    finally:
        bs.mad_daub_noise_est = real
    np.savez_compressed(os.path.join(HERE, "per_voxel_hrf.npz"), **out)
    print("per_voxel_hrf.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
