#!/usr/bin/env python3
"""The reference's per-voxel workflow in two calls: blind deconvolution of a batch (one HRF dilation per voxel), then
``deconv`` of every voxel WITH ITS OWN estimated HRF and the noise-driven lambda search (``lbda=None``) -- what
examples/icassp_2019/simulation.py:62-72 of the reference fans out over voxels with joblib.

    python examples/blind_then_deconv.py [n_voxels]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pybold_amd  # noqa: E402
from pybold_amd import data, spm_hrf  # noqa: E402

n_voxels = int(sys.argv[1]) if len(sys.argv) > 1 else 256
t_r, hrf_dur = 1.0, 30.0
# synthetic voxels: block signals, HRF dilations spread over the batch
thetas = np.linspace(0.7, 1.6, 4)
Y = torch.cat([data.gen_rnd_bloc_bold_batch((n_voxels + 3) // 4, dur=5, tr=t_r, hrf=spm_hrf(th, t_r, hrf_dur, False)[0], nb_events=5,
                                            avg_dur=12.0, std_dur=1.0, snr=5.0, seed=k)[0] for k, th in enumerate(thetas)])[:n_voxels]
torch.cuda.synchronize()
t0 = time.time()
# 1. bd on the batch: x, z, diff_z and one estimated HRF per voxel, (V, K)
_, _, _, hrf, d = pybold_amd.bd(Y, t_r, lbda=1.0, hrf_dur=hrf_dur, nb_iter=30)
torch.cuda.synchronize()
t1 = time.time()
# 2. deconv of every voxel with its own HRF, lambda chosen per voxel from the noise level: float64 end to end
np.random.seed(0)                                   # (the power iterations draw their start vectors from NumPy's global RNG)
x, z, diff_z, J, R, G, info = pybold_amd.deconv_auto(Y, t_r, hrf.double(), nb_iter=50, nb_sub_iter=200, tol=1.0e-3, engine="auto")
torch.cuda.synchronize()
t2 = time.time()
print("%d voxels x %d scans: bd %.2f s (HRFs %s), deconv(lbda=None) with one HRF per voxel %.2f s on the %s engine; "
      "outer iterations %d..%d, lambda %.3g..%.3g" % (n_voxels, Y.shape[1], t1 - t0, tuple(hrf.shape), t2 - t1, info["engine"],
                                                      info["n_outer"].min(), info["n_outer"].max(), info["lbda"].min(), info["lbda"].max()))
