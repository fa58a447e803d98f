#!/usr/bin/env python3
"""Semi-blind deconvolution with one HRF dilation per parcel of an atlas: a synthetic batch whose parcels were
generated with different dilations, and the dilation `bd_parcels` finds for each.

    python examples/blind_parcels.py [voxels_per_parcel] [scans]

`scans` (default 300): the run length.  From 311 scans on (up to 1 280) the z-steps run on the split matrix-pipe forms by
opt-in only -- `force="gsplit"`, which this example passes for such lengths; without it they run per problem on the
vector forms.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pybold_amd  # noqa: E402
from pybold_amd import data, spm_hrf  # noqa: E402

per_parcel = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
scans = int(sys.argv[2]) if len(sys.argv) > 2 else 300
force = "gsplit" if 311 <= scans <= 1280 else None
t_r, hrf_dur = 0.75, 20.0
true_theta = {11: 0.7, 12: 0.9, 25: 1.1, 40: 1.3}             # atlas label -> the dilation its voxels are generated with
rows, labels = [], []
for i, (label, theta) in enumerate(true_theta.items()):
    h = spm_hrf(theta, t_r, hrf_dur, False)[0]
    Y, _, _ = data.gen_rnd_bloc_bold_batch(per_parcel + 37 * i, dur=scans * t_r / 60.0, tr=t_r, hrf=h, nb_events=max(5, scans // 60), avg_dur=12.0, std_dur=1.0,
                                           snr=10.0, seed=i)
    rows.append(Y)
    labels += [label] * Y.shape[0]
shuffle = torch.randperm(len(labels), generator=torch.Generator().manual_seed(0))      # voxels come in any order
Y = torch.cat(rows)[shuffle.cuda()].contiguous()
labels = np.asarray(labels)[shuffle.numpy()]
torch.cuda.synchronize()
t0 = time.time()
X, Z, W, H, d = pybold_amd.bd_parcels(Y, labels, t_r, lbda=1.7, hrf_dur=hrf_dur, nb_iter=20, nb_inner=100, force=force)
torch.cuda.synchronize()
print("%d voxels x %d scans in %d parcels, 20 x 100 iterations%s: %.2f s"
      % (Y.shape[0], Y.shape[1], len(d["labels"]), " (force=%s)" % force if force else "", time.time() - t0))
for g, label in enumerate(d["labels"]):
    print("  parcel %3d (%5d voxels): theta %.4f (generated with %.2f), normalised cost %.4f"
          % (label, d["sizes"][g], d["theta"][-1, g], true_theta[int(label)], d["J"][-1, g]))
