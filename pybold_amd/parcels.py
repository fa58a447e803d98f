"""Semi-blind deconvolution with ONE HRF dilation PER PARCEL of an atlas: between ``bd`` on a 2-D batch (one dilation
per voxel: noisy and slow) and :func:`pybold_amd.distributed.bd_shared` (one for every voxel: wrong where regions
differ).  The haemodynamic delay is a property of a region, so the voxels of a parcel share one dilation; the model is
G independent ``bd_shared`` problems, and the loop below is that of ``_bd_shared_device_loop`` for all of them at once
(pybold/bold_signal.py:281-382 for the structure; :217-222, :329-333 for the theta-step written as normal equations).

Every step is batched over parcels and stays on the device: the z-step with each wave's operator tiles built from its
parcel's taps (``pb_fista_solve_grouped``), the normal equations summed per parcel in one pass
(``pb_hrf_normal_eq_w_grouped``), the 1-D searches (``pb_theta_fit``, one workgroup per parcel) and the step constants
(``pb_gram_frobenius``).  Single GPU; float32 ``Y``; no early stopping.
"""
import os

import numpy as np
import torch

from . import _lib, solver
from .hrf_model import MAX_DELTA, MIN_DELTA

# Series of 311 .. 1 280 scans (up to 48 taps) on the split matrix-pipe forms of the grouped z-step is OPT-IN
# (PB_FLAG_GROUPED_SPLIT): the environment variable PYBOLD_AMD_PARCELS_SPLIT ("1" is on; the convention of
# PYBOLD_AMD_PP_SPLIT, bold_signal.py) ORs the flag into every z-step of bd_parcels.  Read when a loop starts.
def parcels_split_opt_in():
    return os.environ.get("PYBOLD_AMD_PARCELS_SPLIT", "0") == "1"


def sort_by_label(labels):
    """``(distinct labels (G,), order (V,), offsets (G + 1,))``: ``order`` lists the rows parcel by parcel (stable: the
    caller's order inside a parcel), parcel ``g`` -- label ``distinct[g]`` -- owning ``order[offsets[g]:offsets[g + 1]]``."""
    lab = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels).ravel()
    distinct, inverse, counts = np.unique(lab, return_inverse=True, return_counts=True)
    order = np.argsort(inverse.ravel(), kind="stable")
    return distinct, order, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _parcel_loop(Y, po, t_r, lbda, theta, hrf_dur, bounds, nb_iter, nb_inner, force, guard_work=None):
    """The outer loop on rows sorted by parcel; device tensors only, nothing returns to the host:
    ``(W, taps (G, K), thetas [nb_iter + 1 tensors (G,)], costs [nb_iter + 1 tensors (G,)])``.  ``guard_work``: the buffer
    of the conditioning guard -- given, every z-step goes through it (:func:`pybold_amd.solver.fista_solve_grouped`)."""
    V, n = Y.shape
    dev = Y.device
    base = force if isinstance(force, int) else solver._FORCE[force]
    if parcels_split_opt_in():
        base |= _lib.PB_FLAG_GROUPED_SPLIT
    taps = solver.spm_hrf_batch(theta, t_r, hrf_dur)                    # (G, K)
    K = taps.shape[1]
    ne_len = K * K + K + 1
    W = torch.zeros((V, n), dtype=torch.float64, device=dev)
    msg = torch.empty((po.G, ne_len + 1), dtype=torch.float64, device=dev)
    lib = _lib.load()
    work_z = torch.empty((max(int(lib.pb_fista_grouped_work_len(V, po.G, K)), 2),), dtype=torch.int32, device=dev)
    work_ne = torch.empty((max(int(lib.pb_hrf_normal_eq_w_grouped_work_len(V, po.G, K)), 1),), dtype=torch.float64, device=dev)
    thetas, costs = [theta], []
    for it in range(nb_iter + 1):
        last = it == nb_iter
        step = 1.0 / solver.gram_frobenius_batch(taps, n)               # (G,): pybold/bold_signal.py:249-254 per parcel
        # an intermediate z-step keeps sparse iterates on the matrix pipe (HipOps.z_step(last=False)); the last one keeps the guard
        W, _ = solver.fista_solve_grouped(Y, taps, step, po, lbda, nb_inner, W0=W, inplace=True,
                                          force=base if last else base | _lib.PB_FLAG_NO_RHO_GUARD, work=work_z,
                                          guard_work=guard_work, guard=guard_work is not None)
        solver.hrf_normal_eq_w_grouped(W, Y, K, po, work=work_ne, out=msg)
        ne, l1, yy = msg[:, :ne_len], msg[:, ne_len], msg[:, ne_len - 1]
        if not last:
            theta, f, taps = solver.theta_fit(ne, t_r, hrf_dur, bounds[0])
            thetas.append(theta)
        else:                                                           # last z-step: price the current HRFs
            Gm, b = ne[:, :K * K].reshape(po.G, K, K), ne[:, K * K:K * K + K]
            f = 0.5 * yy - (taps * b).sum(dim=1) + 0.5 * torch.einsum("gk,gkl,gl->g", taps, Gm, taps)
        costs.append((2.0 * f + lbda * l1) / yy)
    return W, taps, thetas, costs


def bd_parcels(Y, labels, t_r, lbda=1.0, theta_0=None, hrf_dur=20.0, bounds=None, nb_iter=20, nb_inner=100, force=None,
               verbose=0, guard=None):
    """``bd`` with one HRF dilation per parcel.  ``Y``: ``(V, N)``, NumPy or a float32 CUDA tensor; ``labels``: ``(V,)``
    integers, any values in any order -- the voxels with the same label share one dilation.  ``lbda``: a scalar.
    ``theta_0``: a scalar, or one start value per parcel in the order of the sorted distinct labels.  Structure, step
    constant and cost bookkeeping are those of :func:`pybold_amd.distributed.bd_shared` per parcel: ``nb_iter`` outer
    iterations of z-step (``nb_inner`` iterations, warm-started) and theta-step, then a closing z-step.

    Returns ``(X, Z, W, H, d)``: ``X, Z, W`` float64 CUDA ``(V, N)`` in the caller's row order, ``H`` float64 CUDA
    ``(G, K)`` with one HRF per parcel, and ``d`` with ``'labels'`` (the G distinct labels: row ``g`` of ``H``, column
    ``g`` of ``'theta'`` and ``'J'`` belong to ``d['labels'][g]``), ``'sizes'`` (voxels per parcel), ``'theta'``
    ``(nb_iter + 1, G)`` and ``'J'`` ``(nb_iter + 2, G)``, the cost of every parcel normalised by its own ``||y||^2``.
    ``force`` is handed to the z-steps (``"mfma"``, ``"valu"``: tests and measurements; ``"gsplit"``, ``"gsplit_mfma"``:
    the opt-in below).  Up to 310 scans with up to 33 taps the z-steps run on the matrix pipe; 311 .. 1 280 scans with up to
    48 taps do so only by opt-in -- ``force="gsplit"`` or ``PYBOLD_AMD_PARCELS_SPLIT=1`` in the environment, which adds
    ``PB_FLAG_GROUPED_SPLIT`` to whatever ``force`` says (:func:`pybold_amd.solver.fista_solve_grouped`) -- and on the
    per-problem vector forms otherwise.  Rows are sorted by label
    once; with ``verbose=0`` nothing returns to the host before the loop ends.  ``guard`` (opt-in; ``None``: the environment
    variable ``PYBOLD_AMD_PP_GUARD``, ``"1"`` is on, read when the loop starts): every z-step through the conditioning guard
    (:func:`pybold_amd.solver.fista_solve_grouped`); ``d['guard'] = {'float64': n, 'vector': n}`` are the counts of the
    last z-step, read after the loop."""
    if not torch.is_tensor(Y):
        Y = torch.from_numpy(np.ascontiguousarray(np.asarray(Y), dtype=np.float32)).to(solver.device())
    if Y.dim() != 2 or Y.dtype != torch.float32 or not Y.is_cuda:
        raise TypeError("Y must be (V, N): a NumPy array or a float32 CUDA tensor")
    V, n = Y.shape
    if V == 0:
        raise ValueError("bd_parcels: empty voxel batch")
    if torch.is_tensor(lbda) or np.ndim(lbda) > 0:
        raise ValueError("bd_parcels: lbda must be a scalar")
    distinct, order, offsets = sort_by_label(labels)
    if order.size != V:
        raise ValueError("bd_parcels: labels must hold one label per voxel (%d), got %d" % (V, order.size))
    G = distinct.size
    dev = Y.device
    if theta_0 is not None and (torch.is_tensor(theta_0) or np.ndim(theta_0) > 0):
        th0 = np.asarray(theta_0.cpu() if torch.is_tensor(theta_0) else theta_0, dtype=np.float64).ravel()
        if th0.size != G:
            raise ValueError("bd_parcels: theta_0 must be a scalar or hold one dilation per parcel (%d), got %d" % (G, th0.size))
    else:
        th0 = np.full((G,), MAX_DELTA if theta_0 is None else float(theta_0))
    if th0.min() < MIN_DELTA or th0.max() > MAX_DELTA:
        raise ValueError("bd_parcels: theta_0 must lie in [%g, %g]" % (MIN_DELTA, MAX_DELTA))
    if bounds is None:
        bounds = [(MIN_DELTA + 1.0e-1, MAX_DELTA - 1.0e-1)]
    order_dev = torch.from_numpy(order).to(dev)
    po = solver.ParcelOffsets(offsets, dev)
    Ys = Y.index_select(0, order_dev).contiguous()
    theta = torch.from_numpy(th0).to(dev)
    guard_work = solver.guard_work_buffer(V, n, dev) if solver.pp_guard_opt_in(guard) else None
    Ws, taps, thetas, costs = _parcel_loop(Ys, po, t_r, float(lbda), theta, hrf_dur, bounds, int(nb_iter), int(nb_inner), force,
                                           guard_work)
    row_parcel = torch.repeat_interleave(torch.arange(G, device=dev), torch.from_numpy(po.sizes).to(dev))
    Xs, Zs = solver.fista_outputs_pp(Ws, taps.index_select(0, row_parcel))
    X, Z, W = (torch.empty_like(Ws).index_copy_(0, order_dev, T) for T in (Xs, Zs, Ws))
    d = {"labels": distinct, "sizes": po.sizes.copy(),
         "theta": torch.stack(thetas).cpu().numpy(),
         "J": np.concatenate([np.ones((1, G)), torch.stack(costs).cpu().numpy()])}
    if guard_work is not None:
        d["guard"] = solver.guard_counts(guard_work)
    if verbose > 0:
        for it in range(nb_iter + 1):
            th = d["theta"][min(it + 1, nb_iter)]
            print("bd_parcels outer %d: theta in [%.4f, %.4f], median J %.6f" % (it, th.min(), th.max(), np.median(d["J"][it + 1])))
    return X, Z, W, taps, d
