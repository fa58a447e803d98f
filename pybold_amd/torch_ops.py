"""``torch.ops.pybold_hip``: the solver entry points as registered PyTorch operators
(``pybold_amd/csrc/torch_ops.cpp``, a ``TORCH_LIBRARY`` shim over the C ABI of
``libpybold_hip.so``): tensors in, launches on PyTorch's current stream of the tensors' device,
``RuntimeError`` with the library's message on a bad call.  ``load()`` registers them (once) and
returns the ``torch.ops.pybold_hip`` namespace; the ctypes path (``pybold_amd.solver``) and this one
call the same kernels."""
import os

import torch

from . import solver

_HERE = os.path.dirname(os.path.abspath(__file__))
OPS_PATH = os.path.join(_HERE, "libpybold_torch_ops.so")
_loaded = False


def load():
    global _loaded
    if not _loaded:
        if not os.path.exists(OPS_PATH):
            raise ImportError("pybold_amd: %s not found; build it with `make -C pybold_amd/csrc` "
                              "(needs PyTorch's headers)" % OPS_PATH)
        torch.ops.load_library(OPS_PATH)
        _loaded = True
    return torch.ops.pybold_hip


def fista_solve(Y, hrf, lbda, step, n_iter, W0=None, want_J=False, stop_mode=0, tol=0.0, wind=6, y_rep=1, flags=0):
    """The same contract as :func:`pybold_amd.solver.fista_solve` through ``torch.ops.pybold_hip.fista_solve``
    (scalar ``lbda``); returns ``(W, J or None, n_done)``."""
    import numpy as np
    ops = load()
    dev = Y.device
    taps = torch.from_numpy(np.ascontiguousarray(np.asarray(hrf, dtype=np.float64).ravel()))
    P, N = Y.shape[0] * int(y_rep), Y.shape[1]
    if W0 is None:
        W = torch.empty((P, N), dtype=torch.float64, device=dev)
        flags |= solver.PB_FLAG_COLD_START
    else:
        W = W0.clone()
    J = torch.full((P, max(int(n_iter), 1)), float("nan"), dtype=torch.float32, device=dev) if want_J else None
    n_done = torch.empty((P,), dtype=torch.int32, device=dev)
    lbda_vec = None if np.ndim(lbda) == 0 and not torch.is_tensor(lbda) else torch.as_tensor(lbda, dtype=torch.float64).to(dev)
    ops.fista_solve(Y, W, taps, taps.to(dev), float(step), 0.0 if lbda_vec is not None else float(lbda), lbda_vec,
                    solver._betas_on(dev, int(n_iter)), int(n_iter), J, int(stop_mode), float(tol), int(wind), n_done,
                    int(y_rep), int(flags))
    return W, J, n_done


def _auto_lbda_solve(op, Y, hrf, step, sigma, early_stopping, tol, wind, nb_iter, nb_sub_iter, outer_chunk, W0, want_trace):
    import numpy as np
    ops = load()
    dev = Y.device
    taps = torch.from_numpy(np.ascontiguousarray(np.asarray(hrf, dtype=np.float64).ravel()))
    W = torch.empty_like(Y) if W0 is None else W0.clone()
    R, G, J = (torch.full((Y.shape[0], int(nb_iter)), float("nan"), dtype=torch.float64, device=dev)
               for _ in range(3)) if want_trace else (None, None, None)
    alpha, lbda, n_outer, n_inner = getattr(ops, op)(
        Y, W, W0 is None, taps, float(step), solver._betas_on(dev, int(nb_sub_iter)),
        torch.as_tensor(sigma, dtype=torch.float64).to(dev).contiguous().ravel(), bool(early_stopping), float(tol),
        int(wind), int(nb_iter), int(nb_sub_iter), int(outer_chunk), R, G, J)
    return W, {"alpha": alpha, "lbda": lbda, "n_outer": n_outer, "n_inner": n_inner, "R": R, "G": G, "J": J}


def _bind_search(op, like):
    def search(Y, hrf, step, sigma, early_stopping=True, tol=1.0e-6, wind=6, nb_iter=1000, nb_sub_iter=1000,
               outer_chunk=0, W0=None, want_trace=True):
        return _auto_lbda_solve(op, Y, hrf, step, sigma, early_stopping, tol, wind, nb_iter, nb_sub_iter,
                                outer_chunk, W0, want_trace)
    search.__name__ = search.__qualname__ = op
    search.__doc__ = "The same contract as :func:`pybold_amd.solver.%s` through ``torch.ops.pybold_hip.%s``." % (like, op)
    return search


for _form in solver.F64_FORMS.values():                # auto_lbda_solve, _split, _long, _split_long: one per form's operator
    globals()[_form.op] = _bind_search(_form.op, _form.public.search)


def mad_daub_noise_est(Y, c=0.6744):
    """``torch.ops.pybold_hip.mad_daub_noise_est``: the noise level of every row of a CUDA ``(V, N)`` tensor."""
    return load().mad_daub_noise_est(Y, float(c))
