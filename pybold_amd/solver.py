"""Device-level batched API over the C ABI (``include/pybold_hip.h``).

Everything here takes and returns ``torch`` CUDA tensors (PyTorch is used for
device memory and streams only); the arithmetic happens in the hand-written
HIP kernels of ``libpybold_hip.so``.  Rows are problems ("voxels"), the last
dimension is time.
"""
import collections
import os

import numpy as np
import torch

from . import _lib
from ._lib import (PB_FLAG_COLD_START, PB_FLAG_NO_CERT, PB_FLAG_FORCE_CERT, PB_FLAG_DIRECT_FIR, PB_FLAG_ONE_STREAM, PB_FLAG_FORCE_FAST, PB_FLAG_FORCE_GENERIC, PB_FLAG_FORCE_PAIR, PB_FLAG_FORCE_WIDE,
                   PB_FLAG_NO_PAIR, PB_FLAG_ONE_LAUNCH, PB_STOP_LOOPS, PB_STOP_NONE, PB_STOP_WINDOW)

_STOP = {None: PB_STOP_NONE, "none": PB_STOP_NONE, "loops": PB_STOP_LOOPS,
         "window": PB_STOP_WINDOW}
# "fast" = a register-resident kernel (library picks single-row or pair form);
# "fast1" / "fast2" pin the single-row / two-problems-per-row form
# "wide" pins the one-problem-per-wave form; "one" = library dispatch restricted to a single launch;
# "fast2d" / "direct": pair form with direct FIRs instead of the 2-parallel fast FIRs;
# "seq": library dispatch without the internal side stream
_FORCE = {None: 0, "generic": PB_FLAG_FORCE_GENERIC, "fast": PB_FLAG_FORCE_FAST,
          "fast1": PB_FLAG_FORCE_FAST | PB_FLAG_NO_PAIR | PB_FLAG_ONE_LAUNCH,
          "fast2": PB_FLAG_FORCE_FAST | PB_FLAG_FORCE_PAIR | PB_FLAG_ONE_LAUNCH,
          "fast2d": PB_FLAG_FORCE_FAST | PB_FLAG_FORCE_PAIR | PB_FLAG_ONE_LAUNCH | PB_FLAG_DIRECT_FIR,
          "direct": PB_FLAG_DIRECT_FIR,
          "wide": PB_FLAG_FORCE_FAST | PB_FLAG_FORCE_WIDE | PB_FLAG_ONE_LAUNCH,
          "one": PB_FLAG_ONE_LAUNCH, "seq": PB_FLAG_ONE_STREAM,
          # window rule: "cert" = no-fire certificate on the pair form + exact re-solve whatever
          # tol * n_iter is; "nocert" = always the full rule (single-row form)
          "cert": PB_FLAG_FORCE_CERT, "cert2": PB_FLAG_FORCE_CERT | PB_FLAG_FORCE_PAIR | PB_FLAG_ONE_LAUNCH,
          "certonly": PB_FLAG_FORCE_CERT | PB_FLAG_FORCE_PAIR | PB_FLAG_ONE_LAUNCH | _lib.PB_FLAG_CERT_NO_RESOLVE,
          "nocert": PB_FLAG_NO_CERT,
          # "valu": library dispatch without the matrix-pipe form; "mfma": everything on it, one launch
          "valu": _lib.PB_FLAG_NO_MFMA, "valuseq": _lib.PB_FLAG_NO_MFMA | PB_FLAG_ONE_STREAM,
          "mfma": PB_FLAG_ONE_LAUNCH | _lib.PB_FLAG_FORCE_MFMA,
          # the same on the two dense near tiles (plain solves with up to 32 taps take the 2:4-sparse joined tile otherwise);
          # "dense_tiles": library dispatch with that kernel
          "mfma_dense": PB_FLAG_ONE_LAUNCH | _lib.PB_FLAG_FORCE_MFMA | _lib.PB_FLAG_MFMA_DENSE_TILES,
          "dense_tiles": _lib.PB_FLAG_MFMA_DENSE_TILES,
          "mfma_denseonly": PB_FLAG_ONE_LAUNCH | _lib.PB_FLAG_FORCE_MFMA | _lib.PB_FLAG_MFMA_DENSE_TILES | _lib.PB_FLAG_CERT_NO_RESOLVE,
          # "mfma2": everything on the matrix-pipe form with each series split over two waves, one launch
          # a partitioned call, measurement aids: only the dense class is solved / only the sparse class
          "path_dense": _lib.PB_FLAG_ONLY_DENSE, "path_sparse": _lib.PB_FLAG_ONLY_SPARSE,
          # the host-side plan of round 4 (no partition on the device)
          "noill": _lib.PB_FLAG_NO_ILL_GUARD,     # partitioned, but ill-conditioned series stay with their class (measurement aid)
          "nopart": _lib.PB_FLAG_NO_PARTITION, "nopartseq": _lib.PB_FLAG_NO_PARTITION | PB_FLAG_ONE_STREAM,
          "mfma2": _lib.PB_FLAG_FORCE_MFMA2, "mfma2only": _lib.PB_FLAG_FORCE_MFMA2 | _lib.PB_FLAG_CERT_NO_RESOLVE,
          "mfma2cert": _lib.PB_FLAG_FORCE_MFMA2 | PB_FLAG_FORCE_CERT,
          "mfma2certonly": _lib.PB_FLAG_FORCE_MFMA2 | PB_FLAG_FORCE_CERT | _lib.PB_FLAG_CERT_NO_RESOLVE,
          # intermediate solve of an outer loop: the matrix-pipe form keeps sparse iterates (no accuracy guard)
          "intermediate": _lib.PB_FLAG_NO_RHO_GUARD,
          "intermediate_noresolve": _lib.PB_FLAG_NO_RHO_GUARD | _lib.PB_FLAG_CERT_NO_RESOLVE,   # measurement aid
          # diagnostic: no re-solve of the problems a guard handed back (they keep n_done = -1)
          "noresolve": _lib.PB_FLAG_CERT_NO_RESOLVE,          # ... through the default dispatch
          "mfmaonly": PB_FLAG_ONE_LAUNCH | _lib.PB_FLAG_FORCE_MFMA | _lib.PB_FLAG_CERT_NO_RESOLVE,
          "mfmacert": PB_FLAG_ONE_LAUNCH | _lib.PB_FLAG_FORCE_MFMA | PB_FLAG_FORCE_CERT,
          "mfmacertonly": PB_FLAG_ONE_LAUNCH | _lib.PB_FLAG_FORCE_MFMA | PB_FLAG_FORCE_CERT | _lib.PB_FLAG_CERT_NO_RESOLVE,
          # fista_solve_grouped only (opt-in): 311 .. 1 280 scans on the split matrix-pipe forms -- "gsplit": library dispatch;
          # "gsplit_mfma": every unit on them, one launch; "gsplit_mfmaonly": ... and no re-solve of what the guards hand back
          "gsplit": _lib.PB_FLAG_GROUPED_SPLIT,
          "gsplit_mfma": PB_FLAG_ONE_LAUNCH | _lib.PB_FLAG_FORCE_MFMA | _lib.PB_FLAG_GROUPED_SPLIT,
          "gsplit_mfmaonly": PB_FLAG_ONE_LAUNCH | _lib.PB_FLAG_FORCE_MFMA | _lib.PB_FLAG_GROUPED_SPLIT | _lib.PB_FLAG_CERT_NO_RESOLVE,
          # "mfma_row": every row on the one-series-per-wave matrix-pipe kernel alone (129 .. 320 scans, up to 33 taps, plain
          # solves; rows its guards hand back keep n_done = -1, no re-solve); "vector_leftovers": library dispatch without that
          # kernel -- what whole rounds leave of the dense class stays on the vector kernel (A/B runs, fallback)
          "mfma_row": _lib.PB_FLAG_FORCE_MFMA_ROW, "vector_leftovers": _lib.PB_FLAG_VECTOR_LEFTOVERS}

# The float64 register family, one row per form: what Python has to know of `kF64[]` (csrc/dispatch.h).  No limit
# of a form stands here -- the `*_supported` queries ask the library.  `force`: the name that asks a float64 solve for the form;
# `solve` / `solve_pp`: the C entry point and flag bits that name selects with the taps on the host / with one HRF per problem
# (None: no such solve); `solve_query`, `search_query`: its `pb_*_supported` queries; `search`, `search_pp`: its lambda-search
# entry points; `op`: its `torch.ops.pybold_hip` search operator; `public`: the names of this module bound to it (below, beside
# `_auto_lbda_solve`) -- the search, the search with one HRF per problem, the solve query, the search query.
_F64Names = collections.namedtuple("_F64Names", "search search_pp solve_query search_query")
_F64Form = collections.namedtuple("_F64Form", "key force solve solve_pp solve_query search_query search search_pp op public")
F64_FORMS = collections.OrderedDict((f.key, f) for f in (
    _F64Form("one_wave", "fast",
             ("pb_fista_solve_d", PB_FLAG_FORCE_FAST), ("pb_fista_solve_pp_d", PB_FLAG_FORCE_FAST),
             None, "pb_auto_lbda_supported", "pb_auto_lbda_d", "pb_auto_lbda_pp_d", "auto_lbda_solve",
             _F64Names("auto_lbda_solve", "auto_lbda_solve_pp", None, "auto_lbda_supported")),
    _F64Form("four_waves", "split",
             None, ("pb_fista_solve_pp_d", _lib.PB_FLAG_PP_SPLIT),
             "pb_fista_pp_split_supported", "pb_auto_lbda_split_supported", "pb_auto_lbda_split_d", "pb_auto_lbda_split_pp_d",
             "auto_lbda_solve_split",
             _F64Names("auto_lbda_solve_split", "auto_lbda_solve_split_pp", "pp_split_supported", "auto_lbda_split_supported")),
    _F64Form("long", "long_hrf",
             ("pb_fista_solve_d", _lib.PB_FLAG_LONG_HRF), ("pb_fista_solve_pp_d", _lib.PB_FLAG_LONG_HRF),
             "pb_fista_long_hrf_supported", "pb_auto_lbda_long_supported", "pb_auto_lbda_long_d", "pb_auto_lbda_long_pp_d",
             "auto_lbda_solve_long",
             _F64Names("auto_lbda_solve_long", "auto_lbda_solve_long_pp", "long_hrf_supported", "auto_lbda_long_supported")),
    # (the four-wave form for long HRFs has solve entry points of its own, with the same parameter lists, in the place of a flag)
    _F64Form("four_waves_long", "split_long_hrf",
             ("pb_fista_solve_split_long_d", 0), ("pb_fista_solve_split_long_pp_d", 0),
             "pb_fista_split_long_hrf_supported", "pb_auto_lbda_split_long_supported", "pb_auto_lbda_split_long_d",
             "pb_auto_lbda_split_long_pp_d", "auto_lbda_solve_split_long",
             _F64Names("auto_lbda_solve_split_long", "auto_lbda_solve_split_long_pp", "split_long_hrf_supported",
                       "auto_lbda_split_long_supported"))))
_F64_BY_FORCE = dict((f.force, f) for f in F64_FORMS.values())
_F64_SPLIT_PP_ONLY = "force='split' names the four-wave form with one HRF per problem: fista_solve_pp_d only"
_F64_FORCE_NAMES = {          # what a float64 solve answers to any other `force`: taps on the host / one HRF per problem
    False: "float64 y: force must be None, 'fast' (register-resident float64 "
           "kernel, one problem per wave), 'generic' (LDS kernel), 'long_hrf' (the register form "
           "for HRFs of up to 48 taps, up to 640 scans) or 'split_long_hrf' (the same over four waves, "
           "641..1280 scans)",
    True: "float64 y: force must be None, 'fast' (register-resident float64 kernel, one problem per "
          "wave), 'split' (the same over four waves, 641..1280 scans), 'generic' (LDS kernel), "
          "'long_hrf' (one problem per wave, HRFs of up to 48 taps) or 'split_long_hrf' (four waves, "
          "641..1280 scans, HRFs of up to 48 taps)"}


def _f64_solve_route(force, pp):
    """``(C entry point, flag bits)`` of a float64 solve asked for by ``force`` -- :func:`fista_solve_pp_d` (``pp``) or
    :func:`fista_solve` on a float64 ``Y``; ``ValueError`` for a name that is no float64 form's."""
    if force in (None, "generic"):                      # the library's dispatch / its LDS kernel: no form of the table
        return "pb_fista_solve_pp_d" if pp else "pb_fista_solve_d", _FORCE[force]
    form = _F64_BY_FORCE.get(force)
    route = form and (form.solve_pp if pp else form.solve)
    if route:
        return route
    raise ValueError(_F64_SPLIT_PP_ONLY if force == "split" else _F64_FORCE_NAMES[pp])


_warned = set()


def warn_once(key, message, stacklevel=3):
    """One ``RuntimeWarning`` per process and ``key``: the silent performance cliffs of the
    dispatch (LDS kernel, all-float64 kernel) are made loud here, not in a header."""
    if key not in _warned:
        _warned.add(key)
        import warnings
        warnings.warn(message, RuntimeWarning, stacklevel=stacklevel)


def _warn_if_slow_kernel(lib, N, K, P, want_J, stop, wind, flags):
    """The any-size LDS kernel is 10-20x slower per voxel-iteration than the register-resident
    forms; say so once when a batch of some size lands on it by dispatch (not by `force`)."""
    if P < 256 or (flags & (PB_FLAG_FORCE_GENERIC | PB_FLAG_FORCE_FAST)):
        return
    form = lib.pb_fista_which_kernel(int(N), int(K), int(P), int(bool(want_J)), _STOP[stop], int(wind))
    if form in (1, 2, 3) and P >= 16384 and not (flags & (_lib.PB_FLAG_NO_MFMA | PB_FLAG_NO_PAIR | PB_FLAG_FORCE_PAIR | PB_FLAG_FORCE_WIDE)):
        # a machine-filling batch on a vector form although a matrix-pipe form exists for neighbouring shapes: say which
        # limit the call ran into (rates at 300 / 600 scans: matrix pipe 4.8 / 2.0e9 voxel-iterations/s, vector forms
        # 1.4-3.0e9, one problem per wave 0.5-0.6e9 -- DESIGN 6)
        why = []
        if N <= 128:
            why = []                                  # (short series: the pair form is the fast one there)
        elif N > 1280:
            why.append("series of %d scans (matrix-pipe forms: 129..1280)" % N)
        elif K > 48 or (K > 33 and _STOP[stop] != PB_STOP_NONE and N <= 224):
            why.append("HRF of %d taps (matrix-pipe forms: <= 48 taps; <= 33 with a stop rule up to 224 scans)" % K)
        elif _STOP[stop] == PB_STOP_LOOPS and want_J:
            why.append("the _loops_deconv rule with a cost trace")
        elif _STOP[stop] == PB_STOP_WINDOW:
            why.append("the window rule with wind=%d / this tolerance (matrix pipe: wind = 6 and tol * n_iter < 0.02)" % wind)
        if why:
            warn_once(("vector", N, K, _STOP[stop], wind, bool(want_J)),
                      "pybold_amd: %d problems (N=%d, K=%d) run on the float32 vector forms (%s), 1.5-4x below the "
                      "matrix-pipe rate: %s" % (P, N, K, KERNEL_NAMES[form].split(" (")[0], "; ".join(why)))
    if form != 0:
        return
    why = []
    if _STOP[stop] == PB_STOP_WINDOW and wind not in (4, 6, 8):
        why.append("wind=%d (register-resident window rule: wind in {4, 6, 8})" % wind)
    if _STOP[stop] == PB_STOP_WINDOW and N > 1216:
        why.append("window rule beyond 1216 scans")
    if K > 48:
        why.append("HRF of %d taps (> 48)" % K)
    if N > 2432:
        why.append("series of %d scans (> 2432)" % N)
    warn_once(("lds", N, K, _STOP[stop], wind),
              "pybold_amd: %d problems (N=%d, K=%d) run on the any-size LDS kernel, 10-20x slower per "
              "voxel-iteration than the register-resident kernels: %s" % (P, N, K, "; ".join(why) or "shape outside the tables"))


def device(dev=None):
    """The HIP device to run on; raises when no GPU is visible (no CPU path)."""
    if not torch.cuda.is_available():
        raise RuntimeError("pybold_amd needs a ROCm GPU (MI355X); none is visible "
                           "and there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)


def momentum_betas(n_iter, t0=1.0):
    """``beta_k = (t_k - 1) / t_{k+1}`` with ``t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2``
    in float64, exactly the scalar sequence of pybold/bold_signal.py:60,68-71."""
    betas = np.empty(n_iter, dtype=np.float64)
    t_old = float(t0)
    for k in range(n_iter):
        t = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t_old ** 2))
        betas[k] = (t_old - 1.0) / t
        t_old = t
    return betas


_beta_cache = {}


def _betas_on(dev, n_iter):
    key = (dev.type, dev.index)
    cur = _beta_cache.get(key)
    if cur is None or cur.numel() < n_iter:
        n = max(n_iter, 1024, 2 * (cur.numel() if cur is not None else 0))
        cur = torch.from_numpy(momentum_betas(n)).to(dev)
        _beta_cache[key] = cur
    return cur


_inited = set()


def _ensure_init(dev):
    """The first use of a device asks the library for its side stream (``pb_init``): created
    before the application's own streams it overlaps best with the caller's
    (include/pybold_hip.h)."""
    if dev.index not in _inited:
        _inited.add(dev.index)
        with torch.cuda.device(dev):
            _lib.load().pb_init()           # optional: a failure only postpones the creation


def _stream_ptr(dev):
    _ensure_init(dev)
    return torch.cuda.current_stream(dev).cuda_stream


def _as_taps(hrf):
    taps = np.ascontiguousarray(np.asarray(hrf, dtype=np.float64).ravel())
    if taps.size < 1:
        raise ValueError("empty HRF")
    return taps


def _rows(t, dtype, name):
    if t.dim() != 2:
        raise ValueError("%s must be 2-D (problems, time), got %s" % (name, tuple(t.shape)))
    if t.dtype != dtype or not t.is_cuda:
        raise TypeError("%s must be a CUDA tensor of %s" % (name, dtype))
    if t.stride(1) != 1:
        t = t.contiguous()
    return t


def _y_rows(Y, fn_f32, fn_f64):
    """Observed series are float32 (batch layout) or float64 (reference arithmetic):
    returns the checked tensor and the matching entry point."""
    if torch.is_tensor(Y) and Y.dtype == torch.float64:
        return _rows(Y, torch.float64, "Y"), fn_f64
    return _rows(Y, torch.float32, "Y"), fn_f32


def _ld(t):
    """Leading dimension in elements (a single-row view may report stride 0)."""
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _warm_start(W0, shape, dev, inplace=False):
    """``(W, cold flag)``: the iterate a solve works in.  Without ``W0`` the kernels start from 0 themselves (no memset, no
    read: ``PB_FLAG_COLD_START``); else a copy of ``W0`` -- with ``inplace``, ``W0`` itself where its rows need no copy."""
    if W0 is None:
        return torch.empty(shape, dtype=torch.float64, device=dev), PB_FLAG_COLD_START
    W = _rows(W0, torch.float64, "W0")
    if not inplace or W.data_ptr() != W0.data_ptr():
        W = W.clone()
    if W.shape != shape:
        raise ValueError("W0 must be %s, got %s" % (shape, tuple(W.shape)))
    return W, 0


def _lbda_arg(lbda, dev, n=None):
    """``(lbda_scalar, lbda_dev)``: a scalar as a number, anything else as a float64 vector on ``dev`` (of ``n`` entries,
    where the caller says how many)."""
    if np.ndim(lbda) == 0 and not torch.is_tensor(lbda):
        return float(lbda), None
    lbda_dev = torch.as_tensor(lbda, dtype=torch.float64).to(dev).contiguous().ravel()
    if n is not None and lbda_dev.numel() != n:
        raise ValueError("per-problem lbda must have %d entries" % n)
    return 0.0, lbda_dev


def has_fast_path(n_scans, n_taps):
    return bool(_lib.load().pb_fista_has_fast_path(int(n_scans), int(n_taps)))


KERNEL_NAMES = {0: "fista_generic_kernel (LDS)", 1: "fista_fast_kernel (register-resident)",
                2: "fista_pair_ffa_kernel (register-resident, two problems per row, fast FIRs)",
                3: "fista_fast_kernel (register-resident, one problem per wave)",
                4: "fista_mfma_kernel (register-resident, 16 problems per wave, both operators on the matrix pipe)",
                5: "fista_mfma2_kernel (register-resident, 16 problems per two waves -- every series split over two "
                   "SIMDs --, both operators on the matrix pipe)",
                6: "fista_mfma4_kernel (register-resident, 16 problems per workgroup of four waves -- every series split over "
                   "the four SIMDs of a compute unit --, both operators on the matrix pipe)",
                7: "fista_exact_kernel (register-resident, float64 end to end, one problem per wave)",
                8: "fista_exact_split_kernel (register-resident, float64 end to end, one problem per workgroup of four "
                   "waves)",
                9: "fista_exact_pp_kernel (register-resident, float64 end to end, one problem per wave, one HRF per problem)"}


def which_kernel(n_scans, n_taps, n_problems, want_J=False, stop=None, wind=6):
    """Name of the kernel :func:`fista_solve` dispatches to for this call shape."""
    return KERNEL_NAMES[_lib.load().pb_fista_which_kernel(
        int(n_scans), int(n_taps), int(n_problems), int(bool(want_J)), _STOP[stop], int(wind))]


def which_kernel_f64(n_scans, n_taps, want_J=False, stop=None, wind=6):
    """Name of the kernel :func:`fista_solve` dispatches to for a float64 ``Y`` of this shape (``pb_fista_solve_d``: the
    1-D calls of the API, ``deconv(lbda=None)``); raises ``ValueError`` where not even the LDS kernel holds the shape."""
    form = _lib.load().pb_fista_which_kernel_d(int(n_scans), int(n_taps), int(bool(want_J)), _STOP[stop], int(wind))
    if form < 0:
        raise ValueError("no float64 kernel for %d scans, %d taps, wind=%d: the series exceeds LDS" % (n_scans, n_taps, wind))
    return KERNEL_NAMES[form]


def which_kernel_pp_f64(n_scans, n_taps, want_J=False, stop=None, wind=6):
    """Name of the kernel :func:`fista_solve_pp_d` dispatches to for this shape (``pb_fista_which_kernel_pp_d``); raises
    ``ValueError`` where not even the LDS kernel holds the shape."""
    form = _lib.load().pb_fista_which_kernel_pp_d(int(n_scans), int(n_taps), int(bool(want_J)), _STOP[stop], int(wind))
    if form < 0:
        raise ValueError("no float64 kernel for %d scans, %d taps, wind=%d: the series exceeds LDS" % (n_scans, n_taps, wind))
    return KERNEL_NAMES[form]


def launch_plan(n_scans, n_taps, n_problems, stop=None, wind=6, force=None):
    """``(n_main, main kernel, tail kernel)``: how :func:`fista_solve` lays the problems out --
    the first ``n_main`` (whole rounds of waves) in one launch, the rest in a second one
    (``force="valu"``: the plan without the matrix-pipe form)."""
    import ctypes
    nm, mf, tf = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.load().pb_fista_plan_ex(int(n_scans), int(n_taps), int(n_problems), _STOP[stop], int(wind),
                                 _FORCE[force], ctypes.byref(nm), ctypes.byref(mf), ctypes.byref(tf))
    return nm.value, (KERNEL_NAMES[mf.value] if nm.value else None), KERNEL_NAMES[tf.value]


def fista_solve(Y, hrf, lbda, step, n_iter, W0=None, want_J=False, stop=None,
                tol=0.0, wind=6, y_rep=1, force=None, lmax=None, dense_ratio=0.0):
    """Run ``n_iter`` iterations of the reference recurrence
    (pybold/bold_signal.py:62-72, :259-276) for every row of ``Y`` in one launch.

    Y     float32 CUDA ``(V, N)`` (the batch layout; register-resident kernels), or
          float64 CUDA ``(V, N)``: float64 end to end (``pb_fista_solve_d``: register-resident
          kernels for K <= 32 -- one problem per wave for N <= 640, one per workgroup of four
          waves for N <= 1280 --, else the LDS kernel; :func:`which_kernel_f64`), the
          reference's arithmetic -- what the 1-D calls of the API use.  ``force="long_hrf"`` (opt-in,
          ``PB_FLAG_LONG_HRF``): the one-wave register form for HRFs of up to 48 taps, ``N <= 640``, window rule at
          ``wind == 6`` -- :func:`long_hrf_supported`; any other shape is an error.  Without it 33+ taps run on the
          LDS kernel.  ``force="split_long_hrf"`` (opt-in, ``pb_fista_solve_split_long_d``): the same holder with one problem per
          workgroup of four waves, ``641 <= N <= 1280``, ``K <= 48`` -- :func:`split_long_hrf_supported`; any other shape
          is an error
    hrf   1-D array of K taps (host)
    lbda  scalar, or array/tensor of ``V * y_rep`` per-problem values
    step  ``1 / L``
    W0    optional float64 CUDA ``(P, N)`` warm start (not modified)
    stop  None | "loops" (_loops_deconv rule) | "window" (deconv rule)
    lmax  optional float64 CUDA ``(V,)``: :func:`lambda_max` of every series, if the caller has it (a regularisation
          path, BASELINE config 5, does); otherwise the library computes it when it partitions the call: the problems
          with ``lbda < dense_ratio * lmax`` run on the matrix-pipe form, the sparse rest on the float32 vector forms
          (``pb_fista_solve_ex``; any call shape since round 5).  ``dense_ratio <= 0`` takes the default for the series
          length: ``PB_PATH_DENSE_RATIO`` 0.19 up to 310 scans, ``_LONG`` 0.22 up to 640, ``_LONGER`` 0.26 up to 1 280
    Returns ``(W float64 (P, N), J float32 (P, n_iter) or None, n_done int32 (P,))``.
    """
    if force == "split":
        raise ValueError(_F64_SPLIT_PP_ONLY)
    lib = _lib.load()
    f64 = torch.is_tensor(Y) and Y.dtype == torch.float64
    if force == "long_hrf" and not f64:
        raise ValueError("force='long_hrf' names the float64 register form for HRFs of up to 48 taps: float64 Y only")
    if force == "split_long_hrf" and not f64:
        raise ValueError("force='split_long_hrf' names the four-wave float64 register form for HRFs of up to 48 taps: "
                         "float64 Y only")
    Y = _rows(Y, torch.float64 if f64 else torch.float32, "Y")
    dev = Y.device
    V, N = Y.shape
    P = V * int(y_rep)
    taps = _as_taps(hrf)
    taps_dev = torch.from_numpy(taps).to(dev)
    W, cold = _warm_start(W0, (P, N), dev)
    if not f64 and not (torch.is_tensor(lbda) and lbda.is_cuda) and (np.asarray(lbda) < 0).any():
        # pybold/bold_signal.py:66 with a negative threshold GROWS every entry (its lambda search gets there,
        # :141-145); only the float64 kernels restate that expression, the float32-FIR kernels clamp
        raise ValueError("negative lbda: only the float64 path (float64 Y) reproduces the reference's prox for it")
    lbda_scalar, lbda_dev = _lbda_arg(lbda, dev, P)
    betas = _betas_on(dev, n_iter)
    J = torch.empty((P, max(n_iter, 1)), dtype=torch.float64 if f64 else torch.float32,
                    device=dev) if want_J else None
    if J is not None:
        J.fill_(float("nan"))
    n_done = torch.empty((P,), dtype=torch.int32, device=dev)
    if f64:
        entry, flags = _f64_solve_route(force, pp=False)
        with torch.cuda.device(dev):
            rc = getattr(lib, entry)(
                Y.data_ptr(), _ld(Y), int(y_rep), W.data_ptr(), _ld(W), P, N,
                taps.ctypes.data, taps_dev.data_ptr(), taps.size, float(step), lbda_scalar,
                lbda_dev.data_ptr() if lbda_dev is not None else None,
                betas.data_ptr(), int(n_iter),
                J.data_ptr() if J is not None else None, _ld(J) if J is not None else 0,
                _STOP[stop], float(tol), int(wind), n_done.data_ptr(), flags | cold,
                _stream_ptr(dev))
        _lib.check(rc, entry)
        return W, J, n_done
    # Every float32 call goes through pb_fista_solve_ex with a workspace: where the matrix-pipe form can carry the call
    # (129..310 scans, >= 4 096 problems) the problems are partitioned on the device -- dense class on the matrix
    # pipe, sparse class (lambda near lambda_max) on the float32 vector forms -- so that nothing is solved twice.
    if lmax is not None:
        lmax = lmax.to(device=dev, dtype=torch.float64).contiguous().ravel()
        if lmax.numel() != V:
            raise ValueError("lmax must have one entry per series (%d)" % V)
    work = torch.empty((int(lib.pb_fista_work_len(P, int(y_rep))),), dtype=torch.int32, device=dev)
    _warn_if_slow_kernel(lib, N, taps.size, P, want_J, stop, wind, _FORCE[force])
    with torch.cuda.device(dev):
        rc = lib.pb_fista_solve_ex(
            Y.data_ptr(), _ld(Y), int(y_rep), W.data_ptr(), _ld(W), P, N,
            taps.ctypes.data, taps_dev.data_ptr(), taps.size, float(step), lbda_scalar,
            lbda_dev.data_ptr() if lbda_dev is not None else None,
            betas.data_ptr(), int(n_iter),
            J.data_ptr() if J is not None else None, _ld(J) if J is not None else 0,
            _STOP[stop], float(tol), int(wind), n_done.data_ptr(), _FORCE[force] | cold,
            _stream_ptr(dev), lmax.data_ptr() if lmax is not None else None, float(dense_ratio),
            work.data_ptr(), work.numel())
    _lib.check(rc, "pb_fista_solve_ex")
    return W, J, n_done


def fista_solve_backtrack(Y, hrf, lbda, step0, n_iter, eta=0.5, max_halvings_per_iter=40, W0=None, y_rep=1):
    """OPT-IN EXTRA (never part of a parity run; the reference has a constant step only): the recurrence of
    :func:`fista_solve` with a backtracked step -- ``pb_fista_solve_backtrack_d``.  ``Y`` float64 CUDA ``(V, N)``; ``step0``
    any positive start step (a caller without ``spectral_radius_est``).  Returns ``(W, step, halvings)``: the iterate, the
    final step and the number of step reductions of every problem."""
    lib = _lib.load()
    Y = _rows(Y, torch.float64, "Y")
    dev = Y.device
    V, N = Y.shape
    P = V * int(y_rep)
    taps_dev = torch.from_numpy(_as_taps(hrf)).to(dev)
    cold = 0
    if W0 is None:
        W = torch.empty((P, N), dtype=torch.float64, device=dev)
        cold = PB_FLAG_COLD_START
    else:
        W = _rows(W0, torch.float64, "W0").clone()        # (no shape check here: _warm_start would add one)
    lbda_scalar, lbda_dev = _lbda_arg(lbda, dev)
    betas = _betas_on(dev, n_iter)
    step =torch.empty((P,), dtype=torch.float64, device=dev)
    halv = torch.empty((P,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.pb_fista_solve_backtrack_d(
            Y.data_ptr(), _ld(Y), int(y_rep), W.data_ptr(), _ld(W), P, N, taps_dev.data_ptr(), taps_dev.numel(),
            float(step0), float(eta), int(max_halvings_per_iter), lbda_scalar,
            lbda_dev.data_ptr() if lbda_dev is not None else None, betas.data_ptr(), int(n_iter), None,
            step.data_ptr(), halv.data_ptr(), cold, _stream_ptr(dev))
    _lib.check(rc, "pb_fista_solve_backtrack_d")
    return W, step, halv


class FistaPlan:
    """Pre-allocated, launch-only form of :func:`fista_solve` for hot loops and
    graph capture: ``run()`` makes ONE ``pb_fista_solve`` call on the current stream of the
    plan's device (a cold start: no memset, the kernels start from 0) and allocates nothing.
    That call enqueues up to four kernels -- whole rounds of waves on the densest form, the
    remainder on others, part of it on the library's side stream (forked from and joined back
    into the current stream; see ``include/pybold_hip.h``)."""

    def __init__(self, Y, hrf, lbda, step, n_iter, y_rep=1, force="fast", W=None, lmax=None, dense_ratio=0.0):
        self.lib = _lib.load()
        self.Y = _rows(Y, torch.float32, "Y")
        self.dev = self.Y.device
        V, self.N = self.Y.shape
        self.P = V * int(y_rep)
        self.y_rep = int(y_rep)
        self.taps = _as_taps(hrf)
        self.taps_dev = torch.from_numpy(self.taps).to(self.dev)
        if W is None:
            W = torch.zeros((self.P, self.N), dtype=torch.float64, device=self.dev)
        elif tuple(W.shape) != (self.P, self.N) or W.stride(1) != 1:
            raise ValueError("W must be (%d, %d) with unit stride along time" % (self.P, self.N))
        self.W = _rows(W, torch.float64, "W")
        self.n_done = torch.empty((self.P,), dtype=torch.int32, device=self.dev)
        self.lbda, self.lbda_dev = _lbda_arg(lbda, self.dev)
        self.step = float(step)
        self.n_iter = int(n_iter)
        self.betas = _betas_on(self.dev, self.n_iter)
        self.flags = _FORCE[force]
        # workspace of the device-side partition (pb_fista_solve_ex); lambda_max of every series if the caller has it
        self.lmax, self.dense_ratio = None, float(dense_ratio)
        if lmax is not None:
            self.lmax = lmax.to(device=self.dev, dtype=torch.float64).contiguous().ravel()
            if self.lmax.numel() != V:
                raise ValueError("lmax must have one entry per series (%d)" % V)
        self.work = torch.empty((int(self.lib.pb_fista_work_len(self.P, self.y_rep)),), dtype=torch.int32, device=self.dev)

    def launch(self, cold=False):
        """Only the solver launch: the iterate continues from its current value, or
        (``cold``) starts from 0 without being read."""
        # the library finds its per-device side stream and wave count through the CURRENT device
        with torch.cuda.device(self.dev):
            rc = self.lib.pb_fista_solve_ex(
                self.Y.data_ptr(), _ld(self.Y), self.y_rep, self.W.data_ptr(), _ld(self.W), self.P,
                self.N, self.taps.ctypes.data, self.taps_dev.data_ptr(), self.taps.size, self.step,
                self.lbda, self.lbda_dev.data_ptr() if self.lbda_dev is not None else None,
                self.betas.data_ptr(), self.n_iter, None, 0, PB_STOP_NONE, 0.0, 0,
                self.n_done.data_ptr(), self.flags | (PB_FLAG_COLD_START if cold else 0), _stream_ptr(self.dev),
                self.lmax.data_ptr() if self.lmax is not None else None, self.dense_ratio,
                self.work.data_ptr(), self.work.numel())
        _lib.check(rc, "pb_fista_solve_ex")

    def run(self):
        """Cold start (what ``deconv`` does, pybold/bold_signal.py:57): solve from w = 0."""
        self.launch(cold=True)
        return self.W


def round_size(n_scans, n_taps, dev=None):
    """Problems in one full round of waves of the densest plain kernel form for this shape
    (two waves on every SIMD of the device), or None when only the LDS kernel applies."""
    n_main, main, tail = launch_plan(n_scans, n_taps, 1 << 22)
    # problems per wave x waves per SIMD of each form
    per_simd = {KERNEL_NAMES[4]: 16, KERNEL_NAMES[5]: 8, KERNEL_NAMES[2]: 16, KERNEL_NAMES[1]: 8,
                KERNEL_NAMES[3]: 2}.get(main if n_main else tail)
    if per_simd is None:
        return None
    return torch.cuda.get_device_properties(device(dev)).multi_processor_count * 4 * per_simd


class HostPipeline:
    """Host buffers in, (optionally) host buffers out: ``y`` (float32, pinned host memory)
    -> ``diff_z``, in chunks of ``chunk`` voxels on separate streams so that the H2D copy of
    chunk c+1 and the D2H copy of chunk c-1 overlap the solve of chunk c.

    ``out_dtype=None``: the result stays in HBM (float64 ``(V, N)``, ``self.W``);
    ``torch.float32`` / ``torch.float64``: it is copied back into pinned host memory
    (``self.out``) through two device slots of ``chunk`` voxels.  ``chunk`` defaults to one
    full round of waves (:func:`round_size`: 16 384 voxels at N <= 304), which leaves the
    solver's own cost unchanged but for the launch boundaries (measured at config-3 size:
    17.25 ms in 7 chunks against 16.76 ms in one call) and one chunk copy exposed at each end.
    Everything is allocated here; ``run`` allocates nothing."""

    def __init__(self, n_voxels, n_scans, hrf, lbda, step, n_iter, chunk=None, out_dtype=torch.float32,
                 dev=None, force=None):
        self.dev = device(dev)
        _ensure_init(self.dev)                      # the library's side stream before ours
        self.V, self.N = int(n_voxels), int(n_scans)
        if chunk is None:
            chunk = round_size(self.N, len(_as_taps(hrf)), self.dev) or 8192
            if self.V < 3 * chunk:                  # too few chunks to hide anything: measured slower
                chunk = self.V                      # than copy, solve, copy on one stream
        self.chunk = max(1, min(int(chunk), max(self.V, 1)))
        self.out_dtype = out_dtype
        self.bounds = [(lo, min(lo + self.chunk, self.V)) for lo in range(0, self.V, self.chunk)]
        self.s_in, self.s_cmp, self.s_out = (torch.cuda.Stream(self.dev) for _ in range(3))
        lam = None if (np.ndim(lbda) == 0 and not torch.is_tensor(lbda)) else \
            torch.as_tensor(lbda, dtype=torch.float64).ravel()
        self.Yd = [torch.empty((self.chunk, self.N), dtype=torch.float32, device=self.dev) for _ in range(2)]
        if out_dtype is None:
            self.W = torch.empty((self.V, self.N), dtype=torch.float64, device=self.dev)
            self.out = None
        else:
            self.W = None
            self.Wd = [torch.empty((self.chunk, self.N), dtype=torch.float64, device=self.dev) for _ in range(2)]
            self.Od = self.Wd if out_dtype == torch.float64 else [
                torch.empty((self.chunk, self.N), dtype=out_dtype, device=self.dev) for _ in range(2)]
            self.out = torch.empty((self.V, self.N), dtype=out_dtype).pin_memory()
        self.plans = []
        for c, (lo, hi) in enumerate(self.bounds):
            b = c % 2
            self.plans.append(FistaPlan(self.Yd[b][:hi - lo], hrf, lbda if lam is None else lam[lo:hi], step, n_iter,
                                        force=force, W=self.W[lo:hi] if self.W is not None else self.Wd[b][:hi - lo]))
        self.ev_in = [torch.cuda.Event() for _ in range(2)]
        self.ev_cmp = [torch.cuda.Event() for _ in range(2)]
        self.ev_out = [torch.cuda.Event() for _ in range(2)]

    def run(self, Yh, sync=True):
        """``Yh``: float32 host tensor ``(V, N)`` (pinned, or the copies are synchronous).
        Returns ``self.out`` (pinned host) or ``self.W`` (HBM); with ``sync=False`` the work is
        only enqueued and ordered before later work on the current stream."""
        if tuple(Yh.shape) != (self.V, self.N) or Yh.dtype != torch.float32 or Yh.is_cuda:
            raise ValueError("Yh must be a float32 host tensor of shape (%d, %d)" % (self.V, self.N))
        cur = torch.cuda.current_stream(self.dev)
        if len(self.bounds) == 1:                   # one chunk: everything on the current stream
            self.Yd[0][:self.V].copy_(Yh, non_blocking=True)
            self.plans[0].run()
            if self.out is not None:
                if self.Od is not self.Wd:
                    self.Od[0][:self.V].copy_(self.Wd[0][:self.V])
                self.out.copy_(self.Od[0][:self.V], non_blocking=True)
            if sync:
                cur.synchronize()
            return self.out if self.out is not None else self.W
        for s in (self.s_in, self.s_cmp, self.s_out):
            s.wait_stream(cur)
        for c, (lo, hi) in enumerate(self.bounds):
            b, n = c % 2, hi - lo
            with torch.cuda.stream(self.s_in):
                if c >= 2:
                    self.s_in.wait_event(self.ev_cmp[b])        # chunk c-2 no longer reads this slot
                self.Yd[b][:n].copy_(Yh[lo:hi], non_blocking=True)
                self.ev_in[b].record(self.s_in)
            with torch.cuda.stream(self.s_cmp):
                self.s_cmp.wait_event(self.ev_in[b])
                if c >= 2 and self.out is not None:
                    self.s_cmp.wait_event(self.ev_out[b])       # chunk c-2 has left this slot
                self.plans[c].run()
                if self.out is not None and self.Od is not self.Wd:
                    self.Od[b][:n].copy_(self.Wd[b][:n])
                self.ev_cmp[b].record(self.s_cmp)
            if self.out is not None:
                with torch.cuda.stream(self.s_out):
                    self.s_out.wait_event(self.ev_cmp[b])
                    self.out[lo:hi].copy_(self.Od[b][:n], non_blocking=True)
                    self.ev_out[b].record(self.s_out)
        for s in (self.s_in, self.s_cmp, self.s_out):
            cur.wait_stream(s)
        if sync:
            cur.synchronize()
        return self.out if self.out is not None else self.W


def fista_outputs(W, hrf):
    """``z = cumsum(w)`` and ``x = hrf * z`` (pybold/bold_signal.py:74-75), float64."""
    lib = _lib.load()
    W = _rows(W, torch.float64, "W")
    dev = W.device
    P, N = W.shape
    taps_dev = torch.from_numpy(_as_taps(hrf)).to(dev)
    Z = torch.empty_like(W)
    X = torch.empty_like(W)
    with torch.cuda.device(dev):
        rc = lib.pb_fista_outputs(W.data_ptr(), _ld(W), P, N, taps_dev.data_ptr(),
                                  taps_dev.numel(), Z.data_ptr(), _ld(Z),
                                  X.data_ptr(), _ld(X), _stream_ptr(dev))
    _lib.check(rc, "pb_fista_outputs")
    return X, Z


def fista_outputs_into(W, taps_dev, Z, X):
    """:func:`fista_outputs` into caller-owned buffers, taps already on the device: one launch, nothing allocated (the
    form a timed loop wants)."""
    lib = _lib.load()
    P, N = W.shape
    with torch.cuda.device(W.device):
        rc = lib.pb_fista_outputs(W.data_ptr(), _ld(W), P, N, taps_dev.data_ptr(), taps_dev.numel(), Z.data_ptr(), _ld(Z),
                                  X.data_ptr(), _ld(X), _stream_ptr(W.device))
    _lib.check(rc, "pb_fista_outputs")


def fista_stats(W, Y, hrf, y_rep=1):
    """Per-problem ``||hrf * cumsum(w) - y||^2`` and ``||w||_1`` (float64 ``(P,)``
    each): the R / G terms of pybold/bold_signal.py:141-157."""
    lib = _lib.load()
    W = _rows(W, torch.float64, "W")
    Y, fn = _y_rows(Y, lib.pb_fista_stats, lib.pb_fista_stats_d)
    dev = W.device
    P, N = W.shape
    taps_dev = torch.from_numpy(_as_taps(hrf)).to(dev)
    r2 = torch.empty((P,), dtype=torch.float64, device=dev)
    l1 = torch.empty((P,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = fn(W.data_ptr(), _ld(W), Y.data_ptr(), _ld(Y), int(y_rep), P, N,
                                taps_dev.data_ptr(), taps_dev.numel(), r2.data_ptr(),
                                l1.data_ptr(), _stream_ptr(dev))
    _lib.check(rc, "pb_fista_stats")
    return r2, l1


def spectral_radius(x0, hrf, nb_iter=30, tol=1.0e-6):
    """Power iteration of pybold/utils.py:94-109 for ``H = toeplitz(hrf) . cumsum``
    from the start vector ``x0`` (1-D float64 array), in one kernel launch.
    Returns ``(rho, iterations done)``."""
    lib = _lib.load()
    dev = device()
    x = torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float64).ravel()).to(dev)
    t = torch.from_numpy(_as_taps(hrf)).to(dev)
    out = torch.empty((2,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.pb_spectral_radius(x.data_ptr(), x.numel(), t.data_ptr(), t.numel(), int(nb_iter),
                                    float(tol), out.data_ptr(), _stream_ptr(dev))
    _lib.check(rc, "pb_spectral_radius")
    rho, n_it = out.cpu().numpy()
    return float(rho), int(n_it)


def spectral_radius_batch(X0, taps, nb_iter=30, tol=1.0e-6):
    """:func:`spectral_radius` for one HRF per row in one launch (``pb_spectral_radius_pp``): ``X0`` float64 ``(V, N)``
    start vectors, ``taps`` float64 ``(V, K)`` (arrays or CUDA tensors; padded row strides are kept).  Row ``v`` gets
    the bits ``spectral_radius(X0[v], taps[v])`` gives.  Returns ``(rho (V,) float64, n_it (V,) int)`` as NumPy arrays."""
    lib = _lib.load()
    dev = device(X0.device if torch.is_tensor(X0) and X0.is_cuda else None)
    X = _rows(torch.as_tensor(X0, dtype=torch.float64).to(dev), torch.float64, "X0")
    T = _rows(torch.as_tensor(taps, dtype=torch.float64).to(dev), torch.float64, "taps")
    V, N = X.shape
    if T.shape[0] != V:
        raise ValueError("taps must have one row per row of X0: %s against %s" % (tuple(T.shape), tuple(X.shape)))
    out = torch.empty((V, 2), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.pb_spectral_radius_pp(X.data_ptr(), _ld(X), V, N, T.data_ptr(), _ld(T), T.shape[1], int(nb_iter),
                                       float(tol), out.data_ptr(), _stream_ptr(dev))
    _lib.check(rc, "pb_spectral_radius_pp")
    o = out.cpu().numpy()
    return o[:, 0].copy(), o[:, 1].astype(np.int64)


def _apply(fn_name, X, n_out, taps=None, n_in=None):
    lib = _lib.load()
    X = _rows(X, torch.float64, "x")
    dev = X.device
    V, n_src = X.shape
    out = torch.empty((V, n_out), dtype=torch.float64, device=dev)
    fn = getattr(lib, fn_name)
    with torch.cuda.device(dev):
        if taps is None:
            rc = fn(X.data_ptr(), _ld(X), out.data_ptr(), _ld(out), V, n_src,
                    _stream_ptr(dev))
        else:
            t = torch.from_numpy(_as_taps(taps)).to(dev)
            if fn_name in ("pb_conv", "pb_op_forward"):
                dim_in, dim_out = n_src, n_out
            else:                       # adjoint forms: input lives in the range
                dim_in, dim_out = n_out, n_src
            rc = fn(X.data_ptr(), _ld(X), out.data_ptr(), _ld(out), V, dim_in,
                    dim_out, t.data_ptr(), t.numel(), _stream_ptr(dev))
    _lib.check(rc, fn_name)
    return out


def integ_op(X):
    """Row-wise cumulative sum (DiscretInteg.op, pybold/linear.py:15-28)."""
    return _apply("pb_integ_op", X, X.shape[1])


def integ_adj(X):
    """Row-wise reverse cumulative sum (DiscretInteg.adj, pybold/linear.py:30-43)."""
    return _apply("pb_integ_adj", X, X.shape[1])


def conv(X, taps, dim_out=None):
    """``toeplitz_from_kernel(taps, n_in, dim_out) @ x`` per row (convolution.py:105-132)."""
    return _apply("pb_conv", X, X.shape[1] if dim_out is None else dim_out, taps)


def corr(R, taps, dim_in=None):
    """``toeplitz_from_kernel(taps, dim_in, n_out).T @ r`` per row."""
    return _apply("pb_corr", R, R.shape[1] if dim_in is None else dim_in, taps)


def spectral(X, index_map, pad_left, filt, corr=False):
    """Length-L circular convolution (``corr=False``) or correlation of each row padded
    through ``index_map`` (int32 [L], -1 = zero), read at ``[pad_left, pad_left + N)``:
    the product of the reference's padded-FFT functions (convolution.py:9-102) with the
    filter ``filt`` prepared by the caller (include/pybold_hip.h, pb_spectral_conv)."""
    lib = _lib.load()
    X = _rows(X, torch.float64, "x")
    dev = X.device
    V, N = X.shape
    m = torch.from_numpy(np.ascontiguousarray(index_map, dtype=np.int32).ravel()).to(dev)
    c = torch.from_numpy(np.ascontiguousarray(filt, dtype=np.float64).ravel()).to(dev)
    out = torch.empty((V, N), dtype=torch.float64, device=dev)
    name = "pb_spectral_corr" if corr else "pb_spectral_conv"
    with torch.cuda.device(dev):
        rc = getattr(lib, name)(X.data_ptr(), _ld(X), out.data_ptr(), _ld(out), V, N, m.data_ptr(), m.numel(),
                                int(pad_left), c.data_ptr(), c.numel(), _stream_ptr(dev))
    _lib.check(rc, name)
    return out


def op_forward(X, taps, dim_out=None):
    """``ConvAndLinear(DiscretInteg(), taps, n_in, dim_out).op`` (linear.py:73-93)."""
    return _apply("pb_op_forward", X, X.shape[1] if dim_out is None else dim_out, taps)


def op_adjoint(R, taps, dim_in=None):
    """``ConvAndLinear(DiscretInteg(), taps, dim_in, n_out).adj`` (linear.py:95-113)."""
    return _apply("pb_op_adjoint", R, R.shape[1] if dim_in is None else dim_in, taps)


def hrf_cost(Z, Y, taps):
    """``0.5 ||y_v - taps_c * z_v||^2`` for every voxel v and candidate HRF c
    (hrf_fit_err, pybold/bold_signal.py:217-222).  ``taps`` is ``(K,)`` or
    ``(C, K)``; returns float64 ``(C, V)``."""
    lib = _lib.load()
    Z = _rows(Z, torch.float64, "Z")
    Y, fn = _y_rows(Y, lib.pb_hrf_cost, lib.pb_hrf_cost_d)
    dev = Z.device
    V, N = Z.shape
    if torch.is_tensor(taps):
        t_dev = taps.to(device=dev, dtype=torch.float64).reshape(-1, taps.shape[-1]).contiguous()
        C, K = t_dev.shape
    else:
        t = np.atleast_2d(np.asarray(taps, dtype=np.float64))
        C, K = t.shape
        t_dev = torch.from_numpy(np.ascontiguousarray(t)).to(dev)
    cost = torch.empty((C, V), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = fn(Z.data_ptr(), _ld(Z), Y.data_ptr(), _ld(Y), V, N,
                             t_dev.data_ptr(), K, C, cost.data_ptr(), _stream_ptr(dev))
    _lib.check(rc, "pb_hrf_cost")
    return cost


# ---- per-voxel HRFs (batched blind deconvolution) ---------------------------
def fista_solve_pp(Y, taps, steps, lbda, n_iter, W0=None, stop=None, tol=0.0, force=None,
                   inplace=False, guard_work=None, guard=False):
    """:func:`fista_solve` with one HRF and one step per problem: ``taps`` float64
    CUDA ``(V, K)``, ``steps`` float64 CUDA ``(V,)`` -- or ONE HRF ``(K,)`` and ONE
    step ``(1,)`` living in device memory and shared by every problem (the shared-HRF
    blind step: taps come straight from :func:`theta_fit`).  ``inplace=True`` iterates
    in ``W0`` itself instead of a copy.  ``guard=True`` (opt-in): the conditioning guard
    of ``pb_fista_solve_pp_guarded`` -- rows the operator barely sees are solved again in
    float64 (or, off the matrix pipe, on a float32 vector form), every other row keeps
    the bits of the plain call; ``guard_work``: an int32 CUDA buffer of
    :func:`guard_work_len` words to reuse, read afterwards by :func:`guard_counts`.
    Returns ``(W, n_done)``."""
    lib = _lib.load()
    Y = _rows(Y, torch.float32, "Y")
    dev = Y.device
    V, N = Y.shape
    shared = taps.dim() == 1          # ONE HRF / step in device memory for every problem
    if shared:
        if taps.dtype != torch.float64 or not taps.is_cuda:
            raise TypeError("taps must be a float64 CUDA tensor")
        taps = taps.contiguous().reshape(1, -1)
    else:
        taps = _rows(taps, torch.float64, "taps")
        if taps.shape[0] != V:
            raise ValueError("taps must have one row per voxel")
    steps = steps.to(device=dev, dtype=torch.float64).contiguous().ravel()
    if steps.numel() != (1 if shared else V):
        raise ValueError("steps must have one entry per voxel (one in all for a shared HRF)")
    W, cold = _warm_start(W0, (V, N), dev, inplace)
    lbda_scalar, lbda_dev = _lbda_arg(lbda, dev)
    betas = _betas_on(dev, n_iter)
    n_done = torch.empty((V,), dtype=torch.int32, device=dev)
    if guard:
        guard_work = _guard_work(guard_work, V, N, cold, dev)
        with torch.cuda.device(dev):
            rc = lib.pb_fista_solve_pp_guarded(
                Y.data_ptr(), _ld(Y), W.data_ptr(), _ld(W), V, N, taps.data_ptr(),
                0 if shared else _ld(taps), taps.shape[1], steps.data_ptr(), lbda_scalar,
                lbda_dev.data_ptr() if lbda_dev is not None else None, betas.data_ptr(), int(n_iter),
                _STOP[stop], float(tol), n_done.data_ptr(), guard_work.data_ptr(), guard_work.numel(),
                _FORCE[force] | cold, _stream_ptr(dev))
        _lib.check(rc, "pb_fista_solve_pp_guarded")
        return W, n_done
    with torch.cuda.device(dev):
        rc = lib.pb_fista_solve_pp(
            Y.data_ptr(), _ld(Y), W.data_ptr(), _ld(W), V, N, taps.data_ptr(),
            0 if shared else _ld(taps), taps.shape[1], steps.data_ptr(), lbda_scalar,
            lbda_dev.data_ptr() if lbda_dev is not None else None, betas.data_ptr(), int(n_iter),
            _STOP[stop], float(tol), n_done.data_ptr(), _FORCE[force] | cold, _stream_ptr(dev))
    _lib.check(rc, "pb_fista_solve_pp")
    return W, n_done


# ---- the conditioning guard of the solves whose HRF lives in device memory (opt-in; csrc/guard.h) ---------------------
def guard_work_len(n_rows, n_scans, cold=False):
    """int32 words of the work buffer of a guarded solve (``pb_fista_guard_work_len``); smaller for a cold start."""
    return int(_lib.load().pb_fista_guard_work_len(int(n_rows), int(n_scans), PB_FLAG_COLD_START if cold else 0))


def pp_guard_opt_in(guard=None):
    """The switch of the blind-deconvolution loops (``bd`` on a 2-D batch, ``bd_shared``, ``bd_parcels``): ``guard`` as
    given, ``None``: the environment variable ``PYBOLD_AMD_PP_GUARD`` (``"1"`` is on; the convention of
    ``PYBOLD_AMD_PARCELS_SPLIT``).  Read when a loop starts."""
    if guard is None:
        return os.environ.get("PYBOLD_AMD_PP_GUARD", "0") == "1"
    return bool(guard)


def guard_work_buffer(n_rows, n_scans, dev, cold=False):
    """A zeroed work buffer for guarded solves of this shape on ``dev`` (zeroed: :func:`guard_counts` reads 0 from it
    before the first call and after calls on an empty batch, which launch nothing)."""
    return torch.zeros((max(guard_work_len(n_rows, n_scans, cold), 8),), dtype=torch.int32, device=dev)


def _guard_work(work, V, N, cold, dev):
    need = guard_work_len(V, N, cold != 0)
    if work is None or work.dtype != torch.int32 or work.numel() < need or work.device != dev:
        work = torch.zeros((max(need, 8),), dtype=torch.int32, device=dev)      # (an empty batch launches nothing: counts 0)
    return work


def guard_counts(guard_work):
    """``{'float64': n, 'vector': n}``: the rows the last guarded solve that used this work buffer solved again in
    float64 / on the float32 vector form.  Reads two words from the device (synchronises)."""
    head = guard_work[:4].cpu()
    return {"float64": int(head[1]), "vector": int(head[3])}


def guard_supported(n_scans, n_taps, stop=None):
    """The float64 kernel a guarded solve of this shape re-solves ill-conditioned rows on (``pb_fista_guard_supported``):
    1 one wave per row, 2 four waves, 3 / 4 the same for HRFs of 33 .. 48 taps, 5 the LDS kernel; 0: no guard for the
    shape (more than 64 taps or 1 344 scans) -- a guarded call then runs the plain solve and marks nothing."""
    return int(_lib.load().pb_fista_guard_supported(int(n_scans), int(n_taps), _STOP[stop]))


def pp_uses_matrix_pipe(n_scans, n_taps, n_rows, shared=True, stop=None, force=None):
    """Whether :func:`fista_solve_pp` puts rows of such a call on a matrix-pipe form (``pb_fista_pp_has_matrix_pipe``,
    host-only): the calls whose guard also lists the rows to keep off the matrix pipe."""
    return bool(_lib.load().pb_fista_pp_has_matrix_pipe(int(n_scans), int(n_taps), int(n_rows), 1 if shared else 0, _STOP[stop],
                                                        force if isinstance(force, int) else _FORCE[force]))


def conditioning_marks(Y, taps, offsets=None):
    """What the conditioning guard would do with every row of ``Y`` (float32 CUDA ``(V, N)``): int32 ``(V,)`` -- 2 the
    row is solved in float64 (``gamma_2 < 1e-2``), 1 it is kept off the matrix pipe (``gamma_2`` below 7e-2 / 3e-2 / 2e-2
    by shape), 0 it keeps the plain call's answer.  ``gamma_2 = lambda_max / (||y||_2 sum|c| / sqrt(N))``, ``c =
    cumsum(h)``, for the row's own HRF: ``taps`` float64 CUDA ``(K,)`` (one for all rows), ``(V, K)`` (one per row) or,
    with ``offsets`` (``G + 1`` integers or a :class:`ParcelOffsets`), ``(G, K)`` (one per parcel).  Up to 64 taps and
    1 344 scans (``pb_conditioning_marks``)."""
    lib = _lib.load()
    Y = _rows(Y, torch.float32, "Y")
    dev = Y.device
    V, N = Y.shape
    if taps.dtype != torch.float64 or not taps.is_cuda:
        raise TypeError("taps must be a float64 CUDA tensor")
    po = None
    if taps.dim() == 1:
        if offsets is not None:
            raise ValueError("offsets go with one HRF per parcel, taps (G, K)")
        taps, ldt = taps.contiguous().reshape(1, -1), 0
    else:
        taps = _rows(taps, torch.float64, "taps")
        ldt = _ld(taps)
        if offsets is not None:
            po = _parcel_offsets(offsets, dev, V)
        if taps.shape[0] != (po.G if po is not None else V):
            raise ValueError("taps must have one row per %s" % ("parcel" if po is not None else "row of Y"))
    marks = torch.empty((V,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.pb_conditioning_marks(Y.data_ptr(), _ld(Y) if V else N, V, N, taps.data_ptr(), ldt, taps.shape[1],
                                       po.dev.data_ptr() if po is not None else None, po.G if po is not None else 0,
                                       marks.data_ptr(), _stream_ptr(dev))
    _lib.check(rc, "pb_conditioning_marks")
    return marks


def fista_solve_pp_d(Y, taps, steps, lbda, n_iter, W0=None, want_J=False, stop=None, tol=0.0, wind=6, force=None):
    """:func:`fista_solve` on a float64 ``Y`` with one HRF and one step per problem (``pb_fista_solve_pp_d``): float64 end
    to end, the reference's arithmetic, every stop rule, the cost trace, negative lambdas.

    Y      float64 CUDA ``(V, N)``;  taps  float64 CUDA ``(V, K)``;  steps  float64 ``(V,)``
    lbda   scalar or ``(V,)``;  W0  optional float64 CUDA ``(V, N)`` warm start (not modified)
    force  None | "fast" (the register form, one problem per wave: ``N <= 640``, ``K <= 32``, window rule at
           ``wind == 6``) | "generic" (the LDS kernel); :func:`which_kernel_pp_f64` names the dispatch's choice
           | "split" (opt-in, ``PB_FLAG_PP_SPLIT``: one problem per workgroup of four waves, ``641 <= N <= 1280``,
           ``K <= 32``, window rule at ``wind == 6`` -- :func:`pp_split_supported`; any other shape is an error.
           Without it such series run on the LDS kernel)
           | "long_hrf" (opt-in, ``PB_FLAG_LONG_HRF``: one problem per wave, ``N <= 640``, ``K <= 48``, window rule at
           ``wind == 6`` -- :func:`long_hrf_supported`; any other shape is an error.  Without it 33+ taps run on the
           LDS kernel)
           | "split_long_hrf" (opt-in, ``pb_fista_solve_split_long_pp_d``: one problem per workgroup of four waves,
           ``641 <= N <= 1280``, ``K <= 48``, window rule at ``wind == 6`` -- :func:`split_long_hrf_supported`; any
           other shape is an error)
    Returns ``(W float64 (V, N), J float64 (V, n_iter) or None, n_done int32 (V,))``."""
    lib = _lib.load()
    Y = _rows(Y, torch.float64, "Y")
    dev = Y.device
    V, N = Y.shape
    taps = _rows(taps, torch.float64, "taps")
    if taps.shape[0] != V:
        raise ValueError("taps must have one row per voxel: %s against %s" % (tuple(taps.shape), tuple(Y.shape)))
    steps = torch.as_tensor(steps, dtype=torch.float64).to(dev).contiguous().ravel()
    if steps.numel() != V:
        raise ValueError("steps must have one entry per voxel (%d)" % V)
    entry, flags = _f64_solve_route(force, pp=True)
    W, cold = _warm_start(W0, (V, N), dev)
    lbda_scalar, lbda_dev = _lbda_arg(lbda, dev, V)
    betas = _betas_on(dev, n_iter)
    J = torch.full((V, max(n_iter, 1)), float("nan"), dtype=torch.float64, device=dev) if want_J else None
    n_done = torch.empty((V,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = getattr(lib, entry)(
            Y.data_ptr(), _ld(Y), 1, W.data_ptr(), _ld(W), V, N, taps.data_ptr(), _ld(taps), taps.shape[1],
            steps.data_ptr(), lbda_scalar, lbda_dev.data_ptr() if lbda_dev is not None else None,
            betas.data_ptr(), int(n_iter), J.data_ptr() if J is not None else None, _ld(J) if J is not None else 0,
            _STOP[stop], float(tol), int(wind), n_done.data_ptr(), flags | cold, _stream_ptr(dev))
    _lib.check(rc, entry)
    return W, J, n_done


def fista_stats_pp(W, Y, taps):
    """:func:`fista_stats` with one HRF per row (float64 ``Y``; ``taps`` float64 CUDA ``(V, K)``): the residual comes
    from :func:`fista_outputs_pp`, the two sums from ``torch`` (the host engine of the per-voxel lambda search; the
    device engine forms them in its kernel)."""
    X, _ = fista_outputs_pp(W, taps)
    return ((X - Y) ** 2).sum(dim=1), W.abs().sum(dim=1)


def fista_outputs_pp(W, taps):
    """``z = cumsum(w)``, ``x = taps_v * z`` with one HRF per row."""
    lib = _lib.load()
    W = _rows(W, torch.float64, "W")
    taps = _rows(taps, torch.float64, "taps")
    dev = W.device
    P, N = W.shape
    Z = torch.empty_like(W)
    X = torch.empty_like(W)
    with torch.cuda.device(dev):
        rc = lib.pb_fista_outputs_pp(W.data_ptr(), _ld(W), P, N, taps.data_ptr(), _ld(taps),
                                     taps.shape[1], Z.data_ptr(), _ld(Z), X.data_ptr(), _ld(X),
                                     _stream_ptr(dev))
    _lib.check(rc, "pb_fista_outputs_pp")
    return X, Z


def hrf_cost_pv(Z, Y, taps):
    """``0.5 ||y_v - taps[c, v] * z_v||^2``: ``taps`` float64 CUDA ``(C, V, K)`` ->
    float64 ``(C, V)``."""
    lib = _lib.load()
    Z = _rows(Z, torch.float64, "Z")
    Y, fn = _y_rows(Y, lib.pb_hrf_cost_pv, lib.pb_hrf_cost_pv_d)
    dev = Z.device
    V, N = Z.shape
    if taps.dim() != 3 or taps.shape[1] != V or taps.dtype != torch.float64:
        raise ValueError("taps must be float64 (C, V, K)")
    taps = taps.contiguous()
    C, _, K = taps.shape
    cost = torch.empty((C, V), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = fn(Z.data_ptr(), _ld(Z), Y.data_ptr(), _ld(Y), V, N, taps.data_ptr(),
                                K, C, cost.data_ptr(), _stream_ptr(dev))
    _lib.check(rc, "pb_hrf_cost_pv")
    return cost


def gram_frobenius_batch(taps, n):
    """``||A^T A||_F`` per row of ``taps`` (float64 CUDA ``(P, K)``), ``A =
    toeplitz(taps_p, n, n) tril(1)`` (pybold/bold_signal.py:249-253)."""
    lib = _lib.load()
    taps = _rows(taps, torch.float64, "taps")
    dev = taps.device
    P, K = taps.shape
    out = torch.empty((P,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.pb_gram_frobenius(taps.data_ptr(), _ld(taps), P, K, int(n), out.data_ptr(),
                                   _stream_ptr(dev))
    _lib.check(rc, "pb_gram_frobenius")
    return out


def spm_hrf_batch(deltas, t_r, dur, dt=0.001, p_delay=6, undershoot=16.0, p_disp=1.0, u_disp=1.0,
                  p_u_ratio=0.167):
    """Un-normalised SPM HRFs for a CUDA vector of dilations (any shape), sampled
    like ``spm_hrf(delta, t_r, dur, normalized_hrf=False)`` (pybold/hrf_model.py:12-39).
    Returns float64 CUDA ``deltas.shape + (K,)``."""
    lib = _lib.load()
    dev = deltas.device
    d = deltas.to(torch.float64).contiguous()
    t_dev = _sample_times_on(dev, t_r, dur, dt)
    M, K = d.numel(), t_dev.numel()
    out = torch.empty((M, K), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.pb_spm_hrf(d.data_ptr(), M, t_dev.data_ptr(), K, p_delay / p_disp, dt / p_disp,
                            undershoot / u_disp, dt / u_disp, p_u_ratio, out.data_ptr(),
                            _stream_ptr(dev))
    _lib.check(rc, "pb_spm_hrf")
    return out.reshape(tuple(deltas.shape) + (K,))


# ---- regularisation path, post-processing, theta-step on the device ------------
def lambda_max(Y, hrf):
    """``|| H^T y_v ||_inf`` per voxel (float64 ``(V,)``), ``H = toeplitz(hrf) . cumsum``:
    the smallest ``lbda`` whose ``deconv`` solution is ``diff_z = 0``; a
    regularisation path is ``lbda = c * lambda_max`` with ``c`` in ``(0, 1]``."""
    lib = _lib.load()
    Y, fn = _y_rows(Y, lib.pb_lambda_max, lib.pb_lambda_max_d)
    dev = Y.device
    V, N = Y.shape
    taps_dev = torch.from_numpy(_as_taps(hrf)).to(dev)
    out = torch.empty((V,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = fn(Y.data_ptr(), _ld(Y), V, N, taps_dev.data_ptr(), taps_dev.numel(), out.data_ptr(),
                _stream_ptr(dev))
    _lib.check(rc, "pb_lambda_max")
    return out


MAD_DAUB_NMAX = 8192         # pb_mad_daub_noise_est: longest row (include/pybold_hip.h)


def mad_daub_noise_est(Y, c=0.6744):
    """Noise level of every row of a float32 or float64 CUDA ``(V, N)`` tensor (float64 ``(V,)``): the MAD of the
    level-1 db3 detail band / ``c`` (pybold/utils.py:10-25), the operations of ``utils.mad_daub_noise_est`` in the
    same order on the device.  ``5 <= N <= 8192``; the library refuses other lengths (``PyboldHipError``)."""
    lib = _lib.load()
    Y, fn = _y_rows(Y, lib.pb_mad_daub_noise_est, lib.pb_mad_daub_noise_est_d)
    dev = Y.device
    V, N = Y.shape
    out = torch.empty((V,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = fn(Y.data_ptr(), _ld(Y), V, N, float(c), out.data_ptr(), _stream_ptr(dev))
    _lib.check(rc, "pb_mad_daub_noise_est")
    return out


def _auto_lbda_solve(entry, pp, Y, hrf, step, sigma, early_stopping, tol, wind, nb_iter, nb_sub_iter, outer_chunk, W0, want_trace):
    """The one body of the eight searches: ``entry`` of a row of ``F64_FORMS``; ``pp``: ``hrf`` is CUDA ``(V, K)``, ``step`` ``(V,)``."""
    if pp:
        Y = _rows(Y, torch.float64, "Y")
        hrf = _rows(hrf, torch.float64, "taps")
        if hrf.shape[0] != Y.shape[0]:
            raise ValueError("taps must have one row per voxel: %s against %s" % (tuple(hrf.shape), tuple(Y.shape)))
        step = torch.as_tensor(step, dtype=torch.float64).to(Y.device).contiguous().ravel()
        if step.numel() != Y.shape[0]:
            raise ValueError("steps must have one entry per voxel (%d)" % Y.shape[0])
    lib = _lib.load()
    Y = _rows(Y, torch.float64, "Y")
    dev = Y.device
    V, N = Y.shape
    taps = None if pp else _as_taps(hrf)
    nb_iter, nb_sub_iter = int(nb_iter), int(nb_sub_iter)
    W, _ = _warm_start(W0, (V, N), dev)               # (a cold start is an argument of the searches, not a flag)
    if torch.is_tensor(sigma):
        sig = sigma.to(device=dev, dtype=torch.float64).reshape(-1)
    else:
        sig = torch.from_numpy(np.ascontiguousarray(np.atleast_1d(np.asarray(sigma, dtype=np.float64)).ravel())).to(dev)
    if sig.numel() == 1 and V != 1:
        sig = sig.expand(V)
    sig = sig.contiguous()
    if sig.numel() != V:
        raise ValueError("sigma must have one entry per row of Y (%d)" % V)
    betas = _betas_on(dev, nb_sub_iter)
    trace = [torch.full((V, max(nb_iter, 1)), float("nan"), dtype=torch.float64, device=dev) if want_trace else None
             for _ in range(3)]
    alpha = torch.empty((V,), dtype=torch.float64, device=dev)
    lbda = torch.empty((V,), dtype=torch.float64, device=dev)
    n_outer = torch.empty((V,), dtype=torch.int32, device=dev)
    n_inner = torch.empty((V,), dtype=torch.int64, device=dev)
    work = torch.empty((int(lib.pb_auto_lbda_work_len(V)),), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = getattr(lib, entry)(
            Y.data_ptr(), _ld(Y), W.data_ptr(), _ld(W), int(W0 is None), V, N,
            *((hrf.data_ptr(), _ld(hrf), hrf.shape[1], step.data_ptr()) if pp else (taps.ctypes.data, taps.size, float(step))),
            betas.data_ptr(), sig.data_ptr(),
            int(bool(early_stopping)), float(tol), int(wind), nb_iter, nb_sub_iter, int(outer_chunk),
            trace[0].data_ptr() if want_trace else None, trace[1].data_ptr() if want_trace else None,
            trace[2].data_ptr() if want_trace else None, _ld(trace[0]) if want_trace else 0,
            alpha.data_ptr(), lbda.data_ptr(), n_outer.data_ptr(), n_inner.data_ptr(),
            work.data_ptr(), work.numel(), _stream_ptr(dev))
    _lib.check(rc, entry)
    return W, {"alpha": alpha, "lbda": lbda, "n_outer": n_outer, "n_inner": n_inner,
               "R": trace[0], "G": trace[1], "J": trace[2]}


def _bind_search(entry, pp):
    if pp:
        def search(Y, taps, steps, sigma, early_stopping=True, tol=1.0e-6, wind=6, nb_iter=1000, nb_sub_iter=1000,
                   outer_chunk=0, W0=None, want_trace=True):
            return _auto_lbda_solve(entry, True, Y, taps, steps, sigma, early_stopping, tol, wind, nb_iter, nb_sub_iter,
                                    outer_chunk, W0, want_trace)
    else:
        def search(Y, hrf, step, sigma, early_stopping=True, tol=1.0e-6, wind=6, nb_iter=1000, nb_sub_iter=1000,
                   outer_chunk=0, W0=None, want_trace=True):
            return _auto_lbda_solve(entry, False, Y, hrf, step, sigma, early_stopping, tol, wind, nb_iter, nb_sub_iter,
                                    outer_chunk, W0, want_trace)
    return search


def _bind_query(query, with_stop):
    if with_stop:                                       # a solve's query: the stop rule decides too
        def supported(n_scans, n_taps, stop=None, wind=6):
            return bool(getattr(_lib.load(), query)(int(n_scans), int(n_taps), _STOP[stop], int(wind)))
    else:
        def supported(n_scans, n_taps, wind=6):
            return bool(getattr(_lib.load(), query)(int(n_scans), int(n_taps), int(wind)))
    return supported


# What each public name of the family says of itself; the functions are bound below, one per name of a row's `public`.
_F64_DOCS = {
    "auto_lbda_solve":
    """The noise-driven lambda search of ``deconv(lbda=None)`` (pybold/bold_signal.py:99-214) for every row of ``Y``
    as one device-resident solve (``pb_auto_lbda_d``: one voxel per wave, no host round trip, no synchronisation).

    Y      float64 CUDA ``(V, N)``, ``N <= 640``;  hrf  1-D array of ``K <= 32`` taps (host);  step  ``1 / L``
    sigma  float64 ``(V,)`` noise levels (CUDA tensor, array or scalar)
    W0     optional float64 CUDA ``(V, N)`` warm start (not modified)
    outer_chunk  outer iterations per launch (0: the library's choice); changes no bit of the result
    Returns ``(W, info)``: the final iterate and a dict of CUDA tensors ``alpha``, ``lbda`` (float64 ``(V,)``),
    ``n_outer`` (int32), ``n_inner`` (int64, inner iterations summed) and, with ``want_trace``, ``R``, ``G``, ``J``
    (float64 ``(V, nb_iter)``, NaN from a voxel's ``n_outer`` on).""",
    "auto_lbda_solve_split":
    """:func:`auto_lbda_solve` for series of ``641 <= N <= 1280`` scans (``pb_auto_lbda_split_d``: one voxel per
    workgroup of four waves): the same arguments, the same return value.""",
    "auto_lbda_solve_long":
    """:func:`auto_lbda_solve` for HRFs of up to 48 taps (``pb_auto_lbda_long_d``: one voxel per wave, the taps in one
    VGPR pair; :func:`auto_lbda_long_supported`): the same arguments, the same return value; with ``K <= 32`` the same
    bits.  Opt-in: :func:`auto_lbda_solve` keeps its limit of 32 taps.""",
    "auto_lbda_solve_split_long":
    """:func:`auto_lbda_solve_split` for HRFs of up to 48 taps (``pb_auto_lbda_split_long_d``: one voxel per workgroup of
    four waves, the taps in one VGPR pair of every wave; :func:`auto_lbda_split_long_supported`): the same arguments, the
    same return value; with ``K <= 32`` the same bits.  Opt-in: :func:`auto_lbda_solve_split` keeps its limit of 32 taps.""",
    "auto_lbda_solve_pp":
    """:func:`auto_lbda_solve` with one HRF and one step per voxel (``pb_auto_lbda_pp_d``): ``taps`` float64 CUDA
    ``(V, K)``, ``steps`` float64 ``(V,)``; the same limits (:func:`auto_lbda_supported`), the same return value.""",
    "auto_lbda_solve_split_pp":
    """:func:`auto_lbda_solve_pp` for series of ``641 <= N <= 1280`` scans (``pb_auto_lbda_split_pp_d``: one voxel per
    workgroup of four waves; :func:`auto_lbda_split_supported` answers for its shapes): the same arguments, the same
    return value.  Opt-in: :func:`auto_lbda_solve_pp` keeps its limit of 640 scans.""",
    "auto_lbda_solve_long_pp":
    """:func:`auto_lbda_solve_pp` for HRFs of up to 48 taps (``pb_auto_lbda_long_pp_d``;
    :func:`auto_lbda_long_supported` answers for its shapes): the same arguments, the same return value.  Opt-in:
    :func:`auto_lbda_solve_pp` keeps its limit of 32 taps.""",
    "auto_lbda_solve_split_long_pp":
    """:func:`auto_lbda_solve_split_pp` for HRFs of up to 48 taps (``pb_auto_lbda_split_long_pp_d``;
    :func:`auto_lbda_split_long_supported` answers for its shapes): the same arguments, the same return value.  Opt-in:
    :func:`auto_lbda_solve_split_pp` keeps its limit of 32 taps.""",
    "pp_split_supported":
    """Whether :func:`fista_solve_pp_d` with ``force="split"`` carries this shape (``pb_fista_pp_split_supported``:
    ``641 <= N <= 1280``, ``K <= 32``, the window rule at ``wind == 6``).""",
    "long_hrf_supported":
    """Whether :func:`fista_solve` (float64 ``Y``) and :func:`fista_solve_pp_d` with ``force="long_hrf"`` carry this
    shape (``pb_fista_long_hrf_supported``: ``N <= 640``, ``K <= 48``, the window rule at ``wind == 6``).""",
    "split_long_hrf_supported":
    """Whether :func:`fista_solve` (float64 ``Y``) and :func:`fista_solve_pp_d` with ``force="split_long_hrf"`` carry this
    shape (``pb_fista_split_long_hrf_supported``: ``641 <= N <= 1280``, ``K <= 48``, the window rule at ``wind == 6``).""",
    "auto_lbda_supported":
    """Whether :func:`auto_lbda_solve` and :func:`auto_lbda_solve_pp` carry this shape (``pb_auto_lbda_supported``:
    ``N <= 640``, ``K <= 32``, ``wind == 6``).""",
    "auto_lbda_split_supported":
    """Whether :func:`auto_lbda_solve_split` and :func:`auto_lbda_solve_split_pp` carry this shape
    (``pb_auto_lbda_split_supported``: ``641 <= N <= 1280``, ``K <= 32``, ``wind == 6``).""",
    "auto_lbda_long_supported":
    """Whether :func:`auto_lbda_solve_long` and :func:`auto_lbda_solve_long_pp` carry this shape
    (``pb_auto_lbda_long_supported``: ``N <= 640``, ``K <= 48``, ``wind == 6``).""",
    "auto_lbda_split_long_supported":
    """Whether :func:`auto_lbda_solve_split_long` and :func:`auto_lbda_solve_split_long_pp` carry this shape
    (``pb_auto_lbda_split_long_supported``: ``641 <= N <= 1280``, ``K <= 48``, ``wind == 6``)."""}

for _form in F64_FORMS.values():
    for _name, _fn in zip(_form.public, (_bind_search(_form.search, False), _bind_search(_form.search_pp, True),
                                         _form.solve_query and _bind_query(_form.solve_query, True),
                                         _bind_query(_form.search_query, False))):
        if _name:
            _fn.__name__ = _fn.__qualname__ = _name
            _fn.__doc__ = _F64_DOCS[_name]
            globals()[_name] = _fn


def inf_norm_rows(X):
    """``x / (max|x| + 1e-12)`` for every row of a float64 CUDA ``(V, n)`` tensor
    (pybold/utils.py:112-115 applied row-wise)."""
    lib = _lib.load()
    X = _rows(X, torch.float64, "x")
    dev = X.device
    V, n = X.shape
    out = torch.empty_like(X)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        rc = lib.pb_inf_norm(X.data_ptr(), _ld(X), out.data_ptr(), _ld(out), V, n, _stream_ptr(dev))
    _lib.check(rc, "pb_inf_norm")
    return out


def hrf_normal_eq(Z, Y, n_taps, per_voxel=False, work=None):
    """One pass over ``(Z, Y)`` -> the normal equations of ``hrf_fit_err``
    (pybold/bold_signal.py:217-222) in the ``K`` taps: ``G (K, K)``, ``b (K,)``, ``yy``
    packed as ``K*K + K + 1`` float64 -- summed over voxels (``per_voxel=False``, shape
    ``(len,)``; zeros for an empty shard) or one set per voxel (``(V, len)``)."""
    lib = _lib.load()
    Z = _rows(Z, torch.float64, "Z")
    Y, fn = _y_rows(Y, lib.pb_hrf_normal_eq, lib.pb_hrf_normal_eq_d)
    dev = Z.device
    V, N = Z.shape
    K = int(n_taps)
    ne = int(lib.pb_hrf_normal_eq_len(K))
    if per_voxel:
        out = torch.empty((V, ne), dtype=torch.float64, device=dev)
        work_ptr, work_len = None, 0
    else:
        out = torch.empty((ne,), dtype=torch.float64, device=dev)
        if work is None or work.numel() < ne:
            work = torch.empty((2048 * ne,), dtype=torch.float64, device=dev)
        work_ptr, work_len = work.data_ptr(), work.numel()
    with torch.cuda.device(dev):
        rc = fn(Z.data_ptr(), _ld(Z) if V else N, Y.data_ptr(), _ld(Y) if V else N, V, N, K,
                int(bool(per_voxel)), work_ptr, work_len, out.data_ptr(), _stream_ptr(dev))
    _lib.check(rc, "pb_hrf_normal_eq")
    return out


def hrf_sample_times(t_r, dur, dt=0.001):
    """Sample times of ``spm_hrf(., t_r, dur)`` (pybold/hrf_model.py:25: the fine
    ``linspace`` grid includes its end point, then decimation by ``int(t_r / dt)``)."""
    return np.ascontiguousarray(np.linspace(0, dur, int(float(dur) / dt))[::int(t_r / dt)])


_times_cache = {}


def _sample_times_on(dev, t_r, dur, dt=0.001):
    """The HRF sample times as a device tensor, uploaded once per (device, t_r, dur): a
    pageable host-to-device copy would otherwise synchronise every call."""
    key = (dev.type, dev.index, float(t_r), float(dur), float(dt))
    t = _times_cache.get(key)
    if t is None:
        t = torch.from_numpy(hrf_sample_times(t_r, dur, dt)).to(dev)
        _times_cache[key] = t
    return t


def theta_fit(ne, t_r, dur, bounds, n_refine=3, dt=0.001, p_delay=6, undershoot=16.0, p_disp=1.0,
              u_disp=1.0, p_u_ratio=0.167):
    """``argmin_theta 0.5 ||y - h(theta) * z||^2`` over ``bounds = (lo, hi)`` from normal
    equations (:func:`hrf_normal_eq`), entirely on the device: ``ne`` is ``(len,)`` (one
    shared set) or ``(M, len)``.  Returns ``(theta (M,), cost (M,), taps (M, K))`` float64
    CUDA tensors; nothing is copied to the host."""
    lib = _lib.load()
    one = ne.dim() == 1
    ne2 = _rows(ne.reshape(1, -1) if one else ne, torch.float64, "ne")
    dev = ne2.device
    t_dev = _sample_times_on(dev, t_r, dur, dt)
    K = t_dev.numel()
    if ne2.shape[1] != int(lib.pb_hrf_normal_eq_len(K)):
        raise ValueError("normal equations do not match an HRF of %d taps" % K)
    M = ne2.shape[0]
    theta = torch.empty((M,), dtype=torch.float64, device=dev)
    cost = torch.empty((M,), dtype=torch.float64, device=dev)
    taps = torch.empty((M, K), dtype=torch.float64, device=dev)
    lo, hi = float(bounds[0]), float(bounds[1])
    with torch.cuda.device(dev):
        rc = lib.pb_theta_fit(ne2.data_ptr(), _ld(ne2), M, K, t_dev.data_ptr(), p_delay / p_disp,
                              dt / p_disp, undershoot / u_disp, dt / u_disp, p_u_ratio, lo, hi,
                              int(n_refine), theta.data_ptr(), cost.data_ptr(), taps.data_ptr(),
                              _ld(taps), _stream_ptr(dev))
    _lib.check(rc, "pb_theta_fit")
    return theta, cost, taps


# ---- the shared-HRF outer iteration in three launches (z-step, normal equations, theta fit) -------
def hrf_normal_eq_w(W, Y, n_taps, work=None, out=None):
    """:func:`hrf_normal_eq` (summed over voxels) straight from the innovation ``W = diff_z``: the
    cumulative sum (pybold/bold_signal.py:326) and ``sum_v ||w_v||_1`` are taken in the same pass.
    Returns float64 ``(K*K + K + 2,)``: the normal equations followed by the L1 sum -- the message of
    the outer iteration's one all-reduce (``pb_hrf_normal_eq_w``)."""
    lib = _lib.load()
    W = _rows(W, torch.float64, "W")
    Y = _rows(Y, torch.float32, "Y")
    dev = W.device
    V, N = W.shape
    K = int(n_taps)
    ne = int(lib.pb_hrf_normal_eq_len(K)) + 1
    if out is None:
        out = torch.empty((ne,), dtype=torch.float64, device=dev)
    if work is None or work.numel() < ne:
        work = torch.empty((2048 * ne,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.pb_hrf_normal_eq_w(W.data_ptr(), _ld(W) if V else N, Y.data_ptr(), _ld(Y) if V else N, V, N, K,
                                    work.data_ptr(), work.numel(), out.data_ptr(), _stream_ptr(dev))
    _lib.check(rc, "pb_hrf_normal_eq_w")
    return out


def theta_fit_step(msg, t_r, dur, bounds, n_scans, lbda, n_refine=3, dt=0.001, p_delay=6, undershoot=16.0,
                   p_disp=1.0, u_disp=1.0, p_u_ratio=0.167):
    """:func:`theta_fit` on ONE message of :func:`hrf_normal_eq_w` that also leaves on the device what the
    next z-step and the cost trace need: returns ``(theta (1,), cost (1,), taps (K,), step (1,),
    jcost (1,))`` with ``step = 1 / ||A^T A||_F`` for the new HRF on ``n_scans`` scans and ``jcost =
    (2 F(theta*) + lbda ||w||_1) / ||y||^2`` (pybold/bold_signal.py:249-254, :337-342)."""
    lib = _lib.load()
    dev = msg.device
    t_dev = _sample_times_on(dev, t_r, dur, dt)
    K = t_dev.numel()
    if msg.dtype != torch.float64 or msg.numel() != int(lib.pb_hrf_normal_eq_len(K)) + 1 or not msg.is_contiguous():
        raise ValueError("msg must be the contiguous float64 output of hrf_normal_eq_w for %d taps" % K)
    out = torch.empty((4 + K,), dtype=torch.float64, device=dev)
    theta, cost, step, jc, taps = out[0:1], out[1:2], out[2:3], out[3:4], out[4:]
    with torch.cuda.device(dev):
        rc = lib.pb_theta_fit_step(msg.data_ptr(), K, t_dev.data_ptr(), p_delay / p_disp, dt / p_disp,
                                   undershoot / u_disp, dt / u_disp, p_u_ratio, float(bounds[0]), float(bounds[1]),
                                   int(n_refine), int(n_scans), float(lbda), theta.data_ptr(), cost.data_ptr(),
                                   taps.data_ptr(), step.data_ptr(), jc.data_ptr(), _stream_ptr(dev))
    _lib.check(rc, "pb_theta_fit_step")
    return theta, cost, taps, step, jc


# ---- one HRF per parcel: rows contiguous by parcel (pb_fista_solve_grouped, pb_hrf_normal_eq_w_grouped) -------------
class ParcelOffsets:
    """Row ranges of the parcels of a grouped call, once on the host (checked, sizes the launches) and once on the
    device (what the kernels' unit table is built from): parcel ``g`` owns the rows ``offsets[g] .. offsets[g + 1] - 1``,
    ``0 = offsets[0] <= ... <= offsets[G] = V``.  Built once per batch, so that a loop of grouped calls uploads nothing."""

    def __init__(self, offsets, dev):
        host = np.ascontiguousarray(np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets).ravel(), dtype=np.int64)
        if host.size < 1 or host[0] != 0 or np.any(np.diff(host) < 0) or host[-1] >= 2 ** 31:
            raise ValueError("offsets must run 0 = offsets[0] <= offsets[1] <= ... <= offsets[G] = number of rows")
        self.host = host.astype(np.int32)
        self.dev = torch.from_numpy(self.host).to(dev)
        self.G = int(host.size - 1)
        self.rows = int(host[-1])
        self.sizes = np.diff(host)

    def waves(self):
        """Matrix-pipe waves of a grouped solve: ``sum ceil(n_g / 16)``."""
        return int(_lib.load().pb_fista_grouped_waves(self.host.ctypes.data, self.G, self.rows))


def _parcel_offsets(offsets, dev, rows):
    po = offsets if isinstance(offsets, ParcelOffsets) else ParcelOffsets(offsets, dev)
    if po.rows != rows or po.dev.device != dev:
        raise ValueError("offsets end at row %d on %s, the batch has %d rows on %s" % (po.rows, po.dev.device, rows, dev))
    return po


def grouped_wave_table(offsets, per=16):
    """The unit table of a grouped call from the host build of its planner (``pb_fista_grouped_plan``; no GPU):
    ``(table (units, 3) int32 -- first row, rows <= per, parcel --, first (G + 1,) int32 -- first unit of every parcel)``.
    ``per = 16``: the wave table of :func:`fista_solve_grouped`."""
    lib = _lib.load()
    host = np.ascontiguousarray(np.asarray(offsets).ravel(), dtype=np.int32)
    G, rows = host.size - 1, int(host[-1]) if host.size else -1
    n = lib.pb_fista_grouped_plan(host.ctypes.data, G, rows, int(per), None, None) if host.size else -1
    if n < 0:
        raise ValueError("offsets must run 0 = offsets[0] <= offsets[1] <= ... <= offsets[G] = number of rows")
    table = np.full((n, 3), -1, dtype=np.int32)
    first = np.full((G + 1,), -1, dtype=np.int32)
    assert lib.pb_fista_grouped_plan(host.ctypes.data, G, rows, int(per), table.ctypes.data, first.ctypes.data) == n
    return table, first


def grouped_route(offsets, n_scans, n_taps, force=None):
    """What :func:`fista_solve_grouped` decides for these parcels (``offsets``: ``G + 1`` integers or a
    :class:`ParcelOffsets`), series length, HRF length and ``force`` (a name or raw ``PB_FLAG_*`` bits), from the host side
    of the library (``pb_fista_grouped_route``; no launch): ``(code, main_units, row_cut)`` -- ``code`` in the numbering of
    :func:`which_kernel`'s library call: 4 the one-wave matrix-pipe form, 5 two waves per unit of 16 rows, 6 four waves,
    0 every row on the per-problem vector route, -1 the call would raise; ``main_units`` units of the table run in that
    launch, the rows from ``row_cut`` on (the number of rows: none) on the vector forms behind it."""
    import ctypes
    host = offsets.host if isinstance(offsets, ParcelOffsets) else np.ascontiguousarray(np.asarray(offsets).ravel(), dtype=np.int32)
    mu, rc = ctypes.c_int(0), ctypes.c_int(0)
    code = _lib.load().pb_fista_grouped_route(host.ctypes.data, int(host.size - 1), int(host[-1]) if host.size else 0, int(n_scans),
                                              int(n_taps), force if isinstance(force, int) else _FORCE[force], ctypes.byref(mu),
                                              ctypes.byref(rc))
    return int(code), mu.value, rc.value


def fista_solve_grouped(Y, taps, steps, offsets, lbda, n_iter, W0=None, force=None, inplace=False, work=None, guard_work=None,
                        guard=False):
    """:func:`fista_solve_pp` with one HRF and one step per PARCEL: the rows of ``Y`` (float32 CUDA ``(V, N)``) are
    contiguous by parcel, ``offsets`` (``G + 1`` integers or a :class:`ParcelOffsets`) their ranges, ``taps`` float64
    CUDA ``(G, K)``, ``steps`` float64 CUDA ``(G,)``.  129 .. 310 scans with up to 33 taps run on the matrix pipe, a
    wave's 16 problems all of one parcel (calls of 4 096 rows or more; ``force="mfma"`` / ``"mfmaonly"``: whatever the
    number of rows, an error for other shapes), everything else -- and ``force="valu"`` -- on the per-problem vector
    forms with each row's parcel's taps.  Opt-in, ``force="gsplit"`` (``PB_FLAG_GROUPED_SPLIT``): 311 .. 1 280 scans with
    up to 48 taps run on the split matrix-pipe forms too -- two waves per unit of 16 rows up to 640 scans, four beyond; whole
    passes and large remainders there, the rest behind them on the vector forms (:func:`grouped_route` tells) --,
    ``"gsplit_mfma"`` / ``"gsplit_mfmaonly"``: every unit there, whatever the number of rows.  Without the opt-in those
    lengths run on the vector route.  ``force`` may also be raw ``PB_FLAG_*`` bits.  No stop rule.  ``work``: an int32 CUDA buffer of
    ``pb_fista_grouped_work_len(V, G, K)`` words to reuse.  ``guard=True`` (opt-in): the conditioning guard of
    :func:`fista_solve_pp` around this call (``pb_fista_solve_grouped_guarded``), ``guard_work`` its buffer.  Returns
    ``(W, n_done)``."""
    lib = _lib.load()
    Y = _rows(Y, torch.float32, "Y")
    dev = Y.device
    V, N = Y.shape
    taps = _rows(taps, torch.float64, "taps")
    po = _parcel_offsets(offsets, dev, V)
    G, K = taps.shape
    if G != po.G:
        raise ValueError("taps must have one row per parcel (%d), got %d" % (po.G, G))
    steps = steps.to(device=dev, dtype=torch.float64).contiguous().ravel()
    if steps.numel() != G:
        raise ValueError("steps must have one entry per parcel")
    W, cold = _warm_start(W0, (V, N), dev, inplace)
    lbda_scalar, lbda_dev = _lbda_arg(lbda, dev)
    betas = _betas_on(dev, n_iter)
    n_done = torch.empty((V,), dtype=torch.int32, device=dev)
    need = int(lib.pb_fista_grouped_work_len(V, G, K))
    if work is None or work.dtype != torch.int32 or work.numel() < need or work.device != dev:
        work = torch.empty((max(need, 2),), dtype=torch.int32, device=dev)
    if guard:
        guard_work = _guard_work(guard_work, V, N, cold, dev)
        with torch.cuda.device(dev):
            rc = lib.pb_fista_solve_grouped_guarded(
                Y.data_ptr(), _ld(Y) if V else N, W.data_ptr(), _ld(W) if V else N, V, N, taps.data_ptr(), _ld(taps) if G else K, K,
                steps.data_ptr(), G, po.host.ctypes.data, po.dev.data_ptr(), lbda_scalar,
                lbda_dev.data_ptr() if lbda_dev is not None else None, betas.data_ptr(), int(n_iter), n_done.data_ptr(),
                work.data_ptr(), work.numel(), guard_work.data_ptr(), guard_work.numel(),
                (force if isinstance(force, int) else _FORCE[force]) | cold, _stream_ptr(dev))
        _lib.check(rc, "pb_fista_solve_grouped_guarded")
        return W, n_done
    with torch.cuda.device(dev):
        rc = lib.pb_fista_solve_grouped(
            Y.data_ptr(), _ld(Y) if V else N, W.data_ptr(), _ld(W) if V else N, V, N, taps.data_ptr(), _ld(taps) if G else K, K,
            steps.data_ptr(), G, po.host.ctypes.data, po.dev.data_ptr(), lbda_scalar,
            lbda_dev.data_ptr() if lbda_dev is not None else None, betas.data_ptr(), int(n_iter), n_done.data_ptr(),
            work.data_ptr(), work.numel(), (force if isinstance(force, int) else _FORCE[force]) | cold, _stream_ptr(dev))
    _lib.check(rc, "pb_fista_solve_grouped")
    return W, n_done


def hrf_normal_eq_w_grouped(W, Y, n_taps, offsets, work=None, out=None):
    """:func:`hrf_normal_eq_w` with one set per parcel (rows contiguous by parcel, ``offsets`` as in
    :func:`fista_solve_grouped`): float64 ``(G, K*K + K + 2)``, row ``g`` = the normal equations of parcel ``g``'s rows
    followed by their ``sum ||w_v||_1``, from ONE pass over ``(W, Y)`` with a fixed summation order."""
    lib = _lib.load()
    W = _rows(W, torch.float64, "W")
    Y = _rows(Y, torch.float32, "Y")
    dev = W.device
    V, N = W.shape
    K = int(n_taps)
    po = _parcel_offsets(offsets, dev, V)
    ne = int(lib.pb_hrf_normal_eq_len(K)) + 1
    if out is None:
        out = torch.empty((po.G, ne), dtype=torch.float64, device=dev)
    if out.shape != (po.G, ne) or out.dtype != torch.float64 or out.stride(-1) != 1:
        raise ValueError("out must be float64 %s with contiguous rows" % ((po.G, ne),))
    need = int(lib.pb_hrf_normal_eq_w_grouped_work_len(V, po.G, K))
    if work is None or work.dtype != torch.float64 or work.numel() < need or work.device != dev:
        work = torch.empty((max(need, 1),), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.pb_hrf_normal_eq_w_grouped(W.data_ptr(), _ld(W) if V else N, Y.data_ptr(), _ld(Y) if V else N, V, N, K, po.G,
                                            po.host.ctypes.data, po.dev.data_ptr(), work.data_ptr(), work.numel(),
                                            out.data_ptr(), _ld(out) if po.G else ne, _stream_ptr(dev))
    _lib.check(rc, "pb_hrf_normal_eq_w_grouped")
    return out
