"""Drop-in counterparts of ``pybold/bold_signal.py`` running on MI355X.

Same function names, argument order, defaults and return tuples as the
reference.  ``y`` may be 1-D (reference behaviour, NumPy in / NumPy float64 out)
or a 2-D ``(V, N)`` batch of voxels solved in one kernel launch (the axis the
reference fans out with joblib, examples/icassp_2019/simulation.py:62-72).  A
CUDA tensor in gives CUDA tensors out (x, z, diff_z stay in HBM).

Deviations from the reference, all deliberate:
  * the fixed-lambda ``deconv`` does not print one line per iteration
    (pybold/bold_signal.py:79-80 does, unconditionally);
  * a 2-D batch ``y`` is stored in float32 in HBM (the iterate and its update stay
    float64 on chip); a 1-D ``y`` is computed in float64 end to end; outputs are
    float64 like the reference's;
  * ``_loops_deconv`` does not overwrite the caller's ``diff_z`` (the reference
    does at :261; every caller rebinds the returned array);
  * ``deconv(lbda=None)`` (noise-driven lambda search, :99-214) estimates the
    noise level with an in-package db3 detail band instead of PyWavelets
    (``utils.mad_daub_noise_est``; parity of that estimate is unpinned -- everything
    else of the branch is pinned against the reference with the estimate injected,
    tests/golden/auto_lbda.npz); it computes in float64 end to end, batches included
    (see ``_deconv_auto_lbda``).
  * ``deconv`` / ``deconv_auto`` with a 2-D ``hrf`` ``(V, K)`` -- one HRF per voxel, the last step of the reference's
    per-voxel workflow (``bd`` per voxel, then ``deconv`` with the estimated HRF) -- keep the batch ``y`` in float64
    for that call and compute in float64 end to end, fixed lambda included: voxel ``v`` is solved as the reference
    solves ``deconv(y[v], t_r, hrf[v], ...)``, the ``v``-th of ``V`` consecutive calls (its start vector of the
    power iteration is row ``v`` of one ``np.random.randn(V, N)`` draw).
Beyond the reference's surface: ``deconv_auto`` is that ``lbda=None`` call with the noise level as an argument and the
whole search resident on the device (``engine``), see there.
There is no CPU fallback: without the HIP library or a GPU these raise.
"""
import collections
import os

import numpy as np
import torch
from scipy.optimize import fmin_l_bfgs_b

from . import solver
from .convolution import kernel_from_toeplitz, toeplitz_from_kernel
from .hrf_model import MAX_DELTA, MIN_DELTA, spm_hrf
from .linear import ConvAndLinear, DiscretInteg
from .utils import gram_frobenius, mad_daub_noise_est, spectral_radius_est


class _Shape:
    """How to hand results back: 1-D or batch, NumPy (reference behaviour) or the
    caller's CUDA tensors (no host round trip)."""

    def __init__(self, one_d, on_device):
        self.one_d, self.on_device = one_d, on_device

    def __bool__(self):             # truthiness = "input was 1-D"
        return self.one_d


def _y_to_device(y):
    """-> (CUDA (V, N), _Shape).  A 2-D batch is stored as float32 (the layout of the
    register-resident kernels).  A 1-D series -- the reference's own call pattern -- stays
    float64 and runs on the all-float64 kernels (``pb_fista_solve_d`` & co.): same
    arithmetic as the reference end to end, which also keeps the finite-difference
    L-BFGS-B of the theta-step on the reference's trajectory."""
    if torch.is_tensor(y):
        one_d = y.dim() == 1
        on_device = y.is_cuda
        t = y.to(device=solver.device(y.device if y.is_cuda else None),
                 dtype=torch.float64 if one_d else torch.float32)
    else:
        a = np.asarray(y)
        one_d, on_device = a.ndim == 1, False
        t = torch.from_numpy(np.ascontiguousarray(
            a, dtype=np.float64 if one_d else np.float32)).to(solver.device())
    return (t.reshape(1, -1) if one_d else t), _Shape(one_d, on_device)


def _host(t, shape):
    """Result in the caller's world: float64 NumPy, or the CUDA tensor itself when
    the input was one."""
    if isinstance(shape, _Shape) and shape.on_device:
        return t[0] if shape.one_d else t
    a = t.cpu().numpy()
    return a[0] if shape else a


def _shape_of(a):
    return tuple(a.shape) if torch.is_tensor(a) else tuple(np.shape(a))


def _per_voxel_hrf(y, hrf, who):
    """Whether ``hrf`` holds one HRF per voxel (2-D).  Refuses, before anything touches a device, the shapes that are
    neither that nor the reference's single 1-D HRF."""
    hs, ys = _shape_of(hrf), _shape_of(y)
    if len(hs) < 2:
        return False
    if len(hs) > 2 or len(ys) != 2 or hs[0] != ys[0]:
        raise ValueError("%s: one HRF per voxel takes y of shape (V, N) and hrf of shape (V, K) with the same V; "
                         "got y of shape %s and hrf of shape %s" % (who, ys, hs))
    return True


def _pv_to_device(y, hrf):
    """-> (Y float64 CUDA (V, N), taps float64 CUDA (V, K), _Shape): the per-voxel-HRF calls are float64 end to end."""
    on_device = torch.is_tensor(y) and y.is_cuda
    dev = solver.device(y.device if on_device else None)
    Y = (y if torch.is_tensor(y) else torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64))).to(device=dev, dtype=torch.float64)
    T = (hrf if torch.is_tensor(hrf) else torch.from_numpy(np.ascontiguousarray(hrf, dtype=np.float64))).to(device=dev, dtype=torch.float64)
    if Y.shape[0] == 0:
        raise ValueError("deconv: empty voxel batch")
    return Y, T, _Shape(False, on_device)


def _pv_steps(T, n):
    """``1 / (0.9 rho_v)`` of every voxel's operator (NumPy ``(V,)``): the power iteration of ``spectral_radius_est`` from
    one ``np.random.randn(V, n)`` draw, row ``v`` the draw of the ``v``-th of ``V`` consecutive 1-D calls."""
    rho, _ = solver.spectral_radius_batch(np.random.randn(T.shape[0], n), T)
    return 1.0 / (0.9 * rho)


# How the batch path of `deconv` reaches the library: "ctypes" (pybold_amd._lib, the default) or "torch_ops"
# (torch.ops.pybold_hip: the TORCH_LIBRARY shim over the same C ABI) -- same kernels, bit-identical results
# (tests/test_torch_ops.py).  Initialised from the environment variable PYBOLD_AMD_DISPATCH.
DISPATCH = os.environ.get("PYBOLD_AMD_DISPATCH", "ctypes")

# Which engine a 2-D `deconv(lbda=None)` runs on: "host" (the default: `_deconv_auto_lbda`, one launch over all voxels per
# outer iteration, the outer loop in NumPy) or "device" (`deconv_auto(engine="device")`: the whole search resident on
# the device, one voxel per wave -- series of up to 640 scans, HRFs of up to 32 taps, wind = 6; other shapes keep the
# host loop) or "device_split" (the same, and series of 641 .. 1 280 scans on the search with one voxel per workgroup of four
# waves, `deconv_auto(engine="device_split")`; shapes neither carries keep the host loop).  1-D calls always keep the host
# loop.  "device_split_pp": everything "device_split" does, and calls with one HRF per voxel (a 2-D `hrf`) of 641 .. 1 280
# scans on `deconv_auto(engine="device_split_pp")`.  "device_long_hrf": everything "device" does, and HRFs of 33 .. 48 taps
# (1-D or one per voxel) on series of up to 640 scans on `deconv_auto(engine="device_long_hrf")`.  "device_split_long_hrf":
# everything "device_split" does, and HRFs of 33 .. 48 taps (1-D or one per voxel) on series of 641 .. 1 280 scans on
# `deconv_auto(engine="device_split_long_hrf")`.  Initialised from the environment variable PYBOLD_AMD_AUTO_LBDA.
AUTO_LBDA = os.environ.get("PYBOLD_AMD_AUTO_LBDA", "host")

# Opt-in: the fixed-lambda solves with one HRF per voxel (a 2-D `hrf`: `deconv` with a `lbda`, and the inner solves of the
# host-loop lambda search) run series of 641 .. 1 280 scans on the register-resident form with one voxel per workgroup of
# four waves (`solver.fista_solve_pp_d(force="split")`) instead of the LDS kernel, where `solver.pp_split_supported` says
# the shape is carried.  Off by default: no call changes its kernel unless asked.  Initialised from the environment
# variable PYBOLD_AMD_PP_SPLIT ("1" is on).
PER_VOXEL_SPLIT = os.environ.get("PYBOLD_AMD_PP_SPLIT", "0") == "1"


# Opt-in: the float64 fixed-lambda solves of `deconv` (1-D calls, the inner solves of the host-loop lambda search, a 2-D
# `hrf`) run HRFs of 33 .. 48 taps on series of up to 640 scans on the one-wave register form with the taps in one VGPR pair
# (`force="long_hrf"`) instead of the LDS kernel, where `solver.long_hrf_supported` says the shape is carried.  Off by
# default: no call changes its kernel unless asked.  Initialised from the environment variable PYBOLD_AMD_LONG_HRF ("1" is on).
LONG_HRF = os.environ.get("PYBOLD_AMD_LONG_HRF", "0") == "1"


# Opt-in: the same for series of 641 .. 1 280 scans -- HRFs of 33 .. 48 taps on the four-wave register form with the taps in
# one VGPR pair of every wave (`force="split_long_hrf"`) instead of the LDS kernel, where `solver.split_long_hrf_supported`
# says the shape is carried.  Up to 32 taps the switch names nothing: the existing four-wave forms carry those calls and are
# faster (1.7-1.85x: DESIGN 5.8).  Measured against the LDS kernel at 42 taps, 1 .. 16 384 voxels: 1.2-3.8x faster at 700 scans,
# 2.2-6.0x at 1 200, the host-loop search 2.1-8.9x; no point slower (profiles/split_long_hrf.txt).  Off by default: no call changes
# its kernel unless asked.  Initialised from the environment variable PYBOLD_AMD_SPLIT_LONG_HRF ("1" is on).
SPLIT_LONG_HRF = os.environ.get("PYBOLD_AMD_SPLIT_LONG_HRF", "0") == "1"


# The three switches above: (the module attribute, read at call time; the form of `solver.F64_FORMS` it turns on, whose `force`
# name and solve query are used; the fewest taps at which it names the form -- up to 32 the default register forms carry the call).
_SWITCHES = (("PER_VOXEL_SPLIT", "four_waves", 1), ("LONG_HRF", "long", 33), ("SPLIT_LONG_HRF", "four_waves_long", 33))


def _switch_force(switches, n, n_taps, stop, wind):
    for switch, key, min_taps in switches:
        form = solver.F64_FORMS[key]
        if globals()[switch] and n_taps >= min_taps and getattr(solver, form.public.solve_query)(n, n_taps, stop, wind):
            return form.force
    return None


def _long_hrf_force(n, n_taps, stop, wind):
    """``force`` of a float64 solve: ``"long_hrf"`` when ``LONG_HRF`` is on, the HRF has more than 32 taps (up to 32 the
    default register form carries the call) and the shape is carried; ``"split_long_hrf"`` likewise under
    ``SPLIT_LONG_HRF`` (the two carry disjoint series lengths)."""
    return _switch_force(_SWITCHES[1:], n, n_taps, stop, wind)


def _pv_force(n, n_taps, stop, wind):
    """``force`` of a per-voxel-HRF solve: ``"split"`` when ``PER_VOXEL_SPLIT`` is on and the shape is carried,
    ``"long_hrf"`` / ``"split_long_hrf"`` likewise under ``LONG_HRF`` / ``SPLIT_LONG_HRF``."""
    return _switch_force(_SWITCHES, n, n_taps, stop, wind)


# The engines of the `lbda=None` search that are resident on the device, one row each: the form of `solver.F64_FORMS` whose
# search it runs; the HRFs it takes ("1d": one for all voxels, "pv": one per voxel, "any"); the fewest taps at which it is the
# engine to run; `fallback`: the engine asked next when it does not carry a call -- under `AUTO_LBDA` always ("device_split"
# also means everything "device" does), in `deconv_auto` only with `named_fallback`, where every other engine asked for by name
# refuses; then what `deconv_auto(engine=...)` answers after "deconv_auto(engine='...'): " to the wrong kind of HRF and to a
# shape beyond its limits.
_Engine = collections.namedtuple("_Engine", "name form hrf min_taps fallback named_fallback wrong_hrf limit")
_THIS_CALL = "; this call has %d scans, %d taps, wind = %d"
_SPLIT_LIMIT = ("the four-wave device-resident lambda search carries series of 641..1280 scans, HRFs of up to 32 taps and "
                "wind = 6" + _THIS_CALL)
_ENGINES = collections.OrderedDict((e.name, e) for e in (
    _Engine("device", "one_wave", "any", 1, None, False, None,
            "the device-resident lambda search carries series of up to 640 scans, HRFs of up to 32 taps and wind = 6" + _THIS_CALL),
    _Engine("device_split", "four_waves", "1d", 1, "device", False,
            "the four-wave device-resident lambda search takes one HRF for all voxels; with one HRF per voxel (hrf of shape "
            "{hrf}) the device-resident search carries series of up to 640 scans (engine='device'), longer ones run the host "
            "loop (engine='host') or, opt-in, the four-wave search with per-voxel HRFs (engine='device_split_pp')", _SPLIT_LIMIT),
    _Engine("device_split_pp", "four_waves", "pv", 1, "device_split", False,
            "the four-wave device-resident lambda search with one HRF per voxel takes hrf of shape (V, K); a 1-D hrf runs on "
            "engine='device_split'", _SPLIT_LIMIT),
    _Engine("device_long_hrf", "long", "any", 33, "device", False, None,
            "the device-resident lambda search for long HRFs carries HRFs of 33..48 taps, series of up to 640 scans and "
            "wind = 6 (up to 32 taps: engine='device')" + _THIS_CALL),
    # (asked for by name it still runs what "device_split" does: the existing four-wave search, faster up to 32 taps)
    _Engine("device_split_long_hrf", "four_waves_long", "any", 33, "device_split", True, None,
            "the four-wave device-resident lambda search for long HRFs carries HRFs of 33..48 taps (1-D, or one per voxel), "
            "series of 641..1280 scans and wind = 6 (up to 32 taps with one HRF for all voxels it runs engine='device_split'; "
            "one HRF per voxel of up to 32 taps: engine='device_split_pp'; up to 640 scans: engine='device_long_hrf')"
            + _THIS_CALL)))


def _engine_that_carries(asked, n, n_taps, wind, per_voxel, by_name):
    """The engine of ``_ENGINES`` that runs a call asking for ``asked`` -- itself, or down its fallbacks the first whose
    HRF kind, tap floor and form's search (``solver.auto_lbda*_supported``) fit -- or None.  ``by_name``: as
    ``deconv_auto(engine=asked)`` falls back; else as ``AUTO_LBDA = asked`` does."""
    row = _ENGINES.get(asked)
    while row is not None:
        carried = getattr(solver, solver.F64_FORMS[row.form].public.search_query)
        if row.hrf in ("any", "pv" if per_voxel else "1d") and n_taps >= row.min_taps and carried(n, n_taps, wind):
            return row.name
        row = _ENGINES.get(row.fallback) if (row.named_fallback or not by_name) else None
    return None


def _resolve_engine(engine, n, n_taps, wind, per_voxel, hrf_shape):
    """What ``deconv_auto(engine=engine)`` runs: "host", or the device engine that carries the call; the ``ValueError`` of an
    engine asked for by name that does not; for "auto" the host loop with one warning."""
    if engine == "host":
        return engine
    row = _ENGINES["device" if engine == "auto" else engine]
    if row.hrf not in ("any", "pv" if per_voxel else "1d"):
        raise ValueError("deconv_auto(engine=%r): " % (engine,) + row.wrong_hrf.format(hrf=hrf_shape))
    runs = _engine_that_carries(row.name, n, n_taps, wind, per_voxel, by_name=True)
    if runs is None:
        limit = row.limit % (n, n_taps, wind)
        if engine != "auto":
            raise ValueError("deconv_auto(engine=%r): " % (engine,) + limit)
        solver.warn_once(("auto-lambda-host", n, n_taps, wind), "deconv_auto: " + limit + ": running the host loop.",
                         stacklevel=4)                # (the caller of deconv_auto, as from there)
        runs = "host"
    return runs


def deconv(y, t_r, hrf, lbda=None, early_stopping=True, tol=1.0e-6,  # noqa
           wind=6, nb_iter=1000, nb_sub_iter=1000, verbose=0):
    """Deconvolve BOLD signal(s) ``y`` with the HRF ``hrf``
    (pybold/bold_signal.py:13-97): ``min_w 0.5 ||h * cumsum(w) - y||^2 +
    lbda ||w||_1`` by the reference's FISTA-like loop, constant step
    ``1 / (0.9 rho)``.

    Returns ``(x, z, diff_z, J, None, None)`` with ``J`` normalised by ``J[0]``.
    For a 2-D ``y`` every output gains a leading voxel axis and ``J`` is
    ``(V, max iterations run)`` padded with NaN after a voxel's early stop.

    ``hrf`` of shape ``(V, K)`` beside a ``(V, N)`` batch (NumPy, or a float64 CUDA tensor): ONE HRF PER VOXEL, what ``bd``
    on a batch returns.  Voxel ``v`` is solved as the reference solves ``deconv(y[v], t_r, hrf[v], ...)``, the ``v``-th of
    ``V`` consecutive calls, in float64 end to end (``lbda`` a scalar or ``(V,)``; ``lbda=None`` likewise, see
    ``deconv_auto``).  Any other 2-D or higher ``hrf`` is a ``ValueError``.
    """
    per_voxel = _per_voxel_hrf(y, hrf, "deconv")
    if lbda is None:
        if AUTO_LBDA in _ENGINES and _n_dim(y) == 2:   # (1-D calls, and what no engine of AUTO_LBDA's carries: the host loop)
            n_taps = int(_shape_of(hrf)[-1]) if per_voxel else np.size(hrf)
            engine = _engine_that_carries(AUTO_LBDA, _n_scans(y), n_taps, wind, per_voxel, by_name=False)
            if engine:
                return deconv_auto(y, t_r, hrf, early_stopping=early_stopping, tol=tol, wind=wind, nb_iter=nb_iter,
                                   nb_sub_iter=nb_sub_iter, engine=engine, verbose=verbose)[:6]
        return _deconv_auto_lbda(y, hrf, early_stopping, tol, wind, nb_iter, nb_sub_iter, verbose)
    if per_voxel:
        # one HRF per voxel: float64 end to end (pb_fista_solve_pp_d; the torch.ops shim has no such operator, so
        # DISPATCH == "torch_ops" takes this path too)
        Y, T, one_d = _pv_to_device(y, hrf)
        stop = "window" if early_stopping else None
        W, J, n_done = solver.fista_solve_pp_d(Y, T, _pv_steps(T, Y.shape[1]), lbda, int(nb_iter), want_J=True,
                                               stop=stop, tol=tol, wind=wind,
                                               force=_pv_force(Y.shape[1], T.shape[1], stop, wind))
        X, Z = solver.fista_outputs_pp(W, T)
        return _deconv_results(Y, one_d, X, Z, W, J, n_done, verbose)
    Y, one_d = _y_to_device(y)
    n = Y.shape[1]
    if Y.shape[0] == 0:
        raise ValueError("deconv: empty voxel batch")
    hrf = np.asarray(hrf, dtype=np.float64)
    H = ConvAndLinear(DiscretInteg(), hrf, dim_in=n, dim_out=n)
    grad_lipschitz_cst = 0.9 * spectral_radius_est(H, (n,))
    step = 1.0 / grad_lipschitz_cst
    if DISPATCH == "torch_ops" and Y.dtype == torch.float32:
        # the same kernels through the registered PyTorch operators (torch.ops.pybold_hip, csrc/torch_ops.cpp)
        from . import torch_ops
        W, J, n_done = torch_ops.fista_solve(Y, hrf, lbda, step, int(nb_iter), want_J=True,
                                             stop_mode=solver._STOP["window" if early_stopping else None],
                                             tol=tol, wind=wind)
        X, Z = torch_ops.load().fista_outputs(W, torch.from_numpy(np.ascontiguousarray(hrf)).to(W.device))
    else:
        stop = "window" if early_stopping else None
        W, J, n_done = solver.fista_solve(
            Y, hrf, lbda, step, int(nb_iter), want_J=True, stop=stop, tol=tol, wind=wind,
            force=_long_hrf_force(n, hrf.size, stop, wind) if Y.dtype == torch.float64 else None)
        X, Z = solver.fista_outputs(W, hrf)
    return _deconv_results(Y, one_d, X, Z, W, J, n_done, verbose)


def _deconv_results(Y, one_d, X, Z, W, J, n_done, verbose):
    """The return tuple of the fixed-lambda ``deconv``: ``J`` normalised by ``J[0]`` and NaN-padded after a voxel's stop."""
    n_max = max(int(n_done.max()), 1)
    if one_d.on_device:
        # CUDA in -> CUDA out: the cost trace is normalised on the device and stays there
        # (a (V, n_iter) trace of a large batch is hundreds of MB: no PCIe round trip)
        Jd = J[:, :n_max].to(torch.float64)
        Jd = Jd / (Jd[:, :1] + 1.0e-30)
        if verbose > 0:
            last = Jd.gather(1, (n_done.long() - 1).clamp(min=0)[:, None])
            print("deconv: {0} voxel(s), {1} iteration(s), final normalised cost "
                  "{2:.6f}".format(Y.shape[0], n_max, float(last.nanmean())))
        if one_d:
            return X[0], Z[0], W[0], Jd[0, :int(n_done[0])], None, None
        return X, Z, W, Jd, None, None
    n_done = n_done.cpu().numpy()
    J = J.cpu().numpy().astype(np.float64)[:, :n_max]
    J = J / (J[:, :1] + 1.0e-30)
    if verbose > 0:
        print("deconv: {0} voxel(s), {1} iteration(s), final normalised cost "
              "{2:.6f}".format(Y.shape[0], int(n_done.max()),
                               float(np.nanmean(J[np.arange(len(n_done)), n_done - 1]))))
    if one_d:
        return _host(X, one_d), _host(Z, one_d), _host(W, one_d), J[0, :n_done[0]], None, None
    return _host(X, one_d), _host(Z, one_d), _host(W, one_d), J, None, None


def _n_dim(y):
    return y.dim() if torch.is_tensor(y) else np.ndim(y)


def _n_scans(y):
    return int(y.shape[-1]) if torch.is_tensor(y) else int(np.shape(y)[-1])


def deconv_auto(y, t_r, hrf, sigma=None, early_stopping=True, tol=1.0e-6, wind=6, nb_iter=1000,  # noqa
                nb_sub_iter=1000, outer_chunk=None, engine="auto", verbose=0):
    """``deconv(y, t_r, hrf)`` with ``lbda=None`` -- the reference's default call, its noise-driven lambda search
    (pybold/bold_signal.py:99-214) -- with the engine and the noise level in the caller's hands.

    sigma   noise level per voxel (scalar for a 1-D ``y``, ``(V,)`` array or tensor for a batch); ``None``: the db3
            MAD estimate (``mad_daub_noise_est``), on the device for a CUDA ``y``, on the host otherwise
    engine  "device": the whole search as one device-resident solve (``solver.auto_lbda_solve``: one voxel per
            wave, no host round trip; series of up to 640 scans, HRFs of up to 32 taps, ``wind == 6`` --
            ``ValueError`` otherwise); "host": the host-driven loop ``deconv(lbda=None)`` runs by default;
            "auto": the device where it carries the call, else the host loop with one warning;
            "device_split": the device-resident solve with one voxel per workgroup of four waves
            (``solver.auto_lbda_solve_split``: series of 641 .. 1 280 scans, HRFs of up to 32 taps, ``wind == 6`` --
            ``ValueError`` otherwise; ``"device"`` and ``"auto"`` do not reach it);
            "device_split_pp": the same with one HRF per voxel (``solver.auto_lbda_solve_split_pp``; a 2-D ``hrf`` is
            required, the same limits -- ``ValueError`` otherwise; no other engine reaches it);
            "device_long_hrf": the one-wave device-resident solve for HRFs of 33 .. 48 taps (``solver.auto_lbda_solve_long`` /
            ``solver.auto_lbda_solve_long_pp``: a 1-D or ``(V, K)`` ``hrf``, series of up to 640 scans, ``wind == 6`` --
            ``ValueError`` otherwise; no other engine reaches it, ``"device"`` and ``"auto"`` keep their limit of 32 taps);
            "device_split_long_hrf": everything ``"device_split"`` does, and HRFs of 33 .. 48 taps on series of 641 .. 1 280
            scans on the four-wave search with the taps in one VGPR pair of every wave (``solver.auto_lbda_solve_split_long``;
            a ``(V, K)`` ``hrf`` on ``solver.auto_lbda_solve_split_long_pp``), ``wind == 6`` -- ``ValueError`` otherwise; no
            other engine reaches it
    hrf     1-D, or ``(V, K)`` beside a ``(V, N)`` batch: one HRF per voxel (``solver.auto_lbda_solve_pp`` on the device engine,
            the host loop on ``solver.fista_solve_pp_d``; ``"device_split"`` takes one HRF for all voxels, ``ValueError``;
            ``"device_split_pp"`` takes one per voxel)
    outer_chunk  device engine: outer iterations per kernel launch (``None``: the library's choice); no effect on
            the result

    Returns ``(x, z, diff_z, J, R, G, info)``: the first six exactly as ``deconv(lbda=None)`` returns them for the
    same input (lists for a 1-D ``y``; ``(n_outer, V)`` arrays padded with NaN for a batch, trimmed to the longest
    row's outer iterations; CUDA in -> ``x, z, diff_z`` CUDA); ``info`` holds ``alpha``, ``lbda`` (final, per
    voxel), ``n_outer``, ``n_inner`` (outer / summed inner iterations per voxel), ``sigma`` and ``engine``."""
    if engine not in ("auto", "host") + tuple(_ENGINES):
        raise ValueError("deconv_auto: engine must be 'auto', 'device', 'host', 'device_split', 'device_split_pp', "
                         "'device_split_long_hrf' or 'device_long_hrf', got %r" % (engine,))
    per_voxel = _per_voxel_hrf(y, hrf, "deconv_auto")
    n, n_taps = _n_scans(y), (int(_shape_of(hrf)[-1]) if per_voxel else int(np.size(hrf)))
    engine = _resolve_engine(engine, n, n_taps, wind, per_voxel, _shape_of(hrf))
    on_device = torch.is_tensor(y) and y.is_cuda
    if sigma is None:
        if on_device and 5 <= n <= solver.MAD_DAUB_NMAX and y.dtype in (torch.float32, torch.float64):
            sigma = solver.mad_daub_noise_est(torch.atleast_2d(y))
        else:
            y_host = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y, dtype=np.float64)
            sigma = np.atleast_1d(mad_daub_noise_est(y_host))
    if engine == "host":
        info = {}
        out = _deconv_auto_lbda(y, hrf, early_stopping, tol, wind, nb_iter, nb_sub_iter, verbose, sigma=sigma, info=info)
        info["engine"] = "host"
        return out + (info,)

    names = solver.F64_FORMS[_ENGINES[engine].form].public      # (looked up on `solver` at call time)
    if per_voxel:
        Y, T, one_d = _pv_to_device(y, hrf)
        V = Y.shape[0]
        solve = getattr(solver, names.search_pp)
        W, res = solve(Y, T, _pv_steps(T, n), sigma, early_stopping=early_stopping, tol=tol, wind=wind,
                       nb_iter=int(nb_iter), nb_sub_iter=int(nb_sub_iter), outer_chunk=int(outer_chunk or 0))
        X, Z = solver.fista_outputs_pp(W, T)
        return _deconv_auto_results(one_d, V, X, Z, W, res, sigma, engine, verbose)
    one_d = _Shape(_n_dim(y) == 1, on_device)
    if torch.is_tensor(y):
        Y = torch.atleast_2d(y).to(device=solver.device(y.device if on_device else None), dtype=torch.float64)
    else:
        Y = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(np.asarray(y, dtype=np.float64)))).to(solver.device())
    V = Y.shape[0]
    if V == 0:
        raise ValueError("deconv_auto: empty voxel batch")
    hrf = np.asarray(hrf, dtype=np.float64)
    H = ConvAndLinear(DiscretInteg(), hrf, dim_in=n, dim_out=n)
    step = 1.0 / (0.9 * spectral_radius_est(H, (n,)))
    solve = getattr(solver, names.search)
    W, res = solve(Y, hrf, step, sigma, early_stopping=early_stopping, tol=tol, wind=wind,
                   nb_iter=int(nb_iter), nb_sub_iter=int(nb_sub_iter), outer_chunk=int(outer_chunk or 0))
    X, Z = solver.fista_outputs(W, hrf)
    return _deconv_auto_results(one_d, V, X, Z, W, res, sigma, engine, verbose)


def _deconv_auto_results(one_d, V, X, Z, W, res, sigma, engine, verbose):
    """The return tuple of ``deconv_auto`` from what a device-resident search hands back."""
    n_outer = res["n_outer"].cpu().numpy()
    n_max = int(n_outer.max())
    J, R, G = (res[k][:, :n_max].t().cpu().numpy() for k in ("J", "R", "G"))       # (n_outer, V), NaN after a row's stop
    info = {"alpha": res["alpha"].cpu().numpy(), "lbda": res["lbda"].cpu().numpy(), "n_outer": n_outer,
            "n_inner": res["n_inner"].cpu().numpy(),
            "sigma": sigma.cpu().numpy() if torch.is_tensor(sigma) else np.broadcast_to(np.asarray(sigma, dtype=np.float64), (V,)).copy(),
            "engine": engine}
    if verbose > 0:
        print("deconv_auto: {0} voxel(s), {1} outer iteration(s) at most, {2} inner iterations in all".format(
            V, n_max, int(info["n_inner"].sum())))
    if one_d:
        return (_host(X, one_d), _host(Z, one_d), _host(W, one_d), [float(v) for v in J[:, 0]],
                [float(v) for v in R[:, 0]], [float(v) for v in G[:, 0]], info)
    return _host(X, one_d), _host(Z, one_d), _host(W, one_d), J, R, G, info


def _deconv_auto_lbda(y, hrf, early_stopping, tol, wind, nb_iter, nb_sub_iter, verbose, sigma=None, info=None):
    """``lbda=None`` branch of ``deconv`` (pybold/bold_signal.py:99-214), batched.

    Per voxel: ``sigma`` = db3 MAD noise level (:103); ``alpha_0 = 1``,
    ``lbda = 1/(2 alpha)``, ``mu = 1e-4`` (:104-106); each outer iteration runs a
    warm-started inner solve of at most ``nb_sub_iter`` iterations with the
    window rule (ONE kernel launch for all voxels, per-voxel lambda), then
    ``alpha += mu (||x - y||^2 - N sigma^2)`` (:141-145); a voxel leaves the
    outer loop on the windowed ``alpha`` rule (:164-178) and keeps its iterate;
    a last inner solve (:181-209) ends the run.  Returns ``(x, z, diff_z, J, R, G)``:
    lists of floats for a 1-D ``y`` (as the reference), ``(n_outer, V)`` arrays
    padded with NaN for a batch.
    """
    y_host = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y, dtype=np.float64)
    if sigma is None:
        sigma = np.atleast_1d(mad_daub_noise_est(y_host))
    else:                                            # the caller's noise level (deconv_auto): scalar or one per voxel
        sigma = np.atleast_1d(sigma.detach().cpu().numpy() if torch.is_tensor(sigma) else np.asarray(sigma, dtype=np.float64))
    per_voxel = _per_voxel_hrf(y, hrf, "deconv")
    if per_voxel:
        Y, T, one_d = _pv_to_device(y, hrf)
    else:
        Y, one_d = _y_to_device(y)
    if Y.dtype != torch.float64:
        if Y.shape[0] >= 1024:
            solver.warn_once("auto-lambda-f64",
                             "deconv(lbda=None) on %d voxels runs on the all-float64 kernels (one problem per wave, ~3x "
                             "slower than the float32-FIR batch kernels; one problem per workgroup of four waves for "
                             "641..1280 scans; the LDS kernel beyond 1280 scans / 32 taps): "
                             "the decisions of this branch sit on rounding knife edges." % Y.shape[0])
        # Two knife edges (both pinned against the reference: tests/golden/auto_lbda.npz).  (1) The inner window rule
        # compares iterates with gradient points (the aliasing of :65/:72), so its criterion tends to a CONSTANT
        # proportional to lambda instead of 0; the search drives lambda down until that constant crosses `tol`, i.e.
        # "stop the inner solve after 8 iterations or run all of them" flips on the 1e-7 rounding of the float32-FIR
        # kernels (measured: whole trajectories diverge).  (2) alpha -- hence lambda = 1/(2 alpha) -- goes NEGATIVE
        # in the reference (:141-145; it does in its default call on the golden series) and :66 with a negative
        # threshold is discontinuous at 0: sign(u) |th|.  The reference keeps the last sample of diff_z EXACTLY 0
        # (h[0] = 0); a float32 residue there is blown up to |th| per iteration.  So the whole branch runs on the
        # float64 kernels, which restate :66 and keep that zero (fista_exact.h, generic.h), batches included.
        if torch.is_tensor(y) and y.is_cuda:                 # already on the device: widen there
            Y = Y.double() if y.dtype != torch.float64 else torch.atleast_2d(y).contiguous()
        else:
            Y = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(y_host), dtype=np.float64)).to(Y.device)
    V, n = Y.shape
    dev = Y.device
    stop = "window" if early_stopping else None
    if per_voxel:                                  # one HRF and one step per voxel: the same loop on the per-voxel entry points
        steps = _pv_steps(T, n)
        force = _pv_force(n, T.shape[1], stop, wind)

        def solve(lbda, W):
            return solver.fista_solve_pp_d(Y, T, steps, lbda, int(nb_sub_iter), W0=W, stop=stop, tol=tol, wind=wind,
                                           force=force)

        def stats(W):
            return solver.fista_stats_pp(W, Y, T)

        def outputs(W):
            return solver.fista_outputs_pp(W, T)
    else:
        hrf = np.asarray(hrf, dtype=np.float64)
        H = ConvAndLinear(DiscretInteg(), hrf, dim_in=n, dim_out=n)
        grad_lipschitz_cst = 0.9 * spectral_radius_est(H, (n,))
        step = 1.0 / grad_lipschitz_cst

        def solve(lbda, W):
            return solver.fista_solve(Y, hrf, lbda, step, int(nb_sub_iter), W0=W, stop=stop, tol=tol, wind=wind,
                                      force=_long_hrf_force(n, hrf.size, stop, wind))

        def stats(W):
            return solver.fista_stats(W, Y, hrf)

        def outputs(W):
            return solver.fista_outputs(W, hrf)

    alpha = np.ones(V)
    lbda = 1.0 / (2.0 * alpha)
    mu = 1.0e-4
    active = np.ones(V, dtype=bool)
    l_alpha = []                                   # last `wind` alpha vectors
    J, R, G = [], [], []
    W = torch.zeros((V, n), dtype=torch.float64, device=dev)
    n_inner = torch.zeros((V,), dtype=torch.int64, device=dev) if info is not None else None
    n_outer = np.zeros(V, dtype=np.int32)
    for i in range(nb_iter):
        W_new, _, n_done = solve(lbda, W)
        n_outer += active
        if n_inner is not None:                      # (inner iterations of the voxels still searching: deconv_auto's info)
            n_inner += torch.where(torch.from_numpy(active).to(dev), n_done.long(), torch.zeros_like(n_inner))
        if active.all():
            W = W_new
        else:
            W = torch.where(torch.from_numpy(active).to(dev)[:, None], W_new, W)
        r2, l1 = stats(W)
        r, g = r2.cpu().numpy(), l1.cpu().numpy()
        grad = r - n * sigma ** 2
        alpha = np.where(active, alpha + mu * grad, alpha)
        lbda = 1.0 / (2.0 * alpha)
        l_alpha.append(alpha.copy())
        if len(l_alpha) > wind:
            l_alpha = l_alpha[1:]
        nan = np.where(active, 0.0, np.nan)
        R.append(r + nan)
        G.append(g + nan)
        J.append(0.5 * r + lbda * g + nan)
        if verbose > 0:
            print("Main loop: iteration {0:03d}, |grad| = {1:0.6f}, lbda = {2:0.6f},".format(
                i + 1, float(np.abs(grad[active]).mean()), float(lbda[active].mean())))
        if early_stopping and i > wind:
            sub_wind_len = int(wind / 2)
            old_iter = np.mean(l_alpha[:-sub_wind_len], axis=0)
            new_iter = np.mean(l_alpha[-sub_wind_len:], axis=0)
            diff = np.abs(new_iter - old_iter) / np.abs(new_iter)
            active &= ~(diff < tol)
            if not active.any():
                break
    W, _, n_done = solve(lbda, W)
    X, Z = outputs(W)
    if info is not None:
        info.update(alpha=alpha.copy(), lbda=lbda.copy(), n_outer=n_outer, n_inner=(n_inner + n_done.long()).cpu().numpy(),
                    sigma=np.broadcast_to(sigma, (V,)).copy())
    if one_d:
        keep = [k for k in range(len(J)) if not np.isnan(J[k][0])]
        return (_host(X, one_d), _host(Z, one_d), _host(W, one_d), [float(J[k][0]) for k in keep],
                [float(R[k][0]) for k in keep], [float(G[k][0]) for k in keep])
    return (_host(X, one_d), _host(Z, one_d), _host(W, one_d), np.array(J), np.array(R),
            np.array(G))


def hrf_fit_err(theta, z, y, t_r, hrf_dur):
    """``0.5 || y - h(theta) * z ||^2`` (pybold/bold_signal.py:217-222); the
    convolution and the reduction run on the GPU."""
    theta = float(np.ravel(theta)[0])
    h, _ = spm_hrf(theta, t_r, hrf_dur, False)
    Y, _ = _y_to_device(y)
    Z = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(np.asarray(z, dtype=np.float64)))).to(Y.device)
    return float(solver.hrf_cost(Z, Y, h).sum().item())


class _Tracker:
    """L-BFGS-B callback recording the cost (pybold/utils.py:28-45)."""

    def __init__(self, f, args, verbose=0):
        self.J, self.f, self.args, self.verbose, self.idx = [], f, list(args), verbose, 0

    def __call__(self, x):
        self.idx += 1
        j = self.f(*([x] + self.args))
        if self.verbose > 2:
            print("At iterate {0}, tracked function = {1:.6f}".format(self.idx, j))
        self.J.append(j)


def hrf_estim(z, y, t_r, dur, verbose=0):
    """HRF dilation fit for a known block signal (pybold/bold_signal.py:225-239)."""
    args = (z, y, t_r, dur)
    bounds = [(MIN_DELTA + 1.0e-1, MAX_DELTA - 1.0e-1)]
    f_cost = _Tracker(hrf_fit_err, args, verbose)
    theta, _, _ = fmin_l_bfgs_b(func=hrf_fit_err, x0=MAX_DELTA, args=args, bounds=bounds,
                                approx_grad=True, callback=f_cost, maxiter=99999,
                                pgtol=1.0e-12)
    h, _ = spm_hrf(float(np.ravel(theta)[0]), t_r, dur, False)
    return h, f_cost.J


class _BlindTrace:
    """Normalised cost bookkeeping of ``bd`` (pybold/bold_signal.py:306-313,
    :337-342, :371-380): residual ``r`` and cost ``J`` relative to their initial
    values, sparsity ``g`` raw."""

    def __init__(self, x, y, w, lbda):
        self.y, self.lbda = y, lbda
        self.r0 = float(np.sum(np.square(x - y)))
        g0 = float(np.sum(np.abs(w)))
        self.j0 = self.r0 + lbda * g0
        self.J, self.r, self.g, self.theta = [1.0], [1.0], [g0], []

    def record(self, x, w, eps):
        r = float(np.sum(np.square(x - self.y)))
        g = float(np.sum(np.abs(w)))
        self.J.append((r + self.lbda * g) / self.j0 + eps)
        self.r.append(r / self.r0 + eps)
        self.g.append(g)

    def stalled(self, wind, tol):
        half = int(wind / 2)                          # rule of :350-356
        older, newer = np.mean(self.J[:-half]), np.mean(self.J[-half:])
        return (newer - older) / newer < tol

    def as_dict(self):
        return {'J': np.array(self.J), 'r': np.array(self.r), 'g': np.array(self.g),
                'l_alpha': [], 'theta': np.array(self.theta)}     # 'theta': extra key (per outer iteration)


def _loops_deconv(y, diff_z, H, lbda, nb_iter, early_stopping, wind, tol):
    """Inner FISTA loop of the blind solver (pybold/bold_signal.py:246-278):
    warm start ``diff_z``, step ``1 / ||A^T A||_F`` with ``A = H tril(1)``.
    ``H`` must be the causal Toeplitz matrix of an HRF (what ``bd`` passes);
    the GPU works matrix-free from its first column.  Returns ``diff_z``."""
    taps = kernel_from_toeplitz(H)
    Y, one_d = _y_to_device(y)
    n = Y.shape[1]
    step = 1.0 / gram_frobenius(taps, n)
    W0 = torch.from_numpy(np.ascontiguousarray(
        np.atleast_2d(np.asarray(diff_z, dtype=np.float64)))).to(Y.device)
    W, _, _ = solver.fista_solve(Y, taps, lbda, step, int(nb_iter), W0=W0,
                                 stop="loops" if early_stopping else None, tol=tol, wind=wind)
    return _host(W, one_d)


def bd(y, t_r, lbda=1.0, theta_0=None, z_0=None, hrf_dur=20.0,  # noqa
       bounds=None, nb_iter=100, nb_sub_iter=1000, nb_last_iter=10000,
       print_period=50, early_stopping=False, wind=4, tol=1.0e-12, verbose=0):
    """Blind deconvolution of one voxel (pybold/bold_signal.py:281-382):
    alternate the GPU z-step (:func:`_loops_deconv`, ``nb_iter`` inner
    iterations exactly like the reference's call at :324) with a bounded
    L-BFGS-B fit of the HRF dilation ``theta`` on the GPU-evaluated cost.
    ``nb_sub_iter`` and ``nb_last_iter`` are accepted and unused, as in the
    reference.  Returns ``(x, z, diff_z, h, d)``.

    A 2-D ``y`` (voxels, scans) is solved for all voxels at once with one HRF
    dilation per voxel (``pybold_amd.blind.bd_batch``; the theta-step is then a
    batched section search instead of SciPy's L-BFGS-B, see that module)."""
    if (torch.is_tensor(y) and y.dim() == 2) or (not torch.is_tensor(y) and np.ndim(y) == 2):
        from .blind import bd_batch
        Y, shape = _y_to_device(y)
        X, Z, W, taps, d = bd_batch(Y, t_r, lbda=lbda, theta_0=theta_0, z_0=z_0, hrf_dur=hrf_dur,
                                    bounds=bounds, nb_iter=nb_iter, early_stopping=early_stopping,
                                    wind=wind, tol=tol, verbose=verbose)
        return _host(X, shape), _host(Z, shape), _host(W, shape), _host(taps, shape), d
    y = np.asarray(y).astype(np.float64)
    n = len(y)
    dev = solver.device()
    theta = MAX_DELTA if theta_0 is None else theta_0
    h, _ = spm_hrf(theta, t_r, hrf_dur, False)       # may lie outside `bounds` (:291-292)
    if bounds is None:
        bounds = [(MIN_DELTA + 1.0e-1, MAX_DELTA - 1.0e-1)]

    def outputs(w, taps):
        X, Z = solver.fista_outputs(torch.from_numpy(np.ascontiguousarray(w[None])).to(dev), taps)
        return X.cpu().numpy()[0], Z.cpu().numpy()[0]

    if z_0 is None:
        diff_z = np.zeros(n)
        x = np.zeros(n)
    else:                                            # warm start from a block signal (:299-301)
        z_0 = np.asarray(z_0, dtype=np.float64)
        diff_z = np.concatenate([[0.0], np.diff(z_0)])
        x = solver.conv(torch.from_numpy(z_0[None].copy()).to(dev), h).cpu().numpy()[0]

    trace = _BlindTrace(x, y, diff_z, lbda)
    if verbose > 0:
        print("normalized global cost-function (init): {0:.6f}".format(trace.J[-1]))

    def z_step(w, taps):
        return _loops_deconv(y, w, toeplitz_from_kernel(taps, dim_in=n, dim_out=n), lbda, nb_iter,
                             early_stopping, wind, tol)

    for idx in range(nb_iter):
        diff_z = z_step(diff_z, h)
        z = DiscretInteg().op(diff_z)                 # block signal of this iterate (:326)
        theta, _, _ = fmin_l_bfgs_b(func=hrf_fit_err, x0=theta, args=(z, y, t_r, hrf_dur),
                                    bounds=bounds, approx_grad=True, maxiter=999, pgtol=1.0e-12)
        trace.theta.append(float(np.ravel(theta)[0]))
        h, _ = spm_hrf(float(np.ravel(theta)[0]), t_r, hrf_dur, False)
        x, z = outputs(diff_z, h)
        trace.record(x, diff_z, eps=1.0e-30)
        if (verbose > 0) and ((idx + 1) % print_period == 0):
            print("normalized global cost-function ({0:03d}/{1:03d}): "
                  "{2:.6f}".format(idx + 1, nb_iter, trace.J[-1]))
        if early_stopping and idx > wind and trace.stalled(wind, tol):
            break

    diff_z = z_step(diff_z, h)                        # last solve with the final HRF (:365-369)
    x, z = outputs(diff_z, h)
    trace.record(x, diff_z, eps=0.0)
    d = trace.as_dict()
    return x, z, diff_z, h, d
