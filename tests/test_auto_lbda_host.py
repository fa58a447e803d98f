"""CPU-only checks of the device-resident lambda search (`pb_auto_lbda_d`, `deconv_auto`) and of the noise-level entry
points: argument validation that never reaches a device, the support table, the register reports of the build, the
exports.  The parity tests are in tests/test_gpu_auto_lbda_device.py."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not glob.glob(os.path.join(ROOT, "pybold_amd", "csrc", "build", "auto_*.res")):
        ge.build()
    return _lib.load()


def _auto(lib, **over):
    """pb_auto_lbda_d on pointers that are never dereferenced: validation must fail first."""
    fake = ctypes.c_void_p(4096)
    taps = np.ones(4)
    a = dict(y=fake, ldy=300, w=fake, ldw=300, cold=1, V=4, N=300, taps=taps.ctypes.data, K=4, step=1.0, betas=fake,
             sigma=fake, early=1, tol=1e-6, wind=6, nb_iter=10, nb_sub_iter=10, chunk=0, R=None, G=None, J=None, ldt=0,
             alpha=fake, lbda=fake, n_outer=fake, n_inner=fake, work=fake, work_len=lib.pb_auto_lbda_work_len(4), stream=None)
    a.update(over)
    rc = lib.pb_auto_lbda_d(a["y"], a["ldy"], a["w"], a["ldw"], a["cold"], a["V"], a["N"], a["taps"], a["K"], a["step"],
                            a["betas"], a["sigma"], a["early"], a["tol"], a["wind"], a["nb_iter"], a["nb_sub_iter"],
                            a["chunk"], a["R"], a["G"], a["J"], a["ldt"], a["alpha"], a["lbda"], a["n_outer"],
                            a["n_inner"], a["work"], a["work_len"], a["stream"])
    return rc, lib.pb_last_error()


def test_auto_lbda_argument_errors_do_not_reach_the_gpu(lib):
    for over, word in ((dict(wind=4), b"wind"), (dict(wind=8), b"wind"), (dict(N=641, ldy=641, ldw=641), b"640"),
                       (dict(K=33), b"32 taps"), (dict(nb_iter=0), b"nb_iter"), (dict(nb_iter=-3), b"nb_iter"),
                       (dict(y=None), b"NULL"), (dict(w=None), b"NULL"), (dict(sigma=None), b"NULL"), (dict(taps=None), b"NULL"),
                       (dict(betas=None), b"NULL"), (dict(work=None), b"NULL"),
                       (dict(work_len=lib.pb_auto_lbda_work_len(4) - 1), b"workspace"), (dict(work_len=0), b"workspace"),
                       (dict(ldy=299), b"leading dimension"), (dict(step=0.0), b"step"),
                       (dict(R=ctypes.c_void_p(4096), ldt=9), b"ldt"), (dict(N=0), b"bad size")):
        rc, msg = _auto(lib, **over)
        assert rc == -1 and word in msg, (over, rc, msg)
    from pybold_amd import _lib
    with pytest.raises(_lib.PyboldHipError):
        _lib.check(_auto(lib, wind=5)[0], "pb_auto_lbda_d")
    # zero voxels is a no-op, not an error
    assert _auto(lib, V=0, work_len=0)[0] == 0
    assert lib.pb_auto_lbda_work_len(0) == 0 and lib.pb_auto_lbda_work_len(1000) >= 10 * 1000


def test_noise_level_argument_errors_do_not_reach_the_gpu(lib):
    fake = ctypes.c_void_p(4096)
    for fn in (lib.pb_mad_daub_noise_est, lib.pb_mad_daub_noise_est_d):
        assert fn(fake, 8193, 3, 8193, 0.6744, fake, None) == -1 and b"8192" in lib.pb_last_error()
        assert fn(fake, 4, 3, 4, 0.6744, fake, None) == -1 and b"outside" in lib.pb_last_error()
        assert fn(fake, 100, 3, 300, 0.6744, fake, None) == -1 and b"bad size" in lib.pb_last_error()
        assert fn(None, 300, 3, 300, 0.6744, fake, None) == -1 and b"NULL" in lib.pb_last_error()
        assert fn(fake, 300, 3, 300, 0.6744, None, None) == -1 and b"NULL" in lib.pb_last_error()
        assert fn(fake, 300, 3, 300, 0.0, fake, None) == -1
        assert fn(fake, 300, 0, 300, 0.6744, fake, None) == 0


def test_supported_shapes(lib):
    """The (S, KT) pairs of exact_table.inc: up to 640 scans, up to 32 taps, and the window of the register-resident rule."""
    for n, k, wind, want in ((1, 1, 6, 1), (5, 1, 6, 1), (64, 27, 6, 1), (300, 30, 6, 1), (320, 32, 6, 1), (321, 32, 6, 1),
                             (640, 32, 6, 1), (641, 30, 6, 0), (640, 33, 6, 0), (1200, 28, 6, 0), (300, 30, 4, 0),
                             (300, 30, 8, 0), (300, 30, 5, 0), (0, 30, 6, 0), (300, 0, 6, 0), (-1, 30, 6, 0)):
        assert lib.pb_auto_lbda_supported(n, k, wind) == want, (n, k, wind)
    from pybold_amd import solver
    assert solver.auto_lbda_supported(300, 30) and not solver.auto_lbda_supported(641, 30)


def test_no_instantiation_of_the_search_kernel_spills(lib):
    """One voxel lives in a wave for up to a million inner iterations: a spill there is paid every pass."""
    table = open(os.path.join(ROOT, "pybold_amd", "csrc", "exact_table.inc")).read()
    pairs = re.findall(r"^PB_EXACT\((\d+), *(\d+)\)", table, flags=re.M)
    assert len(pairs) >= 2
    for s, kt in pairs:
        path = os.path.join(ROOT, "pybold_amd", "csrc", "build", "auto_%s_%s.res" % (s, kt))
        assert os.path.exists(path), path
        text = open(path).read()
        names = re.findall(r"Function Name: (\S*auto_lbda_kernel\S*)", text)
        scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
        assert len(names) == 2 and len(scratch) == 2, (path, names)          # STOP = 0 and STOP = 2
        assert scratch == [0, 0], (path, scratch)


def test_exports_and_switch(monkeypatch):
    import pybold_amd
    from pybold_amd import bold_signal, solver, torch_ops
    assert callable(pybold_amd.deconv_auto) and pybold_amd.deconv_auto is bold_signal.deconv_auto
    assert bold_signal.AUTO_LBDA == os.environ.get("PYBOLD_AMD_AUTO_LBDA", "host")
    assert callable(solver.auto_lbda_solve) and callable(solver.mad_daub_noise_est)
    assert callable(torch_ops.auto_lbda_solve) and callable(torch_ops.mad_daub_noise_est)
    import inspect
    sig = inspect.signature(pybold_amd.deconv_auto)
    assert list(sig.parameters) == ["y", "t_r", "hrf", "sigma", "early_stopping", "tol", "wind", "nb_iter", "nb_sub_iter",
                                    "outer_chunk", "engine", "verbose"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["sigma"], d["early_stopping"], d["tol"], d["wind"], d["nb_iter"], d["nb_sub_iter"], d["outer_chunk"], d["engine"],
            d["verbose"]) == (None, True, 1e-6, 6, 1000, 1000, None, "auto", 0)
    assert "sigma" in inspect.signature(bold_signal._deconv_auto_lbda).parameters
    # shapes the device engine does not carry are refused by name before anything touches a device
    y = np.zeros((2, 641))
    for kw, word in ((dict(), "641 scans"), (dict(wind=4), "wind = 4")):
        with pytest.raises(ValueError, match=word):
            pybold_amd.deconv_auto(y if not kw else np.zeros((2, 300)), 1.0, np.ones(30), sigma=1.0, engine="device", **kw)
    with pytest.raises(ValueError, match="33 taps"):
        pybold_amd.deconv_auto(np.zeros((2, 300)), 1.0, np.ones(33), sigma=1.0, engine="device")
    with pytest.raises(ValueError, match="engine"):
        pybold_amd.deconv_auto(np.zeros((2, 300)), 1.0, np.ones(30), engine="gpu")


def test_operators_are_registered(lib):
    from pybold_amd import torch_ops
    ops = torch_ops.load()
    assert hasattr(ops, "auto_lbda_solve") and hasattr(ops, "mad_daub_noise_est")


# ---- the inputs of the device-against-host comparison (tests/test_gpu_auto_lbda_device.py) -----------------------------
DEVICE_VS_HOST_BUDGETS = ((5, 50, 1.0e-6), (20, 10, 1.0e-6), (60, 300, 1.0e-2))      # (nb_iter, nb_sub_iter, tol)


def device_vs_host_rows(g):
    """64 rows ``(Y (64, 300), sigma (64,))`` from golden cases 1-2 (the series of auto_lbda.npz): scaled and reversed
    copies, each with the fixture's three noise levels, and the negated series with two of them; solved with the HRF of
    case 1.  The scales are chosen so that alpha stays away from 0 in the oracle's own runs (next test): near alpha = 0
    lambda = 1 / (2 alpha) amplifies a last-digit difference without bound (DESIGN, Numerics)."""
    sig = g["c1_sigma"]
    rows = []
    for case, scales in (("c1", (1.0, 1.6, 2.0, 2.5, 3.0)), ("c2", (1.0, 2.0, 2.5, 3.0, 4.0))):
        y = g[case + "_y"]
        for base in (y, y[::-1].copy()):
            for sc in scales:
                rows += [(sc * base, float(s)) for s in sig]
    for case in ("c1", "c2"):
        rows += [(-g[case + "_y"], float(s)) for s in sig[:2]]
    assert len(rows) == 64
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows])


def test_oracle_keeps_alpha_away_from_zero_on_the_comparison_rows(golden):
    """The ground of the 1e-9 bound of the device-against-host test: on every one of its 64 rows and at every budget the
    oracle's alpha trajectory keeps |alpha| > 1e-2, so lambda <= 50 and a rounding-level difference in a residual sum
    (the only thing that differs between the two engines: its reduction order) is not amplified beyond ~1e-12."""
    from oracle import c_oracle
    g = golden("auto_lbda")
    Y, sigma = device_vs_host_rows(g)
    n = Y.shape[1]
    worst = np.inf
    for nb_iter, nb_sub_iter, tol in DEVICE_VS_HOST_BUDGETS:
        _, _, R, _, n_outer = c_oracle.deconv_auto_lbda_batch(Y, g["c1_hrf"], sigma, float(g["c1_lipschitz"]), nb_iter=nb_iter,
                                                             nb_sub_iter=nb_sub_iter, tol=tol, threads=8)
        for v in range(len(sigma)):
            alpha = 1.0 + np.cumsum(1.0e-4 * (R[v, :n_outer[v]] - n * sigma[v] ** 2))
            worst = min(worst, np.abs(alpha).min())
            assert np.abs(alpha).min() > 1.0e-2, (nb_iter, nb_sub_iter, v, np.abs(alpha).min())
    print("min |alpha| over 64 rows x 3 budgets: %.4f" % worst)
