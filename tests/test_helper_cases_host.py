"""CPU-only checks of tests/helper_cases.py, the cases of tests/test_gpu_helper_kernels.py: every reference agrees with an
independent statement (oracle/pybold_oracle.py, a plain double loop for the rectangular products); every integer case meets
its 2^53 precondition and keeps its bits in another summation order (the kernels' own chunked scan, taps descending);
every derived bound covers the error of plain float64 NumPy and of the emulated scan, and the carrier row does cancel; the
LDS formulas are the library's (empty batches: no GPU); the case list is complete; and two one-line mutants of the block
primitives -- a chunk total that drops its last element, a tap range one short -- break the integer-family equality."""
import ctypes
import os

import numpy as np
import pytest

import helper_cases as hc
from oracle import pybold_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_ROW_CASES = tuple(c for g in ("operators", "outputs", "statistics") for c in hc.row_cases(g))
SMALL = tuple(c for c in ALL_ROW_CASES if max(c.n_in, c.n_out) <= 65 and c.n_in == c.n_out)
RECT_CASES = tuple(c for c in ALL_ROW_CASES if c.n_in != c.n_out)

needs_longdouble = pytest.mark.skipif(not hc.LD_OK, reason="np.longdouble has a %d-bit mantissa here (63 needed for the real "
                                                           "family's reference)" % hc.LD_NMANT)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


# ---- an independent statement of every operation (float64) -----------------------------------------------------------------
def oracle_outputs(case, inp):
    x, k, y = inp["x"].astype(np.float64), inp["taps"], None if inp["y"] is None else inp["y"].astype(np.float64)
    e = case.entry[:-2] if case.entry.endswith("_d") else case.entry
    n_in, n_out = case.n_in, case.n_out
    if e == "integ_op":
        return {"out": orc.integ_op(x)}
    if e == "integ_adj":
        return {"out": orc.integ_adj(x)}
    if e in ("conv", "corr", "op_forward", "op_adjoint"):
        T = orc.toeplitz_from_kernel(k, n_in, n_out)
        if e == "conv":
            return {"out": x.dot(T.T)}
        if e == "corr":
            return {"out": x.dot(T)}
        if e == "op_forward":
            return {"out": orc.integ_op(x).dot(T.T)}
        return {"out": orc.integ_adj(x.dot(T))}
    if e == "outputs":
        xo, z = orc.fista_outputs(x, k)
        return {"z": z, "x": xo}
    if e == "outputs_pp":
        pairs = [orc.fista_outputs(x[r], k[r]) for r in range(len(x))]
        return {"z": np.stack([p[1] for p in pairs]), "x": np.stack([p[0] for p in pairs])}
    if e == "stats":
        H = orc.DenseH(k, n_in)
        yy = y[np.arange(len(x)) // case.opt]
        return {"r2": ((H.op(x) - yy) ** 2).sum(axis=1), "l1": np.abs(x).sum(axis=1)}
    if e == "lambda_max":
        return {"out": orc.lambda_max(y, k)}
    if e == "hrf_cost":
        return {"cost": np.stack([0.5 * ((y - orc.causal_conv(k[c], x)) ** 2).sum(axis=1) for c in range(case.opt)])}
    if e == "hrf_cost_pv":
        return {"cost": np.stack([[0.5 * ((y[v] - orc.causal_conv(k[c, v], x[v])) ** 2).sum() for v in range(len(x))]
                                  for c in range(case.opt)])}
    raise KeyError(case.entry)


@pytest.mark.parametrize("case", SMALL + RECT_CASES, ids=hc.case_id)
def test_references_agree_with_the_oracle(case):
    ref = hc.reference(case, "integer")
    want = oracle_outputs(case, ref["inputs"])
    for name, (v, _) in ref["outs"].items():
        assert bits_equal(v, want[name]), (hc.case_id(case), name)        # integers: exact in any statement
    if hc.LD_OK:
        ref = hc.reference(case, "real")
        want = oracle_outputs(case, ref["inputs"])
        for name, (v, b) in ref["outs"].items():
            assert hc.ratio(want[name], v, b) <= 1.0, (hc.case_id(case), name)


@pytest.mark.parametrize("case", [c for c in RECT_CASES if c.entry in ("conv", "corr")], ids=hc.case_id)
def test_rectangular_products_against_a_double_loop(case):
    ref = hc.reference(case, "integer")
    x, k = ref["inputs"]["x"], ref["inputs"]["taps"]
    n_src, n_dst = x.shape[1], (case.n_out if case.entry == "conv" else case.n_in)
    out = np.zeros((len(x), n_dst))
    for i in range(n_dst):
        for m in range(case.K):
            s = i - m if case.entry == "conv" else i + m
            if 0 <= s < n_src:
                out[:, i] += k[m] * x[:, s]
    assert bits_equal(out, ref["outs"]["out"][0])


# ---- the two families --------------------------------------------------------------------------------------------------
def test_integer_family_precondition_and_order_independence():
    for case in ALL_ROW_CASES + tuple(hc.limit_case(e) for e in hc.ROW_ENTRIES):
        rows = 3 if case in ALL_ROW_CASES else 2
        ref = hc.reference(case, "integer", rows)
        assert max(ref["mags"]) < hc.TWO53, hc.case_id(case)
        assert np.abs(ref["inputs"]["x"]).max() >= 1
        other = hc.evaluate(case, ref["inputs"], np.float64, None, emu=True, rev_taps=True)
        for name, (v, _) in ref["outs"].items():
            assert bits_equal(other[name][0], v), (hc.case_id(case), name)


@needs_longdouble
def test_real_family_bounds_cover_float64_numpy_and_the_emulated_scan():
    worst = {}
    for case in ALL_ROW_CASES + tuple(hc.limit_case(e) for e in hc.ROW_ENTRIES):
        rows = 3 if case in ALL_ROW_CASES else 2
        ref = hc.reference(case, "real", rows)
        for emu in (False, True):
            got = hc.evaluate(case, ref["inputs"], np.float64, None, emu=emu)
            for name, (v, b) in ref["outs"].items():
                assert (b >= 0).all() and np.isfinite(b.astype(np.float64)).all()      # (0: a sum of no terms)
                r = hc.ratio(got[name][0], v, b)
                assert r <= 1.0, (hc.case_id(case), name, emu, r)
                worst[emu] = max(worst.get(emu, 0.0), r)
    print("worst error / bound: plain NumPy %.3f, emulated block_cumsum %.3f" % (worst[False], worst[True]))
    assert worst[False] > 1.0e-3 and worst[True] > 1.0e-3          # (not vacuous: within three decades of the errors)


@needs_longdouble
def test_the_carrier_row_cancels():
    for case in ALL_ROW_CASES:
        if case.entry in hc.CUMSUM_ON_ROW and case.n_in >= 2:
            assert hc.cancellation(case) >= 1.0e6, hc.case_id(case)


@needs_longdouble
def test_subtracting_the_own_chunk_total_misses_the_bound():
    """The scan as it was before this test existed -- prefix = wave offset + inclusive total - own total -- rounds at the size
    of the thread's own chunk: on the row that spans twelve decades it misses the per-element bound by orders of magnitude,
    while the scan from the neighbour's inclusive total stays inside (the regression the GPU cases hold)."""
    now, old = 0.0, 0.0
    for case in hc.row_cases("operators"):
        if case.entry in hc.INTEG and case.n_in > hc.THREADS:          # (two or more elements per thread)
            ref = hc.reference(case, "real")
            v, b = ref["outs"]["out"]
            rev = case.entry == "integ_adj"
            now = max(now, hc.ratio(hc.emu_block_cumsum(ref["inputs"]["x"], rev), v, b))
            old = max(old, hc.ratio(hc.emu_block_cumsum(ref["inputs"]["x"], rev, mutant="subtract"), v, b))
    print("worst error / bound of the two scans: %.3f now, %.1f with the subtraction" % (now, old))
    assert now <= 1.0 < 10.0 < old


# ---- mutants of the block primitives (CPU emulation) ------------------------------------------------------------------------
def test_a_dropped_chunk_element_breaks_the_integer_equality():
    for entry in ("integ_op", "integ_adj"):
        case = hc.Case(entry, 257, 257, 0, None)
        ref = hc.reference(case, "integer")
        rev = entry == "integ_adj"
        assert bits_equal(hc.emu_block_cumsum(ref["inputs"]["x"], rev), ref["outs"]["out"][0])
        assert not bits_equal(hc.emu_block_cumsum(ref["inputs"]["x"], rev, mutant="drop_last"), ref["outs"]["out"][0])


def test_a_tap_range_one_short_breaks_the_integer_equality():
    for n, K in ((257, 257), (257, 258), (2, 3), (63, 1)):
        case = hc.Case("conv", n, n, K, None)
        ref = hc.reference(case, "integer")
        x, k = ref["inputs"]["x"], ref["inputs"]["taps"]
        assert bits_equal(hc.emu_block_conv(k, x, n), ref["outs"]["out"][0])
        assert not bits_equal(hc.emu_block_conv(k, x, n, mutant="m1_short"), ref["outs"]["out"][0])


# ---- Lipschitz constants, inf_norm --------------------------------------------------------------------------------------
@needs_longdouble
def test_gram_reference_is_the_dense_norm():
    for K, N in ((1, 1), (3, 2), (2, 2), (65, 65), (66, 65), (30, 120), (12, 40), (40, 12)):
        taps = hc.gram_taps(K, N)
        want = np.array([orc.gram_lipschitz(t, N) for t in taps])
        got = hc.gram_reference(taps, N).astype(np.float64)
        np.testing.assert_allclose(got, want, rtol=1e-12)
    lim = hc.gram_taps(hc.LIMIT_K, hc.GRAM_LIMIT_N)
    assert (lim[1] == 2.0 * lim[0]).all()
    both = hc.gram_reference(np.stack([lim[0, :8], 2.0 * lim[0, :8]]), 40)
    assert both[1] == 4 * both[0]                                       # (what the limit rows rely on)
    assert {(K <= N and K <= 1024) for K, N in hc.GRAM_CASES + hc.GRAM_LIMIT_CASES} == {True, False}
    for want in ((1024, 1100), (1025, 1100), (1, 1), (3, 2)) + tuple((N + d, N) for N in (2, 65, 257) for d in (0, 1)):
        assert want in hc.GRAM_CASES
    assert hc.GRAM_LIMIT_CASES == ((2000, 19992), (30, 19992))


@needs_longdouble
def test_spectral_references():
    cases = hc.spectral_cases()
    assert {(c.N, c.nb_iter) for c in cases} == {(N, it) for N in (1, 2, 65, 257, 513) for it in (0, 2, 30)}
    for N in (1, 2, 65, 257, 513):
        assert {c.K for c in cases if c.N == N} == {1, N, N + 3}
    stops = set()
    for c in cases:
        ref = hc.spectral_reference(c)
        assert ref["tol"] > 0
        for r, norms in enumerate(ref["traces"]):
            rho, steps = hc.power_result(norms, ref["tol"])
            assert steps == ref["steps"][r] and rho == ref["rho"][r]
            for i in range(1, steps + 1):                     # the criterion of every iteration the loop evaluates
                d = abs(norms[i] - norms[i - 1])
                assert abs(d - ref["tol"]) >= hc.TOL_MARGIN * ref["tol"], (c, r, i)
            stops.add((c.nb_iter, int(steps)))
            if c.N <= 65:
                H = orc.DenseH(ref["taps"][r], c.N)
                want = orc.spectral_radius_est(H, ref["x0"][r], nb_iter=c.nb_iter, tol=ref["tol"])
                assert abs(float(rho) - want) <= hc.RHO_RTOL * want, (c, r)
    assert any(it == 30 and 2 < s < 30 for it, s in stops)     # (the stop fires inside the loop, not only at its ends)


def test_inf_norm_reference():
    assert hc.INF_NORM_N == (1, 255, 256, 257, 100003)
    for n in hc.INF_NORM_N:
        x = hc.inf_norm_inputs(n)
        assert (x[1] == 0).all()
        assert bits_equal(hc.inf_norm_reference(x), orc.inf_norm(x, axis=1))


# ---- the LDS formulas are the library's ---------------------------------------------------------------------------------
def _empty_call(lib, entry, n, K):
    """The entry point on an empty batch (V = 0: sizes are checked, nothing is launched)."""
    fn = getattr(lib, hc.ENTRY_POINT[entry])
    if entry in hc.INTEG:
        return fn(None, n, None, n, 0, n, None)
    if entry in hc.RECT_ENTRIES:
        return fn(None, n, None, n, 0, n, n, None, K, None)
    if entry == "outputs":
        return fn(None, n, 0, n, None, K, None, n, None, n, None)
    if entry == "outputs_pp":
        return fn(None, n, 0, n, None, K, K, None, n, None, n, None)
    if entry.startswith("stats"):
        return fn(None, n, None, n, 1, 0, n, None, K, None, None, None)
    if entry.startswith("lambda_max"):
        return fn(None, n, 0, n, None, K, None, None)
    if entry.startswith("hrf_cost"):
        return fn(None, n, None, n, 0, n, None, K, 1, None, None)
    if entry == "spectral_radius_pp":
        return fn(None, n, 0, n, None, K, K, 2, 1e-6, None, None)
    if entry == "gram_frobenius":
        return fn(None, K, 0, K, n, None, None)
    raise KeyError(entry)


def test_lds_limits_match_the_library(lib):
    want = {"integ_op": 9996, "conv": 9981, "outputs": 9981, "stats": 9981, "lambda_max": 9981, "hrf_cost": 19962,
            "spectral_radius_pp": 6654, "gram_frobenius": 19992}
    for entry in hc.ROW_ENTRIES + ("spectral_radius_pp", "gram_frobenius"):
        n, K = hc.limit_shape(entry)
        if entry in want:
            assert n == want[entry], entry
        assert hc.lds_doubles(entry, n, K) <= hc.LDS_DOUBLES_MAX < hc.lds_doubles(entry, n + 1, K)
        assert _empty_call(lib, entry, n, K) == 0, (entry, lib.pb_last_error())
        n1, _ = hc.over_shape(entry)
        assert n1 == n + 1
        assert _empty_call(lib, entry, n1, K) != 0, entry
        assert b"exceeds LDS" in lib.pb_last_error(), (entry, lib.pb_last_error())
    # pb_spectral_radius has no batch argument and checks its pointers first: the error side only, on pointers never read
    fake = ctypes.c_void_p(4096)
    n1, K = hc.over_shape("spectral_radius")
    assert lib.pb_spectral_radius(fake, n1, fake, K, 2, 1e-6, fake, None) != 0
    assert b"exceeds LDS" in lib.pb_last_error()
    assert hc.GRAM_LIMIT_N == hc.limit_shape("gram_frobenius")[0]


# ---- completeness ------------------------------------------------------------------------------------------------------
def test_case_list_is_complete():
    named = ("pb_fista_outputs", "pb_fista_outputs_pp", "pb_fista_stats", "pb_fista_stats_d", "pb_hrf_cost", "pb_hrf_cost_d",
             "pb_hrf_cost_pv", "pb_hrf_cost_pv_d", "pb_lambda_max", "pb_lambda_max_d", "pb_spectral_radius",
             "pb_spectral_radius_pp", "pb_gram_frobenius", "pb_integ_op", "pb_integ_adj", "pb_conv", "pb_corr", "pb_op_forward",
             "pb_op_adjoint", "pb_inf_norm")
    grouped = [e for g in hc.GROUPS.values() for e in g]
    assert sorted(hc.ENTRY_POINT[e] for e in grouped) == sorted(named)
    from pybold_amd import _lib
    for name in named:
        assert name in _lib.SIGNATURES, name
    assert hc.EDGE_N == (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000)
    for entry in hc.ROW_ENTRIES:
        mine = [c for c in ALL_ROW_CASES if c.entry == entry]
        assert {c.n_in for c in mine if c.n_in == c.n_out} == set(hc.EDGE_N), entry
        if entry in hc.RECT_ENTRIES:
            for n_in, n_out in ((1, 300), (300, 1), (255, 257), (257, 255), (513, 100), (100, 513)):
                assert {c.K for c in mine if (c.n_in, c.n_out) == (n_in, n_out)} == {1, 30, max(n_in, n_out) + 1}
    for n in hc.EDGE_N:
        ks = hc.tap_counts(n)
        assert 1 <= len(ks) <= 4 and len(set(ks)) == len(ks) and min(ks) >= 1
        assert set(ks) <= {1, 2, n - 1, n, n + 1, 2 * n, 30, 127}
        if n >= 2:
            assert n in ks and n + 1 in ks
    assert {k for n in hc.EDGE_N for k in hc.tap_counts(n)} >= {1, 2, 30, 127}
    for f32 in hc.F32_Y:                                   # both y types
        assert f32 in hc.ROW_ENTRIES and f32 + "_d" in hc.ROW_ENTRIES
        a = hc.make_inputs(hc.Case(f32, 5, 5, 2, 1), "integer", 3, M=3)
        b = hc.make_inputs(hc.Case(f32 + "_d", 5, 5, 2, 1), "integer", 3, M=3)
        assert a["y"].dtype == np.float32 and b["y"].dtype == np.float64
    assert {c.opt for c in ALL_ROW_CASES if c.entry == "outputs"} == {"z", "x", "zx"}
    assert {c.opt for c in ALL_ROW_CASES if c.entry == "stats"} == {1, 2}
    assert {c.opt for c in ALL_ROW_CASES if c.entry == "hrf_cost"} == {1, 3}
