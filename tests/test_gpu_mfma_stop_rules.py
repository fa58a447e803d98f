"""The stop rules of the matrix-pipe kernels -- `fista_mfma_kernel`, `fista_mfma2_kernel`, `fista_mfma4_kernel` -- at the edges of
every compiled rule instance, row by row (tests/stop_rule_cases.py): each instance at the masked corner (the smallest series
of its block count with the fewest taps) and the full corner (the longest with the most taps a pinned call accepts), under
the _loops_deconv rule (evaluated in full inside the kernel) and the window rule (wind = 6, a no-fire certificate with an
exact re-solve of the rows it flags).

The inputs stay clear of the tolerance (the oracle's criterion is 1 % of tol away from tol at every test) and dense (the
accuracy guard has no reason to hand a row back), so EVERY row must stop where the float64 oracle does, and every row's
iterate is compared with the C oracle's after that row's own number of iterations (1e-5; cost traces 3e-5).  The pins that
do not re-solve show which rows the kernel itself produced; they are the same bits as under the pins that do.

PB_MFMA_STOP_RULES_REPORT=<file> appends one line per case: the source of profiles/mfma_stop_rules.txt."""
import functools
import os
import time

import numpy as np
import pytest
import torch

import stop_rule_cases as sc
import table_shapes as ts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from pybold_amd import solver
    assert torch.cuda.is_available()
    return solver


@functools.lru_cache(maxsize=None)
def built(case):
    """Inputs of a case (conditions asserted in stop_rule_cases.check_selection; NoInputs is an error) with the oracle's
    iterates at its own stop iterations, shared by the calls of the case and left unchanged."""
    inp = sc.inputs(case)
    inp["W"] = sc.iterates_at(inp, inp["n_done"])
    for a in (inp["Y"], inp["W"], inp["n_done"]) + (() if inp["W0"] is None else (inp["W0"],)):
        a.setflags(write=False)
    return inp


def _solve(solver, c, force, want_J):
    Y = torch.from_numpy(c["Y"].astype(np.float32)).cuda()
    W0 = None if c["W0"] is None else torch.from_numpy(c["W0"].copy()).cuda()
    W, J, nd = solver.fista_solve(Y, c["taps"].copy(), c["lbda"], c["step"], c["n_iter"], W0=W0, want_J=want_J, stop=c["rule"], tol=c["tol"],
                                  wind=sc.WIND, force=force)
    torch.cuda.synchronize()
    return W.cpu().numpy(), None if J is None else J.cpu().numpy().astype(np.float64), nd.cpu().numpy().astype(np.int64)


def _report(line):
    path = os.environ.get("PB_MFMA_STOP_RULES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("case", sc.cases(), ids=sc.case_id)
def test_stop_rule_at_the_edges_of_an_instance(solver, case):
    t0 = time.time()
    assert ts.mfma_instance(case.form, case.N, case.K) == case.instance and sc.reaches(case.form, case.N, case.K, case.rule)
    c = built(case)
    V, n_iter, ref_nd, fired = len(c["n_done"]), c["n_iter"], c["n_done"], c["fired"]
    resolve, only, cert, certonly = sc.PINS[case.form]
    if case.rule == "loops":
        W, _, nd = _solve(solver, c, resolve, False)
        print("%s N=%d K=%d loops tol=%g n_iter=%d: n_done %s (oracle %s)" % (case.instance, case.N, case.K, c["tol"], n_iter, nd.tolist(),
                                                                              ref_nd.tolist()))
        verdict = sc.judge(c, W, nd)
        # the kernel itself, not the re-solve, produced the judged rows
        W1, _, nd1 = _solve(solver, c, only, False)
        kept = nd1 >= 0
        print("   %d of %d rows kept without the re-solve; worst row %.3e" % (kept.sum(), V, verdict.err))
        assert 3 * kept.sum() >= 2 * V, nd1
        assert (kept & ~fired).any() and len(set(ref_nd[kept & fired].tolist())) >= 3, nd1
        assert (nd1[kept] == nd[kept]).all() and np.array_equal(W1[kept], W[kept])
        # ... on the matrix pipe: the vector forms round otherwise
        Wv, _, _ = _solve(solver, c, "valu", False)
        assert not np.array_equal(Wv[kept], W[kept])
    else:
        W, J, nd = _solve(solver, c, cert, True)
        print("%s N=%d K=%d window tol=%g n_iter=%d: n_done %s (oracle %s)" % (case.instance, case.N, case.K, c["tol"], n_iter, nd.tolist(),
                                                                               ref_nd.tolist()))
        verdict = sc.judge(c, W, nd, J)
        # soundness of the certificate alone: every row whose rule fires is flagged; a row it clears ran every iteration
        W1, J1, nd1 = _solve(solver, c, certonly, True)
        flagged = nd1 == -1
        kept = ~flagged
        assert flagged[fired].all(), (nd1, ref_nd)
        assert (nd1[kept] == n_iter).all(), (nd1, ref_nd)
        if kept.any():
            rows = np.flatnonzero(kept)
            err = np.linalg.norm(W1[rows] - c["W"][rows], axis=1) / np.linalg.norm(c["W"][rows], axis=1)
            assert err.max() < sc.EPS, err
            np.testing.assert_allclose(J1[rows], sc.trace(c)[rows], rtol=sc.RTOL_J)
            assert np.array_equal(W1[rows], W[rows])
        print("   the certificate cleared %d of %d rows that never fire; worst row %.3e, trace %.3e" % (kept.sum(), (~fired).sum(),
                                                                                                       verdict.err, verdict.jerr))
    assert verdict.differed == 0
    _report("%-16s %4d x %2d  %-6s tol %-5g budget %3d  firing iterations %2d  kept %2d / %d  row %.2e  trace %s  %.2f s" % (
        case.instance, case.N, case.K, case.rule, c["tol"], n_iter, len(set(ref_nd[fired].tolist())), kept.sum(), V, verdict.err,
        "   -    " if verdict.jerr is None else "%.2e" % verdict.jerr, time.time() - t0))
