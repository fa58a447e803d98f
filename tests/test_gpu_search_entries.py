"""Every device-resident lambda search at the edges of its instance, row by row.

The search of `deconv(lbda=None)` is compiled once per line of exact_table.inc, exact_split_table.inc, exact_long_table.inc
and exact_split_long_table.inc, with the taps on the host and with one HRF per voxel, with STOP == 2 and STOP == 0: 24
kernels behind the eight `solver.auto_lbda_solve*` entry points.  tests/search_cases.py lists their edge shapes -- the last
length of an instance, where no sample of the last strip is masked, and its first, where the last strip or wave holds one
sample (five scans on the first one-wave instance); one tap, all taps, 33 taps -- and draws rows whose stops differ: at the
FIRE budget (40, 30, 1e-1) the alpha window fires at different outer iterations, on one row never, and every inner solve stops
on its window rule; at the QUIET budget (12, 20, 1e-6) nothing fires; OFF is `early_stopping=False` at (8, 40), the STOP == 0
kernels.  One row of every case drives lambda negative.  No criterion of any row comes closer to the tolerance than 1e-4 of
it, and |alpha| stays above 1e-2 (tests/test_search_cases_host.py), so every count is compared exactly and every value to
1e-9, the bound of tests/test_gpu_auto_lbda_device.py::test_shapes_against_the_oracle.

On every row: n_outer and n_inner equal the float64 reference's; alpha, lbda, W and the first n_outer entries of R, G, J are
within 1e-9 of it; the traces are NaN from n_outer on; W is finite.  At the full corners a second FIRE call in launches of
three outer iterations (rows that are done share a workgroup with rows that are not) is bit-equal to the first, and a warm
QUIET call is held to the reference's warm run.  The 48-tap forms at one tap return the bits of the 32-tap forms.

PB_SEARCH_ENTRIES_REPORT=<file> appends one JSON line per case (profiles/search_entries.txt is made from it)."""
import json
import os
import time

import numpy as np
import pytest
import torch

import search_cases as sc

pytestmark = pytest.mark.gpu

EPS = 1.0e-9
OUTPUTS = ("W", "alpha", "lbda", "n_outer", "n_inner", "R", "G", "J")


@pytest.fixture(scope="module")
def solver():
    from pybold_amd import solver
    assert torch.cuda.is_available()
    return solver


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()          # (a copy: the cases' arrays are read-only)


def _report(**kw):
    path = os.environ.get("PB_SEARCH_ENTRIES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(kw) + "\n")


def _call(solver, form, pp, d, budget, W0=None, outer_chunk=0):
    """One call of the form's entry point on the rows of a case: the outputs as NumPy arrays, the seconds it took, and the
    warm start's device tensor with the returned iterate's (for the aliasing check)."""
    nb_iter, nb_sub_iter, tol, early = sc.BUDGETS[budget]
    f = sc.FORMS[form]
    fn = getattr(solver, f.entry_pp if pp else f.entry)
    Y, sigma = dev(d["Y"]), dev(d["sigma"])
    taps, steps = (dev(d["taps"]), dev(d["steps"])) if pp else (d["taps"], float(d["steps"][0]))
    W0d = None if W0 is None else dev(W0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    W, res = fn(Y, taps, steps, sigma, early_stopping=early, tol=tol, nb_iter=nb_iter, nb_sub_iter=nb_sub_iter, W0=W0d,
                outer_chunk=outer_chunk)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    out = {k: res[k].cpu().numpy() for k in OUTPUTS[1:]}
    out["W"] = W.cpu().numpy()
    return out, seconds, (W0d, W)


def rel(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def _against(out, runs, nb_iter, what):
    """Every row of a call against its reference run; returns the worst relative error."""
    worst = 0.0
    assert out["W"].shape[0] == len(runs) and out["R"].shape == out["G"].shape == out["J"].shape == (len(runs), nb_iter)
    for v, run in enumerate(runs):
        n = run.n_outer
        assert int(out["n_outer"][v]) == n, "%s row %d: n_outer %d, the reference %d" % (what, v, int(out["n_outer"][v]), n)
        assert int(out["n_inner"][v]) == run.n_inner, "%s row %d: n_inner %d, the reference %d" % (what, v, int(out["n_inner"][v]),
                                                                                                 run.n_inner)
        assert np.isfinite(out["W"][v]).all(), "%s row %d: W is not finite" % (what, v)
        errs = {"alpha": rel(out["alpha"][v], run.alpha[-1]), "lbda": rel(out["lbda"][v], run.lbda), "W": rel(out["W"][v], run.W)}
        for k, want in (("R", run.R), ("G", run.G), ("J", run.J)):
            assert not np.isnan(out[k][v, :n]).any() and np.isnan(out[k][v, n:]).all(), "%s row %d: NaN padding of %s" % (what, v, k)
            errs[k] = rel(out[k][v, :n], want)
        bad = {k: e for k, e in errs.items() if not e < EPS}
        assert not bad, "%s row %d (n_outer %d, n_inner %d): %s" % (what, v, n, run.n_inner, bad)
        worst = max(worst, max(errs.values()))
    return worst


def _same_bits(a, b, what):
    for k in OUTPUTS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s: %s differs in %d entries" % (
            what, k, int((x.view(np.uint8) != y.view(np.uint8)).sum()))


@pytest.mark.parametrize("c,budget", [pytest.param(c, b, id=sc.case_id(c, b)) for c in sc.cases() for b in sc.BUDGETS])
def test_search_entry(solver, c, budget):
    d = sc.case(c)
    name = sc.case_id(c, budget)
    if d["N"] != c.N:
        print("   no draw of %d scans meets the conditions of a search case: %d scans" % (c.N, d["N"]))
    nb_iter, nb_sub_iter, tol, early = sc.BUDGETS[budget]
    runs = d["ref"][budget]
    out, seconds, _ = _call(solver, c.form, c.pp, d, budget)
    print("%s N=%d: n_outer %s (reference %s) n_inner %s (reference %s)" % (
        name, d["N"], out["n_outer"].tolist(), [r.n_outer for r in runs], out["n_inner"].tolist(), [r.n_inner for r in runs]))
    worst = _against(out, runs, nb_iter, name)
    print("   worst rel. error %.2e, %.3f s" % (worst, seconds))
    if budget == "OFF":
        assert (out["n_outer"] == nb_iter).all() and (out["n_inner"] == (nb_iter + 1) * nb_sub_iter).all()
    extra = {}
    if c.corner == "full" and budget == "FIRE":
        # launch boundaries between the rows' stops: rows that are done share a workgroup with rows that are not
        chunked, s, _ = _call(solver, c.form, c.pp, d, budget, outer_chunk=3)
        seconds += s
        _same_bits(chunked, out, name + " outer_chunk=3")
        extra["chunked"] = "bit-equal"
    if c.corner == "full" and budget == "QUIET":
        warm, s, (W0d, Wd) = _call(solver, c.form, c.pp, d, budget, W0=d["W0"])
        seconds += s
        extra["warm"] = _against(warm, d["ref"]["WARM"], nb_iter, name + " warm")
        assert torch.equal(W0d, dev(d["W0"])), "warm start modified"
        assert Wd.data_ptr() != W0d.data_ptr(), "the iterate aliases the warm start"
        assert not np.array_equal(warm["W"], out["W"])
        print("   warm start: worst rel. error %.2e" % extra["warm"])
    short = sc.FORMS[c.form].short
    if short is not None and c.K == 1:
        # "with K <= 32 the same bits": the 32-tap entry point of the same lengths on the same inputs
        same, s, _ = _call(solver, short, c.pp, d, budget)
        seconds += s
        _same_bits(out, same, name + " against " + (sc.FORMS[short].entry_pp if c.pp else sc.FORMS[short].entry))
        extra["short_form"] = "bit-equal"
    f = sc.FORMS[c.form]
    _report(entry_point=f.entry_pp if c.pp else f.entry, table=f.table, instance=list(c.entry), corner=c.corner, N=d["N"], N_asked=c.N,
            K=c.K, budget=budget, worst=worst, n_outer=out["n_outer"].tolist(), n_inner=out["n_inner"].tolist(),
            negative_row=d["negative"], seconds=seconds, **extra)
