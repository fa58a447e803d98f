"""Every line of the four kernel tables (fast_table.inc, wide_table.inc, exact_table.inc, exact_split_table.inc), every
family of kernels a line compiles (csrc/launch_fast.h, fista_pair.h, fista_pair_ffa.h, fista_exact*.h) and every variant of
a family -- cold / warm start, cost trace, the _loops_deconv rule, the window rule at wind 4, 6 and 8 -- run at the edge
shapes of the entry's region (tests/table_shapes.py): the full corner (largest N, K = KT: no masked sample in the last
strip, no zero-padded tap) and the masked corner (smallest N, smallest K).  Each case is a small solve against the float64
oracle: oracle/c_oracle.py for iterates and cost traces, oracle/pybold_oracle.py for the stop rules.

Batches end in a partial block: 37 problems on the 16-lane forms (a lone problem in the last row of the pair forms), 5
on the forms with one problem per wave, 3 on the four-wave form.  Bounds are the project's: 1e-5 per row on the
float32-storage forms and 3e-5 on their cost traces (tests/test_gpu_parity.py, tests/test_gpu_mfma.py), 1e-10 on the float64
forms (tests/test_gpu_round2.py).  The stop-rule inputs are drawn such that the oracle's criterion stays 1 % of tol away
from tol on every row (table_shapes.stop_rule_inputs): n_done must equal the oracle's on every row.  The certificate
families take table_shapes.certificate_inputs (warm rows that fire at once, cold rows far from firing): `certonly` must flag
the firing rows and only those, `cert2` must equal the oracle on all rows.

Which form a pinned call runs is table_shapes.forced_form / forced_form_pp (tests/test_table_shapes_host.py); where a pin
cannot reach a compiled family at a shape the case is skipped with the reason (none is, as the tables stand: the
per-problem-taps cases of the wide table take their corners from the part of a region that route_pp() hands to that form,
table_shapes.edge_shapes_pp_wide).  A stop-rule case at a corner of one scan runs at the next length that can meet the
conditions on its inputs (2 or 3 scans; 64 or 96 for the certificate); the case prints the length used.  PB_TABLE_ENTRIES_REPORT=<file> appends one
JSON line per case (family, errors, seconds): the source of profiles/table_entries.txt."""
import functools
import json
import os
import time

import numpy as np
import pytest
import torch

import table_shapes as ts
from oracle import c_oracle
from oracle import pybold_oracle as orc

pytestmark = pytest.mark.gpu

EPS = {False: 1.0e-5, True: 1.0e-10}            # relative row error: float32-storage forms, float64 forms
RTOL_J = {False: 3.0e-5, True: 1.0e-10}
V16, VWAVE, VSPLIT = 37, 5, 3
N_ITER = 60
LBDA = 0.5

PLAIN = ("cold", "warm", "J")
LOOPS = ("loops", "loopsJ")


def _windows(winds):
    return tuple("win%d%s" % (w, j) for w in winds for j in ("", "J"))


# family -> (table, problems, float64, variants, needs the pair forms)
FAMILIES = {
    "single_row": ("fast", V16, False, PLAIN + LOOPS + _windows(ts.WINDS), False),
    "one_per_wave": ("wide", VWAVE, False, PLAIN + LOOPS + _windows(ts.WINDS), False),
    "pp_single_row": ("fast", V16, False, ("warm", "loops"), False),
    "pp_one_per_wave": ("wide", VWAVE, False, ("warm", "loops"), False),
    "pair_ffa": ("fast", V16, False, PLAIN, True),
    "pair_direct": ("fast", V16, False, ("cold", "J"), True),
    "pair_cert": ("fast", V16, False, ("win6", "win6J"), True),
    "pair_dev": ("fast", V16, False, ("cold", "warm"), True),
    "pair_split": ("fast", V16, False, ("cold", "J", "win6"), True),
    "f64_one_wave": ("exact", VWAVE, True, PLAIN + LOOPS + _windows((6,)), False),
    "f64_four_waves": ("exact_split", VSPLIT, True, PLAIN + LOOPS + _windows((6,)), False),
    "f64_pp": ("exact", VWAVE, True, PLAIN + LOOPS + _windows((6,)), False),
}


def _cases():
    out = []
    for family, (table, V, f64, variants, pair) in FAMILIES.items():
        for entry in ts.entries(table):
            if pair and not ts.has_pair(entry):
                continue
            if family == "pair_split":
                shapes = ts.split_edge_shapes(entry)
            elif family == "pp_one_per_wave":
                shapes = ts.edge_shapes_pp_wide(entry, V)      # (the corners of what route_pp() hands to this form)
            else:
                shapes = ts.edge_shapes(table, entry)
            for corner, N, K in shapes:
                for variant in variants:
                    if variant.startswith("win") and not ts.ring_fits(entry[0], "window", int(variant[3]), f64):
                        continue                   # (not compiled: no increment ring beyond 20 samples per lane)
                    out.append(pytest.param(family, entry, N, K, variant,
                                            id="%s-%s_%d_%d-%s_%dx%d-%s" % (family, table, entry[0], entry[1], corner, N, K, variant)))
    return out


def rel_rows(a, b):
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    return float((np.linalg.norm(a - b, axis=1) / (np.linalg.norm(b, axis=1) + 1e-300)).max())


def dev(a, f64=True):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64 if f64 else np.float32)).cuda()


def _variant(variant):
    """(stop, wind, cost trace, warm)"""
    if variant.startswith("win"):
        return "window", int(variant[3]), variant.endswith("J"), False
    if variant.startswith("loops"):
        return "loops", 6, variant.endswith("J"), False
    return None, 6, variant == "J", variant == "warm"


def _pp_taps(rng, base, N, V, independent):
    """One HRF and one step per problem.  Short series: independent draws, each with its own spectral norm; longer ones:
    the base HRF under a different gain and sign per row (the spectral norm scales with the gain: exact steps for one
    decomposition)."""
    if independent and N <= 320:
        taps = 0.3 * rng.randn(V, len(base))
        return taps, np.array([1.0 / ts.lipschitz(t, N) for t in taps])
    return ts.scaled_taps(base, ts.lipschitz(base, N), V)


@functools.lru_cache(maxsize=None)
def plain_case(N, K, V, f64, pp):
    """Inputs and oracle results of the variants without a stop rule, shared by the families: cold start with one lambda,
    warm start with one lambda per problem; iterate and cost trace after N_ITER iterations."""
    rng = np.random.RandomState(7919 * N + 31 * K + V + (1 << 20) * f64 + (1 << 21) * pp)
    base = 0.3 * rng.randn(K)
    Y = rng.randn(V, N)
    if not f64:
        Y = Y.astype(np.float32).astype(np.float64)
    lam = LBDA * (0.5 + rng.rand(V))
    W0 = 0.01 * rng.randn(V, N)
    if pp:
        taps, steps = _pp_taps(rng, base, N, V, True)
        out = {}
        for name, lb, w0 in (("cold", np.full(V, LBDA), None), ("warm", lam, W0)):
            res = [c_oracle.fista_batch(Y[v:v + 1], taps[v], float(lb[v]), float(steps[v]), N_ITER,
                                        W0=None if w0 is None else w0[v:v + 1], want_J=True, threads=1) for v in range(V)]
            out[name] = (np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res]))
    else:
        taps, steps = base, 1.0 / ts.lipschitz(base, N)
        out = {"cold": c_oracle.fista_batch(Y, taps, LBDA, steps, N_ITER, want_J=True, threads=4)[:2],
               "warm": c_oracle.fista_batch(Y, taps, lam, steps, N_ITER, W0=W0, want_J=True, threads=4)[:2]}
    for a in (Y, W0, lam):
        a.setflags(write=False)
    return dict(Y=Y, taps=taps, steps=steps, lam=lam, W0=W0, ref=out)


@functools.lru_cache(maxsize=None)
def stop_case(table, entry, split, N, K, V, f64, pp, rule, wind, certificate=False):
    """Inputs of a stop-rule case (table_shapes.stop_rule_inputs: conditions checked there) with the oracle's iterate,
    stop iteration and cost trace: orc.loops_batch / orc.deconv_fixed_lbda row by row; the trace from the C oracle."""
    inp = ts.stop_rule_inputs_near(table, entry, N, K, V, rule, split=split, wind=wind, seed=1 + f64 + 2 * pp, float32=not f64,
                                   per_problem_taps=pp, n_iter=N_ITER, certificate=certificate)
    Y, n_iter, tol = inp["Y"], inp["n_iter"], inp["tol"]
    taps2 = np.broadcast_to(inp["taps"], (V, K)) if inp["taps"].ndim == 1 else inp["taps"]
    steps = np.broadcast_to(np.asarray(inp["steps"], dtype=np.float64), (V,))
    W, nd, J = np.empty_like(Y), np.empty(V, dtype=np.int64), np.empty((V, n_iter))
    W0 = inp.get("W0")
    for v in range(V):
        if rule == "loops":
            w, n = orc.loops_batch(Y[v:v + 1], taps2[v], inp["lbda"], steps[v], n_iter, tol)
            W[v], nd[v] = w[0], n[0]
        else:
            o = orc.deconv_fixed_lbda(Y[v], taps2[v], inp["lbda"], nb_iter=n_iter, tol=tol, wind=wind, lipschitz=1.0 / steps[v],
                                      dense=False, w0=None if W0 is None else W0[v])
            W[v], nd[v] = o[2], o[4]
        J[v] = c_oracle.fista_batch(Y[v:v + 1], taps2[v], inp["lbda"], float(steps[v]), n_iter, want_J=True, threads=1,
                                    W0=None if W0 is None else W0[v:v + 1])[1][0]
    # the selection's own recurrence and the oracle agree on where every row stops
    assert (nd == inp["n_done"]).all(), (nd, inp["n_done"])
    fired = nd < n_iter
    assert fired.sum() * 3 >= V and len(set(nd[fired])) >= 2 and (~fired).any(), nd
    return dict(inp, W=W, nd=nd, J=J, W0=W0)


def _report(**kw):
    path = os.environ.get("PB_TABLE_ENTRIES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(kw) + "\n")


def _solve(solver, family, c, lbda, n_iter, W0, want_J, stop, tol, wind, force=None):
    """One call of the family's entry point: (W, J or None, n_done) as NumPy arrays."""
    f64 = FAMILIES[family][2]
    Y = dev(c["Y"], f64)
    W0d = None if W0 is None else dev(W0)
    taps, steps = c["taps"], c["steps"]
    if family in ("pp_single_row", "pp_one_per_wave", "pair_dev"):
        td = dev(taps)
        sd = dev(np.atleast_1d(steps))
        force = force or {"pp_single_row": "fast1", "pp_one_per_wave": "fast", "pair_dev": "fast2"}[family]
        W, nd = solver.fista_solve_pp(Y, td, sd, lbda, n_iter, W0=W0d, stop=stop, tol=tol, force=force)
        J = None
    elif family == "f64_pp":
        W, J, nd = solver.fista_solve_pp_d(Y, dev(taps), dev(steps), lbda, n_iter, W0=W0d, want_J=want_J, stop=stop, tol=tol,
                                           wind=wind, force="fast")
    else:
        force = force or {"single_row": "fast1", "one_per_wave": "wide", "pair_ffa": "fast2", "pair_direct": "fast2d",
                          "pair_split": "fast2", "f64_one_wave": "fast", "f64_four_waves": None}[family]
        W, J, nd = solver.fista_solve(Y, taps, lbda, float(steps), n_iter, W0=W0d, want_J=want_J, stop=stop, tol=tol, wind=wind,
                                      force=force)
    torch.cuda.synchronize()
    if W0 is not None:
        assert torch.equal(W0d, dev(W0)), "warm start modified"
    return W.cpu().numpy(), None if J is None else J.cpu().numpy().astype(np.float64), nd.cpu().numpy()


def _reaches(solver, family, entry, N, K, V, stop, wind):
    """None when the family's pin runs the entry's kernel of that family at this shape, else the reason."""
    if family == "f64_four_waves":
        name = solver.which_kernel_f64(N, K, stop=stop, wind=wind)
        return None if name == solver.KERNEL_NAMES[8] else "the dispatch runs %s" % name
    if family in ("f64_one_wave", "f64_pp"):
        return None                                     # (force="fast": that form or an error)
    if family in ("pp_single_row", "pp_one_per_wave", "pair_dev"):
        want = {"pp_single_row": ts.SINGLE_ROW, "pp_one_per_wave": ts.WIDE, "pair_dev": ts.PAIR}[family]
        force = {"pp_single_row": "fast1", "pp_one_per_wave": "fast", "pair_dev": "fast2"}[family]
        form, e, why = ts.forced_form_pp(N, K, V, family == "pair_dev", stop, force)
    else:
        want = {"single_row": ts.SINGLE_ROW, "one_per_wave": ts.WIDE, "pair_split": ts.PAIR + " split"}.get(family, ts.PAIR)
        force = {"single_row": "fast1", "one_per_wave": "wide", "pair_direct": "fast2d", "pair_cert": "cert2"}.get(family, "fast2")
        if family == "pair_split" and stop == "window":
            force = "cert2"
        form, e, why = ts.forced_form(N, K, V, stop, wind, force)
    if form == want and e == entry:
        return None
    return "force=%r runs the %s form of %s here%s" % (force, form, e, (": " + why) if why else "")


@pytest.fixture(scope="module")
def solver():
    from pybold_amd import solver
    assert torch.cuda.is_available()
    return solver


@pytest.mark.parametrize("family,entry,N,K,variant", _cases())
def test_table_entry(solver, family, entry, N, K, variant):
    table, V, f64, _, _ = FAMILIES[family]
    stop, wind, want_J, warm = _variant(variant)
    pp = family in ("pp_single_row", "pp_one_per_wave", "f64_pp")
    why = _reaches(solver, family, entry, N, K, V, stop, wind)
    if why:
        print("SKIP %s %s (%d, %d) N=%d K=%d %s: %s" % (family, table, entry[0], entry[1], N, K, variant, why))
        _report(family=family, table=table, entry=entry, N=N, K=K, variant=variant, skipped=why)
        pytest.skip(why)
    t0 = time.time()
    eps, rtol = EPS[f64], RTOL_J[f64]
    jerr = None
    if stop is None:
        c = plain_case(N, K, V, f64, pp)
        Wr, Jr = c["ref"]["warm" if warm else "cold"]
        W, J, nd = _solve(solver, family, c, c["lam"] if warm else LBDA, N_ITER, c["W0"] if warm else None, want_J, None, 0.0, 6)
        err = rel_rows(W, Wr)
        print("%s %s N=%d K=%d %s: iterate %.3e" % (family, entry, N, K, variant, err))
        assert (nd == N_ITER).all(), nd
        assert err < eps, err
        if want_J:
            assert J is not None, "no cost trace returned"
            jerr = float(np.abs(J / Jr - 1.0).max())
            print("   cost trace %.3e" % jerr)
            np.testing.assert_allclose(J, Jr, rtol=rtol)
    else:
        cert = family == "pair_cert" or (family == "pair_split" and stop == "window")
        c = stop_case(table, entry, family == "pair_split", N, K, V, f64, pp, "loops" if stop == "loops" else "window", wind, cert)
        if c["N"] != N:
            print("   no batch of %d scans meets the conditions of a stop-rule case: %d scans" % (N, c["N"]))
            N = c["N"]
        Wr, ndr, Jr, n_iter = c["W"], c["nd"], c["J"], c["n_iter"]
        if cert:
            # the certificate's own verdict (fista_pair_ffa.h: "a problem whose certificate fails at some iteration (the rule
            # may or may not have fired) is flagged"): every row whose rule fires comes back flagged, n_done = -1; a row it
            # clears ran every iteration and holds the oracle's iterate
            W1, _, nd1 = _solve(solver, family, c, c["lbda"], n_iter, c["W0"], want_J, stop, c["tol"], wind, force="certonly")
            flagged = nd1 == -1
            assert flagged[ndr < n_iter].all(), (nd1, ndr)
            assert not flagged[ndr >= n_iter].any(), (nd1, ndr)       # (certificate_inputs: the other rows are far from firing)
            assert (nd1[~flagged] == n_iter).all(), (nd1, ndr)
            if (~flagged).any():
                assert rel_rows(W1[~flagged], Wr[~flagged]) < eps
            print("   certificate flagged %d of %d rows, %d fire" % (flagged.sum(), V, (ndr < n_iter).sum()))
            force = "cert2"
        else:
            force = None
        W, J, nd = _solve(solver, family, c, c["lbda"], n_iter, c["W0"], want_J, stop, c["tol"], wind, force=force)
        live = np.linalg.norm(Wr, axis=1) > 0
        err = rel_rows(W[live], Wr[live]) if live.any() else 0.0
        print("%s %s N=%d K=%d %s tol=%g n_iter=%d: n_done %s (oracle %s) iterate %.3e" % (family, entry, N, K, variant, c["tol"], n_iter,
                                                                                          nd.tolist(), ndr.tolist(), err))
        assert (nd == ndr).all(), (nd, ndr)
        assert err < eps, err
        assert np.abs(W[~live]).max(initial=0.0) == 0.0
        if want_J:
            assert J is not None, "no cost trace returned"
            jerr = 0.0
            for v in range(V):
                jerr = max(jerr, float(np.abs(J[v, :nd[v]] / Jr[v, :nd[v]] - 1.0).max()))
            print("   cost trace %.3e" % jerr)
            for v in range(V):
                np.testing.assert_allclose(J[v, :nd[v]], Jr[v, :nd[v]], rtol=rtol)
                assert np.isnan(J[v, nd[v]:]).all(), v           # nothing written past a row's last iteration
    _report(family=family, table=table, entry=entry, N=N, K=K, variant=variant, err=err, jerr=jerr, seconds=time.time() - t0)
