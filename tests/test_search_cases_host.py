"""CPU-only checks of tests/search_cases.py, the helper behind tests/test_gpu_search_entries.py: the enumeration yields the
instances of the four float64 tables and nothing else, every case's shape is one its form's search accepts, the rows of every
case meet the conditions that make its stop decisions testable, and the restated search agrees with both float64 oracles on
every row at every budget.  No kernel is launched."""
import glob
import os
import re

import numpy as np
import pytest

import search_cases as sc
import table_shapes as ts
from oracle import c_oracle
from oracle import pybold_oracle as orc

CASES = sc.cases()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not glob.glob(os.path.join(ts.ROOT, "pybold_amd", "csrc", "build", "auto_*.res")):
        ge.build()
    return _lib.load()


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - b) / (np.linalg.norm(b) + 1e-300))


def test_the_enumeration_is_the_four_tables():
    """Every PB_EXACT* line of the four .inc files is an instance, each with a full and a masked corner at one tap and at
    all its taps (the 48-tap lines at 33 too), for the host-taps and the pp entry point: 60 cases as the tables stand."""
    lines = {}
    for fname in sorted(glob.glob(os.path.join(ts.CSRC, "exact*_table.inc"))):
        found = re.findall(r"^(PB_EXACT\w*)\((\d+), *(\d+)\)", open(fname).read(), flags=re.M)
        assert found, fname
        lines[os.path.basename(fname)] = sorted((int(s), int(kt)) for _, s, kt in found)
    mine = {ts.TABLES[f.table][0]: [e for e, _, _ in sc.instances(f.name)] for f in sc.FORMS.values()}
    assert mine == lines, (mine, lines)
    want = 0
    for form in sc.FORMS:
        for entry, first, last in sc.instances(form):
            n_taps = 3 if entry[1] > 33 else 2
            want += 2 * 2 * n_taps
            got = [c for c in CASES if c.form == form and c.entry == entry]
            assert {(c.corner, c.N) for c in got} == {("full", last), ("masked", first)}, (form, entry)
            assert {c.K for c in got} == ({1, entry[1]} | ({33} if entry[1] > 33 else set()))
            assert {c.pp for c in got} == {False, True} and len(got) == 4 * n_taps
    assert len(CASES) == want == len(set(CASES))
    assert len({sc.case_id(c) for c in CASES}) == len(CASES)
    print("%d cases x %d budgets" % (len(CASES), len(sc.BUDGETS)))
    if {k: v for k, v in lines.items()} == {"exact_table.inc": [(5, 32), (10, 32)], "exact_split_table.inc": [(5, 32)],
                                            "exact_long_table.inc": [(5, 48), (10, 48)], "exact_split_long_table.inc": [(5, 48)]}:
        assert len(CASES) == 60
        assert sorted({c.N for c in CASES}) == [5, 320, 321, 640, 641, 1280]


def test_every_case_is_a_shape_its_search_accepts(lib):
    """pb_auto_lbda*_supported says 1 for every case (at the length asked for and at the length used), the case lands on the
    instance it is named after, and the first length below and the first tap count above a form are refused."""
    for c in CASES:
        f = sc.FORMS[c.form]
        fn = getattr(lib, f.supported)
        table = ts.entries(f.table)
        for n in {c.N, sc.case(c)["N"]}:
            assert fn(n, c.K, sc.WIND) == 1, (sc.case_id(c), n)
            assert ts.pick_cheapest(table, n, c.K, ts.per_lane(f.table)) == c.entry, (sc.case_id(c), n)
    for form, f in sc.FORMS.items():
        fn = getattr(lib, f.supported)
        inst = sc.instances(form)
        first, last, k_max = inst[0][1], inst[-1][2], max(e[1] for e, _, _ in inst)
        below = first - 1 if sc.four_waves(form) else 0             # (the one-wave forms serve every length from one scan on)
        assert fn(first, 1, sc.WIND) == 1 and fn(last, k_max, sc.WIND) == 1
        assert fn(below, 1, sc.WIND) == 0 and fn(last + 1, 1, sc.WIND) == 0, form
        assert fn(last, k_max + 1, sc.WIND) == 0 and fn(first, k_max + 1, sc.WIND) == 0, form


def test_lengths_at_the_short_corners():
    used = {}
    for c in CASES:
        if sc._short(c):
            used[sc.case_id(c)] = sc.case(c)["N"]
            assert c.N == sc.MIN_SCANS and (used[sc.case_id(c)] == c.N or used[sc.case_id(c)] in ts.LADDER)
        else:
            assert sc.case(c)["N"] == c.N
    print("%d cases; lengths used at the short corners:" % len(CASES))
    for name, n in used.items():
        print("   %-64s %d scans" % (name, n))
    assert len(used) == sum(2 * (3 if sc.instances(f)[0][0][1] > 33 else 2) for f in sc.FORMS if not sc.four_waves(f))
    assert min(used.values()) == sc.MIN_SCANS


@pytest.mark.parametrize("c", CASES, ids=sc.case_id)
def test_case_conditions_and_oracles(c):
    """The stored references of a case meet every condition (search_cases.check, restated here row by row where a count is
    cheap to state), and on every row and budget the restated search equals orc.deconv_auto_lbda in n_outer exactly and in W,
    R, G, J to 1e-13; c_oracle.deconv_auto_lbda_batch agrees to 1e-12 and in n_outer."""
    d = sc.case(c)
    sc.check(d)
    V, N, neg, ref = d["V"], d["N"], d["negative"], d["ref"]
    assert V == (3 if sc.four_waves(c.form) else 6) and d["Y"].shape == (V, N) and not d["Y"].flags.writeable
    assert (d["W0"] is not None) == (c.corner == "full") and ("WARM" in ref) == (c.corner == "full")
    assert d["taps"].shape == ((V, c.K) if c.pp else (c.K,)) and max(d["draws"]) <= sc.REDRAWS + 1
    for name, runs in ref.items():
        nb_iter, nb_sub_iter, tol, early = sc.BUDGETS["QUIET" if name == "WARM" else name]
        for v, run in enumerate(runs):
            assert np.abs(run.alpha).min() > sc.ALPHA_MIN and len(run.alpha) == run.n_outer == len(run.J)
            assert run.lbda == 1.0 / (2.0 * run.alpha[-1])
            if early:
                assert sc.clearance(run, tol) >= sc.CLEAR
                assert len(run.crit_alpha) == max(run.n_outer - 7, 0)          # first evaluated at outer iteration 8
                assert (run.crit_alpha[:-1] >= tol).all()
                assert run.n_outer == nb_iter or run.crit_alpha[-1] < tol
            else:
                assert not run.crit_alpha.size and not run.crit_inner.size
            if name in ("QUIET", "WARM", "OFF"):
                assert (run.n_outer, run.n_inner) == (nb_iter, (nb_iter + 1) * nb_sub_iter), (name, v)
    fire, nb_iter, nb_sub_iter = ref["FIRE"], sc.BUDGETS["FIRE"][0], sc.BUDGETS["FIRE"][1]
    stops = [r.n_outer for r in fire]
    assert min(stops) < nb_iter and stops[neg] == nb_iter
    assert N < 320 or len({n for n in stops if n < nb_iter}) >= 2, stops
    assert all(r.n_inner < (r.n_outer + 1) * nb_sub_iter for v, r in enumerate(fire) if v != neg)
    assert (fire[neg].alpha < 0).any() and (ref["QUIET"][neg].alpha < 0).any()
    # the oracles, row by row (pp: each row with its own taps and Lipschitz constant)
    worst = [0.0, 0.0]
    for name in sc.BUDGETS:
        nb_iter, nb_sub_iter, tol, early = sc.BUDGETS[name]
        for v, run in enumerate(ref[name]):
            hrf = d["taps"][v] if c.pp else d["taps"]
            kw = dict(early_stopping=early, tol=tol, nb_iter=nb_iter, nb_sub_iter=nb_sub_iter)
            _, _, wo, Jo, Ro, Go = orc.deconv_auto_lbda(d["Y"][v], hrf, float(d["sigma"][v]), float(d["lips"][v]), **kw)
            assert len(Jo) == run.n_outer, (name, v, len(Jo), run.n_outer)
            errs = [rel(run.W, wo), rel(run.R, Ro), rel(run.G, Go), rel(run.J, Jo)]
            assert max(errs) <= 1e-13, (name, v, errs)
            Wc, Jc, Rc, Gc, nc = c_oracle.deconv_auto_lbda_batch(d["Y"][v:v + 1], hrf, d["sigma"][v:v + 1], float(d["lips"][v]),
                                                                 threads=1, **kw)
            n = run.n_outer
            assert int(nc[0]) == n, (name, v, int(nc[0]), n)
            assert np.isnan(Jc[0, n:]).all()
            errc = [rel(Wc[0], run.W), rel(Rc[0, :n], run.R), rel(Gc[0, :n], run.G), rel(Jc[0, :n], run.J)]
            assert max(errc) <= 1e-12, (name, v, errc)
            worst = [max(worst[0], max(errs)), max(worst[1], max(errc))]
    print("%s at %d scans: FIRE stops %s, n_inner %s; draws %s; restatement vs NumPy oracle %.1e, vs C oracle %.1e"
          % (sc.case_id(c), N, stops, [r.n_inner for r in fire], list(d["draws"]), worst[0], worst[1]))
