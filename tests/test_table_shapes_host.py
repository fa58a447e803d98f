"""CPU-only checks of tests/table_shapes.py, the tables-as-test-data helper behind tests/test_gpu_table_entries.py: no
table has a dead line, the restated pickers agree with the library's own queries over the whole grid of shapes, the pins
of the GPU test reach the kernel family they are meant to reach at every edge shape (or the case is a listed skip), and
the selection of stop-rule inputs agrees with the oracles.  No kernel is launched."""
import ctypes
import os

import numpy as np
import pytest

import table_shapes as ts

NONE, LOOPS, WINDOW = 0, 1, 2
STOPS = ((None, NONE, 6),) + (("loops", LOOPS, 6),) + tuple(("window", WINDOW, w) for w in ts.WINDS)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from pybold_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_tables_parse_and_have_no_dead_line():
    for table in ts.TABLES:
        tab = ts.entries(table)
        assert tab and len(set(tab)) == len(tab), (table, tab)
        for e in tab:
            shapes = ts.edge_shapes(table, e)
            assert len(shapes) == 2, "no shape of the grid selects %s %s: a dead line" % (table, e)
            for _, N, K in shapes:
                assert ts.pick(table, N, K) == e and N <= ts.per_lane(table) * e[0] and K <= e[1]
            (_, nf, kf), (_, nm, km) = shapes
            assert kf == e[1] and nm <= nf and km <= kf
    # the grid is wide enough: no table reaches its border
    for table in ts.TABLES:
        cov = ts.covered(table)
        assert not cov[ts.N_GRID].any() and not cov[:, ts.K_GRID].any(), table


def test_regions_come_from_the_enumerated_set():
    """Regions need not be rectangles: the corners of the current fast table that a rectangle would get wrong.

    A snapshot: these are facts of the fast and wide tables as they stand, so the test steps aside (a skip, with the reason)
    as soon as a line of either table changes -- the checks that follow a changed table are the other tests of this file."""
    if ts.entries("wide") != ((5, 30), (5, 32), (12, 32), (19, 30), (19, 32), (19, 48), (20, 32), (20, 48), (38, 32)) or \
            ts.entries("fast") != ((8, 16), (10, 30), (10, 48), (15, 27), (15, 30), (18, 28), (19, 27), (19, 30), (19, 32), (19, 40),
                              (19, 48), (24, 32), (38, 30)):
        pytest.skip("fast_table.inc or wide_table.inc has changed: these are facts of the table this test was written against")
    r = set(ts.region("fast", (19, 32)))                               # a rectangle: 161..304 scans, 31..32 taps
    assert r == {(n, k) for n in range(161, 305) for k in (31, 32)}
    assert ts.edge_shapes("fast", (19, 32)) == [("full", 304, 32), ("masked", 161, 31)]
    r = set(ts.region("fast", (19, 30)))                               # L-shaped: (18, 28) takes 28 taps up to 288 scans
    assert {k for n, k in r if n == 241} == {29, 30} and {k for n, k in r if n == 288} == {29, 30}
    assert {k for n, k in r if n == 289} == {28, 29, 30} and {k for n, k in r if n == 304} == {28, 29, 30} and len(r) == 144
    assert ts.edge_shapes("fast", (19, 30)) == [("full", 304, 30), ("masked", 241, 29)]
    r = set(ts.region("fast", (10, 30)))                               # N <= 128 only beyond the 16 taps of (8, 16)
    assert {k for n, k in r if n == 128} == set(range(17, 31)) and {k for n, k in r if n == 129} == set(range(1, 31))
    assert ts.edge_shapes("fast", (10, 30)) == [("full", 160, 30), ("masked", 1, 17)]
    assert ts.edge_shapes("wide", (19, 48)) == [("full", 1216, 48), ("masked", 1, 33)]
    # the split pair form: only where no whole-series pair entry fits -- beyond the 304 scans of the (19, *) entries
    assert ts.split_edge_shapes((8, 16)) == [] and ts.split_edge_shapes((19, 32))[:2] == [("lo", 305, 32), ("hi", 608, 32)]
    assert ts.split_edge_shapes((10, 30)) == [("hi", 320, 30), ("masked", 305, 1)]


def test_restatement_agrees_with_has_fast_path(lib):
    want = ts.covered("fast") | ts.covered("wide")
    got = np.zeros_like(want)
    for N in range(1, ts.N_GRID + 1):
        for K in range(1, ts.K_GRID + 1):
            got[N, K] = lib.pb_fista_has_fast_path(N, K)
    assert (got == want).all(), np.argwhere(got != want)[:5]
    # the vectorised choice is the scalar picker's
    rng = np.random.RandomState(0)
    for table in ts.TABLES:
        for N, K in zip(rng.randint(1, ts.N_GRID + 1, 400), rng.randint(1, ts.K_GRID + 1, 400)):
            e = ts.pick(table, int(N), int(K))
            assert (e is not None) == bool(ts.covered(table)[N, K])
            assert e is None or (int(N), int(K)) in set(ts.region(table, e))


@pytest.mark.parametrize("stop,code,wind", STOPS)
def test_restatement_agrees_with_the_float64_queries(lib, stop, code, wind):
    """pb_fista_which_kernel_d: 7 exactly where exact_table.inc has an entry, 8 exactly where only exact_split_table.inc
    has one; pb_fista_which_kernel_pp_d: 9 exactly where exact_table.inc has one (no four-wave form behind it); with the
    window rule only at wind = 6."""
    rule = ts.ring_fits(1, stop, wind, float64=True)
    one, four = ts.covered("exact") & rule, ts.covered("exact_split") & rule
    assert not (one & four).any()
    for N in range(1, ts.N_GRID + 1):
        for K in range(1, ts.K_GRID + 1):
            d = lib.pb_fista_which_kernel_d(N, K, 0, code, wind)
            pp = lib.pb_fista_which_kernel_pp_d(N, K, 0, code, wind)
            assert (d == 7) == one[N, K] and (d == 8) == four[N, K] and d in (7, 8, 0, -1), (N, K, d)
            assert (pp == 9) == one[N, K] and pp in (9, 0, -1), (N, K, pp)


def _plan_form(lib, N, K, P, code, wind, flags):
    nm, mf, tf = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert lib.pb_fista_plan_ex(N, K, P, code, wind, flags, ctypes.byref(nm), ctypes.byref(mf), ctypes.byref(tf)) == 0
    return mf.value if nm.value else tf.value


def test_pins_reach_the_family_at_every_edge_shape(lib):
    """`fast1` gives the single-row kernel of the entry, `wide` one problem per wave of the entry, `fast2` the pair kernel
    where the entry has one and the single-row kernel where it has none (route() restated: table_shapes.forced_form).

    solver.launch_plan is compared as far as it goes: pb_fista_plan_ex reads the pins of a form as "the plan without the
    matrix pipe" (capi.hip), so it names the cheapest form for the batch, not the pinned one -- it must still agree on
    whether a register-resident form carries the call at all (form 0, the LDS kernel, exactly where the restated route ends
    there: PB_FLAG_FORCE_FAST turns that into an error instead of another kernel)."""
    from pybold_amd import solver
    for table, V, force, want in (("fast", 37, "fast1", ts.SINGLE_ROW), ("wide", 5, "wide", ts.WIDE)):
        for e in ts.entries(table):
            for _, N, K in ts.edge_shapes(table, e):
                for stop, code, wind in STOPS:
                    form, got, why = ts.forced_form(N, K, V, stop, wind, force)
                    if ts.ring_fits(e[0], stop, wind):
                        assert (form, got) == (want, e), (table, e, N, K, stop, wind, form, got, why)
                    else:
                        assert got != e and why, (table, e, N, K, stop, wind, form, got)
                    plan = _plan_form(lib, N, K, V, code, wind, solver._FORCE[force])
                    assert (plan == 0) == (form == ts.GENERIC), (table, e, N, K, stop, wind, plan, form)
                    assert solver.launch_plan(N, K, V, stop, wind, force)[2] == solver.KERNEL_NAMES[plan]
    for e in ts.entries("fast"):
        for _, N, K in ts.edge_shapes("fast", e):
            form, got, why = ts.forced_form(N, K, 37, None, 6, "fast2")
            if ts.has_pair(e):
                assert (form, got) == (ts.PAIR, e)
                for force in ("fast2d", "cert2", "certonly"):
                    stop, wind = ("window", 6) if force != "fast2d" else (None, 6)
                    assert ts.forced_form(N, K, 37, stop, wind, force)[:2] == (ts.PAIR, e)
                assert ts.forced_form(N, K, 1, None, 6, "fast2")[0] == ts.SINGLE_ROW          # a lone problem has no pair
                assert ts.forced_form_pp(N, K, 37, True, None, "fast2")[:2] == (ts.PAIR, e)
            elif ts.pick_split(N, K) is None:
                assert (form, got) == (ts.SINGLE_ROW, e) and why
            else:
                assert form == ts.PAIR + " split" and ts.has_pair(got)                        # (another entry's pair form)
            assert ts.forced_form_pp(N, K, 37, False, None, "fast1")[:2] == (ts.SINGLE_ROW, e)
            assert ts.forced_form_pp(N, K, 37, False, "loops", "fast1")[:2] == (ts.SINGLE_ROW, e)
    for e in ts.entries("fast"):
        for _, N, K in ts.split_edge_shapes(e):
            assert ts.pick_split(N, K) == e and 16 * e[0] < N <= 32 * e[0]
            assert ts.forced_form(N, K, 37, None, 6, "fast2")[:2] == (ts.PAIR + " split", e)
            assert ts.forced_form(N, K, 37, "window", 6, "cert2")[:2] == (ts.PAIR + " split", e)
    # per-problem taps, one problem per wave: reached where no single-row entry takes the shape first, or on a short entry --
    # the GPU cases take their corners from that part of the region, so every entry runs at two shapes of its own
    for e in ts.entries("wide"):
        for _, N, K in ts.edge_shapes("wide", e):
            form, got, _ = ts.forced_form_pp(N, K, 5, False, None, "fast")
            assert form in (ts.WIDE, ts.SINGLE_ROW) and (form != ts.WIDE or got == e)
            assert (form == ts.WIDE) == (ts.pick("fast", N, K) is None or e[0] <= 8)
        shapes = ts.edge_shapes_pp_wide(e, 5)
        assert len(shapes) == 2 and shapes[0][2] == e[1], (e, shapes)
        for _, N, K in shapes:
            assert ts.pick("wide", N, K) == e
            for stop in (None, "loops"):
                assert ts.forced_form_pp(N, K, 5, False, stop, "fast")[:2] == (ts.WIDE, e), (e, N, K)
    # (the unpinned queries do not discriminate among the 16-lane forms at these batch sizes: which_kernel and the plan
    # without the matrix pipe name the same form for one problem and for 37 -- the cheapest one, not a pinned one)
    for e in ts.entries("fast"):
        if ts.has_pair(e):
            for _, N, K in ts.edge_shapes("fast", e):
                assert solver.launch_plan(N, K, 37, force="valu")[2] == solver.launch_plan(N, K, 1, force="valu")[2]


def test_the_gpu_cases_cover_every_compiled_instance():
    """Every (entry, family, variant) that launch_fast.h and the pair, exact and exact-split launchers compile appears
    at both corners in the parametrisation of tests/test_gpu_table_entries.py."""
    import test_gpu_table_entries as gt
    seen = {}
    for p in gt._cases():
        family, entry, N, K, variant = p.values
        seen.setdefault((family, entry, variant), []).append((N, K))
    per_stop = 2 * (2 + len(ts.WINDS))                      # cost trace x (none, loops, three windows)
    for e in ts.entries("fast"):
        for family, table in (("single_row", "fast"),):
            have = {v for (f, en, v) in seen if f == family and en == e}
            stops = {v for v in have if v in ("cold", "J") or v.startswith(("loops", "win"))}
            assert len(stops) == (per_stop if e[0] <= 20 else 4) and "warm" in have, (e, have)
        assert {v for (f, en, v) in seen if f == "pp_single_row" and en == e} == {"warm", "loops"}
        for family in ("pair_ffa", "pair_direct", "pair_cert", "pair_dev"):
            assert any(f == family and en == e for (f, en, _) in seen) == ts.has_pair(e), (family, e)
        assert any(f == "pair_split" and en == e for (f, en, _) in seen) == bool(ts.split_region(e))
    for e in ts.entries("wide"):
        have = {v for (f, en, v) in seen if f == "one_per_wave" and en == e}
        assert len(have - {"warm"}) == (per_stop if e[0] <= 20 else 4), (e, have)
        assert {v for (f, en, v) in seen if f == "pp_one_per_wave" and en == e} == {"warm", "loops"}
    for family, table in (("f64_one_wave", "exact"), ("f64_pp", "exact"), ("f64_four_waves", "exact_split")):
        for e in ts.entries(table):
            have = {v for (f, en, v) in seen if f == family and en == e}
            assert have - {"warm"} == {"cold", "J", "loops", "loopsJ", "win6", "win6J"}, (family, e, have)
    for key, shapes in seen.items():
        assert len(set(shapes)) >= 2 or key[0] == "pair_split", key
    ids = [p.id for p in gt._cases()]
    assert len(set(ids)) == len(ids)


def test_selection_of_stop_rule_inputs_agrees_with_the_oracles():
    """table_shapes.trajectory restates the recurrence only to read the criteria: on a small shape its stop iterations are
    orc.loops_batch's and orc.deconv_fixed_lbda's at every tolerance and window, and the drawn inputs meet the conditions
    the GPU test relies on."""
    from oracle import pybold_oracle as orc
    rng = np.random.RandomState(5)
    N, K, V, n_iter = 70, 9, 12, 60
    taps = 0.3 * rng.randn(K)
    step = 1.0 / ts.lipschitz(taps, N)
    Y = rng.randn(V, N) * (10.0 ** rng.uniform(-1.5, 1.0, size=(V, 1)))
    crit_l, crit_w = ts.trajectory(Y, taps, 0.5, step, n_iter)
    some = 0
    for tol in ts.TOLS:
        nd, fired, clear = ts.fire_iteration(crit_l, tol, n_iter)
        _, nd_o = orc.loops_batch(Y, taps, 0.5, step, n_iter, tol)
        assert (nd[clear] == nd_o[clear]).all()
        some += int(fired.sum())
        for wind in ts.WINDS:
            nd, fired, clear = ts.fire_iteration(crit_w[wind], tol, n_iter)
            nd_o = np.array([orc.deconv_fixed_lbda(Y[v], taps, 0.5, nb_iter=n_iter, tol=tol, wind=wind, lipschitz=1.0 / step,
                                                   dense=False)[4] for v in range(V)])
            assert (nd[clear] == nd_o[clear]).all(), (tol, wind, nd, nd_o)
            assert (nd[fired] > wind + 1).all()
            some += int(fired.sum())
    assert some > 20
    for rule, wind, V, pp in (("loops", 6, 37, False), ("window", 4, 5, False), ("window", 8, 37, False), ("window", 6, 3, False),
                              ("loops", 6, 5, True)):
        c = ts.stop_rule_inputs(161, 31, V, rule, wind=wind, per_problem_taps=pp)
        assert c["Y"].shape == (V, 161) and c["tol"] in ts.TOLS
        fired = c["n_done"] < c["n_iter"]
        assert 3 * fired.sum() >= V and len(set(c["n_done"][fired])) >= 2 and (~fired).any()
        crit_l, crit_w = ts.trajectory(c["Y"], c["taps"], c["lbda"], c["steps"], c["n_iter"])
        nd, _, clear = ts.fire_iteration(crit_l if rule == "loops" else crit_w[wind], c["tol"], c["n_iter"])
        assert clear.all() and (nd == c["n_done"]).all()
        again = ts.stop_rule_inputs(161, 31, V, rule, wind=wind, per_problem_taps=pp)
        assert np.array_equal(again["Y"], c["Y"]) and again["tol"] == c["tol"]            # deterministic


def test_certificate_inputs_meet_the_conditions():
    """The batch of the certificate families: the conditions of a stop-rule case, the rows that never fire are cold and
    stay `certificate_reach` times tol above tol, the rows that fire are warm; too few tracked samples, no inputs."""
    assert ts.certificate_reach(4, 8, False) is None and ts.certificate_reach(1, 10, False) is None
    assert abs(ts.certificate_reach(128, 8, False) - 2 * np.sqrt(1.04 * 8)) < 1e-12            # 16 tracked samples of 16 S
    assert abs(ts.certificate_reach(608, 19, True) - 2 * np.sqrt(1.04 * 19)) < 1e-12           # 32 of 32 S in a split series
    assert ts.certificate_reach(60, 8, False) is None                                          # seven tracked samples
    assert abs(ts.certificate_reach(61, 8, False) - 2 * np.sqrt(1.04 * 61 / 8)) < 1e-12        # eight
    with pytest.raises(ts.NoInputs):
        ts.certificate_inputs(1, 1, 37, 8)
    for N, K, S, split in ((161, 31, 19, False), (305, 32, 19, True)):
        c = ts.certificate_inputs(N, K, 37, S, split=split, seed=1)
        fired = c["n_done"] < c["n_iter"]
        assert c["tol"] in ts.TOLS and c["n_iter"] <= 60
        assert 3 * fired.sum() >= 37 and len(set(c["n_done"][fired])) >= 2 and (~fired).any()
        crit = ts.trajectory(c["Y"], c["taps"], c["lbda"], c["steps"], c["n_iter"], W0=c["W0"])[1][6]
        nd, _, clear = ts.fire_iteration(crit, c["tol"], c["n_iter"])
        assert clear.all() and (nd == c["n_done"]).all()
        cold = np.abs(c["W0"]).max(axis=1) == 0
        assert cold[~fired].all() and (np.nanmin(crit[~fired], axis=1) >= c["reach"] * c["tol"]).all()
        again = ts.certificate_inputs(N, K, 37, S, split=split, seed=1)
        assert np.array_equal(again["Y"], c["Y"]) and np.array_equal(again["W0"], c["W0"])
    near = ts.stop_rule_inputs_near("fast", (8, 16), 1, 1, 37, "window", wind=6, seed=1, certificate=True)
    assert near["N"] == 64                                 # (eight tracked samples from 61 scans on; 64: the next of LADDER)
