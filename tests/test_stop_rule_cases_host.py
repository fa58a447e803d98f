"""tests/stop_rule_cases.py on the CPU: the case list against table_shapes.mfma_instance (no compiled rule instance of the
matrix-pipe kernels without its corners), the conditions on the inputs of a case, and the judge against results that are
wrong in one row -- what tests/test_gpu_mfma_stop_rules.py relies on, checked without a GPU."""
import numpy as np
import pytest

import stop_rule_cases as sc
import table_shapes as ts
from oracle import pybold_oracle as orc


def _block_range(form, instance):
    """(first N, last N) of the series lengths `mfma_instance` puts on an instance, at the fewest taps of its tile count."""
    k = 1 if instance.endswith("2t") else 34
    ns = [n for n in range(sc.N_LO, sc.N_HI + 1) if ts.mfma_instance(form, n, k) == instance]
    return ns[0], ns[-1]


def test_case_list_covers_every_rule_instance():
    k_max = sc.max_taps()
    assert 34 < k_max <= sc.K_HI
    # every instance mfma_instance names over 129 .. 1 280 scans and 1 .. k_max taps -- but the one-wave form with three near
    # tiles, which has no rule variant (pick_mfma(.., stop_rule = true) of dispatch.h)
    named = {(form, ts.mfma_instance(form, n, k)) for form in sc.FORMS for n in range(sc.N_LO, sc.N_HI + 1) for k in (1, 33, 34, k_max)}
    named = {(f, i) for f, i in named if i is not None and not (f == "mfma" and i.endswith("3t"))}
    assert len(named) == len({i for _, i in named}) >= 45
    listed = {}
    for c in sc.cases():
        assert ts.mfma_instance(c.form, c.N, c.K) == c.instance and sc.reaches(c.form, c.N, c.K, c.rule), c
        listed.setdefault((c.form, c.instance, c.rule), {})[c.corner] = (c.N, c.K)
    assert set(listed) == {(f, i, r) for f, i in named for r in sc.RULES}
    for (form, inst, rule), got in listed.items():
        lo, hi = _block_range(form, inst)
        two = inst.endswith("2t")
        assert {"masked", "full"} <= set(got), (inst, rule, got)
        assert got["masked"] == (lo, 1 if two else 34), (inst, rule, got)
        n_full = got["full"][0]
        top = got.get("taps", got["full"])[1]
        assert top == max(k for k in (range(1, 34) if two else range(34, sc.K_HI + 1)) for n in range(lo, hi + 1) if sc.reaches(form, n, k, rule))
        # the most taps of the tile count -- the one-wave form's certificate is planned beside the pair form's: 30 or 32 taps
        if rule == "loops" or form != "mfma":
            assert top == (33 if two else k_max), (inst, rule, got)
        else:
            assert top >= 30, (inst, rule, got)
        # the longest series of the block range, but where no backup form carries the rule there (the increment ring of the
        # window rule ends at 304 scans on the single-row entries)
        assert n_full == max(n for n in range(lo, hi + 1) if any(sc.reaches(form, n, k, rule) for k in (1, 34))), (inst, rule, got)
        if rule == "loops":
            assert n_full == hi
    assert len(sc.cases()) >= 4 * len(named)
    assert len({sc.case_id(c) for c in sc.cases()}) == len(sc.cases())


def test_the_launchers_refuse_what_the_list_leaves_out():
    assert not sc.reaches("mfma", 300, 34, "loops") and not sc.reaches("mfma", 300, 34, "window")       # no rule beside three tiles
    assert not sc.reaches("mfma2", 224, 34, "loops") and sc.reaches("mfma2", 225, 34, "loops")          # four blocks per wave
    assert not sc.reaches("mfma", 310, 33, "loops") and sc.reaches("mfma", 310, 32, "loops")            # no single-row entry
    assert not sc.reaches("mfma", 305, 20, "window") and sc.reaches("mfma", 304, 20, "window")          # no increment ring
    assert not sc.reaches("mfma4", 1280, 49, "loops") and sc.reaches("mfma4", 1280, 48, "loops")        # no backup form


def _host_cases():
    out = [c for c in sc.cases() if c.form == "mfma" and c.corner in ("masked", "full")]
    for form in ("mfma2", "mfma4"):
        insts = [c.instance for c in sc.cases() if c.form == form]
        ends = {insts[0], insts[-1]}
        out += [c for c in sc.cases() if c.form == form and c.instance in ends and c.corner in ("masked", "full")]
    return out


@pytest.mark.parametrize("case", _host_cases(), ids=sc.case_id)
def test_selection_conditions(case):
    inp = sc.inputs(case)                                   # (raises NoInputs where no batch meets them: no case may)
    V, n_iter, tol, nd, fired = sc.V_ROWS, inp["n_iter"], inp["tol"], inp["n_done"], inp["fired"]
    sc.check_selection(inp)
    assert inp["Y"].shape == (V, case.N) and len(inp["taps"]) == case.K and n_iter <= sc.BUDGET and tol >= 1e-3
    assert (inp["Y"] == inp["Y"].astype(np.float32)).all()
    # the criteria, restated: table_shapes.trajectory on the rows kept (the selection ran on the operator as a matrix)
    crit_l, crit_w = ts.trajectory(inp["Y"], inp["taps"], inp["lbda"], inp["step"], n_iter, W0=inp["W0"])
    crit = crit_l if case.rule == "loops" else crit_w[sc.WIND]
    np.testing.assert_allclose(inp["crit"], crit, rtol=1e-7, atol=0.0)
    nd2, fired2, clear2 = ts.fire_iteration(crit, tol, n_iter)
    assert (nd2 == nd).all() and (fired2 == fired).all() and clear2.all()
    tested = np.isfinite(crit) & (np.arange(n_iter)[None, :] < nd[:, None])
    assert (np.abs(crit - tol)[tested] >= sc.BAND * tol).all()
    # half of the rows fire, at three iterations or more, one past the first periodic range check; some never do
    assert 2 * fired.sum() >= V and len(set(nd[fired].tolist())) >= 3 and nd[fired].max() > 8 and (~fired).any()
    assert fired[:16].all() and (~fired[16:]).any() and V % 16 == 5
    # dense at the stopping iteration, with a factor 2 to spare: the accuracy guard has no reason to hand a row back
    Wr = sc.iterates_at(inp, nd)
    assert (inp["lbda"] * inp["step"] <= 0.5 * 0.02 * np.abs(Wr).max(axis=1)).all()
    # the oracle stops where the selection says (the warm rows of a window case through deconv_fixed_lbda's w0)
    if case.rule == "loops":
        Wo, ndo = orc.loops_batch(inp["Y"], inp["taps"], inp["lbda"], inp["step"], n_iter, tol)
        assert (ndo == nd).all()
        assert (np.linalg.norm(Wo - Wr, axis=1) <= 1e-9 * np.linalg.norm(Wr, axis=1)).all()
    else:
        for v in (0, 7, 15, 16, 17, V - 1):
            o = orc.deconv_fixed_lbda(inp["Y"][v], inp["taps"], inp["lbda"], nb_iter=n_iter, tol=tol, wind=sc.WIND,
                                      lipschitz=1.0 / inp["step"], dense=False, w0=inp["W0"][v])
            assert o[4] == nd[v] and np.linalg.norm(o[2] - Wr[v]) <= 1e-9 * np.linalg.norm(Wr[v])


@pytest.fixture(scope="module", params=["loops", "window"])
def judged(request):
    case = [c for c in sc.cases() if c.form == "mfma" and c.corner == "full" and c.rule == request.param][0]
    inp = sc.inputs(case)
    W = sc.iterates_at(inp, inp["n_done"])
    J = sc.trace(inp).copy()
    J[np.arange(inp["n_iter"])[None, :] >= inp["n_done"][:, None]] = np.nan
    for a in (W, J):
        a.setflags(write=False)
    return inp, W, J


def test_judge_accepts_the_oracle(judged):
    inp, W, J = judged
    v = sc.judge(inp, W, inp["n_done"], J)
    assert v.err < 1e-12 and v.differed == 0 and v.jerr < 1e-12
    assert sc.judge(inp, W * (1.0 + 3e-6), inp["n_done"]).err == pytest.approx(3e-6, rel=1e-3)
    assert sc.judge(inp, W.astype(np.float32), inp["n_done"].astype(np.int32), J.astype(np.float32)).err < 1e-6


@pytest.mark.parametrize("change", ["one iteration later", "one iteration earlier", "the next iteration's iterate",
                                    "the last iteration's iterate", "left at its start", "scaled by 1 + 3e-5", "trace past the stop",
                                    "n_done of zero", "trace off by 1e-4"])
def test_judge_catches_one_wrong_row(judged, change):
    inp, W, J = judged
    nd = inp["n_done"].copy()
    W, J = W.copy(), J.copy()
    v = int(np.flatnonzero(inp["fired"] & inp["clear"])[5])           # a clear row that fires
    if change == "one iteration later":
        nd[v] += 1
        W[v] = sc.iterates_at(inp, nd)[v]                   # (even with the iterate of that iteration)
    elif change == "one iteration earlier":
        nd[v] -= 1
        W[v] = sc.iterates_at(inp, nd)[v]
    elif change == "the next iteration's iterate":
        W[v] = sc.iterates_at(inp, nd + 1)[v]
    elif change == "the last iteration's iterate":
        W[v] = sc.iterates_at(inp, np.full_like(nd, inp["n_iter"]))[v]
    elif change == "left at its start":
        W[v] = 0.0 if inp["W0"] is None else inp["W0"][v]
    elif change == "scaled by 1 + 3e-5":
        W[v] *= 1.0 + 3e-5
    elif change == "trace past the stop":
        J[v, nd[v]] = J[v, nd[v] - 1]
    elif change == "n_done of zero":
        nd[v] = 0
    elif change == "trace off by 1e-4":
        J[v, nd[v] - 1] *= 1.0 + 1e-4
    with pytest.raises(AssertionError):
        sc.judge(inp, W, nd, J)


def test_judge_allows_one_iteration_on_rows_that_are_not_clear(judged):
    """The edited sweeps of tests/test_gpu_round4.py, test_gpu_round5.py and test_gpu_mfma.py: a row not known to be clear may
    stop one iteration apart -- and is compared with the oracle's iterate of THAT iteration."""
    inp, W, _ = judged
    sweep = sc.sweep_case(inp["Y"], inp["taps"], inp["lbda"], inp["step"], inp["n_iter"], inp["n_done"], W0=inp["W0"])
    nd = inp["n_done"].copy()
    v = int(np.flatnonzero(inp["fired"])[3])
    nd[v] += 1
    with pytest.raises(AssertionError):
        sc.judge(sweep, W, nd)                              # the iterate of the oracle's iteration under another n_done
    W2 = W.copy()
    W2[v] = sc.iterates_at(inp, nd)[v]
    assert sc.judge(sweep, W2, nd).differed == 1
    nd[v] += 1
    W2[v] = sc.iterates_at(inp, nd)[v]
    with pytest.raises(AssertionError):
        sc.judge(sweep, W2, nd)                             # two iterations apart
