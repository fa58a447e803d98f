"""The row-in-LDS helper kernels of csrc/generic.h at the edges of their block primitives (cases, references and bounds:
tests/helper_cases.py; their own checks: tests/test_helper_cases_host.py).  Every case runs two input families of three
rows: small integers, where every summation order gives the same float64 bits and the kernel must return them EXACTLY, and
reals (amplitudes over twelve decades, a cancelling carrier, a DC offset) against a longdouble reference within a bound
derived per output element.  Every buffer is a framed, padded window (tests/frames.py): guard bands and inputs must come
back untouched, and the packed call must return the bits of the padded one.

The limit test runs each entry at the longest row its launcher's `exceeds LDS` check admits (up to 160 000 bytes of dynamic
LDS) on two rows, and expects the loud error one scan further.

PB_HELPER_KERNELS_REPORT=<file> appends one JSON line per case (entry, shape, family, worst error / bound, seconds): the
source of profiles/helper_kernels.txt."""
import functools
import json
import os
import time

import numpy as np
import pytest
import torch

import frames
import helper_cases as hc

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32


def report(entry, shape, family, ratio, seconds):
    print("%s %s %s: error / bound %.3g, %.3f s" % (entry, shape, family, ratio, seconds))
    path = os.environ.get("PB_HELPER_KERNELS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"entry": hc.ENTRY_POINT[entry], "shape": shape, "family": family, "ratio": ratio,
                                "seconds": round(seconds, 4)}) + "\n")


def host(frame):
    return frame.contiguous().cpu().numpy()


def launch(case, inp, packed):
    """One call of the case's entry point on framed buffers.  ({output name: frame}, input frames)"""
    e = case.entry
    x = inp["x"]
    rows = x.shape[0]
    f2 = functools.partial(frames.frame2d, device=DEV, packed=packed)
    f1 = functools.partial(frames.frame1d, device=DEV, packed=packed)
    ydt = F32 if e in hc.F32_Y else F64
    ins, outs = [], {}
    if e in hc.GROUPS["operators"]:
        src = f2("W", rows, x.shape[1], F64, fill=x)
        n_dst = case.n_in if e in ("corr", "op_adjoint") else case.n_out
        outs["out"] = f2("out", rows, n_dst, F64)
        ins = [src.snapshot()]
        outs["out"].snapshot()
        if e in hc.INTEG:
            getattr(frames, e)(src, outs["out"])
        else:
            getattr(frames, e)(src, outs["out"], inp["taps"])
    elif e in ("outputs", "outputs_pp"):
        w = f2("W", rows, case.n_in, F64, fill=x)
        z = f2("out", rows, case.n_in, F64) if "z" in case.opt else None
        xo = f2("y", rows, case.n_in, F64) if "x" in case.opt else None
        ins = [w.snapshot()]
        for name, f in (("z", z), ("x", xo)):
            if f is not None:
                outs[name] = f.snapshot()
        if e == "outputs":
            frames.fista_outputs(w, inp["taps"], z=z, x=xo)
        else:
            taps = f2("taps_pp", rows, case.K, F64, fill=inp["taps"]).snapshot()
            ins.append(taps)
            frames.fista_outputs_pp(w, taps, case.K, z=z, x=xo)
    elif e in ("stats", "stats_d"):
        w = f2("W", rows, case.n_in, F64, fill=x)
        y = f2("y", inp["y"].shape[0], case.n_in, ydt, fill=inp["y"])
        outs = {"r2": f1("r2", rows, F64), "l1": f1("l1", rows, F64)}
        ins = [w.snapshot(), y.snapshot()]
        for f in outs.values():
            f.snapshot()
        frames.fista_stats(w, y, inp["taps"], outs["r2"], outs["l1"], y_rep=case.opt)
    elif e in ("lambda_max", "lambda_max_d"):
        y = f2("y", rows, case.n_in, ydt, fill=inp["y"])
        outs = {"out": f1("out", rows, F64).snapshot()}
        ins = [y.snapshot()]
        frames.lambda_max(y, inp["taps"], outs["out"])
    elif e.startswith("hrf_cost"):
        z = f2("W", rows, case.n_in, F64, fill=x)
        y = f2("y", rows, case.n_in, ydt, fill=inp["y"])
        taps = f1("taps", inp["taps"].size, F64, fill=inp["taps"].ravel())
        outs = {"cost": f1("cost", case.opt * rows, F64).snapshot()}
        ins = [z.snapshot(), y.snapshot(), taps.snapshot()]
        (frames.hrf_cost_pv if "_pv" in e else frames.hrf_cost)(z, y, taps, case.K, case.opt, outs["cost"])
    else:
        raise KeyError(e)
    torch.cuda.synchronize()
    return outs, ins


def check_frames(outs, ins, packed_outs):
    for name, f in outs.items():
        f.assert_outside_untouched()
        assert not bool(f.is_sentinel().any()), "%s: a cell of the window was never written" % name
        assert torch.equal(f.window_bits(), packed_outs[name].window_bits()), \
            "%s differs between the framed and the packed call" % name
    for f in ins:
        f.assert_untouched()


def run_case(case, rows=3):
    shape = "%dx%d K=%d" % (case.n_in, case.n_out, case.K) + ("" if case.opt is None else " opt=%s" % (case.opt,))
    for family in ("integer", "real"):
        t0 = time.time()
        ref = hc.reference(case, family, rows)
        outs, ins = launch(case, ref["inputs"], packed=False)
        packed_outs, packed_ins = launch(case, ref["inputs"], packed=True)
        check_frames(outs, ins, packed_outs)
        for f in packed_ins:
            f.assert_untouched()
        worst = 0.0
        for name, frame in outs.items():
            want, bound = ref["outs"][name]
            got = host(frame).reshape(np.shape(want))
            r = hc.ratio(got, want, bound)
            worst = max(worst, r)
        report(case.entry, shape, family, worst, time.time() - t0)
        if family == "integer":
            assert worst == 0.0, "%s: the integer family is not reproduced bit for bit" % hc.case_id(case)
        else:
            assert worst <= 1.0, "%s: |got - ref| reaches %.3g of the derived bound" % (hc.case_id(case), worst)


def _params(group):
    return [pytest.param(c, id=hc.case_id(c)) for c in hc.row_cases(group)]


@pytest.mark.parametrize("case", _params("operators"))
def test_operators(case):
    run_case(case)


@pytest.mark.parametrize("case", _params("outputs"))
def test_outputs(case):
    run_case(case)


@pytest.mark.parametrize("case", _params("statistics"))
def test_statistics_cost_lambda_max(case):
    run_case(case)


# ---- Lipschitz constants -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gram_ref(K, N):
    taps = hc.gram_taps(K, N)
    return taps, hc.gram_reference(taps, N)


def run_gram(K, N):
    t0 = time.time()
    taps_h, want = gram_ref(K, N)
    res = []
    for packed in (False, True):
        taps = frames.frame2d("taps_pp", taps_h.shape[0], K, F64, DEV, fill=taps_h, packed=packed).snapshot()
        out = frames.frame1d("out", taps_h.shape[0], F64, DEV, packed=packed).snapshot()
        frames.gram_frobenius(taps, K, N, out)
        torch.cuda.synchronize()
        taps.assert_untouched()
        out.assert_outside_untouched()
        res.append(out)
    assert torch.equal(res[0].window_bits(), res[1].window_bits())
    got = host(res[0])
    rel = float((np.abs(got.astype(hc.LD) - want) / want).max())
    report("gram_frobenius", "K=%d N=%d" % (K, N), "real", rel / hc.GRAM_RTOL, time.time() - t0)
    assert np.isfinite(got).all() and rel <= hc.GRAM_RTOL, (K, N, rel)


@pytest.mark.parametrize("K,N", hc.GRAM_CASES)
def test_gram_frobenius(K, N):
    run_gram(K, N)


def run_spectral(case, rows=3):
    t0 = time.time()
    ref = hc.spectral_reference(case, rows)
    res = []
    for packed in (False, True):
        x0 = frames.frame2d("W", rows, case.N, F64, DEV, fill=ref["x0"], packed=packed).snapshot()
        taps = frames.frame2d("taps_pp", rows, case.K, F64, DEV, fill=ref["taps"], packed=packed).snapshot()
        out = frames.frame1d("out", 2 * rows, F64, DEV, packed=packed).snapshot()
        frames.spectral_radius_pp(x0, taps, case.K, case.nb_iter, ref["tol"], out)
        torch.cuda.synchronize()
        x0.assert_untouched()
        taps.assert_untouched()
        out.assert_outside_untouched()
        res.append(out)
    assert torch.equal(res[0].window_bits(), res[1].window_bits())
    got = host(res[0]).reshape(rows, 2)
    for r in range(rows):                                   # the single-row entry point: the bits of row r
        x1 = frames.frame1d("x0", case.N, F64, DEV, fill=ref["x0"][r]).snapshot()
        t1 = frames.frame1d("taps", case.K, F64, DEV, fill=ref["taps"][r]).snapshot()
        o1 = frames.frame1d("out", 2, F64, DEV).snapshot()
        frames.spectral_radius(x1, t1, case.nb_iter, ref["tol"], o1)
        torch.cuda.synchronize()
        x1.assert_untouched()
        t1.assert_untouched()
        o1.assert_outside_untouched()
        assert np.array_equal(host(o1).view(np.int64), got[r].view(np.int64)), "row %d: pb_spectral_radius_pp differs" % r
    rel = float((np.abs(got[:, 0].astype(hc.LD) - ref["rho"]) / ref["rho"]).max())
    report("spectral_radius_pp", "N=%d K=%d nb_iter=%d tol=%.3g steps=%s" % (case.N, case.K, case.nb_iter, ref["tol"],
                                                                          ref["steps"].tolist()), "real",
           rel / hc.RHO_RTOL, time.time() - t0)
    assert (got[:, 1] == ref["steps"]).all(), (got[:, 1], ref["steps"])
    assert rel <= hc.RHO_RTOL, (case, rel)


@pytest.mark.parametrize("case", hc.spectral_cases(), ids=lambda c: "N%d-K%d-it%d" % c)
def test_spectral_radius(case):
    run_spectral(case)


# ---- pb_inf_norm ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", hc.INF_NORM_N)
def test_inf_norm(n):
    t0 = time.time()
    x_h = hc.inf_norm_inputs(n)
    want = hc.inf_norm_reference(x_h)
    res = []
    for packed in (False, True):
        x = frames.frame2d("W", 3, n, F64, DEV, fill=x_h, packed=packed).snapshot()
        out = frames.frame2d("out", 3, n, F64, DEV, packed=packed).snapshot()
        frames.inf_norm(x, out)
        torch.cuda.synchronize()
        x.assert_untouched()
        out.assert_outside_untouched()
        res.append(out)
    assert torch.equal(res[0].window_bits(), res[1].window_bits())
    r = hc.ratio(host(res[0]), want, None)
    report("inf_norm", "n=%d" % n, "real", r, time.time() - t0)
    assert r == 0.0 and (want[1] == 0.0).all()


# ---- the longest rows the launchers admit ---------------------------------------------------------------------------------
LIMIT_ENTRIES = hc.ROW_ENTRIES + ("spectral_radius_pp",) + tuple("gram_frobenius-K%d" % K for K, _ in hc.GRAM_LIMIT_CASES)


@pytest.mark.parametrize("entry", LIMIT_ENTRIES)
def test_limit_shape_runs_and_the_next_length_is_refused(entry):
    """Each launcher documents rows of up to LDS_DOUBLES_MAX doubles as supported: the limit length must run and be right
    (two rows, the same references and bounds), one scan more must be refused with `exceeds LDS`."""
    from pybold_amd._lib import PyboldHipError
    if entry.startswith("gram_frobenius"):                  # (2000 taps: the O(N^2) kernel; 30: the closed form)
        run_gram(int(entry.split("-K")[1]), hc.GRAM_LIMIT_N)
        with pytest.raises(PyboldHipError, match="exceeds LDS"):
            taps = frames.frame2d("taps_pp", 2, hc.LIMIT_K, F64, DEV, fill=hc.gram_taps(hc.LIMIT_K, hc.GRAM_LIMIT_N))
            frames.gram_frobenius(taps, hc.LIMIT_K, hc.GRAM_LIMIT_N + 1, frames.frame1d("out", 2, F64, DEV))
        return
    if entry == "spectral_radius_pp":
        n, K = hc.limit_shape(entry)
        run_spectral(hc.Spectral(n, K, 2), rows=2)
        x0 = frames.frame2d("W", 2, n + 1, F64, DEV, fill=np.ones((2, n + 1)))
        taps = frames.frame2d("taps_pp", 2, K, F64, DEV, fill=np.ones((2, K)))
        with pytest.raises(PyboldHipError, match="exceeds LDS"):
            frames.spectral_radius_pp(x0, taps, K, 2, 1.0e-6, frames.frame1d("out", 4, F64, DEV))
        x1 = frames.frame1d("x0", n + 1, F64, DEV, fill=np.ones(n + 1))
        with pytest.raises(PyboldHipError, match="exceeds LDS"):
            frames.spectral_radius(x1, frames.frame1d("taps", K, F64, DEV, fill=np.ones(K)), 2, 1.0e-6,
                                   frames.frame1d("out", 2, F64, DEV))
        return
    case = hc.limit_case(entry)
    assert (case.n_in, case.K) == hc.limit_shape(entry)
    run_case(case, rows=2)
    over = case._replace(n_in=case.n_in + 1, n_out=case.n_out + 1)
    assert (over.n_in, over.K) == hc.over_shape(entry)
    with pytest.raises(PyboldHipError, match="exceeds LDS"):
        launch(over, hc.make_inputs(over, "integer", 2, M=1), packed=False)
