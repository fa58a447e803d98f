"""GPU tests of the opt-in conditioning guard for solves whose HRF lives in device memory: `solver.conditioning_marks`,
`fista_solve_pp(guard=True)` with one HRF for all rows and one per row, `fista_solve_grouped(guard=True)`, the
blind-deconvolution loops with the switch, and capture into a graph.

Input of the solve tests, 64 rows: the 16 families of tests/test_gpu_round5.py::test_ill_conditioned_series_are_solved_in_float64
restated at the case's length (rows 0..15), the same again (16..31), and 32 block series at SNR 1 dB (32..63).  The float64
oracle solves every case once per (lambda, start) and is shared by the guarded and the unguarded comparison.

Figures of a run (worst error per family, guard on and off): profiles/pp_guard.txt.
"""
import os

import numpy as np
import pytest
import torch

from oracle import pybold_oracle as orc

pytestmark = pytest.mark.gpu

EPS = 1.0e-5                     # the project's eps
GAMMA_F64 = 1.0e-2               # csrc/dispatch.h: PART_GAMMA_F64
FAMILY_NAMES = ["ordinary", "white noise", "alternating", "period 3", "period 4", "period 6", "period 10", "diff noise",
                "diff2 noise", "alt + 1e-3 y", "alt + 1e-2 y", "alt + 0.1 y", "modulated alt", "ones", "37 alt", "1e-3 alt"]
N_FAM, N_BLOCK = 16, 32


def gamma_matrix_pipe(n, k):     # csrc/dispatch.h: part_gamma_matrix_pipe
    if k > 33 or n <= 310:
        return 7.0e-2
    return 3.0e-2 if n <= 640 else 2.0e-2


def rel_rows(a, b):
    return np.linalg.norm(a - b, axis=1) / (np.linalg.norm(b, axis=1) + 1e-300)


def hrf_for(k, delta=1.0):
    h = orc.spm_hrf(delta, 1.0, float(k), False)[0][:k].copy()
    assert len(h) == k
    return h


@pytest.fixture(scope="module")
def solver():
    from pybold_amd import solver as s
    return s


_BATCHES = {}


def batch_for(n, k):
    """(Y float32 numpy (64, n), the shared HRF)."""
    if (n, k) in _BATCHES:
        return _BATCHES[(n, k)]
    from pybold_amd import data
    hrf = hrf_for(k)
    ev, avg = (5, 12.0) if n >= 250 else (2, 8.0)
    Yb, _, _ = data.gen_rnd_bloc_bold_batch(N_BLOCK + 1, dur=(n + 0.5) / 60.0, tr=1.0, hrf=hrf, nb_events=ev, avg_dur=avg, std_dur=1.0,
                                            snr=1.0, seed=100 + n + k, device="cuda")
    Yb = Yb.cpu().numpy().astype(np.float64)
    assert Yb.shape == (N_BLOCK + 1, n)
    y = Yb[0]                                                    # the ordinary series of the families ...
    if n == 300:                                                 # ... at 300 scans the golden series of the test restated here
        y = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "case1.npz"))["y"].astype(np.float64)
        assert y.shape == (300,)
    t = np.arange(n)
    rng = np.random.RandomState(1)
    alt = np.where(t % 2 == 0, 1.0, -1.0)
    hp = rng.randn(n)
    fams = [y, rng.randn(n), alt, np.sin(2 * np.pi * t / 3), np.sin(2 * np.pi * t / 4), np.sin(2 * np.pi * t / 6),
            np.sin(2 * np.pi * t / 10), np.diff(np.r_[0.0, hp]), np.diff(np.r_[0.0, 0.0, hp], n=2), alt + 1e-3 * y,
            alt + 1e-2 * y, alt + 0.1 * y, alt * (1 + np.sin(2 * np.pi * t / 100)), np.ones(n), 37.0 * alt, 1e-3 * alt]
    assert len(fams) == N_FAM == len(FAMILY_NAMES)
    Y = np.concatenate([np.stack(fams), np.stack(fams), Yb[1:]]).astype(np.float32)
    _BATCHES[(n, k)] = (Y, hrf)
    return _BATCHES[(n, k)]


def gamma2(Y, taps_rows):
    """float64 restatement of the statistic: lambda_max / (||y||_2 sum_{t<N} |cumsum(h)[t]| / sqrt(N)) per row."""
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[1]
    out = np.zeros(len(Y))
    for p in range(len(Y)):
        h = taps_rows[p]
        lm = np.abs(orc.integ_adj(orc.causal_corr(h, Y[p:p + 1]))).max()
        c = np.cumsum(np.r_[h, np.zeros(max(n - len(h), 0))])[:n]
        den = np.linalg.norm(Y[p]) * np.abs(c).sum() / np.sqrt(n)
        out[p] = lm / den if den > 0 else np.inf
    return out


def marks_from_gamma(g, n, k):
    return np.where(g < GAMMA_F64, 2, np.where(g < gamma_matrix_pipe(n, k), 1, 0))


# HRF layouts of a case: every row's taps (64, K) for the oracle, and what the library is given
PER_ROW_DILATIONS = np.linspace(0.6, 1.9, 8)
PARCEL_DILATIONS = [0.7, 0.7, 1.3, 1.8]      # (the two copies of the families, parcels 0 and 1, meet the same HRF)
OFFSETS = np.array([0, 16, 32, 48, 64])


def rows_taps(kind, k):
    if kind == "shared":
        return np.tile(hrf_for(k), (64, 1))
    if kind == "perrow":                             # (the two copies of a family share a dilation: rows p and p + 16)
        return np.stack([hrf_for(k, PER_ROW_DILATIONS[(p % 16) % 8]) for p in range(64)])
    return np.stack([hrf_for(k, PARCEL_DILATIONS[p // 16]) for p in range(64)])


CASES = [("shared", 129, 20, "mfma"), ("shared", 300, 20, "mfma"), ("shared", 310, 33, "mfma"), ("shared", 311, 30, "mfma2"),
         ("shared", 600, 28, "mfma2"), ("shared", 600, 40, "mfma2"), ("shared", 1200, 28, "mfma2"),
         ("perrow", 300, 20, None), ("perrow", 600, 28, None), ("perrow", 700, 28, None),
         ("grouped", 300, 20, "mfma"), ("grouped", 600, 28, "gsplit_mfma"), ("grouped", 1200, 28, "gsplit_mfma")]


def oracle_solve(Y64, T, lam, steps, n_iter, W0=None):
    """Rows grouped by HRF, each group one call of the C float64 oracle."""
    from oracle import c_oracle
    out = np.zeros_like(Y64)
    keys = {}
    for p in range(len(Y64)):
        keys.setdefault(T[p].tobytes(), []).append(p)
    for rows in keys.values():
        rows = np.array(rows)
        lb = lam[rows] if np.ndim(lam) > 0 else lam
        W, _, _ = c_oracle.fista_batch(Y64[rows], T[rows[0]], lb, float(steps[rows[0]]), n_iter,
                                       W0=None if W0 is None else W0[rows], threads=8)
        out[rows] = W
    return out


def steps_for(T, n):
    """1 / ||A^T A||_F of every row's HRF (orc.gram_lipschitz: the z-steps' own constant), one norm per distinct HRF."""
    seen = {}
    for h in T:
        if h.tobytes() not in seen:
            seen[h.tobytes()] = 1.0 / orc.gram_lipschitz(h, n)
    return np.array([seen[h.tobytes()] for h in T])


def device_args(solver, kind, T, steps):
    """The HRFs and steps of a layout in device memory (built once: nothing is uploaded inside a captured call)."""
    if kind == "shared":
        return dict(taps=torch.from_numpy(T[0]).cuda(), steps=torch.tensor([steps[0]], dtype=torch.float64, device="cuda"))
    if kind == "perrow":
        return dict(taps=torch.from_numpy(T).cuda(), steps=torch.from_numpy(steps).cuda())
    return dict(taps=torch.from_numpy(T[OFFSETS[:-1]]).cuda(), steps=torch.from_numpy(steps[OFFSETS[:-1]]).cuda(),
                po=solver.ParcelOffsets(OFFSETS, torch.device("cuda", torch.cuda.current_device())))


def library_solve(solver, kind, Yd, dv, lam, n_iter, force, guard, W0=None, guard_work=None, inplace=False):
    lam_arg = torch.from_numpy(lam).cuda() if np.ndim(lam) > 0 else float(lam)
    if kind == "grouped":
        return solver.fista_solve_grouped(Yd, dv["taps"], dv["steps"], dv["po"], lam_arg, n_iter, W0=W0, force=force, inplace=inplace,
                                          guard_work=guard_work, guard=guard)
    return solver.fista_solve_pp(Yd, dv["taps"], dv["steps"], lam_arg, n_iter, W0=W0, force=force, inplace=inplace,
                                 guard_work=guard_work, guard=guard)


def outputs_err(solver, W, T, ref):
    """Worst of diff_z, z and x per row against the oracle's."""
    X, Z = solver.fista_outputs_pp(W, torch.from_numpy(T).cuda())
    zr = np.cumsum(ref, axis=1)
    xr = np.stack([orc.causal_conv(T[p], zr[p:p + 1])[0] for p in range(len(ref))])
    return np.maximum(np.maximum(rel_rows(W.cpu().numpy(), ref), rel_rows(Z.cpu().numpy(), zr)), rel_rows(X.cpu().numpy(), xr))


@pytest.mark.parametrize("kind,n,k,force", CASES)
def test_guarded_solves_hold_eps_and_leave_ordinary_rows_alone(solver, kind, n, k, force):
    """lambda in {0, 0.05 lambda_max, 1}, 500 iterations at the z-steps' step 1 / ||A^T A||_F, cold start and a warm start of
    2 x 250 iterations in place.  guard=True: every row within 1e-5 of the float64 oracle on diff_z, z and x, the two
    copies of a family bit-equal, n_done >= 0; the 32 block rows carry the bits and n_done of the unguarded call.
    guard=False on the same input: the worst family exceeds 1e-5 -- on 11 of the 13 routes (1.1e-5 at 300 / 20 shared ..
    6.7e-3 at 311 / 30); at 129 / 20 shared (8.9e-6) and 300 / 20 per row (6.5e-6) it stays just below, see
    OFF_STAYS_BELOW_EPS.  (The bounds of the guard were calibrated with deconv's step 1 / (0.9 rho), not with this one: a
    family that misses eps under the guard is reported, the bounds stay.)  310 / 33 with one HRF for all rows has no
    matrix-pipe form in pb_fista_solve_pp (no two-problems-per-row entry beyond 32 taps, which that route starts from):
    its main form is a vector form and the call builds no mark-1 list; the route query says so and is asserted."""
    Y, _ = batch_for(n, k)
    T = rows_taps(kind, k)
    steps = steps_for(T, n)
    dv = device_args(solver, kind, T, steps)
    Yd = torch.from_numpy(Y).cuda()
    Y64 = Y.astype(np.float64)
    # the main form really is the matrix pipe where the library has one for the layout
    if kind == "shared":
        assert solver.pp_uses_matrix_pipe(n, k, 64, True, None, force) == (not (n <= 310 and k > 32)), (n, k)
    elif kind == "perrow":
        assert not solver.pp_uses_matrix_pipe(n, k, 64, False, None, force)
    else:
        assert solver.grouped_route(OFFSETS, n, k, force) == ({"mfma": 4, "gsplit_mfma": 5 if n <= 640 else 6}[force], 4, 64)
    assert solver.guard_supported(n, k) in (1, 2, 3, 4)
    lmax = np.array([np.abs(orc.integ_adj(orc.causal_corr(T[p], Y64[p:p + 1]))).max() for p in range(64)])
    worst_on = np.zeros(64)
    worst_off = np.zeros(64)
    work = torch.empty((solver.guard_work_len(64, n),), dtype=torch.int32, device="cuda")
    counts = None
    for lam in (0.0, 0.05 * lmax, 1.0):
        ref_cold = oracle_solve(Y64, T, lam, steps, 500)
        ref_half = oracle_solve(Y64, T, lam, steps, 250)
        ref_warm = oracle_solve(Y64, T, lam, steps, 250, W0=ref_half)
        for start, ref in (("cold", ref_cold), ("warm", ref_warm)):
            res = {}
            for guard in (True, False):
                if start == "cold":
                    W, nd = library_solve(solver, kind, Yd, dv, lam, 500, force, guard, guard_work=work if guard else None)
                else:
                    W = torch.zeros((64, n), dtype=torch.float64, device="cuda")
                    for _ in range(2):
                        W, nd = library_solve(solver, kind, Yd, dv, lam, 250, force, guard, W0=W, inplace=True,
                                              guard_work=work if guard else None)
                res[guard] = (W, nd, outputs_err(solver, W, T, ref))
                if guard:
                    counts = solver.guard_counts(work)
            Wg, ndg, eg = res[True]
            Wu, ndu, eu = res[False]
            worst_on = np.maximum(worst_on, eg)
            worst_off = np.maximum(worst_off, eu)
            print("%s N=%d K=%d %s lambda=%s: guard on worst %.2e (row %d), off worst %.2e (row %d), listed %s"
                  % (kind, n, k, start, "vector" if np.ndim(lam) else lam, eg.max(), eg.argmax(), eu.max(), eu.argmax(), counts))
            assert int(ndg.min()) >= 0
            assert torch.equal(Wg[:N_FAM], Wg[N_FAM:2 * N_FAM])               # (the same series anywhere in the batch)
            assert torch.equal(Wg[2 * N_FAM:], Wu[2 * N_FAM:]) and torch.equal(ndg[2 * N_FAM:], ndu[2 * N_FAM:])
    fam_on = np.maximum(worst_on[:N_FAM], worst_on[N_FAM:2 * N_FAM])
    fam_off = np.maximum(worst_off[:N_FAM], worst_off[N_FAM:2 * N_FAM])
    g2 = gamma2(Y64[:N_FAM], T[:N_FAM])
    for f in range(N_FAM):
        print("  family %-14s gamma_2 %.2e  guard on %.2e  off %.2e" % (FAMILY_NAMES[f], g2[f], fam_on[f], fam_off[f]))
    print("  block rows: guard on %.2e  off %.2e" % (worst_on[2 * N_FAM:].max(), worst_off[2 * N_FAM:].max()))
    assert counts["float64"] >= 2 * 8                      # the families far below the float64 bound, both copies
    assert worst_on.max() < EPS, [(FAMILY_NAMES[f], g2[f], fam_on[f]) for f in range(N_FAM) if fam_on[f] >= EPS]
    # guard off: the worst family misses eps -- the guard is what holds it.  Two routes are the exception at this step
    # constant (500 iterations of 1 / ||A^T A||_F move an iterate less far than deconv's step): their measured worst is kept
    # here and in profiles/pp_guard.txt, and nothing is asserted of their unguarded error.
    if (kind, n, k) in OFF_STAYS_BELOW_EPS:
        print("  guard off stays below eps on this route: %.2e (recorded %.2e)" % (fam_off.max(), OFF_STAYS_BELOW_EPS[(kind, n, k)]))
    else:
        assert fam_off.max() > EPS, fam_off.max()


# routes on which the unguarded worst family was measured BELOW eps (MI355X, this test's input): the value measured
OFF_STAYS_BELOW_EPS = {("shared", 129, 20): 8.9e-6, ("perrow", 300, 20): 6.5e-6}


# gamma_2 of the families at 300 scans with the 20-tap SPM HRF, float64 on the CPU: alternating, period 3 / 4 / 6, both
# differenced noises, alt + 1e-3 y, alt + 1e-2 y, modulated alt, 37 alt, 1e-3 alt 1.5e-3 .. 5.2e-3 (mark 2); alt + 0.1 y 2.9e-2
# (mark 1); ones 1.0, the ordinary series 8.8e-2 or more (mark 0); white noise 7.1e-2 and the period-10 sinusoid 1.2e-2 sit on a
# bound and are left out of the equality.
MARKS_300_20 = {"alternating": 2, "period 3": 2, "period 4": 2, "period 6": 2, "diff noise": 2, "diff2 noise": 2, "alt + 1e-3 y": 2,
                "alt + 1e-2 y": 2, "modulated alt": 2, "37 alt": 2, "1e-3 alt": 2, "alt + 0.1 y": 1, "ones": 0}


@pytest.mark.parametrize("n,k", [(300, 20), (600, 28), (1200, 28)])
def test_marks_equal_a_float64_restatement_away_from_the_bounds(solver, n, k):
    """`solver.conditioning_marks` for the three HRF layouts against gamma_2 in float64 NumPy, on the rows whose gamma_2 is
    at least 25 % clear of both bounds (the float32 pass may class a series on a bound either way); an all-zero row is 0."""
    Y, _ = batch_for(n, k)
    Y = np.concatenate([Y, np.zeros((1, n), dtype=np.float32)])
    Yd = torch.from_numpy(Y).cuda()
    bounds = (GAMMA_F64, gamma_matrix_pipe(n, k))
    for kind in ("shared", "perrow", "grouped"):
        T = np.concatenate([rows_taps(kind, k), rows_taps(kind, k)[-1:]])
        if kind == "shared":
            got = solver.conditioning_marks(Yd, torch.from_numpy(T[0]).cuda())
        elif kind == "perrow":
            got = solver.conditioning_marks(Yd, torch.from_numpy(T).cuda())
        else:
            off = np.r_[OFFSETS[:-1], 65]
            got = solver.conditioning_marks(Yd, torch.from_numpy(T[off[:-1]]).cuda(), offsets=off)
        got = got.cpu().numpy()
        g = gamma2(Y, T)
        clear = np.all([(g < 0.75 * b) | (g > 1.25 * b) for b in bounds], axis=0)
        assert clear[-1] and got[-1] == 0                                     # the all-zero row
        want = marks_from_gamma(g, n, k)
        print("marks %s N=%d K=%d: %d of 65 rows clear of the bounds; gamma_2 of the families %s"
              % (kind, n, k, int(clear.sum()), " ".join("%.1e" % v for v in g[:N_FAM])))
        assert clear[2 * N_FAM:].all() and (want[2 * N_FAM:] == 0).all()      # block signals: far above the bounds
        assert clear[:N_FAM].sum() >= 10
        assert np.array_equal(got[clear], want[clear]), (kind, np.nonzero(clear & (got != want))[0], g[clear & (got != want)])
        if (n, k, kind) == (300, 20, "shared"):
            for name, mark in MARKS_300_20.items():
                f = FAMILY_NAMES.index(name)
                assert clear[f], (name, g[f])             # (the margin itself, before the comparison)
                assert got[f] == mark and got[N_FAM + f] == mark, (name, g[f], got[f])
            assert 8.0e-2 < g[0] < 1.0e-1 and (not clear[0] or got[0] == 0)       # the golden series: 8.8e-2


def test_guarded_calls_replay_from_a_graph_bit_for_bit(solver):
    """One guarded `fista_solve_pp` call (shared HRF, the matrix pipe as its main form) and one guarded grouped call,
    captured with `torch.cuda.graph` and replayed once: the bits of the eager call."""
    n, k = 300, 20
    Y, hrf = batch_for(n, k)
    Yd = torch.from_numpy(Y).cuda()
    rng = np.random.RandomState(3)
    W0 = torch.from_numpy(0.01 * rng.randn(64, n)).cuda()
    for kind in ("shared", "grouped"):
        T = rows_taps(kind, k)
        dv = device_args(solver, kind, T, steps_for(T, n))
        work = torch.empty((solver.guard_work_len(64, n),), dtype=torch.int32, device="cuda")
        We, nde = library_solve(solver, kind, Yd, dv, 1.0, 100, "mfma", True, W0=W0.clone(), inplace=True, guard_work=work)
        eager_counts = solver.guard_counts(work)
        assert eager_counts["float64"] > 0 and eager_counts["vector"] > 0
        torch.cuda.synchronize()
        Ws = W0.clone()
        work.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            Wc, ndc = library_solve(solver, kind, Yd, dv, 1.0, 100, "mfma", True, W0=Ws, inplace=True, guard_work=work)
        assert Wc.data_ptr() == Ws.data_ptr()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(Wc, We) and torch.equal(ndc, nde), kind
        assert solver.guard_counts(work) == eager_counts


def test_an_empty_batch_reports_no_listed_rows(solver):
    """A guarded call on no rows launches nothing (a rank's shard may be empty): the counts read 0, not what the buffer held."""
    Y, hrf = batch_for(300, 20)
    taps = torch.from_numpy(hrf).cuda()
    step = torch.tensor([1.0 / orc.gram_lipschitz(hrf, 300)], dtype=torch.float64, device="cuda")
    W, nd = solver.fista_solve_pp(torch.from_numpy(Y[:0]).cuda(), taps, step, 1.0, 10, guard=True)
    assert W.shape == (0, 300) and nd.shape == (0,)
    work = solver.guard_work_buffer(0, 300, W.device)
    solver.fista_solve_pp(torch.from_numpy(Y[:0]).cuda(), taps, step, 1.0, 10, guard_work=work, guard=True)
    assert solver.guard_counts(work) == {"float64": 0, "vector": 0}


# ---- the blind-deconvolution loops ------------------------------------------------------------------------------------
T_R, DUR, N_LOOP = 1.0, 20.0, 300


class _OneProcess:                                   # the oracle loop never talks to other ranks
    world_size, rank = 1, 0

    @staticmethod
    def allreduce_(t):
        return t


@pytest.fixture(scope="module")
def loop_batch(solver):
    Y, _ = batch_for(N_LOOP, 20)
    Yd = torch.from_numpy(Y).cuda()
    h2 = orc.spm_hrf(2.0, T_R, DUR, False)[0]
    lm = solver.lambda_max(Yd[2 * N_FAM:], h2)
    return Yd, 0.05 * float(lm.min())


def test_bd_shared_with_the_guard(solver, loop_batch, monkeypatch):
    """3 x 50 iterations: theta per outer iteration against the float64 oracle loop within the bound of
    tests/test_gpu_parcels.py (twice the |dtheta| of the unguarded library loop against the same oracle, or 1e-6);
    d['guard'] holds the counts of the last z-step; guard off = keyword absent, bit for bit; a captured loop too."""
    from oracle.shared_ops import OracleOps
    from pybold_amd import distributed
    monkeypatch.delenv("PYBOLD_AMD_PP_GUARD", raising=False)
    Yd, lbda = loop_batch
    kw = dict(lbda=lbda, theta_0=2.0, hrf_dur=DUR, nb_iter=3, nb_inner=50)
    Wo, ho, do = distributed.bd_shared(Yd.cpu(), T_R, ops=OracleOps(N_LOOP, T_R, DUR), comm=_OneProcess(), **kw)
    W0, h0, d0 = distributed.bd_shared(Yd, T_R, **kw)
    Wf, hf, df = distributed.bd_shared(Yd, T_R, guard=False, **kw)
    assert "guard" not in d0 and "guard" not in df
    assert torch.equal(W0, Wf) and np.array_equal(d0["theta"], df["theta"]) and np.array_equal(d0["J"], df["J"])
    Wg, hg, dg = distributed.bd_shared(Yd, T_R, guard=True, **kw)
    assert set(dg["guard"]) == {"float64", "vector"} and dg["guard"]["float64"] >= 16
    th_o = np.asarray(do["theta"], dtype=np.float64)
    worst_plain = float(np.abs(np.asarray(d0["theta"]) - th_o).max())
    worst_guard = float(np.abs(np.asarray(dg["theta"]) - th_o).max())
    print("bd_shared 3 x 50, 64 rows: |dtheta| against the oracle loop %.3e guarded, %.3e unguarded; listed %s"
          % (worst_guard, worst_plain, dg["guard"]))
    assert worst_guard <= max(2.0 * worst_plain, 1e-6)
    # the environment variable is the same switch
    monkeypatch.setenv("PYBOLD_AMD_PP_GUARD", "1")
    We, he, de = distributed.bd_shared(Yd, T_R, **kw)
    assert torch.equal(We, Wg) and de["guard"] == dg["guard"]
    monkeypatch.delenv("PYBOLD_AMD_PP_GUARD")
    g = distributed.BdSharedGraph(Yd, T_R, guard=True, **kw)
    g.launch()
    Wc, hc, dc = g.result()
    assert g.graph is not None, g.fallback
    assert torch.equal(Wc, Wg) and np.array_equal(dc["theta"], dg["theta"]) and dc["guard"] == dg["guard"]


def test_bd_parcels_with_the_guard(solver, loop_batch, monkeypatch):
    """4 parcels of 16 rows, 3 x 50 iterations, every z-step forced onto the matrix pipe: theta per outer iteration and
    parcel against the oracle loop of the parcel's rows alone, within the bound of tests/test_gpu_parcels.py."""
    import pybold_amd
    from oracle.shared_ops import OracleOps
    from pybold_amd import distributed
    monkeypatch.delenv("PYBOLD_AMD_PP_GUARD", raising=False)
    Yd, lbda = loop_batch
    labels = np.repeat([3, 1, 2, 0], 16)
    kw = dict(lbda=lbda, theta_0=2.0, hrf_dur=DUR, nb_iter=3, nb_inner=50)
    out0 = pybold_amd.bd_parcels(Yd, labels, T_R, force="mfma", **kw)
    outf = pybold_amd.bd_parcels(Yd, labels, T_R, force="mfma", guard=False, **kw)
    assert "guard" not in out0[4] and "guard" not in outf[4]
    assert torch.equal(out0[2], outf[2]) and np.array_equal(out0[4]["theta"], outf[4]["theta"])
    X, Z, W, H, d = pybold_amd.bd_parcels(Yd, labels, T_R, force="mfma", guard=True, **kw)
    assert set(d["guard"]) == {"float64", "vector"} and d["guard"]["float64"] >= 16
    worst_guard = worst_shared = 0.0
    for g, lab in enumerate(d["labels"]):
        rows = np.nonzero(labels == lab)[0]
        Yp = Yd[torch.from_numpy(rows).cuda()].contiguous()
        _, _, do = distributed.bd_shared(Yp.cpu(), T_R, ops=OracleOps(N_LOOP, T_R, DUR), comm=_OneProcess(), **kw)
        _, _, ds = distributed.bd_shared(Yp, T_R, **kw)
        th_o = np.asarray(do["theta"], dtype=np.float64)
        worst_shared = max(worst_shared, float(np.abs(np.asarray(ds["theta"]) - th_o).max()))
        worst_guard = max(worst_guard, float(np.abs(d["theta"][:, g] - th_o).max()))
    print("bd_parcels 3 x 50, 4 parcels of 16: |dtheta| against the per-parcel oracle loops %.3e guarded; bd_shared on each parcel "
          "alone, unguarded: %.3e; listed %s" % (worst_guard, worst_shared, d["guard"]))
    assert worst_guard <= max(2.0 * worst_shared, 1e-6)


def test_bd_on_a_batch_takes_the_switch_from_the_environment(solver, loop_batch, monkeypatch):
    """`bd` keeps the reference's signature: PYBOLD_AMD_PP_GUARD is its only switch for 2-D input.  Two outer iterations:
    off = variable absent, bit for bit; on: d['guard'] is there (one HRF per row: no matrix pipe, no vector list), the two
    copies of a family stay bit-equal, and -- rows are independent in this loop and every z-step is guarded -- the block
    rows, never marked, carry the bits of the unguarded run through the whole loop.  theta after the loop against the float64
    single-voxel oracle loop (`orc.bd`, L-BFGS-B in its theta-step) on three rows the guard re-solves and two block rows:
    within the bound of tests/test_gpu_parcels.py, twice the |dtheta| of the unguarded loop against the same oracle or 1e-6."""
    import pybold_amd
    Yd, lbda = loop_batch
    kw = dict(lbda=lbda, theta_0=1.0, hrf_dur=DUR, nb_iter=2)
    monkeypatch.delenv("PYBOLD_AMD_PP_GUARD", raising=False)
    x0, z0, w0, h0, d0 = pybold_amd.bd(Yd, T_R, **kw)
    monkeypatch.setenv("PYBOLD_AMD_PP_GUARD", "0")
    x1, z1, w1, h1, d1 = pybold_amd.bd(Yd, T_R, **kw)
    assert "guard" not in d0 and "guard" not in d1
    assert torch.equal(torch.as_tensor(w0), torch.as_tensor(w1)) and np.array_equal(d0["theta"], d1["theta"])
    monkeypatch.setenv("PYBOLD_AMD_PP_GUARD", "1")
    xg, zg, wg, hg, dg = pybold_amd.bd(Yd, T_R, **kw)
    assert set(dg["guard"]) == {"float64", "vector"} and dg["guard"]["float64"] >= 16 and dg["guard"]["vector"] == 0
    wg, w0 = torch.as_tensor(wg), torch.as_tensor(w0)
    assert torch.equal(wg[2 * N_FAM:], w0[2 * N_FAM:]) and np.array_equal(dg["theta"][2 * N_FAM:], d0["theta"][2 * N_FAM:])
    assert torch.equal(wg[:N_FAM], wg[N_FAM:2 * N_FAM])
    marks = solver.conditioning_marks(Yd, torch.as_tensor(hg).cuda().double().contiguous()).cpu().numpy()
    rows = [FAMILY_NAMES.index("alternating"), FAMILY_NAMES.index("period 3"), FAMILY_NAMES.index("diff noise"), 2 * N_FAM, 2 * N_FAM + 1]
    assert all(marks[r] == 2 for r in rows[:3]) and all(marks[r] == 0 for r in rows[3:])
    Yh = Yd.cpu().numpy().astype(np.float64)
    for r in rows:
        do = orc.bd(Yh[r], T_R, **kw)[4]
        th_o = float(do["theta"][-1])
        e_plain, e_guard = abs(float(d0["theta"][r]) - th_o), abs(float(dg["theta"][r]) - th_o)
        print("bd 2-D row %d (mark %d): theta oracle %.8f, |dtheta| guarded %.3e, unguarded %.3e" % (r, marks[r], th_o, e_guard, e_plain))
        assert e_guard <= max(2.0 * e_plain, 1e-6), (r, e_guard, e_plain)
