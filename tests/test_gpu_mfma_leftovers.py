"""GPU tests of fista_mfma_row_kernel (pybold_amd/csrc/fista_mfma_row.h): one series per wave on the matrix pipe, the
kernel that takes the dense rows the whole rounds of a partitioned call leave.

1. The kernel alone (`force="mfma_row"`: every row on it, no re-solve) against the float64 oracle (oracle/c_oracle.py):
   N in {129, 160, 161, 300, 310, 320} x K in {1, 2, 30, 32, 33} x P in {1, 5, 70}, 40 iterations (once 500 at (300, 30)),
   cold start with a per-problem lambda vector and warm start with a scalar lambda, a lambda vector with y_rep = 2 -- every
   call on FRAMED buffers (tests/frames.py: padded ldy / ldw, guard rows, guards around the vectors), which must stay
   untouched outside their windows.  Every row within EPS = 1e-5 (relative l2 on diff_z) and n_done == n_iter.
   The lambdas are 0.01 lambda_max of their series: dense solutions, which the kernel's accuracy guard (threshold above
   0.02 max|w|: sparse solutions go back to the float32 operators) keeps.  The worst error is printed beside that of
   `force="mfma"` (the one-wave form, 310 scans at most) on the same rows.
2. Hand-back: a row whose warm start leaves the float16 range and a row at 0.9 lambda_max come back with n_done = -1 and
   their warm start bit for bit; as the left-overs of a default call of 16 384 + 5 problems the same rows are re-solved.
3. The wiring: a default (partitioned) call of 16 384 + 48 problems at (300, 30) whose 48 left-overs are half dense, half
   sparse -- the end of the dense class lies inside the one-problem-per-wave candidate's range."""
import numpy as np
import pytest
import torch

import frames
from oracle import c_oracle
from oracle import pybold_oracle as orc

pytestmark = pytest.mark.gpu

EPS = 1.0e-5
NI = 40
F32, F64, I32 = torch.float32, torch.float64, torch.int32
DENSE = 0.01                       # lambda / lambda_max of the dense rows

_worst = {"mfma_row": 0.0, "mfma": 0.0}


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def hrf_for(K):
    """SPM HRFs at TR 1 s cut to K taps (tests/test_gpu_layout.py); one and two taps: a gain, a delayed gain."""
    if K >= 20:
        h = orc.spm_hrf(1.0, 1.0, float(K), False)[0][:K].copy()
        assert len(h) == K
        return h
    return np.array([0.8]) if K == 1 else np.array([0.0, 0.6])


def rel_rows(a, b):
    return np.linalg.norm(a - b, axis=1) / (np.linalg.norm(b, axis=1) + 1e-300)


_ops = {}


def operator(N, K):
    """(hrf, step, T): T[t, s] = cumsum(h)[t - s], the operator K_h . cumsum as a matrix (lambda_max = ||T^T y||_inf)."""
    if (N, K) not in _ops:
        h = hrf_for(K)
        c = np.cumsum(np.r_[h, np.zeros(N - K)])
        idx = np.arange(N)[:, None] - np.arange(N)[None, :]
        T = np.where(idx >= 0, c[np.clip(idx, 0, N - 1)], 0.0)
        _ops[(N, K)] = (h, 1.0 / orc.gram_lipschitz(h, N), T)
    return _ops[(N, K)]


def block_series(V, N, K, seed):
    """Block signals at SNR 1 dB: five random steps in z, through the operator, plus white noise; float32."""
    h, _, T = operator(N, K)
    rng = np.random.RandomState(seed)
    dz = np.zeros((V, N))
    for v in range(V):
        dz[v, rng.choice(np.arange(5, N - 5), 10, replace=False)] = rng.choice([-1.0, 1.0], 10) * rng.uniform(0.5, 1.5, 10)
    X = dz @ T.T
    noise = rng.randn(V, N)
    noise *= (np.linalg.norm(X, axis=1) / np.linalg.norm(noise, axis=1) * 10.0 ** (-1.0 / 20.0))[:, None]
    Y = (X + noise).astype(np.float32)
    return Y, np.abs(Y.astype(np.float64) @ T).max(axis=1)


_cases = {}


def case(N, K):
    """70 rows of (N, K) with their oracle, cold (lambda vector) and warm (scalar lambda), computed once."""
    if (N, K) in _cases:
        return _cases[(N, K)]
    h, step, _ = operator(N, K)
    Y, lmax = block_series(70, N, K, seed=1000 * N + K)
    rng = np.random.RandomState(N + K)
    lam = DENSE * lmax
    lam_s = float(DENSE * lmax.min())
    W0 = 0.01 * rng.randn(70, N) * Y.std()
    Yd = Y.astype(np.float64)
    cold = c_oracle.fista_batch(Yd, h, lam, step, NI, threads=16)[0]
    warm = c_oracle.fista_batch(Yd, h, lam_s, step, NI, W0=W0, threads=16)[0]
    for a in (Y, lam, W0, cold, warm):
        a.setflags(write=False)
    _cases[(N, K)] = (h, step, Y, lam, lam_s, W0, cold, warm)
    return _cases[(N, K)]


def solve(Y, W0, hrf, step, n_iter, lam, force, y_rep=1, P=None, work=False):
    """pb_fista_solve_ex on framed buffers; W0 None: cold start.  Checks every guard band; returns (W, n_done, w frame)."""
    from pybold_amd import _lib
    d = dev()
    P = Y.shape[0] * y_rep if P is None else P
    N = Y.shape[1]
    y = frames.frame2d("y", Y.shape[0], N, F32, d, fill=Y)
    w = frames.frame2d("W", P, N, F64, d, fill=W0)
    nd = frames.frame1d("n_done", P, I32, d)
    lv = frames.frame1d("lbda", P, F64, d, fill=lam) if np.ndim(lam) else None
    wk = frames.frame1d("work", int(_lib.load().pb_fista_work_len(P, y_rep)), I32, d) if work else None
    fr = [f for f in (y, w, nd, lv, wk) if f is not None]
    for f in fr:
        f.snapshot()
    betas = frames.fista_solve_ex(y, w, hrf, step, n_iter, lbda=0.0 if lv is not None else float(lam), lbda_v=lv, n_done=nd,
                                  y_rep=y_rep, force=force, cold=W0 is None, work=wk)
    torch.cuda.synchronize()
    for f in (w, nd) + ((wk,) if wk is not None else ()):
        f.assert_outside_untouched()
    for f in (y, betas) + ((lv,) if lv is not None else ()):
        f.assert_untouched()
    return w.view.cpu().numpy(), nd.view.cpu().numpy(), w


# ---- 1: the kernel alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 5, 70])
@pytest.mark.parametrize("K", [1, 2, 30, 32, 33])
@pytest.mark.parametrize("N", [129, 160, 161, 300, 310, 320])
def test_kernel_alone_cold_and_warm(N, K, P):
    h, step, Y, lam, lam_s, W0, cold, warm = case(N, K)
    W, nd, _ = solve(Y[:P], None, h, step, NI, lam[:P], "mfma_row")
    e_cold = rel_rows(W, cold[:P]).max()
    assert (nd == NI).all(), nd
    W, nd, _ = solve(Y[:P], W0[:P], h, step, NI, lam_s, "mfma_row")
    e_warm = rel_rows(W, warm[:P]).max()
    assert (nd == NI).all(), nd
    e_ref = float("nan")
    if N <= 310:                                   # the one-wave form on the same rows
        Wm, ndm, _ = solve(Y[:P], None, h, step, NI, lam[:P], "mfma")
        e_ref = rel_rows(Wm, cold[:P]).max()
        _worst["mfma"] = max(_worst["mfma"], e_ref)
    _worst["mfma_row"] = max(_worst["mfma_row"], e_cold, e_warm)
    print("N=%d K=%d P=%d: mfma_row cold %.2e warm %.2e | mfma cold %.2e | worst so far: mfma_row %.2e, mfma %.2e"
          % (N, K, P, e_cold, e_warm, e_ref, _worst["mfma_row"], _worst["mfma"]))
    assert e_cold < EPS and e_warm < EPS


def test_kernel_alone_500_iterations():
    h, step, Y, lam, _, _, _, _ = case(300, 30)
    ref = c_oracle.fista_batch(Y[:5].astype(np.float64), h, lam[:5], step, 500, threads=16)[0]
    W, nd, _ = solve(Y[:5], None, h, step, 500, lam[:5], "mfma_row")
    Wm, _, _ = solve(Y[:5], None, h, step, 500, lam[:5], "mfma")
    e, em = rel_rows(W, ref).max(), rel_rows(Wm, ref).max()
    print("500 iterations at (300, 30): mfma_row %.2e | mfma %.2e" % (e, em))
    assert (nd == 500).all() and e < EPS


@pytest.mark.parametrize("N,K,P", [(129, 2, 5), (300, 30, 70), (300, 30, 5), (320, 33, 69)])
def test_kernel_alone_lambda_vector_with_y_rep_2(N, K, P):
    """Problem p reads series p // 2 and its own lambda (0.005 / 0.015 lambda_max of its series, alternating)."""
    h, step, Y, lam, _, W0, _, _ = case(N, K)
    V = (P + 1) // 2
    lam2 = (np.repeat(lam[:V], 2) * np.tile([0.5, 1.5], V))[:P]
    Yo = np.repeat(Y[:V].astype(np.float64), 2, axis=0)[:P]
    ref = c_oracle.fista_batch(Yo, h, lam2, step, NI, W0=W0[:P], threads=16)[0]
    W, nd, _ = solve(Y[:V], W0[:P], h, step, NI, lam2, "mfma_row", y_rep=2, P=P)
    e = rel_rows(W, ref).max()
    print("N=%d K=%d P=%d y_rep=2: mfma_row %.2e" % (N, K, P, e))
    assert (nd == NI).all() and e < EPS


# ---- 2: hand-back ----------------------------------------------------------------------------------------------------------
def handback_rows():
    """Five rows of (300, 30): row 1 starts 1000 max|y| high (|sigma w| leaves the float16 range), row 3 has 0.9 lambda_max."""
    h, step, Y, lam, _, W0, _, _ = case(300, 30)
    lam5, W5 = lam[:5].copy(), W0[:5].copy()
    W5[1] = 1000.0 * np.abs(Y[1]).max() * np.sign(W5[1])
    lam5[3] = 0.9 * lam[3] / DENSE
    ref = c_oracle.fista_batch(Y[:5].astype(np.float64), h, lam5, step, NI, W0=W5, threads=16)[0]
    return h, step, Y[:5], lam5, W5, ref


def test_hand_back_rows_are_not_stored():
    h, step, Y, lam5, W5, ref = handback_rows()
    W, nd, _ = solve(Y, W5, h, step, NI, lam5, "mfma_row")
    assert nd.tolist() == [NI, -1, NI, -1, NI], nd
    for p in (1, 3):
        assert (W[p].view(np.int64) == W5[p].view(np.int64)).all(), "row %d was stored" % p
    assert rel_rows(W[[0, 2, 4]], ref[[0, 2, 4]]).max() < EPS
    # the one-wave form hands the same two rows back
    _, ndm, _ = solve(Y, W5, h, step, NI, lam5, "mfmaonly")
    assert ndm.tolist() == [NI, -1, NI, -1, NI], ndm


def test_hand_back_rows_are_re_solved_by_the_default_call():
    """The same five rows as the LAST rows of a default (partitioned) call of 16 384 + 5 problems.  The list of the call holds
    its dense rows in order, so the whole round takes the 16 384 filler rows and the five are what it leaves: the four
    dense ones go to fista_mfma_row_kernel -- which hands the overflow row back to the call's re-solve --, the row at
    0.9 lambda_max is the call's only sparse row and goes to the vector kernel.  The call hands nothing back:
    n_done == n_iter everywhere and each of the five rows within EPS of the oracle."""
    h, step, Y5, lam5, W5, ref = handback_rows()
    _, _, Yc, lamc, _, W0c, _, _ = case(300, 30)
    reps = -(-ROUND // 70)
    Y = np.concatenate([np.tile(Yc, (reps, 1))[:ROUND], Y5])
    lam = np.concatenate([np.tile(lamc, reps)[:ROUND], lam5])
    W0 = np.concatenate([np.tile(W0c, (reps, 1))[:ROUND], W5])
    W, nd, _ = solve(Y, W0, h, step, NI, lam, None, work=True)
    assert (nd == NI).all(), nd[nd != NI]
    err = rel_rows(W[ROUND:], ref)
    print("default call of 16 384 + 5 problems, the five hand-back rows: %s" % " ".join("%.2e" % e for e in err))
    assert err.max() < EPS
    fill = c_oracle.fista_batch(Yc[:8].astype(np.float64), h, lamc[:8], step, NI, W0=W0c[:8], threads=16)[0]
    assert rel_rows(W[:8], fill).max() < EPS
    # the dense three that are in range are the new kernel's bits (rows 0, 2, 4 of the five)
    Wr, _, _ = solve(Y5, W5, h, step, NI, lam5, "mfma_row")
    assert (W[ROUND:][[0, 2, 4]].view(np.int64) == Wr[[0, 2, 4]].view(np.int64)).all()


ROUND, LEFT, N_DENSE_LEFT = 16384, 48, 24


# ---- 3: the wiring ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wiring():
    """16 384 + 48 problems at (300, 30): rows from 16 384 + 24 on are sparse (0.5 lambda_max), every other row dense, so the
    list array holds the dense rows in order, then the sparse ones, and the end of the dense class, 16 408, lies inside the
    range [16 384, 16 432) that the whole round leaves to the one-problem-per-wave candidate.  Warm start; the dense
    left-over 16 390 starts outside the float16 range (handed back by the matrix-pipe kernel, re-solved by the call)."""
    from pybold_amd import solver
    N, K, P = 300, 30, ROUND + LEFT
    h, step, _ = operator(N, K)
    Y, lmax = block_series(P, N, K, seed=77)
    lam = DENSE * lmax
    lam[ROUND + N_DENSE_LEFT:] = 0.5 * lmax[ROUND + N_DENSE_LEFT:]
    rng = np.random.RandomState(5)
    W0 = 0.01 * rng.randn(P, N) * Y.std()
    W0[ROUND + 6] = 1000.0 * np.abs(Y[ROUND + 6]).max() * np.sign(W0[ROUND + 6])
    sample = np.sort(rng.choice(ROUND, 64, replace=False))
    rows = np.r_[sample, np.arange(ROUND, P)]
    ref = c_oracle.fista_batch(Y[rows].astype(np.float64), h, lam[rows], step, NI, W0=W0[rows], threads=16)[0]
    out = {}
    for force in (None, "vector_leftovers"):
        out[force] = solve(Y, W0, h, step, NI, lam, force, work=True)[:2]
    return dict(h=h, step=step, Y=Y, lam=lam, W0=W0, rows=rows, ref=ref, out=out, solver=solver, P=P)


def test_wiring_leftovers_match_the_oracle(wiring):
    W, nd = wiring["out"][None]
    rows, ref = wiring["rows"], wiring["ref"]
    assert (nd == NI).all()
    err = rel_rows(W[rows], ref)
    print("default call: seeded sample of the whole round %.2e, dense left-overs %.2e, sparse left-overs %.2e, re-solved row %.2e"
          % (err[:64].max(), err[64:64 + N_DENSE_LEFT].max(), err[64 + N_DENSE_LEFT:].max(), err[64 + 6]))
    assert err.max() < EPS


def test_wiring_runs_the_new_kernel_on_the_dense_leftovers_only(wiring):
    """Rows are solved independently and every kernel is deterministic: the dense left-overs of the default call equal the
    rows of a solve on fista_mfma_row_kernel alone bit for bit (but the handed-back one, which the call re-solved), the
    sparse left-overs those of the one-problem-per-wave vector kernel alone."""
    g = wiring
    W, _ = g["out"][None]
    dense = np.arange(ROUND, ROUND + N_DENSE_LEFT)
    sparse = np.arange(ROUND + N_DENSE_LEFT, g["P"])
    Wr, ndr, _ = solve(g["Y"][dense], g["W0"][dense], g["h"], g["step"], NI, g["lam"][dense], "mfma_row")
    assert ndr.tolist() == [NI] * 6 + [-1] + [NI] * (N_DENSE_LEFT - 7)
    keep = np.delete(np.arange(N_DENSE_LEFT), 6)
    assert (W[dense][keep].view(np.int64) == Wr[keep].view(np.int64)).all()
    Wv, _, _ = solve(g["Y"][sparse], g["W0"][sparse], g["h"], g["step"], NI, g["lam"][sparse], "wide")
    assert (W[sparse].view(np.int64) == Wv.view(np.int64)).all()
    Wd, _, _ = solve(g["Y"][dense], g["W0"][dense], g["h"], g["step"], NI, g["lam"][dense], "wide")
    assert (W[dense][keep].view(np.int64) != Wd[keep].view(np.int64)).any(axis=1).all()      # (not the vector kernel's bits)


def test_wiring_off_switch_is_the_vector_kernel_bit_for_bit(wiring):
    g = wiring
    W, nd = g["out"]["vector_leftovers"]
    left = np.arange(ROUND, g["P"])
    assert (nd == NI).all()
    Wv, _, _ = solve(g["Y"][left], g["W0"][left], g["h"], g["step"], NI, g["lam"][left], "wide")
    assert (W[left].view(np.int64) == Wv.view(np.int64)).all()
    # the whole round does not see the switch (seeded sample)
    rows = g["rows"][:64]
    assert (W[rows].view(np.int64) == g["out"][None][0][rows].view(np.int64)).all()


def test_wiring_moves_no_plan(wiring):
    """The queries answer what they answered before the kernel existed (the plan of a call is not touched)."""
    s = wiring["solver"]
    assert s.launch_plan(300, 30, ROUND + LEFT) == (ROUND, s.KERNEL_NAMES[4], s.KERNEL_NAMES[3])
    assert s.which_kernel(300, 30, ROUND + LEFT) == s.KERNEL_NAMES[4]
    assert s.launch_plan(300, 30, 100000) == (98304, s.KERNEL_NAMES[4], s.KERNEL_NAMES[3])
    assert s.launch_plan(300, 30, 100000, force="vector_leftovers") == s.launch_plan(300, 30, 100000)
