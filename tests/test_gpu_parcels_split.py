"""GPU tests of the grouped z-step (`fista_solve_grouped`) on the split matrix-pipe forms -- PB_FLAG_GROUPED_SPLIT:
launch_mfma2_grouped<NBA, NBB> at 311 .. 640 scans, launch_mfma4_grouped<A> at 641 .. 1 280, two near tiles (K <= 33) and
three (34 .. 48 taps) -- at the first and the last length of every compiled instance, and of `bd_parcels` with the opt-in.

Inputs and float64 references come from tests/parcel_split_cases.py and tests/parcel_cases.py (conditions checked on the CPU
by tests/test_parcel_split_host.py): ten parcels, four of them empty with NaN taps and steps, HRFs whose gains span five
orders of magnitude and both signs, so every workgroup of a grouped launch has its own tap scale and step.

Every number asserted is the project's bound for the quantity (1e-5 relative L2 per row for the matrix-pipe solves: EPS of
tests/test_gpu_mfma.py), exact equality, or the routing rule restated in parcel_split_cases.

Reference: pybold/bold_signal.py:62-72 (the recurrence), :281-382 (bd)."""
import functools

import numpy as np
import pytest
import torch

from oracle import pybold_oracle as orc
from tests import parcel_cases as pc
from tests import parcel_split_cases as ps

pytestmark = pytest.mark.gpu

EPS = 1.0e-5                  # tests/test_gpu_mfma.py
T_R = 0.75


def rel_rows(a, b):
    return np.linalg.norm(a - b, axis=1) / (np.linalg.norm(b, axis=1) + 1e-300)


@pytest.fixture(scope="module")
def solver():
    from pybold_amd import solver as s
    return s


def on_device(case):
    """The tensors of a case: (Y, taps, steps, lbda, W0)."""
    lbda = case["lbda"] if np.ndim(case["lbda"]) == 0 else torch.from_numpy(np.array(case["lbda"])).cuda()
    W0 = None if case["W0"] is None else torch.from_numpy(np.array(case["W0"])).cuda()
    return (torch.from_numpy(np.array(case["Y"])).cuda(), torch.from_numpy(np.array(case["taps"])).cuda(),
            torch.from_numpy(np.array(case["steps"])).cuda(), lbda, W0)


def rows_of(lbda, r0, r1):
    return lbda if not torch.is_tensor(lbda) else lbda[r0:r1].contiguous()


# ---- 1: every instance against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,variant", ps.CASES)
def test_every_split_instance_against_the_oracle(solver, N, K, variant):
    """`force="gsplit_mfmaonly"` on the ten-parcel layout: all 84 rows run their 60 iterations on the matrix pipe -- none is
    handed back, none left out --, every row within 1e-5 of the oracle, the result finite (the NaN taps and steps of the empty
    parcels are never read), the warm start unmodified and not aliased."""
    case = ps.case(N, K, variant)
    assert solver.grouped_route(pc.OFFSETS, N, K, "gsplit_mfmaonly") == (5 if N <= 640 else 6, 9, pc.ROWS)
    Y, taps, steps, lbda, W0 = on_device(case)
    before = None if W0 is None else W0.clone()
    W, nd = solver.fista_solve_grouped(Y, taps, steps, pc.OFFSETS, lbda, case["n_iter"], W0=W0, force="gsplit_mfmaonly")
    err = rel_rows(W.cpu().numpy(), case["ref"])
    print("grouped split z-step N=%d K=%d %s: worst rel L2 vs the float64 oracle %.3e (row %d)" % (N, K, variant, err.max(), int(err.argmax())))
    nd = nd.cpu().numpy()
    assert (nd == case["n_iter"]).all(), np.where(nd != case["n_iter"])[0]
    assert bool(torch.isfinite(W).all())
    assert err.max() < EPS, (float(err.max()), int(err.argmax()))
    if W0 is not None:
        assert torch.equal(W0, before) and W.data_ptr() != W0.data_ptr()


# ---- 2: independence of parcels, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", ps.BIT_SHAPES)
def test_parcels_are_independent_bit_for_bit(solver, N, K):
    """Every non-empty parcel solved alone -- a grouped call with G = 1 on its rows, taps, step and lambda rows, the same
    instantiation -- gives the bits the ten-parcel call gives for those rows.  The comparison with the shared form
    (`fista_solve_pp`, one HRF in device memory, force="mfma2only") on parcels of two rows or more is printed, not asserted
    (tests/test_gpu_parcels_variants.py says why that form's route can differ); profiles/parcels_split.txt keeps it."""
    case = ps.case(N, K, "warm")
    Y, taps, steps, lbda, W0 = on_device(case)
    n_iter = case["n_iter"]
    W, nd = solver.fista_solve_grouped(Y, taps, steps, pc.OFFSETS, lbda, n_iter, W0=W0, force="gsplit_mfmaonly")
    shared_equal = {}
    for g in pc.NONEMPTY:
        r0, r1 = int(pc.OFFSETS[g]), int(pc.OFFSETS[g + 1])
        args = (Y[r0:r1].contiguous(), taps[g:g + 1].contiguous(), steps[g:g + 1].contiguous())
        Wa, nda = solver.fista_solve_grouped(*args, [0, r1 - r0], rows_of(lbda, r0, r1), n_iter, W0=W0[r0:r1].contiguous(),
                                             force="gsplit_mfmaonly")
        assert torch.equal(nd[r0:r1], nda), g
        assert torch.equal(W[r0:r1], Wa), (g, float((W[r0:r1] - Wa).abs().max()))
        if r1 - r0 >= 2:
            Ws, nds = solver.fista_solve_pp(args[0], taps[g].contiguous(), args[2], rows_of(lbda, r0, r1), n_iter,
                                            W0=W0[r0:r1].contiguous(), force="mfma2only")
            shared_equal[pc.SIZES[g]] = bool(torch.equal(W[r0:r1], Ws)) and bool(torch.equal(nd[r0:r1], nds))
    print("grouped split z-step N=%d K=%d warm: every parcel alone (G = 1) bit-equal; equal to the shared form's rows, by parcel size: %s"
          % (N, K, shared_equal))


# ---- 3: layout -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force", ["gsplit_mfmaonly", "gsplit"])
@pytest.mark.parametrize("N,K", ps.LAYOUT_SHAPES)
def test_padded_leading_dimensions_and_guard_bands(solver, N, K, force):
    """Y, the taps (ldt > K) and the in-place iterate as windows of larger allocations (tests/frames.py): the inputs are
    untouched, W is untouched outside its window and written everywhere inside, and the result has the bits of the packed
    call -- on the matrix pipe and through the library's dispatch (84 rows: the vector route)."""
    from tests import frames
    case = ps.case(N, K, "warm")
    assert solver.grouped_route(pc.OFFSETS, N, K, force)[0] == (0 if force == "gsplit" else 5 if N <= 640 else 6)
    Y, taps, steps, lbda, W0 = on_device(case)
    packed, ndp = solver.fista_solve_grouped(Y, taps, steps, pc.OFFSETS, lbda, case["n_iter"], W0=W0, force=force)
    fy = frames.frame2d("y", pc.ROWS, N, torch.float32, "cuda", fill=Y)
    ft = frames.frame2d("taps_pp", len(pc.SIZES), K, torch.float64, "cuda", fill=taps)
    fw = frames.frame2d("W", pc.ROWS, N, torch.float64, "cuda", fill=W0)
    assert ft.ld > K and fy.ld > N and fw.ld > N
    for f in (fy, ft, fw):
        f.snapshot()
    W, nd = solver.fista_solve_grouped(fy.view, ft.view, steps, pc.OFFSETS, lbda, case["n_iter"], W0=fw.view, inplace=True, force=force)
    torch.cuda.synchronize()
    assert W.data_ptr() == fw.view.data_ptr()
    fy.assert_untouched()
    ft.assert_untouched()
    fw.assert_outside_untouched()
    assert not bool(fw.is_sentinel().any())
    assert torch.equal(fw.view, packed) and torch.equal(nd, ndp)
    assert int(nd.min()) == case["n_iter"]


# ---- 4: hand-back and re-solve with the parcel's taps ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", ps.HANDBACK_SHAPES)
def test_handed_back_rows_are_resolved_with_their_parcels_taps(solver, N, K):
    """Odd rows far outside the accuracy guard, even rows far inside (by the oracle: test_parcel_split_host.py).  Without the
    re-solve every odd row comes back with n_done = -1 and keeps the zeros of its cold start, every even row is solved; with
    it every row is solved within 1e-5 -- the re-solve reads each row's parcel's taps.  (The start is given as zeros instead of
    the cold-start flag, so that a row left alone is a row of zeros.)"""
    case = ps.handback_case(N, K)
    Y, taps, steps, lbda, _ = on_device(case)
    odd = torch.arange(pc.ROWS, device="cuda") % 2 == 1
    W0 = torch.zeros((pc.ROWS, N), dtype=torch.float64, device="cuda")
    Wn, ndn = solver.fista_solve_grouped(Y, taps, steps, pc.OFFSETS, lbda, case["n_iter"], W0=W0, force="gsplit_mfmaonly")
    assert bool((ndn[odd] == -1).all()) and bool((ndn[~odd] == case["n_iter"]).all()), ndn.cpu().numpy()
    assert bool((Wn[odd] == 0).all())
    W, nd = solver.fista_solve_grouped(Y, taps, steps, pc.OFFSETS, lbda, case["n_iter"], W0=W0, force="gsplit_mfma")
    assert bool((nd == case["n_iter"]).all())
    err = rel_rows(W.cpu().numpy(), case["ref"])
    print("grouped split z-step N=%d K=%d hand-back: worst rel L2 after the re-solve %.3e (row %d)" % (N, K, err.max(), int(err.argmax())))
    assert bool(torch.isfinite(W).all()) and err.max() < EPS, (float(err.max()), int(err.argmax()))
    assert torch.equal(W[~odd], Wn[~odd])


# ---- 5: whole passes and the rows behind them -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_batch(N, sizes):
    """The data of tests/test_gpu_parcels_variants.py::big_batch at another length: 27 taps, dilations 0.8, 1.2, 1.5,
    lambda = 0.05 x the smallest lambda_max of the first 64 rows."""
    from pybold_amd import data, solver
    off = np.concatenate([[0], np.cumsum(sizes)])
    taps = torch.from_numpy(np.stack([orc.spm_hrf(th, T_R, 20.0, False)[0] for th in (0.8, 1.2, 1.5)])).cuda()
    assert taps.shape[1] == 27
    Y, _, _ = data.gen_rnd_bloc_bold_batch(int(sum(sizes)), dur=N * T_R / 60.0, tr=T_R, hrf=taps[1].cpu().numpy(), nb_events=5,
                                           avg_dur=12.0, std_dur=1.0, snr=10.0, seed=2)
    assert Y.shape == (int(sum(sizes)), N)
    steps = 1.0 / solver.gram_frobenius_batch(taps, N)
    lbda = 0.05 * float(solver.lambda_max(Y[:64].contiguous(), taps[1].cpu().numpy()).min())
    return Y, taps, steps, off, lbda


def rows_against_oracle(Y, taps, steps, off, lbda, W, ranges, n_iter):
    for r0, r1 in ranges:
        for g in range(len(off) - 1):
            a, b = max(r0, int(off[g])), min(r1, int(off[g + 1]))
            if a < b:
                ref = orc.fista_batch(Y[a:b].cpu().numpy().astype(np.float64), taps[g].cpu().numpy(), lbda, float(steps[g]), n_iter)
                assert rel_rows(W[a:b].cpu().numpy(), ref).max() < EPS, (a, b, g)


@pytest.mark.parametrize("N,sizes,split_256", [
    (330, (5000, 3500, 300), (5, 512, 8184)),          # 551 units: one pass of 512, 39 behind it; the cut inside the second parcel
    (700, (2500, 1700, 200), (6, 256, 4084)),          # 277 units: one pass of 256, 21 behind it
    (330, (5000, 3500, 2300), (5, 676, 10800)),        # 676 units: the remainder of 164 stays on the matrix pipe
    (700, (2500, 1700, 2500), (6, 421, 6700))])        # 421 units: the remainder of 165 stays
def test_whole_passes_and_the_rows_behind_them(solver, N, sizes, split_256):
    """Library dispatch with the flag alone, 20 iterations: the expectation is `solver.grouped_route`'s, which must equal the
    rule restated with this device's compute units (and, on 256 of them, the figures above).  Every row runs its 20
    iterations -- on the matrix pipe, behind the cut on the vector forms, or re-solved --; rows on both sides of the cut, of
    the parcel boundaries, the first and the last rows against the oracle."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    Y, taps, steps, off, lbda = big_batch(N, sizes)
    po = solver.ParcelOffsets(off, Y.device)
    got = solver.grouped_route(po, N, 27, "gsplit")
    assert got == ps.expected_route(sizes, N, 27, ps.GROUPED_SPLIT, wave_slots=8 * cus), (got, cus)
    if cus == 256:
        assert got == split_256
    code, main_units, cut = got
    print("grouped split z-step N=%d parcels %s on %d compute units: code %d, %d of %d units in the main launch, rows from %d behind it"
          % (N, sizes, cus, code, main_units, po.waves(), cut))
    W, nd = solver.fista_solve_grouped(Y, taps, steps, po, lbda, 20, force="gsplit")
    assert int(nd.min()) == 20 and int(nd.max()) == 20
    V = po.rows
    edges = [0, int(off[1]), int(off[2]), V] + ([cut] if 0 < cut < V else [])
    ranges = sorted(set((max(e - 17, 0), min(e + 17, V)) for e in edges))
    rows_against_oracle(Y, taps, steps, off, lbda, W, ranges, 20)
    if 0 < cut < V:
        # the rows behind the cut are the vector route's: the bits of a force="valu" call on those rows alone
        g0 = int(np.searchsorted(off, cut, side="right")) - 1
        off_b = np.concatenate([[0], np.asarray(off[g0 + 1:]) - cut])
        Wb, ndb = solver.fista_solve_grouped(Y[cut:].contiguous(), taps[g0:].contiguous(), steps[g0:].contiguous(), off_b, lbda, 20,
                                             force="valu")
        assert int(ndb.min()) == 20 and torch.equal(W[cut:], Wb)


# ---- 6: the whole loop ------------------------------------------------------------------------------------------------------------
class _OneProcess:                                   # the oracle loop never talks to other ranks
    world_size, rank = 1, 0

    @staticmethod
    def allreduce_(t):
        return t


BD_SIZES, BD_THETA, BD_LABELS = [1, 15, 16, 17, 33], [0.7, 1.0, 1.3, 0.9, 1.6], [40, 7, 19, -3, 25]      # tests/test_gpu_parcels.py
DUR, NB_ITER, NB_INNER = 20.0, 3, 40


@pytest.mark.parametrize("N", [330, 700])
def test_bd_parcels_whole_loop_with_the_opt_in(solver, monkeypatch, N):
    """`bd_parcels` with every z-step forced onto the split forms against the float64 oracle loop of every parcel alone, with
    the assertions and the theta bound of test_gpu_parcels.py::test_bd_parcels_whole_loop_against_the_per_parcel_oracle_loops.
    With PYBOLD_AMD_PARCELS_SPLIT=1, force="mfma" is the same call bit for bit; without the variable it raises."""
    import pybold_amd
    from oracle.shared_ops import OracleOps
    from pybold_amd import _lib, data, distributed
    monkeypatch.delenv("PYBOLD_AMD_PARCELS_SPLIT", raising=False)
    rows = []
    for p, (n, th) in enumerate(zip(BD_SIZES, BD_THETA)):
        h = orc.spm_hrf(th, T_R, DUR, False)[0]
        Yp, _, _ = data.gen_rnd_bloc_bold_batch(n, dur=N * T_R / 60.0, tr=T_R, hrf=h, nb_events=5, avg_dur=12.0, std_dur=1.0, snr=10.0,
                                                seed=11 + p)
        assert Yp.shape == (n, N)
        rows.append(Yp)
    Y = torch.cat(rows).contiguous()
    lbda = 0.05 * float(solver.lambda_max(Y, orc.spm_hrf(2.0, T_R, DUR, False)[0]).min())
    offsets = np.concatenate([[0], np.cumsum(BD_SIZES)])
    V = int(offsets[-1])
    perm = np.random.RandomState(5).permutation(V)
    labels = np.repeat(BD_LABELS, BD_SIZES)[perm]
    Ysh = Y[torch.from_numpy(perm).cuda()].contiguous()
    kw = dict(lbda=lbda, theta_0=2.0, hrf_dur=DUR, nb_iter=NB_ITER, nb_inner=NB_INNER)
    loops, worst_shared = [], 0.0
    for p in range(len(BD_SIZES)):
        Yp = Y[offsets[p]:offsets[p + 1]]
        Wo, ho, do = distributed.bd_shared(Yp.cpu(), T_R, ops=OracleOps(N, T_R, DUR), comm=_OneProcess(), **kw)
        Ws, hs, ds = distributed.bd_shared(Yp, T_R, **kw)
        loops.append(dict(W=Wo.numpy(), h=np.asarray(ho), theta=np.asarray(do["theta"], dtype=np.float64), J=np.asarray(do["J"])))
        worst_shared = max(worst_shared, float(np.abs(np.asarray(ds["theta"], dtype=np.float64) - loops[-1]["theta"]).max()))
    X, Z, W, H, d = pybold_amd.bd_parcels(Ysh, labels, T_R, force="gsplit_mfma", **kw)
    G = len(BD_SIZES)
    assert X.shape == Z.shape == W.shape == (V, N) and H.shape == (G, 27)
    assert d["theta"].shape == (NB_ITER + 1, G) and d["J"].shape == (NB_ITER + 2, G) and list(d["labels"]) == sorted(BD_LABELS)
    worst = 0.0
    Xn, Zn, Wn = (t.cpu().numpy() for t in (X, Z, W))
    for g, lab in enumerate(d["labels"]):
        o = loops[BD_LABELS.index(int(lab))]
        mine = np.where(labels == lab)[0]                               # this parcel's rows in the caller's order ...
        gen = perm[mine] - offsets[BD_LABELS.index(int(lab))]           # ... and in the oracle loop's order
        Wo = o["W"][gen]
        Zo = np.cumsum(Wo, axis=1)
        Xo = orc.causal_conv(o["h"], Zo)
        for got, want in ((Wn[mine], Wo), (Zn[mine], Zo), (Xn[mine], Xo)):
            assert rel_rows(got, want).max() < 1e-5, (lab, rel_rows(got, want).max())
        np.testing.assert_allclose(d["J"][:, g], o["J"], rtol=1e-6)
        worst = max(worst, float(np.abs(d["theta"][:, g] - o["theta"]).max()))
    print("bd_parcels (force=gsplit_mfma) N=%d, parcels of %s voxels, 3 x 40 iterations: worst |dtheta| vs the per-parcel oracle loops "
          "%.3e; bd_shared on each parcel alone: %.3e" % (N, BD_SIZES, worst, worst_shared))
    assert worst <= max(2.0 * worst_shared, 1e-6), (worst, worst_shared)
    with pytest.raises(_lib.PyboldHipError):
        pybold_amd.bd_parcels(Ysh, labels, T_R, force="mfma", **kw)
    monkeypatch.setenv("PYBOLD_AMD_PARCELS_SPLIT", "1")
    X2, Z2, W2, H2, d2 = pybold_amd.bd_parcels(Ysh, labels, T_R, force="mfma", **kw)
    assert torch.equal(W2, W) and torch.equal(X2, X) and torch.equal(Z2, Z) and torch.equal(H2, H)
    assert np.array_equal(d2["theta"], d["theta"]) and np.array_equal(d2["J"], d["J"])
