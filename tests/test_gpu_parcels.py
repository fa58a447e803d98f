"""GPU tests of the parcel model (one HRF dilation per parcel of an atlas): the grouped normal equations, the grouped
z-step on the matrix pipe and the whole loop of `pybold_amd.bd_parcels`, against code and oracles the project already has
-- mathematically a parcel model is G independent `bd_shared` problems.

Common data: TR 0.75 s, 20 s HRF (K = 27), N = 150 (five blocks of 31 samples: the smallest matrix-pipe variant),
parcels of 1, 15, 16, 17 and 33 voxels (82 rows: a lone problem, one short of a wave, exact, one over, two waves plus
one), generated with dilations 0.7, 1.0, 1.3, 0.9, 1.6, block signals at 10 dB, lambda = 0.05 x the smallest lambda_max
of the batch at theta = 2, theta_0 = 2.  The float64 oracle loops (one per parcel, three outer iterations of 40) are
computed once per module.

Reference: pybold/bold_signal.py:281-382 (bd), :217-222 (hrf_fit_err), :62-72 (the recurrence).
"""
import numpy as np
import pytest
import torch

from oracle import pybold_oracle as orc

pytestmark = pytest.mark.gpu

T_R, DUR, N = 0.75, 20.0, 150
SIZES = [1, 15, 16, 17, 33]
TRUE_THETA = [0.7, 1.0, 1.3, 0.9, 1.6]
LABELS = [40, 7, 19, -3, 25]                        # any values: parcel p of the lists above carries LABELS[p]
NB_ITER, NB_INNER = 3, 40
SEED = 11


class _OneProcess:                                   # the oracle loop never talks to other ranks
    world_size, rank = 1, 0

    @staticmethod
    def allreduce_(t):
        return t


def rel_rows(a, b):
    return np.linalg.norm(a - b, axis=1) / (np.linalg.norm(b, axis=1) + 1e-300)


@pytest.fixture(scope="module")
def solver():
    from pybold_amd import solver as s
    return s


@pytest.fixture(scope="module")
def batch(solver):
    """Rows parcel by parcel (`Y`, `offsets`), and the same rows shuffled with their labels (`Ysh`, `labels`, `perm`)."""
    from pybold_amd import data
    rows = []
    for p, (n, th) in enumerate(zip(SIZES, TRUE_THETA)):
        h = orc.spm_hrf(th, T_R, DUR, False)[0]
        Yp, _, _ = data.gen_rnd_bloc_bold_batch(n, dur=N * T_R / 60.0, tr=T_R, hrf=h, nb_events=5, avg_dur=12.0, std_dur=1.0,
                                                snr=10.0, seed=SEED + p)
        assert Yp.shape == (n, N)
        rows.append(Yp)
    Y = torch.cat(rows).contiguous()
    h2 = orc.spm_hrf(2.0, T_R, DUR, False)[0]
    assert len(h2) == 27
    lbda = 0.05 * float(solver.lambda_max(Y, h2).min())
    offsets = np.concatenate([[0], np.cumsum(SIZES)])
    perm = np.random.RandomState(5).permutation(sum(SIZES))
    labels_sorted = np.repeat(LABELS, SIZES)
    return dict(Y=Y, offsets=offsets, lbda=lbda, perm=perm, Ysh=Y[torch.from_numpy(perm).cuda()].contiguous(),
                labels=labels_sorted[perm])


@pytest.fixture(scope="module")
def oracle_loops(batch):
    """Every parcel solved alone by the float64 oracle loop, and by the shared-HRF loop of the library (`bd_shared`, the
    form these tests measure the parcel loop against): per parcel (W, h, theta trajectory, J)."""
    from oracle.shared_ops import OracleOps
    from pybold_amd import distributed
    out = []
    for p in range(len(SIZES)):
        Yp = batch["Y"][batch["offsets"][p]:batch["offsets"][p + 1]]
        Wo, ho, do = distributed.bd_shared(Yp.cpu(), T_R, lbda=batch["lbda"], theta_0=2.0, hrf_dur=DUR, nb_iter=NB_ITER,
                                           nb_inner=NB_INNER, ops=OracleOps(N, T_R, DUR), comm=_OneProcess())
        Ws, hs, ds = distributed.bd_shared(Yp, T_R, lbda=batch["lbda"], theta_0=2.0, hrf_dur=DUR, nb_iter=NB_ITER, nb_inner=NB_INNER)
        out.append(dict(W=Wo.numpy(), h=np.asarray(ho), theta=np.asarray(do["theta"], dtype=np.float64), J=np.asarray(do["J"]),
                        theta_shared=np.asarray(ds["theta"], dtype=np.float64)))
    worst_shared = max(float(np.abs(o["theta_shared"] - o["theta"]).max()) for o in out)
    return out, worst_shared


# ---- test 2: grouped normal equations ---------------------------------------------------------------------------------
@pytest.mark.parametrize("framed", [False, True])
def test_grouped_normal_equations_equal_the_per_parcel_ones(solver, batch, framed):
    """Row g of `hrf_normal_eq_w_grouped` against `hrf_normal_eq_w` on parcel g's rows alone (the project's tolerance for
    this quantity: rtol 1e-11 with an atol scaled to the set, ||w||_1 at 1e-12); once more with padded leading dimensions
    and guard bands around the output, which must stay untouched."""
    from tests import frames
    K, off = 27, batch["offsets"]
    rng = np.random.RandomState(3)
    V = int(off[-1])
    Wn = (rng.rand(V, N) < 0.1) * rng.randn(V, N)
    W = torch.from_numpy(Wn).cuda()
    Y = batch["Y"]
    ne = K * K + K + 2
    if framed:
        fw = frames.frame2d("W", V, N, torch.float64, "cuda", fill=W)
        fy = frames.frame2d("y", V, N, torch.float32, "cuda", fill=Y)
        fo = frames.frame2d("out", len(SIZES), ne, torch.float64, "cuda")
        for f in (fw, fy, fo):
            f.snapshot()
        got = solver.hrf_normal_eq_w_grouped(fw.view, fy.view, K, off, out=fo.view)
        torch.cuda.synchronize()
        fw.assert_untouched()
        fy.assert_untouched()
        fo.assert_outside_untouched()
        assert not bool(fo.is_sentinel().any())
        got = got.cpu().numpy()
    else:
        got = solver.hrf_normal_eq_w_grouped(W, Y, K, off).cpu().numpy()
    assert got.shape == (len(SIZES), ne)
    for g in range(len(SIZES)):
        ref = solver.hrf_normal_eq_w(W[off[g]:off[g + 1]].contiguous(), Y[off[g]:off[g + 1]].contiguous(), K).cpu().numpy()
        np.testing.assert_allclose(got[g, :-1], ref[:-1], rtol=1e-11, atol=1e-11 * max(np.abs(ref[:-1]).max(), 1e-300))
        np.testing.assert_allclose(got[g, -1], ref[-1], rtol=1e-12)
        np.testing.assert_allclose(got[g, -1], np.abs(Wn[off[g]:off[g + 1]]).sum(), rtol=1e-12)


def test_grouped_normal_equations_of_a_large_and_an_empty_parcel(solver):
    """A parcel of thousands of rows is cut into several units (fixed-order second stage), an empty one gives zeros, and
    two calls give the same bits."""
    K, n = 27, 150
    rng = np.random.RandomState(8)
    sizes = [3000, 0, 1, 70]
    off = np.concatenate([[0], np.cumsum(sizes)])
    V = int(off[-1])
    W = torch.from_numpy((rng.rand(V, n) < 0.1) * rng.randn(V, n)).cuda()
    Y = torch.from_numpy(rng.randn(V, n).astype(np.float32)).cuda()
    got = solver.hrf_normal_eq_w_grouped(W, Y, K, off)
    again = solver.hrf_normal_eq_w_grouped(W, Y, K, off)
    assert torch.equal(got, again)
    got = got.cpu().numpy()
    assert (got[1] == 0).all()
    for g in (0, 2, 3):
        ref = solver.hrf_normal_eq_w(W[off[g]:off[g + 1]].contiguous(), Y[off[g]:off[g + 1]].contiguous(), K).cpu().numpy()
        np.testing.assert_allclose(got[g, :-1], ref[:-1], rtol=1e-11, atol=1e-11 * np.abs(ref[:-1]).max())
        np.testing.assert_allclose(got[g, -1], ref[-1], rtol=1e-12)


# ---- test 3: grouped z-step ------------------------------------------------------------------------------------------
def test_grouped_z_step_on_the_matrix_pipe(solver, batch):
    """`fista_solve_grouped(force="mfmaonly")` with five different HRFs against the shared form on every parcel alone
    (`fista_solve_pp` with one HRF in device memory, force="mfmaonly"): the same `n_done` -- none handed back, a condition
    of this test's data --, every row within 1e-5 of the float64 oracle; whether the rows equal the shared form's bit for
    bit is printed.  The default dispatch and force="valu" are within 1e-5 too; 128 scans cannot be forced onto the
    matrix pipe."""
    from pybold_amd import _lib
    Y, off, lbda = batch["Y"], batch["offsets"], batch["lbda"]
    taps = torch.from_numpy(np.stack([orc.spm_hrf(th, T_R, DUR, False)[0] for th in TRUE_THETA])).cuda()
    steps = 1.0 / solver.gram_frobenius_batch(taps, N)
    Wg, nd = solver.fista_solve_grouped(Y, taps, steps, off, lbda, NB_INNER, force="mfmaonly")
    Wd, ndd = solver.fista_solve_grouped(Y, taps, steps, off, lbda, NB_INNER)
    Wv, ndv = solver.fista_solve_grouped(Y, taps, steps, off, lbda, NB_INNER, force="valu")
    nd = nd.cpu().numpy()
    bit_equal = []
    worst = {"mfmaonly": 0.0, "default": 0.0, "valu": 0.0}
    for g in range(len(SIZES)):
        r0, r1 = int(off[g]), int(off[g + 1])
        Ws, nds = solver.fista_solve_pp(Y[r0:r1].contiguous(), taps[g].contiguous(), steps[g:g + 1].contiguous(), lbda, NB_INNER,
                                        force="mfmaonly")
        nds = nds.cpu().numpy()
        assert (nds == NB_INNER).all(), (g, nds)                        # the shared form hands back none (choice of SEED)
        assert np.array_equal(nd[r0:r1], nds), (g, nd[r0:r1], nds)
        bit_equal.append(bool(torch.equal(Wg[r0:r1], Ws)))
        ref = orc.fista_batch(Y[r0:r1].cpu().numpy().astype(np.float64), taps[g].cpu().numpy(), lbda, float(steps[g]), NB_INNER)
        for tag, Wt in (("mfmaonly", Wg), ("default", Wd), ("valu", Wv)):
            worst[tag] = max(worst[tag], float(rel_rows(Wt[r0:r1].cpu().numpy(), ref).max()))
    print("grouped z-step, 82 rows in 5 parcels, 40 iterations: rel L2 vs float64 oracle %s; rows equal the shared form's bit for bit, parcel by parcel (%s rows): %s"
          % ({k: "%.2e" % v for k, v in worst.items()}, SIZES, bit_equal))
    assert (nd == NB_INNER).all()
    assert int(ndd.min()) == NB_INNER and int(ndv.min()) == NB_INNER
    for tag, err in worst.items():
        assert err < 1e-5, (tag, err)
    with pytest.raises(_lib.PyboldHipError):
        solver.fista_solve_grouped(Y[:, :128].contiguous(), taps, steps, off, lbda, NB_INNER, force="mfma")


def test_grouped_z_step_hands_back_and_resolves_with_the_parcels_taps(solver, batch):
    """Rows the accuracy guard hands back: at half the smallest lambda_max the solutions are sparse, the guard fires
    (n_done = -1 under "mfmaonly", the rows keep their start values), and force="mfma" re-solves those rows in the same
    call on the vector forms with their parcel's taps; a start from given values (zeros) instead of the cold-start flag."""
    Y, off = batch["Y"], batch["offsets"]
    taps = torch.from_numpy(np.stack([orc.spm_hrf(th, T_R, DUR, False)[0] for th in TRUE_THETA])).cuda()
    steps = 1.0 / solver.gram_frobenius_batch(taps, N)
    lmax = torch.cat([solver.lambda_max(Y[off[g]:off[g + 1]].contiguous(), taps[g].cpu().numpy()) for g in range(len(SIZES))])
    lbda = 0.5 * float(lmax.min())
    W0 = torch.zeros((sum(SIZES), N), dtype=torch.float64, device="cuda")
    Wo, ndo = solver.fista_solve_grouped(Y, taps, steps, off, lbda, NB_INNER, W0=W0, force="mfmaonly")
    Wr, ndr = solver.fista_solve_grouped(Y, taps, steps, off, lbda, NB_INNER, W0=W0, force="mfma")
    back = (ndo < 0)
    print("grouped z-step at 0.5 lambda_max: %d of %d rows handed back by the accuracy guard" % (int(back.sum()), len(back)))
    assert bool(back.any())                                             # (sparse solutions: the guard's case)
    assert bool((Wo[back] == 0).all())
    assert int(ndr.min()) == NB_INNER
    for g in range(len(SIZES)):
        r0, r1 = int(off[g]), int(off[g + 1])
        ref = orc.fista_batch(Y[r0:r1].cpu().numpy().astype(np.float64), taps[g].cpu().numpy(), lbda, float(steps[g]), NB_INNER)
        assert rel_rows(Wr[r0:r1].cpu().numpy(), ref).max() < 1e-5, g


def test_grouped_z_step_whole_rounds_and_the_rows_behind_them(solver):
    """17 000 rows in three parcels are 1 064 waves: one whole round (1 024 waves, one per SIMD) runs on the matrix pipe and
    the rows behind it -- the cut falls INSIDE the second parcel -- on the per-problem vector forms with their parcel's
    taps.  Rows on either side of the cut, the first and the last ones against the float64 oracle."""
    from pybold_amd import data
    sizes = [9000, 7384, 616]
    off = np.concatenate([[0], np.cumsum(sizes)])
    thetas = [0.8, 1.2, 1.5]
    taps = torch.from_numpy(np.stack([orc.spm_hrf(th, T_R, DUR, False)[0] for th in thetas])).cuda()
    Y, _, _ = data.gen_rnd_bloc_bold_batch(sum(sizes), dur=N * T_R / 60.0, tr=T_R, hrf=taps[1].cpu().numpy(), nb_events=5, avg_dur=12.0,
                                           std_dur=1.0, snr=10.0, seed=2)
    steps = 1.0 / solver.gram_frobenius_batch(taps, N)
    po = solver.ParcelOffsets(off, Y.device)
    assert po.waves() == 563 + 462 + 39
    lbda = 0.05 * float(solver.lambda_max(Y[:64].contiguous(), taps[1].cpu().numpy()).min())
    W, nd = solver.fista_solve_grouped(Y, taps, steps, po, lbda, 20)
    assert int(nd.min()) == 20 and int(nd.max()) == 20
    cut = 9000 + (1024 - 563) * 16
    for r0, r1 in ((0, 16), (8992, 9008), (cut - 16, cut + 8), (16384 - 8, 16384 + 8), (17000 - 16, 17000)):
        for g in range(3):
            a, b = max(r0, int(off[g])), min(r1, int(off[g + 1]))
            if a < b:
                ref = orc.fista_batch(Y[a:b].cpu().numpy().astype(np.float64), taps[g].cpu().numpy(), lbda, float(steps[g]), 20)
                assert rel_rows(W[a:b].cpu().numpy(), ref).max() < 1e-5, (a, b, g)


# ---- test 4: the whole loop ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force", [None, "mfma"])
def test_bd_parcels_whole_loop_against_the_per_parcel_oracle_loops(solver, batch, oracle_loops, force):
    """`bd_parcels` on the shuffled rows -- default dispatch, and every z-step forced onto the matrix pipe -- against the
    oracle loop of every parcel alone: diff_z, z, x of every row within 1e-5 in the caller's order, J per parcel at 1e-6,
    H[g] = h(theta_g) at 1e-10, and theta after every outer iteration within twice the worst |dtheta| the shared-HRF loop
    (`bd_shared` on each parcel's rows alone) shows against the same oracle, or 1e-6, whichever is larger."""
    import pybold_amd
    loops, worst_shared = oracle_loops
    X, Z, W, H, d = pybold_amd.bd_parcels(batch["Ysh"], batch["labels"], T_R, lbda=batch["lbda"], theta_0=2.0, hrf_dur=DUR,
                                          nb_iter=NB_ITER, nb_inner=NB_INNER, force=force)
    G, V = len(SIZES), sum(SIZES)
    assert X.shape == Z.shape == W.shape == (V, N) and X.dtype == Z.dtype == W.dtype == torch.float64
    assert H.shape == (G, 27) and d["theta"].shape == (NB_ITER + 1, G) and d["J"].shape == (NB_ITER + 2, G)
    assert list(d["labels"]) == sorted(LABELS)
    assert list(d["sizes"]) == [SIZES[LABELS.index(lab)] for lab in sorted(LABELS)]
    worst = 0.0
    X, Z, W, H = (t.cpu().numpy() for t in (X, Z, W, H))
    for g, lab in enumerate(d["labels"]):
        o = loops[LABELS.index(int(lab))]
        mine = np.where(batch["labels"] == lab)[0]                      # this parcel's rows in the caller's order ...
        gen = batch["perm"][mine] - batch["offsets"][LABELS.index(int(lab))]      # ... and in the oracle loop's order
        Wo = o["W"][gen]
        Zo = np.cumsum(Wo, axis=1)
        Xo = orc.causal_conv(o["h"], Zo)
        for got, want in ((W[mine], Wo), (Z[mine], Zo), (X[mine], Xo)):
            assert rel_rows(got, want).max() < 1e-5, (lab, rel_rows(got, want).max())
        np.testing.assert_allclose(d["J"][:, g], o["J"], rtol=1e-6)
        np.testing.assert_allclose(H[g], orc.spm_hrf(float(d["theta"][-1, g]), T_R, DUR, False)[0], rtol=1e-10, atol=1e-14)
        worst = max(worst, float(np.abs(d["theta"][:, g] - o["theta"]).max()))
    print("bd_parcels (force=%s), 5 parcels of %s voxels, 3 x 40 iterations: worst |dtheta| vs the per-parcel oracle loops %.3e; "
          "bd_shared on each parcel alone: %.3e" % (force, SIZES, worst, worst_shared))
    assert worst <= max(2.0 * worst_shared, 1e-6), (worst, worst_shared)


def test_bd_parcels_refuses_bad_arguments(batch):
    import pybold_amd
    Y, labels = batch["Ysh"], batch["labels"]
    with pytest.raises(ValueError):
        pybold_amd.bd_parcels(Y[:0], labels[:0], T_R)
    with pytest.raises(ValueError):
        pybold_amd.bd_parcels(Y, labels[:-1], T_R)
    with pytest.raises(ValueError):
        pybold_amd.bd_parcels(Y, labels, T_R, lbda=np.ones(len(labels)))
    with pytest.raises(ValueError):
        pybold_amd.bd_parcels(Y, labels, T_R, theta_0=pybold_amd.MAX_DELTA + 0.5)
    with pytest.raises(ValueError):
        pybold_amd.bd_parcels(Y, labels, T_R, theta_0=[1.0, 1.0, 1.0, 1.0, pybold_amd.MIN_DELTA - 0.1])
    with pytest.raises(ValueError):
        pybold_amd.bd_parcels(Y, labels, T_R, theta_0=[1.0, 1.0])


# ---- test 5: equivalences ----------------------------------------------------------------------------------------------
def test_one_parcel_is_bd_shared_and_labels_are_only_names(solver, batch, oracle_loops):
    """All labels equal: the shared-HRF loop on the batch (theta within the bound of the whole-loop test, W within 1e-5).
    Relabelling (labels x 7 + 3) changes nothing but d['labels']."""
    import pybold_amd
    from pybold_amd import distributed
    _, worst_shared = oracle_loops
    Y = batch["Ysh"]
    kw = dict(lbda=batch["lbda"], theta_0=2.0, hrf_dur=DUR, nb_iter=NB_ITER, nb_inner=NB_INNER)
    X1, Z1, W1, H1, d1 = pybold_amd.bd_parcels(Y, np.full(len(batch["labels"]), 9), T_R, **kw)
    Ws, hs, ds = distributed.bd_shared(Y, T_R, **kw)
    assert d1["theta"].shape == (NB_ITER + 1, 1) and list(d1["sizes"]) == [sum(SIZES)]
    assert np.abs(d1["theta"][:, 0] - np.asarray(ds["theta"])).max() <= max(2.0 * worst_shared, 1e-6)
    assert rel_rows(W1.cpu().numpy(), Ws.cpu().numpy()).max() < 1e-5
    np.testing.assert_allclose(d1["J"][:, 0], ds["J"], rtol=1e-6)
    Xa, Za, Wa, Ha, da = pybold_amd.bd_parcels(Y, batch["labels"], T_R, **kw)
    Xb, Zb, Wb, Hb, db = pybold_amd.bd_parcels(Y, batch["labels"] * 7 + 3, T_R, **kw)
    assert list(db["labels"]) == [lab * 7 + 3 for lab in da["labels"]]
    for a, b in ((Xa, Xb), (Za, Zb), (Wa, Wb), (Ha, Hb)):
        assert torch.equal(a, b)
    assert np.array_equal(da["theta"], db["theta"]) and np.array_equal(da["J"], db["J"]) and np.array_equal(da["sizes"], db["sizes"])
