"""GPU tests of the parcel model at every compiled variant: the grouped z-step (`fista_solve_grouped`) on each of the
six matrix-pipe instances at both edges of its range of scans with 1, 32 and 33 taps -- the 2:4-sparse kernel and the
dense two-tile kernel --, on the vector route and at shapes with no matrix-pipe form; `bd_parcels` off the matrix pipe;
and the grouped normal equations on each of their three kernels and on every width of their second stage.

Inputs and float64 references come from tests/parcel_cases.py (conditions checked on the CPU by
tests/test_parcel_cases_host.py): ten parcels, four of them empty with NaN taps and steps, HRFs whose gains span five
orders of magnitude and both signs, so every wave of a grouped launch has its own tap scale and step.

Every number asserted is the project's bound for the quantity (1e-5 relative L2 per row for the float32 / matrix-pipe
solves: EPS of tests/test_gpu_mfma.py; rtol 1e-11 with an atol scaled to the set and 1e-12 on ||w||_1 for the normal
equations: tests/test_gpu_round3.py), exact equality, or a condition on the oracle's output.

Reference: pybold/bold_signal.py:62-72 (the recurrence), :217-222 (hrf_fit_err), :281-382 (bd)."""
import functools

import numpy as np
import pytest
import torch

from oracle import pybold_oracle as orc
from tests import parcel_cases as pc

pytestmark = pytest.mark.gpu

EPS = 1.0e-5                  # tests/test_gpu_mfma.py, tests/test_gpu_sparse_tiles.py
T_R = 0.75


def rel_rows(a, b):
    return np.linalg.norm(a - b, axis=1) / (np.linalg.norm(b, axis=1) + 1e-300)


@pytest.fixture(scope="module")
def solver():
    from pybold_amd import solver as s
    return s


def on_device(case):
    """The tensors of a case of parcel_cases.z_step_case: (Y, taps, steps, lbda, W0)."""
    lbda = case["lbda"] if np.ndim(case["lbda"]) == 0 else torch.from_numpy(np.array(case["lbda"])).cuda()
    W0 = None if case["W0"] is None else torch.from_numpy(np.array(case["W0"])).cuda()
    return (torch.from_numpy(np.array(case["Y"])).cuda(), torch.from_numpy(np.array(case["taps"])).cuda(),
            torch.from_numpy(np.array(case["steps"])).cuda(), lbda, W0)


def rows_of(lbda, r0, r1):
    return lbda if not torch.is_tensor(lbda) else lbda[r0:r1].contiguous()


def expanded(taps, steps):
    """One copy of its parcel's HRF and step per row, made on the host side of the call."""
    idx = torch.from_numpy(pc.row_parcel()).cuda()
    return taps.index_select(0, idx).contiguous(), steps.index_select(0, idx).contiguous()


def check_against_oracle(case, W, nd, tag):
    err = rel_rows(W.cpu().numpy(), case["ref"])
    print("grouped z-step N=%d K=%d %s %s: worst rel L2 vs the float64 oracle %.3e (row %d)"
          % (case["N"], case["K"], case["variant"], tag, err.max(), int(err.argmax())))
    assert bool(torch.isfinite(W).all())
    nd = nd.cpu().numpy()
    assert (nd == case["n_iter"]).all(), np.where(nd != case["n_iter"])[0]      # no row handed back, none left out
    assert err.max() < EPS, (tag, float(err.max()), int(err.argmax()))


# ---- 2 (a): every compiled instance against the float64 oracle ---------------------------------------------------------
@pytest.mark.parametrize("variant", pc.VARIANTS)
@pytest.mark.parametrize("N,K", pc.INSTANCE_SHAPES)
def test_every_matrix_pipe_instance_against_the_oracle(solver, N, K, variant):
    """`force="mfmaonly"` on the ten-parcel layout: launch_mfma_grouped<NB> for NB = 5 .. 10 at the first and the last
    length of its range, the sparse kernel (K = 1, 2, 17, 32) and the dense GROUPED kernel (K = 33); cold start with one
    lambda, warm start with one lambda per row.  All 84 rows run their 60 iterations on the matrix pipe -- none is handed
    back: the inputs sit four times inside the accuracy guard by the oracle's own figures --, every row within 1e-5 of
    the oracle, the result finite (the NaN taps and steps of the empty parcels are never read), the warm start unmodified."""
    case = pc.z_step_case(N, K, variant)
    Y, taps, steps, lbda, W0 = on_device(case)
    before = None if W0 is None else W0.clone()
    W, nd = solver.fista_solve_grouped(Y, taps, steps, pc.OFFSETS, lbda, case["n_iter"], W0=W0, force="mfmaonly")
    check_against_oracle(case, W, nd, "mfmaonly")
    if W0 is not None:
        assert torch.equal(W0, before) and W.data_ptr() != W0.data_ptr()


# ---- 2 (b): independence of parcels, bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("N,K", pc.BIT_SHAPES + [pc.RECORDED_SHAPE])
def test_parcels_are_independent_bit_for_bit(solver, N, K):
    """Every non-empty parcel solved alone -- a grouped call with G = 1 on its rows, taps, step and lambda rows, the same
    instantiation -- gives the bits the ten-parcel call gives for those rows: the columns of a matrix product are
    independent, so a leak between parcels, a wrong unit-table row or a wrong tap row shows here.  The comparison with the
    shared form (`fista_solve_pp`, one HRF in device memory, force="mfmaonly") for parcels of two rows or more is printed,
    and asserted at 150 scans with 27 taps, where profiles/bd_parcels.txt records it.  (Seen on an MI355X,
    profiles/parcels_variants.txt: equal wherever the shared form itself runs on the matrix pipe -- route_pp sends it there
    only where the vector entry of the shape carries the pair form, 161 .. 304 scans at 32 taps; at 129 .. 160 and 310
    scans with 32 taps and everywhere with 33 taps it solves on a vector form, another arithmetic.)"""
    case = pc.z_step_case(N, K, "warm")
    Y, taps, steps, lbda, W0 = on_device(case)
    n_iter = case["n_iter"]
    W, nd = solver.fista_solve_grouped(Y, taps, steps, pc.OFFSETS, lbda, n_iter, W0=W0, force="mfmaonly")
    shared_equal = {}
    for g in pc.NONEMPTY:
        r0, r1 = int(pc.OFFSETS[g]), int(pc.OFFSETS[g + 1])
        args = (Y[r0:r1].contiguous(), taps[g:g + 1].contiguous(), steps[g:g + 1].contiguous())
        Wa, nda = solver.fista_solve_grouped(*args, [0, r1 - r0], rows_of(lbda, r0, r1), n_iter, W0=W0[r0:r1].contiguous(),
                                             force="mfmaonly")
        assert torch.equal(nd[r0:r1], nda), g
        assert torch.equal(W[r0:r1], Wa), (g, float((W[r0:r1] - Wa).abs().max()))
        if r1 - r0 >= 2:
            Ws, nds = solver.fista_solve_pp(args[0], taps[g].contiguous(), args[2], rows_of(lbda, r0, r1), n_iter,
                                            W0=W0[r0:r1].contiguous(), force="mfmaonly")
            shared_equal[pc.SIZES[g]] = bool(torch.equal(W[r0:r1], Ws)) and bool(torch.equal(nd[r0:r1], nds))
    print("grouped z-step N=%d K=%d warm: every parcel alone (G = 1) bit-equal; equal to the shared form's rows, by parcel size: %s"
          % (N, K, shared_equal))
    if (N, K) == pc.RECORDED_SHAPE:
        assert all(shared_equal.values()), shared_equal


# ---- 2 (c): layout -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force", ["mfmaonly", None])
@pytest.mark.parametrize("N,K", pc.LAYOUT_SHAPES)
def test_padded_leading_dimensions_and_guard_bands(solver, N, K, force):
    """Y, the taps (ldt > K) and the in-place iterate as windows of larger allocations (tests/frames.py): the inputs are
    untouched, W is untouched outside its window and written everywhere inside, and the result has the bits of the packed
    call -- on the matrix pipe and on the vector route (grouped_expand_kernel reads the padded tap rows there)."""
    from tests import frames
    case = pc.z_step_case(N, K, "warm")
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


# ---- 2 (d), (e): the vector route ----------------------------------------------------------------------------------------
def vector_route(solver, case, force):
    """A grouped call on the per-problem vector forms against the oracle, and against `fista_solve_pp` with the same flags
    on taps and steps expanded per row by the caller: the same entry point with the same arguments, so any difference is
    grouped_expand_kernel's."""
    Y, taps, steps, lbda, W0 = on_device(case)
    W, nd = solver.fista_solve_grouped(Y, taps, steps, pc.OFFSETS, lbda, case["n_iter"], W0=W0, force=force)
    check_against_oracle(case, W, nd, "force=%s" % force)
    taps_rows, step_rows = expanded(taps, steps)
    assert bool(torch.isfinite(taps_rows).all())
    Wp, ndp = solver.fista_solve_pp(Y, taps_rows, step_rows, lbda, case["n_iter"], W0=W0, force=force)
    assert torch.equal(nd, ndp)
    assert torch.equal(W, Wp), float((W - Wp).abs().max())


@pytest.mark.parametrize("variant", pc.VARIANTS)
@pytest.mark.parametrize("force", [None, "valu"])
@pytest.mark.parametrize("N,K", pc.ROUTE_SHAPES)
def test_the_other_routes_at_matrix_pipe_shapes(solver, N, K, force, variant):
    """84 rows stay below the matrix pipe's row threshold, so the default dispatch takes the vector route as force="valu"
    does."""
    vector_route(solver, pc.z_step_case(N, K, variant), force)


@pytest.mark.parametrize("variant", pc.VARIANTS)
@pytest.mark.parametrize("N,K", pc.VECTOR_SHAPES)
def test_shapes_with_no_matrix_pipe_form(solver, N, K, variant):
    """128 and 311 scans, 34 taps, a short and a long series: the default dispatch is the vector route, and forcing the
    matrix pipe is an error."""
    from pybold_amd import _lib
    case = pc.z_step_case(N, K, variant)
    vector_route(solver, case, None)
    Y, taps, steps, lbda, W0 = on_device(case)
    with pytest.raises(_lib.PyboldHipError):
        solver.fista_solve_grouped(Y, taps, steps, pc.OFFSETS, lbda, case["n_iter"], W0=W0, force="mfma")


# ---- 2 (f): whole rounds ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_batch(sizes):
    """The data of test_gpu_parcels.py::test_grouped_z_step_whole_rounds_and_the_rows_behind_them for other parcel sizes:
    150 scans, 27 taps, dilations 0.8, 1.2, 1.5, lambda = 0.05 x the smallest lambda_max of the first 64 rows."""
    from pybold_amd import data, solver
    N = 150
    off = np.concatenate([[0], np.cumsum(sizes)])
    taps = torch.from_numpy(np.stack([orc.spm_hrf(th, T_R, 20.0, False)[0] for th in (0.8, 1.2, 1.5)])).cuda()
    Y, _, _ = data.gen_rnd_bloc_bold_batch(int(sum(sizes)), dur=N * T_R / 60.0, tr=T_R, hrf=taps[1].cpu().numpy(), nb_events=5,
                                           avg_dur=12.0, std_dur=1.0, snr=10.0, seed=2)
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


def needs_1024_wave_rounds():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip("the whole-round split is laid out for 256 compute units (rounds of 1 024 waves); this device has %d" % cus)


def test_whole_rounds_with_a_large_remainder_stay_on_the_matrix_pipe(solver):
    """20 884 rows in parcels of 10 000, 10 584 and 300 are 1 306 waves: the whole round ends at row 16 384, inside the
    second parcel, and the 4 500 rows behind it are more than GROUPED_MFMA_MIN_P, so nothing is split off (capi.hip, the
    branch `P - cut <= GROUPED_MFMA_MIN_P` not taken): the default call has the bits of the forced ones.  At this lambda
    the accuracy guard hands some rows back (n_done = -1 under "mfmaonly", which leaves them unsolved); the default call
    re-solves those on the vector forms as force="mfma" does, so it equals the "mfma" call on every row and the "mfmaonly"
    call on every row that call solved -- rows behind row 16 384 among them."""
    needs_1024_wave_rounds()
    sizes = (10000, 10584, 300)
    Y, taps, steps, off, lbda = big_batch(sizes)
    po = solver.ParcelOffsets(off, Y.device)
    assert po.waves() == 625 + 662 + 19 and 10000 + (1024 - 625) * 16 == 16384 and po.rows - 16384 == 4500
    W, nd = solver.fista_solve_grouped(Y, taps, steps, po, lbda, 20)
    Wf, ndf = solver.fista_solve_grouped(Y, taps, steps, po, lbda, 20, force="mfmaonly")
    Wm, ndm = solver.fista_solve_grouped(Y, taps, steps, po, lbda, 20, force="mfma")
    kept = ndf == 20
    print("whole rounds with a large remainder: the accuracy guard hands back %d of %d rows, %d of the %d behind row 16 384"
          % (int((~kept).sum()), po.rows, int((~kept[16384:]).sum()), po.rows - 16384))
    assert bool((ndf[~kept] == -1).all()) and bool(kept[16384:].any()) and bool(kept[:16384].any())
    assert int(nd.min()) == 20 and int(nd.max()) == 20 and torch.equal(nd, ndm)
    assert torch.equal(W, Wm)
    assert torch.equal(W[kept], Wf[kept])
    V = po.rows
    rows_against_oracle(Y, taps, steps, off, lbda, W, ((0, 17), (9992, 10009), (16376, 16393), (V - 16, V)), 20)


def test_rows_behind_the_whole_rounds_are_the_vector_routes(solver):
    """The 17 000 rows of test_grouped_z_step_whole_rounds_and_the_rows_behind_them (one whole round, 624 rows behind it
    on the vector forms): the rows behind the cut have the bits of a force="valu" call on those 624 rows -- 8 of the second
    parcel, the third parcel -- and the rows before it, those the accuracy guard does not hand back, the bits of the
    force="mfmaonly" call.  (A force="valu" call on all 17 000 rows is no bit-level reference for the rows behind the cut:
    route_pp picks the vector form from the number of rows, one problem per wave for 624 and the single-row form for
    17 000, two arithmetics 3.7e-9 apart here; both are held to 1e-5 of the oracle on every row behind the cut.)"""
    needs_1024_wave_rounds()
    sizes = (9000, 7384, 616)
    Y, taps, steps, off, lbda = big_batch(sizes)
    po = solver.ParcelOffsets(off, Y.device)
    assert po.waves() == 563 + 462 + 39
    cut = 9000 + (1024 - 563) * 16
    W, nd = solver.fista_solve_grouped(Y, taps, steps, po, lbda, 20)
    Wv, ndv = solver.fista_solve_grouped(Y, taps, steps, po, lbda, 20, force="valu")
    Wf, ndf = solver.fista_solve_grouped(Y, taps, steps, po, lbda, 20, force="mfmaonly")
    assert int(nd.min()) == 20 and int(ndv.min()) == 20
    assert cut == 16376 and off[2] - cut == 8
    Wb, ndb = solver.fista_solve_grouped(Y[cut:].contiguous(), taps[1:].contiguous(), steps[1:].contiguous(), [0, 8, 624], lbda, 20,
                                         force="valu")
    assert int(ndb.min()) == 20
    print("rows behind the whole rounds: max |difference| to force='valu' on those rows alone %.3e, to force='valu' on all rows %.3e"
          % (float((W[cut:] - Wb).abs().max()), float((W[cut:] - Wv[cut:]).abs().max())))
    assert torch.equal(W[cut:], Wb)
    rows_against_oracle(Y, taps, steps, off, lbda, W, ((cut, po.rows),), 20)
    rows_against_oracle(Y, taps, steps, off, lbda, Wv, ((cut, po.rows),), 20)
    kept = (ndf == 20)[:cut]
    print("rows behind the whole rounds: the accuracy guard hands back %d of the %d rows before the cut" % (int((~kept).sum()), cut))
    assert bool(kept.any()) and torch.equal(W[:cut][kept], Wf[:cut][kept])


# ---- 3: bd_parcels off the matrix pipe ------------------------------------------------------------------------------------
class _OneProcess:                                   # the oracle loop never talks to other ranks
    world_size, rank = 1, 0

    @staticmethod
    def allreduce_(t):
        return t


BD_SIZES, BD_THETA, BD_LABELS = [1, 17, 5], [0.7, 1.3, 1.0], [12, -4, 30]
NB_ITER, NB_INNER = 3, 40


@pytest.mark.parametrize("N,dur,K", [(100, 20.0, 27), (150, 25.0, 34)])
def test_bd_parcels_whole_loop_off_the_matrix_pipe(solver, N, dur, K):
    """`bd_parcels` where no z-step has a matrix-pipe form -- 100 scans; 150 scans with a 25 s HRF of 34 taps -- against
    the float64 oracle loop of every parcel alone, with the assertions and the theta bound of
    test_gpu_parcels.py::test_bd_parcels_whole_loop_against_the_per_parcel_oracle_loops; force="mfma" is an error."""
    import pybold_amd
    from oracle.shared_ops import OracleOps
    from pybold_amd import _lib, data, distributed
    assert len(orc.spm_hrf(2.0, T_R, dur, False)[0]) == K
    rows = []
    for p, (n, th) in enumerate(zip(BD_SIZES, BD_THETA)):
        h = orc.spm_hrf(th, T_R, dur, False)[0]
        Yp, _, _ = data.gen_rnd_bloc_bold_batch(n, dur=N * T_R / 60.0, tr=T_R, hrf=h, nb_events=5, avg_dur=12.0, std_dur=1.0, snr=10.0,
                                                seed=23 + p)
        assert Yp.shape == (n, N)
        rows.append(Yp)
    Y = torch.cat(rows).contiguous()
    lbda = 0.05 * float(solver.lambda_max(Y, orc.spm_hrf(2.0, T_R, dur, False)[0]).min())
    offsets = np.concatenate([[0], np.cumsum(BD_SIZES)])
    V = int(offsets[-1])
    perm = np.random.RandomState(5).permutation(V)
    labels = np.repeat(BD_LABELS, BD_SIZES)[perm]
    Ysh = Y[torch.from_numpy(perm).cuda()].contiguous()
    kw = dict(lbda=lbda, theta_0=2.0, hrf_dur=dur, nb_iter=NB_ITER, nb_inner=NB_INNER)
    loops, worst_shared = [], 0.0
    for p in range(len(BD_SIZES)):
        Yp = Y[offsets[p]:offsets[p + 1]]
        Wo, ho, do = distributed.bd_shared(Yp.cpu(), T_R, ops=OracleOps(N, T_R, dur), comm=_OneProcess(), **kw)
        Ws, hs, ds = distributed.bd_shared(Yp, T_R, **kw)
        loops.append(dict(W=Wo.numpy(), h=np.asarray(ho), theta=np.asarray(do["theta"], dtype=np.float64), J=np.asarray(do["J"])))
        worst_shared = max(worst_shared, float(np.abs(np.asarray(ds["theta"], dtype=np.float64) - loops[-1]["theta"]).max()))
    X, Z, W, H, d = pybold_amd.bd_parcels(Ysh, labels, T_R, **kw)
    G = len(BD_SIZES)
    assert X.shape == Z.shape == W.shape == (V, N) and X.dtype == Z.dtype == W.dtype == torch.float64
    assert H.shape == (G, K) and d["theta"].shape == (NB_ITER + 1, G) and d["J"].shape == (NB_ITER + 2, G)
    assert list(d["labels"]) == sorted(BD_LABELS)
    assert list(d["sizes"]) == [BD_SIZES[BD_LABELS.index(lab)] for lab in sorted(BD_LABELS)]
    worst = 0.0
    X, Z, W, H = (t.cpu().numpy() for t in (X, Z, W, H))
    for g, lab in enumerate(d["labels"]):
        o = loops[BD_LABELS.index(int(lab))]
        mine = np.where(labels == lab)[0]                               # this parcel's rows in the caller's order ...
        gen = perm[mine] - offsets[BD_LABELS.index(int(lab))]           # ... and in the oracle loop's order
        Wo = o["W"][gen]
        Zo = np.cumsum(Wo, axis=1)
        Xo = orc.causal_conv(o["h"], Zo)
        for got, want in ((W[mine], Wo), (Z[mine], Zo), (X[mine], Xo)):
            assert rel_rows(got, want).max() < 1e-5, (lab, rel_rows(got, want).max())
        np.testing.assert_allclose(d["J"][:, g], o["J"], rtol=1e-6)
        np.testing.assert_allclose(H[g], orc.spm_hrf(float(d["theta"][-1, g]), T_R, dur, False)[0], rtol=1e-10, atol=1e-14)
        worst = max(worst, float(np.abs(d["theta"][:, g] - o["theta"]).max()))
    print("bd_parcels off the matrix pipe, N=%d K=%d, parcels of %s voxels, 3 x 40 iterations: worst |dtheta| vs the per-parcel "
          "oracle loops %.3e; bd_shared on each parcel alone: %.3e" % (N, K, BD_SIZES, worst, worst_shared))
    assert worst <= max(2.0 * worst_shared, 1e-6), (worst, worst_shared)
    with pytest.raises(_lib.PyboldHipError):
        pybold_amd.bd_parcels(Ysh, labels, T_R, force="mfma", **kw)


# ---- 4: grouped normal equations against orc.hrf_normal_eq ------------------------------------------------------------------
def check_normal_equations(got, ref, sizes):
    assert got.shape == ref.shape
    for g, n in enumerate(sizes):
        if n == 0:
            assert (got[g] == 0).all(), g                                # exact zeros
            continue
        np.testing.assert_allclose(got[g, :-1], ref[g, :-1], rtol=1e-11, atol=1e-11 * max(np.abs(ref[g, :-1]).max(), 1e-300),
                                   err_msg="parcel %d" % g)
        np.testing.assert_allclose(got[g, -1], ref[g, -1], rtol=1e-12, err_msg="||w||_1 of parcel %d" % g)


@pytest.mark.parametrize("N,K", pc.NE_KERNEL_SHAPES)
def test_grouped_normal_equations_on_each_kernel(solver, N, K):
    """The ten-parcel layout on the register form <float, 12, 5> ((150, 27), (40, 1)), on the generic wave form past each of
    the register form's limits ((150, 28): K^2 > 768; (321, 27): N > 320; (150, 32)), and on normal_eq_sum_grouped_kernel
    for 33 taps and -- (2069, 32): by csrc/blind.h ne_wave_lds_doubles = 4 (sk(N + 16) + sk(N + K + 16) + 2) + K^2 + 2 K + 2
    with sk(i) = i + i / 8, which is 20 002 > LDS_DOUBLES_MAX = 20 000 first at 2 069 scans for 32 taps -- below 33 taps.
    Empty parcels give exact zeros, two calls the same bits."""
    W, Y, ref, off = pc.ne_case(tuple(pc.SIZES), N, K)
    Wd, Yd = torch.from_numpy(np.array(W)).cuda(), torch.from_numpy(np.array(Y)).cuda()
    got = solver.hrf_normal_eq_w_grouped(Wd, Yd, K, off)
    again = solver.hrf_normal_eq_w_grouped(Wd, Yd, K, off)
    assert torch.equal(got, again)
    print("grouped normal equations N=%d K=%d: the %s kernel" % (N, K, pc.ne_kernel(N, K)))
    check_normal_equations(got.cpu().numpy(), ref, pc.SIZES)


@pytest.mark.parametrize("N,K", pc.NE_FRAMED_SHAPES)
def test_grouped_normal_equations_framed(solver, N, K):
    """The generic wave form and the sum form with padded leading dimensions and guard bands around W, Y and the output."""
    from tests import frames
    W, Y, ref, off = pc.ne_case(tuple(pc.SIZES), N, K)
    G = len(pc.SIZES)
    fw = frames.frame2d("W", pc.ROWS, N, torch.float64, "cuda", fill=np.array(W))
    fy = frames.frame2d("y", pc.ROWS, N, torch.float32, "cuda", fill=np.array(Y))
    fo = frames.frame2d("out", G, pc.ne_len(K), torch.float64, "cuda")
    for f in (fw, fy, fo):
        f.snapshot()
    got = solver.hrf_normal_eq_w_grouped(fw.view, fy.view, K, off, out=fo.view)
    torch.cuda.synchronize()
    fw.assert_untouched()
    fy.assert_untouched()
    fo.assert_outside_untouched()
    assert not bool(fo.is_sentinel().any())
    packed = solver.hrf_normal_eq_w_grouped(fw.contiguous(), fy.contiguous(), K, off)
    assert torch.equal(fo.view, packed)
    check_normal_equations(got.cpu().numpy(), ref, pc.SIZES)


@pytest.mark.parametrize("name", [c[0] for c in pc.NE_REDUCE_CASES])
def test_grouped_normal_equations_on_every_reduce_width(solver, name):
    """normal_eq_reduce_grouped_kernel at each number of entries per workgroup: the largest parcel on either side of 16, 64
    and 256 units of 16 rows (`ladder-*`: 2^6, 2^4, 2^2, 2^0 entries; the ten-parcel layout above runs 2^8), the width
    raised because 100 parcels x 758 entries would be more than 2^16 workgroups (`raised`), and units of 20 rows at
    20 000 rows (`unit20`)."""
    _, sizes, N, K = [c for c in pc.NE_REDUCE_CASES if c[0] == name][0]
    W, Y, ref, off = pc.ne_case(tuple(sizes), N, K)
    Wd, Yd = torch.from_numpy(np.array(W)).cuda(), torch.from_numpy(np.array(Y)).cuda()
    got = solver.hrf_normal_eq_w_grouped(Wd, Yd, K, off)
    assert torch.equal(got, solver.hrf_normal_eq_w_grouped(Wd, Yd, K, off))
    print("grouped normal equations %s: e_log2 before / after the raise, rows per unit = %s" % (name, pc.ne_case_e_log2(sizes, K)))
    check_normal_equations(got.cpu().numpy(), ref, sizes)
