"""Framed buffers for the layout tests (tests/test_frames_host.py, tests/test_gpu_layout.py): a matrix or a vector that
lives as a WINDOW of a larger allocation -- pad columns left and right of every row, guard rows above and below, guard
elements around a vector -- with everything outside the window holding a sentinel.  A kernel that uses the wrong leading
dimension, assumes an aligned row start or stores past column N - 1 / past the last row changes a sentinel or reads one
(a quiet NaN: it poisons the result), and the checkers below name the first cell.

Comparisons are on BIT PATTERNS through an integer view (NaN != NaN: comparing values would see nothing).  A plain
helper module: no fixtures, no pytest configuration.  The call wrappers at the end go through the ctypes handle of the
package (`pybold_amd._lib.load()`) and pass `.ptr` / `.ld` of the frames."""
import numpy as np
import torch

# ---- sentinels: quiet NaNs with a recognisable payload, fixed patterns for integers ------------------------------
_INT_VIEW = {torch.float64: torch.int64, torch.float32: torch.int32, torch.int32: torch.int32, torch.int64: torch.int64}
SENTINEL_BITS = {torch.float64: 0x7FF8DEADBEEF0BAD, torch.float32: 0x7FC0BEEF,
                 torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}

# ---- layouts (elements): left pad, right pad of every row; guard rows; guard of a vector -----------------------------
# y: the offset is no multiple of 4 elements and the total pad is odd, so row starts alternate in alignment
LAYOUT = {"y": (3, 18), "W": (1, 4), "J": (1, 2), "trace": (1, 2), "taps_pp": (1, 2), "out": (1, 4)}
GUARD_ROWS = 2
GUARD_1D = 64          # even: an int32 workspace behind it stays 8-byte aligned (include/pybold_hip.h, work_dev)


def _to_torch(data, dtype, device):
    if torch.is_tensor(data):
        return data.to(device=device, dtype=dtype)
    return torch.from_numpy(np.ascontiguousarray(data)).to(device=device, dtype=dtype)


class _Frame:
    """Shared part: `ibuf` is the whole allocation as integers, `_mask` is True on the window."""

    def snapshot(self):
        """Remember the bits of the whole allocation (call it right before the call under test)."""
        self._snap = self.ibuf.clone()
        return self

    def _first_change(self, where):
        diff = (self.ibuf != self._snap) & where
        if not bool(diff.any()):
            return None
        return tuple(int(i) for i in torch.nonzero(diff)[0].tolist())

    def _fail(self, cell, what):
        got = int(self.ibuf[cell]) & ((1 << (8 * self.ibuf.element_size())) - 1)
        was = int(self._snap[cell]) & ((1 << (8 * self.ibuf.element_size())) - 1)
        raise AssertionError("%s: %s changed at %s (%s; bits 0x%x -> 0x%x)" % (self.name, what, self._describe(cell),
                                                                                self._region(cell), was, got))

    def assert_outside_untouched(self):
        """Nothing outside the window changed since `snapshot()` (for outputs)."""
        cell = self._first_change(~self._mask)
        if cell is not None:
            self._fail(cell, "a cell outside the window")

    def assert_untouched(self):
        """Nothing in the whole allocation changed since `snapshot()` (for inputs)."""
        cell = self._first_change(torch.ones_like(self._mask))
        if cell is not None:
            self._fail(cell, "an input cell")

    def window_bits(self):
        """The window as a packed integer tensor (bit patterns), for equality checks that must see NaNs."""
        return self.view.contiguous().view(_INT_VIEW[self.dtype])

    def is_sentinel(self):
        """Boolean tensor over the window: cells that still hold the sentinel (never written)."""
        return self.window_bits() == _signed(SENTINEL_BITS[self.dtype], self.dtype)


def _signed(bits, dtype):
    width = 64 if _INT_VIEW[dtype] == torch.int64 else 32
    return bits - (1 << width) if bits >= (1 << (width - 1)) else bits


class Frame2D(_Frame):
    """`rows x cols` window of a `(guard_rows + rows + guard_rows) x (left + cols + right)` allocation.

    fill = None: an OUTPUT window, pre-filled with the sentinel (an unwritten cell shows);
    fill = array / tensor of shape (rows, cols): the data of an input (or in/out) window.
    `.view` the window, `.ptr` its first element, `.ld` the leading dimension in elements, `.contiguous()` a packed copy."""

    def __init__(self, rows, cols, dtype, device, left=0, right=0, guard_rows=0, fill=None, name="frame"):
        self.rows, self.cols, self.dtype, self.name = int(rows), int(cols), dtype, name
        self.left, self.right, self.guard_rows = int(left), int(right), int(guard_rows)
        self.ld = self.left + self.cols + self.right
        total_rows = self.rows + 2 * self.guard_rows
        self.ibuf = torch.full((total_rows, self.ld), _signed(SENTINEL_BITS[dtype], dtype), dtype=_INT_VIEW[dtype],
                               device=device)
        self.buf = self.ibuf.view(dtype)
        self.view = self.buf[self.guard_rows:self.guard_rows + self.rows, self.left:self.left + self.cols]
        if fill is not None:
            self.view.copy_(_to_torch(fill, dtype, device).reshape(self.rows, self.cols))
        self._mask = torch.zeros((total_rows, self.ld), dtype=torch.bool, device=device)
        self._mask[self.guard_rows:self.guard_rows + self.rows, self.left:self.left + self.cols] = True
        self._snap = None

    @property
    def ptr(self):
        return self.view.data_ptr() if self.rows and self.cols else self.buf.data_ptr()

    def contiguous(self):
        return self.view.contiguous()

    def _describe(self, cell):
        r, c = cell
        return "(row %d, column %d) of the window" % (r - self.guard_rows, c - self.left)

    def _region(self, cell):
        r, c = cell
        if r < self.guard_rows or r >= self.guard_rows + self.rows:
            return "guard row"
        if c < self.left:
            return "left pad"
        if c >= self.left + self.cols:
            return "right pad"
        return "inside the window"


class Frame1D(_Frame):
    """`n` elements with `guard` sentinel elements on either side (n_done, lbda, sigma, alpha, workspaces ...)."""

    def __init__(self, n, dtype, device, guard=0, fill=None, name="frame"):
        self.n, self.dtype, self.guard, self.name = int(n), dtype, int(guard), name
        self.ibuf = torch.full((self.n + 2 * self.guard,), _signed(SENTINEL_BITS[dtype], dtype), dtype=_INT_VIEW[dtype],
                               device=device)
        self.buf = self.ibuf.view(dtype)
        self.view = self.buf[self.guard:self.guard + self.n]
        if fill is not None:
            self.view.copy_(_to_torch(fill, dtype, device).reshape(self.n))
        self._mask = torch.zeros((self.n + 2 * self.guard,), dtype=torch.bool, device=device)
        self._mask[self.guard:self.guard + self.n] = True
        self._snap = None
        self.ld = 1

    @property
    def ptr(self):
        return self.view.data_ptr() if self.n else self.buf.data_ptr()

    def contiguous(self):
        return self.view.contiguous()

    def _describe(self, cell):
        return "element %d of the window" % (cell[0] - self.guard)

    def _region(self, cell):
        return "guard" if (cell[0] < self.guard or cell[0] >= self.guard + self.n) else "inside the window"


def frame2d(kind, rows, cols, dtype, device, fill=None, packed=False):
    """A matrix in the layout of its kind (LAYOUT), or -- `packed` -- the same data without pads and guards."""
    left, right = (0, 0) if packed else LAYOUT[kind]
    return Frame2D(rows, cols, dtype, device, left, right, 0 if packed else GUARD_ROWS, fill, name=kind)


def frame1d(name, n, dtype, device, fill=None, packed=False):
    return Frame1D(n, dtype, device, 0 if packed else GUARD_1D, fill, name=name)


# ---- call wrappers: frames in, return code checked ---------------------------------------------------------------------
def _p(f):
    return None if f is None else f.ptr


def _l(f):
    return 0 if f is None else f.ld


def _env():
    from pybold_amd import _lib, solver
    return _lib.load(), _lib, solver


def betas_frame(dev, n_iter):
    """The momentum factors of a call as an input frame of exactly n_iter entries between guards, snapshot taken: the
    wrappers below pass it as betas_dev and return it, for the caller's `assert_untouched()` after the call."""
    _, _, solver = _env()
    return Frame1D(int(n_iter), torch.float64, dev, GUARD_1D, solver._betas_on(dev, n_iter)[:int(n_iter)], name="betas").snapshot()


def _taps(hrf, dev):
    taps = np.ascontiguousarray(np.asarray(hrf, dtype=np.float64).ravel())
    return taps, torch.from_numpy(taps).to(dev)


def fista_solve_ex(y, w, hrf, step, n_iter, lbda=0.0, lbda_v=None, J=None, n_done=None, stop=None, tol=0.0, wind=6,
                   y_rep=1, force=None, cold=False, work=None, lmax=None, dense_ratio=0.0):
    """pb_fista_solve_ex: y Frame2D float32, w Frame2D float64 (in/out), J Frame2D float32, lbda_v / n_done / work /
    lmax Frame1D."""
    lib, _lib, solver = _env()
    dev = w.buf.device
    taps, taps_dev = _taps(hrf, dev)
    betas = betas_frame(dev, n_iter)
    with torch.cuda.device(dev):
        rc = lib.pb_fista_solve_ex(
            y.ptr, y.ld, int(y_rep), w.ptr, w.ld, w.rows, w.cols, taps.ctypes.data, taps_dev.data_ptr(), taps.size,
            float(step), float(lbda), _p(lbda_v), betas.ptr, int(n_iter), _p(J), _l(J), solver._STOP[stop],
            float(tol), int(wind), _p(n_done), solver._FORCE[force] | (_lib.PB_FLAG_COLD_START if cold else 0),
            solver._stream_ptr(dev), _p(lmax), float(dense_ratio), _p(work), work.n if work is not None else 0)
    _lib.check(rc, "pb_fista_solve_ex")
    return betas


def fista_solve_path(y, w, hrf, step, n_iter, lbda_v, lmax, n_done, work, y_rep=1, force=None, cold=False,
                     dense_ratio=0.0):
    lib, _lib, solver = _env()
    dev = w.buf.device
    taps, taps_dev = _taps(hrf, dev)
    betas = betas_frame(dev, n_iter)
    with torch.cuda.device(dev):
        rc = lib.pb_fista_solve_path(
            y.ptr, y.ld, int(y_rep), w.ptr, w.ld, w.rows, w.cols, taps.ctypes.data, taps_dev.data_ptr(), taps.size,
            float(step), _p(lbda_v), _p(lmax), float(dense_ratio), betas.ptr, int(n_iter), _p(n_done), _p(work),
            work.n if work is not None else 0, solver._FORCE[force] | (_lib.PB_FLAG_COLD_START if cold else 0),
            solver._stream_ptr(dev))
    _lib.check(rc, "pb_fista_solve_path")
    return betas


def fista_solve_d(y, w, hrf, step, n_iter, lbda=0.0, lbda_v=None, J=None, n_done=None, stop=None, tol=0.0, wind=6,
                  y_rep=1, force=None, cold=False):
    """pb_fista_solve_d: y Frame2D float64, J Frame2D float64."""
    lib, _lib, solver = _env()
    dev = w.buf.device
    taps, taps_dev = _taps(hrf, dev)
    betas = betas_frame(dev, n_iter)
    with torch.cuda.device(dev):
        rc = lib.pb_fista_solve_d(
            y.ptr, y.ld, int(y_rep), w.ptr, w.ld, w.rows, w.cols, taps.ctypes.data, taps_dev.data_ptr(), taps.size,
            float(step), float(lbda), _p(lbda_v), betas.ptr, int(n_iter), _p(J), _l(J), solver._STOP[stop],
            float(tol), int(wind), _p(n_done), solver._FORCE[force] | (_lib.PB_FLAG_COLD_START if cold else 0),
            solver._stream_ptr(dev))
    _lib.check(rc, "pb_fista_solve_d")
    return betas


def fista_solve_pp(y, w, taps, step_vec, n_iter, K, lbda=0.0, lbda_v=None, n_done=None, stop=None, tol=0.0, force=None,
                   cold=False):
    """pb_fista_solve_pp: `taps` a Frame2D float64 [P][ldt] (per-problem HRFs) or a Frame1D of K taps (ONE shared HRF,
    ldt = 0); `step_vec` Frame1D of P steps (of one step for a shared HRF)."""
    lib, _lib, solver = _env()
    dev = w.buf.device
    betas = betas_frame(dev, n_iter)
    ldt = taps.ld if isinstance(taps, Frame2D) else 0
    with torch.cuda.device(dev):
        rc = lib.pb_fista_solve_pp(
            y.ptr, y.ld, w.ptr, w.ld, w.rows, w.cols, taps.ptr, ldt, int(K), step_vec.ptr, float(lbda), _p(lbda_v),
            betas.ptr, int(n_iter), solver._STOP[stop], float(tol), _p(n_done),
            solver._FORCE[force] | (_lib.PB_FLAG_COLD_START if cold else 0), solver._stream_ptr(dev))
    _lib.check(rc, "pb_fista_solve_pp")
    return betas


def fista_solve_backtrack_d(y, w, hrf, step0, n_iter, lbda=0.0, lbda_v=None, n_done=None, step_out=None, halvings=None,
                            eta=0.5, max_halvings_per_iter=40, y_rep=1, cold=False):
    lib, _lib, solver = _env()
    dev = w.buf.device
    _, taps_dev = _taps(hrf, dev)
    betas = betas_frame(dev, n_iter)
    with torch.cuda.device(dev):
        rc = lib.pb_fista_solve_backtrack_d(
            y.ptr, y.ld, int(y_rep), w.ptr, w.ld, w.rows, w.cols, taps_dev.data_ptr(), taps_dev.numel(), float(step0),
            float(eta), int(max_halvings_per_iter), float(lbda), _p(lbda_v), betas.ptr, int(n_iter), _p(n_done),
            _p(step_out), _p(halvings), _lib.PB_FLAG_COLD_START if cold else 0, solver._stream_ptr(dev))
    _lib.check(rc, "pb_fista_solve_backtrack_d")
    return betas


def auto_lbda_d(y, w, hrf, step, sigma, nb_iter, nb_sub_iter, R=None, G=None, J=None, alpha=None, lbda=None,
                n_outer=None, n_inner=None, work=None, early_stopping=True, tol=1.0e-6, wind=6, outer_chunk=0, cold=False):
    """pb_auto_lbda_d: y, w Frame2D float64; R / G / J Frame2D float64 of one leading dimension; sigma, alpha, lbda
    (float64), n_outer (int32), n_inner (int64), work (float64) Frame1D."""
    lib, _lib, solver = _env()
    dev = w.buf.device
    taps, _ = _taps(hrf, dev)
    betas = betas_frame(dev, nb_sub_iter)
    tr = [t for t in (R, G, J) if t is not None]
    assert len({t.ld for t in tr}) <= 1
    with torch.cuda.device(dev):
        rc = lib.pb_auto_lbda_d(
            y.ptr, y.ld, w.ptr, w.ld, int(bool(cold)), w.rows, w.cols, taps.ctypes.data, taps.size, float(step),
            betas.ptr, sigma.ptr, int(bool(early_stopping)), float(tol), int(wind), int(nb_iter), int(nb_sub_iter),
            int(outer_chunk), _p(R), _p(G), _p(J), tr[0].ld if tr else 0, _p(alpha), _p(lbda), _p(n_outer), _p(n_inner),
            work.ptr, work.n, solver._stream_ptr(dev))
    _lib.check(rc, "pb_auto_lbda_d")
    return betas


def fista_outputs(w, hrf, z=None, x=None):
    lib, _lib, solver = _env()
    dev = w.buf.device
    _, taps_dev = _taps(hrf, dev)
    with torch.cuda.device(dev):
        rc = lib.pb_fista_outputs(w.ptr, w.ld, w.rows, w.cols, taps_dev.data_ptr(), taps_dev.numel(), _p(z), _l(z), _p(x),
                                  _l(x), solver._stream_ptr(dev))
    _lib.check(rc, "pb_fista_outputs")


def fista_outputs_pp(w, taps, K, z=None, x=None):
    lib, _lib, solver = _env()
    dev = w.buf.device
    with torch.cuda.device(dev):
        rc = lib.pb_fista_outputs_pp(w.ptr, w.ld, w.rows, w.cols, taps.ptr, taps.ld, int(K), _p(z), _l(z), _p(x), _l(x),
                                     solver._stream_ptr(dev))
    _lib.check(rc, "pb_fista_outputs_pp")


def fista_stats(w, y, hrf, r2, l1, y_rep=1):
    """pb_fista_stats (float32 y) or pb_fista_stats_d (float64 y), by the dtype of the y frame."""
    lib, _lib, solver = _env()
    dev = w.buf.device
    _, taps_dev = _taps(hrf, dev)
    fn, name = (lib.pb_fista_stats_d, "pb_fista_stats_d") if y.dtype == torch.float64 else (lib.pb_fista_stats, "pb_fista_stats")
    with torch.cuda.device(dev):
        rc = fn(w.ptr, w.ld, y.ptr, y.ld, int(y_rep), w.rows, w.cols, taps_dev.data_ptr(), taps_dev.numel(), r2.ptr, l1.ptr,
                solver._stream_ptr(dev))
    _lib.check(rc, name)


def lambda_max(y, hrf, out):
    """pb_lambda_max (float32 y) or pb_lambda_max_d (float64 y)."""
    lib, _lib, solver = _env()
    dev = y.buf.device
    _, taps_dev = _taps(hrf, dev)
    fn, name = (lib.pb_lambda_max_d, "pb_lambda_max_d") if y.dtype == torch.float64 else (lib.pb_lambda_max, "pb_lambda_max")
    with torch.cuda.device(dev):
        rc = fn(y.ptr, y.ld, y.rows, y.cols, taps_dev.data_ptr(), taps_dev.numel(), out.ptr, solver._stream_ptr(dev))
    _lib.check(rc, name)


def hrf_normal_eq_w(w, y, K, work, out):
    lib, _lib, solver = _env()
    dev = w.buf.device
    with torch.cuda.device(dev):
        rc = lib.pb_hrf_normal_eq_w(w.ptr, w.ld, y.ptr, y.ld, w.rows, w.cols, int(K), work.ptr, work.n, out.ptr,
                                    solver._stream_ptr(dev))
    _lib.check(rc, "pb_hrf_normal_eq_w")


# ---- the row-in-LDS helpers (tests/test_gpu_helper_kernels.py) -----------------------------------------------------------
def _taps_dev(taps, dev):
    """Taps as a packed device vector; None (the two scans take none) passes as a null pointer."""
    if taps is None:
        return None, 0, 0
    t = _taps(taps, dev)[1]
    return t, t.data_ptr(), t.numel()


def _op(name, x, out, n_in, n_out, taps):
    """pb_conv / pb_corr / pb_op_forward / pb_op_adjoint: x and out are Frame2D float64 of the same number of rows."""
    lib, _lib, solver = _env()
    dev = x.buf.device
    keep, ptr, K = _taps_dev(taps, dev)
    with torch.cuda.device(dev):
        rc = getattr(lib, name)(x.ptr, x.ld, out.ptr, out.ld, x.rows, int(n_in), int(n_out), ptr, K, solver._stream_ptr(dev))
    _lib.check(rc, name)


def _integ(name, x, out):
    lib, _lib, solver = _env()
    dev = x.buf.device
    with torch.cuda.device(dev):
        rc = getattr(lib, name)(x.ptr, x.ld, out.ptr, out.ld, x.rows, x.cols, solver._stream_ptr(dev))
    _lib.check(rc, name)


def integ_op(x, out):
    _integ("pb_integ_op", x, out)


def integ_adj(x, out):
    _integ("pb_integ_adj", x, out)


def conv(x, out, hrf):
    """x: n_in columns, out: n_out columns."""
    _op("pb_conv", x, out, x.cols, out.cols, hrf)


def corr(r, out, hrf):
    """r: n_out columns (the range of the Toeplitz matrix), out: n_in columns."""
    _op("pb_corr", r, out, out.cols, r.cols, hrf)


def op_forward(x, out, hrf):
    _op("pb_op_forward", x, out, x.cols, out.cols, hrf)


def op_adjoint(r, out, hrf):
    _op("pb_op_adjoint", r, out, out.cols, r.cols, hrf)


def _hrf_cost(base, z, y, taps, K, n_hrf, cost):
    lib, _lib, solver = _env()
    dev = z.buf.device
    name = base + ("_d" if y.dtype == torch.float64 else "")
    with torch.cuda.device(dev):
        rc = getattr(lib, name)(z.ptr, z.ld, y.ptr, y.ld, z.rows, z.cols, taps.ptr, int(K), int(n_hrf), cost.ptr,
                                solver._stream_ptr(dev))
    _lib.check(rc, name)


def hrf_cost(z, y, taps, K, n_hrf, cost):
    """pb_hrf_cost (float32 y) or pb_hrf_cost_d: taps a Frame1D of n_hrf * K packed taps, cost a Frame1D of n_hrf * V."""
    _hrf_cost("pb_hrf_cost", z, y, taps, K, n_hrf, cost)


def hrf_cost_pv(z, y, taps, K, n_hrf, cost):
    """pb_hrf_cost_pv (float32 y) or pb_hrf_cost_pv_d: taps a Frame1D of n_hrf * V * K packed taps."""
    _hrf_cost("pb_hrf_cost_pv", z, y, taps, K, n_hrf, cost)


def gram_frobenius(taps, K, N, out):
    """taps: Frame2D [P][ldt] float64, out: Frame1D of P."""
    lib, _lib, solver = _env()
    dev = taps.buf.device
    with torch.cuda.device(dev):
        rc = lib.pb_gram_frobenius(taps.ptr, taps.ld, taps.rows, int(K), int(N), out.ptr, solver._stream_ptr(dev))
    _lib.check(rc, "pb_gram_frobenius")


def spectral_radius(x0, taps, nb_iter, tol, out):
    """x0, taps: Frame1D float64; out: Frame1D of 2 (norm, steps)."""
    lib, _lib, solver = _env()
    dev = x0.buf.device
    with torch.cuda.device(dev):
        rc = lib.pb_spectral_radius(x0.ptr, x0.n, taps.ptr, taps.n, int(nb_iter), float(tol), out.ptr, solver._stream_ptr(dev))
    _lib.check(rc, "pb_spectral_radius")


def spectral_radius_pp(x0, taps, K, nb_iter, tol, out):
    """x0: Frame2D [V][ldx], taps: Frame2D [V][ldt], out: Frame1D of 2 V."""
    lib, _lib, solver = _env()
    dev = x0.buf.device
    with torch.cuda.device(dev):
        rc = lib.pb_spectral_radius_pp(x0.ptr, x0.ld, x0.rows, x0.cols, taps.ptr, taps.ld, int(K), int(nb_iter), float(tol),
                                       out.ptr, solver._stream_ptr(dev))
    _lib.check(rc, "pb_spectral_radius_pp")


def inf_norm(x, out):
    lib, _lib, solver = _env()
    dev = x.buf.device
    with torch.cuda.device(dev):
        rc = lib.pb_inf_norm(x.ptr, x.ld, out.ptr, out.ld, x.rows, x.cols, solver._stream_ptr(dev))
    _lib.check(rc, "pb_inf_norm")
