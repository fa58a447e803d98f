"""The convolutions of ``pybold/convolution.py``.

* The causal (Toeplitz) half: the dense Toeplitz builder (the reference API hands
  dense ``H`` matrices to ``_loops_deconv``), its inverse (recover the taps from such
  a matrix so the GPU can work matrix-free) and the truncated FIR and its adjoint.
* The spectral half, ``spectral_convolve`` / ``spectral_retro_convolve`` /
  ``spectral_deconvolve`` / ``spectral_retro_deconvolve``: the reference pads a series
  with ``custom_padd`` to ``L`` samples, multiplies spectra and unpads.  That is a
  length-L circular convolution (correlation for the retro forms) of the padded row,
  read at the unpadded positions, and the GPU evaluates it directly through the
  padding's index map (``pb_spectral_conv`` / ``pb_spectral_corr``), without an FFT.

The two halves agree only where the padding leaves at least ``K - 1`` zeros on each
side of the series; :func:`spectral_matches_causal` says where.
"""
import numpy as np
import torch

from .padding import custom_padd_layout


def toeplitz_from_kernel(k, dim_in, dim_out=None):
    """``T[i, j] = k[i - j]`` for ``0 <= i - j < len(k)``, shape
    ``(dim_out, dim_in)`` -- same contract as pybold/convolution.py:105-132."""
    k = np.asarray(k, dtype=np.float64)
    if dim_out is None:
        dim_out = dim_in
    T = np.zeros((dim_out, dim_in))
    for m in range(min(len(k), dim_out)):
        n = min(dim_in, dim_out - m)
        if n <= 0:
            break
        idx = np.arange(n)
        T[idx + m, idx] = k[m]
    return T


def kernel_from_toeplitz(H):
    """Taps of a square causal Toeplitz matrix built by :func:`toeplitz_from_kernel`
    (first column, trailing zeros trimmed).  Raises ``ValueError`` if ``H`` is
    not such a matrix: the GPU solver is matrix-free and supports nothing else."""
    H = np.asarray(H, dtype=np.float64)
    if H.ndim != 2:
        raise ValueError("H must be a 2-D causal Toeplitz matrix")
    col = H[:, 0]
    nz = np.nonzero(col)[0]
    K = int(nz[-1]) + 1 if nz.size else 1
    taps = col[:K].copy()
    if not np.array_equal(H, toeplitz_from_kernel(taps, H.shape[1], H.shape[0])):
        raise ValueError("H is not a causal Toeplitz (convolution) matrix; the "
                         "matrix-free GPU solver cannot represent it")
    return taps


def _rows_on_device(x):
    from . import solver
    a = np.asarray(x, dtype=np.float64)
    one_d = a.ndim == 1
    t = torch.from_numpy(np.ascontiguousarray(a.reshape(1, -1) if one_d else a)).to(solver.device())
    return t, one_d


def simple_convolve(k, x, dim_out=None):
    """``out[i] = sum_m k[m] x[i - m]`` truncated to ``dim_out`` samples -- the
    loop-form definition of pybold/convolution.py:135-164 (== ``toeplitz_from_kernel(k,
    len(x), dim_out) @ x``), evaluated by the GPU Toeplitz-product kernel.  1-D ``x``
    like the reference, or a 2-D batch of rows."""
    from . import solver
    t, one_d = _rows_on_device(x)
    out = solver.conv(t, k, dim_out=t.shape[1] if dim_out is None else int(dim_out)).cpu().numpy()
    return out[0] if one_d else out


def simple_retro_convolve(k, x, dim_out=None):
    """Adjoint form ``out[j] = sum_m k[m] x[j + m]`` (pybold/convolution.py:167-196,
    == ``toeplitz_from_kernel(k, dim_out, len(x)).T @ x``)."""
    from . import solver
    t, one_d = _rows_on_device(x)
    out = solver.corr(t, k, dim_in=t.shape[1] if dim_out is None else int(dim_out)).cpu().numpy()
    return out[0] if one_d else out


def _spectral(k, x, deconvolve, retro):
    from . import solver
    from .linear import _to_dev
    k = np.asarray(k, dtype=np.float64).ravel()
    if k.size < 1:
        raise ValueError("empty kernel")
    t, back = _to_dev(x)
    index_map, p_left = custom_padd_layout(t.shape[1])
    L = index_map.size
    # the reference's filter spectrum is rfft(k, L): k cut to L taps; 1 / rfft(k, L) for the deconvolutions
    filt = np.fft.irfft(1.0 / np.fft.rfft(k, L), L) if deconvolve else k[:L]
    return back(solver.spectral(t, index_map, p_left, filt, corr=retro))


def spectral_convolve(k, x):
    """``k`` convolved with ``x`` through the padded FFT product of pybold/convolution.py:9-31:
    ``x`` padded by ``custom_padd`` to ``L`` samples, circularly convolved with ``k[:L]``,
    unpadded.  Equals :func:`simple_convolve` only where :func:`spectral_matches_causal`.
    1-D ``x`` like the reference, or a 2-D ``(V, N)`` batch of rows; NumPy in -> NumPy
    float64 out, a CUDA tensor in -> a float64 tensor out on its device."""
    return _spectral(k, x, deconvolve=False, retro=False)


def spectral_retro_convolve(k, x):
    """Adjoint form of :func:`spectral_convolve` (conjugate filter spectrum, a circular
    correlation; pybold/convolution.py:34-56)."""
    return _spectral(k, x, deconvolve=False, retro=True)


def spectral_deconvolve(k, x):
    """``x`` circularly filtered with the inverse of ``k``'s length-L spectrum
    (``1 / rfft(k, L)``, pybold/convolution.py:59-79).  A zero bin of that spectrum gives
    non-finite output, as in the reference."""
    return _spectral(k, x, deconvolve=True, retro=False)


def spectral_retro_deconvolve(k, x):
    """Adjoint form of :func:`spectral_deconvolve` (pybold/convolution.py:82-102)."""
    return _spectral(k, x, deconvolve=True, retro=True)


def spectral_matches_causal(n_scans, n_taps):
    """Whether the spectral forms equal the causal truncated FIR and its adjoint
    (:func:`simple_convolve` / :func:`simple_retro_convolve`) for every series of
    ``n_scans`` samples and every filter of ``n_taps`` taps: the ``min(n_taps, L) - 1``
    padded samples on each side of the series (circularly) must all be zeros.  False
    where the padding has no layout (512 scans).  With the default padding and 2 to 64
    taps the forms differ at 342-511 scans (the series against its mirror image), at
    ``L - K + 1 < N <= L`` (zero padding shorter than the filter: the product wraps)
    and at 512."""
    if int(n_taps) < 1:
        raise ValueError("n_taps must be at least 1, got %r" % (n_taps,))
    try:
        index_map, p_left = custom_padd_layout(n_scans)
    except ValueError:
        return False
    L = index_map.size
    d = np.arange(1, min(int(n_taps), L))
    before = index_map[(p_left - d) % L]
    after = index_map[(p_left + int(n_scans) - 1 + d) % L]
    return bool((before < 0).all() and (after < 0).all())
