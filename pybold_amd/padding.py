"""Padding helpers of the spectral operators, the semantics of ``pybold/padding.py``.

``padd`` / ``unpadd`` add and remove a constant border; ``custom_padd`` lays a series
out as the reference's FFT functions see it: padded to a power of two ``L`` (at least
``min_power_of_2``) with zero runs and mirror images around it.  That layout lives in
one place, :func:`custom_padd_layout`, as an index map: ``custom_padd`` gathers through
it on the host and the spectral kernels gather through the same map on the device.
"""
import math
import numbers

import numpy as np

_PADDTYPES = ("center", "left", "right")


def _check_paddtype(paddtype):
    if paddtype not in _PADDTYPES:
        raise ValueError("paddtype must be one of 'left', 'center', 'right', got %r" % (paddtype,))


def _sides(p, paddtype):
    """(left, right) lengths of a padding ``p`` (int or pair); ``None`` for no padding."""
    if isinstance(p, numbers.Integral):
        p = int(p)
        if p < 1:
            return None
        _check_paddtype(paddtype)
        if paddtype == "left":
            return p, 0
        if paddtype == "right":
            return 0, p
        return p // 2, p - p // 2
    _check_paddtype(paddtype)
    if paddtype != "center":
        raise ValueError("a (left, right) padding only goes with paddtype='center', got %r" % (paddtype,))
    left, right = (int(v) for v in p)
    if left < 0 or right < 0:
        raise ValueError("padding lengths must be non-negative, got %r" % (tuple(p),))
    return left, right


def padd(arrays, p, c=0.0, paddtype="center"):
    """Pad an array (or each array of a list) with ``c``: ``p`` samples split as
    ``p // 2`` left and the rest right (``'center'``), all on one side (``'left'`` /
    ``'right'``), or an explicit ``(left, right)`` pair (``'center'`` only).  An int
    ``p < 1`` returns the input unchanged (pybold/padding.py:122-147)."""
    sides = _sides(p, paddtype)
    if sides is None:
        return arrays

    def one(a):
        a = np.asarray(a)
        return np.concatenate([np.full(sides[0], c, dtype=np.float64), a, np.full(sides[1], c, dtype=np.float64)])
    return [one(a) for a in arrays] if isinstance(arrays, list) else one(arrays)


def unpadd(arrays, p, paddtype="center"):
    """Inverse of :func:`padd` for the same ``p`` and ``paddtype``
    (pybold/padding.py:228-253).  The right border of a ``(left, right)`` pair is
    removed by length, so ``right = 0`` keeps the tail (the reference's ``a[left:-0]``
    would return an empty array there)."""
    sides = _sides(p, paddtype)
    if sides is None:
        return arrays

    def one(a):
        return a[sides[0]:len(a) - sides[1]]
    return [one(a) for a in arrays] if isinstance(arrays, list) else one(arrays)


def custom_padd_layout(n_scans, min_power_of_2=1024, min_zero_padd=50, zero_padd_ratio=0.5):
    """Where each sample of ``custom_padd``'s output comes from, for a series of
    ``n_scans`` samples: returns ``(index_map, p_left)`` with ``index_map`` int32 of
    length ``L`` (entry = sample index, ``-1`` = a padded zero) and ``p_left`` the
    offset of sample 0, so that ``custom_padd(a)[0] == a[index_map]`` with zeros at
    ``-1`` and ``unpadd`` keeps ``[p_left, p_left + n_scans)``.

    ``L`` is the next power of two of ``n_scans``, at least ``min_power_of_2``; the
    ``diff = L - n_scans`` padded samples go ``diff // 2`` left, the rest right.  With
    ``z = max(int(zero_padd_ratio * n_scans), min_zero_padd)`` the layout is

    * ``diff == 0``:          ``[ s ]``
    * ``0 < diff < 2 z``:     ``[ zeros | s | zeros ]``
    * ``2 z < diff < 4 z``:   ``[ zeros(z) | mirror | s | mirror | zeros(z) ]``
    * otherwise:              ``[ zeros(z) | mirror | zeros(z) | s | zeros(z) | mirror | zeros(z) ]``,
      the mirrors reflecting ``zeros(z) | s | zeros(z)``

    (mirrors as ``np.pad(..., mode='reflect')``, edge sample not repeated).  The last
    case has no layout when ``diff == 2 z`` -- 512 scans with the defaults -- and
    raises ``ValueError`` there, as the reference does (pybold/padding.py:283-380)."""
    n = int(n_scans)
    if n < 1:
        raise ValueError("custom_padd: the series must hold at least one sample, got %d" % n)
    m2 = float(min_power_of_2)
    if not (m2 > 0 and math.log2(m2).is_integer()):
        raise ValueError("min_power_of_2 must be a power of two, got %r" % (min_power_of_2,))
    L = max(int(m2), 1 << (n - 1).bit_length())
    diff = L - n
    z = max(int(zero_padd_ratio * n), int(min_zero_padd))
    p_left = diff // 2
    p_right = diff - p_left
    s = np.arange(n, dtype=np.int32)

    def zeros(k):
        return np.full(k, -1, dtype=np.int32)

    if diff == 0:
        idx = s
    elif diff < 2 * z:
        idx = np.concatenate([zeros(p_left), s, zeros(p_right)])
    elif 2 * z < diff < 4 * z:
        idx = np.concatenate([zeros(z), np.pad(s, (p_left - z, p_right - z), mode="reflect"), zeros(z)])
    else:
        if p_left < 2 * z:
            raise ValueError(
                "custom_padd: no zeros-mirror-zeros layout for %d samples padded to %d: the %d padded samples "
                "are exactly two zero runs of %d, which leaves the mirror images a negative length (the "
                "reference fails here too); pad the series by one sample or pick min_zero_padd / "
                "zero_padd_ratio so that 2 * zero run != %d" % (n, L, diff, z, diff))
        inner = np.concatenate([zeros(z), s, zeros(z)])
        idx = np.concatenate([zeros(z), np.pad(inner, (p_left - 2 * z, p_right - 2 * z), mode="reflect"), zeros(z)])
    assert idx.size == L
    return np.ascontiguousarray(idx, dtype=np.int32), p_left


def _custom_padd_one(a, **kw):
    a = np.asarray(a)
    idx, p_left = custom_padd_layout(a.shape[0], **kw)
    if idx.size == a.shape[0]:
        return a, 0
    out = np.zeros(idx.size, dtype=np.result_type(a.dtype, np.float64))
    keep = idx >= 0
    out[keep] = a[idx[keep]]
    return out, (p_left, idx.size - a.shape[0] - p_left)


def custom_padd(arrays, min_power_of_2=1024, min_zero_padd=50, zero_padd_ratio=0.5):
    """Zeros-mirror-zeros padding to a power of two (pybold/padding.py:383-423): returns
    ``(padded, p)`` with ``p = (p_left, p_right)``, or ``p = 0`` when the series already
    has the target length (then the input is returned as is).  ``unpadd(padded, p)``
    gives the series back.  A list is padded array by array and ``p`` is that of its
    first array.  The layout is :func:`custom_padd_layout`."""
    kw = dict(min_power_of_2=min_power_of_2, min_zero_padd=min_zero_padd, zero_padd_ratio=zero_padd_ratio)
    if isinstance(arrays, list):
        done = [_custom_padd_one(a, **kw) for a in arrays]
        return [d[0] for d in done], done[0][1]
    return _custom_padd_one(arrays, **kw)
