"""What partial path lengths are for (include/smcrt.h "partial path lengths"): pure numpy on the
records of Engine.partial_paths().

`lengths` is an (n, n_media) array, one row per record; `headers` the structured array that came
with it (abi.ppath_dtype()). Nothing here touches the GPU.
"""
from __future__ import annotations

import numpy as np


def time_of_flight(lengths, n_by_medium, c):
    """sum_m n_m * len_m / c per record: `n_by_medium` the refractive index of each medium, `c`
    the speed of light in vacuum in the scene's length unit per time unit."""
    lengths = np.asarray(lengths, dtype=np.float64)
    n = np.asarray(n_by_medium, dtype=np.float64)
    if lengths.ndim != 2 or n.shape != (lengths.shape[1],):
        raise ValueError("lengths must be (n, n_media) and n_by_medium (n_media,)")
    return (lengths * n).sum(axis=1) / float(c)


def reweight(weights, lengths, mua_from, mua_to):
    """w * exp(-sum_m (mua_to - mua_from)_m * len_m) per record: the weight the record would have
    had if the run had been made with absorption `mua_to` instead of `mua_from` (the same
    scattering, anisotropy and indices). An unchanged absorption gives the weights back bit for
    bit."""
    weights = np.asarray(weights, dtype=np.float64)
    lengths = np.asarray(lengths, dtype=np.float64)
    a, b = np.asarray(mua_from, dtype=np.float64), np.asarray(mua_to, dtype=np.float64)
    if (lengths.ndim != 2 or a.shape != (lengths.shape[1],) or b.shape != a.shape
            or weights.shape != (lengths.shape[0],)):
        raise ValueError("weights must be (n,), lengths (n, n_media) and both mua (n_media,)")
    return weights * np.exp(-(lengths * (b - a)).sum(axis=1))


def tof_histogram(headers, lengths, n_by_medium, c, edges, detector):
    """The weighted time-of-flight histogram of one detector: the records of `detector` binned by
    time_of_flight into `edges` (ascending; bin i holds edges[i] <= t < edges[i + 1], so the left
    edge is inclusive and a time outside [edges[0], edges[-1]) is dropped), each adding its header
    weight."""
    edges = np.asarray(edges, dtype=np.float64)
    if edges.ndim != 1 or len(edges) < 2 or np.any(np.diff(edges) <= 0.0):
        raise ValueError("edges must be at least two ascending values")
    sel = np.asarray(headers["detector"]) == int(detector)
    t = time_of_flight(np.asarray(lengths, dtype=np.float64)[sel], n_by_medium, c)
    w = np.asarray(headers["weight"], dtype=np.float64)[sel]
    idx = np.searchsorted(edges, t, side="right") - 1
    ok = (idx >= 0) & (idx < len(edges) - 1)
    out = np.zeros(len(edges) - 1)
    np.add.at(out, idx[ok], w[ok])
    return out
