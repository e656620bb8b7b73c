"""Restatements of the separable Gaussian smoothing (include/coma_unet.h `coma_gauss_smooth3d`, DESIGN.md section 4 "Target
smoothing"), written from the specification, numpy only.  The GPU tests judge the kernel against these; test_smooth_cpu.py
pins `smooth64` against scipy's gaussian_filter and torch's conv2d.

Along an axis with taps w[0 .. n-1], radius r = (n - 1) / 2:  out[i] = sum_k w[k] v[i - r + k], v outside the volume being 0
("zeros") or the nearest voxel inside ("nearest").  taps_zyx: per axis a 1-D array, or None for an axis that is skipped.

* `smooth64`: fp64 throughout, unrounded taps.
* `smooth32`: the kernel's arithmetic contract -- passes in the order x, y, z; per pass s = 0, then s = fma(w[k], v[k], s) for
  k ascending, taps and values fp32, every fma rounded once to fp32; the result of a pass is what the next pass reads.
* `bound`: the worst-case distance between the two, counted from the operations above."""
import numpy as np

U = 2.0 ** -24                      # fp32 unit roundoff
# the fused multiply-add is emulated in a wider format: the product of two fp32 values is exact in 48 bits, the sum is
# rounded to the wide format and then to fp32.  With x87 extended precision (64-bit significand) the two roundings differ
# from one only when the exact sum lies within 2^-40 ulp of an fp32 tie; with plain fp64 within 2^-29.
WIDE = np.longdouble if np.finfo(np.longdouble).nmant > 52 else np.float64


def _pad(v, axis, r, boundary):
    width = [(0, 0)] * v.ndim
    width[axis] = (r, r)
    return np.pad(v, width, mode="edge" if boundary == "nearest" else "constant")


def _windows(v, axis, n):
    """v padded along `axis` -> the n shifted views out[i] reads, tap order."""
    size = v.shape[axis] - (n - 1)
    return [np.take(v, np.arange(k, k + size), axis=axis) for k in range(n)]


def smooth64(vol, taps_zyx, boundary="zeros"):
    out = np.asarray(vol, dtype=np.float64)
    for axis, w in zip((-1, -2, -3), (taps_zyx[2], taps_zyx[1], taps_zyx[0])):
        if w is None:
            continue
        w = np.asarray(w, dtype=np.float64)
        views = _windows(_pad(out, axis, w.size // 2, boundary), axis, w.size)
        out = sum(wk * v for wk, v in zip(w, views))
    return out


def smooth32(vol, taps_zyx, boundary="zeros"):
    out = np.asarray(vol, dtype=np.float32)
    for axis, w in zip((-1, -2, -3), (taps_zyx[2], taps_zyx[1], taps_zyx[0])):
        if w is None:
            continue
        w = np.asarray(w).astype(np.float32)
        views = _windows(_pad(out, axis, w.size // 2, boundary), axis, w.size)
        s = np.zeros(views[0].shape, dtype=np.float32)
        for wk, v in zip(w, views):
            s = (WIDE(wk) * v.astype(WIDE) + s.astype(WIDE)).astype(np.float32)
        out = s
    return out


def bound(taps_zyx, xmax):
    """|fp32 contract - smooth64| <= this, for |input| <= xmax.  Per pass with n taps, S = sum |w| and inputs bounded by m:
    rounding the taps to fp32 moves the exact sum by <= U S m; the chain's n fused multiply-adds each round a partial sum that
    is itself <= (1 + gamma) S m.  Together <= gamma_{n+1} S m with gamma_j = j U / (1 - j U) (Higham, Accuracy and Stability,
    lemma 3.1); the error the pass inherits is amplified by at most S.  Three passes of radius R with S <= 1 give the first-order
    figure 3 (2R + 2) 2^-24 max|x|."""
    err, m = 0.0, float(xmax)
    for w in (taps_zyx[2], taps_zyx[1], taps_zyx[0]):
        if w is None:
            continue
        w = np.asarray(w, dtype=np.float64)
        S = float(np.abs(w).sum()) * (1 + U)
        j = w.size + 1
        err = S * err + j * U / (1 - j * U) * S * m
        m = S * m + err             # what the next pass reads is the computed value, not the exact one
    return err


def volume(shape, seed):
    """fp32 values in [0, 1) with a few planted large ones, so that a wrong neighbour shows."""
    rng = np.random.default_rng(seed)
    v = rng.random(shape).astype(np.float32)
    flat = v.reshape(-1)
    flat[rng.integers(0, flat.size, max(flat.size // 50, 1))] *= np.float32(4.0)
    return v


# three different asymmetric tap vectors (z: 5 taps, y: 3 taps, x: 9 taps) for the impulse tests: no symmetry hides a
# reversed or swapped axis
ASYM = (np.array([0.05, 0.1, 0.5, 0.25, 0.125]), np.array([0.2, 0.7, 0.15]),
        np.array([0.01, 0.02, 0.03, 0.04, 0.6, 0.11, 0.07, 0.08, 0.09]))
