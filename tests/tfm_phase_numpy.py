"""NumPy oracle of phase-coherence imaging (include/rtus.h: rtus_tfm_phase).  NumPy only.

Definitions (the header's): p_k is the analytic FMC a[tx, rx] interpolated linearly at the pair's sample position, real and
imaginary parts separately, with tests/tfm_analytic_numpy.py's positions, edge rules and leg rule; p_k = 0 for a pair without a
path or with a position outside the record.  N = T R (tx and rx legs with a path); U = sum of u_k = p_k / |p_k| (0 where p_k = 0);
B = sum of sign(Re p_k); vcf = |U| / N clamped to [0, 1]; scf = 1 - sqrt(1 - (B / N)^2); both NaN when N = 0.

``fp32=False``: everything in fp64 — the definition.
``fp32=True``: the kernel's arithmetic up to p_k — legs (t fs - t0 fs / 2) in fp64 rounded to float32 (-1e8 for a leg without a
path), s = tau_tx + tau_rx in float32, i = floor(s), w = s - i, each part fmaf(w, x[i + 1] - x[i], x[i]) with the difference
rounded to float32.  The fused multiply-add is the fp64 expression w d + x rounded to float32: the product of two float32 is exact
in fp64, so the sum is rounded once in fp64 and its sign (and whether it is zero) is the kernel's.  Signs and zero tests are taken
from that p_k; phasors and sums stay in fp64.  ``kernel_sum=True`` adds U32 / vcf32: the phasors rounded to float32 and summed in
float32 in the kernel's order (receive tiles of 64, then tx ascending, then rx ascending inside the tile).
"""
from fractions import Fraction

import numpy as np

NO_PATH = np.float32(-1.0e8)
RX_TILE = 64


def legs_f32(tt, fs, t0, fused=False):
    """[n_e, n_f] float32: a leg's half of the sample position, NO_PATH where it is not finite or >= 1e8 in magnitude.
    ``fused``: the multiplication and the subtraction as ONE rounding in fp64 (exact rational arithmetic), which is what a
    compiler that contracts t * fs - h computes; a test can hold its cases to give the same float32 either way."""
    tt = np.asarray(tt, dtype=np.float64)
    h = 0.5 * t0 * fs
    with np.errstate(all="ignore"):
        v = tt * fs - h
        if fused:
            fin = np.isfinite(tt)
            F, H = Fraction(float(fs)), Fraction(float(h))
            v[fin] = [float(Fraction(float(t)) * F - H) for t in tt[fin]]
        v = v.astype(np.float32)
        return np.where(np.abs(v) < -NO_PATH, v, NO_PATH)              # NaN fails the compare


def samples(a, fs, t0, tt_tx, tt_rx=None, fp32=False):
    """-> (P [n_tx, n_rx, n_f]: every pair's interpolated sample (complex64 with fp32, else complex128), ok_tx [n_tx, n_f],
    ok_rx [n_rx, n_f]: the legs with a path)"""
    a = np.asarray(a)
    if a.dtype == np.float32 and a.ndim == 4 and a.shape[3] == 2:
        a = np.ascontiguousarray(a).view(np.complex64)[..., 0]
    n_tx, n_rx, n_t = a.shape
    tt_tx = np.asarray(tt_tx, dtype=np.float64)
    tt_rx = tt_tx if tt_rx is None else np.asarray(tt_rx, dtype=np.float64)
    n_f = tt_tx.shape[1]
    rows = np.arange(n_rx)[:, None]
    if fp32:
        a = a.astype(np.complex64)
        tau_tx, tau_rx = legs_f32(tt_tx, fs, t0), legs_f32(tt_rx, fs, t0)
        ok_tx, ok_rx = tau_tx > NO_PATH, tau_rx > NO_PATH
        pad = np.concatenate([a, np.zeros((n_tx, n_rx, 1), dtype=np.complex64)], axis=2)          # sample n_t = 0
        P = np.zeros((n_tx, n_rx, n_f), dtype=np.complex64)
        for tx in range(n_tx):
            s = tau_tx[tx][None, :] + tau_rx                             # float32 + float32 -> float32
            fl = np.floor(s)
            w = (s - fl).astype(np.float64)                              # (the float32 difference, widened)
            ok = (fl >= 0) & (fl < n_t)                                  # no path: s <= -1e8 + 1e8 < 0
            i = np.where(ok, fl, 0).astype(np.int64)
            v0, v1 = pad[tx][rows, i], pad[tx][rows, i + 1]
            re = (w * (v1.real - v0.real).astype(np.float64) + v0.real.astype(np.float64)).astype(np.float32)
            im = (w * (v1.imag - v0.imag).astype(np.float64) + v0.imag.astype(np.float64)).astype(np.float32)
            P[tx].real = np.where(ok, re, np.float32(0))
            P[tx].imag = np.where(ok, im, np.float32(0))
        return P, ok_tx, ok_rx
    a = a.astype(np.complex128)
    with np.errstate(all="ignore"):
        ok_tx, ok_rx = (np.isfinite(v) & (np.abs(v) < np.float32(1e8))     # (the leg rule reads the float32 value: the header's)
                        for v in ((tt_tx * fs - 0.5 * t0 * fs).astype(np.float32), (tt_rx * fs - 0.5 * t0 * fs).astype(np.float32)))
    pad = np.concatenate([a, np.zeros((n_tx, n_rx, 1))], axis=2)
    P = np.zeros((n_tx, n_rx, n_f), dtype=np.complex128)
    for tx in range(n_tx):
        with np.errstate(all="ignore"):
            s = (tt_tx[tx][None, :] + tt_rx - t0) * fs
            ok = ok_tx[tx][None, :] & ok_rx & np.isfinite(s) & (s >= 0) & (s < n_t)
        i = np.where(ok, np.floor(np.where(ok, s, 0.0)), 0).astype(np.int64)
        w = np.where(ok, s - i, 0.0)
        v0, v1 = pad[tx][rows, i], pad[tx][rows, i + 1]
        P[tx] = np.where(ok, (v0.real + w * (v1.real - v0.real)) + 1j * (v0.imag + w * (v1.imag - v0.imag)), 0.0)
    return P, ok_tx, ok_rx


def unit(P):
    """p / |p| in fp64, 0 where p = 0 (the modulus by hypot: no under- or overflow)"""
    re, im = P.real.astype(np.float64), P.imag.astype(np.float64)
    m = np.hypot(re, im)
    with np.errstate(all="ignore"):
        return np.where(m > 0, (re + 1j * im) / m, 0.0)


def vcf_of(U, N):
    """|U| / N clamped to [0, 1]; NaN when N = 0"""
    N = np.asarray(N, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(N == 0, np.nan, np.minimum(np.abs(U) / N, 1.0))


def scf_of(B, N):
    """1 - sqrt(1 - (B / N)^2) in fp64; NaN when N = 0"""
    B, N = np.asarray(B, dtype=np.float64), np.asarray(N, dtype=np.float64)
    with np.errstate(all="ignore"):
        q = B / N
        return np.where(N == 0, np.nan, 1.0 - np.sqrt(1.0 - q * q))


def kernel_order_sum(u):
    """the phasors u [n_tx, n_rx, n_f] rounded to float32 and summed in float32 in the kernel's order -> complex128 [n_f]"""
    n_tx, n_rx, n_f = u.shape
    ur, ui = u.real.astype(np.float32), u.imag.astype(np.float32)
    sr, si = np.zeros(n_f, dtype=np.float32), np.zeros(n_f, dtype=np.float32)
    for r0 in range(0, n_rx, RX_TILE):
        for tx in range(n_tx):
            for r in range(r0, min(r0 + RX_TILE, n_rx)):
                sr = sr + ur[tx, r]
                si = si + ui[tx, r]
    assert sr.dtype == np.float32
    return sr.astype(np.float64) + 1j * si.astype(np.float64)


def tfm_phase(a, fs, t0, tt_tx, tt_rx=None, fp32=False, kernel_sum=False):
    """-> dict(U complex128 [n_f], B int64 [n_f], N int64 [n_f], vcf, scf float64 [n_f]; with ``kernel_sum`` also U32, vcf32)"""
    P, ok_tx, ok_rx = samples(a, fs, t0, tt_tx, tt_rx, fp32)
    u = unit(P)
    N = ok_tx.sum(axis=0).astype(np.int64) * ok_rx.sum(axis=0).astype(np.int64)
    U = u.sum(axis=(0, 1))
    B = np.sign(P.real).astype(np.int64).sum(axis=(0, 1))
    r = dict(U=U, B=B, N=N, vcf=vcf_of(U, N), scf=scf_of(B, N))
    if kernel_sum:
        r["U32"] = kernel_order_sum(u)
        r["vcf32"] = vcf_of(r["U32"], N)
    return r
