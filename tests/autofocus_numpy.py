"""Independent NumPy oracle of the adaptive-TFM entries (include/rtus.h: rtus_fmc_analytic, rtus_surface_find) and of the
post-processing of api.measure_surface, plus a generator of surface-echo FMC.  NumPy only, fp64 throughout.

Definitions (the header's): the analytic FMC is x + i (h * x) with the Hamming-windowed FIR Hilbert transformer h; the couplant
image is |sum_tx sum_rx a_tx,rx(s)| over straight rays at speed c1, real and imaginary parts interpolated linearly and separately,
rtus_tfm's edge rules; the column peak is the first index of the column's maximum with a parabolic step clamped to [-1/2, 1/2].
"""
import numpy as np

import surface_numpy as S


def hilbert_taps(n_taps):
    """h[m] for m = -M..M: 2 / (pi m) * Hamming(m) at odd m, 0 at even m"""
    M = (n_taps - 1) // 2
    m = np.arange(-M, M + 1)
    w = 0.54 + 0.46 * np.cos(np.pi * m / M)
    h = np.zeros(n_taps)
    odd = m % 2 != 0
    h[odd] = 2.0 / (np.pi * m[odd]) * w[odd]
    return h


def analytic(fmc, n_taps=63):
    """x + i sum_m h[m] x[n - m] along the last axis; samples outside the record are zero -> complex128"""
    x = np.asarray(fmc, dtype=np.float64)
    M = (n_taps - 1) // 2
    n_t = x.shape[-1]
    pad = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(M, M)])
    im = np.zeros_like(x)
    for i, m in enumerate(range(-M, M + 1)):
        h = hilbert_taps(n_taps)[i]
        if h:
            im += h * pad[..., M - m:M - m + n_t]                        # x[n - m]
    return x + 1j * im


def envelope_image(a, fs, t0, xe, ze, c1, xk, zj):
    """couplant envelope image A[k, j] = |sum_tx sum_rx a[tx, rx](s)|, s = (|E_tx - P| + |E_rx - P|) / c1 fs - t0 fs"""
    a = np.asarray(a)
    n_e, _, n_t = a.shape
    xe, ze = np.asarray(xe, dtype=np.float64), np.asarray(ze, dtype=np.float64)
    px, pz = np.meshgrid(np.asarray(xk, dtype=np.float64), np.asarray(zj, dtype=np.float64), indexing="ij")
    px, pz = px.ravel(), pz.ravel()
    d = np.hypot(xe[:, None] - px[None, :], ze[:, None] - pz[None, :]) / c1 * fs - 0.5 * t0 * fs     # [n_e, n_p]
    pad = np.concatenate([a.astype(np.complex128), np.zeros((n_e, n_e, 1))], axis=2)                 # sample n_t = 0
    acc = np.zeros(px.size, dtype=np.complex128)
    rows = np.arange(n_e)[:, None]
    for tx in range(n_e):
        s = d[tx][None, :] + d
        ok = (s >= 0) & (s < n_t)
        i = np.where(ok, np.floor(s), 0).astype(np.int64)
        w = np.where(ok, s - i, 0.0)
        v0, v1 = pad[tx][rows, i], pad[tx][rows, i + 1]
        acc += np.where(ok, v0 + w * (v1 - v0), 0.0).sum(axis=0)
    return np.abs(acc).reshape(len(xk), len(zj))


def column_peak(A, z_lo, dz):
    """-> (z_peak [n_s], amp [n_s]) by the header's rules"""
    A = np.asarray(A, dtype=np.float64)
    n_s, n_z = A.shape
    fin = np.isfinite(A).all(axis=1)
    j = np.argmax(np.where(np.isfinite(A), A, -1.0), axis=1)            # first index of the maximum
    k = np.arange(n_s)
    amp = np.where(fin, A[k, j], np.nan)
    z = np.full(n_s, np.nan)
    ok = fin & (j > 0) & (j < n_z - 1) & (amp > 0)
    jj = np.clip(j, 1, n_z - 2)
    am, a0, ap = A[k, jj - 1], A[k, jj], A[k, jj + 1]
    with np.errstate(all="ignore"):
        d = np.clip((am - ap) / (2.0 * (am - 2.0 * a0 + ap)), -0.5, 0.5)
    z[ok] = z_lo + (j[ok] + d[ok]) * dz
    return z, amp


def profile(x0, dx, z_peak, amp, threshold=0.1):
    """valid, trim, fill: -> (x0 of the first kept column, zs, valid) or None when fewer than 4 columns remain"""
    z_peak, amp = np.asarray(z_peak, dtype=np.float64), np.asarray(amp, dtype=np.float64)
    top = np.nanmax(amp)
    valid = np.isfinite(z_peak) & np.isfinite(amp) & (amp >= threshold * top)
    idx = np.flatnonzero(valid)
    if idx.size == 0 or idx[-1] - idx[0] + 1 < 4:
        return None
    zs = []
    for k in range(idx[0], idx[-1] + 1):
        if valid[k]:
            zs.append(z_peak[k])
            continue
        lo, hi = idx[idx < k][-1], idx[idx > k][0]                     # nearest valid neighbours
        u = (k - lo) / (hi - lo)
        zs.append(z_peak[lo] + u * (z_peak[hi] - z_peak[lo]))
    return x0 + idx[0] * dx, np.array(zs), valid


def _burst(dt, f0, cycles):
    """oracle/tfm_numpy.synth_fmc's pulse: a Gaussian-windowed tone burst"""
    sig = cycles / f0 / 2.355
    return np.exp(-0.5 * (dt / sig) ** 2) * np.cos(2 * np.pi * f0 * dt)


def _splat(fmc, tx, rx, tau, amp, fs, t0, f0, cycles):
    """add amp * burst(t - tau) to the pairs (tx, rx), each in a short window around its arrival"""
    n_t = fmc.shape[-1]
    half = int(np.ceil(5 * cycles / f0 / 2.355 * fs))
    c = np.rint((tau - t0) * fs).astype(np.int64)
    idx = c[:, None] + np.arange(-half, half + 1)[None, :]
    assert idx.min() >= 0 and idx.max() < n_t, "an echo window crosses the end of the record"
    dt = t0 + idx / fs - tau[:, None]
    fmc[tx[:, None], rx[:, None], idx] += np.asarray(amp)[..., None] * _burst(dt, f0, cycles)


def synth_fmc(xe, ze, c1, fs, n_t, x0, dx, zs, x_lo, x_hi, *, t0=0.0, f0=5e6, cycles=2.5, scatterer=None, c2=None):
    """FMC float32 [n_e, n_e, n_t] of the surface echo: point reflectors every lambda/8 of x (lambda in the couplant) along the
    natural spline through zs (surface_numpy.spline) over [x_lo, x_hi], each weighted by the arc length it stands for, straight rays
    at c1.  ``scatterer`` = (xs, zs, amplitude) below the surface adds its echo with the times of surface_numpy.table (speed c2 in
    the part).  Only tx <= rx is computed; the block is mirrored."""
    xe, ze = np.asarray(xe, dtype=np.float64), np.asarray(ze, dtype=np.float64)
    coef = S.spline(x0, dx, zs)
    h = c1 / f0 / 8
    px = np.arange(x_lo, x_hi + 0.5 * h, h)
    pz, p1, _ = S.spline_eval(coef, x0, dx, px)
    w = h * np.sqrt(1 + p1 * p1) / (c1 / f0)                            # arc length per reflector, in wavelengths
    tx, rx = np.triu_indices(xe.size)
    fmc = np.zeros((xe.size, xe.size, n_t))
    d = np.hypot(xe[:, None] - px[None, :], ze[:, None] - pz[None, :]) / c1
    for p in range(px.size):
        _splat(fmc, tx, rx, d[tx, p] + d[rx, p], w[p], fs, t0, f0, cycles)
    if scatterer is not None:
        xs, zsc, amp = scatterer
        t = S.table(x0, dx, zs, c1, c2, xe, ze, [xs], [zsc])["t"][:, 0]
        assert np.isfinite(t).all()
        _splat(fmc, tx, rx, t[tx] + t[rx], amp, fs, t0, f0, cycles)
    fmc[rx, tx] = fmc[tx, rx]
    return fmc.astype(np.float32)
