"""NumPy oracle of the envelope TFM with coherence factor (include/rtus.h: rtus_tfm_analytic).  NumPy only, fp64 throughout.

Definitions (the header's): S[f] = sum over (tx, rx) of the analytic FMC a[tx, rx] interpolated linearly at the sample position
(tt_tx[tx, f] + tt_rx[rx, f] - t0) fs, real and imaginary parts separately, with oracle/tfm_numpy.py's edge rules; a leg has a path
when float32(t fs - t0 fs / 2) is finite with |.| < 1e8; N[f] = T[f] R[f] (tx and rx with a path); E[f] = the sum of |a(s)|^2 over the pairs;
cf = |S|^2 / (N E) clamped to 1, NaN when N = 0, 0 when E = 0 < N.  Pairs whose position falls outside the record count in N with
value zero.
"""
import numpy as np


def leg_has_path(tt, fs, t0):
    """[n_e, n_f] bool: the leg's half sample position, ROUNDED TO FLOAT32 as the header has it, is finite and below 1e8 in
    magnitude.  The rounding decides for the fp64 values in (99999996, 1e8): they round onto the float32 1e8 and have no path
    (tests/das_exact_numpy.py puts legs there)."""
    with np.errstate(all="ignore"):
        v = (np.asarray(tt, dtype=np.float64) * fs - 0.5 * t0 * fs).astype(np.float32)
        return np.isfinite(v) & (np.abs(v) < np.float32(1e8))


def coherence(S, N, E):
    """cf = |S|^2 / (N E), clamped to 1; NaN when N = 0, 0 when E = 0 < N"""
    S, N, E = np.asarray(S), np.asarray(N, dtype=np.float64), np.asarray(E, dtype=np.float64)
    with np.errstate(all="ignore"):
        c = np.minimum(np.abs(S) ** 2 / (N * E), 1.0)
    return np.where(N == 0, np.nan, np.where(E == 0, 0.0, c))


def tfm_analytic(a, fs, t0, tt_tx, tt_rx=None):
    """-> dict(image complex128 [n_f], N [n_f], E [n_f], cf [n_f]) for a complex FMC a [n_tx, n_rx, n_t]"""
    a = np.asarray(a)
    if a.dtype == np.float32 and a.ndim == 4 and a.shape[3] == 2:
        a = a[..., 0] + 1j * a[..., 1].astype(np.float64)
    a = a.astype(np.complex128)
    n_tx, n_rx, n_t = a.shape
    tt_tx = np.asarray(tt_tx, dtype=np.float64)
    tt_rx = tt_tx if tt_rx is None else np.asarray(tt_rx, dtype=np.float64)
    n_f = tt_tx.shape[1]
    ok_tx, ok_rx = leg_has_path(tt_tx, fs, t0), leg_has_path(tt_rx, fs, t0)
    pad = np.concatenate([a, np.zeros((n_tx, n_rx, 1))], axis=2)          # sample n_t = 0
    rows = np.arange(n_rx)[:, None]
    S = np.zeros(n_f, dtype=np.complex128)
    E = np.zeros(n_f)
    for tx in range(n_tx):
        with np.errstate(all="ignore"):
            s = (tt_tx[tx][None, :] + tt_rx - t0) * fs                   # [n_rx, n_f]
            ok = ok_tx[tx][None, :] & ok_rx & np.isfinite(s) & (s >= 0) & (s < n_t)
        i = np.where(ok, np.floor(np.where(ok, s, 0.0)), 0).astype(np.int64)
        w = np.where(ok, s - i, 0.0)
        v0, v1 = pad[tx][rows, i], pad[tx][rows, i + 1]
        v = np.where(ok, (v0.real + w * (v1.real - v0.real)) + 1j * (v0.imag + w * (v1.imag - v0.imag)), 0.0)
        S += v.sum(axis=0)
        E += (v.real ** 2 + v.imag ** 2).sum(axis=0)
    N = ok_tx.sum(axis=0).astype(np.float64) * ok_rx.sum(axis=0)
    return dict(image=S, N=N, E=E, cf=coherence(S, N, E))
