"""NumPy oracle of TFM and envelope TFM over a half-matrix capture (include/rtus.h: rtus_tfm_hmc, rtus_tfm_analytic_hmc).  NumPy
only, fp64 throughout.

The packed block h [n_pairs, n_t] holds the record of (i, j), i <= j, at p = i n_e - i (i - 1) / 2 + (j - i).  The sum is written
as the definition's TRIANGULAR double sum — i ascending, j ascending from i, each record once — not as tfm_analytic on the unpacked
matrix: S = sum of c_ij, c_ii = a_ii(s_ii), c_ij = a_ij(s_ij) + a_ij(s_ji), s_ij from tt_tx[i] and tt_rx[j], s_ji from tt_tx[j] and
tt_rx[i]; path and edge rules are tests/tfm_analytic_numpy.py's.  E sums |.|^2 of the same terms, A their moduli; N = T R.
"""
import numpy as np

from tfm_analytic_numpy import coherence, leg_has_path


def n_elements(n_pairs):
    n_e = (int(np.sqrt(8 * n_pairs + 1)) - 1) // 2
    assert n_e * (n_e + 1) // 2 == n_pairs, f"{n_pairs} is not a triangular number"
    return n_e


def packed_index(i, j, n_e):
    """p(i, j) of the header, i <= j"""
    return i * n_e - i * (i - 1) // 2 + (j - i)


def _interp(pad, rows, s, ok, n_t):
    """the records pad[rows] ([m, n_t + 1], sample n_t = 0) at the positions s [m, n_f] where ok -> complex [m, n_f]"""
    with np.errstate(all="ignore"):
        ok = ok & np.isfinite(s) & (s >= 0) & (s < n_t)
    i = np.where(ok, np.floor(np.where(ok, s, 0.0)), 0).astype(np.int64)
    w = np.where(ok, s - i, 0.0)
    k = np.arange(rows.size)[:, None]
    v0, v1 = pad[rows][k, i], pad[rows][k, i + 1]
    return np.where(ok, (v0.real + w * (v1.real - v0.real)) + 1j * (v0.imag + w * (v1.imag - v0.imag)), 0.0)


def tfm_hmc(h, fs, t0, tt_tx, tt_rx=None):
    """-> dict(image complex128 [n_f] (real input: its imaginary part is 0), N, E, cf, A [n_f]) for a packed block h [n_pairs, n_t],
    real or complex (or float32 [n_pairs, n_t, 2])"""
    h = np.asarray(h)
    if h.dtype == np.float32 and h.ndim == 3 and h.shape[2] == 2:
        h = h[..., 0] + 1j * h[..., 1].astype(np.float64)
    h = h.astype(np.complex128)
    n_pairs, n_t = h.shape
    n_e = n_elements(n_pairs)
    tt_tx = np.asarray(tt_tx, dtype=np.float64)
    tt_rx = tt_tx if tt_rx is None else np.asarray(tt_rx, dtype=np.float64)
    n_f = tt_tx.shape[1]
    ok_tx, ok_rx = leg_has_path(tt_tx, fs, t0), leg_has_path(tt_rx, fs, t0)
    pad = np.concatenate([h, np.zeros((n_pairs, 1))], axis=1)              # sample n_t = 0
    S = np.zeros(n_f, dtype=np.complex128)
    E, A = np.zeros(n_f), np.zeros(n_f)
    for i in range(n_e):
        j = np.arange(i, n_e)
        rows = packed_index(i, j, n_e)                                     # contiguous: p(i, i) .. p(i, n_e - 1)
        with np.errstate(all="ignore"):
            s_ij = (tt_tx[i][None, :] + tt_rx[j] - t0) * fs               # [n_e - i, n_f]
            s_ji = (tt_tx[j] + tt_rx[i][None, :] - t0) * fs
        a_ij = _interp(pad, rows, s_ij, ok_tx[i][None, :] & ok_rx[j], n_t)
        a_ji = _interp(pad, rows, s_ji, ok_tx[j] & ok_rx[i][None, :], n_t)
        a_ji[0] = 0.0                                                      # the diagonal counts once
        S += (a_ij + a_ji).sum(axis=0)
        E += (np.abs(a_ij) ** 2 + np.abs(a_ji) ** 2).sum(axis=0)
        A += (np.abs(a_ij) + np.abs(a_ji)).sum(axis=0)
    N = ok_tx.sum(axis=0).astype(np.float64) * ok_rx.sum(axis=0)
    return dict(image=S, N=N, E=E, cf=coherence(S, N, E), A=A)
