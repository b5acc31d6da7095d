"""NumPy oracle of the envelope TFM with carrier-aware (IQ) interpolation (include/rtus.h: rtus_tfm_iq, rtus_tfm_iq_hmc).  NumPy
only; the step in fp64.

The step, per pair, with a0, a1 the two neighbouring samples and w the fraction of the position (the header's):
    q = a1 R,  R = (cos 2 pi nu, -sin 2 pi nu) rounded to fp32,  nu = f_demod / fs
    b = a0 + w (q - a0)
    p = b exp(2 pi i nu w)
    S += p;  E += |p|^2;  A += |p|;  N = T R;  cf = |S|^2 / (N E)
The sample POSITIONS are formed the way the kernels form them — each leg's half position t fs - t0 fs / 2 in fp64, rounded once to
fp32; the no-path clamp; the fp32 sum of the two halves; floor, then w = s - floor (exact) — so that a comparison with the kernels
measures the arithmetic of the step and not the rounding of the positions (1e-4 of a sample, which a carrier turns into phase).
Edge rules: rtus_tfm_analytic's (sample n_t reads as zero, a negative position contributes nothing, positions outside the record
count in N with value zero).  A packed (half-matrix) block goes through hmc_unpack's index rule: record (i, j), i <= j, serves
(i, j) and (j, i); the sum over the full symmetric matrix is the header's triangular sum in exact arithmetic, term by term.

``emulate=True`` runs the step and the sums in fp32 (each product and sum rounded as the header writes them, the phasor the
correctly rounded sine and cosine of the fp32 product nu w, plain recursive sums tx-major): what the kernels may differ by.
"""
import numpy as np

from tfm_analytic_numpy import coherence

NO_PATH = np.float32(-1.0e8)


def half_positions(tt, fs, t0):
    """a table's legs as the kernels hold them -> float32 [n_e, n_f]: (t fs - t0 fs / 2) rounded once; NO_PATH where that is not
    finite or not below 1e8 in magnitude"""
    with np.errstate(all="ignore"):
        v = (np.asarray(tt, dtype=np.float64) * float(fs) - 0.5 * float(t0) * float(fs)).astype(np.float32)
        return np.where(np.abs(v) < -NO_PATH, v, NO_PATH).astype(np.float32)


def unpack(h):
    """[n_pairs, n_t] -> the symmetric [n_e, n_e, n_t] (hmc_unpack's rule: numpy.triu_indices' order)"""
    n_pairs = h.shape[0]
    n_e = (int(np.sqrt(8 * n_pairs + 1)) - 1) // 2
    assert n_e * (n_e + 1) // 2 == n_pairs, f"{n_pairs} is not a triangular number"
    i, j = np.triu_indices(n_e)
    full = np.empty((n_e, n_e, h.shape[1]), dtype=h.dtype)
    full[i, j] = h
    full[j, i] = h
    return full


def rotation(f_demod, fs, exact=False):
    """-> (cos 2 pi nu, sin 2 pi nu) rounded to fp32 as the header has them (``exact``: not rounded — the algebra of the step
    alone), as float64, and nu"""
    nu = float(f_demod) / float(fs)
    cs, sn = np.cos(2.0 * np.pi * nu), np.sin(2.0 * np.pi * nu)
    return (float(cs), float(sn), nu) if exact else (float(np.float32(cs)), float(np.float32(sn)), nu)


def step(a0, a1, w, f_demod, fs, emulate=False, exact_r=False):
    """the carrier-aware step on complex arrays a0, a1 and fractions w -> p (complex128)"""
    cs, sn, nu = rotation(f_demod, fs, exact_r and not emulate)
    if not emulate:
        q = a1 * (cs - 1j * sn)
        b = a0 + w * (q - a0)
        return b * np.exp(2j * np.pi * nu * w)
    f = np.float32
    fma = lambda x, y, z: (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(f)
    r0, i0, r1, i1 = (np.asarray(x, dtype=f) for x in (a0.real, a0.imag, a1.real, a1.imag))
    w = np.asarray(w, dtype=f)
    cs, sn = f(cs) * np.ones_like(w), f(sn) * np.ones_like(w)
    qr, qi = fma(i1, sn, r1 * cs), fma(-r1, sn, i1 * cs)
    br, bi = fma(w, qr - r0, r0), fma(w, qi - i0, i0)
    x = (f(nu) * w).astype(np.float64)
    c, s = np.cos(2.0 * np.pi * x).astype(f), np.sin(2.0 * np.pi * x).astype(f)
    return fma(-bi, s, br * c).astype(np.float64) + 1j * fma(br, s, bi * c).astype(np.float64)


def tfm_iq(a, fs, t0, f_demod, tt_tx, tt_rx=None, emulate=False):
    """-> dict(image complex128 [n_f], N, E, cf, A [n_f]) for a complex FMC a [n_tx, n_rx, n_t], or a packed half-matrix block
    [n_pairs, n_t] (2-D: unpacked first; then both tables have n_e rows)"""
    a = np.asarray(a)
    assert np.iscomplexobj(a)
    if a.ndim == 2:
        a = unpack(a)
    a = a.astype(np.complex128)
    n_tx, n_rx, n_t = a.shape
    h_tx = half_positions(tt_tx, fs, t0)
    h_rx = h_tx if tt_rx is None else half_positions(tt_rx, fs, t0)
    assert h_tx.shape[0] == n_tx and h_rx.shape[0] == n_rx
    n_f = h_tx.shape[1]
    pad = np.concatenate([a, np.zeros((n_tx, n_rx, 1))], axis=2)          # sample n_t = 0
    rows = np.arange(n_rx)[:, None]
    S = np.zeros(n_f, dtype=np.complex128)
    E, A = np.zeros(n_f), np.zeros(n_f)
    S32 = np.zeros((2, n_f), dtype=np.float32)
    for tx in range(n_tx):
        s = h_tx[tx][None, :] + h_rx                                       # fp32 sum, [n_rx, n_f]
        fl = np.floor(s)
        w = (s - fl).astype(np.float64)                                    # exact in fp32
        ok = (fl >= 0) & (fl < n_t)
        i = np.where(ok, fl, 0).astype(np.int64)
        p = np.where(ok, step(pad[tx][rows, i], pad[tx][rows, i + 1], w, f_demod, fs, emulate), 0.0)
        if emulate:
            for k in range(n_rx):
                S32[0] += p[k].real.astype(np.float32)
                S32[1] += p[k].imag.astype(np.float32)
        S += p.sum(axis=0)
        E += (p.real ** 2 + p.imag ** 2).sum(axis=0)
        A += np.abs(p).sum(axis=0)
    if emulate:
        S = S32[0].astype(np.float64) + 1j * S32[1].astype(np.float64)
    N = (h_tx > NO_PATH).sum(axis=0).astype(np.float64) * (h_rx > NO_PATH).sum(axis=0)
    return dict(image=S, N=N, E=E, cf=coherence(S, N, E), A=A)
