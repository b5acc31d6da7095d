"""NumPy oracle of the FMC simulator (include/rtus.h: rtus_fmc_sim, rtus_fmc_sim_echo): the same formulas and the same pinned
position arithmetic as the kernel, with fp64 sums.

An arrival (tau, a) adds a p(t_j - tau) to the samples t_j = t0 + j / fs.  The wavelet p is the table ``pulse`` sampled at
fs * oversample with time zero at index ``centre``, continued with p[-1] = p[n_p] = 0, zero beyond, linear in between.
    d  = ((tau - t0) * fs) * oversample      x0 = centre - d      i0 = floor(x0)      w = float32(x0 - i0)
sample j reads the table at i = i0 + j * oversample with the weight w.  What differs from the kernel: the amplitude products,
the interpolation and the sums are fp64 here (the kernel's are fp32), so the two agree to the fp32 summation bound and not by bits.
"""
import numpy as np


def place(tau, t0, fs, oversample, centre):
    """-> (ok bool, ip0 int64, w float64 holding float32 values): ip0 = i0 + 1, the index of sample 0 into the padded table"""
    tau = np.asarray(tau, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = ((tau - np.float64(t0)) * np.float64(fs)) * np.float64(oversample)
        ok = np.abs(d) < 1073741824.0                                           # NaN fails
        x0 = np.float64(centre) - np.where(ok, d, 0.0)
    fl = np.floor(x0)
    w = (x0 - fl).astype(np.float32).astype(np.float64)
    return ok, fl.astype(np.int64) + 1, w


def amplitude(*factors):
    """the product of the complex64 factors (None: 1), left to right in fp64, and whether every factor and every partial product,
    rounded to fp32, is finite (the kernel multiplies in fp32: a product that overflows there drops the arrival)"""
    a, ok = None, None
    for f in factors:
        if f is None:
            continue
        f = np.asarray(f, dtype=np.complex64)
        fin = np.isfinite(f.real) & np.isfinite(f.imag)
        f = np.where(fin, f, 0).astype(np.complex128)
        a, ok = (f, fin) if a is None else (a * f, ok & fin)
        with np.errstate(over="ignore"):
            p32 = a.astype(np.complex64)
        ok = ok & np.isfinite(p32.real) & np.isfinite(p32.imag)
    return a, ok


def scan(tau, a, pulse, centre, oversample, fs, t0, n_t, init=None):
    """one A-scan from its arrivals tau [n] (fp64), a [n] complex (None: 1) -> (complex128 [n_t], touched bool [n_t], sum |a| over
    the arrivals that count).  ``init``: what the record holds before (accumulate)."""
    pulse = np.asarray(pulse, dtype=np.complex64).astype(np.complex128)
    n_p, os_ = pulse.size, int(oversample)
    pad = np.concatenate([[0.0], pulse, [0.0]])                                 # pad[ip] = p[ip - 1]
    tau = np.atleast_1d(np.asarray(tau, dtype=np.float64))
    ok, ip0, w = place(tau, t0, fs, os_, centre)
    if a is None:
        a = np.ones(tau.size, dtype=np.complex128)
    else:
        a, fin = amplitude(a)
        ok = ok & fin
    j_first = np.where(ip0 >= 0, 0, (-ip0 + os_ - 1) // os_)
    j_last = np.where(ip0 > n_p, -1, np.minimum((n_p - ip0) // os_, n_t - 1))
    ok = ok & (j_first <= j_last)
    out = np.zeros(n_t, dtype=np.complex128) if init is None else np.asarray(init).astype(np.complex128).copy()
    touched = np.zeros(n_t, dtype=bool)
    for m in range(n_p // os_ + 2):
        j = j_first + m
        v = ok & (j <= j_last)
        if not v.any():
            continue
        jv = j[v]
        ip = ip0[v] + jv * os_
        lo, hi = pad[ip], pad[ip + 1]
        np.add.at(out, jv, a[v] * (lo + w[v] * (hi - lo)))
        touched[jv] = True
    return out, touched, float(np.abs(a[ok]).sum())


def simulate(tt_tx, tt_rx, pulse, centre, oversample, fs, t0, n_t, q=None, w_tx=None, w_rx=None, init=None, pairs=None):
    """scatterer form -> (fmc complex128 [n_tx, n_rx, n_t], touched, sum_abs [n_tx, n_rx]); ``pairs``: only these (tx, rx) are
    computed (the others stay zero)"""
    tt_tx, tt_rx = np.asarray(tt_tx, dtype=np.float64), np.asarray(tt_rx, dtype=np.float64)
    n_tx, n_rx = tt_tx.shape[0], tt_rx.shape[0]
    fmc = np.zeros((n_tx, n_rx, n_t), dtype=np.complex128)
    touched = np.zeros((n_tx, n_rx, n_t), dtype=bool)
    sa = np.zeros((n_tx, n_rx))
    todo = pairs if pairs is not None else [(i, j) for i in range(n_tx) for j in range(n_rx)]
    for i, j in todo:
        with np.errstate(invalid="ignore"):
            tau = tt_tx[i] + tt_rx[j]
        a = None
        if q is not None or w_tx is not None or w_rx is not None:
            fs_ = [q, None if w_tx is None else np.asarray(w_tx)[i], None if w_rx is None else np.asarray(w_rx)[j]]
            a = _product(fs_, tau.size)
        fmc[i, j], touched[i, j], sa[i, j] = scan(tau, a, pulse, centre, oversample, fs, t0, n_t, None if init is None else init[i, j])
    return fmc, touched, sa


def _product(factors, n):
    """the factors' product with a NaN wherever one of them (or the fp32 product) is not finite: scan() drops those"""
    a, ok = amplitude(*[None if f is None else np.broadcast_to(np.asarray(f, dtype=np.complex64), (n,)) for f in factors])
    return np.where(ok, a, np.nan + 0j)


def simulate_echo(t_pair, amp, pulse, centre, oversample, fs, t0, n_t, init=None):
    """echo form: t_pair [n_tx, n_rx, n_a], amp the same shape or None"""
    t_pair = np.asarray(t_pair, dtype=np.float64)
    n_tx, n_rx = t_pair.shape[:2]
    fmc = np.zeros((n_tx, n_rx, n_t), dtype=np.complex128)
    touched = np.zeros((n_tx, n_rx, n_t), dtype=bool)
    sa = np.zeros((n_tx, n_rx))
    for i in range(n_tx):
        for j in range(n_rx):
            a = None if amp is None else np.asarray(amp, dtype=np.complex64)[i, j]
            fmc[i, j], touched[i, j], sa[i, j] = scan(t_pair[i, j], a, pulse, centre, oversample, fs, t0, n_t,
                                                      None if init is None else init[i, j])
    return fmc, touched, sa
