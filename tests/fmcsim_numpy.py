"""NumPy oracle of the FMC simulator (include/rtus.h: rtus_fmc_sim, rtus_fmc_sim_echo): the same formulas and the same pinned
position arithmetic as the kernel, with fp64 sums.

An arrival (tau, a) adds a p(t_j - tau) to the samples t_j = t0 + j / fs.  The wavelet p is the table ``pulse`` sampled at
fs * oversample with time zero at index ``centre``, continued with p[-1] = p[n_p] = 0, zero beyond, linear in between.
    d  = ((tau - t0) * fs) * oversample      x0 = centre - d      i0 = floor(x0)      w = float32(x0 - i0)
sample j reads the table at i = i0 + j * oversample with the weight w.  What differs from the kernel: the amplitude products,
the interpolation and the sums are fp64 here (the kernel's are fp32), so the two agree to the fp32 summation bound and not by bits.

scan() is the fast oracle and shares the kernel's index arithmetic (first and last sample of an arrival, a padded table);
scan_by_definition() is the header's sentence per sample and shares none of it: tests/test_fmcsim_cpu.py holds the two together.
"""
import math

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


def scan_by_definition(tau, a, pulse, centre, oversample, fs, t0, n_t, edges=None):
    """scan() from the text of include/rtus.h, sample by sample: for every arrival d = ((tau - t0) fs) oversample, x0 = centre - d,
    i0 = floor(x0), w = (float)(x0 - i0); sample j reads the table at i = i0 + j oversample and is touched iff -1 <= i <= n_p - 1;
    it receives a (P(i) + w (P(i + 1) - P(i))) with P zero outside [0, n_p).  Plain loops over the arrivals and over every sample of
    the record, Python floats (fp64, each operation rounded on its own).  -> what scan() returns.
    ``edges``: a list that receives, per arrival that counts, (k, first sample, last sample, |its own term at the first|, |at the
    last|)."""
    table = [complex(v) for v in np.asarray(pulse, dtype=np.complex64).ravel()]
    n_p, os_ = len(table), int(oversample)

    def P(i):
        return table[i] if 0 <= i < n_p else 0j

    tau = [float(t) for t in np.atleast_1d(np.asarray(tau, dtype=np.float64))]
    with np.errstate(over="ignore", invalid="ignore"):
        amp = [1 + 0j] * len(tau) if a is None else [complex(v) for v in np.atleast_1d(np.asarray(a)).astype(np.complex64)]
    out, touched, sum_abs = [0j] * n_t, [False] * n_t, 0.0
    for k, (t, ak) in enumerate(zip(tau, amp)):
        if not (math.isfinite(ak.real) and math.isfinite(ak.imag)):
            continue
        d = ((t - float(t0)) * float(fs)) * float(os_)
        if not abs(d) < 2.0 ** 30:                                              # NaN fails
            continue
        x0 = float(centre) - d
        i0 = math.floor(x0)
        w = float(np.float32(x0 - i0))
        first = last = None
        for j in range(n_t):
            i = i0 + j * os_
            if -1 <= i <= n_p - 1:
                term = ak * (P(i) + w * (P(i + 1) - P(i)))
                out[j] += term
                touched[j] = True
                if first is None:
                    first = (j, abs(term))
                last = (j, abs(term))
        if first is not None:
            sum_abs += abs(ak)
            if edges is not None:
                edges.append((k, first[0], last[0], first[1], last[1]))
    return np.array(out, dtype=np.complex128), np.array(touched, dtype=bool), sum_abs


# ------------------------------------------------------------------------------- inputs that are not small anywhere
def random_complex(rng, shape):
    """complex64 m exp(2 pi i phi), m uniform in [0.5, 1.5], phi uniform in [0, 1): as a wavelet no entry is small next to the
    peak, so a table entry or a sample off by one shows at full size"""
    m, phi = rng.uniform(0.5, 1.5, shape), rng.uniform(0.0, 1.0, shape)
    return (m * np.exp(2j * np.pi * phi)).astype(np.complex64)


def times_at(k, rng, fs, oversample, t0):
    """arrival times t0 + (k + f) / (fs oversample), k integers (any shape), f uniform in [0.1, 0.9]: sample 0 reads the table at
    i0 = centre - k - 1 with the weight 1 - f, away from 0 and 1, and no placement sits within a rounding of a table node"""
    k = np.asarray(k, dtype=np.int64)
    return float(t0) + (k + rng.uniform(0.1, 0.9, k.shape)) / (float(fs) * int(oversample))


def edge_steps(n_p, centre, oversample, n_t):
    """the table steps k (times_at) of seven arrivals around the two ends of a record, each the start of a run: an arrival at
    k + m, m = 0, 1, 2, ..., moves through the table one entry at a time.  With J = n_t - 1, an arrival at k is touched in samples
    j with k - centre <= j oversample <= k - centre + n_p.
        0, 1  sample 0 cuts the pulse: it reads i0 = oversample .. -1 (run of 6 each, 12 together: every phase of the first
              oversample + 1 entries, then pulses that start inside)
        2, 3  sample J cuts the pulse: it reads i = n_p .. n_p - 11 (n_p: sample J is just missed)
        4     wholly inside, about the middle of the record
        5     before the record: k = centre - n_p - 1 is the last that writes nothing, centre - n_p reads p[n_p - 1] at sample 0
        6     after the record: k = centre + J oversample reads p[-1] at sample J, one more writes nothing"""
    J = n_t - 1
    return np.array([centre - oversample - 1, centre - oversample + 5,
                     centre - n_p + J * oversample - 1, centre - n_p + J * oversample + 5,
                     centre + oversample * (n_t // 2) - n_p // 2,
                     centre - n_p - 3,
                     centre + J * oversample - 3], dtype=np.int64)


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
