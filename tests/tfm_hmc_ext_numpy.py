"""NumPy definitions of phase-coherence and weighted TFM over a half-matrix capture (include/rtus.h: rtus_tfm_phase_hmc,
rtus_tfm_weighted_hmc).  NumPy only; the delay-and-sum rules are tests/das_exact_numpy.py's, the phasor and the factors
tests/tfm_phase_numpy.py's.

The packed triangle is walked record by record.  Record (i, j), i <= j, is sampled at s_ij (tt_tx[i], tt_rx[j]) -> p1 and, off the
diagonal, at s_ji (tt_tx[j], tt_rx[i]) -> p2 (with one table p2 == p1 bit for bit).  THE PAIR FIRST: what a record adds to a sum is
formed from its two samples before it meets the running sum.
    S   += p1 + p2                                  B += sign(Re p1) + sign(Re p2)          N = T R
    U   += u(p1) + u(p2)                            u = p / |p|, 0 for p = 0
    S_w += W_ij p1 + W_ji p2,  W_ij = w_tx[i] w_rx[j]   (two delay tables)
    S_w += (W_ij + W_ji) p1                             (one delay table: the weights' sum first; the diagonal W_ii p1)
    P    = (sum over tx legs with a path of |w_tx|^2) (sum over rx legs with a path of |w_rx|^2)
A leg has a path iff its time has one and (weighted sums only) its weight is finite; a leg without one has weight 0.
The header's fp32 statements for the weights (a = (ar, ai), b = (br, bi); r() = one rounding to float32):
    a b:  re = r(r(ar br) - ai bi)        im = r(r(ar bi) + r(ai br))         (symmetric in a, b)
    W p:  re = r(r(Wr pr) - Wi pi)        im = r(Wr pi + r(Wi pr))
    chain of P:  sum = r(wi wi + r(wr wr + sum)), elements ascending;  P = r(ptx prx), the product in fp64
With ``exact=True`` (inputs under das_exact_numpy's GENERATOR RULES) r() ASSERTS that nothing rounds (_exact32) — every product,
W_ij + W_ji, every term and every partial sum in the kernel's order — so the sums can be compared with no tolerance, in any order.
With ``exact=False`` the samples p are the kernel's float32 numbers (fp32 legs and positions, the fused lerp as one fp64 expression
rounded to float32) and everything after them is plain fp64: the definition that random data is held to within a bound.

The kernel's order of the records (rtus_tfm_hmc's): blocks of 16 columns ascending; in the block [c0, c0 + 16) first the rows above
it (i < c0 ascending, j ascending through the block), then the block's triangle (i ascending, j ascending from i).  U32 is the
float32 sum of the float32 phasors in that order, the pair first — the one-table kernel's fmaf(2, u, U) is U + (u + u) in one
rounding, the same number.

VCF_BAR: 4 x the largest |vcf32 - vcf| of that float32 sum against the fp64 sum over the exact cases of every size in HMC_SIZES with
n_e^2 <= 4900, one and two tables, measured by tests/test_tfm_hmc_ext_cpu.py (which holds this constant to its measurement): the
margin tests/test_gpu_tfm_phase.py gives VCF_BAR for the hardware's reciprocal square root.
"""
import numpy as np

import das_exact_numpy as D
import tfm_phase_numpy as TP

f32, f64 = np.float32, np.float64
GROUP = 16
VCF_BAR = 5.2e-7                     # 4 x 1.294e-7 (n_e = 64, one table and two); the hard cap is (4900 + 8) 2^-23 = 5.85e-4
VCF_CAP = (4900 + 8) * 2.0 ** -23
VCF_SIZES = tuple(n for n in D.HMC_SIZES if n * n <= 4900)


def order(n_e):
    """the packed indices of the records in the kernel's order of summation -> int array [n_pairs]"""
    out = []
    for c0 in range(0, n_e, GROUP):
        c1 = min(c0 + GROUP, n_e)
        for i in range(c0):
            out.extend(D.packed_index(i, j, n_e) for j in range(c0, c1))
        for i in range(c0, c1):
            out.extend(D.packed_index(i, j, n_e) for j in range(i, c1))
    out = np.asarray(out, dtype=np.int64)
    assert np.array_equal(np.sort(out), np.arange(n_e * (n_e + 1) // 2))
    return out


def _rounder(exact):
    if exact:
        return D._exact32

    def to32(x, what):
        with np.errstate(all="ignore"):
            return np.asarray(x, dtype=f64).astype(f32).astype(f64)
    return to32


def _lerp(pad, s, ok, r):
    """one plane of the records pad [m, n_t + 1] at the fp32 positions s [m, n_f] -> fp64 holding float32 numbers"""
    n_t = pad.shape[1] - 1
    fl = np.floor(s)
    w = (s - fl).astype(f32)
    inrec = ok & (fl >= 0) & (fl < n_t)
    i = np.where(inrec, fl, 0).astype(np.int64)
    w = np.where(inrec, w, 0).astype(f64)
    k = np.arange(pad.shape[0])[:, None]
    v0, v1 = pad[k, i], pad[k, i + 1]
    d = r(v1 - v0, "x[i + 1] - x[i]")
    return np.where(inrec, r(w * d + v0, "fmaf(w, d, x[i])"), 0.0)


def samples(h, fs, t0, tt_tx, tt_rx=None, exact=True):
    """-> dict(p1, p2 complex128 [n_pairs, n_f] (float32 numbers; p2 = 0 on the diagonal), i, j [n_pairs], tau / ok of both tables)"""
    pre, pim = D._planes(h)
    n_pairs = pre.shape[0]
    n_e = (int(np.sqrt(8 * n_pairs + 1)) - 1) // 2
    assert n_e * (n_e + 1) // 2 == n_pairs
    tau_tx, ok_tx, _ = D.legs(tt_tx, fs, t0)
    tau_rx, ok_rx, _ = (tau_tx, ok_tx, None) if tt_rx is None else D.legs(tt_rx, fs, t0)
    assert tau_tx.shape[0] == n_e and tau_rx.shape[0] == n_e
    i, j = np.triu_indices(n_e)
    assert np.array_equal(D.packed_index(i, j, n_e), np.arange(n_pairs))
    r = _rounder(exact)
    s1, k1 = D.position(tau_tx[i], ok_tx[i], tau_rx[j], ok_rx[j])
    s2, k2 = D.position(tau_tx[j], ok_tx[j], tau_rx[i], ok_rx[i])
    k2 = k2 & (i != j)[:, None]                                          # the diagonal has p1 only
    p1 = _lerp(pre, s1, k1, r) + 1j * _lerp(pim, s1, k1, r)
    p2 = _lerp(pre, s2, k2, r) + 1j * _lerp(pim, s2, k2, r)
    return dict(p1=p1, p2=p2, i=i, j=j, n_e=n_e, ok_tx=ok_tx, ok_rx=ok_rx)


def _cmul(a, b, r):
    """the header's a b -> (re, im)"""
    re = r(r(a.real * b.real, "ar br") - a.imag * b.imag, "re(a b)")
    im = r(r(a.real * b.imag, "ar bi") + r(a.imag * b.real, "ai br"), "im(a b)")
    return re, im


def _times(wr, wi, p, r):
    """the header's W p -> (re, im)"""
    re = r(r(wr * p.real, "Wr pr") - wi * p.imag, "re(W p)")
    im = r(wr * p.imag + r(wi * p.real, "Wi pr"), "im(W p)")
    return re, im


def _power(g, ok, r):
    """the chain fmaf(wi, wi, fmaf(wr, wr, sum)) over the elements ascending, legs without a path left out -> [n_f]"""
    s = np.zeros(g.shape[1])
    for e in range(g.shape[0]):
        nxt = r(g[e].imag * g[e].imag + r(g[e].real * g[e].real + s, "wr wr + sum"), "wi wi + ...")
        s = np.where(ok[e], nxt, s)
    return s


def bits(x):
    """the mantissa bits that each value of x (multiples of 1/16) needs"""
    n = np.abs(np.rint(x * 16.0)).astype(np.int64)
    assert np.array_equal(n, np.abs(x * 16.0)), "not a multiple of 1/16"
    low = n & -n
    return np.where(n > 0, np.floor(np.log2(np.maximum(n // np.maximum(low, 1), 1))) + 1, 0).astype(np.int64)


def walk(h, fs, t0, tt_tx, tt_rx=None, w_tx=None, w_rx=None, exact=True):
    """The packed walk with the pair-first rule.
    -> dict(S complex128, B, N, T, R int64, U complex128 (fp64 sum), U32 complex128 (the float32 sum in the kernel's order), vcf,
    vcf32 float64, scf float32 (scf_header) [n_f]; with weights also S_w (the two-delay-table rule), S_w1 (the one-delay-table rule;
    None with two delay tables), P and Aw = sum of |W_ij| |p1| + |W_ji| |p2| (the scale of S_w's rounding error); with ``exact``
    also widest: the mantissa bits of the widest partial sum of S, S_w and S_w1 in the kernel's order)"""
    q = samples(h, fs, t0, tt_tx, tt_rx, exact)
    r = _rounder(exact)
    p1, p2, i, j, n_e, ok_tx, ok_rx = (q[k] for k in ("p1", "p2", "i", "j", "n_e", "ok_tx", "ok_rx"))
    perm = order(n_e)
    widest = 0

    def total(t, what):
        """the sum of the records' terms; exact: every partial sum in the kernel's order is a float32 number"""
        nonlocal widest
        if not exact:
            return t.sum(axis=0)
        c = D._exact32(np.cumsum(t[perm], axis=0), f"a partial sum of {what}")
        widest = max(widest, int(bits(c).max()))
        return c[-1]

    t_re, t_im = r(p1.real + p2.real, "the pair's sum"), r(p1.imag + p2.imag, "the pair's sum")
    S = total(t_re, "S") + 1j * total(t_im, "S")
    T, R = ok_tx.sum(axis=0).astype(np.int64), ok_rx.sum(axis=0).astype(np.int64)
    N = T * R
    B = (np.sign(p1.real) + np.sign(p2.real)).astype(np.int64).sum(axis=0)
    u1, u2 = TP.unit(p1), TP.unit(p2)
    U = (u1 + u2).sum(axis=0)
    pair_re = (u1.real.astype(f32) + u2.real.astype(f32))[perm]          # float32 + float32: the pair first
    pair_im = (u1.imag.astype(f32) + u2.imag.astype(f32))[perm]
    assert pair_re.dtype == f32
    U32 = np.cumsum(pair_re, axis=0, dtype=f32)[-1].astype(f64) + 1j * np.cumsum(pair_im, axis=0, dtype=f32)[-1].astype(f64)
    out = dict(S=S, B=B, N=N, T=T, R=R, U=U, U32=U32, vcf=TP.vcf_of(U, N), vcf32=TP.vcf_of(U32, N), scf=D.scf_header(B, N))
    if w_tx is not None:
        if not exact:
            r = lambda x, what: x                                        # after the samples: plain fp64
        w_tx = np.asarray(w_tx).astype(np.complex128)
        w_rx = w_tx if w_rx is None else np.asarray(w_rx).astype(np.complex128)
        okw_tx, okw_rx = ok_tx & D._finite_c(w_tx), ok_rx & D._finite_c(w_rx)
        g_tx, g_rx = np.where(okw_tx, w_tx, 0.0), np.where(okw_rx, w_rx, 0.0)
        diag = (i == j)[:, None]
        a_re, a_im = _cmul(g_tx[i], g_rx[j], r)                          # W_ij
        b_re, b_im = _cmul(g_tx[j], g_rx[i], r)                          # W_ji
        c1, c2 = _times(a_re, a_im, p1, r), _times(b_re, b_im, p2, r)
        two_re = r(c1[0] + np.where(diag, 0.0, c2[0]), "the pair's weighted sum")
        two_im = r(c1[1] + np.where(diag, 0.0, c2[1]), "the pair's weighted sum")
        out["S_w"] = total(two_re, "S_w") + 1j * total(two_im, "S_w")
        out["Aw"] = (np.hypot(a_re, a_im) * np.abs(p1) + np.hypot(b_re, b_im) * np.abs(p2)).sum(axis=0)
        out["S_w1"] = None
        if tt_rx is None:                                                # one gather: (W_ij + W_ji) p1
            w_re = r(a_re + np.where(diag, 0.0, b_re), "W_ij + W_ji")
            w_im = r(a_im + np.where(diag, 0.0, b_im), "W_ij + W_ji")
            one = _times(w_re, w_im, p1, r)
            out["S_w1"] = total(one[0], "S_w (one delay table)") + 1j * total(one[1], "S_w (one delay table)")
        ptx, prx = _power(g_tx, okw_tx, r), _power(g_rx, okw_rx, r)
        out["P"] = r(ptx * prx, "P")
    if exact:
        out["widest"] = widest
    return out


_cache = {}


def exact_case(n_e, two, two_w):
    """D.hmc_case(n_e, two) with D.weights: one weight table (w_rx None) or two -> dict(h, fs, t0, tt_tx, tt_rx, w_tx, w_rx, cols)"""
    key = ("case", n_e, two, two_w)
    if key not in _cache:
        c = dict(D.hmc_case(n_e, two))
        rng = np.random.default_rng(5000 + n_e + 100 * two_w)
        c["w_tx"] = D.weights(rng, n_e, D.N_F)
        c["w_rx"] = D.weights(rng, n_e, D.N_F) if two_w else None
        _cache[key] = D._frozen(c)
    return _cache[key]


def exact_model(n_e, two, two_w):
    key = ("model", n_e, two, two_w)
    if key not in _cache:
        c = exact_case(n_e, two, two_w)
        m = walk(c["h"], c["fs"], c["t0"], c["tt_tx"], c["tt_rx"], c["w_tx"], c["w_rx"], exact=True)
        _cache[key] = D._frozen({k: v for k, v in m.items() if v is not None})
    return _cache[key]
