"""The delay-and-sum family's arithmetic restated so that it can be compared BIT FOR BIT, and the inputs that make that possible.
NumPy only.

include/rtus.h (rtus_tfm, rtus_tfm_analytic, rtus_tfm_hmc, rtus_tfm_weighted, rtus_tfm_phase, rtus_fmc_synth_tx) fixes every
operation of the family:
    tau = float32(t fs - t0 fs / 2)          each leg, formed in fp64 and rounded once; no path unless tau is finite and |tau| < 1e8
    s   = tau_tx + tau_rx                    in fp32;  i = floor(s), w = s - i
    p   = fmaf(w, x[i + 1] - x[i], x[i])     each part, the difference rounded to fp32; nothing for i < 0 or i >= n_t; x[n_t] = 0
What it leaves open is only the rounding of the running sums, which follows the kernels' order.  So the inputs here are chosen
such that NO operation rounds: then every order gives the same sums, and a plain loop must match the kernels with no tolerance.

The rules that make everything exact (GENERATOR RULES):
  * fs = 2^25; times are multiples of 2^-27 s (positions: multiples of 1/4 sample); t0 is a multiple of 2^-24 s (t0 fs / 2 is an
    integer), so t fs - t0 fs / 2 is exact in fp64 and in fp32;
  * records hold integers in [-4, 4] (real and imaginary parts separately): x[i + 1] - x[i] is an integer in [-8, 8], w (x[i + 1] -
    x[i]) a multiple of 1/4, p a multiple of 1/4 with |p| <= 4, |p|^2 a multiple of 1/16 below 32;
  * weights (rtus_tfm_weighted) are Gaussian integers with parts in [-2, 2];
  * n_tx n_rx <= 2^13: a partial sum of S stays below 2^15 in multiples of 1/4 (17 bits), of E below 2^18 in multiples of 1/16
    (22 bits), of the weighted sum below 2^19 in multiples of 1/4 — all within fp32's 24 bits.  tests/test_das_exact_cpu.py measures
    the widest partial sum of every case and holds it to 24 bits.
The model checks these premises as it runs (_exact32): inputs that break a rule raise instead of comparing rounded numbers.

The hand-made focal-point columns (HAND) put positions ON the decision points that random data only comes near: s = +0 and -0,
s = -2^-23 (floor -1, w = 1 - 2^-23), s = n_t - 1 and s = n_t exactly, an exact sum below n_t whose fp32 sum IS n_t, legs on the
fp32 value 1e8, at the fp64 value 99999997 (which rounds to the fp32 1e8: no path) and at 99999992 (the largest fp32 below 1e8: a
path), their negatives, NaN and infinite legs, and a column without any path.
"""
import numpy as np

FS = 2.0 ** 25
N_T = 24
N_F = 257
LIMIT = np.float32(1.0e8)            # a leg has a path iff |tau| < LIMIT (csrc/rtus_das.h: das_clamp)
BESIDE = 99999992.0                  # the largest fp32 below 1e8
ROUNDS = 99999997.0                  # an fp64 value below 1e8 whose fp32 is 1e8
f32, f64 = np.float32, np.float64


def _exact32(x, what):
    """x (fp64) must be a float32 number: the premise of the whole comparison"""
    x = np.asarray(x, dtype=f64)
    with np.errstate(all="ignore"):
        good = (x.astype(f32).astype(f64) == x) | np.isnan(x)
    assert np.all(good), f"{what}: the inputs break the generator's rules (a value needs more than 24 bits)"
    return x


def legs(tt, fs, t0):
    """-> (tau float32 [n_e, n_f], ok bool [n_e, n_f], v float64: the leg before its rounding to fp32)"""
    tt = np.asarray(tt, dtype=f64)
    with np.errstate(all="ignore"):
        v = tt * f64(fs) - 0.5 * f64(t0) * f64(fs)
        tau = v.astype(f32)
        ok = np.isfinite(tau) & (np.abs(tau) < LIMIT)
    return tau, ok, v


def position(tau_a, ok_a, tau_b, ok_b):
    """the pair's position in fp32 where both legs have a path (elsewhere -1: before the record) -> (s float32, ok)"""
    ok = ok_a & ok_b
    with np.errstate(all="ignore"):
        s = np.where(ok, (tau_a + tau_b).astype(f32), f32(-1.0)).astype(f32)
    return s, ok


def _sample(pad_re, pad_im, s, ok):
    """the records pad_* [m, n_t + 1] (fp64 copies of fp32 data, sample n_t = 0) at the fp32 positions s [m, n_f] -> (re, im) fp64,
    each a float32 number; 0 where the pair has no path or the position is outside the record"""
    n_t = pad_re.shape[1] - 1
    fl = np.floor(s)
    w = (s - fl).astype(f32)                                             # exact in fp32 for every finite s
    inrec = ok & (fl >= 0) & (fl < n_t)
    i = np.where(inrec, fl, 0).astype(np.int64)
    w = np.where(inrec, w, 0).astype(f64)
    k = np.arange(pad_re.shape[0])[:, None]
    out = []
    for pad in (pad_re, pad_im):
        v0, v1 = pad[k, i], pad[k, i + 1]
        d = _exact32(v1 - v0, "x[i + 1] - x[i]")
        p = _exact32(w * d + v0, "fmaf(w, d, x[i])")                     # w d is exact in fp64; the sum must be exact too
        out.append(np.where(inrec, p, 0.0))
    return out[0], out[1]


def _planes(a):
    """complex (or float32 [..., 2], or real) records [..., n_t] -> fp64 planes [..., n_t + 1] with sample n_t = 0"""
    a = np.asarray(a)
    if a.dtype == f32 and a.ndim >= 2 and a.shape[-1] == 2 and not np.iscomplexobj(a):
        a = a[..., 0] + 1j * a[..., 1].astype(f64)
    a = a.astype(np.complex128)
    z = np.zeros(a.shape[:-1] + (1,))
    return np.concatenate([a.real, z], axis=-1), np.concatenate([a.imag, z], axis=-1)


def _finite_c(w):
    return np.isfinite(w.real) & np.isfinite(w.imag)


def cf_header(S, E, N):
    """rtus_tfm_analytic's cf from the fp32 sums: |S|^2 / (N E) in fp64, 0 when E = 0 < N, clamped to 1, NaN when N = 0 -> float32"""
    re, im, en, n = (np.asarray(v, dtype=f64) for v in (S.real, S.imag, E, N))
    with np.errstate(all="ignore"):
        c = np.where(en > 0, (re * re + im * im) / (n * en), 0.0)
        c = np.where(c > 1.0, 1.0, c)
    return np.where(n > 0, c, np.nan).astype(f32)


def scf_header(B, N):
    """rtus_tfm_phase's scf from the integers: 1 - sqrt(1 - (B / N)^2) in fp64, NaN when N = 0 -> float32"""
    b, n = np.asarray(B, dtype=f64), np.asarray(N, dtype=f64)
    with np.errstate(all="ignore"):
        q = b / n
        c = 1.0 - np.sqrt(1.0 - q * q)
    return np.where(n > 0, c, np.nan).astype(f32)


def tfm(a, fs, t0, tt_tx, tt_rx=None, w_tx=None, w_rx=None, terms=False):
    """The full-matrix family on a complex FMC a [n_tx, n_rx, n_t] (a real one: its imaginary plane is zero).
    -> dict(S complex128, E, A float64, T, R, N, B int64, U complex128 [n_f]; with weights also S_w complex128 and P float64);
    with ``terms`` also the per-pair terms, [n_tx n_rx, n_f] each, in (tx, rx) order: t_re, t_im, t_e (and t_wre, t_wim).
    S, E, S_w and P are exact: each is a float32 number and so is every partial sum, in any order."""
    pre, pim = _planes(a)
    n_tx, n_rx = pre.shape[:2]
    tau_tx, ok_tx, _ = legs(tt_tx, fs, t0)
    tau_rx, ok_rx, _ = (tau_tx, ok_tx, None) if tt_rx is None else legs(tt_rx, fs, t0)
    n_f = tau_tx.shape[1]
    assert tau_tx.shape[0] == n_tx and tau_rx.shape[0] == n_rx
    weighted = w_tx is not None
    if weighted:
        w_tx = np.asarray(w_tx).astype(np.complex128)
        w_rx = w_tx if w_rx is None else np.asarray(w_rx).astype(np.complex128)
        okw_tx, okw_rx = ok_tx & _finite_c(w_tx), ok_rx & _finite_c(w_rx)     # a leg with a non-finite weight has no path
        g_tx, g_rx = np.where(okw_tx, w_tx, 0.0), np.where(okw_rx, w_rx, 0.0)
    S_re, S_im, E, A = (np.zeros(n_f) for _ in range(4))
    W_re, W_im = np.zeros(n_f), np.zeros(n_f)
    U = np.zeros(n_f, dtype=np.complex128)
    B = np.zeros(n_f, dtype=np.int64)
    keep = {k: [] for k in ("t_re", "t_im", "t_e", "t_wre", "t_wim")}
    for tx in range(n_tx):                                               # the pairs of one transmit element at a time
        s, ok = position(tau_tx[tx][None, :], ok_tx[tx][None, :], tau_rx, ok_rx)
        re, im = _sample(pre[tx], pim[tx], s, ok)
        e = _exact32(re * re + im * im, "|p|^2")
        m = np.hypot(re, im)
        S_re += re.sum(axis=0); S_im += im.sum(axis=0); E += e.sum(axis=0); A += m.sum(axis=0)
        B += np.sign(re).astype(np.int64).sum(axis=0)
        with np.errstate(all="ignore"):
            U += np.where(m > 0, (re + 1j * im) / m, 0.0).sum(axis=0)
        if weighted:
            sw, okw = position(tau_tx[tx][None, :], okw_tx[tx][None, :], tau_rx, okw_rx)
            wre, wim = _sample(pre[tx], pim[tx], sw, okw)
            g = g_tx[tx][None, :] * g_rx                                 # Gaussian integers: exact
            tw = g * (wre + 1j * wim)
            W_re += _exact32(tw.real, "w_tx w_rx p").sum(axis=0); W_im += _exact32(tw.imag, "w_tx w_rx p").sum(axis=0)
        if terms:
            keep["t_re"].append(re); keep["t_im"].append(im); keep["t_e"].append(e)
            if weighted:
                keep["t_wre"].append(tw.real); keep["t_wim"].append(tw.imag)
    T, R = ok_tx.sum(axis=0).astype(np.int64), ok_rx.sum(axis=0).astype(np.int64)
    r = dict(S=_exact32(S_re, "S") + 1j * _exact32(S_im, "S"), E=_exact32(E, "E"), A=A, T=T, R=R, N=T * R, B=B, U=U)
    if weighted:
        P = (g_tx.real ** 2 + g_tx.imag ** 2).sum(axis=0) * (g_rx.real ** 2 + g_rx.imag ** 2).sum(axis=0)
        r.update(S_w=_exact32(W_re, "S_w") + 1j * _exact32(W_im, "S_w"), P=_exact32(P, "P"))
    if terms:
        r.update({k: np.concatenate(v, axis=0) for k, v in keep.items() if v})
    return r


def packed_index(i, j, n_e):
    """the record of (i, j), i <= j, of a half-matrix capture (numpy.triu_indices' order)"""
    return i * n_e - i * (i - 1) // 2 + (j - i)


def tfm_hmc(h, fs, t0, tt_tx, tt_rx=None, terms=False):
    """The half-matrix family on a packed complex block h [n_pairs, n_t]: the packed triangle walked row by row, each record
    gathered at s_ij (tt_tx[i], tt_rx[j]) and at s_ji (tt_tx[j], tt_rx[i]), the two ADDED TO EACH OTHER FIRST, the diagonal counted
    once.  -> dict(S, E, A, T, R, N) as tfm(); with ``terms`` t_re, t_im, t_e [n_pairs, n_f] (one term per record: the pair's sum)."""
    pre, pim = _planes(h)
    n_pairs = pre.shape[0]
    n_e = (int(np.sqrt(8 * n_pairs + 1)) - 1) // 2
    assert n_e * (n_e + 1) // 2 == n_pairs
    tau_tx, ok_tx, _ = legs(tt_tx, fs, t0)
    tau_rx, ok_rx, _ = (tau_tx, ok_tx, None) if tt_rx is None else legs(tt_rx, fs, t0)
    n_f = tau_tx.shape[1]
    S_re, S_im, E, A = (np.zeros(n_f) for _ in range(4))
    keep = {k: [] for k in ("t_re", "t_im", "t_e")}
    for i in range(n_e):
        j = np.arange(i, n_e)
        rows = packed_index(i, j, n_e)
        s_ij, ok_ij = position(tau_tx[i][None, :], ok_tx[i][None, :], tau_rx[j], ok_rx[j])
        s_ji, ok_ji = position(tau_tx[j], ok_tx[j], tau_rx[i][None, :], ok_rx[i][None, :])
        re1, im1 = _sample(pre[rows], pim[rows], s_ij, ok_ij)
        re2, im2 = _sample(pre[rows], pim[rows], s_ji, ok_ji)
        re2[0] = 0.0; im2[0] = 0.0                                       # the diagonal counts once
        re, im = _exact32(re1 + re2, "the pair's sum"), _exact32(im1 + im2, "the pair's sum")
        e = _exact32(_exact32(re1 * re1 + im1 * im1, "|p|^2") + _exact32(re2 * re2 + im2 * im2, "|p|^2"), "the pair's energy")
        S_re += re.sum(axis=0); S_im += im.sum(axis=0); E += e.sum(axis=0)
        A += (np.hypot(re1, im1) + np.hypot(re2, im2)).sum(axis=0)
        if terms:
            keep["t_re"].append(re); keep["t_im"].append(im); keep["t_e"].append(e)
    T, R = ok_tx.sum(axis=0).astype(np.int64), ok_rx.sum(axis=0).astype(np.int64)
    r = dict(S=_exact32(S_re, "S") + 1j * _exact32(S_im, "S"), E=_exact32(E, "E"), A=A, T=T, R=R, N=T * R)
    if terms:
        r.update({k: np.concatenate(v, axis=0) for k, v in keep.items()})
    return r


def synth(fmc, fs, d):
    """rtus_fmc_synth_tx as a plain loop: out[v][rx][n] = sum over tx of fmaf(w, x[i + 1] - x[i], x[i]), sh = d fs in fp64,
    m = ceil(sh), i = n - m, w = float32(m - sh); a tx with a non-finite delay or |sh| >= 1e8 is skipped.  Exact under the
    generator's rules (integer records, delays on the 1/4-sample lattice, n_tx <= 2^13) -> float32 [n_v, n_rx, n_t]"""
    fmc = np.asarray(fmc, dtype=f32).astype(f64)
    d = np.atleast_2d(np.asarray(d, dtype=f64))
    n_tx, n_rx, n_t = fmc.shape
    pad = np.concatenate([np.zeros((n_tx, n_rx, 1)), fmc, np.zeros((n_tx, n_rx, 1))], axis=2)   # x[-1] = x[n_t] = 0
    out = np.zeros((d.shape[0], n_rx, n_t))
    n = np.arange(n_t)
    for v in range(d.shape[0]):
        for tx in range(n_tx):
            with np.errstate(all="ignore"):
                sh = d[v, tx] * f64(fs)
            if not abs(sh) < 1.0e8:                                      # (NaN and infinities fail)
                continue
            m = np.ceil(sh)
            w = f64(f32(m - sh))
            assert w == m - sh, "the delay is not on the lattice"
            i = n - int(m)
            inside = (i >= -1) & (i < n_t)
            k = np.where(inside, i, -1) + 1                              # index into pad; -1 -> x[-1] = 0 (and x[0] after it)
            x0, x1 = np.where(inside, pad[tx][:, k], 0.0), np.where(inside, pad[tx][:, k + 1], 0.0)
            out[v] += _exact32(w * _exact32(x1 - x0, "x[i + 1] - x[i]") + x0, "the term")
            _exact32(out[v], "the running sum")
    return out.astype(f32)


# ------------------------------------------------------------------------------------------------------------ the generator
def records(rng, shape):
    """complex64 records [..., n_t] of integers in [-4, 4]; the first and the last sample of every record are non-zero in both
    parts (an index that wraps to sample 0, or a dropped last sample, changes the sum)"""
    def plane():
        x = rng.integers(-4, 5, shape).astype(f64)
        for k in (0, -1):
            e = x[..., k]
            e[e == 0] = 3.0
        return x
    return (plane() + 1j * plane()).astype(np.complex64)


def weights(rng, n_e, n_f):
    """complex64 [n_e, n_f] Gaussian integers with parts in [-2, 2]; about 1 % of the entries NaN or infinite"""
    w = (rng.integers(-2, 3, (n_e, n_f)) + 1j * rng.integers(-2, 3, (n_e, n_f))).astype(np.complex64)
    m = rng.random((n_e, n_f))
    w[m < 0.005] = np.nan
    w[(m >= 0.005) & (m < 0.01)] = np.complex64(complex(np.inf, 1.0))
    return w


def _round_pair(n_t, over):
    """two fp32 legs (a, b) with a + b < n_t exactly and fp32(a + b) == n_t; a + a and b + b are outside the record.
    ``over`` = False: the exact sum is the tie n_t - ulp / 2 (to even: n_t); True: above the tie"""
    b = np.nextafter(f32(n_t + 8), f32(0))                               # the largest fp32 below n_t + 8
    ulp = f64(n_t + 8) - f64(b)
    a = -(8.0 - ulp / 2 - (ulp / 4 if over else 0.0))
    assert f64(f32(a)) == a and a + f64(b) < n_t and f32(a) + b == f32(n_t), "no such pair of fp32 legs at this n_t"
    assert 2 * a < 0 and 2 * f64(b) >= n_t
    return a, f64(b)


def hand_columns(n_t):
    """[(name, the cycle of leg values in samples (element e takes cycle[e % len]; the second table starts one later), ...)].
    Every pair sum of every column is a whole sample or contributes nothing, except where the name ends in "_q"."""
    tiny = -1.0 - 2.0 ** -23
    return [
        ("zero_pm", (3.0, -3.0)),                                        # s = 3 + (-3) = +0; 6 and -6 beside it
        ("zero_neg", (-0.0, -0.0)),                                      # s = -0 (t0 = 0; else +0)
        ("zero_half", (0.0, 0.0)),
        ("tiny_neg", (1.0, tiny)),                                       # s = -2^-23: floor -1, w = 1 - 2^-23
        ("before_half", (-0.25, -0.25)),                                 # s = -0.5 from equal legs (one element)
        ("last", (n_t - 4.0, 3.0)),                                      # s = n_t - 1 exactly
        ("last_half", ((n_t - 1) / 2.0, (n_t - 1) / 2.0)),
        ("inlast_half_q", (n_t / 2.0 - 0.25, n_t / 2.0 - 0.25)),         # s = n_t - 0.5 from equal legs
        ("end", (n_t - 5.0, 5.0)),                                       # s = n_t exactly
        ("end_half", (n_t / 2.0, n_t / 2.0)),
        ("round_tie", _round_pair(n_t, False)),                          # exact sum < n_t, fp32 sum == n_t
        ("round_over", _round_pair(n_t, True)),
        ("e8_on", (1.0e8, 2.0, -1.0e8, 5.0)),
        ("e8_round", (ROUNDS, 2.0, -ROUNDS, 5.0)),                       # fp64 legs that round onto the fp32 1e8: no path
        ("e8_beside", (BESIDE, 2.0, -BESIDE, 5.0)),                      # paths; BESIDE + (-BESIDE) = 0 is in the record
        ("e8_mix", (1.0e8, 8.0 - BESIDE, ROUNDS, BESIDE, -1.0e8, -ROUNDS)),   # 1e8 + (8 - BESIDE) would be sample 16 if 1e8 had a path
        ("non_finite", (np.nan, 3.0, np.inf, 4.0, -np.inf, 1.0)),
        ("no_path", (np.nan,)),
    ]


ROUNDING = ("round_tie", "round_over", "e8_on", "e8_round", "e8_beside", "e8_mix")   # where fp64 oracles and the header may differ


def table(rng, n_e, n_t, t0, fs=FS, n_f=N_F, second=False, whole=False):
    """-> (tt float64 [n_e, n_f] in seconds, cols {name: column}).  The first columns are random: half positions on the 1/4-sample
    lattice (``whole``: whole samples) over [-3, n_t / 2 + 3], 3 % of them NaN; the last columns are hand_columns(n_t) (``whole``:
    without the "_q" ones).  ``second``: the other table of a two-table case (the cycles start one later)."""
    h = 0.5 * t0 * fs
    assert h == np.floor(h) and fs == FS
    hand = [c for c in hand_columns(n_t) if not (whole and c[0].endswith("_q"))]
    n_r = n_f - len(hand)
    step = 1 if whole else 4
    leg = rng.integers(-3 * step, (n_t // 2 + 3) * step + 1, (n_e, n_r)).astype(f64) / step
    leg[rng.random(leg.shape) < 0.03] = np.nan
    cols = {}
    extra = np.empty((n_e, len(hand)))
    for k, (name, cyc) in enumerate(hand):
        extra[:, k] = [cyc[(e + second) % len(cyc)] for e in range(n_e)]
        cols[name] = n_r + k
    leg = np.concatenate([leg, extra], axis=1)
    with np.errstate(all="ignore"):
        tt = (leg + h) / fs if h else leg / fs                           # (-0.0 + 0.0 would lose the sign)
        back = tt * fs - h
    assert np.array_equal(back, np.where(leg == 0, back, leg), equal_nan=True), "a time does not give its leg back exactly"
    return tt, cols


def census(tau_a, ok_a, va, tau_b, ok_b, vb, n_t, hmc=False):
    """how many pairs (legs) of a case fall into each edge class.  tau/ok/v: legs() of the two tables [n_e, n_f].  ``hmc``: the
    pairs are (i, j) and (j, i) of one aperture, which for the census is the same set as the full matrix"""
    s, ok = position(tau_a[:, None, :], ok_a[:, None, :], tau_b[None, :, :], ok_b[None, :, :])
    with np.errstate(all="ignore"):
        exact = va[:, None, :] + vb[None, :, :]                          # the sum of the fp64 legs (exact at these magnitudes)
        fin = ok & np.isfinite(exact)
    tau = np.concatenate([tau_a, tau_b]).astype(f64)
    v = np.concatenate([va, vb])
    with np.errstate(all="ignore"):
        return {
            "s in [-1, 0)": int((ok & (s >= -1) & (s < 0)).sum()),
            "s == 0": int((ok & (s == 0)).sum()),
            "s == -0.0": int((ok & (s == 0) & np.signbit(s)).sum()),
            "s == -2^-23": int((ok & (s == f32(-2.0 ** -23))).sum()),
            "s in (n_t - 1, n_t)": int((ok & (s > n_t - 1) & (s < n_t)).sum()),
            "s == n_t - 1": int((ok & (s == n_t - 1)).sum()),
            "s == n_t": int((ok & (s == n_t)).sum()),
            "exact sum < n_t, fp32 sum == n_t": int((fin & (s == n_t) & (np.where(fin, exact, 0) < n_t)).sum()),
            "leg == +-1e8": int((np.abs(tau) == 1.0e8).sum() - ((np.abs(tau) == 1.0e8) & (tau != v)).sum()),
            "leg rounds onto +-1e8": int(((np.abs(tau) == 1.0e8) & (tau != v)).sum()),
            "leg == +-99999992": int((np.abs(tau) == BESIDE).sum()),
        }


def sparse_value(head, tail, n_t, s):
    """a record that is zero except for its first len(head) and last len(tail) samples, at the fp32 positions s (whole or on the
    lattice) -> fp64: the long-record cases, without the record"""
    s = np.asarray(s, dtype=f32)
    fl = np.floor(s)
    w = (s - fl).astype(f64)
    i = fl.astype(np.int64)

    def x(k):
        k = np.asarray(k)
        out = np.zeros(k.shape, dtype=np.complex128)
        lo = (k >= 0) & (k < len(head))
        hi = (k >= n_t - len(tail)) & (k < n_t)
        out[lo] = np.asarray(head)[k[lo]]
        out[hi] = np.asarray(tail)[k[hi] - (n_t - len(tail))]
        return out
    x0, x1 = x(i), x(i + 1)
    inrec = (i >= 0) & (i < n_t)
    p = np.where(inrec, x0 + w * (x1 - x0), 0.0)
    _exact32(p.real, "p"); _exact32(p.imag, "p")
    return p


# ------------------------------------------------------------------------------------------------------------ the cases
T0 = 3.0 * 2.0 ** -24                # a time origin that is not zero: t0 fs / 2 = 3 samples
#             seed n_tx n_rx tables  t0      (tables: "one" — tt_rx is tt_tx; "copy" — an equal copy: another pointer; "two")
FULL_CASES = {
    "1x1_one": (11, 1, 1, "one", 0.0),
    "1x1_two": (12, 1, 1, "two", T0),
    "3x15": (13, 3, 15, "two", 0.0),                 # a tail of fifteen gathers
    "2x16": (14, 2, 16, "two", T0),                  # exactly one group of sixteen
    "2x17": (15, 2, 17, "two", 0.0),                 # a group and a tail of one; the weighted kernel's second tile
    "5x63": (16, 5, 63, "two", T0),                  # three groups and a tail of fifteen
    "64x64_one": (17, 64, 64, "one", T0),            # one table, one tile: the transmit delay is a row of the tile
    "64x64_copy": (17, 64, 64, "copy", T0),          # the same numbers through two pointers: the transmit delay is formed again
    "65x65_one": (18, 65, 65, "one", 0.0),           # one table, two tiles: not in the tile
    "4x129": (19, 4, 129, "two", T0),                # three receive tiles
}
HMC_SIZES = (1, 15, 16, 17, 31, 32, 33, 48, 64, 65, 81)
_cache = {}


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return d


def full_case(name, whole=False):
    """-> dict(a complex64 [n_tx, n_rx, n_t], fs, t0, n_t, tt_tx, tt_rx (None: one table), w_tx, w_rx (None: w_tx), cols, tables)"""
    key = ("full", name, whole)
    if key not in _cache:
        seed, n_tx, n_rx, tables, t0 = FULL_CASES[name]
        rng = np.random.default_rng(seed + 1000 * whole)
        a = records(rng, (n_tx, n_rx, N_T))
        tt_tx, cols = table(rng, n_tx, N_T, t0, whole=whole)
        w_tx = weights(rng, n_tx, N_F)
        tt_rx = w_rx = None
        if tables == "two":
            tt_rx, _ = table(rng, n_rx, N_T, t0, second=True, whole=whole)
            w_rx = weights(rng, n_rx, N_F)
        elif tables == "copy":
            tt_rx, w_rx = tt_tx.copy(), w_tx.copy()
        _cache[key] = _frozen(dict(a=a, fs=FS, t0=t0, n_t=N_T, tt_tx=tt_tx, tt_rx=tt_rx, w_tx=w_tx, w_rx=w_rx, cols=cols, tables=tables))
    return _cache[key]


def hmc_case(n_e, two, whole=False):
    """-> dict(h complex64 [n_pairs, n_t], fs, t0, n_t, tt_tx, tt_rx (None: one table), cols)"""
    key = ("hmc", n_e, two, whole)
    if key not in _cache:
        rng = np.random.default_rng(100 + n_e + 1000 * whole)
        t0 = T0 if n_e % 2 else 0.0
        h = records(rng, (n_e * (n_e + 1) // 2, N_T))
        tt_tx, cols = table(rng, n_e, N_T, t0, whole=whole)
        tt_rx = table(rng, n_e, N_T, t0, second=True, whole=whole)[0] if two else None
        _cache[key] = _frozen(dict(h=h, fs=FS, t0=t0, n_t=N_T, tt_tx=tt_tx, tt_rx=tt_rx, cols=cols))
    return _cache[key]


def full_model(name, whole=False, terms=False):
    key = ("full_model", name, whole, terms)
    if key not in _cache:
        c = full_case(name, whole)
        _cache[key] = _frozen(tfm(c["a"], c["fs"], c["t0"], c["tt_tx"], c["tt_rx"], c["w_tx"], c["w_rx"], terms=terms))
    return _cache[key]


def hmc_model(n_e, two, whole=False, terms=False):
    key = ("hmc_model", n_e, two, whole, terms)
    if key not in _cache:
        c = hmc_case(n_e, two, whole)
        _cache[key] = _frozen(tfm_hmc(c["h"], c["fs"], c["t0"], c["tt_tx"], c["tt_rx"], terms=terms))
    return _cache[key]


# ------------------------------------------------------------------------------------------------------------ synthesis
def synth_case(n_tx, n_v, n_t, n_rx=2):
    """-> (fmc float32 [n_tx, n_rx, n_t] of integers in [-4, 4], first and last sample non-zero; delays float64 [n_v, n_tx] in
    seconds at fs = FS).  Shifts on the 1/4-sample lattice over [-(n_t + 3), n_t + 3]; in every law, spread over the transmit
    elements (64 further in each law: every tile of 128 gets them), the hand-made ones: whole shifts that put i = n - m on -1, 0,
    n_t - 1 and past either end, quarter shifts beside them, NaN, infinities, +-1e8 (not fired) and +-(1e8 - 1/4) (fired, nothing
    inside the record)."""
    key = ("synth", n_tx, n_v, n_t, n_rx)
    if key not in _cache:
        rng = np.random.default_rng(7000 + 1000 * n_tx + 10 * n_t + n_v)
        fmc = np.ascontiguousarray(records(rng, (n_tx, n_rx, n_t)).real.astype(f32))
        sh = rng.integers(-4 * (n_t + 3), 4 * (n_t + 3) + 1, (n_v, n_tx)).astype(f64) / 4
        special = [0.0, -0.0, 1.0, -1.0, 0.25, -0.25, 0.75, n_t - 1.0, n_t - 0.75, float(n_t), n_t + 1.0, -(n_t - 1.0), -float(n_t),
                   -(n_t - 0.25), np.nan, np.inf, -np.inf, 1.0e8, -1.0e8, 1.0e8 - 0.25, -(1.0e8 - 0.25)]
        for v in range(n_v):
            for k, x in enumerate(special):
                sh[v, (13 * k + 5 + 64 * v) % n_tx] = x
        d = sh / FS
        with np.errstate(all="ignore"):
            assert np.array_equal(d * FS, sh, equal_nan=True)
        fmc.flags.writeable = False
        d.flags.writeable = False
        _cache[key] = (fmc, d)
    return _cache[key]


def synth_census(d, n_t):
    """how many (law, tx) of a synthesis case fall into each class of the kernel's index rule"""
    with np.errstate(all="ignore"):
        sh = np.asarray(d, dtype=f64) * FS
        fired = np.abs(sh) < 1.0e8
        m = np.where(fired, np.ceil(sh), 0.0)
        w = np.where(fired, m - sh, 0.0)
    tile2 = np.arange(sh.shape[1])[None, :] >= 128
    return {
        "i == -1 with w > 0": int((fired & (m >= 1) & (m <= n_t) & (w > 0)).sum()),
        "i == -1 with w == 0": int((fired & (m >= 1) & (m <= n_t) & (w == 0)).sum()),
        "i == n_t - 1 with w > 0": int((fired & (m <= 0) & (m >= -(n_t - 1)) & (w > 0)).sum()),
        "wholly before the record": int((fired & (m > n_t)).sum()),
        "wholly past the record": int((fired & (m <= -n_t)).sum()),
        "fired at |shift| just below 1e8": int((fired & (np.abs(sh) > 9.0e7)).sum()),
        "not fired": int((~fired).sum()),
        "fired in the second tile": int((fired & tile2).sum()),
    }
