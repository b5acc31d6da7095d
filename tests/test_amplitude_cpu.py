"""CPU: the amplitude oracle (tests/amplitude_numpy.py) against first principles — the plane-wave coefficients against a 40-digit
mpmath solve of the boundary conditions, energy balance, reciprocity and normal incidence; the spreading factor against a
finite-difference ray tube traced with Snell's law through a wavy spline and the backwall; the phase convention against a broadband
pulse past a critical angle; the weighted delay-and-sum oracle against the unweighted one."""
import mpmath as mp
import numpy as np
import pytest

import amplitude_numpy as A
import surface_numpy as S
import tfm_analytic_numpy as TA

WATER_STEEL = (1000.0, 1480.0, 7850.0, 5900.0, 3230.0)        # rho1, c1, rho2, c_l, c_t
OIL_ALU = (870.0, 1740.0, 2700.0, 6320.0, 3080.0)
PAIRS = [WATER_STEEL, OIL_ALU]


# ---------------------------------------------------------------------------------------------- mpmath: the boundary conditions
def _mp_wave(mode, p, c, lam, mu, s):
    """(u_n, sigma_nn, sigma_tn) / (i w) of one wave from sigma = lam div(u) I + mu (grad u + grad u^T), in mpmath"""
    a = 1 / (c * c) - p * p
    q = mp.sqrt(a) if a >= 0 else 1j * mp.sqrt(-a)
    st, sn = p, s * q                                              # slowness (t, n)
    dt, dn = c * st, c * sn                                        # direction
    pt, pn = (dt, dn) if mode == "L" else (-dn, dt)                # polarisation
    div = st * pt + sn * pn
    return pn, lam * div + 2 * mu * sn * pn, mu * (st * pn + sn * pt)


def _mp_solve(cols, rhs):
    M = mp.matrix([[cols[j][i] for j in range(len(cols))] for i in range(len(rhs))])
    return mp.lu_solve(M, mp.matrix(rhs))


def _mp_coefs(kind, mode, p, rho1, c1, rho2, cl, ct):
    mp.mp.dps = 40
    p = mp.mpf(p)
    lf, mu2, l2 = rho1 * c1 ** 2, rho2 * ct ** 2, rho2 * (cl ** 2 - 2 * ct ** 2)
    lf, mu2, l2 = mp.mpf(lf), mp.mpf(mu2), mp.mpf(l2)
    c1, cl, ct = mp.mpf(c1), mp.mpf(cl), mp.mpf(ct)
    cm = cl if mode == "L" else ct
    if kind == "fs":
        inc, ref = _mp_wave("L", p, c1, lf, 0, 1), _mp_wave("L", p, c1, lf, 0, -1)
        wl, wt = _mp_wave("L", p, cl, l2, mu2, 1), _mp_wave("T", p, ct, l2, mu2, 1)
        x = _mp_solve([(-ref[0], -ref[1], 0), wl, wt], [inc[0], inc[1], 0])
    elif kind == "sf":
        inc = _mp_wave(mode, p, cm, l2, mu2, -1)
        wl, wt = _mp_wave("L", p, cl, l2, mu2, 1), _mp_wave("T", p, ct, l2, mu2, 1)
        tf = _mp_wave("L", p, c1, lf, 0, -1)
        x = _mp_solve([wl, wt, (-tf[0], -tf[1], 0)], [-inc[0], -inc[1], -inc[2]])
    else:
        inc = _mp_wave(mode, p, cm, l2, mu2, 1)
        wl, wt = _mp_wave("L", p, cl, l2, mu2, -1), _mp_wave("T", p, ct, l2, mu2, -1)
        x = _mp_solve([wl[1:], wt[1:]], [-inc[1], -inc[2]])
    return np.array([complex(v) for v in x])


def _np_coefs(kind, mode, p, rho1, c1, rho2, cl, ct):
    if kind == "fs":
        return np.array(A.fluid_solid(p, rho1, c1, rho2, cl, ct), dtype=complex)
    if kind == "sf":
        return np.array(A.solid_fluid(mode, p, rho1, c1, rho2, cl, ct), dtype=complex)
    return np.array(A.free(mode, p, rho2, cl, ct), dtype=complex)


CASES = [("fs", "L"), ("sf", "L"), ("sf", "T"), ("free", "L"), ("free", "T")]


def _slowness(kind, mode, deg, rho1, c1, rho2, cl, ct):
    c_in = c1 if kind == "fs" else (cl if mode == "L" else ct)
    return np.sin(np.radians(deg)) / c_in


@pytest.mark.parametrize("pair", PAIRS, ids=["water-steel", "oil-aluminium"])
@pytest.mark.parametrize("kind,mode", CASES)
def test_closed_forms_against_mpmath(pair, kind, mode):
    rho1, c1, rho2, cl, ct = pair
    degs = np.r_[np.arange(0.0, 89.5, 1.0), 89.0, 13.0, 14.4, 14.6, 27.5, 28.0, -35.0]
    for d in degs:
        p = _slowness(kind, mode, d, *pair)
        got = _np_coefs(kind, mode, p, *pair)
        ref = _mp_coefs(kind, mode, p, *pair)
        assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref))), (kind, mode, d, got, ref)


def _energy_terms(kind, mode, p, rho1, c1, rho2, cl, ct):
    """rho c cos(theta) of the incident wave and of every outgoing wave (0 for an evanescent one)"""
    def f(rho, c):
        a = 1 / c ** 2 - p ** 2
        return rho * c * c * np.sqrt(a) if a > 0 else 0.0
    if kind == "fs":
        return f(rho1, c1), [f(rho1, c1), f(rho2, cl), f(rho2, ct)]
    c_in = cl if mode == "L" else ct
    if kind == "sf":
        return f(rho2, c_in), [f(rho2, cl), f(rho2, ct), f(rho1, c1)]
    return f(rho2, c_in), [f(rho2, cl), f(rho2, ct)]


@pytest.mark.parametrize("pair", PAIRS, ids=["water-steel", "oil-aluminium"])
@pytest.mark.parametrize("kind,mode", CASES)
def test_energy_balance(pair, kind, mode):
    for d in np.r_[np.arange(0.0, 89.5, 0.5), -20.0, -60.0]:
        p = _slowness(kind, mode, d, *pair)
        e_in, e_out = _energy_terms(kind, mode, p, *pair)
        c = _np_coefs(kind, mode, p, *pair)
        bal = sum(e * abs(x) ** 2 for e, x in zip(e_out, c))
        assert abs(bal - e_in) <= 1e-12 * e_in, (kind, mode, d, bal, e_in)


def _energy_norm(rho_in, c_in, rho_out, c_out, p):
    ci, co = np.sqrt(1 / c_in ** 2 - p ** 2) * c_in, np.sqrt(1 / c_out ** 2 - p ** 2) * c_out
    return np.sqrt(rho_out * c_out * co / (rho_in * c_in * ci))


@pytest.mark.parametrize("pair", PAIRS, ids=["water-steel", "oil-aluminium"])
def test_reciprocity(pair):
    rho1, c1, rho2, cl, ct = pair
    sp = {"L": cl, "T": ct}
    signs = {}
    for p in np.linspace(-0.99, 0.99, 45) / max(cl, c1):
        for m in ("L", "T"):
            if 1 / sp[m] ** 2 - p ** 2 <= 0 or 1 / c1 ** 2 - p ** 2 <= 0:
                continue
            fwd = A.fluid_solid(p, rho1, c1, rho2, cl, ct)[1 if m == "L" else 2] * _energy_norm(rho1, c1, rho2, sp[m], p)
            bwd = A.solid_fluid(m, p, rho1, c1, rho2, cl, ct)[2] * _energy_norm(rho2, sp[m], rho1, c1, p)
            r = complex(fwd / bwd) if abs(bwd) > 1e-9 else None
            if r is not None:
                assert abs(abs(r) - 1) <= 1e-12 and abs(r.imag) <= 1e-12
                assert signs.setdefault(("s", m), np.sign(r.real)) == np.sign(r.real)
        for mi, mo in (("L", "T"),):
            if 1 / ct ** 2 - p ** 2 <= 0 or 1 / cl ** 2 - p ** 2 <= 0:
                continue
            fwd = A.free(mi, p, rho2, cl, ct)[1] * _energy_norm(rho2, cl, rho2, ct, p)
            bwd = A.free(mo, p, rho2, cl, ct)[0] * _energy_norm(rho2, ct, rho2, cl, p)
            if abs(bwd) > 1e-9:
                r = complex(fwd / bwd)
                assert abs(abs(r) - 1) <= 1e-12 and abs(r.imag) <= 1e-12
                assert signs.setdefault("b", np.sign(r.real)) == np.sign(r.real)
    assert len(signs) == 3


@pytest.mark.parametrize("pair", PAIRS, ids=["water-steel", "oil-aluminium"])
def test_normal_incidence(pair):
    rho1, c1, rho2, cl, ct = pair
    z1, z2 = rho1 * c1, rho2 * cl
    R, TL, TT = A.fluid_solid(0.0, *pair)
    assert abs(TL - 2 * z1 / (z1 + z2)) < 1e-15 and abs(TT) < 1e-15 and abs(R - (z2 - z1) / (z1 + z2)) < 1e-15
    assert abs(A.solid_fluid("L", 0.0, *pair)[2] - 2 * z2 / (z1 + z2)) < 1e-14
    RL, RT = A.free("L", 0.0, rho2, cl, ct)
    assert abs(RL + 1) < 1e-15 and abs(RT) < 1e-15                  # (u_n of the reflected L counts along its own direction)
    RL, RT = A.free("T", 0.0, rho2, cl, ct)
    assert abs(RL) < 1e-15 and abs(abs(RT) - 1) < 1e-15


# ---------------------------------------------------------------------------------------------- spreading: finite-difference ray tube
X0, DX, NS = -0.03, 1e-3, 61
ZB = 0.05
C1, R1, R2, CL, CT = 1480.0, 1000.0, 7850.0, 5900.0, 3230.0
MEDIA = (C1, R1, CL, CT, R2, ZB)


def _wavy():
    x = X0 + DX * np.arange(NS)
    return 0.02 + 0.0012 * np.sin(2 * np.pi * x / 0.012)


def _rot(d, a):
    c, s = np.cos(a), np.sin(a)
    return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1]])      # angle from +z towards +x grows by a


def _hit_surface(coef, P, d, l0):
    l = l0
    for _ in range(60):
        x = P[0] + l * d[0]
        s, s1, _ = S.spline_eval(coef, X0, DX, np.array([x]))
        f = s[0] - (P[1] + l * d[1])
        l -= f / (s1[0] * d[0] - d[1])
        if abs(f) < 1e-17:
            break
    x = P[0] + l * d[0]
    s, s1, s2 = S.spline_eval(coef, X0, DX, np.array([x]))
    n = np.array([-s1[0], 1.0]) / np.hypot(s1[0], 1.0)
    return np.array([x, s[0]]), n, s2[0]


def _snell(d, n, c_in, c_out, reflect):
    sg = 1.0 if d @ n > 0 else -1.0
    n = n * sg
    t = np.array([n[1], -n[0]])
    p = (d @ t) / c_in
    q = np.sqrt(1 / c_out ** 2 - p ** 2)
    return c_out * (p * t + (-q if reflect else q) * n)


def _trace(coef, start, d, legs, lens):
    """legs: [(kind, c_before, c_after)], kind 'surf' / 'back'; lens: the main ray's segment lengths (Newton's first guess)"""
    P = np.array(start, dtype=float)
    for (kind, ci, co), l0 in zip(legs, lens):
        if kind == "surf":
            Q, n, _ = _hit_surface(coef, P, d, l0)
            d = _snell(d, n, ci, co, False)
        else:
            Q = P + (ZB - P[1]) / d[1] * d
            d = _snell(d, np.array([0.0, 1.0]), ci, co, True)
        P = Q
    return P, d


def _offset(P, d, F, dm):
    """where the line P + l d crosses the line through F perpendicular to dm, along (dm_z, -dm_x)"""
    e = np.array([dm[1], -dm[0]])
    M = np.array([[d[0], -e[0]], [d[1], -e[1]]])
    l, w = np.linalg.solve(M, F - P)
    return w


def _geometry(coef, leg, xe, phi, l_last):
    """shoot the leg from the element (xe, 0) at launch angle phi: (x_entry, x_back, F) obeying Snell's law exactly"""
    sp = {"L": CL, "T": CT}
    d = np.array([np.sin(phi), np.cos(phi)])
    S_, n, _ = _hit_surface(coef, np.array([xe, 0.0]), d, 0.02 / d[1])
    d = _snell(d, n, C1, sp[leg[0]], False)
    if len(leg) == 1:
        return S_[0], np.nan, S_ + l_last * d
    B = S_ + (ZB - S_[1]) / d[1] * d
    d = _snell(d, np.array([0.0, 1.0]), sp[leg[0]], sp[leg[1]], True)
    return S_[0], B[0], B + l_last * d


def _fd_G(coef, leg, up, E, xs, xb, F, delta=1e-6):
    sp = {"L": CL, "T": CT}
    s, _, _ = S.spline_eval(coef, X0, DX, np.array([xs]))
    Sp = np.array([xs, s[0]])
    pts = [E, Sp] + ([np.array([xb, ZB])] if len(leg) == 2 else []) + [F]
    cs = [C1, sp[leg[0]]] + ([sp[leg[1]]] if len(leg) == 2 else [])
    kinds = ["surf"] + (["back"] if len(leg) == 2 else [])
    if up:
        pts, cs, kinds = pts[::-1], cs[::-1], kinds[::-1]
    lens = [np.hypot(*(pts[k + 1] - pts[k])) for k in range(len(pts) - 1)]
    legs = [(k, cs[i], cs[i + 1]) for i, k in enumerate(kinds)]
    d0 = (pts[1] - pts[0]) / lens[0]
    dm = (pts[-1] - pts[-2]) / lens[-1]
    w = []
    for sgn in (1, -1):
        P, d = _trace(coef, pts[0], _rot(d0, sgn * delta), legs, lens)
        w.append(_offset(P, d, pts[-1], dm))
    J = (w[0] - w[1]) / (2 * delta)
    # the cosine product from the main ray's geometry
    return J


@pytest.mark.parametrize("leg", ["L", "T", "LL", "LT", "TL", "TT"])
@pytest.mark.parametrize("up", [False, True], ids=["down", "up"])
def test_spreading_against_a_finite_difference_ray_tube(leg, up):
    zs = _wavy()
    coef = S.spline(X0, DX, zs)
    checked, signs = 0, set()
    for xe in np.linspace(-0.012, 0.012, 9):
        for phi in np.radians([-9.0, -5.0, -2.0, 2.0, 4.5, 8.0, 11.0]):
            with np.errstate(invalid="ignore"):
                xs, xb, F = _geometry(coef, leg, xe, phi, 0.012)
            if not (F[1] > 0.025 and F[1] < ZB):                      # (NaN: past a critical angle on this ripple)
                continue
            amp, parts = A.amplitude(X0, DX, zs, MEDIA, leg, up, xe, 0.0, F[0], F[1], xs, xb, parts=True)
            J_fd = _fd_G(coef, leg, up, np.array([xe, 0.0]), xs, xb, F)
            assert abs(abs(parts["J"]) - abs(J_fd)) <= 1e-6 * abs(J_fd), (leg, up, xe, phi, parts["J"], J_fd)
            G_fd = np.sqrt(parts["prod"] / abs(J_fd))
            assert abs(parts["G"] - G_fd) <= 1e-6 * G_fd
            s2 = S.spline_eval(coef, X0, DX, np.array([xs]))[2][0]
            signs.add(np.sign(s2))
            checked += 1
    assert checked >= 15 and signs == {-1.0, 1.0}                # convex and concave entry points


def test_spreading_flat_closed_forms():
    zs = np.full(NS, 0.02)
    xe, xs = -0.001, 0.001
    for leg in ("L", "T"):
        c2 = CL if leg == "L" else CT
        s1 = (xs - xe) / np.hypot(xs - xe, 0.02)
        s2 = s1 * c2 / C1
        d2 = np.array([s2, np.sqrt(1 - s2 * s2)])
        F = np.array([xs, 0.02]) + 0.015 * d2
        r1, r2 = np.hypot(xs - xe, 0.02), 0.015
        c1t, c2t = np.sqrt(1 - s1 * s1), np.sqrt(1 - s2 * s2)
        ref = 1 / np.sqrt(r1 + r2 * (c2 / C1) * c1t ** 2 / c2t ** 2)
        for up in (False, True):
            _, parts = A.amplitude(X0, DX, zs, MEDIA, leg, up, xe, 0.0, F[0], F[1], xs, parts=True)
            if not up:
                assert abs(parts["G"] - ref) <= 1e-12 * ref
            else:                                                   # up: launched in the part, ending in the couplant
                refu = 1 / np.sqrt(r2 + r1 * (C1 / c2) * c2t ** 2 / c1t ** 2)
                assert abs(parts["G"] - refu) <= 1e-12 * refu


# ---------------------------------------------------------------------------------------------- phase convention
def _analytic(x):
    n = x.shape[-1]
    X = np.fft.fft(x)
    h = np.zeros(n)
    h[0] = 1
    h[1:(n + 1) // 2] = 2
    if n % 2 == 0:
        h[n // 2] = 1
    return np.fft.ifft(X * h)


@pytest.mark.parametrize("kind,mode,deg", [("fs", "L", 26.0), ("free", "T", 36.0), ("free", "T", 60.0), ("sf", "T", 36.0)])
def test_phase_convention(kind, mode, deg):
    """the e^{-iwt} solution applied to a broadband pulse (R for the physical w > 0, i.e. numpy's NEGATIVE frequencies, and its
    conjugate for the others): the output's analytic signal is the TABULATED coefficient (the conjugate) times the input's.  Every
    case is past a critical angle: fluid -> T in steel past the first, T at the backwall and T -> couplant past T -> L conversion."""
    pair = WATER_STEEL
    p = _slowness(kind, mode, deg, *pair)
    c = _np_coefs(kind, mode, p, *pair)
    R = c[2] if kind in ("fs", "sf") else c[1]                         # T out of the couplant, the couplant out of T, T -> T
    assert abs(R.imag) > 0.1 * abs(R)                                   # a complex coefficient: the test sees the convention
    n, fs, f0 = 4096, 100e6, 5e6
    t = np.arange(n) / fs - 20e-6
    x = np.cos(2 * np.pi * f0 * t) * np.exp(-(t * f0 / 2.0) ** 2)      # (no DC to speak of: its phase is undefined)
    X = np.fft.fft(x)
    fr = np.fft.fftfreq(n)
    H = np.where(fr < 0, R, np.conj(R))                                 # numpy's e^{+i 2 pi f t}: f < 0 is the physical w > 0
    H[0] = R.real
    y = np.fft.ifft(X * H).real
    ya, xa = _analytic(y), _analytic(x)
    assert np.max(np.abs(ya - np.conj(R) * xa)) <= 1e-9 * np.max(np.abs(xa))
    assert np.max(np.abs(ya - R * xa)) > 0.1 * np.max(np.abs(xa))      # (and not the coefficient itself)


# ---------------------------------------------------------------------------------------------- the weighted delay-and-sum oracle
def test_weighted_oracle_with_unit_weights_is_the_analytic_oracle():
    rng = np.random.default_rng(3)
    n_tx, n_rx, n_t, n_f, fs = 5, 6, 64, 40, 1.0
    a = (rng.standard_normal((n_tx, n_rx, n_t)) + 1j * rng.standard_normal((n_tx, n_rx, n_t))).astype(np.complex64)
    ttx, trx = rng.uniform(-5, 40, (n_tx, n_f)), rng.uniform(-5, 40, (n_rx, n_f))
    ttx[1, 3] = np.nan
    trx[2, 5] = np.inf
    Sw, P = A.tfm_weighted(a, fs, ttx, np.ones((n_tx, n_f)), trx, np.ones((n_rx, n_f)))
    ref = TA.tfm_analytic(a, fs, 0.0, ttx, trx)["image"]
    assert np.max(np.abs(Sw - ref)) <= 1e-4 * np.max(np.abs(ref))
    okt = np.isfinite(ttx).sum(0)
    okr = np.isfinite(trx).sum(0)
    assert np.array_equal(P, (okt * okr).astype(float))
