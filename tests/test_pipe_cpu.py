"""CPU: the lens-to-pipe-wall oracle (tests/pipe_numpy.py) against a 40-digit joint solve in (alpha, beta) at the corners of the
reference's sweep, Snell's law at both interfaces, the lens-only limit, the validity rules and the lens clearance; argument
validation of rtus_tt_pipe* through ctypes (status codes, no GPU touched) and of the Python layer."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import pipe_numpy as O

mp.mp.dps = 40
LENS = O.Lens()
XE = np.array([-0.0189, 0.0, 0.0189])
ZE = np.full(3, O.D)
CORNERS = [(r, off) for r in (0.01, 0.037, 0.06) for off in (-0.01, 0.0038, 0.01)]


def _wall_points(pipe, depth_frac=0.4, deg=(-14.0, 3.0, 16.0)):
    r = pipe.r - depth_frac * (pipe.r - pipe.ri)
    th = np.radians(np.asarray(deg))
    return pipe.x0 + r * np.sin(th), r * np.cos(th)


def _mp_solve(xe, ze, xf, zf, pipe, a0, b0):
    """T at the stationary point of |P(a) - E| / c1 + |Q(b) - P(a)| / c2 + |F - Q(b)| / c3 near (a0, b0), in mpmath"""
    c1, c2, c3, d = mp.mpf(O.C1), mp.mpf(O.C2), mp.mpf(pipe.c3), mp.mpf(O.L0) + mp.mpf(O.H0)
    Tl = mp.mpf(O.L0) / c1 + mp.mpf(O.H0) / c2
    A = c1 ** 2 / c2 ** 2 - 1
    Cc = c1 ** 2 * Tl ** 2 - d ** 2
    E, F = (mp.mpf(float(xe)), mp.mpf(float(ze))), (mp.mpf(float(xf)), mp.mpf(float(zf)))
    R, X0 = mp.mpf(pipe.r), mp.mpf(pipe.x0)

    def P(a):
        B = 2 * d * mp.cos(a) - 2 * Tl * c1 ** 2 / c2
        h = (-B - mp.sqrt(B ** 2 - 4 * A * Cc)) / (2 * A)
        return h * mp.sin(a), h * mp.cos(a)

    def T(a, b):
        px, pz = P(a)
        qx, qz = X0 + R * mp.sin(b), R * mp.cos(b)
        return (mp.sqrt((px - E[0]) ** 2 + (pz - E[1]) ** 2) / c1 + mp.sqrt((qx - px) ** 2 + (qz - pz) ** 2) / c2
                + mp.sqrt((F[0] - qx) ** 2 + (F[1] - qz) ** 2) / c3)
    if abs(a0) == O.ALPHA_MAX:          # the lens leg's least time pinned at an end of the interval (near the focus): beta alone
        a = mp.mpf(float(a0))
        b = mp.findroot(lambda v: mp.diff(lambda w: T(a, w), v), mp.mpf(float(b0)))
        return T(a, b), a, b
    g = lambda a, b: (mp.diff(lambda v: T(v, b), a), mp.diff(lambda v: T(a, v), b))      # noqa: E731
    a, b = mp.findroot(g, (mp.mpf(float(a0)), mp.mpf(float(b0))))
    return T(a, b), a, b


@pytest.mark.parametrize("r_outer,off", CORNERS)
def test_oracle_against_mpmath(r_outer, off):
    pipe = O.Pipe(r_outer, off, 0.6 * r_outer)
    xf, zf = _wall_points(pipe)
    # two pairs per corner, about 20 in all: the edge elements against the outer points, the centre element against the middle one
    pairs = (np.array([0, 2]), np.array([0, 2])) if r_outer != 0.037 else (np.array([0, 1, 2]), np.array([2, 1, 0]))
    o = O.table(LENS, pipe, XE, ZE, xf, zf, pairs=pairs)
    assert np.isfinite(o["t"]).all()
    for n, (i, j) in enumerate(zip(*pairs)):
        t, a, b = _mp_solve(XE[i], ZE[i], xf[j], zf[j], pipe, o["alpha"][n], o["beta"][n])
        assert abs(float(t) - o["t"][n]) <= 1e-14 * o["t"][n], (r_outer, off, i, j)
        assert abs(float(a) - o["alpha"][n]) <= 1e-9 and abs(float(b) - o["beta"][n]) <= 1e-9


@pytest.mark.parametrize("r_outer,off", [(0.037, 0.0038), (0.01, -0.01), (0.06, 0.01)])
def test_oracle_paths_obey_snell(r_outer, off):
    pipe = O.Pipe(r_outer, off, 0.5 * r_outer)
    xf, zf = _wall_points(pipe, deg=np.linspace(-20, 20, 9))
    o = O.table(LENS, pipe, XE, ZE, xf, zf)
    g = np.isfinite(o["t"])
    assert g.mean() > 0.5
    ie, jf = np.nonzero(g)
    r1, r2 = O.snell_residuals(LENS, pipe, XE[ie], ZE[ie], xf[jf], zf[jf], o["alpha"][g], o["beta"][g])
    free = np.abs(o["alpha"][g]) < O.ALPHA_MAX              # (a lens leg pinned at an end of the interval refracts by no law)
    assert np.max(np.abs(r1[free]), initial=0.0) <= 1e-9 and np.max(np.abs(r2)) <= 1e-9


def test_oracle_equal_speeds_is_the_lens_leg():
    """c3 = c2, a solid bar: the wall is water, the outer circle refracts nothing and T is the lens leg's least time to F"""
    pipe = O.Pipe(0.037, 0.0038, 0.0, c3=O.C2)
    rng = np.random.default_rng(3)
    rr, th = rng.uniform(0.002, 0.036, 40), rng.uniform(-0.5, 0.5, 40)
    xf, zf = 0.0038 + rr * np.sin(th), rr * np.cos(th)
    o = O.table(LENS, pipe, XE, ZE, xf, zf)
    ref, _ = O.lens_min(LENS, XE[:, None], ZE[:, None], xf[None, :], zf[None, :])
    assert np.isfinite(o["t"]).all()
    assert np.max(np.abs(o["t"] - ref) / ref) <= 1e-14


def bore_case():
    """points 0.5 mm above the bore of a pipe 10 mm off the lens axis, +-85 deg about its centre"""
    th = np.radians(np.linspace(-85, 85, 35))
    xf, zf = 0.01 + 0.0301 * np.sin(th), 0.0301 * np.cos(th)
    return xf, zf, O.Pipe(0.037, 0.01, 0.0), O.Pipe(0.037, 0.01, 0.0296)


def test_oracle_validity_rules():
    pipe = O.Pipe(0.037, 0.0038, 0.029)
    # rule 1 and 2 on hand-made segments: from outside / from inside the circle; clear of / through the bore
    q = pipe.q(0.0)
    assert O.qualifies(0.0038, 0.08, q[0], q[1], 0.0038, 0.033, pipe)
    assert not O.qualifies(0.0038, 0.0, q[0], q[1], 0.0038, 0.033, pipe)
    q = pipe.q(0.5)
    assert not O.qualifies(q[0], 0.08, q[0], q[1], 0.0038 - 0.031 * np.sin(1.2), 0.031 * np.cos(1.2), pipe)
    assert O.qualifies(q[0], 0.08, q[0], q[1], 0.0038 - 0.031 * np.sin(0.2), 0.031 * np.cos(0.2), pipe)
    # points outside the wall (in the bore, in the water, below the centre's depth on the far side) are NaN
    xf = np.array([0.0038, 0.0038, 0.0038 + 0.04, 0.0038])
    zf = np.array([0.01, 0.05, 0.0, 0.029])
    o = O.table(LENS, pipe, XE, ZE, xf, zf)
    assert np.isnan(o["t"]).all()
    # every finite entry's path obeys both rules; a bore that reaches up to the points occludes some paths that a solid bar allows
    # (the pipe 10 mm off the lens axis: the rays do not arrive along the radius, and the far points are reached across the wall)
    xf, zf, solid_pipe, bore_pipe = bore_case()
    solid = O.table(LENS, solid_pipe, XE, ZE, xf, zf)
    bore = O.table(LENS, bore_pipe, XE, ZE, xf, zf)
    g = np.isfinite(bore["t"])
    ie, jf = np.nonzero(g)
    px, pz, _, _ = LENS.point(bore["alpha"][g])
    qx, qz, _, _ = bore_pipe.q(bore["beta"][g])
    assert O.qualifies(px, pz, qx, qz, xf[jf], zf[jf], bore_pipe).all()
    lost = np.isfinite(solid["t"]) & ~g
    assert lost.any() and g.any()
    assert (bore["t"][g] >= solid["t"][g] * (1 - 1e-15)).all()           # a rule can only take paths away


def test_lens_clearance():
    assert 0.0767 < O.clearance(LENS, 0.0) < 0.0769
    assert 0.0692 < O.clearance(LENS, 0.01) < 0.0694 and 0.0692 < O.clearance(LENS, -0.01) < 0.0694


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def test_status_codes(rtus):
    L = rtus.lib()
    p = lambda a: a.ctypes.data                                                       # noqa: E731
    fake = C.c_void_p(256)                                                           # device pointers are never dereferenced by the checks
    lens = rtus.Params().lens()
    xe, ze, xf, zf, tt = _d([0.0]), _d([O.D]), _d([0.0038]), _d([0.033]), np.zeros(1)
    a_max = rtus.ALPHA_MAX
    for dev in (True, False):
        def pipe_call(r_outer=0.037, r_inner=0.029, x_off=0.0038, c3=5600.0, ln=lens, a_lo=-a_max, a_hi=a_max, b_lo=-np.pi / 2,
                      b_hi=np.pi / 2, n_scan=64, e=xe, n_e=1, n_f=1, out=tt, ws=fake, wsb=1 << 30, pipe=True):
            pp = C.byref(rtus.Pipe(r_outer, r_inner, x_off, c3)) if pipe else None
            lp = None if ln is None else C.byref(ln)
            args = (lp, a_lo, a_hi, pp, b_lo, b_hi, n_scan, None if e is None else p(e), p(ze), n_e, p(xf), p(zf), n_f,
                    None if out is None else p(out), None, None)
            return L.rtus_tt_pipe_dev(*args, ws, wsb, None) if dev else L.rtus_tt_pipe(*args, 0)
        assert pipe_call(ln=None) == -1 and pipe_call(pipe=False) == -1 and pipe_call(e=None) == -1 and pipe_call(out=None) == -1
        assert pipe_call(n_e=0) == -1 and pipe_call(n_f=0) == -1 and pipe_call(n_scan=3) == -1
        assert pipe_call(a_lo=0.5, a_hi=0.5) == -1 and pipe_call(a_hi=np.nan) == -1
        assert pipe_call(b_lo=0.2, b_hi=0.1) == -1 and pipe_call(b_hi=np.inf) == -1
        assert pipe_call(c3=0.0) == -1 and pipe_call(c3=-5600.0) == -1 and pipe_call(c3=np.inf) == -1 and pipe_call(c3=np.nan) == -1
        assert pipe_call(r_outer=0.0) == -1 and pipe_call(r_outer=np.nan) == -1 and pipe_call(x_off=np.nan) == -1
        assert pipe_call(r_inner=-1e-3) == -1 and pipe_call(r_inner=0.037) == -1 and pipe_call(r_inner=0.05) == -1
        assert pipe_call(r_inner=np.nan) == -1
        bad = rtus.Params(c2=np.inf).lens()
        assert pipe_call(ln=bad) == -1
        # a pipe that touches the lens: 0.07 clears it by 6.8 mm on the axis but not at a 10 mm offset (69.3 mm); 0.08 never
        assert pipe_call(r_outer=0.07, x_off=0.01, r_inner=0.0) == -1 and pipe_call(r_outer=0.07, x_off=-0.01, r_inner=0.0) == -1
        assert pipe_call(r_outer=0.08, x_off=0.0, r_inner=0.0) == -1 and pipe_call(r_outer=0.1, x_off=0.0038, r_inner=0.0) == -1
        assert pipe_call(n_scan=65537) == -5 and pipe_call(n_e=65535 * 8 + 1) == -5 and pipe_call(n_e=2048, n_scan=1 << 16) == -5
        if dev:
            assert pipe_call(ws=None) == -4 and pipe_call(wsb=16) == -4 and pipe_call(ws=C.c_void_p(257)) == -4
            assert pipe_call(r_outer=0.07, x_off=0.0, r_inner=0.0, ws=None) == -4        # accepted by every argument check
    assert L.rtus_tt_pipe_workspace_bytes(64, 466) >= 64 * 466 * 16 + 466 * 16
    assert L.rtus_tt_pipe_workspace_bytes(0, 466) == 0 and L.rtus_tt_pipe_workspace_bytes(64, 3) == 0
    assert L.rtus_tt_pipe_workspace_bytes(64, 65537) == 0


def test_python_layer_before_any_gpu_call(rtus):
    p = rtus.Params(r_outer=0.037, pipe_offset=0.0038)
    with pytest.raises(ValueError):
        rtus.travel_time_pipe([0.0, 1.0], [O.D], [0.0], [0.03], params=p)
    with pytest.raises(rtus.RtusError) as ei:
        rtus.travel_time_pipe([0.0], [O.D], [0.0], [0.03], params=rtus.Params(r_outer=0.09))
    assert ei.value.status == -1
    with pytest.raises(rtus.RtusError):
        rtus.travel_time_pipe([0.0], [O.D], [0.0], [0.03], r_inner=0.04, params=p)
    xf, zf = rtus.pipe_wall_grid(0.03, 0.036, 4, 5, -0.5, 0.5, params=p)
    assert xf.shape == (20,) and zf.shape == (20,)
    r = np.hypot(xf - 0.0038, zf).reshape(4, 5)
    th = np.arctan2(xf - 0.0038, zf).reshape(4, 5)
    assert np.allclose(r, np.linspace(0.03, 0.036, 4)[:, None]) and np.allclose(th, np.linspace(-0.5, 0.5, 5)[None, :])


def _recount(pipe, xe, ze, xf, zf, n_grid=4033):
    """every interior minimum of T(beta) of one (element, point) on a grid eight times the oracle's, each refined by plain bisection
    of T': (T, alpha, beta, rule 1, rule 2, margin of rule 2 [m]) sorted by T — O.table's detail fields, worked out one entry at a
    time in scalar arithmetic"""
    a = (-O.ALPHA_MAX, O.ALPHA_MAX)
    beta = np.linspace(-np.pi / 2, np.pi / 2, n_grid)
    d1 = O._dT(LENS, pipe, xe, ze, xf, zf, beta, *a)[0]
    found = []
    for i in np.nonzero((d1[:-1] < 0) & (d1[1:] >= 0))[0]:
        lo, hi = beta[i], beta[i + 1]
        for _ in range(100):
            mid = 0.5 * (lo + hi)
            if O._dT(LENS, pipe, xe, ze, xf, zf, mid, *a)[0] < 0:
                lo = mid
            else:
                hi = mid
        b = 0.5 * (lo + hi)
        _, T, al, px, pz, qx, qz = (float(v) for v in O._dT(LENS, pipe, xe, ze, xf, zf, b, *a))
        outside = (qx - px) * (qx - pipe.x0) + (qz - pz) * qz < 0
        # the wall segment's point nearest to the centre (pipe.x0, 0)
        sx, sz, cx, cz = xf - qx, zf - qz, qx - pipe.x0, qz
        t = min(max(-(cx * sx + cz * sz) / (sx * sx + sz * sz), 0.0), 1.0)
        near = float(np.hypot(cx + t * sx, cz + t * sz))
        found.append((T, al, b, bool(outside), near >= pipe.ri, near - pipe.ri))
    return sorted(found)


def _thin_wall_case():
    """the 10 mm pipe 3.8 mm off the axis with a 0.5 mm wall: up to three minima per entry, the earliest often through the bore"""
    pipe = O.Pipe(0.01, 0.0038, 0.0095)
    xe, ze = np.array([-0.0189, -0.0081, 0.0189]), np.full(3, O.D)          # (-8.1 mm: element 18 of the reference's 64)
    rr, th = np.meshgrid([0.0097, 0.00984], np.r_[np.linspace(-1.5, 1.5, 21), -1.1, -1.0875, -1.075], indexing="ij")
    return pipe, xe, ze, (pipe.x0 + rr * np.sin(th)).ravel(), (rr * np.cos(th)).ravel()


def test_oracle_detail_against_a_recount():
    pipe, xe, ze, xf, zf = _thin_wall_case()
    o = O.table(LENS, pipe, xe, ze, xf, zf, detail=True)
    plain = O.table(LENS, pipe, xe, ze, xf, zf)
    for k in ("t", "alpha", "beta", "flag"):
        assert np.array_equal(o[k], plain[k], equal_nan=True)
    assert set(o) == set(plain) | {"n_min", "rank", "rej1", "rej2"}
    seen = set()
    for i in range(xe.size):
        for j in range(xf.size):
            if o["flag"][i, j]:                               # (stationary points closer than a scan step: the grids may differ)
                continue
            m = _recount(pipe, xe[i], ze[i], xf[j], zf[j])
            ok = [k for k, v in enumerate(m) if v[3] and v[4]]
            rank = ok[0] if ok else -1
            early = m[:rank] if ok else m
            want = (len(m), rank, sum(not v[3] for v in early), sum(not v[4] for v in early))
            assert (o["n_min"][i, j], o["rank"][i, j], o["rej1"][i, j], o["rej2"][i, j]) == want, (i, j, want)
            if ok:
                assert abs(o["t"][i, j] - m[rank][0]) <= 1e-14 * m[rank][0] and abs(o["beta"][i, j] - m[rank][2]) <= 1e-9
            else:
                assert np.isnan(o["t"][i, j])
            seen.add(want[:2])
    # the case holds what it is for: one, two and three minima, winners of every rank, entries without a winner
    assert {(1, 0), (2, 0), (2, 1), (3, 2)} <= seen and any(r == -1 and n >= 1 for n, r in seen), sorted(seen)
    assert (~o["flag"]).mean() > 0.9


def _mp_rules(a, b, xf, zf, pipe):
    """the two validity rules at the path (alpha, beta) in mpmath -> (rule 1, rule 2, margin of rule 2)"""
    c1, c2, d = mp.mpf(O.C1), mp.mpf(O.C2), mp.mpf(O.L0) + mp.mpf(O.H0)
    Tl = mp.mpf(O.L0) / c1 + mp.mpf(O.H0) / c2
    A, Cc = c1 ** 2 / c2 ** 2 - 1, c1 ** 2 * Tl ** 2 - d ** 2
    B = 2 * d * mp.cos(a) - 2 * Tl * c1 ** 2 / c2
    h = (-B - mp.sqrt(B ** 2 - 4 * A * Cc)) / (2 * A)
    px, pz = h * mp.sin(a), h * mp.cos(a)
    cx, cz = mp.mpf(pipe.r) * mp.sin(b), mp.mpf(pipe.r) * mp.cos(b)
    qx, qz = mp.mpf(pipe.x0) + cx, cz
    sx, sz = mp.mpf(float(xf)) - qx, mp.mpf(float(zf)) - qz
    t = min(max(-(cx * sx + cz * sz) / (sx * sx + sz * sz), mp.mpf(0)), mp.mpf(1))
    near = mp.sqrt((cx + t * sx) ** 2 + (cz + t * sz) ** 2)
    return (qx - px) * cx + (qz - pz) * cz < 0, near >= mp.mpf(pipe.ri), near - mp.mpf(pipe.ri)


@pytest.mark.parametrize("case", ["third minimum", "second minimum"])
def test_oracle_selection_against_mpmath(case):
    """an entry whose earliest minima are rejected by a rule: every minimum of the entry is solved jointly in 40 digits, the rules
    are applied to the 40-digit paths, and the oracle's entry is the earliest one that qualifies there"""
    if case == "third minimum":
        pipe, xe, ze, xf, zf = _thin_wall_case()
        i, want_rank = 1, 2
        j = int(np.argmin(np.hypot(xf - (pipe.x0 + 0.00984 * np.sin(-1.0875)), zf - 0.00984 * np.cos(-1.0875))))
    else:
        pipe, xe, ze = O.Pipe(0.037, 0.01, 0.0296), XE, ZE
        xf, zf = pipe.x0 + 0.0335 * np.sin(np.array([-1.2, -0.9, 0.9, 1.2])), 0.0335 * np.cos(np.array([-1.2, -0.9, 0.9, 1.2]))
        o = O.table(LENS, pipe, xe, ze, xf, zf, detail=True)
        i, j = (int(v[0]) for v in np.nonzero((o["rank"] == 1) & ~o["flag"]))
        want_rank = 1
    o = O.table(LENS, pipe, xe, ze, xf, zf, detail=True)
    assert o["rank"][i, j] == want_rank and not o["flag"][i, j] and o["n_min"][i, j] == want_rank + 1
    minima = _recount(pipe, xe[i], ze[i], xf[j], zf[j])
    assert len(minima) == want_rank + 1
    solved = []
    for T, al, be, r1, r2, margin in minima:
        t, a, b = _mp_solve(xe[i], ze[i], xf[j], zf[j], pipe, al, be)
        assert abs(float(t) - T) <= 1e-14 * T and abs(float(a) - al) <= 1e-9 and abs(float(b) - be) <= 1e-9
        m1, m2, mm = _mp_rules(a, b, xf[j], zf[j], pipe)
        assert (bool(m1), bool(m2)) == (r1, r2) and abs(float(mm)) > 1e-6          # no rule decided by rounding
        solved.append((t, bool(m1) and bool(m2), a, b))
    solved.sort(key=lambda v: v[0])
    assert [v[1] for v in solved] == [False] * want_rank + [True]
    t, _, a, b = solved[want_rank]
    assert abs(float(t) - o["t"][i, j]) <= 1e-14 * o["t"][i, j]
    assert abs(float(a) - o["alpha"][i, j]) <= 1e-9 and abs(float(b) - o["beta"][i, j]) <= 1e-9
    assert (o["rej1"][i, j], o["rej2"][i, j]) == (0, want_rank)
    assert float(solved[want_rank][0] / solved[0][0]) - 1 > 1e-3 or want_rank == 1           # far outside any fp32 tie margin
