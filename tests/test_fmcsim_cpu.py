"""CPU: the FMC simulator's NumPy oracle (tests/fmcsim_numpy.py) against oracle/tfm_numpy.synth_fmc and against the per-sample
definition of include/rtus.h (scan_by_definition), the oracle's accumulate property, gaussian_pulse, the status codes of rtus_fmc_sim* (argument checks run before any HIP call: no device needed), the
ValueErrors of the Python layer and the exports."""
import numpy as np
import pytest

import fmcsim_numpy as S
from oracle import tfm_numpy as T

F0, CYCLES, FS = 5e6, 2.5, 50e6
SIGMA = CYCLES / F0 / 2.355


def _interp_bound(oversample):
    """h^2 / 8 max|p''| of linear interpolation with step h = 1 / (fs oversample), for p = g e^{i w u}, g = exp(-u^2 / (2 sigma^2)):
    p'' = (g'' + 2 i w g' - w^2 g) e^{i w u} with |g| <= 1, |g'| <= 1 / (sigma sqrt(e)), |g''| <= 1 / sigma^2"""
    h = 1.0 / (FS * oversample)
    w = 2 * np.pi * F0
    return h * h / 8.0 * (1.0 / SIGMA ** 2 + 2.0 * w / (SIGMA * np.sqrt(np.e)) + w * w)


TAIL = 1.6e-8            # the wavelet beyond 6 sigma, cut (and tapered to zero over one table step) by gaussian_pulse
F32 = 2.0 ** -24         # the table is complex64 and synth_fmc returns float32: one rounding each, of values of at most sum |amp|


@pytest.mark.parametrize("oversample", [1, 4, 16])
@pytest.mark.parametrize("n_scat", [1, 3])
def test_oracle_against_synth_fmc(rtus, oversample, n_scat):
    x_el, z_el = (np.arange(8) - 3.5) * 0.6e-3, np.zeros(8)
    scat = [(0.5e-3, 12e-3, 1.0), (-2.1e-3, 17.3e-3, 0.6), (3.3e-3, 9.1e-3, -0.8)][:n_scat]
    c, n_t, t0 = 5900.0, 451, 1.0e-6
    ref = T.synth_fmc(x_el, z_el, scat, c, FS, n_t, t0=t0, f0=F0, cycles=CYCLES).astype(np.float64)
    tt = np.stack([np.hypot(x_el - xs, z_el - zs) / c for xs, zs, _ in scat], axis=1)
    q = np.array([a for _, _, a in scat], dtype=np.complex64)
    pulse, centre = rtus.gaussian_pulse(F0, CYCLES, FS, oversample)
    got, _, sa = S.simulate(tt, tt, pulse, centre, oversample, FS, t0, n_t, q=q)
    err = float(np.abs(got.real - ref).max())
    tol = float(sa.max()) * (_interp_bound(oversample) + 2 * TAIL + 2 * F32)
    print(f"oversample {oversample}, {n_scat} scatterers: max |oracle - synth_fmc| {err:.3e}, bound {tol:.3e}")
    assert np.abs(ref).max() > 0.5 and err <= tol


@pytest.mark.parametrize("oversample", [1, 2, 3, 5, 7, 8])
def test_oracle_against_the_definition_per_sample(oversample):
    """scan() (first and last sample of an arrival, a padded table, integer division by the oversampling) against
    scan_by_definition() (none of these) with a wavelet that is not small anywhere and seven arrivals about the record's ends
    (fmcsim_numpy.edge_steps, each moved on by 0..5 table steps): the same samples touched, the values within 1e-14 max|p| sum|a|
    (fp64 sums of at most 7 terms in two groupings: some 1e-15).  And the teeth the GPU tests rely on: every arrival's own term at
    its first and at its last sample is at least 100 times the GPU tests' bound (7 + 16) 2^-23 max|p| sum|a|."""
    os_ = oversample
    rng = np.random.default_rng(400 + os_)
    worst, least, cases = 0.0, np.inf, 0
    for n_p in sorted({1, 2, os_, os_ + 1, 3 * os_ - 1, 37, 200, 2048 - os_}):
        pulse = S.random_complex(rng, n_p)
        for centre in sorted({0, n_p // 2, n_p - 1}):
            for n_t in (5, 1025, 2049, 2500):
                k = S.edge_steps(n_p, centre, os_, n_t) + rng.integers(0, 6, 7)
                if n_p + 1 < os_:                                               # a pulse shorter than a sample step: put one on a sample
                    k[4] = centre + os_ * (n_t // 2) - rng.integers(0, n_p + 1)
                tau, a = S.times_at(k, rng, FS, os_, 0.3e-6), S.random_complex(rng, 7)
                edges = []
                want, t_want, sa_want = S.scan_by_definition(tau, a, pulse, centre, os_, FS, 0.3e-6, n_t, edges=edges)
                got, t_got, sa = S.scan(tau, a, pulse, centre, os_, FS, 0.3e-6, n_t)
                label = (os_, n_p, centre, n_t)
                assert np.array_equal(t_got, t_want), label
                assert len(edges) >= 1 and abs(sa - sa_want) <= 1e-14 * sa, label
                scale = float(np.abs(pulse).max()) * sa
                worst = max(worst, float(np.abs(got - want).max()) / scale)
                least = min([least] + [min(e[3], e[4]) / (23 * 2.0 ** -23 * scale) for e in edges])
                cases += 1
    print(f"oversample {os_}: {cases} cases, max |scan - definition| / (max|p| sum|a|) {worst:.2e}, least edge term / GPU bound {least:.0f}")
    assert worst <= 1e-14 and least >= 100.0


def test_oracle_accumulate_equals_one_call(rtus):
    rng = np.random.default_rng(3)
    pulse, centre = rtus.gaussian_pulse(F0, CYCLES, FS, 4)
    tt_tx, tt_rx = rng.uniform(1e-6, 4e-6, (3, 40)), rng.uniform(1e-6, 4e-6, (2, 40))
    q = (rng.standard_normal(40) + 1j * rng.standard_normal(40)).astype(np.complex64)
    one, _, _ = S.simulate(tt_tx, tt_rx, pulse, centre, 4, FS, 0.0, 500, q=q)
    a, _, _ = S.simulate(tt_tx[:, :17], tt_rx[:, :17], pulse, centre, 4, FS, 0.0, 500, q=q[:17])
    b, _, _ = S.simulate(tt_tx[:, 17:], tt_rx[:, 17:], pulse, centre, 4, FS, 0.0, 500, q=q[17:], init=a)
    assert np.abs(one).max() > 0.5
    assert np.abs(b - one).max() <= 40 * 2.0 ** -52 * np.abs(q).sum()           # fp64 sums in another grouping
    e, _, _ = S.simulate_echo((tt_tx[:, None, :] + tt_rx[None, :, :]), np.broadcast_to(q, (3, 2, 40)), pulse, centre, 4, FS, 0.0, 500)
    assert np.array_equal(e, one)                                               # the two forms state the same arrivals


def test_oracle_drops_what_is_not_finite_and_cuts_at_the_record(rtus):
    pulse, centre = rtus.gaussian_pulse(F0, CYCLES, FS, 8)
    n_t = 200
    tau = np.array([np.nan, np.inf, -np.inf, 1e-6, 2e-6])
    a = np.array([1, 1, 1, np.nan + 0j, 1], dtype=np.complex64)
    out, touched, sa = S.scan(tau, a, pulse, centre, 8, FS, 0.0, n_t)
    only, t2, _ = S.scan(tau[4:], None, pulse, centre, 8, FS, 0.0, n_t)
    assert np.array_equal(out, only) and np.array_equal(touched, t2) and sa == 1.0 and np.isfinite(out).all()
    span = (pulse.size - 1) / 8 / 2                                             # half the pulse, in samples
    assert abs(int(touched.sum()) - (2 * span + 1)) <= 2 and abs(out[100]) == 1.0
    for t_arr, lo, hi in ((0.0, 0, span), ((n_t - 1) / FS, n_t - 1 - span, n_t - 1)):    # cut by either end of the record
        o, t, _ = S.scan([t_arr], None, pulse, centre, 8, FS, 0.0, n_t)
        idx = np.flatnonzero(t)
        assert idx[0] == int(np.ceil(lo - 1e-9)) and idx[-1] == int(np.floor(hi + 1e-9)) and np.abs(o).max() == 1.0
    for t_arr in (-2e-6, (n_t + 100) / FS):                                     # wholly outside
        o, t, s_ = S.scan([t_arr], None, pulse, centre, 8, FS, 0.0, n_t)
        assert not t.any() and not o.any() and s_ == 0.0


def test_gaussian_pulse(rtus):
    for os_ in (1, 8):
        p, c = rtus.gaussian_pulse(F0, CYCLES, FS, os_)
        assert p.dtype == np.complex64 and p.ndim == 1 and p.size == 2 * c + 1
        assert abs(p[c]) == 1.0 and p[c].imag == 0.0
        env = np.abs(p)
        assert np.array_equal(env, env[::-1]) and np.all(np.diff(env[: c + 1]) > 0)
        u = (np.arange(p.size) - c) / (FS * os_)
        assert np.abs(u).max() <= 6 * SIGMA < np.abs(u).max() + 1 / (FS * os_)
        assert np.exp(-0.5 * ((c + 1) / (FS * os_) / SIGMA) ** 2) < np.exp(-18.0) < TAIL      # the first sample left out
        ref = np.exp(-0.5 * (u / SIGMA) ** 2) * np.exp(2j * np.pi * F0 * u)
        assert np.abs(p - ref).max() <= 2.0 ** -23
        r, c2 = rtus.gaussian_pulse(F0, CYCLES, FS, os_, analytic=False)
        assert c2 == c and not r.imag.any() and np.array_equal(r.real, p.real)
    for bad in (dict(f0=0.0), dict(cycles=-1.0), dict(fs=np.inf), dict(oversample=0), dict(oversample=2.5)):
        kw = dict(f0=F0, cycles=CYCLES, fs=FS, oversample=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            rtus.gaussian_pulse(**kw)


def test_status_codes_before_any_hip_call(rtus):
    """-1 / -5 as include/rtus.h lists them, from the loaded library; the pointers are host arrays, which a call that passes its
    checks would never get to on a machine without a device"""
    L = rtus.lib()
    n_tx, n_rx, n_s, n_p, n_t = 2, 3, 5, 33, 64
    tt_tx, tt_rx = np.zeros((n_tx, n_s)), np.zeros((n_rx, n_s))
    t_pair = np.zeros((n_tx, n_rx, n_s))
    q, w = np.ones(n_s, np.complex64), np.ones((n_rx, n_s), np.complex64)
    pulse = np.ones(n_p, np.complex64)
    out = np.zeros((n_tx, n_rx, n_t), np.complex64)
    P = lambda a: None if a is None else a.ctypes.data                          # noqa: E731
    good = dict(tt_tx=P(tt_tx), tt_rx=P(tt_rx), n_tx=n_tx, n_rx=n_rx, n_s=n_s, q=P(q), w_tx=None, w_rx=P(w), pulse=P(pulse), n_p=n_p,
                centre=16, os=4, fs=50e6, t0=0.0, n_t=n_t, out=P(out), flags=0)

    def sim(dev, **kw):
        a = dict(good); a.update(kw)
        f = L.rtus_fmc_sim_dev if dev else L.rtus_fmc_sim
        return f(a["tt_tx"], a["tt_rx"], a["n_tx"], a["n_rx"], a["n_s"], a["q"], a["w_tx"], a["w_rx"], a["pulse"], a["n_p"], a["centre"],
                 a["os"], a["fs"], a["t0"], a["n_t"], a["out"], a["flags"], None if dev else 0)

    def echo(dev, **kw):
        a = dict(good, tt_tx=P(t_pair), q=P(np.ones((n_tx, n_rx, n_s), np.complex64))); a.update(kw)
        f = L.rtus_fmc_sim_echo_dev if dev else L.rtus_fmc_sim_echo
        return f(a["tt_tx"], a["q"], a["n_tx"], a["n_rx"], a["n_s"], a["pulse"], a["n_p"], a["centre"], a["os"], a["fs"], a["t0"],
                 a["n_t"], a["out"], a["flags"], None if dev else 0)

    invalid = [dict(tt_tx=None), dict(pulse=None), dict(out=None), dict(n_tx=0), dict(n_rx=-1), dict(n_s=0), dict(n_p=0), dict(n_t=0),
               dict(fs=0.0), dict(fs=-1.0), dict(fs=np.inf), dict(fs=np.nan), dict(t0=np.nan), dict(t0=np.inf), dict(os=0),
               dict(centre=-1), dict(centre=n_p), dict(flags=4), dict(flags=0x80000001), dict(q=P(q) + 4), dict(out=P(out) + 2)]
    unsupported = [dict(n_t=(1 << 26) + 1), dict(n_p=2045, os=4, centre=0), dict(n_p=2048, os=1, centre=0), dict(n_p=33, os=2016), dict(n_tx=1 << 15, n_rx=1 << 15, n_t=2048)]
    for dev in (True, False):
        for call in (sim, echo):
            for kw in invalid:
                assert call(dev, **kw) == -1, (call.__name__, dev, kw)
            for kw in unsupported:
                assert call(dev, **kw) == -5, (call.__name__, dev, kw)
        assert sim(dev, tt_rx=None) == -1


def test_python_value_errors(rtus):
    pulse, centre = rtus.gaussian_pulse(F0, CYCLES, FS, 8)
    kw = dict(fs=FS, n_t=100, pulse=pulse, centre=centre, oversample=8)
    tt = np.zeros((4, 6))
    bad_sim = [dict(tt_tx=np.zeros(6)), dict(tt_rx=np.zeros((4, 5))), dict(strength=np.ones(5)), dict(w_tx=np.ones((4, 5))),
               dict(w_rx=np.ones((3, 6))), dict(oversample=0), dict(oversample=1.5), dict(centre=-1), dict(centre=pulse.size),
               dict(n_t=0), dict(fs=0.0), dict(pulse=np.ones((2, 2))), dict(pulse=np.ones(2048), centre=0), dict(accumulate=True),
               dict(out=np.zeros((4, 4, 100), np.complex64)), dict(out=np.zeros((4, 4, 99), np.float32)),
               dict(analytic=True, out=np.zeros((4, 4, 100), np.float32))]
    for b in bad_sim:
        a = dict(kw, tt_tx=tt); a.update(b)
        with pytest.raises(ValueError):
            rtus.simulate_fmc(a.pop("tt_tx"), a.pop("tt_rx", None), **a)
    for b in (dict(t_pair=np.zeros(4)), dict(amp=np.ones((4, 5))), dict(accumulate=True), dict(oversample=0)):
        a = dict(kw, t_pair=np.zeros((4, 4))); a.update(b)
        with pytest.raises(ValueError):
            rtus.simulate_echoes(a.pop("t_pair"), a.pop("amp", None), **a)
    amps = {"L": (tt, tt)}
    for legs, views, extra in (({"L": tt}, ["L-X"], {}), ({"L": tt}, ["L"], {}), ({"L": tt}, [], {}),
                               ({"L": tt, "LT": tt}, ["L-LT"], {}),                              # receive leg LT is read as TL
                               ({"L": tt}, ["LT-L"], dict(reciprocal=False)),
                               ({"L": tt, "LT": tt}, ["LT-L"], dict(reciprocal=True)),              # its reciprocal L-LT needs TL
                               ({"L": tt, "T": tt}, ["L-T"], dict(amplitudes=amps)), ({"L": tt}, ["LL-L"], {})):
        with pytest.raises(ValueError):
            rtus.simulate_views(legs, views, **dict(kw, **extra))
    with pytest.raises(TypeError):
        rtus.simulate_fmc(tt)                                                   # the wavelet and the record are required keywords


def test_exports_and_version(rtus):
    import re
    import os
    for name in ("gaussian_pulse", "simulate_fmc", "simulate_echoes", "simulate_views"):
        assert name in rtus.__all__ and callable(getattr(rtus, name))
    for name in ("rtus_fmc_sim_dev", "rtus_fmc_sim", "rtus_fmc_sim_echo_dev", "rtus_fmc_sim_echo"):
        assert name in rtus.EXPORTS and hasattr(rtus.lib(), name)
    assert rtus.lib().rtus_version() >= 114
    from importlib import import_module
    api = import_module("ray-tracing-ultrasound_amd.api")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtus.h")).read()
    val = lambda name: int(re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+)u" % name, hdr).group(1), 16)    # noqa: E731
    assert api.SIM_ANALYTIC == val("RTUS_SIM_ANALYTIC") and api.SIM_ACCUMULATE == val("RTUS_SIM_ACCUMULATE")
