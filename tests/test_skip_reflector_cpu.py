"""CPU: the oracle of the skip legs off a sampled backwall (tests/skip_reflector_numpy.py) against the mirror image of a flat and of a
tilted backwall in one medium and against itself at a finer sampling of a wavy one; the rules of rtus_skip_reflector's definition on
hand-made rows; reflector_mask and backwall_profile on hand-made inputs; and the plumbing of the new entries: exports, version, status
codes through ctypes, Python errors raised before any library call, the kernel's resources from the code object's metadata.
No GPU touched."""
import os

import numpy as np
import pytest

import skip_reflector_numpy as SK
from conftest import ROOT

CL, CT = 5900.0, 3230.0
XE = (np.arange(16) - 7.5) * 0.6e-3
SPAN, DEPTH = 0.020, 0.030
XF, ZF = (v.ravel() for v in np.meshgrid(np.linspace(-0.008, 0.008, 17), np.linspace(0.006, 0.026, 21)))


def _down(xb, zb):
    return np.hypot(XE[:, None] - xb[None, :], zb[None, :]) / CL


def _line(n_p, tilt):
    xb = np.linspace(-SPAN, SPAN, n_p)
    return xb, DEPTH + xb * np.tan(tilt)


def _mirror(tilt):
    """element -> the focal point's mirror image in the line z = DEPTH + x tan(tilt)"""
    n = np.asarray([-np.sin(tilt), np.cos(tilt)])                      # the line's unit normal; the line passes through (0, DEPTH)
    d = XF * n[0] + (ZF - DEPTH) * n[1]
    xm, zm = XF - 2.0 * d * n[0], ZF - 2.0 * d * n[1]
    return np.hypot(XE[:, None] - xm[None, :], zm[None, :]) / CL


@pytest.mark.parametrize("tilt_deg", [0.0, 5.0])
def test_flat_and_tilted_backwall_against_the_mirror_image(tilt_deg):
    """max error at 41 / 81 / 161 points (1, 0.5, 0.25 mm).  Measured flat: 4.3e-10, 6.3e-11, 7.3e-12 s; tilted by 5 degrees:
    7.2e-10, 7.3e-11, 1.0e-11 s — third order in the spacing (8x per halving is the order; 6.7x to 9.9x measured, depending on where
    the bounce points fall between samples; asserted as >= 4x)"""
    tilt = np.deg2rad(tilt_deg)
    ref = _mirror(tilt)
    err = []
    for n_p in (41, 81, 161):
        xb, zb = _line(n_p, tilt)
        t, pos, n_min = SK.skip(_down(xb, zb), xb, zb, CL, XF, ZF)
        assert t.shape == (16, XF.size) and np.isfinite(t).all() and np.all(n_min == 1)
        err.append(float(np.max(np.abs(t - ref))))
    print(f"tilt {tilt_deg} deg: max |dt| at 41 / 81 / 161 points:", err)
    assert err[2] <= 2e-11
    assert all(a >= 4.0 * b for a, b in zip(err[:-1], err[1:])), err


def test_wavy_backwall_converges_and_has_competing_bounces():
    """30 mm + 0.5 mm sin(2 pi x / 20 mm): 161 points against 1281 (measured 1.2e-11 s with L up, 1.3e-11 s with T up); every entry
    finite; some entries see two interior minima"""
    wavy = lambda xb: DEPTH + 0.0005 * np.sin(2 * np.pi * xb / 0.020)      # noqa: E731
    twos = 0
    for c_up in (CL, CT):
        out = []
        for n_p in (161, 1281):
            xb = np.linspace(-SPAN, SPAN, n_p)
            out.append(SK.skip(_down(xb, wavy(xb)), xb, wavy(xb), c_up, XF, ZF))
        assert np.isfinite(out[0][0]).all() and np.isfinite(out[1][0]).all()
        err = float(np.max(np.abs(out[0][0] - out[1][0])))
        two = int((out[0][2] == 2).sum())
        print(f"c_up {c_up}: 161 against 1281 points max |dt| = {err:.3e} s; n_min == 2 in {two} of {out[0][2].size} entries")
        assert err <= 5e-11
        twos += two
    assert twos > 0


def _one(row):
    """a hand-made row of sums: every reflector point one unit from the focal point at unit speed, so S_j = (row_j - 1) + 1 exactly"""
    row = np.asarray(row, dtype=np.float64)
    t, pos, n_min = SK.skip((row - 1.0)[None, :], np.zeros(row.size), np.ones(row.size), 1.0, [0.0], [0.0])
    return float(t[0, 0]), float(pos[0, 0]), int(n_min[0, 0])


def test_rules_of_the_definition():
    nan, inf = np.nan, np.inf
    t, pos, n = _one([1.0, 2.0, 3.0, 4.0])                     # the minimum at the first point
    assert np.isnan(t) and pos == 0.0 and n == 0
    t, pos, n = _one([4.0, 3.0, 2.0, 1.0])                     # ... at the last
    assert np.isnan(t) and pos == 3.0 and n == 0
    t, pos, n = _one([5.0, nan, 1.0, 2.0, 3.0])                # a NaN neighbour
    assert np.isnan(t) and pos == 2.0 and n == 0
    t, pos, n = _one([5.0, 2.0, 1.0, inf, 3.0])                # an infinite one is not finite either
    assert np.isnan(t) and pos == 2.0 and n == 0
    t, pos, n = _one([-inf, 2.0, 1.0, 2.0, 3.0])               # -inf is not a least FINITE sum
    assert t == 1.0 and pos == 2.0 and n == 1
    t, pos, n = _one([3.0, 1.0, 1.0, 3.0])                     # a tie goes to the first index; neither point is a strict minimum
    assert pos == 1.5 and n == 0 and t == 1.0 - (0.25 * 2.0) * 0.5
    t, pos, n = _one([nan, nan, nan])                          # nothing finite
    assert np.isnan(t) and np.isnan(pos) and n == 0
    t, pos, n = _one([3.0, 1.0, 2.0])                          # a = 3, b = 1, c = 2: d1 = 1, d2 = 3, delta = 1/6
    assert t == 1.0 - 0.25 * (0.5 / 3.0) and pos == 1.0 + 0.5 / 3.0 and n == 1
    for row, p in (([7.0], 0.0), ([2.0, 1.0], 1.0), ([1.0, 2.0], 0.0), ([1.0, 1.0], 0.0)):     # n_p = 1, 2: never bracketed
        t, pos, n = _one(row)
        assert np.isnan(t) and pos == p and n == 0
    t, pos, n = _one([5.0, 2.0, 4.0, 1.0, 3.0, nan, 0.5, 0.25, 6.0])      # three dips, the last the deepest
    assert n == 3 and pos > 6.5
    # a coordinate that is not finite makes its own sum not finite, nothing else
    down = np.asarray([[3.0, 1.0, 2.0, 0.0]])
    t, pos, n = SK.skip(down, [0.0, 0.0, 0.0, np.nan], [1.0, 1.0, 1.0, 1.0], 1.0, [0.0, np.inf], [0.0, 0.0])
    assert t[0, 0] == 2.0 - 0.25 * (0.5 / 3.0) and n[0, 0] == 1 and np.isnan(t[0, 1]) and np.isnan(pos[0, 1])
    # the up leg is sqrt(dx dx + dz dz) / c, not hypot: one value where the two differ
    xb, zb = np.asarray([0.1, 0.3, 0.7]), np.asarray([0.9, 1.1, 1.3])
    u = SK.up_table(xb, zb, 3.0, [0.05], [0.2])
    dx, dz = 0.05 - xb, 0.2 - zb
    assert np.array_equal(u[0], np.sqrt(dx * dx + dz * dz) / 3.0)


def test_reflector_mask(rtus):
    xb, zb = np.asarray([0.0, 1.0, 3.0]), np.asarray([1.0, 1.0, 2.0])
    xf = np.asarray([0.0, 3.0, -1e-12, 3.0 + 1e-9, 2.0, 2.0, 2.0, 1.0, np.nan, 0.5])
    zf = np.asarray([0.5, 1.9, 0.5, 0.5, 1.5, 1.5 - 1e-9, 1.6, 1.0, 0.0, np.nan])
    want = [True, True, False, False, False, True, False, False, False, False]      # the ends count; ON the polyline does not
    assert list(rtus.reflector_mask(xb, zb, xf, zf)) == want
    assert list(SK.reflector_mask(xb, zb, xf, zf)) == want
    rng = np.random.default_rng(3)
    xr, zr = np.sort(rng.uniform(-1, 1, 9)), rng.uniform(1, 2, 9)
    px, pz = rng.uniform(-1.2, 1.2, 400), rng.uniform(0.8, 2.2, 400)
    assert np.array_equal(rtus.reflector_mask(xr, zr, px, pz), SK.reflector_mask(xr, zr, px, pz))
    for bad in (([0.0, 0.0, 1.0], [1.0, 1.0, 1.0]), ([0.0, 2.0, 1.0], [1.0, 1.0, 1.0]), ([0.0], [1.0]), ([0.0, 1.0], [1.0])):
        with pytest.raises(ValueError):
            rtus.reflector_mask(*bad, [0.0], [0.0])


def test_backwall_profile(rtus):
    n_x, n_z, x0, dx, z_lo, dz = 9, 40, -0.004, 1e-3, 0.020, 0.25e-3
    depth = 0.0251 + 0.0004 * np.arange(n_x)                              # between pixels
    z = z_lo + dz * np.arange(n_z)
    img = np.exp(-0.5 * ((z[None, :] - depth[:, None]) / 0.6e-3) ** 2)
    img[:, 2] = 3.0                                                       # a stronger echo above z_min (the front's ringing)
    img[4] *= 0.05                                                        # a dim column: filled from its neighbours
    img[8] = np.linspace(0.0, 1.0, n_z)                                   # brightest at the last pixel: no peak inside the window
    img[0, 4] = 2.0                                                       # brightest at the first allowed pixel
    r = rtus.backwall_profile(img, x0, dx, z_lo, dz, z_min=0.021)
    o = SK.backwall_profile(img, x0, dx, z_lo, dz, z_min=0.021)
    assert sorted(r) == ["amplitude", "dx", "valid", "x0", "z_peak", "zs"]
    assert list(r["valid"]) == [False, True, True, True, False, True, True, True, False]
    assert np.isnan(r["z_peak"][0]) and np.isnan(r["z_peak"][8]) and np.isfinite(r["z_peak"][4])
    assert r["x0"] == x0 + dx and r["dx"] == dx and r["zs"].shape == (7,)
    for k in ("zs", "z_peak", "amplitude", "valid"):
        assert np.allclose(r[k], o[k], rtol=0, atol=1e-15, equal_nan=True), k
    # a Gaussian sampled at a quarter of its width: the parabola is within a few per cent of a pixel
    ok = r["valid"]
    assert np.max(np.abs(r["z_peak"][ok] - depth[ok])) < 0.05 * dz
    assert abs(r["zs"][3] - 0.5 * (r["zs"][2] + r["zs"][4])) < 1e-15                # the dim column, interpolated
    assert r["amplitude"][0] == 2.0 and r["amplitude"][8] == 1.0
    # without z_min the ringing wins everywhere: every peak at pixel 2, refined between its neighbours
    top = rtus.backwall_profile(img, x0, dx, z_lo, dz)
    assert np.all(np.abs(top["z_peak"][1:8] - (z_lo + 2 * dz)) < 0.5 * dz)
    with pytest.raises(ValueError):
        rtus.backwall_profile(img, x0, dx, z_lo, dz, z_min=z[-2])         # two pixels left
    with pytest.raises(ValueError):
        rtus.backwall_profile(img[0], x0, dx, z_lo, dz)
    with pytest.raises(ValueError):
        rtus.backwall_profile(np.linspace(0, 1, n_z)[None, :].repeat(5, 0), x0, dx, z_lo, dz)       # no column has a peak


def test_exports_version_and_status_codes(rtus):
    L = rtus.lib()
    assert L.rtus_version() >= 117
    for name in ("rtus_skip_reflector", "rtus_skip_reflector_dev"):
        assert name in rtus.EXPORTS and hasattr(L, name)
    for name in ("skip_travel_time_reflector", "reflector_mask", "skip_travel_time_layers_profile", "skip_travel_time_surface_profile",
                 "view_legs_layers_profile", "view_legs_surface_profile", "backwall_profile"):
        assert name in rtus.__all__ and callable(getattr(rtus, name))
    from importlib import import_module
    assert callable(import_module("ray-tracing-ultrasound_amd.device").skip_reflector_dev)
    buf = np.zeros(64)
    p = buf.ctypes.data
    base = dict(td=p, n_e=2, xb=p, zb=p, n_p=3, c=5900.0, xf=p, zf=p, n_f=4, tt=p)

    def call(dev, **kw):
        a = {**base, **kw}
        args = (a["td"], a["n_e"], a["xb"], a["zb"], a["n_p"], a["c"], a["xf"], a["zf"], a["n_f"], a["tt"], None, None)
        return L.rtus_skip_reflector_dev(*args, None) if dev else L.rtus_skip_reflector(*args, 0)
    for dev in (False, True):
        for name in ("td", "xb", "zb", "xf", "zf", "tt"):
            assert call(dev, **{name: None}) == -1, name
        for name in ("n_e", "n_p", "n_f"):
            assert call(dev, **{name: 0}) == -1 and call(dev, **{name: -3}) == -1, name
        for c in (0.0, -5900.0, np.inf, -np.inf, np.nan):
            assert call(dev, c=c) == -1, c
        assert call(dev, n_e=1 << 16, n_f=1 << 15) == -5                   # n_e n_f = 2^31
        assert call(dev, n_e=1 << 16, n_f=1 << 16) == -5
        assert call(dev, n_e=1 << 16, n_f=1 << 16, tt=None) == -1          # invalid before unsupported
        assert call(dev, n_e=1 << 16, n_f=1 << 16, c=0.0) == -1


def test_python_wrapper_validation(rtus, monkeypatch):
    from importlib import import_module
    api = import_module("ray-tracing-ultrasound_amd.api")

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(api._lib, "lib", no_library)
    xb, zb = np.linspace(-0.01, 0.01, 5), np.full(5, 0.03)
    xe, ze, xf, zf = np.zeros(4), np.zeros(4), np.zeros(3), np.full(3, 0.02)
    td = np.zeros((4, 5))
    good = dict(tt_down=td, xb=xb, zb=zb, c_up=CL, xf=xf, zf=zf)
    for kw in (dict(tt_down=td[0]), dict(tt_down=np.zeros((4, 6))), dict(tt_down=np.zeros((0, 5))), dict(zb=zb[:4]), dict(xf=xf[:2]),
               dict(xf=np.zeros(0), zf=np.zeros(0)), dict(c_up=0.0), dict(c_up=-1.0), dict(c_up=np.nan), dict(c_up=np.inf),
               dict(out=np.zeros((4, 2))), dict(out=np.zeros((4, 3), dtype=np.float32))):
        with pytest.raises(ValueError):
            rtus.skip_travel_time_reflector(**{**good, **kw})
    z_if, c = [0.01], [1480.0, CL]
    lay = lambda **kw: rtus.skip_travel_time_layers_profile(**{**dict(z_if=z_if, c=c, xb=xb, zb=zb, xe=xe, ze=ze, xf=xf, zf=zf), **kw})      # noqa: E731
    for kw in (dict(zb=np.r_[zb[:4], 0.01]), dict(zb=np.r_[zb[:4], 0.009]), dict(xb=xb[::-1].copy()), dict(c=[1480.0]), dict(zf=zf[:2]),
               dict(z_if=0.001 * np.arange(1, 10), c=np.full(10, 1480.0))):
        with pytest.raises(ValueError):
            lay(**kw)
    zs = np.full(21, 0.01)
    sur = lambda **kw: rtus.skip_travel_time_surface_profile(**{**dict(x0=-0.01, dx=1e-3, zs=zs, c1=1480.0, c2=CL, xb=xb, zb=zb, xe=xe,      # noqa: E731
                                                                  ze=ze, xf=xf, zf=zf), **kw})
    for kw in (dict(x0=-0.009), dict(x0=-0.011), dict(zb=np.r_[zb[:4], 0.01]), dict(xb=np.r_[xb[:4], xb[3]]), dict(zs=zs[:1]),
               dict(zf=zf[:2])):
        with pytest.raises(ValueError):
            sur(**kw)
    with pytest.raises(ValueError):
        rtus.view_legs_layers_profile(z_if, [1480.0], CL, CT, xb, zb, xe, ze, xf, zf, legs=("LL", "XX"))
    with pytest.raises(ValueError):
        rtus.view_legs_layers_profile(z_if, [1480.0, 1.0], CL, CT, xb, zb, xe, ze, xf, zf)
    with pytest.raises(ValueError):
        rtus.view_legs_layers_profile(z_if, [1480.0], CL, CT, xb, np.r_[zb[:4], 0.01], xe, ze, xf, zf)
    with pytest.raises(ValueError):
        rtus.view_legs_surface_profile(-0.009, 1e-3, zs, 1480.0, CL, CT, xb, zb, xe, ze, xf, zf)
    with pytest.raises(ValueError):
        rtus.view_legs_surface_profile(-0.01, 1e-3, zs, 1480.0, CL, CT, xb, zb, xe, ze, xf, zf, legs=("LX",))


def test_kernel_resources_of_the_skip_reflector_kernel():
    """rtus_skip_reflector.hip compiled device-only to assembly with the Makefile's flags: both instances (with and without
    n_min's bookkeeping) have no scratch, no spilled register, at most 128 VGPRs (four waves per SIMD; 38 and 36 here) and the tile
    of 32 points x 64 focal points in LDS (16,384 bytes).  Metadata only."""
    import re
    import subprocess
    import tempfile
    csrc = os.path.join(ROOT, "ray-tracing-ultrasound_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    keys = (".vgpr_count:", ".vgpr_spill_count:", ".sgpr_spill_count:", ".private_segment_fixed_size:", ".group_segment_fixed_size:")
    kernels = []
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "rtus_skip_reflector.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, "rtus_skip_reflector.hip"), "-o", out],
                       check=True, capture_output=True, timeout=600)
        meta = open(out).read().split("amdhsa.kernels:")[1]
        for entry in re.split(r"\n  - \.", meta)[1:]:                     # one entry per kernel; its keys in any order
            v = {}
            for ln in ("." + entry).splitlines():
                ln = ln.strip().lstrip("- ")
                for key in keys + (".name:",):
                    if ln.startswith(key):
                        v[key] = ln.split()[1]
            kernels.append(v)
    print(kernels)
    assert len(kernels) == 2 and all("rtus_skip_reflector_kernel" in v[".name:"] for v in kernels), kernels
    for v in kernels:
        assert all(key in v for key in keys), v
        assert int(v[".private_segment_fixed_size:"]) == 0 and int(v[".vgpr_spill_count:"]) == 0 and int(v[".sgpr_spill_count:"]) == 0, v
        assert int(v[".vgpr_count:"]) <= 128, v
        assert int(v[".group_segment_fixed_size:"]) == 32 * 64 * 8, v
