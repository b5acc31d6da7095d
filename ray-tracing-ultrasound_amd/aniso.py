"""Anisotropic parts (austenitic weld metal, cladding, carbon-fibre laminates): travel times where the speed depends on the ray's
direction (rtus_tt_aniso_surface, rtus_tt_aniso_direct; include/rtus.h), and the host side that turns elastic constants into what
the kernels take — the GROUP SLOWNESS over the ray angle as a Fourier series of period pi,

    S(psi) = a[0] + sum_{k=1..K} (a[k] cos 2k psi + b[k] sin 2k psi),   K <= 16,

psi from the +z axis (depth), positive towards +x.  The helpers are NumPy and run no kernel:

    psi, s = group_slowness_ti(C11, C13, C33, C55, rho, "qP")      # Christoffel: one plane of a transversely isotropic medium
    a, b, residual = fit_group_slowness(psi, s, 16, tilt=grain_angle)
    tt = travel_time_surface_aniso(x0, dx, zs, c1, (a, b), xe, ze, xf, zf)      # feeds any beamformer as it is

Not in the reference."""
import numpy as np

from . import _lib
from .api import _f64, _out, _points, _ptr

K_MAX = 16          # harmonics the kernels take (include/rtus.h)


def _series(slowness):
    """``slowness`` = (a, b) -> float64 vectors of one length K + 1 >= 1 (what the C layer reads from the host pointers); the
    series itself (K <= 16, finite, positive) is the C layer's to refuse"""
    try:
        a, b = slowness
    except (TypeError, ValueError):
        raise ValueError("slowness must be a pair (a, b) of equal-length float64 vectors") from None
    a, b = _f64(a, "slowness a"), _f64(b, "slowness b")
    if a.shape != b.shape or a.size < 1:
        raise ValueError("slowness must be a pair (a, b) of equal-length float64 vectors, K + 1 >= 1 coefficients each")
    return a, b, a.size - 1


def travel_time_surface_aniso(x0, dx, zs, c1, slowness, xe, ze, xf, zf, *, return_entry=False, out=None, device=0):
    """Element x focal-point Fermat travel times through ONE curved interface into an ANISOTROPIC part -> tt[n_e, n_f].

    travel_time_surface with the part's speed replaced by its group slowness over the ray angle, ``slowness`` = (a, b), the
    series S(psi) = a[0] + sum_k (a[k] cos 2k psi + b[k] sin 2k psi), K = len(a) - 1 <= 16, psi the ray's angle from +z (down),
    positive towards +x (fit_group_slowness, elliptical_slowness make one; ``([1 / c2], [0])`` is the isotropic part).  An entry is
    the least travel time over the interior local minima of T(x) = |E - S(x)|/c1 + |F - S(x)| S(psi(x)) and NaN without one, for
    an element not strictly above the whole profile, or for a focal point outside the extent or not below the surface.  Occlusion
    is not checked.  ``return_entry``: also the x of the winning entry point, -> (tt, x_entry).  ``out``: optional float64
    [n_e, n_f] result buffer.  RtusError (status -1) for K > 16, a coefficient that is not finite or a series that is not positive.
    The table feeds focal_delays / tfm_image / simulate_fmc as it is.  Definition and guarantee: include/rtus.h
    (rtus_tt_aniso_surface).

    NOT in the reference: parity unpinned, see DESIGN.md.
    """
    zs = _f64(zs, "zs")
    a, b, K = _series(slowness)
    xe, ze, xf, zf = _points(xe, ze, xf, zf)
    tt = _out(out, (xe.size, xf.size), np.float64)
    xn = np.empty((xe.size, xf.size), dtype=np.float64) if return_entry else None
    st = _lib.lib().rtus_tt_aniso_surface(float(x0), float(dx), _ptr(zs), zs.size, float(c1), _ptr(a), _ptr(b), K, _ptr(xe), _ptr(ze),
                                          xe.size, _ptr(xf), _ptr(zf), xf.size, _ptr(tt), _ptr(xn), int(device))
    _lib.check(st, "rtus_tt_aniso_surface")
    return (tt, xn) if return_entry else tt


def travel_time_aniso(slowness, xe, ze, xf, zf, *, out=None, device=0):
    """Element x point travel times INSIDE an anisotropic part, the probe in contact (no couplant path) -> tt[n_e, n_f]:
    tt = |F - E| S(psi), psi the direction from the element to the point, ``slowness`` = (a, b) as in travel_time_surface_aniso.
    Any relative position is accepted (S has period pi); 0 at zero distance; NaN for a non-finite coordinate.  ``out``: optional
    float64 [n_e, n_f] result buffer.  Definition: include/rtus.h (rtus_tt_aniso_direct).  Not in the reference."""
    a, b, K = _series(slowness)
    xe, ze, xf, zf = _points(xe, ze, xf, zf)
    tt = _out(out, (xe.size, xf.size), np.float64)
    st = _lib.lib().rtus_tt_aniso_direct(_ptr(a), _ptr(b), K, _ptr(xe), _ptr(ze), xe.size, _ptr(xf), _ptr(zf), xf.size, _ptr(tt),
                                         int(device))
    _lib.check(st, "rtus_tt_aniso_direct")
    return tt


# ---------------------------------------------------------------------------------------------------- host side, NumPy only
def eval_group_slowness(a, b, psi):
    """S(psi) of the series (a, b) at the angles ``psi`` [rad] -> array of psi's shape"""
    a, b = _f64(a, "a"), _f64(b, "b")
    if a.shape != b.shape or a.size < 1:
        raise ValueError("a and b must have one length, K + 1 >= 1")
    psi = np.asarray(psi, dtype=np.float64)
    k = np.arange(1, a.size).reshape((-1,) + (1,) * psi.ndim)
    shp = (-1,) + (1,) * psi.ndim
    return a[0] + np.sum(a[1:].reshape(shp) * np.cos(2 * k * psi) + b[1:].reshape(shp) * np.sin(2 * k * psi), axis=0)


def group_slowness_ti(C11, C13, C33, C55, rho, mode="qP", *, C66=None, n=4096):
    """Group slowness of a transversely isotropic medium in a plane through its symmetry axis (the axis along z), from the
    Christoffel equation -> (psi [n], s [n]): the group (ray) angle from the axis and the group slowness 1 / V_g there, for the
    phase angles theta_i = i pi / n.  Elastic constants in Pa, ``rho`` in kg/m^3; ``mode`` "qP", "qSV" or "SH" (SH needs ``C66``).

    Phase velocity: 2 rho v^2 = C11 sin^2 + C33 cos^2 + C55 +- sqrt(((C11 - C55) sin^2 - (C33 - C55) cos^2)^2 + 4 (C13 + C55)^2
    sin^2 cos^2) (+ qP, - qSV); rho v^2 = C66 sin^2 + C55 cos^2 (SH).  psi = theta + atan(v' / v), V_g = sqrt(v^2 + v'^2), v'
    analytic.  ValueError where psi(theta) is not strictly increasing: the wave surface has cusps (qSV in weld metal) and no series
    in the ray angle gives one time per direction."""
    if mode not in ("qP", "qSV", "SH"):
        raise ValueError('mode must be "qP", "qSV" or "SH"')
    if int(n) < 8:
        raise ValueError("n must be at least 8")
    th = np.pi * np.arange(int(n)) / int(n)
    s2, c2, sin2, cos2 = np.sin(th) ** 2, np.cos(th) ** 2, np.sin(2 * th), np.cos(2 * th)
    if mode == "SH":
        if C66 is None:
            raise ValueError("the SH mode needs C66")
        W = (C66 * s2 + C55 * c2) / rho                          # v^2
        dW = (C66 - C55) * sin2 / rho
    else:
        P = C11 * s2 + C33 * c2 + C55
        M = (C11 - C55) * s2 - (C33 - C55) * c2
        g = (C13 + C55) ** 2
        D = M * M + g * sin2 * sin2
        dD = 2 * M * (C11 + C33 - 2 * C55) * sin2 + 4 * g * sin2 * cos2
        if not np.all(D > 0):
            raise ValueError("degenerate constants: the qP and qSV sheets touch")
        r = np.sqrt(D)
        sg = 1.0 if mode == "qP" else -1.0
        W = (P + sg * r) / (2 * rho)
        dW = ((C11 - C33) * sin2 + sg * dD / (2 * r)) / (2 * rho)
    if not np.all(W > 0):
        raise ValueError("the constants give no real phase velocity")
    v = np.sqrt(W)
    dv = dW / (2 * v)
    psi = th + np.arctan(dv / v)
    if not (np.all(np.diff(psi) > 0) and psi[0] + np.pi > psi[-1]):
        raise ValueError(f"the group angle is not increasing in the phase angle: the {mode} wave surface has cusps")
    return psi, 1.0 / np.sqrt(v * v + dv * dv)


def _fit_uniform(s, K, tilt):
    """the series of samples s_j = S0(j pi / N), rotated by ``tilt`` -> (a, b, residual)"""
    K = int(K)
    N = s.size
    if not 0 <= K <= K_MAX:
        raise ValueError(f"K must be 0 .. {K_MAX}")
    if N < 2 * K + 2:
        raise ValueError("too few samples for K harmonics")
    F = np.fft.rfft(s) / N
    a0 = np.r_[F[0].real, 2 * F[1:K + 1].real]
    b0 = np.r_[0.0, -2 * F[1:K + 1].imag]
    u = np.pi * np.arange(N) / N
    residual = float(np.max(np.abs(eval_group_slowness(a0, b0, u) - s) / s))
    k = np.arange(K + 1)
    c, sn = np.cos(2 * k * tilt), np.sin(2 * k * tilt)
    return a0 * c - b0 * sn, a0 * sn + b0 * c, residual


def fit_group_slowness(psi, s, K, *, tilt=0.0):
    """The series of a sampled group slowness -> (a [K + 1], b [K + 1], residual).  ``psi`` [rad] strictly increasing over one
    period (less than pi from first to last; group_slowness_ti's), ``s`` > 0 the slowness there.  The samples are resampled
    (linearly, with period pi) to the uniform grid j pi / N, N = len(psi), and transformed; the coefficients up to K are kept.
    ``tilt`` [rad]: the grain orientation, S(psi) = S0(psi - tilt) — each (a_k, b_k) rotated by 2 k tilt.  ``residual``: the
    largest relative misfit of the series on the grid; choose K by it."""
    psi, s = _f64(psi, "psi"), _f64(s, "s")
    if psi.shape != s.shape or psi.size < 8:
        raise ValueError("psi and s must have one length, at least 8")
    if not (np.all(np.diff(psi) > 0) and psi[-1] - psi[0] < np.pi):
        raise ValueError("psi must be strictly increasing and span less than pi")
    if not (np.all(np.isfinite(s)) and np.all(s > 0)):
        raise ValueError("s must be finite and positive")
    u = np.pi * np.arange(psi.size) / psi.size
    return _fit_uniform(np.interp(u, psi, s, period=np.pi), K, float(tilt))


def elliptical_slowness(v_x, v_z, K=12, *, tilt=0.0):
    """The elliptical medium — group velocity v_x along x, v_z along z, S = sqrt(sin^2 psi / v_x^2 + cos^2 psi / v_z^2) — as a
    series -> (a, b), the ``slowness`` of travel_time_surface_aniso.  ``tilt`` [rad] rotates the ellipse's z axis towards +x.
    (The series of an ellipse converges geometrically: 6100 / 5300 m/s is at rounding with K = 12.)"""
    if not (np.isfinite(v_x) and np.isfinite(v_z) and v_x > 0 and v_z > 0):
        raise ValueError("v_x and v_z must be positive")
    u = np.pi * np.arange(4096) / 4096
    a, b, _ = _fit_uniform(np.sqrt((np.sin(u) / v_x) ** 2 + (np.cos(u) / v_z) ** 2), K, float(tilt))
    return a, b
