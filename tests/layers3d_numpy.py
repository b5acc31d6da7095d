"""NumPy definition of the matrix-array travel-time table (rtus_tt_layers3): element (xe, ye, ze) x point (xf, yf, zf) least
times through horizontal layers.

Independent of the kernel's parametrisation (which iterates on q = tan(theta) in the fastest layer, in fp32, from a lower bound):
here the unknown is the ray parameter p = sin(theta_i) / c_i itself, bracketed on [0, 1 / c_max) and bisected in fp64 until the
bracket stops shrinking, and the time is the tau-p form T = p r + sum h_i sqrt(1 - p^2 c_i^2) / c_i, which is stationary in p at
the ray: the bisection's last-bit error in p enters T squared.
"""
import numpy as np


def reach(xe, ye, xf, yf):
    """r[e, f] = sqrt(dx dx + dy dy), dx = xf - xe, dy = yf - ye"""
    dx = np.asarray(xf, dtype=np.float64)[None, :] - np.asarray(xe, dtype=np.float64)[:, None]
    dy = np.asarray(yf, dtype=np.float64)[None, :] - np.asarray(ye, dtype=np.float64)[:, None]
    return np.sqrt(dx * dx + dy * dy)


def tt_reach(z_if, c, ze, zf, r):
    """least time over lateral reach r[e, f] between depths ze[e] and zf[f]; NaN where zf <= ze or anything is not finite"""
    z_if = np.asarray(z_if, dtype=np.float64).reshape(-1)
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    ze = np.asarray(ze, dtype=np.float64)[:, None]
    zf = np.asarray(zf, dtype=np.float64)[None, :]
    r = np.asarray(r, dtype=np.float64)
    ok = (zf > ze) & np.isfinite(r) & np.isfinite(ze) & np.isfinite(zf)
    zs, zt = np.where(ok, ze, 0.0), np.where(ok, zf, 1.0)
    rr = np.where(ok, r, 0.0)
    # thickness of every layer along the path: layer i spans [edges[i], edges[i + 1]]
    edges = np.concatenate([[-np.inf], z_if, [np.inf]])
    h = np.stack([np.maximum(np.minimum(edges[i + 1], zt) - np.maximum(edges[i], zs), 0.0) for i in range(c.size)], axis=-1)
    cc = np.broadcast_to(c, h.shape)
    c_max = np.max(np.where(h > 0.0, cc, 0.0), axis=-1)

    def cosines(p):
        pc = p[..., None] * cc
        return np.sqrt(np.maximum((1.0 - pc) * (1.0 + pc), 0.0))

    def x_of(p):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = h * (p[..., None] * cc) / cosines(p)
        return np.sum(np.where(h > 0.0, t, 0.0), axis=-1)

    lo, hi = np.zeros_like(rr), 1.0 / c_max                 # X(lo) = 0 <= r < X(hi) = +inf
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        below = x_of(mid) <= rr
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    p = lo
    t = p * rr + np.sum(h * cosines(p) / cc, axis=-1)
    return np.where(ok, t, np.nan)


def tt_layers3(z_if, c, xe, ye, ze, xf, yf, zf):
    """tt[e, f]: the definition of rtus_tt_layers3"""
    return tt_reach(z_if, c, ze, zf, reach(xe, ye, xf, yf))


def skip_tt_layers3(z_if, c, z_back, xe, ye, ze, xf, yf, zf, c_up=None):
    """the skip leg off a planar backwall: the direct time on the extended stack to the mirrored depth"""
    z_if = np.asarray(z_if, dtype=np.float64).reshape(-1)
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    zf = np.asarray(zf, dtype=np.float64)
    c_up = c[-1] if c_up is None else c_up
    t = tt_layers3(np.r_[z_if, z_back], np.r_[c, c_up], xe, ye, ze, xf, yf, 2.0 * z_back - zf)
    front = z_if[-1] if z_if.size else -np.inf
    t[:, ~((zf > front) & (zf < z_back))] = np.nan
    return t
