"""Plain NumPy restatement of the skip legs off a sampled backwall (include/rtus.h: rtus_skip_reflector): the table of up legs
U[f, j] in the header's order of operations, then tests/specular_numpy.py's reduction — so the kernel's results are these bits.  Plus
NumPy twins of api.reflector_mask and api.backwall_profile, written as loops over the points and columns.  Nothing here touches the
GPU.  The oracle of tests/test_skip_reflector_cpu.py and tests/test_gpu_skip_reflector.py."""
import numpy as np

import specular_numpy as SP


def up_table(xb, zb, c_up, xf, zf):
    """U [n_f, n_p]: dx = xf - xb, dz = zf - zb, r2 = dx dx + dz dz, sqrt, / c_up — every operation rounded on its own"""
    xb, zb, xf, zf = (np.asarray(v, dtype=np.float64) for v in (xb, zb, xf, zf))
    with np.errstate(all="ignore"):
        dx = xf[:, None] - xb[None, :]
        dz = zf[:, None] - zb[None, :]
        r2 = dx * dx + dz * dz
        return np.sqrt(r2) / np.float64(c_up)


def skip(tt_down, xb, zb, c_up, xf, zf):
    """-> (tt, pos float64, n_min int32), each [n_e, n_f]"""
    t, pos, n_min = SP.specular(tt_down, up_table(xb, zb, c_up, xf, zf))
    return t[0], pos[0], n_min[0]


def reflector_mask(xb, zb, xf, zf):
    """True where xb[0] <= xf <= xb[-1] and the point lies strictly above the polyline (z down)"""
    xb, zb = np.asarray(xb, dtype=np.float64), np.asarray(zb, dtype=np.float64)
    out = np.zeros(len(xf), dtype=bool)
    for f, (x, z) in enumerate(zip(xf, zf)):
        if not (xb[0] <= x <= xb[-1]):
            continue
        k = min(int(np.searchsorted(xb, x, side="right")) - 1, len(xb) - 2)
        w = (x - xb[k]) / (xb[k + 1] - xb[k])
        out[f] = z < zb[k] + w * (zb[k + 1] - zb[k])
    return out


def backwall_profile(image, x0, dx, z_lo, dz, z_min=None, threshold=0.1):
    """per column: the brightest pixel at a depth >= z_min, the three-point parabola on the amplitudes, NaN at the window's edges;
    then valid = finite and amplitude >= threshold * max, trim to the valid span, fill by linear interpolation in x"""
    img = np.asarray(image, dtype=np.float64)
    n_x, n_z = img.shape
    j_min = 0
    if z_min is not None:
        while z_lo + j_min * dz < z_min - 1e-9 * dz:
            j_min += 1
    z_peak, amp = np.full(n_x, np.nan), np.zeros(n_x)
    for k in range(n_x):
        j = j_min + int(np.argmax(img[k, j_min:]))
        amp[k] = img[k, j]
        if j == j_min or j == n_z - 1:
            continue
        a, b, c = img[k, j - 1], img[k, j], img[k, j + 1]
        den = (a - b) + (c - b)
        z_peak[k] = z_lo + (j + (0.5 * (a - c) / den if den != 0 else 0.0)) * dz
    valid = np.isfinite(z_peak) & (amp >= threshold * amp.max())
    idx = np.nonzero(valid)[0]
    lo, hi = int(idx[0]), int(idx[-1])
    zs = np.asarray([z_peak[k] if valid[k] else np.interp(x0 + k * dx, x0 + idx * dx, z_peak[idx]) for k in range(lo, hi + 1)])
    return dict(x0=x0 + lo * dx, dx=dx, zs=zs, valid=valid, z_peak=z_peak, amplitude=amp)
