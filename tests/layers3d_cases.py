"""Shared inputs of the matrix-array travel-time tests (test_layers3d_cpu.py, test_gpu_layers3d.py)."""
import numpy as np

Z_IF2, C_SLOW_FAST, C_FAST_SLOW = [0.010, 0.025], [1480.0, 3200.0, 5900.0], [5900.0, 3200.0, 1480.0]


def small_case():
    """4 x 3 elements x 9 x 7 x 5 points.  Element 2 sits 1 mm below the array's plane, element 7 below the first interface at the
    depth of the first plane of points: its 63 entries there are the NaN entries of the table (zf <= ze)."""
    ix, iy = np.meshgrid(np.arange(4), np.arange(3))
    xe, ye = (ix.ravel() - 1.5) * 1.1e-3, (iy.ravel() - 1.0) * 1.3e-3
    ze = np.zeros(12)
    ze[2], ze[7] = 0.001, 0.012
    zs, ys, xs = np.linspace(0.012, 0.040, 5), np.linspace(-0.009, 0.012, 7), np.linspace(-0.02, 0.016, 9)
    Z, Y, X = np.meshgrid(zs, ys, xs, indexing="ij")
    return xe, ye, ze, X.ravel(), Y.ravel(), Z.ravel()


def oracle_table(z_if, c, xe, ye, ze, xf, yf, zf):
    """The long-double oracle of the planar problem, per element, at the pair's lateral reach."""
    from oracle import cport
    from layers3d_numpy import reach
    r = reach(xe, ye, xf, yf)
    return np.stack([cport.tt_layers(z_if, c, [0.0], [ze[e]], r[e], zf)[0] for e in range(len(xe))])
