"""CPU: the NumPy definition of the matrix-array travel-time table (tests/layers3d_numpy.py) against the long-double oracle of the
planar problem called per element at the pair's lateral reach, the array / grid helpers' orderings, and the wrappers' argument
checks (raised before the library is touched: none of this needs a GPU)."""
import os
import re

import numpy as np
import pytest

import layers3d_numpy as N
from layers3d_cases import C_FAST_SLOW, C_SLOW_FAST, Z_IF2, oracle_table, small_case

TOL = 1e-13          # tests/test_gpu_fermat_layers.py's: |dt| in seconds


def test_numpy_definition_matches_the_oracle_per_element():
    xe, ye, ze, xf, yf, zf = small_case()
    assert xe.size == 12 and xf.size == 9 * 7 * 5
    for c in (C_SLOW_FAST, C_FAST_SLOW):
        ref = oracle_table(Z_IF2, c, xe, ye, ze, xf, yf, zf)
        tt = N.tt_layers3(Z_IF2, c, xe, ye, ze, xf, yf, zf)
        nan = zf[None, :] <= ze[:, None]
        assert nan.sum() == 63
        assert np.array_equal(np.isnan(tt), nan) and np.array_equal(np.isnan(ref), nan)
        err = float(np.max(np.abs(tt - ref)[~nan]))
        print("layers3d_numpy vs oracle: max |dt| = %.3g s" % err)
        assert err < TOL


def test_numpy_definition_closed_forms():
    xe, ye, ze, xf, yf, zf = small_case()
    ok = zf[None, :] > ze[:, None]
    d = np.sqrt((xf[None, :] - xe[:, None]) ** 2 + (yf[None, :] - ye[:, None]) ** 2 + (zf[None, :] - ze[:, None]) ** 2)
    tt = N.tt_layers3(Z_IF2, [1500.0] * 3, xe, ye, ze, xf, yf, zf)
    assert np.max(np.abs(tt - d / 1500.0)[ok]) < 1e-15
    t = N.tt_layers3([0.01, 0.03], [1000.0, 2000.0, 4000.0], [0.002], [-0.001], [0.0], [0.002], [-0.001], [0.05])
    assert abs(t[0, 0] - (0.01 / 1000 + 0.02 / 2000 + 0.02 / 4000)) < 1e-18


def test_matrix_array_and_volume_grid_orderings(rtus):
    xe, ye, ze = rtus.matrix_array(4, 3, 1.5e-3, 2e-3, z=0.002)
    assert xe.shape == ye.shape == ze.shape == (12,) and xe.dtype == ye.dtype == ze.dtype == np.float64
    assert np.array_equal(xe.reshape(3, 4), np.tile((np.arange(4) - 1.5) * 1.5e-3, (3, 1)))       # x fastest
    assert np.array_equal(ye.reshape(3, 4), np.tile(((np.arange(3) - 1.0) * 2e-3)[:, None], (1, 4)))
    assert np.all(ze == 0.002)
    assert xe.sum() == 0.0 and ye.sum() == 0.0                                                    # centred
    x1, y1, z1 = rtus.matrix_array(8, 8, 1.5e-3)
    assert np.array_equal(np.unique(y1), np.unique(x1)) and np.all(z1 == 0.0)                    # pitch_y defaults to pitch_x
    assert np.array_equal(x1[:8], (np.arange(8) - 3.5) * 1.5e-3) and np.all(y1[:8] == y1[0])
    with pytest.raises(ValueError):
        rtus.matrix_array(0, 3, 1e-3)

    xs, ys, zs = np.array([-1.0, 0.0, 1.0, 2.0]), np.array([10.0, 20.0, 30.0]), np.array([100.0, 200.0])
    xf, yf, zf, shape = rtus.volume_grid(xs, ys, zs)
    assert shape == (2, 3, 4) and xf.shape == yf.shape == zf.shape == (24,)
    for v in (xf, yf, zf):
        assert v.dtype == np.float64 and v.flags.c_contiguous
    assert np.array_equal(xf[:4], xs) and np.all(yf[:4] == 10.0) and np.all(zf[:12] == 100.0)   # x fastest, then y, then z
    img = (xf + yf + zf).reshape(shape)
    assert img[1, 2, 3] == 2.0 + 30.0 + 200.0 and img[0, 1, 0] == -1.0 + 20.0 + 100.0
    flat = np.ravel_multi_index((1, 2, 3), shape)
    assert (xf[flat], yf[flat], zf[flat]) == (2.0, 30.0, 200.0)
    with pytest.raises(ValueError):
        rtus.volume_grid(np.zeros((2, 2)), ys, zs)


def test_wrappers_refuse_bad_arguments_before_the_library(rtus, monkeypatch):
    from importlib import import_module
    lib_mod = import_module("ray-tracing-ultrasound_amd._lib")

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(lib_mod, "lib", no_library)
    e3, f5 = np.zeros(3), np.ones(5)
    ok = dict(xe=e3, ye=e3, ze=e3, xf=f5, yf=f5, zf=f5)
    for name in ok:                                                  # each of the six vectors, one value short
        a = dict(ok)
        a[name] = a[name][:-1]
        with pytest.raises(ValueError):
            rtus.travel_time_layers_3d([0.01], [1500.0, 3000.0], **a)
        with pytest.raises(ValueError):
            rtus.skip_travel_time_layers_3d([0.01], [1500.0, 3000.0], 0.03, **a)
        with pytest.raises(ValueError):
            rtus.view_legs_layers_3d([0.01], [1500.0], 5900.0, 3200.0, 0.03, **a)
    with pytest.raises(ValueError):
        rtus.travel_time_layers_3d([0.01], [1500.0], **ok)                                        # len(c) != len(z_if) + 1
    with pytest.raises(ValueError):
        rtus.travel_time_layers_3d([0.01], [1500.0, 3000.0], **dict(ok, xe=np.zeros((3, 1)), ye=np.zeros((3, 1)), ze=np.zeros((3, 1))))
    with pytest.raises(ValueError):
        rtus.travel_time_layers_3d([0.01], [1500.0, 3000.0], out=np.empty((3, 5), dtype=np.float32), **ok)
    with pytest.raises(ValueError):
        rtus.travel_time_layers_3d([0.01], [1500.0, 3000.0], out=np.empty((5, 3)), **ok)
    with pytest.raises(ValueError):
        rtus.skip_travel_time_layers_3d([0.01], [1500.0, 3000.0], 0.005, **ok)                   # backwall above the interface
    with pytest.raises(ValueError):
        rtus.skip_travel_time_layers_3d(np.arange(1, 9) * 1e-3, [1500.0] * 9, 0.03, **ok)        # no room for the backwall
    with pytest.raises(ValueError):
        rtus.view_legs_layers_3d([0.01], [1500.0], 5900.0, 3200.0, 0.03, legs=("L", "XX"), **ok)
    with pytest.raises(ValueError):
        rtus.view_legs_layers_3d([0.01], [1500.0, 1600.0], 5900.0, 3200.0, 0.03, **ok)


def test_tile_constants_mirror_the_header(rtus):
    from importlib import import_module
    api = import_module("ray-tracing-ultrasound_amd.api")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtus.h")).read()
    val = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))
    assert api.LAYERS3_POINTS == val("RTUS_TT_LAYERS3_POINTS") and api.LAYERS3_ROWS == val("RTUS_TT_LAYERS3_ROWS")
    assert rtus.lib().rtus_version() >= 126
