"""The input sets of the skip-leg branch tests (tests/test_pipe_skip_branches_cpu.py, tests/test_gpu_pipe_skip_branches.py): the
places where rtus_tt_pipe_skip decides something that tests/test_gpu_pipe_skip.py's sets never reach - entries with two qualifying
minima of T(beta), the general-trigonometry instantiation, brackets in the first and the last scan cell and on the 64-point tile
seam, windows without (or with only part of) an arc of the bore, points micrometres off the two circles, bad inputs, small windows.

Plain data and helpers, no GPU and no random numbers.  A case is geometry, leg, elements, points, alpha interval, window and
n_scan, with the share of entries the oracle may flag; what the case must hold ON THE ORACLE (tests/pipe_skip_numpy.py, ``detail``)
is asserted by conditions() and the per-kind helpers below, by the CPU test always and by the GPU test before it compares anything.
The oracle's output is computed once per case and process (oracle(): cached) and must not be written to."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import pipe_numpy as O
import pipe_skip_numpy as S
from test_gpu_pipe_branches import HB, SCAN_PAIRS, _scan_cases, _wall_grid
from test_pipe_skip_cpu import CL, CT, LEGS, XE64, ZE64

LENS = O.Lens()
XE8, ZE8 = XE64[::9], ZE64[::9]
CAP = 2e-3                  # tests/test_gpu_pipe_skip.py's FLAG_CAP
CAP_TWO = 0.01              # the two-minima sets (the oracle alone: at most 0.0058)
WIDE = 1.05                 # alpha interval of the general-trigonometry sets
PIPE37 = (0.037, 0.0038, 0.029)

Case = namedtuple("Case", "name ro off ri leg xe ze xf zf a_lo a_hi b_lo b_hi n_scan cap")
CASES = {}


def _add(name, geom, leg, xf, zf, *, a=O.ALPHA_MAX, b_lo=-np.pi / 2, b_hi=np.pi / 2, n_scan=None, cap=CAP, xe=XE8, ze=ZE8):
    ro, off, ri = geom
    CASES[name] = Case(name, ro, off, ri, leg, xe, ze, np.asarray(xf), np.asarray(zf), -a, a, b_lo, b_hi, n_scan, cap)
    return CASES[name]


def pipe(c):
    return O.Pipe(c.ro, c.off, c.ri, LEGS[c.leg][0])


def run_oracle(c, **kw):
    with np.errstate(all="ignore"):
        return S.table(LENS, pipe(c), LEGS[c.leg][1], c.xe, c.ze, c.xf, c.zf, a_lo=c.a_lo, a_hi=c.a_hi, b_lo=c.b_lo, b_hi=c.b_hi,
                       n_scan=c.n_scan, detail=True, **kw)


@lru_cache(maxsize=None)
def oracle(name):
    return run_oracle(CASES[name])


def kernel_kw(rtus, c):
    """skip_travel_time_pipe's keywords for the case"""
    cd, cu = LEGS[c.leg]
    return dict(c_down=cd, c_up=cu, r_inner=c.ri, params=rtus.Params(r_outer=c.ro, pipe_offset=c.off), alpha_lo=c.a_lo, alpha_hi=c.a_hi,
                beta_lo=c.b_lo, beta_hi=c.b_hi, n_scan=c.n_scan)


def conditions(c, o):
    """what every set must hold: the flag cap; at most two interior minima and no rule-1 rejection (the day an input reaches the
    third bracket or a rejected minimum this says so); one minimum of the inner problem at most"""
    label = c.name
    assert o["flag"].mean() <= c.cap, (label, float(o["flag"].mean()))
    assert o["n_min"].max() <= 2, (label, int(o["n_min"].max()))
    assert o["rej1"].sum() == 0, (label, int(o["rej1"].sum()))
    assert o["n_gamma"].max() <= 1, (label, int(o["n_gamma"].max()))


# ---------------------------------------------------------------------------------------------- two qualifying minima
# r_outer, offset, bore; 6 radii x 61 angles over +-1.5 rad, 0.1 mm off the circles, the default scan (127 / 466 points).  The
# oracle's figures (unflagged two-minima entries / of them won by the later beta / flagged share):
#   mid10 LL 59 / 59 / 0, mid10 TT 58 / 22 / 0.0014, thick37 TT 36 / 20 / 0
TWO_GEOMS = {"mid10": (0.01, 0.0038, 0.006), "thick37": (0.037, 0.0038, 0.015)}
TWO_MINIMA = {"mid10 LL": 30, "mid10 TT": 30, "thick37 TT": 20}          # the least count of unflagged two-minima entries
for _n in TWO_MINIMA:
    _g, _leg = _n.split()
    _ro, _off, _ri = TWO_GEOMS[_g]
    _add(_n, TWO_GEOMS[_g], _leg, *_wall_grid(_off, _ri, _ro, 6, 61), cap=CAP_TWO)
# The kernel's scan orders the kept brackets by an fp32 estimate of T (T at the scan point right of the minimum) and the refine
# loop takes them in that order; in the three sets above the winner is ranked FIRST in every two-minima entry (second_bracket(): 0),
# so there the "a later bracket wins" update of the refine loop never runs.  Over all 64 elements the mid10 TT grid holds two
# entries, (element 1, point 206) and (element 6, point 203), whose minima are 3e-6 t apart and whose estimates rank the winner
# second (by 4e-7 and 1e-6 t, several fp32 ulps): the first 8 elements x the points 200 .. 207 hold both
_x, _z = _wall_grid(0.0038, 0.006, 0.01, 6, 61)
RANKED_SECOND = _add("mid10 TT ranked second", TWO_GEOMS["mid10"], "TT", _x[200:208], _z[200:208], cap=CAP_TWO, xe=XE64[:8], ze=ZE64[:8])
TWO_MINIMA[RANKED_SECOND.name] = 2
RANKED_SECOND_MIN = 2       # the least count of two-minima winners that the scan (fp64 model) ranks second in that set


def two_minima(o):
    """the unflagged entries with two interior minima, both with a finite time and past rule 1 -> dict of arrays over them: idx
    (flat index into the table), beta / gamma / t of the winner (w_*) and of the other minimum (u_*), later (the winner is the
    later beta)"""
    m = o["minima"]
    sel = ((o["n_min"] == 2) & ~o["flag"] & np.isfinite(o["t"])).ravel()
    r = {k: [] for k in ("idx", "w_beta", "w_gamma", "w_t", "u_beta", "u_gamma", "u_t")}
    for p in np.nonzero(sel)[0]:
        k = np.nonzero(m["entry"] == p)[0]
        assert k.size == 2
        if not (np.isfinite(m["t"][k]).all() and m["rule1"][k].all()):
            continue
        w, u = (k[0], k[1]) if m["beta"][k[0]] == o["beta"].ravel()[p] else (k[1], k[0])
        assert m["beta"][w] == o["beta"].ravel()[p] and m["t"][w] <= m["t"][u]
        r["idx"].append(p)
        for key, src in (("beta", "beta"), ("gamma", "gamma"), ("t", "t")):
            r["w_" + key].append(m[src][w])
            r["u_" + key].append(m[src][u])
    r = {k: np.asarray(v, dtype=np.intp if k == "idx" else np.float64) for k, v in r.items()}
    r["later"] = r["w_beta"] > r["u_beta"]
    return r


def second_bracket(c, tw):
    """how many of the winners tw (two_minima's) the kernel's scan ranks SECOND: it orders the kept brackets by T at the scan point
    right of each minimum (fp32 there, fp64 here: a model, for printing only)"""
    hb = (c.b_hi - c.b_lo) / ((O.default_n_scan(c.ro, c.b_lo, c.b_hi) if c.n_scan is None else c.n_scan) - 1)
    ie, jf = np.unravel_index(tw["idx"], (c.xe.size, c.xf.size))
    est = []
    for b in (tw["w_beta"], tw["u_beta"]):
        bj = c.b_lo + np.ceil((b - c.b_lo) / hb) * hb
        est.append(S._dT(LENS, pipe(c), LEGS[c.leg][1], c.xe[ie], c.ze[ie], c.xf[jf], c.zf[jf], bj, c.a_lo, c.a_hi)[1])
    return int(np.sum(est[0] > est[1]))


# ---------------------------------------------------------------------------------------------- general trigonometry
# alpha_lo, alpha_hi = -+1.05 rad: past +-1 the kernels run their sincos instantiation.  5 radii x 41 angles over +-1.2 rad; the
# oracle: flagged 0, all 1,640 entries finite, 462 (LL) / 463 (LT) winners past ALPHA_MAX
for _leg in ("LL", "LT"):
    _add("wide " + _leg, PIPE37, _leg, *_wall_grid(0.0038, 0.029, 0.037, 5, 41, -1.2, 1.2), a=WIDE)
    _add("wide-default " + _leg, PIPE37, _leg, *_wall_grid(0.0038, 0.029, 0.037, 5, 41, -1.2, 1.2))

# ---------------------------------------------------------------------------------------------- thin shells
# 61 points over +-0.6 rad on each of three shells: 1 um and 30 um above the bore (the fp32 scan's dF = r_F - r_inner and a_F =
# arccos(r_inner / r_F) get small), 30 um under the outer surface.  The oracle (LL, LT): all finite, none flagged, none grazing
SHELLS = (("bore + 1 um", 0.029 + 1e-6), ("bore + 30 um", 0.029 + 30e-6), ("outer - 30 um", 0.037 - 30e-6))
_th = np.linspace(-0.6, 0.6, 61)
for _leg in ("LL", "LT", "TL"):
    _add("thin " + _leg, PIPE37, _leg, np.concatenate([0.0038 + r * np.sin(_th) for _, r in SHELLS]),
         np.concatenate([r * np.cos(_th) for _, r in SHELLS]))

# ---------------------------------------------------------------------------------------------- windows and arcs
# 16 points at 33 mm, angles -1.2 .. -0.9 rad.  A beta shares an arc of the bore with a point when |beta - theta_F| < arccos(ri / ro)
# + arccos(ri / r_F) = 0.670 + 0.498: under the window 0.6 .. 1.4 none does.  Widened downwards in three steps the window holds W
# on part of the scan only, at its upper end (no winner where the minimum still lies below the window: 16, then 51, of the 128
# entries have one), then every point's minimum.  The mirrored points under windows that begin at -1.4 and are widened upwards
# hold the betas without W at the START of the scan (0, 72, 128 winners)
_th = np.linspace(-1.2, -0.9, 16)
ARC_WINDOWS = (0.6, -0.8, -0.9, -1.3)                        # beta_lo; beta_hi = 1.4
ARC_WINDOWS_UP = (-0.6, 0.85, 0.9, 1.3)                      # beta_hi; beta_lo = -1.4, the points at +0.9 .. +1.2 rad
for _b in ARC_WINDOWS:
    _add(f"arc {_b}", PIPE37, "LL", 0.0038 + 0.033 * np.sin(_th), 0.033 * np.cos(_th), b_lo=_b, b_hi=1.4)
for _b in ARC_WINDOWS_UP:
    _add(f"arc up {_b}", PIPE37, "LL", 0.0038 + 0.033 * np.sin(-_th), 0.033 * np.cos(_th), b_lo=-1.4, b_hi=_b)


# ---------------------------------------------------------------------------------------------- scan edges
@lru_cache(maxsize=None)
def scan_cases(leg):
    """tests/test_gpu_pipe_branches.py's scan cases for the skip leg: per (element, point) pair of SCAN_PAIRS the window is placed
    so that the oracle's winning beta b0 (default window) lies at the fraction fr of scan cell c -> list of (Case, ed, m, c, fr, b0);
    a case with c outside 0 .. n - 2 has its minimum one cell outside the window"""
    ro, off, ri = PIPE37
    out = []
    for ed, rf, th in SCAN_PAIRS:
        xf, zf = off + rf * np.sin(th + np.array([-0.02, 0.0, 0.02])), rf * np.cos(th + np.array([-0.02, 0.0, 0.02]))
        b0 = run_oracle(_add(f"scan {leg} pair {ed}", PIPE37, leg, xf, zf))["beta"][ed, 1]
        assert np.isfinite(b0)
        for m, c, fr in _scan_cases():
            hb, n = (0.999 / 148, 149) if m is None else (HB, m)
            b_lo = b0 - (c + fr) * hb
            b_hi = b_lo + (n - 1) * hb
            if m is None:
                assert O.default_n_scan(ro, b_lo, b_hi) == n
            out.append((_add(f"scan {leg} pair {ed} n {m} cell {c} at {fr}", PIPE37, leg, xf, zf, b_lo=b_lo, b_hi=b_hi, n_scan=m),
                        ed, m, c, fr, b0))
    return out


SCAN_SEEN = {(65, 63), (129, 63), (129, 127), (149, 63), (149, 127), (4, 0), (4, 2), (4, None), (149, None)}
# the cases whose condition the CPU test asserts (all of them are asserted on the GPU): n_scan 4 cells 0 and 2, 65 cell 63, 129
# cells 63 (fraction 1 - 2e-6), 64 (2e-6) and 127, and the minimum one cell outside either end
SCAN_CPU = {(4, 0, 0.03), (4, 2, 0.97), (65, 63, 0.5), (129, 63, 1 - 2e-6), (129, 64, 2e-6), (129, 127, 0.97), (4, -1, 0.97), (4, 3, 0.03)}


def scan_condition(case, o, ed, m, c, fr, b0):
    """the chosen entry's winner is in cell c (NaN when c is outside the window) -> (n, inside)"""
    n = 149 if m is None else m
    inside = 0 <= c <= n - 2
    if inside:
        hb = (case.b_hi - case.b_lo) / (n - 1)
        assert abs(o["beta"][ed, 1] - b0) <= 1e-12 and int(np.floor((o["beta"][ed, 1] - case.b_lo) / hb)) == c, case.name
    else:
        assert np.isnan(o["t"][ed, 1]), case.name
    return n, inside


# ---------------------------------------------------------------------------------------------- bad inputs, small windows
EDGE = _add("edge LT", PIPE37, "LT", *_wall_grid(0.0038, 0.029, 0.037, 5, 21, -0.45, 0.45))
BAD_X = np.array([np.nan, 0.0038, np.inf, 0.0038, 0.0038, 0.0038, 0.0038, 0.0038])
BAD_Z = np.array([0.033, -np.inf, 0.033, 0.029, 0.037, 0.0, -0.029, -0.037])       # ..., exactly r_inner, r_outer, the centre, ...
BAD_AT = np.array([0, 1, 50, 63, 64, 65, 104, 105])                                  # slots of the untouched grid to insert before

SHAPES = {n: _add(f"shapes n_scan {n}", PIPE37, "LT", *_wall_grid(0.0038, 0.029, 0.037, 1, 257, -0.3, 0.3, margin=3e-3), b_lo=-0.6,
                  b_hi=0.6, n_scan=n, xe=XE64[5::6][:9], ze=ZE64[:9]) for n in (4, 64, 65)}
