"""CPU: the fixture of the ray-amplitude branch tests (tests/golden/amp_branches.npz) and the two NumPy oracles on it.

  * the committed fixture is what tests/golden/make_amp_branches.py makes: inputs bit for bit, 40-digit values to 1e-30 relative;
  * every class has its least number of cases, counted from the fixture's labels and from the 40-digit J, slownesses and D stored
    with the cases — never from a kernel's or an oracle's output;
  * tests/amplitude_numpy.py and tests/pipe_amplitude_numpy.py meet the mask rules (NaN, inf and == 0 masks equal to the
    reference's, every entry) and E64 <= 1e-7 per class, E64 the largest |oracle - ref| / |ref| over the class's finite, non-zero
    entries.  The table is printed; it is the one in DESIGN.md, and 16 E64 is the second term of the GPU tests' bar;
  * the forward-shot surface paths are stationary: the time along the path moves by O(h^2) under x_entry +- h (this guards the case
    builder: a path that is not a ray would still have an amplitude, and the classes would be about nothing);
  * the search for an input whose J is exactly zero in fp64 (the W == 0 branch) finds none, as DESIGN.md says."""
import os
import sys

import numpy as np
import pytest

import amp_branch_cases as B
import surface_numpy as S

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


@pytest.fixture(scope="module")
def fx():
    return B.load()


@pytest.fixture(scope="module")
def oracles(fx):
    return {"s_": B.oracle_surface(fx), "p_": B.oracle_pipe(fx)}


def _names(fx, pre):
    return [str(c) for c in fx[pre + "classes"]]


def _count(fx, pre, name, mask=None):
    m = fx[pre + "cls"] == _names(fx, pre).index(name)
    return int(np.sum(m if mask is None else m & mask))


# ---------------------------------------------------------------------------------------------- the fixture is the generator's
def test_fixture_is_reproducible(fx):
    import make_amp_branches as G
    new = G.surface_table()
    new.update(G.pipe_table())
    assert os.path.getsize(B.FIXTURE) < 256 * 1024
    for k, v in new.items():
        old = fx[k]
        assert old.shape == v.shape and old.dtype == v.dtype, k
        if k in ("s_ref", "p_ref"):
            fin = np.isfinite(v)
            assert np.array_equal(np.isnan(v), np.isnan(old)) and np.array_equal(np.isinf(v), np.isinf(old))
            assert np.all(np.abs(v[fin] - old[fin]) <= 1e-30 * np.abs(old[fin])), k
        elif v.dtype.kind == "f":
            assert np.array_equal(v.view(np.uint64), old.view(np.uint64)), k     # bit for bit, NaNs included
        else:
            assert np.array_equal(v, old), k


# ---------------------------------------------------------------------------------------------- the classes have substance
def test_class_minima_surface(fx):
    names = _names(fx, "s_")
    for name, least in B.S_MINIMA.items():
        assert name in names and _count(fx, "s_", name) >= least, (name, least)
    cl_of = np.array([B.MEDIA[m][2] for m in fx["s_med"]])
    c1_of = np.array([B.MEDIA[m][0] for m in fx["s_med"]])
    with np.errstate(invalid="ignore"):
        ds, db, d1 = np.abs(fx["s_ps"]) * cl_of - 1, np.abs(fx["s_pb"]) * cl_of - 1, np.abs(fx["s_ps"]) * c1_of - 1
    for ud in ("down", "up"):
        # critical slownesses: the side and the distance are those of the 40-digit slowness, within 1 % of each delta
        for side, sg in (("minus", -1), ("plus", 1)):
            for label, dist in ((f"crit_surf_cl_{side}_{ud}", ds), (f"crit_back_cl_{side}_{ud}", db)) + \
                    (((f"crit_surf_c1_{side}_up", d1),) if ud == "up" else ()):
                m = fx["s_cls"] == names.index(label)
                assert np.all(np.sign(dist[m]) == sg), label
                for d in B.DELTAS:
                    assert np.sum(np.abs(np.abs(dist[m]) / d - 1) < 0.01) >= 2, (label, d)
        # the tube: both signs of J, |J| down to 1e-9 m / rad on both sides, per direction
        m = fx["s_cls"] == names.index(f"tube_{ud}")
        J = fx["s_J"][m]
        assert np.sum(J > 0) >= B.TUBE_MIN_PER_SIGN and np.sum(J < 0) >= B.TUBE_MIN_PER_SIGN
        assert np.sum((J > 0) & (J < 1.1e-9)) >= 2 and np.sum((J < 0) & (J > -1.1e-9)) >= 2 and np.min(np.abs(J)) > 0.9e-9
        assert np.min(np.abs(fx["s_J"][fx["s_cls"] == names.index(f"ripple_{ud}")])) > 1e-3      # no caustic on the ripple
        # directivity: both sides of the first and the second null at each distance, u of either sign
        for label, sign in ((f"dir_null_{ud}", 1), (f"dir_null_neg_{ud}", -1)):
            m = fx["s_cls"] == names.index(label)
            u = fx["s_width"][m] * fx["s_fc"][m] / 1480.0 * (fx["s_xent"][m] - fx["s_xe"][m]) / np.hypot(fx["s_xent"][m] - fx["s_xe"][m], 0.02)
            assert np.all(np.sign(u) == sign)
            for k in (1, 2):
                for e in B.DIR_EPS:
                    for sg in (-1, 1):
                        assert np.sum(np.abs((np.abs(u) - k) / (sg * e) - 1) < 0.01) >= 1, (label, k, e, sg)
            assert np.all(np.abs(fx["s_D"][m]) < 4e-3) and np.min(np.abs(fx["s_D"][m])) > 0
        # normal incidence: p == 0 exactly, D == 1 exactly, the legs with a T in them are exactly 0
        m = fx["s_cls"] == names.index(f"normal_{ud}")
        assert np.all(fx["s_ps"][m] == 0) and np.all(fx["s_D"][m] == 1.0)
        has_t = np.isin(fx["s_leg"][m], [1, 3, 4, 5])
        assert np.all(fx["s_ref"][m][has_t] == 0) and np.all(fx["s_ref"][m][~has_t] != 0)
        # the no-ray rule: zeros on the far side of the tangent, values on the near side
        for k in ("1", "2"):
            assert np.all(fx["s_ref"][fx["s_cls"] == names.index(f"noray_{k}_neg_{ud}")] == 0)
            r = fx["s_ref"][fx["s_cls"] == names.index(f"noray_{k}_pos_{ud}")]
            assert np.all(np.isfinite(r) & (r != 0))
        assert np.all(fx["s_ref"][fx["s_cls"] == names.index(f"noray_both_{ud}")] == 0)
        for label in ("nan_entry", "nan_back"):
            assert np.all(np.isnan(fx["s_ref"][fx["s_cls"] == names.index(f"{label}_{ud}")]))
        for label in ("inf_entry", "inf_back"):      # include/rtus.h: an infinite x_entry / x_back is no point of the path: no ray
            assert np.all(fx["s_ref"][fx["s_cls"] == names.index(f"{label}_{ud}")] == 0)
    # every leg in both directions where the class applies to every leg
    for label in ("plain", "normal", "tube", "ripple", "nan_entry", "inf_entry"):
        for ud in ("down", "up"):
            assert set(fx["s_leg"][fx["s_cls"] == names.index(f"{label}_{ud}")]) == set(range(6)), label
    # the second pair: c_t < c1 < c_l; p c1 > 1 on an up leg has no transmitted ray and is NOT zeroed (include/rtus.h: the path is an
    # input and is not put to Snell's law; the coefficient is the evanescent wave's): finite, non-zero
    assert B.PERSPEX[3] < B.PERSPEX[0] < B.PERSPEX[2]
    for side in ("minus", "plus"):
        m = fx["s_cls"] == names.index(f"crit_surf_c1_{side}_up")
        assert np.all(fx["s_med"][m] == 1) and np.all(np.isfinite(fx["s_ref"][m]) & (fx["s_ref"][m] != 0))
    assert np.sum((fx["s_med"] == 1) & np.char.startswith(fx["s_classes"][fx["s_cls"]], "crit_surf_cl")) >= 24
    assert not np.isinf(fx["s_ref"]).any()              # no exact caustic among the cases (none was found: DESIGN.md)


def test_class_minima_pipe(fx):
    names = _names(fx, "p_")
    for name, least in B.P_MINIMA.items():
        assert name in names and _count(fx, "p_", name) >= least, (name, least)
    cl = B.P_MEDIA[4]
    with np.errstate(invalid="ignore"):
        dq, db = np.abs(fx["p_pq"]) * cl - 1, np.abs(fx["p_pb"]) * cl - 1
    for ud in ("down", "up"):
        for side, sg in (("minus", -1), ("plus", 1)):
            for label, dist in ((f"crit_outer_cl_{side}_{ud}", dq), (f"crit_bore_cl_{side}_{ud}", db)):
                m = fx["p_cls"] == names.index(label)
                assert np.all(np.sign(dist[m]) == sg), label
                for d in B.DELTAS:
                    assert np.sum(np.abs(np.abs(dist[m]) / d - 1) < 0.01) >= 2, (label, d)
        m = fx["p_cls"] == names.index(f"tube_{ud}")
        J = fx["p_J"][m]
        assert np.sum(J > 0) >= 8 and np.sum(J < 0) >= 8
        assert np.sum((J > 0) & (J < 3.3e-9)) >= 2 and np.sum((J < 0) & (J > -3.3e-9)) >= 2 and np.min(np.abs(J)) > 2.7e-9
        for k in "abcdef":
            assert np.all(fx["p_ref"][fx["p_cls"] == names.index(f"noray_{k}_neg_{ud}")] == 0)
            r = fx["p_ref"][fx["p_cls"] == names.index(f"noray_{k}_pos_{ud}")]
            assert np.all(np.isfinite(r) & (r != 0))
        assert np.all(fx["p_ref"][fx["p_cls"] == names.index(f"pinned_{ud}")] == 0)
        r = fx["p_ref"][fx["p_cls"] == names.index(f"pinned_inside_{ud}")]
        assert np.all(np.isfinite(r) & (r != 0))
        for k in ("alpha", "beta", "gamma"):
            assert np.all(np.isnan(fx["p_ref"][fx["p_cls"] == names.index(f"nan_{k}_{ud}")]))
    # the width on arrival at the outer circle, going down: the lens focus before the circle (W < 0) and beyond it (W > 0)
    # (no Snell path has the former: tests/amp_branch_cases.py, class 6; going up, from F, the tube class has both on its own)
    assert np.sum(fx["p_Wq"][fx["p_cls"] == names.index("tube_down")] > 0) >= 8
    assert np.sum(fx["p_Wq"][fx["p_cls"] == names.index("focus_before_outer_down")] < 0) >= 8
    m = fx["p_cls"] == names.index("tube_up")
    assert np.sum(fx["p_Wq"][m] < 0) >= 8 and np.sum(fx["p_Wq"][m] > 0) >= 8
    # every case has its mirror image, with its own reference value: |A| is kept, the sign follows the mode at F (the header's rule
    # is CHECKED on the 40-digit values here, not assumed by the GPU test)
    a, b = fx["p_mir"] == 0, fx["p_mir"] == 1
    assert a.sum() == b.sum() and np.array_equal(fx["p_alpha"][a], -fx["p_alpha"][b], equal_nan=True)
    assert np.array_equal(fx["p_xoff"][a], -fx["p_xoff"][b])
    sgn = np.where(np.isin(fx["p_leg"][a], [1, 3, 5]), -1.0, 1.0)
    ra, rb = fx["p_ref"][a], fx["p_ref"][b]
    fin = np.isfinite(ra)
    assert np.array_equal(np.isnan(ra), np.isnan(rb)) and np.all(np.abs(rb[fin] - sgn[fin] * ra[fin]) <= 1e-15 * np.abs(ra[fin]))
    assert not np.isinf(fx["p_ref"]).any()


# ---------------------------------------------------------------------------------------------- the oracles against 40 digits
@pytest.mark.parametrize("pre", ["s_", "p_"], ids=["surface", "pipe"])
def test_oracle_against_the_reference(fx, oracles, pre):
    got, ref, cls = oracles[pre], fx[pre + "ref"], fx[pre + "cls"]
    names = _names(fx, pre)
    for k, name in enumerate(names):
        m = cls == k
        assert B.masks_equal(got[m], ref[m]), f"{name}: NaN / inf / zero masks differ from the reference's"
    e64 = B.class_max(cls, B.rel_err(got, ref), len(names))
    print(f"\n{'class':30s} {'cases':>5s} {'compared':>8s} {'E64':>9s} {'stored':>9s}")
    for k, name in enumerate(names):
        m = cls == k
        print(f"{name:30s} {int(m.sum()):5d} {int(np.sum(np.isfinite(ref[m]) & (ref[m] != 0))):8d} {e64[k]:9.2e} {fx[pre + 'E64'][k]:9.2e}")
    assert np.all(e64 <= 1e-7), [n for n, e in zip(names, e64) if e > 1e-7]
    assert np.all(fx[pre + "E64"] <= 1e-7)
    # the stored figures (the GPU bar's) are these, up to what another NumPy build's rounding may move them
    assert np.all(e64 <= 4 * fx[pre + "E64"] + 1e-15) and np.all(fx[pre + "E64"] <= 4 * e64 + 1e-15)


# ---------------------------------------------------------------------------------------------- the shot paths are rays
def _path_time(coef, med, leg, xe, ze, xf, zf, x, xb):
    c1, _, cl, ct, _ = med
    sp = {"L": cl, "T": ct}
    s = S.spline_eval(coef, B.X0, B.DX, x)[0]
    t = np.hypot(x - xe, s - ze) / c1
    if len(leg) == 1:
        return t + np.hypot(xf - x, zf - s) / sp[leg]
    return t + np.hypot(xb - x, B.ZB - s) / sp[leg[0]] + np.hypot(xf - xb, zf - B.ZB) / sp[leg[1]]


def test_shot_surface_paths_are_stationary(fx):
    """T moves by O(h^2) under x_entry +- h (skip legs: under x_back +- h as well).  With C = (1 + s'^2) (1 / (c_a l_a) + 1 / (c_b l_b))
    + |s''| (1 / c_a + 1 / c_b), a bound on the second derivative of T from the two segments that meet at the moved point: each of
    T(x +- h) - T(x) is below C h^2, and their difference (twice h times the first derivative, plus a cubic term) below 1e-4 C h^2,
    at h = 0.1 um, plus 8 ulp of T for the rounding of the three times; an entry point 1e-11 m off the stationary one would fail
    this.  (Not relative to the second derivative itself: it vanishes at a caustic, and the tube class sits on caustics.)  Every
    class shot with Snell's law is covered; the paths made by hand (the no-ray rule, p c1 > 1) and the non-finite ones are not rays
    and are left out."""
    names = _names(fx, "s_")
    shot = np.array([n.split("_")[0] in ("plain", "crit", "normal", "dir", "tube", "ripple", "knots") and not n.startswith("crit_surf_c1_plus")
                     for n in names])[fx["s_cls"]]
    coefs = [S.spline(B.X0, B.DX, B.profile(k)) for k in B.PROFILES]
    h, worst, n = 1e-7, 0.0, 0
    for i in np.nonzero(shot)[0]:
        leg, med = B.LEGS[fx["s_leg"][i]], B.MEDIA[fx["s_med"][i]]
        sp = {"L": med[2], "T": med[3]}
        xe, ze, xf, zf, x, xb = (fx["s_" + k][i] for k in ("xe", "ze", "xf", "zf", "xent", "xback"))
        a = (coefs[fx["s_prof"][i]], med, leg, xe, ze, xf, zf)
        s, s1, s2 = (float(v) for v in S.spline_eval(a[0], B.X0, B.DX, np.float64(x)))
        l1 = np.hypot(x - xe, s - ze)
        if len(leg) == 1:
            l2 = np.hypot(xf - x, zf - s)
            moves = [((h, 0.0), (1 + s1 * s1) * (1 / (med[0] * l1) + 1 / (sp[leg] * l2)) + abs(s2) * (1 / med[0] + 1 / sp[leg]))]
        else:
            l2, l3 = np.hypot(xb - x, B.ZB - s), np.hypot(xf - xb, zf - B.ZB)
            moves = [((h, 0.0), (1 + s1 * s1) * (1 / (med[0] * l1) + 1 / (sp[leg[0]] * l2)) + abs(s2) * (1 / med[0] + 1 / sp[leg[0]])),
                     ((0.0, h), 1 / (sp[leg[0]] * l2) + 1 / (sp[leg[1]] * l3))]
        for (dx, db), C in moves:
            t0, tp, tm = (_path_time(*a, x + k * dx, xb + k * db) for k in (0, 1, -1))
            slack = 8 * np.finfo(np.float64).eps * t0
            assert abs(tp - t0) <= C * h * h + slack and abs(tm - t0) <= C * h * h + slack, (names[fx["s_cls"][i]], leg)
            assert abs(tp - tm) <= 1e-4 * C * h * h + slack, (names[fx["s_cls"][i]], leg, abs(tp - tm), C * h * h, slack)
            worst = max(worst, (abs(tp - tm) - slack) / (C * h * h))
            n += 1
    print("stationarity:", n, "derivatives checked, worst (odd part - rounding) / (C h^2)", worst)
    assert n >= 800


def test_no_exact_caustic_in_fp64():
    """the W == 0.0 branch: around the root of J (leg T, normal incidence under x = +3 mm of the wavy profile, zf = 24.59 mm) no zf
    within +-10^5 ulp gives J == 0.0 in the fp64 oracle — the branch stays untested rather than contrived"""
    z0, zeros, least = B.caustic_search()
    print("root of J at zf =", z0, "exact zeros:", zeros.size, "least |J|:", least)
    assert abs(z0 - 0.02459) < 1e-5 and zeros.size == 0 and least < 1e-16
