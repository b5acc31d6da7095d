"""No GPU: the premises of tests/test_gpu_das_exact.py, so that the GPU file cannot pass (or fail) by accident.

tests/das_exact_numpy.py claims that on its inputs no operation of the delay-and-sum family rounds.  Here that claim is checked
operation by operation: the legs are exact in fp32 (but in the columns built to round); every partial sum of every case, in three
different orders, is the fp64 sum bit for bit and needs at most 24 bits; every case reaches every edge class (the census); and
outside the columns where the fp64 oracles form another position than the header, the model IS the existing oracles, exactly.
"""
import numpy as np
import pytest

import amplitude_numpy as AN
import das_exact_numpy as D
import pwi_numpy as PW
import tfm_analytic_numpy as TA
import tfm_hmc_numpy as TH
import tfm_phase_numpy as TP
from oracle import tfm_numpy as T

FULL = list(D.FULL_CASES)
HMC = [(n_e, two) for n_e in D.HMC_SIZES for two in (False, True)]
LEG_ROUNDS = ("e8_round", "e8_mix")                     # the only columns that hold legs which are not float32 numbers
POS_ROUNDS = ("round_tie", "round_over")                # the only columns where the fp64 position is not the fp32 one


def _tables(c):
    """legs() of the two tables of a case (one table: twice the same)"""
    a = D.legs(c["tt_tx"], c["fs"], c["t0"])
    b = a if c["tt_rx"] is None else D.legs(c["tt_rx"], c["fs"], c["t0"])
    return a, b


def _cases():
    for name in FULL:
        yield name, D.full_case(name)
    for n_e, two in HMC:
        yield f"hmc{n_e}{'_two' if two else ''}", D.hmc_case(n_e, two)


def test_the_legs_are_float32_numbers_but_where_they_are_built_to_round():
    for name, c in _cases():
        for tau, ok, v in _tables(c):
            inexact = ~((tau.astype(np.float64) == v) | np.isnan(v))
            want = np.zeros(v.shape[1], dtype=bool)
            want[[c["cols"][k] for k in LEG_ROUNDS]] = True
            assert not inexact[:, ~want].any(), name
            assert inexact[:, want].any() or v.shape[0] < 2, name        # (one element takes the cycle's first value: 1e8 itself)
            # ... and there the fp64 leg is below 1e8 while its float32 is 1e8: a path in fp64, none under the header
            assert np.all(np.abs(v[inexact]) < 1e8) and np.all(np.abs(tau[inexact]) == np.float32(1e8)) and not ok[inexact].any()


def _bits(x):
    """the mantissa bits that each value of x (multiples of 1/16) needs"""
    n = np.abs(np.rint(x * 16.0)).astype(np.int64)
    assert np.array_equal(n, np.abs(x * 16.0)), "not a multiple of 1/16"
    low = n & -n
    return np.where(n > 0, np.floor(np.log2(np.maximum(n // np.maximum(low, 1), 1))) + 1, 0).astype(np.int64)


def _orders(n, seed):
    yield "ascending", np.arange(n)
    yield "descending", np.arange(n)[::-1]
    yield "shuffled", np.random.default_rng(seed).permutation(n)


def _check_sums(model, keys, name):
    """every partial sum of the float32 running sum, in three orders, is the fp64 partial sum -> the widest partial sum in bits"""
    widest = 0
    for k in keys:
        t = model[k]
        total = t.sum(axis=0)
        for what, order in _orders(t.shape[0], t.shape[0]):
            c64 = np.cumsum(t[order], axis=0)
            c32 = np.cumsum(t[order].astype(np.float32), axis=0, dtype=np.float32)     # sequential float32 additions
            assert c32.dtype == np.float32 and np.array_equal(c32.astype(np.float64), c64), (name, k, what)
            assert np.array_equal(c64[-1], total), (name, k, what)
            widest = max(widest, int(_bits(c64).max()))
    return widest


@pytest.mark.parametrize("name", FULL)
def test_full_matrix_sums_do_not_depend_on_the_order(name):
    m = D.full_model(name, terms=True)
    widest = _check_sums(m, ("t_re", "t_im", "t_e", "t_wre", "t_wim"), name)
    assert np.array_equal(m["t_re"].sum(axis=0), m["S"].real) and np.array_equal(m["t_e"].sum(axis=0), m["E"])
    assert np.array_equal(m["t_wim"].sum(axis=0), m["S_w"].imag)
    print(f"{name}: the widest partial sum needs {widest} bits")
    assert widest <= 24


@pytest.mark.parametrize("n_e,two", HMC)
def test_half_matrix_sums_do_not_depend_on_the_order(n_e, two):
    m = D.hmc_model(n_e, two, terms=True)
    widest = _check_sums(m, ("t_re", "t_im", "t_e"), (n_e, two))
    assert np.array_equal(m["t_im"].sum(axis=0), m["S"].imag) and np.array_equal(m["t_e"].sum(axis=0), m["E"])
    print(f"n_e = {n_e}, {'two tables' if two else 'one table'}: the widest partial sum needs {widest} bits")
    assert widest <= 24


def test_every_case_reaches_every_edge_class():
    """one element with one table is the exception for two classes: s = 2 tau is exact (no sum rounds) and its one leg of the
    1e8 columns is the cycle's first value (1e8 itself)"""
    for name, c in _cases():
        a, b = _tables(c)
        cen = D.census(*a, *b, c["n_t"])
        print(name, cen)
        one_leg = a[0].shape[0] == 1 and c["tt_rx"] is None
        single = a[0].shape[0] == 1 and b[0].shape[0] == 1
        for k, v in cen.items():
            if k == "s == -0.0":
                assert (v > 0) == (c["t0"] == 0.0), (name, k)            # (t0 != 0: the leg -0.0 becomes h - h = +0)
            elif one_leg and k in ("exact sum < n_t, fp32 sum == n_t", "s == -2^-23"):
                assert v == 0, (name, k)
            elif single and k in ("leg rounds onto +-1e8", "leg == +-99999992"):
                continue                                                  # (a cycle's later values need a second element)
            else:
                assert v > 0, (name, k)


def _not(cols, names, n_f):
    keep = np.ones(n_f, dtype=bool)
    keep[[cols[k] for k in names]] = False
    return keep


@pytest.mark.parametrize("name", FULL)
def test_the_model_is_the_fp64_oracles_exactly(name):
    """tfm_analytic_numpy, oracle/tfm_numpy.py (both planes), tfm_phase_numpy (fp64 and fp32 forms) and amplitude_numpy.tfm_weighted.
    The oracles that form the position in fp64 differ in the two columns built so that the fp32 sum rounds onto n_t: there the
    header (the fp32 sum: nothing) decides, and the difference is the last sample times 1 - w."""
    c, m = D.full_case(name), D.full_model(name)
    a, fs, t0, tt_tx = c["a"], c["fs"], c["t0"], c["tt_tx"]
    tt_rx = tt_tx if c["tt_rx"] is None else c["tt_rx"]
    keep = _not(c["cols"], POS_ROUNDS, D.N_F)
    o = TA.tfm_analytic(a, fs, t0, tt_tx, tt_rx)
    assert np.array_equal(o["N"], m["N"])
    assert np.array_equal(o["image"][keep], m["S"][keep]) and np.array_equal(o["E"][keep], m["E"][keep])
    if tt_tx.shape[0] > 1 or c["tt_rx"] is not None:
        assert np.all(o["image"][~keep] != m["S"][~keep])                # the fp64 position is inside the record there
    cf = D.cf_header(m["S"], m["E"], m["N"])
    assert np.array_equal(np.isnan(cf), np.isnan(o["cf"]))
    fin = keep & ~np.isnan(cf)
    assert np.all(np.abs(cf[fin] - o["cf"][fin]) <= 2.0 ** -22)          # (float32 rounding and the oracle's hypot)
    for plane, want in ((a.real, m["S"].real), (a.imag, m["S"].imag)):
        rf = T.tfm(np.ascontiguousarray(plane), fs, t0, tt_tx, tt_rx)
        assert np.array_equal(rf[keep], want[keep])
    p64 = TP.tfm_phase(a, fs, t0, tt_tx, tt_rx)
    p32 = TP.tfm_phase(a, fs, t0, tt_tx, tt_rx, fp32=True)               # the fp32 positions: every column
    assert np.array_equal(p32["N"], m["N"]) and np.array_equal(p32["B"], m["B"]) and np.array_equal(p64["N"], m["N"])
    assert np.array_equal(p64["B"][keep], m["B"][keep])
    assert np.allclose(p32["U"], m["U"], rtol=0, atol=1e-9)
    w_rx = c["w_tx"] if c["w_rx"] is None else c["w_rx"]
    S_w, P = AN.tfm_weighted(a, fs, tt_tx, c["w_tx"], tt_rx, w_rx, t0=t0)
    assert np.array_equal(S_w, m["S_w"])
    assert np.all(np.abs(P - m["P"]) <= 1e-14 * m["P"])                   # (the oracle squares a hypot: |1 + 2i|^2 = 5.000000000000001)


@pytest.mark.parametrize("n_e,two", HMC)
def test_the_half_matrix_model_is_the_fp64_oracle_exactly(n_e, two):
    c, m = D.hmc_case(n_e, two), D.hmc_model(n_e, two)
    keep = _not(c["cols"], POS_ROUNDS, D.N_F)
    o = TH.tfm_hmc(c["h"], c["fs"], c["t0"], c["tt_tx"], c["tt_rx"])
    assert np.array_equal(o["N"], m["N"])
    assert np.array_equal(o["image"][keep], m["S"][keep])
    assert np.all(np.abs(o["E"] - m["E"])[keep] <= 1e-13 * m["E"][keep])  # (the oracle squares a hypot; the full-matrix model below is exact)
    if n_e > 1 or two:
        assert np.all(o["image"][~keep] != m["S"][~keep])
    # in exact arithmetic the half matrix is the full matrix on the unpacked block: the two models agree exactly
    i, j = np.triu_indices(n_e)
    full = np.zeros((n_e, n_e, c["n_t"]), dtype=np.complex64)
    full[i, j] = c["h"]
    full[j, i] = c["h"]
    f = D.tfm(full, c["fs"], c["t0"], c["tt_tx"], c["tt_rx"])
    assert np.array_equal(f["S"], m["S"]) and np.array_equal(f["E"], m["E"]) and np.array_equal(f["N"], m["N"])


def test_whole_sample_cases_have_no_fraction():
    """the cases of the carrier-aware kernels at f_demod != 0: every position that contributes is a whole sample (w = 0)"""
    cases = [D.full_case("5x63", whole=True), D.full_case("64x64_one", whole=True)]
    cases += [D.hmc_case(n_e, two, whole=True) for n_e, two in HMC]
    for c in cases:
        (ta, oa, _), (tb, ob, _) = _tables(c)
        s, ok = D.position(ta[:, None, :], oa[:, None, :], tb[None, :, :], ob[None, :, :])
        inrec = ok & (s >= 0) & (s < c["n_t"])
        assert inrec.sum() > 100 * min(ta.shape[0], 10) and np.array_equal(s[inrec], np.floor(s[inrec]))


def test_synthesis_model_is_the_oracle_exactly():
    """the plain exact loop against tests/pwi_numpy.py's float32 emulation, on the GPU file's generator (two sizes: either side
    of the 128-transmit tile)"""
    for n_tx, n_v, n_t in ((127, 1, 255), (129, 9, 257)):
        fmc, d = D.synth_case(n_tx, n_v, n_t)
        got = D.synth(fmc, D.FS, d)
        assert got.dtype == np.float32 and np.array_equal(got, PW.synth(fmc, D.FS, d))
        cen = D.synth_census(d, n_t)
        print(n_tx, n_v, n_t, cen)
        assert all(v > 0 for k, v in cen.items() if n_tx > 128 or k != "fired in the second tile"), cen
