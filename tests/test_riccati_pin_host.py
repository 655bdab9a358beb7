"""CPU: the pin of the Riccati backward sweep (tests/_rictwin.py) on the host emulator, and what entitles the twin to judge.

  * The host form of the sweep (hb_riccati.hpp compiled for the host: tests/host_emu/hostemu.cpp emu_riccati_gains, the same record
    packing, NaN records behind the horizons and sentinel as hb_riccati_gains) through check() on all twelve cases.
  * The long-double reference against mpmath at 40 digits, on every case (case 10 is bit for bit the data of case 3 and shares its
    run): in each of check()'s four figures the reference lies within a thousandth of the bound it is used for.
  * The self-test: check() must fail, by name, on one entry of K~ moved by 16 x its bound, on one padded gain row set to 1e-300, on
    the sentinel of one slot behind a horizon overwritten, and on the width sequence of case 3 shifted by one stage in what the code
    under test is fed.  The same shift on case 2, whose stages are all 12 wide, must pass: a uniform-width problem cannot show a width
    that is taken from the neighbouring stage.  That is why case 3 exists."""
import ctypes as C

import numpy as np
import pytest

import _rictwin as tw


@pytest.fixture(scope="module")
def emu():
    import _hostemu
    return C.CDLL(str(_hostemu.build()))


def run_emu(lib, args):
    args = [np.ascontiguousarray(a) for a in args]
    n = args[0].shape[0]
    K, k, fail = np.zeros((n, tw.NMAX, 12, 22)), np.zeros((n, tw.NMAX, 12)), np.zeros(n, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = lib.emu_riccati_gains(C.c_int32(tw.B), C.c_int32(tw.NMAX), C.c_int32(n), *(p(a) for a in args), p(K), p(k), p(fail))
    assert rc == 0
    return K, k, fail


@pytest.fixture(scope="module")
def host_gains(emu):
    out = run_emu(emu, tw.arrays())
    for a in out:
        a.setflags(write=False)
    return out


def test_host_sweep_meets_every_check_on_all_twelve_cases(host_gains):
    ratios = tw.check(*host_gains, "host emulator")
    print("worst ratio per case:", " ".join(f"{v:.2f}" for v in ratios.max(axis=1)))


def test_long_double_reference_against_mpmath_at_40_digits():
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 40
    def to_mp(a):   # exact: a long double is the sum of two doubles
        a = np.asarray(a, dtype=tw.LD)
        hi = a.astype(np.float64)
        lo = (a - hi.astype(tw.LD)).astype(np.float64)
        return np.array([mp.mpf(float(h)) + mp.mpf(float(l)) for h, l in zip(hi.ravel(), lo.ravel())], dtype=object).reshape(a.shape)
    ref, bnd = tw.reference(), tw.bounds()
    for i, stages in enumerate(tw.cases()):
        if i == 10:
            continue
        rec = tw.recursion(stages, to_mp, lambda H, rhs: tw.solve_cholesky_loops(H, rhs, sqrt=mp.sqrt), tw._stop(i))
        worst = np.zeros(4)
        for k, r in ref[i]["stages"].items():
            exact = {key: rec[k][key] for key in ("K", "k", "Huu", "Hux", "hu")}
            # the figures of check(), the reference in the place of the code under test and mpmath in the place of the reference
            d = [float(max(abs(v) for v in (to_mp(r[key]) - exact[key]).ravel()) / max(mp.mpf(1), max(abs(v) for v in exact[key].ravel()))) for key in ("K", "k")]
            ninf = lambda m: max(sum(abs(v) for v in row) for row in m) if m.ndim == 2 else max(abs(v) for v in m)   # noqa: E731
            Kl, kl = to_mp(r["K"]), to_mp(r["k"])
            d.append(float(ninf(exact["Huu"] @ Kl + exact["Hux"]) / (ninf(exact["Huu"]) * ninf(Kl) + ninf(exact["Hux"]))))
            d.append(float(ninf(exact["Huu"] @ kl + exact["hu"]) / (ninf(exact["Huu"]) * ninf(kl) + ninf(exact["hu"]))))
            worst = np.maximum(worst, d)
        print(f"case {i:2d}: long double against mpmath {worst}, as a fraction of the bounds {worst / bnd[i]}")
        assert (worst <= 1e-3 * bnd[i]).all(), f"case {i}: the long-double reference is {worst / bnd[i]} of the bounds away from mpmath"


def test_check_fails_by_name_on_each_planted_defect(emu, host_gains):
    K, k, fail = (a.copy() for a in host_gains)
    tw.check(K, k, fail, "self-test, untouched")
    # one entry of K~ moved by 16 x its bound
    bad = K.copy()
    scale = max(1.0, float(np.abs(tw.reference()[4]["stages"][7]["K"]).max()))
    bad[4, 7, 2, 5] += 16 * tw.bounds()[4, 0] * scale
    with pytest.raises(AssertionError, match="forward error of K: case 4 stage 7"):
        tw.check(bad, k, fail, "self-test")
    # one padded gain row set to 1e-300
    bad = K.copy()
    bad[4, 3, 7, :] = 1e-300
    with pytest.raises(AssertionError, match="padded rows: case 4 stage 3"):
        tw.check(bad, k, fail, "self-test")
    # the sentinel of one slot behind a horizon overwritten
    bad = k.copy()
    bad[1, 2, 11] = 0.0
    with pytest.raises(AssertionError, match="sentinel: case 1"):
        tw.check(K, bad, fail, "self-test")
    # the widths of case 3 shifted by one stage in what the code under test is fed (and of its copy, case 10, alike: shifted alone, case 3
    # would first be caught as "differs from its copy")
    with pytest.raises(AssertionError, match="forward error of K: case 3"):
        tw.check(*run_emu(emu, tw.arrays(shift=(3, 10))), "self-test")
    # the same shift on case 2 (all stages 12 wide) changes nothing: a uniform-width problem cannot see it
    shifted = run_emu(emu, tw.arrays(shift=(2,)))
    tw.check(*shifted, "self-test, case 2 shifted")
    assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(shifted[:2], host_gains[:2]))
