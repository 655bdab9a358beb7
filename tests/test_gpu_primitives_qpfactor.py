"""The factorisation primitives of hb_qpfactor.hpp on the DEVICE, where regularised_factor is the structured Householder form
(negative diagonal) and the host twin (tests/host_emu, emu_prim_*) is Givens insertion: two algorithms behind one name, shared by the
three QP solvers.  Properties are evaluated in mpmath (200 bits); where no closed bound is worth the name the device is measured
against the twin on the same inputs, the same way, and allowed 8x its figure (two backward-stable algorithms: a constant of that
size separates their bounds)."""
import numpy as np
import pytest

import _gpuunit
import _primcheck as pc

pytestmark = pytest.mark.gpu
# (instantiation, mA): hb_wbc.hpp regularised_factor<18, false> / UniformDiag / n 16; hb_hoqp.hpp <24, true> / HeadTailDiag / n 12
FACTOR_CASES = [(0, 0), (0, 1), (0, 8), (0, 18), (1, 0), (1, 1), (1, 6), (1, 24)]


@pytest.fixture(scope="module")
def dev():
    return _gpuunit.device()


@pytest.fixture(scope="module")
def twin():
    return _gpuunit.host()


@pytest.fixture(scope="module")
def factor_rows(dev, twin):
    """every case factored once on the device and once on the twin, shared by the tests below"""
    return {key: pc.factor_scenario(dev, key[0], key[1], twin=twin) for key in FACTOR_CASES}


@pytest.mark.parametrize("which,mA", FACTOR_CASES)
def test_regularised_factor(factor_rows, which, mA):
    """mA in {0, 1, n / 2, MA} x se in {1e-4, 1e-5, 1} x {random, a zero column, two equal columns, rows scaled over 8 decades}.
    Asserted in factor_properties: R upper triangular with exact zeros outside the triangle, nothing written outside wstore, a negative
    diagonal, householder_factor's return value equal to R_jj, g = A'b within gamma_mA |A'||b|.  The residual
    |R'R - (A'A + D^2)|_max / |A'A + D^2|_max of the device is at most 8x the twin's on each case, and the twin's is below 1e-13 (a
    well-posed case).  Measured maxima over the 96 cases: device (Householder) 4.6e-16, twin (Givens) 1.3e-15; the largest
    device / twin ratio on one case is 4.7."""
    for cs, r, rt, _, _ in factor_rows[(which, mA)]:
        what = f"{cs['kind']}, mA {mA}, se {cs['se']}"
        print(f"[primcheck] regularised_factor {which} {what}: residual device {r:.3g}, twin {rt:.3g}")
        assert rt <= 1e-13, f"{what}: the twin's residual {rt} says the case is badly posed"
        assert r <= 8.0 * rt, f"{what}: device residual {r} > 8 x twin {rt}"


@pytest.mark.parametrize("which,mA", FACTOR_CASES)
def test_invert_upper(factor_rows, which, mA):
    """invert_upper (through rcp_t) on those R: J below the diagonal exactly zero (asserted in factor_properties),
    |J R - I|_ij <= (n + 2) u (|J||R|)_ij, and the same for the right residual |R J - I| against |R||J| — the one the column-wise
    back substitution guarantees (factor_properties).  Measured on the device: at most 0.53 of the bound on the left, 0.10 on the
    right.  (The host twin's Givens factors reach 0.89 on the left in one ill-conditioned case: tests/test_primitives_host.py.)"""
    rows = factor_rows[(which, mA)]
    left, right = max(r[3] for r in rows), max(r[4] for r in rows)
    pc.report(f"invert_upper {which} mA {mA}: |J R - I| / ((n + 2) u |J||R|)", left, 1.0)
    pc.report(f"invert_upper {which} mA {mA}: |R J - I| / ((n + 2) u |R||J|)", right, 1.0)
    assert right <= 1.0
    assert left <= 1.0


def test_givens_insert_row_and_drop_constraint(dev, twin):
    """givens_insert_row (rsqrt_t) and drop_constraint on the device: R (and J) agree with the same algorithm in mpmath within 8x the host
    twin's own distance from it, case by case; after a drop J'N = [R; 0] holds within 8x the twin's measure, and the working-set
    records (act, lam, is_active, q) come out as on the host.  Measured maxima: distance device 3.7e-16, twin 1.8e-15; J'N - [R; 0]
    device 4.1e-15, twin 4.4e-15; the largest device / twin ratio on one case is 1.03."""
    cases = pc.givens_cases(np.random.default_rng(41))
    rd, rh = pc.givens_measure(cases, pc.givens_run(dev, cases)), pc.givens_measure(cases, pc.givens_run(twin, cases))
    for cs, d, h in zip(cases, rd, rh):
        what = f"{'drop_constraint' if cs['op'] else 'givens_insert_row'} n {cs['n']}" + (f" q {cs['q']} l {cs['l']}" if cs["op"] else "")
        print(f"[primcheck] {what}: distance from mpmath device {d[0]:.3g}, twin {h[0]:.3g}" + (f"; J'N - [R; 0] device {d[1]:.3g}, twin {h[1]:.3g}" if cs["op"] else ""))
        assert d[0] <= 8.0 * h[0], f"{what}: device {d[0]} > 8 x twin {h[0]}"
        if cs["op"]:
            assert d[1] <= 8.0 * h[1], f"{what}: J'N = [R; 0] off by {d[1]} on the device, {h[1]} on the twin"
            assert d[2] == h[2]
