"""The checkers of tests/test_gpu_primitives_*.py on a machine without a GPU: wherever a primitive has a host branch (the tile loops,
log_fd, sincos_*, regularised_factor's Givens form, invert_upper, the 1 / a forms of rcp_t and ric_rcp, rsqrt_t as 1 / sqrt), the same
vectors go through the host twin (the emu_prim_* exports of tests/host_emu/hostemu.cpp, which run the cases of
tests/gpu_unit/prim_cases.hpp) and into the same assertion helpers with the same bounds (tests/_primcheck.py).  The lane primitives
have no host form; their checkers are shown to reject a stale carrier and a foreign group on a numpy model of the DPP shifts, and
the exact tile probes to reject a transposed operand."""
import numpy as np
import pytest

import _gpuunit
import _primcheck as pc


@pytest.fixture(scope="module")
def twin():
    return _gpuunit.host()


# ------------------------------------------------------------------------------------------------------------------ scalar math
@pytest.mark.parametrize("op", ["rcp_t", "ric_rcp"])
def test_reciprocals(twin, op):
    """1.0 / a: correctly rounded (0.5 ulp) inside the 1 ulp the device forms document"""
    assert pc.check_reciprocal(op, lambda x: twin.math(op, x)[0], bound=1.0) <= 0.5


@pytest.mark.parametrize("op", ["sincos_reduced", "sincos_t", "sincos_bounded"])
def test_sincos_absolute_error(twin, op):
    """measured here: 1.59e-16 (sine), 1.55e-16 (cosine) of the documented 2e-16"""
    pc.check_sincos(op, lambda x: tuple(twin.math(op, x)[:2]))


def test_sincos_far_range(twin):
    pc.check_sincos_far("sincos_t", lambda x: tuple(twin.math("sincos_t", x)[:2]), bounded=False)
    pc.check_sincos_far("sincos_bounded", lambda x: tuple(twin.math("sincos_bounded", x)[:2]), bounded=True)


def test_dual_forms(twin):
    """(the reciprocal is 1.0 / a here: 0.5 ulp where the device has 1)"""
    pc.check_dual_sincos("sincos_t(Dual1)", lambda a, ad: twin.math("dual_sincos_t", a, ad))
    pc.check_dual_rcp("rcp_t(Dual1)", lambda a, ad: twin.math("dual_rcp_t", a, ad)[:2], value_ulps=0.5)
    pc.check_dual_sqrt("sqrt_t(Dual1)", lambda a, ad: twin.math("dual_sqrt_t", a, ad)[:2], rcp_ulps=0.5)
    pc.check_dual_div("Dual1 operator/", lambda a, ad, b, bd: twin.math("dual_div", a, ad, b, bd)[:2], rcp_ulps=0.5)


def test_log_fd(twin):
    """measured here: 0.78 ulp of the documented 2"""
    pc.check_log("log_fd", lambda x: twin.math("log_fd", x)[0], bound=2.0)


def test_rsqrt(twin):
    """1 / sqrt(a): two roundings, 1.45 ulp measured, inside the 2 ulp its consumers take"""
    pc.check_rsqrt("rsqrt_t", lambda x: twin.math("rsqrt_t", x)[0], bound=2.0)


def test_checkers_reject_a_wrong_value():
    """the ulp checker on a reciprocal that is 2 ulp off in one point, the absolute checker on a sine that is 3e-16 off"""
    def off(x):
        y = 1.0 / x
        y[7] = pc.step_ulps(y[7], 2)
        return y
    with pytest.raises(AssertionError):
        pc.check_reciprocal("1 / a, one point moved by 2 ulp", off)
    with pytest.raises(AssertionError):
        pc.check_sincos("sine + 3e-16", lambda x: (np.sin(x) + 3e-16, np.cos(x)))
    with pytest.raises(AssertionError):
        pc.check_reciprocal("1 / a with an inexact power of two", lambda x: np.where(x == 4.0, pc.step_ulps(0.25, 1), 1.0 / x))


# ------------------------------------------------------------------------------------------------------------------ lane checkers
def model_scan(v, suffix, stale=False):
    """three rounds of the scan on the numpy model of the DPP shifts, the three components on their own carriers.  stale: the carrier
    of the partial bank mask starts each later round with what the OTHER scan would have left in it (its unwritten lanes are not zero)."""
    out = np.zeros_like(v)
    for c in range(v.shape[0]):
        carriers = [np.zeros(64) for _ in range(3)]
        for r in range(3):
            for k in range(3):
                fn = pc.model_seg8_suffix_sum if suffix else pc.model_seg8_prefix_sum
                if stale and r > 0:
                    carriers[k] = np.roll(out[c, r - 1, k], 3)
                out[c, r, k], carriers[k] = fn(v[c, r, k], carriers[k])
    return out


@pytest.mark.parametrize("suffix", [True, False])
def test_scan_checker_on_the_dpp_model(suffix):
    """the model of seg8_suffix_sum / seg8_prefix_sum (row shifts, bank masks 0x5 / 0xa, bound_ctrl, carriers) passes the exact check
    over three rounds on one carrier; the same model with a stale carrier does not"""
    v = pc.seg8_scan_inputs("int", 3, np.random.default_rng(51))
    name = "suffix" if suffix else "prefix"
    pc.check_seg8_scan(f"model {name}", v, model_scan(v, suffix), suffix, exact=True)
    vf = pc.seg8_scan_inputs("f64", 3, np.random.default_rng(52))
    pc.check_seg8_scan(f"model {name} f64", vf, model_scan(vf, suffix), suffix, exact=False)
    with pytest.raises(AssertionError):
        pc.check_seg8_scan(f"model {name}, stale carrier", v, model_scan(v, suffix, stale=True), suffix, exact=True)


def test_scan_checker_rejects_a_shift_without_its_bank_mask():
    """a suffix sum whose shifts write every lane (bank mask 0xf) pulls the neighbouring group of the DPP row into lanes 4 .. 7"""
    v = pc.seg8_scan_inputs("int", 2, np.random.default_rng(53))
    out = np.zeros_like(v)
    for idx in np.ndindex(v.shape[:-1]):
        x = v[idx].copy()
        for sh in (1, 2, 4):
            x = x + pc.dpp_row_shift(x, np.zeros(64), sh, 0xf)
        out[idx] = x
    with pytest.raises(AssertionError):
        pc.check_seg8_scan("suffix without bank mask", v, out, True, exact=True)


def test_sum_and_product_checkers():
    v = pc.lane_values("f64", 4, np.random.default_rng(54))
    pairwise = v.reshape(4, 8, 8).copy()
    for _ in range(3):
        pairwise = pairwise[..., 0::2] + pairwise[..., 1::2]
    out = np.repeat(pairwise.reshape(4, 8), 8, axis=1)
    pc.check_group_sum("pairwise sums of eight", v, out, 8, 3, exact=False)
    with pytest.raises(AssertionError):
        pc.check_group_sum("one lane left out", v, out - np.repeat(v.reshape(4, 8, 8)[..., 5], 8, axis=1), 8, 3, exact=False)
    inp = pc.prefix_product_inputs(1, np.random.default_rng(55))
    m = inp.transpose(0, 2, 1).reshape(1, 64, 3, 3)
    right, wrong = m.copy(), m.copy()
    for g in range(8):
        for k in range(1, 5):
            right[0, 8 * g + k] = right[0, 8 * g + k - 1] @ m[0, 8 * g + k]
            wrong[0, 8 * g + k] = m[0, 8 * g + k] @ wrong[0, 8 * g + k - 1]        # the product in the other order
    pack = lambda a: np.ascontiguousarray(a.reshape(1, 64, 9).transpose(0, 2, 1))   # noqa: E731
    pc.check_prefix_product("numpy prefix product", inp, pack(right))
    with pytest.raises(AssertionError):
        pc.check_prefix_product("reversed order", inp, pack(wrong))


# ------------------------------------------------------------------------------------------------------------------ tile loops
@pytest.mark.parametrize("site", pc.TILE_SITES, ids=pc.TILE_SITE_IDS)
def test_tile_products(twin, site):
    """the host loops under the exact, poisoned, unit-matrix and rounding scenarios of the GPU test"""
    pc.tile_exact_scenario(twin, site)
    pc.tile_unit_scenario(twin, site)
    pc.tile_rounding_scenario(twin, site)


def test_exact_probes_reject_a_transposed_operand(twin):
    """A laid out transposed on purpose (hb_lq.hpp Kx' M: TA, LDA 29, KR 10 of 12): the integer probe and the unit-matrix probe both fail"""
    site = next(s for s in pc.TILE_SITES if s[4] == "hb_lq.hpp:1147")
    with pytest.raises(AssertionError):
        pc.tile_exact_scenario(twin, site, transpose_A=True)
    with pytest.raises(AssertionError):
        pc.tile_unit_scenario(twin, site, transpose_A=True)


@pytest.mark.parametrize("Mr,Nr", pc.RT_SHAPES)
def test_tile_initialisers_and_stores(twin, Mr, Nr):
    pc.tile_roundtrip_scenario(twin, Mr, Nr)


# ------------------------------------------------------------------------------------------------------------------ QP factorisation
FACTOR_CASES = [(0, 0), (0, 1), (0, 8), (0, 18), (1, 0), (1, 1), (1, 6), (1, 24)]


@pytest.fixture(scope="module")
def factor_rows(twin):
    return {key: pc.factor_scenario(twin, key[0], key[1]) for key in FACTOR_CASES}


@pytest.mark.parametrize("which,mA", FACTOR_CASES)
def test_regularised_factor_givens_form(factor_rows, which, mA):
    """the Givens form: structure, g = A'b within gamma_mA |A'||b| and a residual below 1e-13 on every case (what makes a case well
    posed for the device test).  Measured maximum: 1.28e-15."""
    for cs, r, _, _, right in factor_rows[(which, mA)]:
        assert r <= 1e-13, (cs["kind"], cs["se"], r)
        assert right <= 1.0, (cs["kind"], cs["se"], right)


@pytest.mark.parametrize("which,mA", FACTOR_CASES)
def test_invert_upper(factor_rows, which, mA):
    """|J R - I|_ij <= (n + 2) u (|J||R|)_ij on the Givens factors: n fused multiply-adds, the reciprocal and its product.
    Measured: at most 0.40 of the bound on every case but one — regularised_factor<18, false>, mA 18, rows scaled over 8 decades,
    se 1e-4 (cond(R) 6.6e7) — which reaches 0.89.  (With the accumulation left to the host compiler, unfused, that case was at
    2.14; column-wise back substitution only GUARANTEES the right residual |R J - I|, which is at 0.09 of its bound at most and is
    asserted in test_regularised_factor_givens_form.)"""
    worst = max(r[3] for r in factor_rows[(which, mA)])
    pc.report(f"invert_upper {which} mA {mA}: |J R - I| / ((n + 2) u |J||R|)", worst, 1.0)
    assert worst <= 1.0


def test_givens_primitives(twin):
    """givens_insert_row and drop_constraint on the host against the same algorithm in mpmath (the twin's own distance, which the device
    test takes 8x of).  Every entry passes through at most n rotations; a computed rotation errs by at most gamma_6 of the 2-norm of
    the pair it acts on (Higham, Lemma 19.8), which is at most sqrt 2 of the largest entry: distance <= sqrt(2) gamma_(6 n).
    Measured: 4.9e-16 at most (n = 16: bound 1.5e-14).  The working-set records are asserted in givens_measure."""
    cases = pc.givens_cases(np.random.default_rng(41))
    for cs, (dist, rn, _) in zip(cases, pc.givens_measure(cases, pc.givens_run(twin, cases))):
        print(f"[primcheck] {'drop_constraint' if cs['op'] else 'givens_insert_row'} n {cs['n']}: distance {dist:.3g}, J'N - [R; 0] {rn}")
        assert dist <= np.sqrt(2.0) * pc.gamma(6 * cs["n"]), (cs["op"], cs["n"], dist)
