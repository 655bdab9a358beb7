"""The scalar math of hb_math.hpp (and ric_rcp of hb_riccati.hpp) as the DEVICE compiles it, one primitive per kernel
(tests/gpu_unit/primitives.hip), against exact references computed from the same f64 inputs (tests/_primcheck.py: mpmath at 200 bits
for the worst-case sets, numpy.longdouble for the bulk sets with every point near its bound evaluated again in mpmath).  Every
bound is the claim of the code's own comment; tests/test_primitives_host.py runs the same checks on the host build."""
import numpy as np
import pytest

import _gpuunit
import _primcheck as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return _gpuunit.device()


def test_rcp_t_within_one_ulp(dev):
    """rcp_t (v_rcp_f64 + two Newton steps): "within 1 ulp" of the true reciprocal for normal operands with a normal result, both signs,
    log-uniform in [2^-1000, 2^1000], at 1 +- k ulp, 2 - k ulp (k <= 4) and next to sqrt 2; a power of two comes back exact."""
    pc.check_reciprocal("rcp_t", lambda x: dev.math("rcp_t", x)[0], bound=1.0)


def test_ric_rcp_within_one_ulp(dev):
    """ric_rcp (v_rcp_f64 + one cubic step): the comment's e ~ 2^-23 leaves e^3 ~ 2^-69 before the one final rounding: <= 1 ulp."""
    pc.check_reciprocal("ric_rcp", lambda x: dev.math("ric_rcp", x)[0], bound=1.0)


@pytest.mark.parametrize("op", ["sincos_reduced", "sincos_t", "sincos_bounded"])
def test_sincos_absolute_error(dev, op):
    """"absolute error < 2e-16" for sine and cosine on |a| < 1e5: uniform in [-10, 10], log-uniform in [1e-8, 1e5), the doubles nearest
    to k pi / 2 (every 7th k up to 63661) with their neighbours towards zero, +-0 and nextafter(1e5, 0).  (Measured: 1.59e-16 for the
    sine, 1.55e-16 for the cosine, on the device and on the host build of the same source alike.)"""
    pc.check_sincos(op, lambda x: tuple(dev.math(op, x)[:2]))


def test_sincos_t_beyond_the_reduced_range(dev):
    """at and beyond 1e5 sincos_t takes the library path: within 2 ulp of mpmath for finite arguments, NaN for inf and NaN"""
    pc.check_sincos_far("sincos_t", lambda x: tuple(dev.math("sincos_t", x)[:2]), bounded=False)


def test_sincos_bounded_marks_the_far_range(dev):
    """sincos_bounded has no library path: NaN at and beyond 1e5, for inf and for NaN"""
    pc.check_sincos_far("sincos_bounded", lambda x: tuple(dev.math("sincos_bounded", x)[:2]), bounded=True)


def test_dual_sincos(dev):
    """sincos_t(Dual1): the values as above; the tangents cos(a) a.d and -sin(a) a.d within 4 ulp of the derivative's magnitude plus the
    value bound times |a.d| (tests/_primcheck.py, Dual1 forms)"""
    pc.check_dual_sincos("sincos_t(Dual1)", lambda a, ad: dev.math("dual_sincos_t", a, ad))


def test_dual_rcp(dev):
    pc.check_dual_rcp("rcp_t(Dual1)", lambda a, ad: dev.math("dual_rcp_t", a, ad)[:2], value_ulps=1.0)


def test_dual_sqrt(dev):
    pc.check_dual_sqrt("sqrt_t(Dual1)", lambda a, ad: dev.math("dual_sqrt_t", a, ad)[:2], rcp_ulps=1.0)


def test_dual_division(dev):
    pc.check_dual_div("Dual1 operator/", lambda a, ad, b, bd: dev.math("dual_div", a, ad, b, bd)[:2], rcp_ulps=1.0)


def test_log_fd_within_two_ulp(dev):
    """log_fd with the frexp builtins and rcp_t: "Error < 1 ulp (+ the reciprocal's)" = 2 ulp against mpmath, on the set of the host test
    (test_device_logarithm_scheme_matches_libm), mantissas within 4 ulp of sqrt(1/2) on both sides and arguments within 1e-3 of 1.
    (Measured: 0.69 ulp on the device, 0.78 ulp on the host build.)"""
    pc.check_log("log_fd", lambda x: dev.math("log_fd", x)[0], bound=2.0)


def test_rsqrt_t_within_two_ulp(dev):
    """rsqrt_t is the library's rsqrt() on the device (1 / sqrt on the host: 1.45 ulp, two roundings); givens_insert_row and
    drop_constraint are its consumers, and they take <= 2 ulp.  Measured maximum on the device over this set (log-uniform in
    [1e-300, 1e300]): 0.948 ulp."""
    pc.check_rsqrt("rsqrt_t", lambda x: dev.math("rsqrt_t", x)[0], bound=2.0)


def test_sqrt_t_correctly_rounded(dev):
    """sqrt_t is the IEEE square root: correctly rounded, so bit-equal to numpy's — what check_dual_sqrt builds its tangent tolerance on"""
    x = pc.rsqrt_points()
    pc.check_bits_equal("sqrt_t", dev.math("sqrt_t", x)[0], np.sqrt(x))
