"""Vectors, exact references and assertion helpers of the primitive-layer tests: tests/test_gpu_primitives_*.py run them on the
device wrappers (tests/gpu_unit), tests/test_primitives_host.py on the host twin, so every helper and every bound is exercised
without a GPU as well.

References are computed from the same f64 inputs: mpmath at 200 bits for the worst-case sets and the matrix properties,
numpy.longdouble (64-bit mantissa) for the bulk sets — a bulk point that comes within 1 % of its bound is evaluated again in
mpmath, so the longdouble reference's own 1e-3 ulp never decides a test.  A reference value is kept as an unevaluated sum hi + lo of
two doubles (|lo| <= ulp(hi) / 2: 106 bits); `err_vs` subtracts it without cancellation.

Every check prints its measured figure before it asserts."""
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np

U = 2.0 ** -53                      # unit roundoff of f64
MP = mpmath.mp.clone()
MP.prec = 200
LD_OK = np.finfo(np.longdouble).eps < 2e-19


def gamma(d):
    """gamma_d = d u / (1 - d u): the constant of d accumulated roundings (Higham, Accuracy and Stability, Lemma 3.1)"""
    return d * U / (1.0 - d * U)


# ------------------------------------------------------------------------------------------------------------------ references
def split_mp(vals):
    """list of mpf -> (hi, lo) f64 arrays with hi + lo = value to 106 bits"""
    hi = np.array([float(v) for v in vals])
    lo = np.array([float(v - MP.mpf(h)) if math.isfinite(h) else 0.0 for v, h in zip(vals, hi)])
    return hi, lo


def split_ld(v):
    hi = v.astype(np.float64)
    lo = (v - hi.astype(np.longdouble)).astype(np.float64)
    return hi, lo


def ref_mp(fn, *xs):
    """fn(mpf, ...) -> mpf over the points, 200 bits"""
    return split_mp([fn(*(MP.mpf(float(v)) for v in p)) for p in zip(*xs)])


def err_vs(y, hi, lo):
    """|y - (hi + lo)| (y - hi is exact where it matters: the two are within a factor of two)"""
    return np.abs((y - hi) - lo)


def ulp_true(hi, lo):
    """the f64 ulp of the binade the TRUE value hi + lo lies in (a value just below a power of two has the smaller one)"""
    m, e = np.frexp(np.abs(hi))
    e = np.where((m == 0.5) & (lo * np.sign(hi) < 0), e - 1, e)
    return np.ldexp(1.0, np.maximum(e - 53, -1074))


def report(what, figure, bound, unit=""):
    print(f"[primcheck] {what}: measured {figure:.4g}{unit}, bound {bound:.4g}{unit}")


def check_ulp(what, x, y, ref, bound, refine=None):
    """max |y - ref| / ulp(ref) <= bound.  refine(x_subset) -> (hi, lo) re-evaluates points within 1 % of the bound in mpmath."""
    hi, lo = (np.array(r, dtype=np.float64) for r in ref)
    err = err_vs(y, hi, lo) / ulp_true(hi, lo)
    if refine is not None:
        close = np.nonzero(~(err <= 0.99 * bound))[0]
        assert len(close) <= 5000, f"{what}: {len(close)} points at the bound"
        if len(close):
            h2, l2 = refine(x[close])
            hi[close], lo[close] = h2, l2
            err = err_vs(y, hi, lo) / ulp_true(hi, lo)
    bad = ~(err <= bound)          # (a NaN result is an error as well)
    worst = int(np.argmax(np.where(np.isnan(err), np.inf, err)))
    report(what, float(err[worst]), bound, " ulp")
    assert not bad.any(), f"{what}: {err[worst]} ulp at x = {x[worst]!r} (got {y[worst]!r}, true {hi[worst]!r} + {lo[worst]!r}); {int(bad.sum())} points over {bound}"
    return float(err[worst])


def check_abs(what, x, y, ref, bound, refine=None, strict=True):
    """max |y - ref| < bound"""
    hi, lo = (np.array(r, dtype=np.float64) for r in ref)
    err = err_vs(y, hi, lo)
    if refine is not None:
        close = np.nonzero(~(err <= 0.99 * bound))[0]
        assert len(close) <= 5000, f"{what}: {len(close)} points at the bound"
        if len(close):
            h2, l2 = refine(x[close])
            hi[close], lo[close] = h2, l2
            err = err_vs(y, hi, lo)
    bad = ~(err < bound) if strict else ~(err <= bound)
    worst = int(np.argmax(np.where(np.isnan(err), np.inf, err)))
    report(what, float(err[worst]), bound)
    assert not bad.any(), f"{what}: {err[worst]} at x = {x[worst]!r} (got {y[worst]!r}); {int(bad.sum())} points over {bound}"
    return float(err[worst])


def check_tol(what, x, y, ref, tol):
    """|y - ref| <= tol, point by point"""
    hi, lo = ref
    err = err_vs(y, hi, lo)
    ratio = err / tol
    bad = ~(err <= tol)
    worst = int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)))
    report(what + " (error / tolerance)", float(ratio[worst]), 1.0)
    assert not bad.any(), f"{what}: error {err[worst]} over tolerance {tol[worst]} at {x[worst]!r}; {int(bad.sum())} points over"
    return float(ratio[worst])


def frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    a.setflags(write=False)
    return a


def step_ulps(x, k):
    """x moved by k ulps (k may be negative)"""
    x = np.float64(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


# ------------------------------------------------------------------------------------------------------------------ reciprocals
@functools.lru_cache(None)
def rcp_points():
    """(bulk, special, powers): both signs; log-uniform magnitudes in [2^-1000, 2^1000] (operand and result normal); every 1 +- k ulp and
    2 - k ulp for k <= 4, mantissas next to sqrt 2, at three exponents; exact powers of two."""
    rng = np.random.default_rng(11)
    bulk = rng.choice([-1.0, 1.0], 20000) * np.exp2(rng.uniform(-1000.0, 1000.0, 20000))
    m = [step_ulps(1.0, k) for k in range(-4, 5)] + [step_ulps(2.0, -k) for k in range(1, 5)] + [step_ulps(np.sqrt(2.0), k) for k in range(-4, 5)]
    special = np.array([s * np.ldexp(v, e) for v in m for e in (-1000, 0, 998) for s in (1.0, -1.0)])
    powers = np.array([s * np.ldexp(1.0, e) for e in range(-1000, 1001) for s in (1.0, -1.0)])
    return frozen(bulk), frozen(special), frozen(powers)


def ref_rcp(x, exact=False):
    if exact or not LD_OK:
        return ref_mp(lambda a: 1 / a, x)
    return split_ld(np.longdouble(1.0) / x.astype(np.longdouble))


def check_reciprocal(what, fn, bound=1.0):
    """fn(x) -> y over the three sets: <= bound ulp of the true reciprocal, a power of two comes back exact"""
    bulk, special, powers = rcp_points()
    worst = check_ulp(what + " bulk", bulk, fn(bulk), ref_rcp(bulk), bound, refine=lambda xs: ref_rcp(xs, exact=True))
    worst = max(worst, check_ulp(what + " special", special, fn(special), ref_rcp(special, exact=True), bound))
    y = fn(powers)
    assert np.array_equal(y, 1.0 / powers), f"{what}: a power of two did not come back exact: {powers[y != 1.0 / powers][:4]}"
    return worst


# ------------------------------------------------------------------------------------------------------------------ sine / cosine
SINCOS_BOUND = 2e-16     # hb_math.hpp: "absolute error < 2e-16"


@functools.lru_cache(None)
def sincos_points():
    """(bulk, worst): uniform in [-10, 10] and log-uniform |a| in [1e-8, 1e5), both signs; the double nearest to k pi / 2 and its
    neighbour towards zero for every 7th k in 1 .. 63661, both signs, +-0 and nextafter(1e5, 0)."""
    rng = np.random.default_rng(12)
    bulk = np.concatenate([rng.uniform(-10.0, 10.0, 10000), rng.choice([-1.0, 1.0], 10000) * 10.0 ** rng.uniform(-8.0, 5.0, 10000)])
    bulk = bulk[np.abs(bulk) < 1e5]
    hp = MP.pi / 2
    near = np.array([float(k * hp) for k in range(1, 63662, 7)])
    near = np.concatenate([near, np.nextafter(near, 0.0)])
    worst = np.concatenate([near, -near, [0.0, -0.0, np.nextafter(1e5, 0.0), -np.nextafter(1e5, 0.0)]])
    assert np.abs(worst).max() < 1e5
    return frozen(bulk), frozen(worst)


def _sincos_mp(x):
    return ref_mp(MP.sin, x), ref_mp(MP.cos, x)


@functools.lru_cache(None)
def sincos_reference():
    """((sin hi, lo), (cos hi, lo)) on bulk and on worst: computed once, shared by every test that needs it, never modified"""
    bulk, worst = sincos_points()
    if LD_OK:
        xl = bulk.astype(np.longdouble)
        rb = (split_ld(np.sin(xl)), split_ld(np.cos(xl)))
    else:
        rb = _sincos_mp(bulk)
    rw = _sincos_mp(worst)
    for pair in (*rb, *rw):
        for a in pair:
            a.setflags(write=False)
    return rb, rw


def check_sincos(what, fn):
    """fn(x) -> (s, c): absolute error < 2e-16 on both point sets; returns the measured maxima (sine, cosine)"""
    (bulk, worst), (rb, rw) = sincos_points(), sincos_reference()
    out, on_bulk, on_worst = [], fn(bulk), fn(worst)
    for which, idx in (("sine", 0), ("cosine", 1)):
        mpf = MP.sin if idx == 0 else MP.cos
        yb, yw = on_bulk[idx], on_worst[idx]
        e1 = check_abs(f"{what} {which} bulk", bulk, yb, rb[idx], SINCOS_BOUND, refine=lambda xs, f=mpf: ref_mp(f, xs))
        e2 = check_abs(f"{what} {which} near k pi/2", worst, yw, rw[idx], SINCOS_BOUND)
        out.append(max(e1, e2))
    return tuple(out)


@functools.lru_cache(None)
def sincos_far_points():
    finite = np.array([1e5, np.nextafter(1e5, np.inf), 123456.789, 1e6, 2.0 ** 40 + 1.0, 1e10, 1e22, 1e100, 1.7e308])
    finite = np.concatenate([finite, -finite])
    return frozen(finite), frozen([np.inf, -np.inf, np.nan])


def check_sincos_far(what, fn, bounded):
    """at and beyond 1e5: sincos_t follows the library (<= 2 ulp of mpmath, NaN for inf / NaN); sincos_bounded gives NaN throughout"""
    finite, nonfinite = sincos_far_points()
    s, c = fn(finite)
    sn, cn = fn(nonfinite)
    assert np.isnan(sn).all() and np.isnan(cn).all(), f"{what}: inf / NaN must give NaN, got {sn}, {cn}"
    if bounded:
        assert np.isnan(s).all() and np.isnan(c).all(), f"{what}: NaN expected at and beyond 1e5, got {s}, {c}"
        return
    check_ulp(what + " sine, |a| >= 1e5", finite, s, ref_mp(MP.sin, finite), 2.0)
    check_ulp(what + " cosine, |a| >= 1e5", finite, c, ref_mp(MP.cos, finite), 2.0)


# ------------------------------------------------------------------------------------------------------------------ logarithm, rsqrt
@functools.lru_cache(None)
def log_points():
    """the set of test_device_logarithm_scheme_matches_libm, mantissas within 4 ulp of sqrt(1/2) on both sides (at several exponents) and
    arguments within 1e-3 of 1"""
    rng = np.random.default_rng(3)
    x = np.concatenate([10.0 ** rng.uniform(-12, 12, 20000), rng.uniform(0.05, 400.0, 20000), 1.0 + rng.uniform(-1e-3, 1e-3, 2000),
                        [1.0, 0.5, 2.0, np.sqrt(0.5), np.sqrt(2.0), np.nextafter(np.sqrt(0.5), 0), 0.1, 5.0, 350.0]])
    edge = np.array([np.ldexp(step_ulps(np.sqrt(0.5), k), e) for k in range(-4, 5) for e in (-40, -1, 0, 1, 2, 40)])
    one = np.array([step_ulps(1.0, k) for k in range(-4, 5)])
    return frozen(x), frozen(np.concatenate([edge, one]))


@functools.lru_cache(None)
def log_reference():
    x, edge = log_points()
    rx = split_ld(np.log(x.astype(np.longdouble))) if LD_OK else ref_mp(MP.log, x)
    return rx, ref_mp(MP.log, edge)


def check_log(what, fn, bound=2.0):
    (x, edge), (rx, re_) = log_points(), log_reference()
    e1 = check_ulp(what + " bulk", x, fn(x), rx, bound, refine=lambda xs: ref_mp(MP.log, xs))
    e2 = check_ulp(what + " edges", edge, fn(edge), re_, bound)
    return max(e1, e2)


@functools.lru_cache(None)
def rsqrt_points():
    rng = np.random.default_rng(13)
    return frozen(10.0 ** rng.uniform(-300.0, 300.0, 20000))


def check_rsqrt(what, fn, bound=2.0):
    x = rsqrt_points()
    ref = split_ld(np.longdouble(1.0) / np.sqrt(x.astype(np.longdouble))) if LD_OK else ref_mp(lambda a: 1 / MP.sqrt(a), x)
    return check_ulp(what, x, fn(x), ref, bound, refine=lambda xs: ref_mp(lambda a: 1 / MP.sqrt(a), xs))


# ------------------------------------------------------------------------------------------------------------------ Dual1 forms
# The tangent of a dual operation is a short expression in the operation's VALUES (v_i, each with its value bound b_i) and the incoming
# tangents.  Its tolerance is 4 ulp of the true derivative's magnitude (the roundings of the expression itself: at most four, none of
# them on a cancelling difference) plus sum_i |d tangent / d v_i| b_i, the value bounds carried through to first order — for the
# sine, whose tangent is cos(a) a.d, that is "the value bound times |a.d|".
@functools.lru_cache(None)
def dual_points():
    rng = np.random.default_rng(14)
    n = 4000
    ang = np.concatenate([rng.uniform(-10.0, 10.0, n // 2), rng.choice([-1.0, 1.0], n // 2) * 10.0 ** rng.uniform(-8.0, 5.0, n // 2)])
    ang = np.where(np.abs(ang) < 1e5, ang, 1.0)
    tan = lambda: rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3.0, 3.0, n)   # noqa: E731
    mag = lambda lo, hi: rng.choice([-1.0, 1.0], n) * np.exp2(rng.uniform(lo, hi, n))   # noqa: E731
    return {"ang": frozen(ang), "ang_d": frozen(tan()), "a": frozen(mag(-100, 100)), "a_d": frozen(tan()), "b": frozen(mag(-100, 100)),
            "b_d": frozen(tan()), "pos": frozen(np.abs(mag(-200, 200))), "pos_d": frozen(tan())}


def _ulp_of_mp(vals):
    hi, lo = split_mp(vals)
    return ulp_true(hi, lo)


def check_dual_sincos(what, fn):
    """fn(a, ad) -> (s.v, s.d, c.v, c.d)"""
    p = dual_points()
    a, ad = p["ang"], p["ang_d"]
    sv, sd, cv, cd = fn(a, ad)
    rs, rc = ref_mp(MP.sin, a), ref_mp(MP.cos, a)
    check_abs(what + " value sine", a, sv, rs, SINCOS_BOUND)
    check_abs(what + " value cosine", a, cv, rc, SINCOS_BOUND)
    ds = [MP.cos(MP.mpf(float(x))) * MP.mpf(float(d)) for x, d in zip(a, ad)]
    dc = [-MP.sin(MP.mpf(float(x))) * MP.mpf(float(d)) for x, d in zip(a, ad)]
    check_tol(what + " tangent sine", a, sd, split_mp(ds), 4 * _ulp_of_mp(ds) + SINCOS_BOUND * np.abs(ad))
    check_tol(what + " tangent cosine", a, cd, split_mp(dc), 4 * _ulp_of_mp(dc) + SINCOS_BOUND * np.abs(ad))


def check_dual_rcp(what, fn, value_ulps=1.0):
    """fn(a, ad) -> (r, d): r = 1 / a within value_ulps; d = -a.d r^2, d d / d r = 2 |a.d r|"""
    p = dual_points()
    a, ad = p["a"], p["a_d"]
    r, d = fn(a, ad)
    ref = ref_rcp(a, exact=True)
    check_ulp(what + " value", a, r, ref, value_ulps)
    dt = [-MP.mpf(float(t)) / MP.mpf(float(x)) ** 2 for x, t in zip(a, ad)]
    tol = 4 * _ulp_of_mp(dt) + 2 * np.abs(ad * ref[0]) * value_ulps * ulp_true(*ref)
    check_tol(what + " tangent", a, d, split_mp(dt), tol)


def check_dual_sqrt(what, fn, rcp_ulps=1.0):
    """fn(a, ad) -> (r, d): r = sqrt(a) correctly rounded (0.5 ulp); d = a.d / 2 * rcp(r): through r, |a.d| / (2 r^2) * ulp(r) / 2, and
    through the reciprocal, |a.d| / 2 * rcp_ulps ulp(1 / r)"""
    p = dual_points()
    a, ad = p["pos"], p["pos_d"]
    r, d = fn(a, ad)
    ref = ref_mp(MP.sqrt, a)
    check_ulp(what + " value", a, r, ref, 0.5)
    dt = [MP.mpf(float(t)) / (2 * MP.sqrt(MP.mpf(float(x)))) for x, t in zip(a, ad)]
    inv = ref_mp(lambda x: 1 / MP.sqrt(x), a)
    tol = 4 * _ulp_of_mp(dt) + np.abs(ad) / (2 * ref[0] ** 2) * 0.5 * ulp_true(*ref) + 0.5 * np.abs(ad) * rcp_ulps * ulp_true(*inv)
    check_tol(what + " tangent", a, d, split_mp(dt), tol)


def check_dual_div(what, fn, rcp_ulps=1.0):
    """fn(a, ad, b, bd) -> (q, d).  q = a * rcp(b): the reciprocal's rcp_ulps ulp (<= 2 u rcp_ulps relative) and one rounding:
    |q - a / b| <= (2 rcp_ulps + 1) u |a / b|.  d = (a.d - q b.d) * inv: through q — with the rounding of the product q b.d, which sits in
    front of a difference that may cancel — (2 rcp_ulps + 2) u |q| |b.d / b|; through inv, |a.d - q b.d| rcp_ulps ulp(1 / b)."""
    p = dual_points()
    a, ad, b, bd = p["a"], p["a_d"], p["b"], p["b_d"]
    q, d = fn(a, ad, b, bd)
    rq = ref_mp(lambda x, y: x / y, a, b)
    check_tol(what + " value", a, q, rq, (2 * rcp_ulps + 1) * U * np.abs(rq[0]))
    dt = [(MP.mpf(float(t)) - MP.mpf(float(x)) / MP.mpf(float(y)) * MP.mpf(float(s))) / MP.mpf(float(y)) for x, t, y, s in zip(a, ad, b, bd)]
    inv = ref_rcp(b, exact=True)
    tol = (4 * _ulp_of_mp(dt) + (2 * rcp_ulps + 2) * U * np.abs(rq[0] * bd / b)
           + np.abs(split_mp(dt)[0] * b) * rcp_ulps * ulp_true(*inv))
    check_tol(what + " tangent", a, d, split_mp(dt), tol)


# ------------------------------------------------------------------------------------------------------------------ lane primitives
def lane_values(kind, ncases, rng):
    """64 distinct values per case: small integers (every partial sum exact) or random f64 over six decades, both signs"""
    if kind == "int":
        return np.stack([rng.permutation(np.arange(-40, 24, dtype=np.float64)) for _ in range(ncases)])
    v = rng.choice([-1.0, 1.0], (ncases, 64)) * 10.0 ** rng.uniform(-3.0, 3.0, (ncases, 64))
    assert all(len(set(r)) == 64 for r in v)
    return v


def group_reduce(v, width, fn):
    """fn over each aligned group of `width` lanes, handed to all of them: [ncases][64] -> [ncases][64]"""
    g = v.reshape(v.shape[0], 64 // width, width)
    r = np.array([[fn(list(row)) for row in case] for case in g])
    return np.repeat(r, width, axis=1)


def check_group_sum(what, v, out, width, depth, exact):
    """every lane of a group holds the group's sum: bit-exact for integer data, else within gamma_depth sum |v| (a ladder of `depth`
    pairwise additions: every input passes through `depth` roundings)"""
    ref = group_reduce(v, width, math.fsum)
    if exact:
        assert np.array_equal(out, ref), f"{what}: integer sums differ in {int((out != ref).sum())} lanes"
        print(f"[primcheck] {what}: integer sums bit-exact")
        return
    bound = gamma(depth) * group_reduce(np.abs(v), width, math.fsum)
    err = np.abs(out - ref)     # (ref is the correctly rounded exact sum: its own u |sum| is inside the slack between gamma_d and d u)
    report(what + " (error / gamma bound)", float((err / bound).max()), 1.0)
    assert (err <= bound + U * np.abs(ref)).all(), f"{what}: {float((err / bound).max())} of the gamma_{depth} bound"
    g = out.reshape(out.shape[0], 64 // width, width)
    assert (g == g[:, :, :1]).all(), f"{what}: the lanes of a group do not agree"


def check_bits_equal(what, out, ref):
    a, b = np.ascontiguousarray(out).view(np.uint64), np.ascontiguousarray(ref, dtype=np.float64).view(np.uint64)
    assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} words differ, first at {np.argwhere(a != b)[0]}"
    print(f"[primcheck] {what}: {a.size} words bit-equal")


def seg8_scan_inputs(kind, ncases, rng):
    """[ncases][3 rounds][3 components][64]: lanes 5..7 of every group zero (the contract), different data in all eight groups"""
    v = (rng.integers(-30, 31, (ncases, 3, 3, 64)).astype(np.float64) if kind == "int"
         else rng.choice([-1.0, 1.0], (ncases, 3, 3, 64)) * 10.0 ** rng.uniform(-3.0, 3.0, (ncases, 3, 3, 64)))
    v[..., (np.arange(64) % 8) >= 5] = 0.0
    return v


def seg8_scan_reference(v, suffix):
    """lane k < 5 of a group <- exact sum over lanes k .. 4 (suffix) or 0 .. k (prefix), correctly rounded; and the sum of |.|"""
    g = v.reshape(*v.shape[:-1], 8, 8)
    ref, mag = np.zeros_like(g), np.zeros_like(g)
    for k in range(5):
        sl = slice(k, 5) if suffix else slice(0, k + 1)
        flat = g[..., sl].reshape(-1, g[..., sl].shape[-1])
        ref[..., k] = np.array([math.fsum(r) for r in flat]).reshape(g.shape[:-1])
        mag[..., k] = np.array([math.fsum(np.abs(r)) for r in flat]).reshape(g.shape[:-1])
    return ref.reshape(v.shape), mag.reshape(v.shape)


def check_seg8_scan(what, v, out, suffix, exact):
    """lanes 0..4 of every group, all three rounds on the same carrier: exact for integers, else within gamma_3 sum |v| (three shifts)"""
    ref, mag = seg8_scan_reference(v, suffix)
    live = (np.arange(64) % 8) < 5
    o, r, m = out[..., live], ref[..., live], mag[..., live]
    if exact:
        assert np.array_equal(o, r), f"{what}: {int((o != r).sum())} lanes differ from the exact integer scan (rounds {sorted(set(np.argwhere(o != r)[:, 1]))})"
        print(f"[primcheck] {what}: integer scans bit-exact over three rounds")
        return
    err = np.abs(o - r)
    bound = gamma(3) * m + U * np.abs(r)
    report(what + " (error / gamma_3 bound)", float((err / np.maximum(bound, 1e-300)).max()), 1.0)
    assert (err <= bound).all(), f"{what}: over the gamma_3 bound in {int((err > bound).sum())} lanes"


def dpp_row_shift(v, old, shift, bank):
    """numpy model of one DPP row shift of 64 lanes (row_shl: shift > 0 reads lane i + shift; row_shr: shift < 0) with a bank mask and
    bound_ctrl: a lane whose bank is masked keeps `old`, a lane without a source in its row of 16 reads 0"""
    out = np.array(old, dtype=np.float64).copy()
    for i in range(64):
        r = i % 16
        if (bank >> (r // 4)) & 1:
            s = r + shift
            out[i] = v[i - r + s] if 0 <= s < 16 else 0.0
    return out


def model_seg8_suffix_sum(v, carrier):
    """hb_math.hpp seg8_suffix_sum on the numpy model; returns (result, carrier)"""
    v = np.array(v, dtype=np.float64)
    for sh in (1, 2, 4):
        carrier = dpp_row_shift(v, carrier, sh, 0x5)
        v = v + carrier
    return v, carrier


def model_seg8_prefix_sum(v, carrier):
    v = np.array(v, dtype=np.float64)
    for sh in (1, 2):
        v = v + dpp_row_shift(v, np.zeros(64), -sh, 0xf)
    carrier = dpp_row_shift(v, carrier, -4, 0xa)
    return v + carrier, carrier


def rotation(rng):
    """a random rotation matrix (f64 entries, orthogonal to rounding)"""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def prefix_product_inputs(ncases, rng):
    """[ncases][9][64]: lane k < 5 of a group holds a random rotation (row-major entries e), lanes 5..7 the identity"""
    m = np.zeros((ncases, 64, 3, 3))
    for c in range(ncases):
        for l in range(64):
            m[c, l] = rotation(rng) if l % 8 < 5 else np.eye(3)
    return np.ascontiguousarray(m.reshape(ncases, 64, 9).transpose(0, 2, 1))


def check_prefix_product(what, inp, out):
    """lane k < 5 holds M_0 ... M_k in that order (non-commuting inputs decide the order), against mpmath within 16 u per entry: five
    products of orthogonal matrices, each entry a three-term dot product (gamma_3 per product, entries bounded by 1)"""
    ncases = inp.shape[0]
    m = inp.transpose(0, 2, 1).reshape(ncases, 64, 3, 3)
    o = out.transpose(0, 2, 1).reshape(ncases, 64, 3, 3)
    worst = 0.0
    for c in range(ncases):
        for g in range(8):
            P = MP.eye(3)
            for k in range(5):
                P = P * MP.matrix(m[c, 8 * g + k].tolist())
                for i in range(3):
                    for j in range(3):
                        worst = max(worst, abs(float(MP.mpf(float(o[c, 8 * g + k, i, j])) - P[i, j])))
    report(what, worst, 16 * U)
    assert worst <= 16 * U, f"{what}: {worst} > 16 u"


# ------------------------------------------------------------------------------------------------------------------ tile GEMMs
OFF_A, OFF_B, OFF_C = 0, 1024, 2560     # operand regions of the 4096-word image (the largest: 860, 1536 and 1536 words)
SENTINEL = np.array([0x7FF8DEAD0000BEEF], dtype=np.uint64).view(np.float64)[0]


def slot_is_eq(s, cfm):
    """hb_lq.hpp slot_is_eq / slot_foot / slot_normal"""
    foot = (s >> 2) + 2 * ((s >> 1) & 1) if s < 8 else s - 8
    return s >= 8 or bool((cfm >> foot) & 1)


def tile_weights(d, cfm, sw):
    """(w[k], live[k]) of the call sites' masks: 0/1 on the equality rows under EqStepLive, sw on the soft rows under SoftStepLive"""
    K = d["K"]
    if d["WK"] == 0:
        return np.ones(K), np.ones(K, bool)
    if d["WK"] == 1:
        w = np.array([1.0 if slot_is_eq(k, cfm) else 0.0 for k in range(K)])
        live = np.array([(k // 4) == 2 or ((cfm >> (k // 4)) & 5) != 0 for k in range(K)])
    else:
        w = np.array([0.0 if slot_is_eq(k, cfm) else sw for k in range(K)])
        live = np.array([(k // 4) != 2 and ((~cfm >> (k // 4)) & 5) != 0 for k in range(K)])
    assert not (w[~live] != 0).any()      # a step that is ruled out has zero weights (the contract of step_live)
    return w, live


def tile_depth(d):
    """real depth of the contraction: KR where the product masks (KR < K); where it does not (KR == K) the operands are zero-padded in k,
    and the test leaves the last two k to the padding unless the product is weighted (all twelve slots are real there)"""
    if d["KR"] < d["K"]:
        return d["KR"]
    return d["K"] if d["WK"] else d["K"] - 2


def addr_A(d, i, k):
    return OFF_A + (k * d["LDA"] + i if d["TA"] else i * d["LDA"] + k)


def addr_B(d, k, j, tnb0=0):
    if d["MTB"]:
        return OFF_B + k * 16 * d["NTB"] + 16 * tnb0 + j
    return OFF_B + (j * d["LDB"] + k if d["TB"] else k * d["LDB"] + j)


def tile_image(d, Mr, Nr, A, B, C0, background, poison, cfm=0, sw=1.0, tnb0=0, transpose_A=False):
    """The 4096-word image of one case.  `background` fills every word no live element owns (random finite in the plain run).  With
    `poison`, every word the contracts call irrelevant is made hostile instead: NaN in rows >= Mr / columns >= Nr of the operands, in
    k >= KR where the product masks, behind a K-step that step_live rules out; 1e300 in the rows of Bt beyond the real depth.  Words the
    contracts require to be zero (the k-padding where KR == K) are zero in both.  transpose_A lays A out transposed ON PURPOSE (the
    host test shows the exact probes reject it)."""
    K, MT, NT = d["K"], d["MT"], d["NT"]
    mr, nr, depth = min(Mr, 16 * MT), min(Nr, 16 * NT), tile_depth(d)
    _, live = tile_weights(d, cfm, sw)
    img = np.array(background, dtype=np.float64).copy()
    if poison:
        img[:] = np.nan
    owner = np.zeros(len(img), np.int8)        # 1: required zero, 2: live element
    def put(addr, val, kind):
        assert 0 <= addr < len(img)
        assert not (owner[addr] == 2 and kind == 1) and not (owner[addr] == 1 and kind == 2), "a padding word collides with a live element"
        img[addr], owner[addr] = val, kind
    bacc = d["MTB"] > 0
    for k in range(K):
        real = k < depth
        for i in range(mr):
            a = addr_A(d, k, i) if transpose_A else addr_A(d, i, k)
            if real and live[k]:
                put(a, A[i, k], 2)
            elif real and not poison:
                put(a, A[i, k], 2)           # a ruled-out step: finite data in the plain run, NaN (untouched) in the poisoned one
            elif not real and d["KR"] == K:
                put(a, 0.0, 1)               # zero-padded in k
        for j in range(nr):
            b = addr_B(d, k, j, tnb0)
            if real and (live[k] or not poison):
                put(b, B[k, j], 2)
            elif not real and d["KR"] == K:
                if bacc:
                    put(b, 1e300 if poison else B[k, j], 2)   # rows of Bt beyond the real depth: finite, not zero
                else:
                    put(b, 0.0, 1)
    if bacc and poison:
        # the accumulators of the earlier product are all "live" for its own initialiser; columns outside [16 tnb0, 16 tnb0 + nr) only
        # feed discarded outputs and rows >= K are never contracted over: NaN stays
        pass
    for i in range(mr):
        for j in range(nr):
            put(OFF_C + i * 16 * NT + j, C0[i, j], 2)
    return img


def tile_operands(d, Mr, Nr, rng, kind):
    """A [16 MT][K], B [K][16 NT], C0 [16 MT][16 NT]: small integers (every partial sum exact) or f64 spread over 12 decades"""
    K, M, N = d["K"], 16 * d["MT"], 16 * d["NT"]
    if kind == "int":
        return (rng.integers(-8, 9, (M, K)).astype(np.float64), rng.integers(-8, 9, (K, N)).astype(np.float64),
                rng.integers(-50, 51, (M, N)).astype(np.float64))
    f = lambda shape: rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-6.0, 6.0, shape)   # noqa: E731
    return f((M, K)), f((K, N)), f((M, N))


def to_int(x):
    """f64 array -> (object array of Python ints I, s) with x = I * 2^s exactly"""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    mi = (m * 2.0 ** 53).astype(np.int64).astype(object)
    ex = np.where(mi == 0, 0, e - 53)
    s = int(ex.min()) if ex.size else 0
    sh = (ex - s).astype(object)
    return mi * (2 ** sh), s


def tile_exact(d, Mr, Nr, A, B, C0, cfm=0, sw=1.0):
    """C0 + sum_k w(k) A(i, k) B(k, j) over the real depth and the live steps, exactly (integer arithmetic on the mantissas, Fractions
    at the end); and |C0| + |A| |w| |B|.  The weights are 0, 1 or a power of two, so w(k) A(i, k) is exact in f64."""
    mr, nr, depth = min(Mr, 16 * d["MT"]), min(Nr, 16 * d["NT"]), tile_depth(d)
    w, live = tile_weights(d, cfm, sw)
    assert all(v == 0.0 or math.frexp(v)[0] == 0.5 for v in w)
    ks = [k for k in range(depth) if live[k] and w[k] != 0.0]
    Ai, sa = to_int(A[:mr, ks] * w[ks][None, :])
    Bi, sb = to_int(B[ks, :nr])
    Ci, sc = to_int(C0[:mr, :nr])
    fa, fc = Fraction(2) ** (sa + sb), Fraction(2) ** sc
    P = Ai @ Bi if ks else np.zeros((mr, nr), dtype=object)
    Pm = np.abs(Ai) @ np.abs(Bi) if ks else np.zeros((mr, nr), dtype=object)
    C = [[Fraction(int(P[i, j])) * fa + Fraction(int(Ci[i, j])) * fc for j in range(nr)] for i in range(mr)]
    mag = [[Fraction(int(Pm[i, j])) * fa + Fraction(abs(int(Ci[i, j]))) * fc for j in range(nr)] for i in range(mr)]
    return C, mag


def tile_dst_blank(P, ncases):
    return np.full((ncases, P.TILE_DST), SENTINEL)


def tile_split_dst(d, Mr, Nr, dst):
    """(live block [mr][nr], mask of the words of the destination outside it)"""
    mr, nr, ldd = min(Mr, 16 * d["MT"]), min(Nr, 16 * d["NT"]), 16 * d["NT"] + 3
    idx = (np.arange(mr)[:, None] * ldd + np.arange(nr)[None, :]).ravel()
    outside = np.ones(len(dst), bool)
    outside[idx] = False
    return dst[idx].reshape(mr, nr), outside


def check_sentinel(what, d, Mr, Nr, dst):
    _, outside = tile_split_dst(d, Mr, Nr, dst)
    hit = dst.view(np.uint64)[outside] != SENTINEL.view(np.uint64)
    assert not hit.any(), f"{what}: {int(hit.sum())} destination words outside the live {Mr} x {Nr} block were written"


def check_tile_exact(what, d, Mr, Nr, dst, C):
    """the live block equals the exact (integer) product bit for bit; everything else still holds the sentinel"""
    blk, _ = tile_split_dst(d, Mr, Nr, dst)
    ref = np.array([[float(v) for v in row] for row in C])
    assert all(Fraction(float(r)) == v for row, rr in zip(C, ref) for v, r in zip(row, rr)), "the probe is not exactly representable"
    bad = blk.view(np.uint64) != (ref + 0.0).view(np.uint64)
    bad &= ~((blk == 0.0) & (ref == 0.0))     # (+0 and -0 are the same integer)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {blk.size} elements differ from the exact product, first at {np.argwhere(bad)[0]}: {blk[tuple(np.argwhere(bad)[0])]} != {ref[tuple(np.argwhere(bad)[0])]}"
    check_sentinel(what, d, Mr, Nr, dst)


def check_tile_rounding(what, d, Mr, Nr, dst, C, mag):
    """|err_ij| <= gamma_(K+1) (|C0| + |A||B|)_ij against the exact product: K fused multiply-adds of the matrix cores (or K products
    and K additions of the host loops, with the weight's product) after the start value"""
    blk, _ = tile_split_dst(d, Mr, Nr, dst)
    g = gamma(d["K"] + 1)
    worst = 0.0
    for i, row in enumerate(C):
        for j, v in enumerate(row):
            assert math.isfinite(blk[i, j]), f"{what}: element ({i}, {j}) is {blk[i, j]}"
            err, bound = abs(Fraction(float(blk[i, j])) - v), g * float(mag[i][j])
            worst = max(worst, float(err) / bound if bound else (0.0 if err == 0 else math.inf))
    report(what + f" (error / gamma_{d['K'] + 1} bound)", worst, 1.0)
    assert worst <= 1.0, f"{what}: {worst} of the bound"
    check_sentinel(what, d, Mr, Nr, dst)


# ------------------------------------------------------------------------------------------------------------------ QP factorisation
def mp_array(a):
    """f64 array -> object array of 200-bit mpf (numpy's object loops then run the matrix products in mpmath)"""
    a = np.asarray(a, dtype=np.float64)
    return np.array([MP.mpf(float(v)) for v in a.ravel()], dtype=object).reshape(a.shape)


def mp_absmax(a):
    return max((abs(v) for v in np.asarray(a, dtype=object).ravel()), default=MP.mpf(0))


QF_KINDS = ("random", "zero column", "equal columns", "scaled rows")


def factor_matrix(kind, mA, n, rng):
    A = rng.normal(size=(mA, n))
    if kind == "zero column" and mA:
        A[:, n // 3] = 0.0
    if kind == "equal columns" and mA:
        A[:, n - 2] = A[:, 1]
    if kind == "scaled rows" and mA:
        A *= (10.0 ** np.linspace(-4.0, 4.0, mA))[:, None]     # rows scaled over 8 decades
    return A


def factor_cases(which, mA, rng):
    """the cases of one instantiation at one mA: every kind x every se.  which 0: regularised_factor<18, false>, UniformDiag, n = 16
    (R in a 38-wide block, 16 columns stored: hb_wbc.hpp); which 1: <24, true>, HeadTailDiag, n = 12, ld 12 (hb_hoqp.hpp small_lsqp)."""
    n, lda, ld, wstore = (16, 16, 38, 16) if which == 0 else (12, 12, 12, 12)
    cases = []
    for kind in QF_KINDS:
        for se in (1e-4, 1e-5, 1.0):
            A = factor_matrix(kind, mA, n, rng)
            b = rng.normal(size=mA)
            diag = (se, 0.0, 0) if which == 0 else (math.sqrt(se * se + 1e-12), se, n // 2)   # (head: shifted like a cascade level's z block)
            cases.append({"kind": kind, "se": se, "uniform": which == 0, "A": A, "b": b, "n": n, "mA": mA, "lda": lda, "ld": ld, "wstore": wstore, "diag": diag})
    return cases


def factor_run(P, which, cases):
    nc = len(cases)
    A, b = np.zeros((nc, P.QF_A)), np.zeros((nc, 32))
    par, dpar = np.zeros((nc, 8), np.int32), np.zeros((nc, 2))
    for c, cs in enumerate(cases):
        blk = np.zeros((P.QF_A // cs["lda"], cs["lda"]))
        blk[:cs["mA"], :cs["n"]] = cs["A"]
        A[c, :blk.size] = blk.ravel()
        b[c, :cs["mA"]] = cs["b"]
        par[c, :6] = [cs["n"], cs["mA"], cs["lda"], cs["ld"], cs["wstore"], cs["diag"][2]]
        dpar[c] = cs["diag"][:2]
    blank = np.full((nc, P.QF_R), SENTINEL)
    R, J, g, diag = P.regularised_factor(which, A, b, par, dpar, blank, blank, np.full((nc, 16), SENTINEL))
    return R, J, g, diag


def factor_diag_vector(cs):
    se, tail, n_head = cs["diag"]
    return np.array([se if (cs["uniform"] or k < n_head) else tail for k in range(cs["n"])])


def factor_properties(cs, Rw, Jw, gw, diag, negative_diagonal, grad):
    """structure (asserted) and the measured figures of one case: (residual |R'R - (A'A + D^2)|_max / |A'A + D^2|_max in mpmath,
    invert_upper's worst |J R - I|_ij / ((n + 2) u (|J||R|)_ij), and the same for |R J - I| against |R||J|).
    invert_upper solves R x = e_col column by column by back substitution, so it is the RIGHT residual that rounding-error analysis
    bounds componentwise: (R + dR) x = e_col with |dR| <= gamma_n |R| (Higham, Theorem 8.5; the reciprocal's second half-ulp makes it
    n + 2), hence |R J - I| <= (n + 2) u |R||J|.  The left residual J R - I carries a factor cond(R) more in general."""
    n, ld, ws = cs["n"], cs["ld"], cs["wstore"]
    what = f"{cs['kind']}, mA {cs['mA']}, se {cs['se']}"
    R, J = Rw[:n * ld].reshape(n, ld), Jw[:n * ld].reshape(n, ld)
    sent = SENTINEL.view(np.uint64)
    assert (Rw[n * ld:].view(np.uint64) == sent).all() and (R[:, ws:].view(np.uint64) == sent).all(), f"{what}: R written outside wstore"
    Rt = R[:, :n]
    assert np.isfinite(Rt).all(), f"{what}: R not finite"
    assert (np.tril(Rt, -1) == 0.0).all() and (R[:, n:ws] == 0.0).all(), f"{what}: R is not exactly zero outside the triangle"
    if negative_diagonal:
        assert (np.diag(Rt) < 0.0).all(), f"{what}: the diagonal of the Householder factor is negative by construction"
        assert np.array_equal(diag[:n], np.diag(Rt)), f"{what}: the returned value is not R_jj"
    else:
        assert (np.diag(Rt) != 0.0).all()
    Rm, Am = mp_array(Rt), mp_array(cs["A"])
    H = Am.T @ Am if cs["mA"] else np.full((n, n), MP.mpf(0), dtype=object)
    H = H + np.diag(mp_array(factor_diag_vector(cs)) ** 2)
    resid = float(mp_absmax(Rm.T @ Rm - H) / mp_absmax(H))
    if grad:
        gref = Am.T @ mp_array(cs["b"]) if cs["mA"] else np.full(n, MP.mpf(0), dtype=object)
        gmag = np.abs(cs["A"]).T @ np.abs(cs["b"]) if cs["mA"] else np.zeros(n)
        gerr = np.array([abs(float(MP.mpf(float(gw[j])) - gref[j])) for j in range(n)])
        assert (gerr <= gamma(max(cs["mA"], 1)) * gmag).all(), f"{what}: g = A'b off by {gerr.max()} (gamma_mA |A'||b| = {gamma(max(cs['mA'], 1)) * gmag})"
    # invert_upper
    Jt = J[:, :n]
    assert np.isfinite(Jt).all() and (np.tril(Jt, -1) == 0.0).all(), f"{what}: J below the diagonal must be exactly zero"
    Jm = mp_array(Jt)
    E = Jm @ Rm - np.diag([MP.mpf(1)] * n)
    bound = (n + 2) * U * (np.abs(Jt) @ np.abs(Rt))
    inv_ratio = max(float(abs(E[i, j])) / bound[i, j] for i in range(n) for j in range(n) if bound[i, j] > 0)
    assert all(E[i, j] == 0 for i in range(n) for j in range(n) if bound[i, j] == 0)
    Er = Rm @ Jm - np.diag([MP.mpf(1)] * n)
    bound_r = (n + 2) * U * (np.abs(Rt) @ np.abs(Jt))
    right_ratio = max(float(abs(Er[i, j])) / bound_r[i, j] for i in range(n) for j in range(n) if bound_r[i, j] > 0)
    assert all(Er[i, j] == 0 for i in range(n) for j in range(n) if bound_r[i, j] == 0)
    return resid, inv_ratio, right_ratio


def mp_givens_insert_row(R, npv):
    """hb_qpfactor.hpp givens_insert_row in mpmath (object arrays, in place)"""
    n = len(npv)
    for k in range(n):
        a, b = R[k, k], npv[k]
        if b != 0:
            rh = 1 / MP.sqrt(a * a + b * b)
            cc, ss = a * rh, b * rh
            for j in range(k, n):
                t1, t2 = R[k, j], npv[j]
                R[k, j], npv[j] = cc * t1 + ss * t2, -ss * t1 + cc * t2


def mp_drop_constraint(R, J, l, q):
    """hb_qpfactor.hpp drop_constraint in mpmath: R q x q (in an n x n block), J n x n; returns the new q"""
    n = J.shape[0]
    for j in range(l, q - 1):
        for i in range(j + 2):
            R[i, j] = R[i, j + 1]
    for i in range(q):
        R[i, q - 1] = MP.mpf(0)
    q -= 1
    for j in range(l, q):
        a, b = R[j, j], R[j + 1, j]
        if b != 0:
            rh = 1 / MP.sqrt(a * a + b * b)
            cc, ss = a * rh, b * rh
            for k in range(n):
                if j <= k < q:
                    t1, t2 = R[j, k], R[j + 1, k]
                    R[j, k], R[j + 1, k] = cc * t1 + ss * t2, -ss * t1 + cc * t2
                u1, u2 = J[k, j], J[k, j + 1]
                J[k, j], J[k, j + 1] = cc * u1 + ss * u2, -ss * u1 + cc * u2
        R[j + 1, j] = MP.mpf(0)
    return q


def mp_distance(x, ref):
    """max |x - ref| / max |ref|, x f64, ref mpf"""
    return float(mp_absmax(mp_array(x) - ref) / mp_absmax(ref))


# ------------------------------------------------------------------------------------------------------------------ scenarios
# (instantiation id of tests/gpu_unit/prim_cases.hpp, Mr, Nr, tnb0, call site): exactly the (Mr, Nr) pairs the product passes
TILE_SITES = [
    (0, 22, 32, 0, "hb_riccati.hpp ric_phase1, NTW 2"), (1, 22, 36, 0, "hb_riccati.hpp ric_phase1, NTW 3"),
    (2, 12, 32, 0, "hb_riccati.hpp ric_phase2_gemm, NTW 2"), (3, 12, 36, 0, "hb_riccati.hpp ric_phase2_gemm, NTW 3"),
    (2, 16, 23, 0, "hb_riccati.hpp ric_phase3_mma t0 bacc"), (4, 6, 7, 1, "hb_riccati.hpp ric_phase3_mma t1 bacc"),
    (5, 16, 23, 0, "hb_riccati.hpp ric_phase3_mma t0"), (6, 6, 7, 0, "hb_riccati.hpp ric_phase3_mma t1"),
    (7, 16, 16, 0, "hb_kernels.hip GEMM 1"), (7, 6, 16, 0, "hb_kernels.hip GEMM 1, rows 16.."), (8, 16, 36, 0, "hb_kernels.hip GEMM 1 wide"),
    (8, 6, 36, 0, "hb_kernels.hip GEMM 1 wide, rows 16.."), (7, 16, 4, 0, "hb_kernels.hip GEMM 1 wide, columns 32.."),
    (7, 6, 4, 0, "hb_kernels.hip GEMM 1 wide, last tile"),
    (9, 12, 32, 0, "hb_kernels.hip GEMM 2, w 0"), (9, 12, 16, 0, "hb_kernels.hip GEMM 2, w 1"), (9, 12, 36, 0, "hb_kernels.hip GEMM 2 wide, w 0"),
    (9, 12, 20, 0, "hb_kernels.hip GEMM 2 wide, w 1"), (9, 12, 4, 0, "hb_kernels.hip GEMM 2 wide, w 2"),
    (9, 16, 16, 0, "hb_kernels.hip GEMM 3 (0, 0)"), (9, 16, 7, 0, "hb_kernels.hip GEMM 3 (0, 1)"), (9, 6, 7, 0, "hb_kernels.hip GEMM 3 (1, 1)"),
    (6, 16, 16, 0, "hb_kernels.hip GEMM 3 rest (0, 0)"), (6, 16, 7, 0, "hb_kernels.hip GEMM 3 rest (0, 1)"), (6, 6, 7, 0, "hb_kernels.hip GEMM 3 rest (1, 1)"),
    (10, 29, 9, 0, "hb_lq.hpp:549"), (11, 10, 32, 0, "hb_lq.hpp:605"), (12, 12, 29, 0, "hb_lq.hpp:838"), (13, 10, 32, 0, "hb_lq.hpp:1109"),
    (14, 10, 29, 0, "hb_lq.hpp:1124"), (13, 16, 22, 0, "hb_lq.hpp:1141"), (15, 6, 6, 0, "hb_lq.hpp:1142"), (16, 16, 23, 0, "hb_lq.hpp:1147"),
    (17, 6, 7, 0, "hb_lq.hpp:1148"), (18, 16, 23, 0, "hb_lq.hpp:1149"), (19, 6, 7, 0, "hb_lq.hpp:1150"), (16, 6, 29, 0, "hb_lq.hpp:1171"),
]
TILE_SITE_IDS = [f"{s[4]} [{s[0]}: {s[1]}x{s[2]}]".replace(" ", "_") for s in TILE_SITES]
CFMS = (0, 5, 10, 15, 6, 9)     # contact-flag masks: none, one leg, the other, both, mixed


def site_cfms(d):
    return CFMS if d["WK"] else (0,)


def run_tile(P, tid, d, cases, sw):
    """cases: dicts Mr, Nr, A, B, C0, background, poison, cfm, tnb0 (+ transpose_A) -> destination rows"""
    img = np.stack([tile_image(d, c["Mr"], c["Nr"], c["A"], c["B"], c["C0"], c["background"], c["poison"], c["cfm"], sw, c["tnb0"],
                               c.get("transpose_A", False)) for c in cases])
    par = np.array([[OFF_A, OFF_B, OFF_C, c["Mr"], c["Nr"], c["cfm"], c["tnb0"], 0] for c in cases], np.int32)
    return P.tile_mma(tid, img, par, sw, tile_dst_blank(P, len(cases)))


def tile_exact_scenario(P, site, seed=21, transpose_A=False):
    """integer operands: the live block equals the exact product bit for bit, nothing else is written, and the poisoned image gives the
    same bits as the plain one"""
    tid, Mr, Nr, tnb0, name = site
    d, rng, sw = P.tile_desc(tid), np.random.default_rng(seed + tid), 2.0
    cases = []
    for cfm in site_cfms(d):
        A, B, C0 = tile_operands(d, Mr, Nr, rng, "int")
        bg = rng.normal(size=P.TILE_LDS) * 100.0
        for poison in (False, True):
            cases.append({"Mr": Mr, "Nr": Nr, "A": A, "B": B, "C0": C0, "background": bg, "poison": poison, "cfm": cfm, "tnb0": tnb0,
                          "transpose_A": transpose_A})
    dst = run_tile(P, tid, d, cases, sw)
    for c, out in zip(cases, dst):
        C, _ = tile_exact(d, Mr, Nr, c["A"], c["B"], c["C0"], c["cfm"], sw)
        check_tile_exact(f"{name} cfm {c['cfm']}{' poisoned' if c['poison'] else ''}", d, Mr, Nr, out, C)
    for k in range(0, len(cases), 2):
        check_bits_equal(f"{name} cfm {cases[k]['cfm']}: poisoned vs plain", dst[k + 1], dst[k])


def tile_unit_scenario(P, site, transpose_A=False):
    """A = E_ik, B = E_kj -> C = w(k) E_ij for a handful of (i, k, j), the last live row, column and k among them: pins the transposes,
    the leading dimensions and tnb0"""
    tid, Mr, Nr, tnb0, name = site
    d, sw = P.tile_desc(tid), 2.0
    mr, nr = min(Mr, 16 * d["MT"]), min(Nr, 16 * d["NT"])
    cfm = {0: 0, 1: 15, 2: 0}[d["WK"]]
    w, live = tile_weights(d, cfm, sw)
    ks = [k for k in range(tile_depth(d)) if live[k] and w[k] != 0.0]
    probes = sorted({(0, ks[0], 0), (mr - 1, ks[-1], nr - 1), (mr - 1, ks[0], 0), (0, ks[-1], 0), (0, ks[0], nr - 1), (mr // 2, ks[len(ks) // 2], nr // 2),
                     (min(mr - 1, 1), ks[min(len(ks) - 1, 2)], min(nr - 1, 3))})
    cases = []
    for i, k, j in probes:
        A, B = np.zeros((16 * d["MT"], d["K"])), np.zeros((d["K"], 16 * d["NT"]))
        A[i, k], B[k, j] = 1.0, 1.0
        cases.append({"Mr": Mr, "Nr": Nr, "A": A, "B": B, "C0": np.zeros((16 * d["MT"], 16 * d["NT"])), "background": np.zeros(P.TILE_LDS),
                      "poison": False, "cfm": cfm, "tnb0": tnb0, "transpose_A": transpose_A})
    dst = run_tile(P, tid, d, cases, sw)
    for (i, k, j), c, out in zip(probes, cases, dst):
        C, _ = tile_exact(d, Mr, Nr, c["A"], c["B"], c["C0"], cfm, sw)
        assert C[i][j] == Fraction(float(w[k])) and sum(v != 0 for row in C for v in row) == 1
        check_tile_exact(f"{name} E_{i},{k} E_{k},{j}", d, Mr, Nr, out, C)


def tile_rounding_scenario(P, site, seed=22):
    """operands spread over 12 decades against the exact product.  (The soft weight is a power of two here, so that the weight's
    product adds no rounding of its own and the bound is gamma_(K+1) as for the plain products.)"""
    tid, Mr, Nr, tnb0, name = site
    d, rng, sw = P.tile_desc(tid), np.random.default_rng(seed + tid), 0.25
    cases = []
    for cfm in site_cfms(d)[:3]:
        A, B, C0 = tile_operands(d, Mr, Nr, rng, "f64")
        cases.append({"Mr": Mr, "Nr": Nr, "A": A, "B": B, "C0": C0, "background": np.zeros(P.TILE_LDS), "poison": True, "cfm": cfm, "tnb0": tnb0})
    dst = run_tile(P, tid, d, cases, sw)
    for c, out in zip(cases, dst):
        C, mag = tile_exact(d, Mr, Nr, c["A"], c["B"], c["C0"], c["cfm"], sw)
        check_tile_rounding(f"{name} cfm {c['cfm']}", d, Mr, Nr, out, C, mag)


RT_SHAPES = [(Mr, Nr) for Mr in (1, 6, 16, 22) for Nr in (1, 7, 23, 32, 36)]


def tile_roundtrip_scenario(P, Mr, Nr, seed=23):
    """every initialiser and store, one case each, against numpy; nothing outside the window is written and no initialiser / pre / column
    function is called with an index outside the live range"""
    import _gpuunit
    rng = np.random.default_rng(seed + 100 * Mr + Nr)
    LD, LDD, W = P.RT_LD, P.RT_LDD, P.RT_WORDS
    a2, b2 = rng.normal(size=(32, LD)), rng.normal(size=(32, LD))
    a, b = np.zeros(W), np.zeros(W)
    a[:32 * LD], b[:32 * LD] = a2.ravel(), b2.ravel()
    vec = b[:32]
    scale = 1.7
    live = np.zeros((32, 48), bool)
    live[:Mr, :Nr] = True
    az = np.where(live, a2[:, :48], 0.0)      # the accumulators after tile_init_rm: zero outside Mr x Nr
    bz = np.where(live, b2[:, :48], 0.0)
    csel, c0 = Nr - 1, Nr // 3
    c1, c1w = min(Nr, c0 + max(1, Nr // 2)), min(48, Nr + 2)
    col = np.zeros((32, 48))
    col[:Mr, csel] = vec[:Mr]
    setc = az.copy()
    setc[:Mr, Nr // 2] = vec[:Mr]
    win = lambda lo, hi: (np.arange(48)[None, :] >= lo) & (np.arange(48)[None, :] < hi) & (np.arange(32)[:, None] < Mr)   # noqa: E731
    ops = [("tile_init", 0, 0, 1.0, az, live), ("tile_init_rm", 0, 0, scale, scale * az, live), ("tile_init_col", csel, 0, scale, scale * col, live),
           ("tile_set_col", Nr // 2, 0, scale, scale * setc, live), ("tile_add", 0, 0, scale, scale * (az + bz), live),
           ("tile_store_pre", 0, 0, 1.0, az + 2.0 * bz, live), ("tile_store_rm_cols", c0, c1, scale, scale * az, win(c0, c1)),
           ("tile_store_rm_cols", c0, c1w, scale, scale * az, win(c0, c1w))]
    for name, p0, p1, sc, ref, mask in ops:      # (the scale is an argument of the launch: one launch per value is simplest)
        par = np.array([[_gpuunit.RT_OPS[name], Mr, Nr, p0, p1, 0, 0, 0]], np.int32)
        dst, flag = P.tile_roundtrip(a[None], b[None], par, sc, np.full((1, W), SENTINEL))
        assert flag[0] == 0, f"{name} {Mr} x {Nr}: {flag[0]} calls with an index outside the live range"
        got = np.full((32, 48), SENTINEL)
        rows = dst[0][:32 * LDD].reshape(32, LDD)
        got[:, :] = rows[:, :48]
        want = np.where(mask, ref, SENTINEL)
        bad = got.view(np.uint64) != want.view(np.uint64)
        bad &= ~((got == 0.0) & (want == 0.0))
        assert not bad.any(), f"{name} {Mr} x {Nr} (p0 {p0}, p1 {p1}): {int(bad.sum())} words differ, first at {np.argwhere(bad)[0]}"
        rest = np.concatenate([rows[:, 48:].ravel(), dst[0][32 * LDD:]])
        assert (rest.view(np.uint64) == SENTINEL.view(np.uint64)).all(), f"{name} {Mr} x {Nr}: written outside the tile block"
    print(f"[primcheck] tile round trips {Mr} x {Nr}: {len(ops)} initialiser / store forms bit-equal to numpy")


def factor_scenario(P, which, mA, twin=None, seed=24):
    """regularised_factor + invert_upper of one instantiation at one mA over every kind x se.  Structure and g are asserted on P's output;
    the residual is measured on P and on the twin, the same way; returns [(case, residual, twin residual, invert_upper's left ratio, its
    right ratio)]"""
    rng = np.random.default_rng(seed + 10 * which + mA)
    cases = factor_cases(which, mA, rng)
    out = factor_run(P, which, cases)
    tw = factor_run(twin, which, cases) if twin is not None else None
    rows = []
    for c, cs in enumerate(cases):
        r, inv, inv_r = factor_properties(cs, out[0][c], out[1][c], out[2][c], out[3][c], negative_diagonal=P.on_device, grad=which == 1)
        rt = factor_properties(cs, tw[0][c], tw[1][c], tw[2][c], tw[3][c], negative_diagonal=False, grad=which == 1)[0] if tw else None
        rows.append((cs, r, rt, inv, inv_r))
    return rows


def random_factor(n, q, rng):
    """an upper triangular q x q factor with the negative diagonal of the device's Householder form, in an n x n block"""
    R = np.zeros((n, n))
    R[:q, :q] = np.triu(rng.normal(size=(q, q)))
    R[np.arange(q), np.arange(q)] = -(0.5 + np.abs(rng.normal(size=q)))
    return R


def givens_cases(rng):
    cases = []
    for n, ld in ((12, 12), (16, 38)):
        for zero_at in (None, 0, n // 2):
            npv = rng.normal(size=n)
            if zero_at is not None:
                npv[zero_at] = 0.0        # (a zero entry skips its rotation)
            cases.append({"op": 0, "n": n, "ld": ld, "R": random_factor(n, n, rng), "np": npv})
    n, ld = 12, 12
    for q in (n, 5):
        for l in (0, q // 2, q - 1):
            J = rng.normal(size=(n, n)) + 3.0 * np.eye(n)
            cases.append({"op": 1, "n": n, "ld": ld, "q": q, "l": l, "R": random_factor(n, q, rng), "J": J, "act": rng.permutation(40)[:q],
                          "lam": rng.normal(size=q)})
    return cases


def givens_run(P, cases):
    nc = len(cases)
    par = np.zeros((nc, 8), np.int32)
    R, J = np.zeros((nc, P.QF_R)), np.zeros((nc, P.QF_R))
    npv, lam = np.zeros((nc, 64)), np.zeros((nc, 64))
    act, isa = np.zeros((nc, 64), np.int32), np.ones((nc, 64), np.int32)
    for c, cs in enumerate(cases):
        n, ld = cs["n"], cs["ld"]
        par[c, :5] = [cs["op"], n, ld, cs.get("l", 0), cs.get("q", 0)]
        blk = np.zeros((n, ld))
        blk[:, :n] = cs["R"]
        R[c, :n * ld] = blk.ravel()
        if cs["op"] == 0:
            npv[c, :n] = cs["np"]
        else:
            blk = np.zeros((n, ld))
            blk[:, :n] = cs["J"]
            J[c, :n * ld] = blk.ravel()
            act[c, :cs["q"]], lam[c, :cs["q"]] = cs["act"], cs["lam"]
    return P.givens(par, R, J, npv, act, isa, lam)


def givens_measure(cases, out):
    """per case: (distance of R (and J) from the same algorithm in mpmath, |J'N - [R; 0]| / |R| after a drop or None, bookkeeping)"""
    par, R, J, npv, act, isa, lam = out
    rows = []
    for c, cs in enumerate(cases):
        n, ld = cs["n"], cs["ld"]
        Rg = R[c][:n * ld].reshape(n, ld)[:, :n]
        if cs["op"] == 0:
            Rm, nm = mp_array(cs["R"]), mp_array(cs["np"])
            mp_givens_insert_row(Rm, nm)
            assert (np.tril(Rg, -1) == 0.0).all()
            rows.append((mp_distance(Rg, Rm), None, None))
            continue
        q, l = cs["q"], cs["l"]
        Jg = J[c][:n * ld].reshape(n, ld)[:, :n]
        Rm, Jm = mp_array(cs["R"]), mp_array(cs["J"])
        # N with J'N = [R; 0] for the incoming pair, in mpmath: N = J^-T [R; 0]
        N = MP.inverse(MP.matrix(cs["J"].T.tolist())) * MP.matrix(cs["R"][:, :q].tolist())
        N = np.array([[N[i, j] for j in range(q) if j != l] for i in range(n)], dtype=object)
        q2 = mp_drop_constraint(Rm, Jm, l, q)
        assert par[c, 4] == q2 == q - 1
        assert (np.tril(Rg, -1) == 0.0).all() and (Rg[:, q2:] == 0.0).all()
        dist = max(mp_distance(Rg, Rm), mp_distance(Jg, Jm))
        RN = mp_array(Jg).T @ N - mp_array(Rg[:, :q2])
        book = (act[c][:q2].tolist(), lam[c][:q2].tolist(), isa[c].tolist())
        want = (np.delete(cs["act"], l).tolist(), np.delete(cs["lam"], l).tolist())
        assert book[:2] == want and isa[c][cs["act"][l]] == 0 and isa[c].sum() == 63, "working-set records after the drop"
        rows.append((dist, float(mp_absmax(RN) / mp_absmax(Rm)), book))
    return rows
