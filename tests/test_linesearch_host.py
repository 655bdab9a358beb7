"""CPU: what entitles the twin of the filter line search (tests/_lstwin.py) to judge the device, and the host floor of the node values.

  * The twin's walk, fed with the ORACLE's numbers (baseline from oracle.performance at the base point, Armijo term from node_lq's q, r
    and the oracle's step, trial values from oracle.performance, host arithmetic: nothing fused), gives exactly the step size of
    oracle.mpc_solve(..., iters=1) on every case of the matrix of tests/_lscases.py (P1 x seven settings x points a, b, c; P2 x three).
  * The matrix meets every condition of _lscases.CONDITIONS, from the oracle's walk alone.
  * node_value of the device header compiled for the host (tests/host_emu/hostemu.cpp emu_node_value), node by node, against the
    reference triple (oracle.performance on the one-interval slice of the trial point): at step size 1 for every instance and, for the
    instances the oracle's walk refuses there, at every step size of the last window it evaluates (settings ship, armijo, armijo_slow,
    gamma_slow).  Bound 1e-13 max(1, |expected|) per entry, as tests/test_lq_record_host.py holds the same three quantities at the base
    point.  Measured maxima over all nodes and step sizes, (dt cost, dt |defect|^2, dt |eq|^2):
        P1 (a) 3.3e-15 3.3e-19 5.8e-16   (b) 5.7e-15 3.8e-15 4.6e-15   (c) 1.7e-15 6.5e-23 7.6e-20   P2 (b) 4.0e-15 8.7e-18 1.2e-15
    This is the floor the GPU bound 1e-12 (tests/test_gpu_linesearch.py) stands 200 x above.
  * The reduction: wave_sum is device code of hb_kernels.hip (shfl_down), not a WaveCtx algorithm of a header, so the host emulator cannot
    run it; the twin's wave_sums is held here to an independent scalar restatement and to the exact sum, and on the GPU, bit for bit,
    to the sums the device reports (test_gpu_linesearch.py check D).
Smallest oracle-side margin of any inequality of any trial, (a) and (b) cases: 7.7e-7 (P1 armijo_slow (b)); at (c) down to 3.7e-14."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import _lscases as lc
import _lstwin as tw
from hunter_bipedal_control_amd import abi

BOUND = 1e-13
VALUE_CONFIGS = ("ship", "armijo", "armijo_slow", "gamma_slow")


@pytest.fixture(scope="module")
def matrix(params, oracle):
    return lc.Matrix(params, oracle)


@pytest.fixture(scope="module")
def emu():
    import _hostemu
    return C.CDLL(str(_hostemu.build()))


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_twin_walk_on_the_oracle_numbers_gives_the_oracle_step_size(params, matrix, case):
    from oracle.pyoracle import Oracle
    pt, walks = matrix.point(case[0], case[2]), matrix.walks(case)
    perf = Oracle(params, **lc.CONFIGS[case[1]]).mpc_solve(pt.refs, pt.x0, pt.x.copy(), pt.u.copy(), iters=1)
    print(f"{lc.case_id(case)}: {lc.summary(walks)}  smallest margin {min(w.margin for w in walks):.1e}")
    assert [w.alpha for w in walks] == perf[:, 3].tolist()
    for i, w in enumerate(walks):
        if w.cause == tw.ACCEPTED:    # and the sums it accepted on are the oracle's
            assert np.allclose(w.sums, perf[i, :3], rtol=1e-13, atol=0.0), (i, w.sums, perf[i])
        else:
            assert w.alpha == 0.0 and w.word in (0, 2)


def test_matrix_meets_the_input_conditions(matrix):
    hit = lc.conditions_met(matrix)
    for name, where in hit.items():
        print(f"{name}: {len(where)}  e.g. {where[:3]}")
    assert not [name for name, where in hit.items() if not where]
    margins = [w.margin for case in lc.CASES if case[2] != "c" for w in matrix.walks(case)]
    print(f"smallest margin over the (a) and (b) cases: {min(margins):.1e}")
    assert min(margins) >= lc.MARGIN     # every (a) / (b) decision of the device is held to the oracle's


def _emu_values(emu, params, pt, i, alpha):
    n, r = pt.n[i], pt.refs
    c = lambda a, dt=np.float64: np.ascontiguousarray(a, dtype=dt)   # noqa: E731
    p = lambda a: a.ctypes.data_as(C.c_void_p)                        # noqa: E731
    t, mode, xref, swing = c(r["t"][i, :n + 1]), c(r["mode"][i, :n], np.int32), c(r["x_ref"][i, :n]), c(r["swing"][i, :n]).reshape(n, 24)
    x, u, dx, du = c(pt.x[i, :n + 1]), c(pt.u[i, :n]), c(pt.dx[i, :n + 1]), c(pt.du[i, :n])
    out = np.zeros((n, 3))
    mdl, cfg = abi.make_model(params), abi.make_config(params)
    emu.emu_node_value(C.byref(mdl), C.byref(cfg), C.c_int(n), p(t), p(mode), p(xref), p(swing), p(x), p(u), p(dx), p(du), C.c_double(alpha), p(out))
    return out


@pytest.mark.parametrize("where", [("P1", "a"), ("P1", "b"), ("P1", "c"), ("P2", "b")], ids="-".join)
def test_host_node_value_matches_the_reference_at_the_trial_points(params, matrix, emu, where):
    pt = matrix.point(*where)
    trial = {(i, 1.0) for i in range(pt.B)}
    for name in VALUE_CONFIGS:
        if (where[0], name, where[1]) not in lc.CASES:
            continue
        wins = tw.windows(matrix.cfg(name))
        for i, w in enumerate(matrix.walks((where[0], name, where[1]))):
            if w.last_window >= 0:
                trial |= {(i, a) for a in wins[w.last_window][:w.rows]}
    worst = np.zeros(3)
    for i, alpha in sorted(trial):
        got = _emu_values(emu, params, pt, i, alpha)
        want = pt.node_values(i, pt.x[i] + alpha * pt.dx[i], pt.u[i] + alpha * pt.du[i])
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        worst = np.maximum(worst, err.max(axis=0))
        assert (err <= BOUND).all(), (where, i, alpha, np.argwhere(err > BOUND)[:3], err.max())
    print(f"host node_value {'-'.join(where)}: {len(trial)} (instance, step size) pairs, worst (cost, defect, eq) = " + " ".join(f"{v:.1e}" for v in worst))


# ---- the twin's own pieces ------------------------------------------------------------------------------------------------------------
def _lane_tree_scalar(values):
    """wave_sum restated lane by lane with Python floats: 64 accumulators, then v[l] += v[l + off] for all l at once, own value beyond 63."""
    v = [0.0] * 64
    for k, p in enumerate(values):
        v[k % 64] += float(p)
    off = 32
    while off:
        v = [v[lane] + (v[lane + off] if lane + off < 64 else v[lane]) for lane in range(64)]
        off //= 2
    return v[0]


@pytest.mark.parametrize("n", [1, 2, 60, 63, 64, 65, 70, 129, 200])
def test_wave_sums_is_the_lane_then_tree_order(n):
    rng = np.random.default_rng(n)
    p = rng.standard_normal((n, 3)) * 10.0 ** rng.integers(-8, 8, size=(n, 3))
    got = tw.wave_sums(p)
    for c in range(3):
        assert got[c] == _lane_tree_scalar(p[:, c])
        exact = float(sum(Fraction(float(v)) for v in p[:, c]))
        assert abs(got[c] - exact) <= n * 2.0 ** -52 * np.abs(p[:, c]).sum()
    if n >= 60:    # the order matters at this size: the sequential sum is another number in at least one column
        assert any(got[c] != float(np.add.accumulate(p[:, c])[-1]) for c in range(3))


def test_fma_and_norms_round_once():
    a = 1.0 + 2.0 ** -30
    assert tw.fma(a, a, -(a * a)) == 2.0 ** -60 and a * a - a * a == 0.0
    rng = np.random.default_rng(3)
    for n in (1, 60, 70):
        dx, du = rng.standard_normal((n + 2, 22)), rng.standard_normal((n + 1, 22))
        for fused in (True, False):
            nx, nu = tw.norms(dx, du, n, fused)
            assert abs(nx - math.sqrt(float(sum(Fraction(float(v)) ** 2 for v in dx[:n + 1].reshape(-1))))) <= 1e-13 * nx
            assert abs(nu - math.sqrt(float(sum(Fraction(float(v)) ** 2 for v in du[:n].reshape(-1))))) <= 1e-13 * nu
        # the row behind the last state, and the input row behind the last interval, are not part of the norms
        assert tw.norms(dx, du, n) != tw.norms(dx, du, n + 1)
    assert tw.committed([1.0, a], [a, a], a, [1.0 + a * a, tw.fma(a, a, a)]) and not tw.committed([1.0], [a], a, [np.nextafter(1.0 + a * a, 9.0)])


def test_windows_are_running_products_in_sixteens(params):
    ship = tw.windows(tw.config(params))
    assert [len(w) for w in ship] == [13] and ship[0][0] == 0.5 and ship[0][-1] == 0.5 ** 13
    slow = tw.windows(tw.config(params, alpha_decay=0.9))
    assert [len(w) for w in slow] == [16, 16, 16, 16, 16, 7]
    flat, a = [v for w in slow for v in w], 1.0
    for v in flat:
        a *= 0.9
        assert v == a
    assert any(v != 0.9 ** (k + 1) for k, v in enumerate(flat))      # a power is another number: the twin must not use one
    assert slow[1][0] != 0.9 and flat[-1] >= 1e-4 > flat[-1] * 0.9
    assert tw.windows(tw.config(params, alpha_decay=0.0)) == [] and tw.windows(tw.config(params, alpha_decay=1.0)) == []


def test_walk_rules(params):
    """The order of the rules on synthetic numbers: the deltaTol test before every tail trial and never before the full step, the stop
    below alpha_min, a Riccati failure that refuses what the filter accepts, the branch numbers."""
    cfg = tw.config(params)
    acc = np.array([-1.0, 10.0, 1.0, 0.0])                      # base violation 1 > g_max: branch 1
    better, worse = (9.0, 0.25, 0.0), (9.0, 4.0, 0.0)
    w = tw.walk(cfg, acc, lambda t: better, (0.0, 0.0))          # norms 0: below deltaTol, but the full step is tried first
    assert (w.cause, w.trial, w.alpha, w.branch, w.word, w.last_window) == (tw.ACCEPTED, 0, 1.0, 1, 1, -1)
    w = tw.walk(cfg, acc, lambda t: worse, (0.0, 0.0))
    assert (w.cause, w.trial, w.word, w.last_window, w.rows) == (tw.DELTA_TOL, 1, 2, 0, 0) and tw.expected_status(w) == 0
    w = tw.walk(cfg, acc, lambda t: worse, (1.0, 1.0))
    assert (w.cause, w.trial, w.word, w.last_window, w.rows) == (tw.ALPHA_MIN, 13, 0, 0, 13) and tw.expected_status(w) == 1
    w = tw.walk(cfg, acc, lambda t: better if t == 3 else worse, (1.0, 1.0))
    assert (w.cause, w.trial, w.alpha, w.sums) == (tw.ACCEPTED, 3, 0.125, better)
    w = tw.walk(cfg, acc, lambda t: better, (1.0, 1.0), ric_fail=True)
    assert (w.cause, w.word, w.alpha, w.first_ok) == (tw.RIC_FAIL, 0, 0.0, 0) and tw.expected_status(w, True) == 3
    w = tw.walk(cfg, acc, lambda t: worse, (1.0, 2e-4 / 0.5 ** 5))   # alpha |du| < 1e-4 from trial 6 on, alpha |dx| from trial 14: never both
    assert w.cause == tw.ALPHA_MIN
    w = tw.walk(cfg, acc, lambda t: worse, (1e-4 / 0.5 ** 5 * 0.99, 1e-4 / 0.5 ** 3 * 0.99))
    assert (w.cause, w.trial, w.rows) == (tw.DELTA_TOL, 5, 4)
    small = np.array([-1.0, 10.0, 1e-14, 0.0])                   # base violation 1e-7 < g_min
    assert tw.filter_accept(cfg, 10.0, 1e-7, 9.0, 1e-8, 1.0, -1.0) == (2, True)
    assert tw.filter_accept(cfg, 10.0, 1e-7, 10.0, 1e-8, 1.0, -1.0) == (2, False)       # merit not below base + 1e-4 * armijo
    assert tw.filter_accept(cfg, 10.0, 1e-7, 10.0, 1e-8, 1.0, 1.0) == (3, True)         # armijo > 0: the filter rule, less violation
    assert tw.filter_accept(cfg, 10.0, 1e-7, 10.0, 1e-4, 1.0, -1.0) == (3, False)
    assert tw.walk(cfg, small, lambda t: (9.0, 1e-16, 0.0), (1.0, 1.0)).branch == 2
