"""-m gpu: the filter line search of the device (k_ls_eval, k_ls_decide, k_ls_tail_eval, k_ls_tail_decide, node_value, filter_accept and the
window loop of enqueue_sqp), trial by trial, through hb_mpc_get_linesearch: values against the high-precision reference, decisions
against the exact twin tests/_lstwin.py fed with the DEVICE's own numbers, so that no tie can make a check flaky or forgiving.  The case
matrix, the oracle's side of it and the conditions it meets: tests/_lscases.py; what entitles the twin to judge: tests/test_linesearch_host.py.

One context per case (sqp_iterations = 1, the iterate set, one solve from x0 = x[:, 0]; the rows behind the horizon of the iterate hold a
sentinel).  Per case and instance:
  V  partial[k] at step size 1, and for an instance refused there every row of ls_tail the last evaluated window wrote (the twin says
     which: rows behind n_alpha or below the deltaTol stop are stale and skipped by rule), against oracle.performance on the one-interval
     slice of the trial point formed from the device's own step.  Bound 1e-12 max(1, |expected|) per entry.
  B  acc[1..3] = the sequential sum in node order of the record's cost dt, dyn_sse dt, eq_sse dt, bit for bit; acc[0] against
     sum_k qf_k'dx_k + rf_k'du_k within 1e-12 max(1, sum |terms|) (armijo settings: row and wave form of the forward sweep as well).
  D  the twin's walk on acc, wave_sums(partial), wave_sums of the last window's ls_tail rows (earlier windows: the oracle's sums, admissible
     where every inequality of the trial has an oracle-side relative margin >= 1e-7): the accepted word, perf[0..3], ls_norm and the status
     word bit for bit; where all margins of the instance hold, the oracle's step size as well.  An instance that needs an earlier window
     without that margin is not judged (point (c) only; counted and printed).
  C  the committed iterate: x + alpha dx entry by entry in one of the two admissible roundings (fused, or product then sum); untouched
     without a step; the rows behind n untouched.
  R  Riccati failure (indefinite R~): ric_fail = 1, accepted = 0, iterate unchanged, step 0, status NAN although the filter alone accepts.

Measured on an MI355X (maxima per problem and point over all settings, (dt cost, dt |defect|^2, dt |eq|^2); host floor in
tests/test_linesearch_host.py: 5.7e-15 3.8e-15 4.6e-15):
  P1 (a) 2.8e-15 2.7e-19 6.1e-16   (b) 6.6e-15 1.6e-14 4.3e-15   (c) 1.8e-15 7.3e-23 1.3e-19   P2 (b) 5.3e-15 6.9e-18 1.3e-15
The largest, 1.6e-14 (defect at (b), every setting), is four times the host floor and sixty times under the bound: the device forms the
trial point with a fused multiply-add, the reference from numpy's product and sum, and the defect is a difference of such entries.  No
bound is raised.  acc[0] against the record: at most 2.4e-16 of sum |terms|; acc[1..3], the decisions, perf, ls_norm and the status
word: bit for bit on all 24 cases, row and wave form alike; no instance of the matrix is left unjudged.  At (c) the device decides one
tie differently from the oracle (P1 armijo (c), instance 3: the full step by the Armijo rule where the oracle, margin 4.9e-13, refuses and
stops on deltaTol) — the twin on the device's numbers agrees with the device.
Wrong builds the module catches (made by hand, one at a time, not kept): the step size of k_ls_tail_eval as a power of the decay ->
test_tail_rows_are_evaluated_at_the_walked_step_size; every window started at alpha_decay -> checks D and V of the slow-decay settings;
the sign of the Armijo test flipped -> D of the armijo settings; ls_norm over n 22 state entries -> D (ls_norm) of every case with a
refused full step; the upper force barrier dropped for swing feet in node_value -> V of every case.
"""
import ctypes as C

import numpy as np
import pytest

import _lscases as lc
import _lstwin as tw
from hunter_bipedal_control_amd import abi

pytestmark = pytest.mark.gpu

BOUND = 1e-12
SENTINEL = 7.25
FWD_FORMS = {"row": abi.FORM.RIC_FWD_ROW, "wave": abi.FORM.RIC_FWD_WAVE}
FORM_CASES = [c for c in lc.CASES if c[1] == "armijo"]


class Unjudged(Exception):
    pass


@pytest.fixture(scope="module")
def matrix(params, oracle):
    return lc.Matrix(params, oracle)


def _solver(params, pt, **kw):
    from hunter_bipedal_control_amd.solver import HunterSolver
    return HunterSolver(params, batch=pt.B, max_nodes=pt.x.shape[1] - 1, sqp_iterations=1, **kw)


def _input(pt):
    """The iterate handed to the device: the point, with a sentinel in the rows behind every horizon."""
    x, u = pt.x.copy(), pt.u.copy()
    for i, n in enumerate(pt.n):
        x[i, n + 1:], u[i, n:] = SENTINEL, SENTINEL
    return x, u


def _run(params, pt, **kw):
    s = _solver(params, pt, **kw)
    try:
        x, u = _input(pt)
        s.set_references(pt.refs)
        s.set_trajectory(x, u)
        s.mpc_solve(pt.x0)
        d = dict(s.mpc_linesearch(), x_in=x, u_in=u, perf=s.get_performance(), status=s.mpc_status())
        d["dx"], d["du"] = s.get_step()
        d["x"], d["u"] = s.get_solution()
        d["rec"] = [s.mpc_recovery(i) for i in range(pt.B)]
    finally:
        s.close()
    return d


@pytest.fixture(scope="module")
def device(params, matrix):
    """case (and form) -> everything read back from one solve, kept for the checks of the module."""
    cache = {}

    def get(case, form=None):
        if (case, form) not in cache:
            kw = dict(lc.CONFIGS[case[1]])
            if form is not None:
                kw["reserved"] = FWD_FORMS[form]
            cache[case, form] = _run(params, matrix.point(case[0], case[2]), **kw)
        return cache[case, form]
    return get


def device_walk(matrix, case, d, i):
    """The twin's walk of instance i on the device's own numbers.  Raises Unjudged where it needs a window before the last evaluated one
    whose oracle-side margin is below lc.MARGIN, or passes beyond the window the oracle's walk ends in (a tie decided the other way)."""
    pt, cfg, ow = matrix.point(case[0], case[2]), matrix.cfg(case[1]), matrix.walks(case)[i]
    n, alphas, last = pt.n[i], lc.alphas_of(cfg), ow.last_window

    def sums_of(t):
        if t == 0:
            return tw.wave_sums(d["partial"][i, :n])
        w, row = (t - 1) // tw.WINDOW, (t - 1) % tw.WINDOW
        if w == last:
            return tw.wave_sums(d["ls_tail"][i, row, :n])
        if w > last or ow.margins.get(t, 0.0) < lc.MARGIN:
            raise Unjudged(f"{lc.case_id(case)}[{i}] trial {t}")
        return pt.trial_sums(i, alphas[t])
    return tw.walk(cfg, d["acc"][i], sums_of, tuple(d["ls_norm"][i]), ric_fail=bool(d["ric_fail"][i]))


def _walks(matrix, case, d):
    out = []
    for i in range(len(d["accepted"])):
        try:
            out.append(device_walk(matrix, case, d, i))
        except Unjudged as e:
            print(f"not judged: {e}")
            assert case[2] == "c", e
            out.append(None)
    return out


# ---- V ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_node_values_match_the_reference(matrix, device, case):
    pt, cfg, d = matrix.point(case[0], case[2]), matrix.cfg(case[1]), device(case)
    wins, walks = tw.windows(cfg), _walks(matrix, case, d)
    worst, rows_checked = np.zeros(3), 0

    def hold(got, i, alpha, what):
        nonlocal worst
        want = pt.node_values(i, pt.x[i] + alpha * d["dx"][i], pt.u[i] + alpha * d["du"][i])
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        worst = np.maximum(worst, err.max(axis=0))
        assert (err <= BOUND).all(), (lc.case_id(case), i, what, np.argwhere(~(err <= BOUND))[:4].tolist(), float(err.max()))

    for i, n in enumerate(pt.n):
        hold(d["partial"][i, :n], i, 1.0, "partial")
        w = walks[i]
        if w is not None and w.last_window >= 0:
            for row in range(w.rows):
                hold(d["ls_tail"][i, row, :n], i, wins[w.last_window][row], f"ls_tail window {w.last_window} row {row}")
                rows_checked += 1
    print(f"V {lc.case_id(case)}: worst (cost, defect, eq) = " + " ".join(f"{v:.1e}" for v in worst) + f"; {rows_checked} tail rows")


# ---- B ----------------------------------------------------------------------------------------------------------------------------------
def _baseline(pt, d, tag):
    worst = 0.0
    for i, n in enumerate(pt.n):
        rec = d["rec"][i]
        assert len(rec["meta"]) == n
        want = [0.0, 0.0, 0.0]
        for k in range(n):
            for c in range(3):
                want[c] += float(rec["meta"][k, 3 + c])
        assert tw.same_bits(d["acc"][i, 1:], want), (tag, i, d["acc"][i, 1:].tolist(), want)
        terms = rec["qf"] * d["dx"][i, :n] + rec["rf"] * d["du"][i, :n]
        err, scale = abs(d["acc"][i, 0] - terms.sum()), max(1.0, np.abs(terms).sum())
        worst = max(worst, err / scale)
        assert err <= 1e-12 * scale, (tag, i, d["acc"][i, 0], terms.sum(), err / scale)
    print(f"B {tag}: acc[1..3] bit for bit; armijo worst {worst:.1e}")


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_baseline_is_the_sum_of_the_record(matrix, device, case):
    _baseline(matrix.point(case[0], case[2]), device(case), lc.case_id(case))


@pytest.mark.parametrize("form", list(FWD_FORMS))
@pytest.mark.parametrize("case", FORM_CASES, ids=lc.case_id)
def test_baseline_of_both_forward_sweep_forms(matrix, device, case, form):
    d, ref = device(case, form), device(case)
    _baseline(matrix.point(case[0], case[2]), d, f"{lc.case_id(case)} {form}")
    for key in ("acc", "partial", "accepted", "perf", "x", "u"):     # the forms agree bit for bit: so does everything downstream
        assert tw.same_bits(d[key], ref[key]) if d[key].dtype == np.float64 else np.array_equal(d[key], ref[key]), (form, key)


# ---- D ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_decisions_match_the_twin_on_the_device_numbers(matrix, device, case):
    pt, d = matrix.point(case[0], case[2]), device(case)
    walks, owalks = _walks(matrix, case, d), matrix.walks(case)
    assert not d["ric_fail"].any()
    line = []
    for i, n in enumerate(pt.n):
        w, ow, at = walks[i], owalks[i], (lc.case_id(case), i)
        if w is None:
            line.append(f"[{i}]not judged")
            continue
        line.append(f"[{i}]{w.cause}@{w.trial}" + (f"/b{w.branch}" if w.branch else ""))
        assert int(d["accepted"][i]) == w.word, (at, int(d["accepted"][i]), w.cause, w.trial)
        want = np.r_[w.sums, w.alpha] if w.cause == tw.ACCEPTED else np.r_[d["acc"][i, 1:], 0.0]
        assert tw.same_bits(d["perf"][i], want), (at, d["perf"][i].tolist(), want.tolist(), w.cause, w.trial)
        if w.trial > 0 or w.cause != tw.ACCEPTED:      # refused at step size 1: the norms were written
            assert tw.same_bits(d["ls_norm"][i], tw.norms(d["dx"][i], d["du"][i], n)), (at, d["ls_norm"][i].tolist(), tw.norms(d["dx"][i], d["du"][i], n))
        assert int(d["status"][i]) == tw.expected_status(w), (at, int(d["status"][i]), w.cause)
        if ow.margin >= lc.MARGIN:
            assert (w.cause, w.trial, w.branch) == (ow.cause, ow.trial, ow.branch) and d["perf"][i, 3] == ow.alpha, (at, w.cause, w.trial, ow.cause, ow.trial)
    print(f"D {lc.case_id(case)}: " + " ".join(line))


def test_tail_rows_are_evaluated_at_the_walked_step_size(params, matrix, device):
    """k_ls_tail_eval forms the step size of row j on its own (alpha0 times decay, j times) and k_ls_tail_decide walks and commits its
    own: they must be the same number, to the bit.  A few ulp of alpha move a value by 1e-16 of itself, which no bound against a
    reference can see.  So rows of window 1 of P1 gamma_slow (b) (decay 0.9; the instances that accept there: every row of the window
    was evaluated side by side and later windows leave it alone) are held bit for bit to row 0 of a second context whose alpha_decay IS
    that running product (and whose alpha_min is the same number: one window of one row; row 0 takes no multiplication) for rows where a power of the decay would be another number.  Window 1
    because alpha is large there: at 1e-4 one ulp of alpha no longer moves an entry of x + alpha dx."""
    case = ("P1", "gamma_slow", "b")
    pt, cfg, d = matrix.point("P1", "b"), matrix.cfg("gamma_slow"), device(case)
    first = tw.windows(cfg)[0]
    insts = [i for i, w in enumerate(_walks(matrix, case, d)) if w is not None and w.cause == tw.ACCEPTED and w.last_window == 0 and pt.n[i] > 1]
    rows = [j for j, a in enumerate(first) if a != first[0] * cfg.alpha_decay ** j]
    assert insts and len(rows) >= 3, (insts, rows)
    for j in rows[:3]:
        e = _run(params, pt, **dict(lc.CONFIGS["gamma_slow"], alpha_decay=first[j], alpha_min=first[j]))    # one window of one row
        for i in insts:
            n = pt.n[i]
            assert tw.same_bits(e["partial"][i, :n], d["partial"][i, :n]) and tw.same_bits(e["ls_norm"][i], d["ls_norm"][i]), (i, j)
            assert tw.same_bits(e["ls_tail"][i, 0, :n], d["ls_tail"][i, j, :n]), (i, j, first[j], int(e["accepted"][i]), e["perf"][i].tolist())


# ---- C ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_committed_iterate(matrix, device, case):
    pt, d = matrix.point(case[0], case[2]), device(case)
    for i, n in enumerate(pt.n):
        at, alpha = (lc.case_id(case), i), float(d["perf"][i, 3])
        assert (d["accepted"][i] == 1) == (alpha > 0.0), at
        if d["accepted"][i] == 1:
            assert tw.committed(pt.x[i, :n + 1], d["dx"][i, :n + 1], alpha, d["x"][i, :n + 1]), at
            assert tw.committed(pt.u[i, :n], d["du"][i, :n], alpha, d["u"][i, :n]), at
        else:
            assert tw.same_bits(d["x"][i, :n + 1], pt.x[i, :n + 1]) and tw.same_bits(d["u"][i, :n], pt.u[i, :n]), at
        assert tw.same_bits(d["x"][i, n + 1:], d["x_in"][i, n + 1:]) and tw.same_bits(d["u"][i, n:], d["u_in"][i, n:]), at
        assert not d["dx"][i, 0].any(), at


# ---- R ----------------------------------------------------------------------------------------------------------------------------------
def test_riccati_failure_refuses_what_the_filter_accepts(params, matrix):
    """The recipe of test_gpu_failure_surface.py (negative task-space input weights: R~ indefinite) on P1 at the cold start."""
    pt, cfg = matrix.point("P1", "a"), matrix.cfg("ship")
    d = _run(params, pt, R_task_diag=[-5.0] * len(params["config"]["R_task_diag"]))
    assert (d["ric_fail"] == 1).all() and (d["accepted"] == 0).all() and (d["status"] == abi.HB_INST_NAN).all(), (d["ric_fail"], d["accepted"], d["status"])
    assert (d["perf"][:, 3] == 0.0).all()
    assert tw.same_bits(d["x"], d["x_in"]) and tw.same_bits(d["u"], d["u_in"])
    would = []
    for i, n in enumerate(pt.n):
        part = d["partial"][i, :n]
        if not (np.isfinite(part).all() and np.isfinite(d["acc"][i]).all()):
            continue
        branch, ok = tw.filter_accept(cfg, d["acc"][i, 1], float(np.sqrt(d["acc"][i, 2] + d["acc"][i, 3])), *_mv(tw.wave_sums(part)), 1.0, d["acc"][i, 0])
        if ok:
            would.append((i, branch))
    print(f"R: the filter alone accepts the full step of (instance, branch) {would}")
    assert would


def _mv(s):
    return float(s[0]), float(np.sqrt(s[1] + s[2]))


# ---- the getter -------------------------------------------------------------------------------------------------------------------------
def test_getter_refusals_null_pointers_and_reads_change_nothing(params, matrix):
    from hunter_bipedal_control_amd.solver import HunterHipError
    pt = matrix.point("P1", "b")
    s = _solver(params, pt)
    try:
        s.set_references(pt.refs)
        s.set_trajectory(pt.x, pt.u)
        with pytest.raises(HunterHipError, match=r"failed \(-3\).*no MPC call has completed"):
            s.mpc_linesearch()
        s.mpc_solve(pt.x0)
        for begin, count in ((-1, 1), (0, pt.B + 1), (pt.B, 1), (3, 0)):
            with pytest.raises(HunterHipError, match=r"failed \(-1\).*hb_mpc_get_linesearch: instance range outside the batch"):
                s.mpc_linesearch(begin, count)
        before = s.get_solution() + s.get_step() + (s.get_performance(), s.mpc_status())
        first, again = s.mpc_linesearch(), s.mpc_linesearch()
        assert all(np.array_equal(first[k], again[k]) for k in first) and set(first) == set(s.LINESEARCH_KEYS)
        after = s.get_solution() + s.get_step() + (s.get_performance(), s.mpc_status())
        assert all(tw.same_bits(a, b) if a.dtype == np.float64 else np.array_equal(a, b) for a, b in zip(before, after))
        part = s.mpc_linesearch(2, 3)
        assert all(np.array_equal(part[k], first[k][2:5]) for k in first)
        acc, word = np.full((pt.B, 4), 7.0), np.full(pt.B, 7, dtype=np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        assert s.lib.hb_mpc_get_linesearch(s.ctx, C.c_int32(0), C.c_int32(pt.B), p(acc), None, None, None, p(word), None) == 0
        assert np.array_equal(acc, first["acc"]) and np.array_equal(word, first["accepted"])
        assert s.lib.hb_mpc_get_linesearch(s.ctx, C.c_int32(0), C.c_int32(pt.B), None, None, None, None, None, None) == 0
        assert first["ls_tail"].shape == (pt.B, abi.HB_LS_TAIL_MAX, pt.x.shape[1] - 1, 3)
        s.set_references(pt.refs)
        with pytest.raises(HunterHipError, match=r"failed \(-3\).*replaced since the last MPC call"):
            s.mpc_linesearch()
    finally:
        s.close()
