"""The exact twin of the filter line search (k_ls_eval / k_ls_decide / k_ls_tail_eval / k_ls_tail_decide in hb_kernels.hip, filter_accept
in hb_riccati.hpp, the window loop of enqueue_sqp in hb_api_mpc.hpp), numpy and float64 only.  It restates the ORDER of the device's
arithmetic, so that what it returns is the device's bit pattern and not an approximation of it:

  * sums: per lane l the sum over the nodes l, l + 64, ... in that order, then the shfl_down tree v[l] += v[l + off], off = 32 .. 1, lane 0;
  * step sizes: repeated multiplication (alpha *= decay), never decay ** i; windows of WINDOW = 16, a window's first step size being the
    running product the sequential search holds there;
  * a * b + c written in one expression is ONE rounding on the device (the HIP compiler contracts it into a fused multiply-add) and two
    on the host the oracle is compiled for: `fused` selects which.  Three places: the squares of the norms, the Armijo bound
    base_merit + (armijo_factor alpha) armijo and the merit bound base_merit - gamma_c base_viol.  (1 - gamma_c) base_viol is a
    difference times a factor: not contracted.  fma() below is the correctly rounded one (exact rational arithmetic).

walk() is the decision sequence; the tests feed it the device's own numbers (tests/test_gpu_linesearch.py) or the oracle's
(tests/test_linesearch_host.py: there it must reproduce the step size of oracle.mpc_solve, which is what entitles it to judge)."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

LANES, WINDOW = 64, 16
ACCEPTED, DELTA_TOL, ALPHA_MIN, RIC_FAIL = "accepted", "delta_tol", "alpha_min", "ric_fail"


def fma(a, b, c):
    """a * b + c rounded once."""
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _tree(v):
    """[64][c] lane values -> what lane 0 holds after v[l] += v[l + off], off = 32 .. 1."""
    off = LANES // 2
    while off:
        v[:off] = v[:off] + v[off:2 * off]
        off //= 2
    return v[0].copy()


def wave_sums(partials):
    """partials [n][c] (the rows of the n nodes of one instance at one step size) -> [c]: the sums k_ls_decide / k_ls_tail_decide form."""
    p = np.asarray(partials, dtype=np.float64)
    p = p.reshape(p.shape[0], -1)
    v = np.zeros((LANES, p.shape[1]))
    for k in range(p.shape[0]):        # lane k % 64 meets its nodes in ascending order
        v[k % LANES] += p[k]
    return _tree(v)


def _norm(flat, fused):
    v = np.zeros((LANES, 1))
    if fused:
        for i, e in enumerate(flat):
            v[i % LANES, 0] = fma(e, e, v[i % LANES, 0])
    else:
        for i, e in enumerate(flat):
            v[i % LANES, 0] += e * e
    return float(np.sqrt(_tree(v)[0]))


def norms(dx, du, n, fused=True):
    """|dx|_2 over the (n + 1) 22 state entries and |du|_2 over the n 22 input entries of one instance, as k_ls_decide leaves them in
    ls_norm: the reduction of wave_sums over the squares, then the square root."""
    dx, du = np.asarray(dx, dtype=np.float64), np.asarray(du, dtype=np.float64)
    return _norm(dx[:n + 1].reshape(-1), fused), _norm(du[:n].reshape(-1), fused)


def config(params, **overrides):
    """The line-search settings of a context: the fields of hb_config by name (abi.make_config with the overrides)."""
    from hunter_bipedal_control_amd import abi
    c = abi.make_config(params, **overrides)
    return SimpleNamespace(**{k: float(getattr(c, k)) for k in ("g_max", "g_min", "alpha_decay", "alpha_min", "gamma_c", "armijo_factor", "delta_tol")})


def filter_accept(cfg, base_merit, base_viol, merit, viol, alpha, armijo, fused=True):
    """-> (branch 1 / 2 / 3, verdict): 1 = the violation rule above g_max, 2 = the Armijo rule, 3 = the filter rule."""
    less_viol = viol < (1.0 - cfg.gamma_c) * base_viol
    if viol > cfg.g_max:
        return 1, bool(less_viol)
    if viol < cfg.g_min and base_viol < cfg.g_min and armijo < 0.0:
        t = cfg.armijo_factor * alpha
        bound = fma(t, armijo, base_merit) if fused else base_merit + t * armijo
        return 2, bool(merit < bound)
    bound = fma(-cfg.gamma_c, base_viol, base_merit) if fused else base_merit - cfg.gamma_c * base_viol
    return 3, bool(merit < bound or less_viol)


def windows(cfg):
    """The step sizes of the backtracking tail, window by window, as enqueue_sqp launches them (none if the decay is not in (0, 1))."""
    out = []
    if cfg.alpha_decay > 0.0 and cfg.alpha_decay < 1.0 and cfg.alpha_decay >= cfg.alpha_min:
        a_win = cfg.alpha_decay
        while a_win >= cfg.alpha_min:
            alphas, a = [], a_win
            while a >= cfg.alpha_min and len(alphas) < WINDOW:
                alphas.append(a)
                a *= cfg.alpha_decay
            out.append(alphas)
            a_win = a
    return out


def walk(cfg, acc, sums_of, norm_xu, ric_fail=False, fused=True):
    """The search of one instance.  acc [4]: Armijo term, baseline merit, dyn_sse, eq_sse; sums_of(trial) -> (merit, dyn_sse, eq_sse) of
    trial 0 (the full step) or tail trial t >= 1 (window (t - 1) // 16, row (t - 1) % 16); norm_xu: (|dx|, |du|), read only once the full
    step is refused.  The deltaTol test comes before every tail trial and never before the full step; the search ends below alpha_min.
    -> cause (accepted / delta_tol / alpha_min / ric_fail), trial, alpha (0 without a step), branch of the deciding trial (0: none),
    word (the `accepted` word 0 / 1 / 2), sums (of the accepted trial), last_window (-1: the tail never ran for this instance),
    rows (the rows of that window the evaluation wrote: not behind n_alpha, not below the deltaTol stop), first_ok (ric_fail only: the
    first trial the filter alone accepts, or None)."""
    base_merit, base_viol = acc[1], float(np.sqrt(acc[2] + acc[3]))
    out = SimpleNamespace(cause=None, trial=0, alpha=0.0, branch=0, word=0, sums=None, last_window=-1, rows=0, first_ok=None, trials=[])

    def trial(t, alpha):
        m, d, e = (float(v) for v in sums_of(t))
        branch, ok = filter_accept(cfg, base_merit, base_viol, m, float(np.sqrt(d + e)), alpha, acc[0], fused)
        out.trials.append((t, alpha, branch, ok))
        if ok and ric_fail and out.first_ok is None:
            out.first_ok = t
        if ok and not ric_fail:
            out.cause, out.trial, out.alpha, out.branch, out.word, out.sums = ACCEPTED, t, alpha, branch, 1, (m, d, e)
        return ok and not ric_fail

    if trial(0, 1.0):
        return out
    dx_norm, du_norm = norm_xu
    t = 0
    for w, alphas in enumerate(windows(cfg)):
        below = [a * du_norm < cfg.delta_tol and a * dx_norm < cfg.delta_tol for a in alphas]
        out.last_window, out.rows = w, below.index(True) if True in below else len(alphas)
        for j, alpha in enumerate(alphas):
            t = w * WINDOW + j + 1
            if below[j]:
                out.cause, out.trial, out.word = DELTA_TOL, t, 2
                return out
            if trial(t, alpha):
                return out
    out.cause, out.trial = (RIC_FAIL if ric_fail else ALPHA_MIN), t
    return out


def expected_status(w, ric_fail=False):
    """hb_mpc_get_status of the instance (HB_INST_*): OK for a step and for the deltaTol stop, MAXITER at alpha_min, NAN after a Riccati
    failure, however the walk ended."""
    return 3 if ric_fail else {ACCEPTED: 0, DELTA_TOL: 0, ALPHA_MIN: 1}[w.cause]


def committed(x, dx, alpha, got):
    """Every entry of `got` is x + alpha dx in one of the two admissible roundings (fused, or product then sum) -> bool."""
    x, dx, got = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (x, dx, got))
    plain = x + alpha * dx
    for i in np.flatnonzero(got != plain):
        if got[i] != fma(alpha, dx[i], x[i]):
            return False
    return True


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
