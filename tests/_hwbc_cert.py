"""numpy twin of the per-level certificate of the HierarchicalWbc cascade (hunter_hip.h, HB_HWBC_CERT_*), built from the oracle's task
rows (oracle.hwbc_tasks), and the reference values of a certified instance: the twin evaluated on the ORACLE's own cascade
(oracle.hoqp level by level) with sign-constrained multipliers.  Shared by the CPU, GPU and C++ certificate tests."""
import numpy as np
from scipy.linalg import null_space
from scipy.optimize import nnls

FIELDS = ("res_own", "res_final", "r_hier", "r_in", "r_stat", "r_dual", "r_comp", "n_free", "n_active", "scale")
RES_OWN, RES_FINAL, R_HIER, R_IN, R_STAT, R_DUAL, R_COMP, N_FREE, N_ACTIVE, SCALE = range(10)
# the figures an instance is certified on, per level; r_stat and r_comp relative to scale
CHECKED = ("r_hier", "r_in", "r_stat", "r_comp", "res_gap")
BOUND_DUAL = 1e-7   # r_dual / scale: no oracle counterpart (nnls makes it 0); the WeightedWbc certificate's bound


def tasks_of(oracle, xd, ud, rbd, mode):
    return [oracle.hwbc_tasks(xd, ud, rbd, int(mode), level) for level in range(3)]


def bases(tasks):
    """Orthonormal bases of the search spaces of the three levels."""
    return [np.eye(38), null_space(tasks[0]["A"], rcond=1e-9), null_space(np.vstack([tasks[0]["A"], tasks[1]["A"]]), rcond=1e-9)]


def twin(tasks, x_levels, slack0, dual, Q=None, reached=3):
    """cert [3][10] of §1 of the definition at the given per-level points, level-0 slack and multipliers (dual [3][>= n_in])."""
    Q = bases(tasks) if Q is None else Q
    D, f = tasks[0]["D"], tasks[0]["f"]
    n_in = D.shape[0]
    v0 = slack0[:n_in]
    out = np.zeros((3, 10))
    for k in range(3):
        A, b, x, y = tasks[k]["A"], tasks[k]["b"], x_levels[k], dual[k][:n_in]
        r = A @ x - b
        g = A.T @ r
        s = D @ x - f - v0
        h = g - D.T @ y
        run = k < reached
        out[k, RES_OWN] = np.linalg.norm(r)
        out[k, RES_FINAL] = np.linalg.norm(A @ x_levels[2] - b)
        out[k, R_HIER] = max([np.abs(tasks[j]["A"] @ (x - x_levels[k - 1])).max() for j in range(k)], default=0.0)
        out[k, R_IN] = max(0.0, s.max())
        out[k, R_STAT] = np.linalg.norm(Q[k].T @ h) if run else np.linalg.norm(g)
        out[k, R_DUAL] = max(0.0, y.max())
        out[k, R_COMP] = np.abs(y * s).max()
        out[k, N_FREE] = Q[k].shape[1] if run else 0
        out[k, N_ACTIVE] = np.count_nonzero(v0 > 0.0) if k == 0 else np.count_nonzero(y)
        out[k, SCALE] = max(1.0, np.abs(A.T @ b).max(), np.abs(A.T @ (A @ x)).max())
    return out


def lstsq_dual(tasks, Q, k, x, W):
    """Multipliers of level k >= 1 on the working set W (list of inequality rows): argmin |Q_k'(g_k - D_W'y_W)|_2, zero outside W."""
    A, b, D = tasks[k]["A"], tasks[k]["b"], tasks[0]["D"]
    y = np.zeros(40)
    if len(W):
        y[W] = np.linalg.lstsq(Q[k].T @ D[W].T, Q[k].T @ (A.T @ (A @ x - b)), rcond=None)[0]
    return y


def oracle_certificate(oracle, tasks, eps, reg_steps):
    """The twin on the oracle's own cascade: x_k = oracle.hoqp(tasks[:k + 1]), v0 = (D x_0 - f)_+, multipliers by nnls (y <= 0) on the rows
    with D x_k - f - v0 >= -1e-9 (the oracle exposes no working set).  Returns (cert [3][10], x_levels [3][38], statuses)."""
    Q = bases(tasks)
    D, f = tasks[0]["D"], tasks[0]["f"]
    xs, sts = [], []
    for k in range(3):
        x, _, st = oracle.hoqp(tasks[:k + 1], eps=eps, reg_steps=reg_steps)
        xs.append(np.asarray(x, dtype=np.float64)[:38])
        sts.append(st)
    v0 = np.maximum(D @ xs[0] - f, 0.0)
    dual = np.zeros((3, 40))
    dual[0, :len(f)] = -v0
    for k in (1, 2):
        A, b = tasks[k]["A"], tasks[k]["b"]
        W = np.flatnonzero(D @ xs[k] - f - v0 >= -1e-9)
        if len(W):
            lam = nnls(Q[k].T @ D[W].T, -(Q[k].T @ (A.T @ (A @ xs[k] - b))))[0]
            dual[k, W] = -lam
    slack0 = np.zeros(40)
    slack0[:len(f)] = v0
    return twin(tasks, xs, slack0, dual, Q), np.array(xs), sts


def figures(cert):
    """cert [..., 3, 10] -> dict of the certified figures [..., 3] (CHECKED and r_dual), the relative ones divided by scale."""
    c = np.asarray(cert)
    sc = c[..., SCALE]
    return dict(r_hier=c[..., R_HIER], r_in=c[..., R_IN], r_stat=c[..., R_STAT] / sc, r_comp=c[..., R_COMP] / sc,
                res_gap=np.abs(c[..., RES_FINAL] - c[..., RES_OWN]), r_dual=c[..., R_DUAL] / sc)


def bounds_from_oracle(oracle_certs):
    """Per level and figure: a value is within its bound when it is at most 10 x the oracle's worst over the input set (margin for
    different arithmetic and a different but equivalent basis), or at most 1e-12 (the floor for figures the oracle has at or near 0).
    The two are alternatives, so the bound is the larger of them: the floor never takes the factor-10 margin away from a figure whose
    oracle worst lies just under 1e-12, and the bound is monotone in the oracle's worst.  oracle_certs [B][3][10]."""
    fo = figures(oracle_certs)
    out = {}
    for name in CHECKED:
        worst = fo[name].max(axis=0)
        out[name] = np.maximum(10.0 * worst, 1e-12)
    out["r_dual"] = np.full(3, BOUND_DUAL)
    return out


def certified(cert, bounds):
    """[B] bool: every figure of every level within its bound."""
    fd = figures(cert)
    ok = np.ones(np.asarray(cert).shape[0], dtype=bool)
    for name, bnd in bounds.items():
        ok &= (fd[name] <= bnd).all(axis=-1)
    return ok


def worst_table(cert):
    fd = figures(cert)
    return {name: ["%.1e" % v for v in fd[name].max(axis=0)] for name in fd}


_REF = {}


def reference(oracle, params, name, eps=None, reg_steps=1):
    """Oracle certificates of an input set ("mixed": _mixed_inputs(params, 64, 7), "fast": _fast_inputs(params, 24, 5)), computed once
    per test run and shared: dict(inputs, tasks [B], cert [B][3][10], x [B][3][38], bounds)."""
    from test_wbc_certificate_host import _fast_inputs, _mixed_inputs
    eps = params["config"].get("wbc_eps_reg", 1e-8) if eps is None else eps
    key = (name, eps, reg_steps)
    if key not in _REF:
        inp = _mixed_inputs(params, 64, 7) if name == "mixed" else _fast_inputs(params, 24, 5)
        xd, ud, rbd, mode, _ = inp
        tasks = [tasks_of(oracle, xd[i], ud[i], rbd[i], mode[i]) for i in range(len(mode))]
        res = [oracle_certificate(oracle, t, eps, reg_steps) for t in tasks]
        cert = np.array([r[0] for r in res])
        assert all(st == 0 for r in res for st in r[2]), "the oracle solves every instance of the set"
        _REF[key] = dict(inputs=inp, tasks=tasks, cert=cert, x=np.array([r[1] for r in res]), bounds=bounds_from_oracle(cert))
    return _REF[key]
