"""Shared by tests/test_mpc_certificate_host.py and tests/test_gpu_mpc_certificate.py: the eight ragged all-mode instances of
test_gpu_parity.py::test_ragged_horizons_all_modes_and_off_grid_events, and the numpy side of the MPC certificate (hunter_hip.h
HB_MPC_CERT_*): the dense KKT system of an exported stage QP, the costate recursion and the eight fields."""
import numpy as np

from hunter_bipedal_control_amd import workload
from oracle import refgen

NMAX = 64
SPECS = [("trot", 0.03, 0.75), ("standing_trot", 0.03, 0.7), ("flying_trot", 0.03, 0.7), ("trot", 0.1, 0.015),
         ("flying_trot", 0.26, 0.2), ("stance", 0.0, 0.3), ("trot", 0.37, 0.9), ("standing_trot", 0.2, 0.33)]
FIELDS = ("r_dyn", "r_stat", "obj", "step_max", "u_max", "lambda_max", "scale", "n_nodes")
LQ_KEYS = ("A", "B", "b", "Q", "P", "R", "q", "r")


def ragged_problem(params):
    """-> refs (stacked tables, nmax = 64), x0 [8][22]: n from 1 to 60, modes 0..3 (projected widths 6 / 9 / 12), event times off the grid."""
    tabs, xs = [], []
    for i, (gait, t0, hor) in enumerate(SPECS):
        xi = workload.perturbed_state(params, 100 + i)
        tabs.append(refgen.make_trot_problem(params, t0, hor, xi, (0.25, 0.05, 0.0, 0.2), NMAX, gait=gait))
        xs.append(xi)
    refs, x0 = refgen.stack_tables(tabs), np.stack(xs)
    n = refs["n_nodes"]
    assert n.min() == 1 and n.max() == 60 and len(set(n.tolist())) > 3
    seen = set()
    for i in range(len(SPECS)):
        seen |= set(refs["mode"][i, :n[i]].tolist())
    assert seen == {0, 1, 2, 3}
    return refs, x0


def cold_start(oracle, refs, x0):
    B = x0.shape[0]
    x, u = np.zeros((B, NMAX + 1, 22)), np.zeros((B, NMAX, 22))
    for i in range(B):
        n = int(refs["n_nodes"][i])
        x[i, :n + 1], u[i, :n] = oracle.cold_start(refs["mode"][i, :n], x0[i])
    return x, u


def dense_kkt(lq, n):
    """The stage QP as ONE dense KKT system: variables dx_0..dx_n, u~_0..u~_(n-1); constraints -dx_0 = 0 and
    A dx_k + B u~_k - dx_(k+1) = -b_k, whose multipliers are lambda_0 and lambda_(k+1) of hunter_hip.h.  np.linalg.solve; numpy's own
    residual is asserted first.  -> dict(dx [n+1][22], u [n][12], lam [n+1][22], obj, resid, cond)."""
    nx, nu = 22 * (n + 1), 12 * n
    nz, nc = nx + nu, 22 * (n + 1)
    H, g = np.zeros((nz, nz)), np.zeros(nz)
    G, h = np.zeros((nc, nz)), np.zeros(nc)
    G[:22, :22] = -np.eye(22)
    for k in range(n):
        sx, su = slice(22 * k, 22 * k + 22), slice(nx + 12 * k, nx + 12 * k + 12)
        H[sx, sx], H[su, su], H[su, sx], H[sx, su] = lq["Q"][k], lq["R"][k], lq["P"][k], lq["P"][k].T
        g[sx], g[su] = lq["q"][k], lq["r"][k]
        rows = slice(22 * (k + 1), 22 * (k + 2))
        G[rows, sx], G[rows, su] = lq["A"][k], lq["B"][k]
        G[rows, 22 * (k + 1):22 * (k + 2)] = -np.eye(22)
        h[rows] = -lq["b"][k]
    K = np.block([[H, G.T], [G, np.zeros((nc, nc))]])
    rhs = np.r_[-g, h]
    z = np.linalg.solve(K, rhs)
    resid = np.abs(K @ z - rhs).max()
    assert resid <= 1e-11, resid
    zz = z[:nz]
    return dict(dx=z[:nx].reshape(n + 1, 22), u=z[nx:nz].reshape(n, 12), lam=z[nz:].reshape(n + 1, 22), obj=g @ zz + 0.5 * zz @ H @ zz,
                resid=resid)


def costate_recursion(lq, n, dx, u):
    lam = np.zeros((n + 1, 22))
    for k in range(n - 1, -1, -1):
        lam[k] = lq["q"][k] + lq["Q"][k] @ dx[k] + lq["P"][k].T @ u[k] + lq["A"][k].T @ lam[k + 1]
    return lam


def numpy_fields(lq, n, dx, u, lam):
    """The eight fields of hunter_hip.h recomputed from the exported QP and a point (dx, u~, lambda)."""
    inf = lambda v: np.abs(v).max() if np.size(v) else 0.0  # noqa: E731
    r_dyn, r_stat, obj, scale = inf(dx[0]), 0.0, 0.0, 0.0
    for k in range(n):
        A, B, b, Q, P, R, q, r = (lq[key][k] for key in LQ_KEYS)
        r_dyn = max(r_dyn, inf(dx[k + 1] - (A @ dx[k] + B @ u[k] + b)))
        r_stat = max(r_stat, inf(r + P @ dx[k] + R @ u[k] + B.T @ lam[k + 1]))
        obj += q @ dx[k] + r @ u[k] + 0.5 * dx[k] @ Q @ dx[k] + u[k] @ P @ dx[k] + 0.5 * u[k] @ R @ u[k]
        scale = max(scale, inf(r), inf(P @ dx[k]), inf(R @ u[k]), inf(B.T @ lam[k + 1]))
    return dict(r_dyn=r_dyn, r_stat=r_stat, obj=obj, step_max=inf(dx[:n + 1]), u_max=inf(u[:n]), lambda_max=inf(lam[:n + 1]), scale=scale,
                n_nodes=n)


def check_against_numpy(lq, n, dx, u, lam, cert, kkt=None, tag=""):
    """CPU tests 1-3 of the certificate on one instance: the point against the dense solve, the fields against numpy's recomputation,
    and certified.  cert: dict of the eight fields.  -> the measured figures (for the record)."""
    kkt = kkt or dense_kkt(lq, n)
    f = numpy_fields(lq, n, dx, u, lam)
    m = dict(d_dx=np.abs(dx[:n + 1] - kkt["dx"]).max(), d_u=np.abs(u[:n] - kkt["u"]).max(), d_lam=np.abs(lam[:n + 1] - kkt["lam"]).max(),
             d_obj=abs(cert["obj"] - kkt["obj"]), r_dyn=cert["r_dyn"], r_stat_rel=cert["r_stat"] / cert["scale"], scale=cert["scale"],
             u_max=cert["u_max"], lambda_max=cert["lambda_max"], step_max=cert["step_max"])
    print(f"mpc certificate {tag} n={n}: " + " ".join(f"{k}={v:.3e}" for k, v in m.items()))
    # 1. the point against the dense KKT solve
    assert m["d_dx"] <= 1e-9, (tag, m)
    assert m["d_u"] <= 1e-9 * max(1.0, cert["u_max"]), (tag, m)
    assert m["d_lam"] <= 1e-9 * max(1.0, cert["lambda_max"]), (tag, m)
    assert m["d_obj"] <= 1e-9 * max(1.0, abs(kkt["obj"])), (tag, m)
    assert not lam[n].any(), "lambda_n = 0 exactly"
    # 2. the reported fields against numpy's recomputation on the exported QP
    for name in ("r_dyn", "r_stat"):
        assert abs(cert[name] - f[name]) <= 1e-9 * f["scale"], (tag, name, cert[name], f[name])
    assert abs(cert["obj"] - f["obj"]) <= 1e-9 * max(1.0, abs(f["obj"])), (tag, cert["obj"], f["obj"])   # (the bound of the dense comparison)
    for name in ("scale", "step_max", "u_max", "lambda_max"):
        assert abs(cert[name] - f[name]) <= 1e-12 * f[name], (tag, name, cert[name], f[name])
    assert cert["n_nodes"] == n
    # 3. certified
    assert cert["r_dyn"] <= 1e-12 * max(1.0, cert["step_max"]), (tag, m)
    assert cert["r_stat"] <= 1e-9 * cert["scale"], (tag, m)
    return m
