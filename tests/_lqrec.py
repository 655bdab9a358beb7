"""Shared by tests/test_lq_record_host.py and tests/test_gpu_lq_record.py: the stage record of the LQ approximation (hb_lq.hpp; exported by
hb_mpc_get_lq + hb_mpc_get_recovery, or by the host twin's emu_lq_records) held to the oracle's UNPROJECTED node LQ (oracle/ocp.hpp
node_lq: A, B, b, Q, P, R, q, r, C, D, e), node by node.  Pure numpy plus the oracle.

Why not block against block: the record's Kx is the BASIC least-squares solution of a pivoted Cholesky, the oracle's Px the minimum-norm
one; both are right and they differ by O(1e2), so A~ and At, Q~ and Qt, ... legitimately differ.  Instead the oracle's unprojected LQ is
lifted through the record's OWN change of variables du = T u~ + K dx + k (hunter_hip.h, hb_mpc_get_recovery) — after T, K, k have been
shown to be a valid one from the oracle's constraint (D T = 0 with full kernel rank; both normal equations) — and every block follows
from the formulas of node_lq."""
import numpy as np

import _mpc_cert as mc

LQ_KEYS = mc.LQ_KEYS + ("n_til",)
REC_KEYS = ("Kx", "ke", "Z", "dF", "qf", "rf", "meta", "dt", "dq")
MIN_NODES_PER_BRANCH = 8
SEED = 7
# the checks of check_record, by name (the figures it returns carry the toleranced ones)
EXACT = ("n_f", "n_f + n_z", "mode", "R padding", "B padding", "P padding", "r padding", "Z padding", "dF", "Q symmetric", "dt", "rank T")
TOLERANCED = ("D T", "normal K", "normal k", "A", "B", "b", "Q", "P", "R", "q", "r", "qf", "rf", "cost", "dyn_sse", "eq_sse", "dq")


def contact_flags(mode):
    """feet [L_f1, R_f1, L_f2, R_f2] (oracle/ocp.hpp mode_to_contact_flags)"""
    L, R = mode in (2, 3), mode in (1, 3)
    return [L, R, L, R]


def instance_nodes(refs, x, u, i):
    """The node inputs of instance i at the linearisation point (x, u): one dict per interval."""
    n = int(refs["n_nodes"][i])
    return [dict(dt=float(refs["t"][i, k + 1] - refs["t"][i, k]), mode=int(refs["mode"][i, k]), x_ref=refs["x_ref"][i, k].copy(),
                 swing=np.asarray(refs["swing"][i, k]).reshape(4, 6).copy(), x=x[i, k].copy(), u=u[i, k].copy(), x_next=x[i, k + 1].copy())
            for k in range(n)]


# ---- the two linearisation points -----------------------------------------------------------------------------------------------------
def _limits(oracle):
    m, c = oracle.model, oracle.config
    return dict(q_lower=np.array(m.q_lower[:]), q_upper=np.array(m.q_upper[:]), qd_limit=np.array(m.qd_limit[:]),
                d_fric=c.friction_barrier_delta, d_pos=c.pos_limit_barrier[1], d_vel=c.vel_limit_barrier[1], d_force=c.force_limit_barrier[1],
                f_lo=c.force_limit[0], f_hi=c.force_limit[1])


def branch_counts(oracle, refs, x, u):
    """Nodes of the point (x, u) with at least one barrier argument on each branch, from oracle-side quantities only: the friction cone
    value of oracle.friction_cone on the contact feet, the model's limits and the configured deltas (h > delta: logarithmic)."""
    L = _limits(oracle)
    names = [f"{fam} {side} {br}" for fam, sides in (("friction", ("",)), ("position", ("lower", "upper")), ("rate", ("lower", "upper")),
                                                      ("force", ("lower", "upper"))) for side in sides for br in ("log", "ext")]
    cnt = {" ".join(nm.split()): 0 for nm in names}

    def mark(hit, fam, h, delta):
        h = np.atleast_1d(h)
        if (h > delta).any():
            hit.add(f"{fam} log")
        if (h <= delta).any():
            hit.add(f"{fam} ext")

    for i in range(len(refs["n_nodes"])):
        for k in range(int(refs["n_nodes"][i])):
            hit = set()
            cf = contact_flags(int(refs["mode"][i, k]))
            hs = [oracle.friction_cone(u[i, k, 3 * f:3 * f + 3])[0] for f in range(4) if cf[f]]
            if hs:
                mark(hit, "friction", np.array(hs), L["d_fric"])
            q, qd, Fz = x[i, k, 12:], u[i, k, 12:], u[i, k, 2:12:3]
            mark(hit, "position lower", q - L["q_lower"], L["d_pos"])
            mark(hit, "position upper", L["q_upper"] - q, L["d_pos"])
            mark(hit, "rate lower", qd + L["qd_limit"], L["d_vel"])
            mark(hit, "rate upper", L["qd_limit"] - qd, L["d_vel"])
            mark(hit, "force lower", Fz - L["f_lo"], L["d_force"])
            mark(hit, "force upper", L["f_hi"] - Fz, L["d_force"])
            for name in hit:
                cnt[name] += 1
    return cnt


def _plant(oracle, refs, x, u):
    """Barrier arguments the noise does not reach, planted on the long instances: per node one joint rate beyond qd_limit - delta on either
    side, one joint position beyond the limit's delta on either side, and the normal force of one contact foot beyond force_hi - delta;
    each at three depths: inside the delta zone, on the limit, beyond the limit."""
    L = _limits(oracle)
    depth = (0.5, 0.0, -2.0)   # argument of the barrier in units of its delta
    for i in range(len(refs["n_nodes"])):
        n = int(refs["n_nodes"][i])
        if n < 20:
            continue
        for k in range(2, 14):
            d = depth[k % 3]
            ju, jl = k % 10, (k + 5) % 10
            u[i, k, 12 + ju] = L["qd_limit"][ju] - d * L["d_vel"]
            u[i, k, 12 + jl] = -L["qd_limit"][jl] + d * L["d_vel"]
            pu, pl = (k + 2) % 10, (k + 7) % 10
            x[i, k, 12 + pu] = L["q_upper"][pu] - d * L["d_pos"]
            x[i, k, 12 + pl] = L["q_lower"][pl] + d * L["d_pos"]
            feet = [f for f in range(4) if contact_flags(int(refs["mode"][i, k]))[f]]
            if feet:
                u[i, k, 3 * feet[k % len(feet)] + 2] = L["f_hi"] - d * L["d_force"]


def iterates(params, oracle):
    """-> refs, x0, {"a": (x, u), "b": (x, u)}: the ragged problem of _mpc_cert.ragged_problem (8 instances, 268 nodes, n = 1 .. 60, modes 0-3)
    at (a) the cold start and (b) a seeded generic iterate: state + 0.1 N(0,1), forces + 15 N N(0,1), joint rates + 1 rad/s N(0,1), plus
    the planted nodes of _plant.  x0 of (b) is its x[:, 0].  Asserts — as a condition on the inputs, from oracle-side quantities alone —
    that at (b) every barrier family is met on its logarithmic and on its quadratic-extension branch, the double-sided ones on
    both sides, on at least MIN_NODES_PER_BRANCH nodes each; all four modes; n = 1 and n = 60."""
    refs, x0 = mc.ragged_problem(params)
    xa, ua = mc.cold_start(oracle, refs, x0)
    rng = np.random.default_rng(SEED)
    xb, ub = xa.copy(), ua.copy()
    for i in range(len(refs["n_nodes"])):
        n = int(refs["n_nodes"][i])
        xb[i, :n + 1] += 0.1 * rng.standard_normal((n + 1, 22))
        ub[i, :n, :12] += 15.0 * rng.standard_normal((n, 12))
        ub[i, :n, 12:] += 1.0 * rng.standard_normal((n, 10))
    _plant(oracle, refs, xb, ub)
    ca, cb = branch_counts(oracle, refs, xa, ua), branch_counts(oracle, refs, xb, ub)
    print("lq record iterates: nodes per barrier branch (a) " + str(ca) + " (b) " + str(cb))
    for name in cb:
        assert cb[name] >= MIN_NODES_PER_BRANCH, f"iterate (b) meets '{name}' on {cb[name]} nodes only"
    n = refs["n_nodes"]
    assert n.min() == 1 and n.max() == 60 and int(n.sum()) == 268
    assert {int(m) for i in range(len(n)) for m in refs["mode"][i, :n[i]]} == {0, 1, 2, 3}
    return refs, x0, dict(a=(xa, ua), b=(xb, ub))


# ---- the checker ----------------------------------------------------------------------------------------------------------------------
def lift(mode, n_f, n_z, Kx, ke, Z, dF):
    """T [22][n_f + n_z], K [22][22], k [22] of du = T u~ + K dx + k (hunter_hip.h) from one record's recovery data."""
    T = np.zeros((22, n_f + n_z))
    col = 0
    for foot, c in enumerate(contact_flags(mode)):
        if c:
            for a in range(3):
                if col < n_f:
                    T[3 * foot + a, col] = 1.0
                col += 1
    T[12:, n_f:] = Z[:, :n_z]
    K = np.zeros((22, 22))
    K[12:] = Kx
    return T, K, np.r_[dF, ke]


def _rel(got, want):
    want = np.asarray(want, dtype=float)
    return float(np.abs(np.asarray(got) - want).max() / max(1.0, np.abs(want).max())) if want.size else 0.0


def check_record(oracle, nodes, rec, bound, tag="", bounds=None, verbose=True):
    """nodes: the node inputs of one instance (instance_nodes); rec: its exported arrays, [n] stages each (LQ_KEYS + REC_KEYS).  Every
    check of EXACT and TOLERANCED on every node; a toleranced figure is max |got - expected| / max(1, max |expected|) of its block and
    is held to `bound` (`bounds`: {check: bound} for single blocks).  Raises one AssertionError naming every failed check as
    "[name]" with the first node it failed on; -> {check: (worst figure, node)} of the toleranced checks (printed).  The oracle's LQ of a
    node is computed once and kept in its dict (key "lq"), never changed."""
    fig, failed = {name: (0.0, -1) for name in TOLERANCED}, {}
    bounds = bounds or {}

    def exact(name, ok, k, what=""):
        if not ok:
            failed.setdefault(name, f"[{name}] node {k} mode {nodes[k]['mode']} {what}")

    def tol(name, got, want, k):
        v = _rel(got, want)
        if not v <= fig[name][0]:    # (a NaN replaces the worst)
            fig[name] = (v, k)
        if not v <= bounds.get(name, bound):
            failed.setdefault(name, f"[{name}] node {k} mode {nodes[k]['mode']}: {v:.3e} > {bounds.get(name, bound):.1e}")

    assert all(len(rec[key]) == len(nodes) for key in LQ_KEYS + REC_KEYS), (tag, "record length", len(nodes))
    for k, nd in enumerate(nodes):
        if "lq" not in nd:
            nd["lq"] = oracle.node_lq(nd["dt"], nd["mode"], nd["x_ref"], nd["swing"], nd["x"], nd["u"], nd["x_next"])
        o = nd["lq"]
        A, B, b, Q, P, R, q, r = (rec[key][k] for key in mc.LQ_KEYS)
        Kx, ke, Z, dF, qf, rf, meta, dt, dq = (rec[key][k] for key in REC_KEYS)
        cf = contact_flags(nd["mode"])
        n_f, n_z = int(meta[0]), int(meta[1])
        nt = n_f + n_z
        # structure, exactly
        exact("n_f", meta[0] == 3 * sum(cf), k, f"{meta[0]}")
        exact("n_f + n_z", meta[1] == n_z and nt == 22 - o["rank"] and int(rec["n_til"][k]) == nt and 0 <= n_z <= 6 and nt <= 12, k,
              f"n_f {meta[0]} n_z {meta[1]} n_til {rec['n_til'][k]} rank D {o['rank']}")
        exact("mode", meta[2] == nd["mode"], k, f"{meta[2]}")
        exact("dt", dt == nd["dt"], k, f"{dt!r} != {nd['dt']!r}")
        if meta[0] != 3 * sum(cf) or not 0 <= n_z <= 6 or nt > 12:
            continue   # (the widths index everything below: this node has failed already)
        pad = np.eye(12)
        pad[:nt, :nt] = R[:nt, :nt]
        exact("R padding", np.array_equal(R, pad), k)
        exact("B padding", not B[:, nt:].any(), k)
        exact("P padding", not P[nt:].any(), k)
        exact("r padding", not r[nt:].any(), k)
        exact("Z padding", not Z[:, n_z:].any(), k)
        exact("dF", np.array_equal(dF, np.concatenate([np.zeros(3) if cf[f] else -nd["u"][3 * f:3 * f + 3] for f in range(4)])), k)
        exact("Q symmetric", np.array_equal(Q, Q.T), k)
        # T, K, k are a valid change of variables for the ORACLE's constraint C dx + D du + e = 0
        T, K, kk = lift(nd["mode"], n_f, n_z, Kx, ke, Z, dF)
        C_, D, e = o["C"], o["D"], o["e"]
        exact("rank T", np.linalg.matrix_rank(T) == nt, k)
        tol("D T", D @ T, np.zeros((D.shape[0], nt)), k)
        tol("normal K", D.T @ (D @ K), -(D.T @ C_), k)
        tol("normal k", D.T @ (D @ kk), -(D.T @ e), k)
        # the eight projected blocks against the lifted oracle (oracle/ocp.hpp node_lq)
        oA, oB, ob, oQ, oP, oR, oq, orr = (o[key] for key in mc.LQ_KEYS)
        tol("A", A, oA + oB @ K, k)
        tol("B", B[:, :nt], oB @ T, k)
        tol("b", b, ob + oB @ kk, k)
        tol("R", R[:nt, :nt], T.T @ oR @ T, k)
        tol("P", P[:nt], T.T @ (oP + oR @ K), k)
        tol("Q", Q, oQ + K.T @ oP + oP.T @ K + K.T @ oR @ K, k)
        tol("r", r[:nt], T.T @ (orr + oR @ kk), k)
        tol("q", q, oq + K.T @ orr + (oP.T + K.T @ oR) @ kk, k)
        # the unprojected gradients and the line-search scalars
        tol("qf", qf, oq, k)
        tol("rf", rf, orr, k)
        tol("cost", meta[3], nd["dt"] * o["cost"], k)
        tol("dyn_sse", meta[4], nd["dt"] * (ob @ ob), k)
        tol("eq_sse", meta[5], nd["dt"] * (e @ e), k)
        tol("dq", dq, ob[12:], k)
    if verbose:
        print(f"lq record {tag} ({len(nodes)} nodes): " + " ".join(f"{name}={v:.2e}@{k}" for name, (v, k) in fig.items()))
    assert not failed, (tag, sorted(failed.values()))
    return fig


def merge(worst, fig, inst):
    """Running per-check maxima over instances: {check: (figure, instance, node)}."""
    for name, (v, k) in fig.items():
        if name not in worst or not v <= worst[name][0]:
            worst[name] = (v, inst, k)
    return worst


def recovered_du(mode, rec_k, u_til, dx):
    """du = T u~ + K dx + k of one stage, from its exported record, the projected input and the state step."""
    n_f, n_z = int(rec_k["meta"][0]), int(rec_k["meta"][1])
    T, K, kk = lift(mode, n_f, n_z, rec_k["Kx"], rec_k["ke"], rec_k["Z"], rec_k["dF"])
    return T @ u_til[:n_f + n_z] + K @ dx + kk
