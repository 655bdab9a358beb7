"""-m gpu: the hand-over of the iterate between MPC calls through the C ABI, against the independent twin tests/_iterate_twin.py on the scenario
table tests/_iterate_cases.py (the CPU side of the same table: tests/test_iterate_host.py).

A context with sqp_iterations = 0 runs no SQP iteration, so hb_mpc_solve performs exactly the warm start onto new node tables (k_warm_shift
behind the host's grid_saved / grid_dirty bookkeeping and the x / xp buffer swap) and hb_mpc_get_solution returns what it wrote;
hb_mpc_set_trajectory sets an arbitrary iterate.  Selected samples must agree bit for bit, interpolated entries within 4 * 2^-53 (|v0| + |v1|),
weight compensation within 1e-12 (the bounds are derived in _iterate_twin.py)."""
import numpy as np
import pytest

import _iterate_cases as cases
import _iterate_twin as tw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(params):
    return cases.build(params)


def _solver(params, batch=cases.B, max_nodes=cases.NMAX):
    from hunter_bipedal_control_amd.solver import HunterSolver
    return HunterSolver(params, batch=batch, max_nodes=max_nodes, sqp_iterations=0)


def _start(s, params, case):
    """the iterate (X, U) on the previous tables"""
    s.set_references(cases.with_references(case["prev"], params))
    s.reset(case["x0"])
    s.set_trajectory(case["X"], case["U"])


def _send_new_tables(s, params, case):
    """new tables for the instances [0, 10) in two calls; 10 and 11 keep theirs"""
    new = cases.with_references(case["new"], params)
    s.set_references(cases.rows(new, 0, 5), 0)
    s.set_references(cases.rows(new, 5, cases.N_DIRTY), 5)


def _later(tables, params, shift):
    """the tables `shift` intervals later, for every instance"""
    out = dict(tables)
    out["t"] = tables["t"] + shift * float(params["config"]["dt"])
    return out


def test_warm_shift_matches_the_twin(params, case):
    want_X, want_U, plan = tw.warm_shift(case["prev"], case["X"], case["U"], case["new"], case["dirty"], case["weight"])
    cases.assert_reach(plan)
    s = _solver(params)
    try:
        _start(s, params, case)
        status = s.mpc_status()
        _send_new_tables(s, params, case)
        s.mpc_solve()
        got_X, got_U = s.get_solution()
        assert np.array_equal(s.mpc_status(), status)
    finally:
        s.close()
    worst = tw.check_shift(got_X, got_U, want_X, want_U, plan, case["new"], case["dirty"])
    print(f"warm shift, device: worst interpolation error / bound {worst:.3f}")
    n = int(case["new"]["n_nodes"][0])          # identical tables re-sent: the source itself
    assert tw.same_bits(got_X[0, :n + 1], case["X"][0, :n + 1]) and tw.same_bits(got_U[0, :n], case["U"][0, :n])


def test_table_update_sequences(params, case):
    prev, new, dirty, X, U, w = case["prev"], case["new"], case["dirty"], case["X"], case["U"], case["weight"]
    third = _later(new, params, 0.7)
    everyone = np.ones(cases.B, dtype=np.int32)
    s = _solver(params)
    try:
        # a solve with no table change leaves the iterate as it is, NaN rows included
        _start(s, params, case)
        s.mpc_solve()
        x, u = s.get_solution()
        assert tw.same_bits(x, X) and tw.same_bits(u, U)

        # two table updates and no solve in between: the shift starts from the grid the iterate lives on
        _send_new_tables(s, params, case)
        s.set_references(cases.with_references(third, params))
        s.mpc_solve()
        x, u = s.get_solution()
        wx, wu, plan = tw.warm_shift(prev, X, U, third, everyone, w)
        tw.check_shift(x, u, wx, wu, plan, third, everyone, "A -> B -> C, one solve")

        # a table change, a solve, another table change, a solve: the twin applied twice (the buffers swap back); the second step of the
        # twin starts from the device's first result, which the first step has pinned to the twin
        _start(s, params, case)
        _send_new_tables(s, params, case)
        s.mpc_solve()
        x1, u1 = s.get_solution()
        wx, wu, plan = tw.warm_shift(prev, X, U, new, dirty, w)
        tw.check_shift(x1, u1, wx, wu, plan, new, dirty, "A -> B")
        s.mpc_solve()                                                  # and nothing moves without a table change
        x1b, u1b = s.get_solution()
        assert tw.same_bits(x1b, x1) and tw.same_bits(u1b, u1)
        s.set_references(cases.with_references(third, params))
        s.mpc_solve()
        x2, u2 = s.get_solution()
        wx, wu, plan = tw.warm_shift(new, x1, u1, third, everyone, w)
        tw.check_shift(x2, u2, wx, wu, plan, third, everyone, "A -> B, solve, B -> C, solve")

        # a masked reset between the table update and the solve: the cold start on the NEW tables for the two (one with new tables, one
        # without), the shift for the rest
        _start(s, params, case)
        _send_new_tables(s, params, case)
        mask = np.zeros(cases.B, dtype=np.uint8)
        mask[[2, 10]] = 1
        x0 = case["x0"] + 0.01
        s.reset_masked(mask, x0)
        s.mpc_solve()
        x, u = s.get_solution()
        wx, wu, plan = tw.warm_shift(prev, X, U, new, dirty, w)
        cx, cu = tw.cold_start(new, x0, mask, wx, wu, w)
        for b in (2, 10):
            n = int(new["n_nodes"][b])
            assert tw.same_bits(x[b, :n + 1], cx[b, :n + 1]) and np.abs(u[b, :n] - cu[b, :n]).max() <= tw.WEIGHT_TOL, b
        assert tw.same_bits(x[10], cx[10]) and tw.same_bits(u[10, new["n_nodes"][10]:], U[10, new["n_nodes"][10]:])     # its NaN rows came along
        keep = np.delete(np.arange(cases.B), [2, 10])
        sub = lambda a: a[keep]
        tw.check_shift(sub(x), sub(u), sub(cx), sub(cu), {k: sub(v) for k, v in plan.items()}, cases.rows_at(new, keep), sub(dirty), "masked reset")
        assert s.mpc_status().max() == 0

        # an iterate given after the table update is taken as it is, on the new tables: no shift
        _start(s, params, case)
        _send_new_tables(s, params, case)
        X2, U2 = X[::-1].copy(), U[::-1].copy()
        s.set_trajectory(X2, U2)
        s.mpc_solve()
        x, u = s.get_solution()
        assert tw.same_bits(x, X2) and tw.same_bits(u, U2)
    finally:
        s.close()


def test_cold_start_rows(params, case):
    cs = cases.cold_start_case(case)
    tabs = cs["tables"]
    s = _solver(params)
    try:
        s.set_references(cases.with_references(tabs, params))
        s.reset(np.zeros((cases.B, 22)))
        for mask in (cs["mask"], None):
            s.set_trajectory(cs["X_before"], cs["U_before"])
            if mask is None:
                s.reset(cs["x0"])
            else:
                s.reset_masked(mask, cs["x0"])
            x, u = s.get_solution()
            want_X, want_U = tw.cold_start(tabs, cs["x0"], mask, cs["X_before"], cs["U_before"], case["weight"])
            tw.check_cold_start(x, u, want_X, want_U, tabs, mask, "masked" if mask is not None else "all")
    finally:
        s.close()
    n = tabs["n_nodes"]
    assert n.min() == 1 and n.max() == cases.NMAX and set(np.concatenate([tabs["mode"][b, :n[b]] for b in range(cases.B)])) == {0, 1, 2, 3}


def test_policy_matches_the_twin_at_the_edges(params, case):
    q = cases.policy_queries(case, params)
    tabs = case["prev"]
    want = tw.policy(tabs, case["X"], case["U"], q["t_now"], q["rbd"], q["walk"], params["config"]["default_joint_state"])
    s = _solver(params)
    try:
        s.set_references(cases.with_references(tabs, params))
        s.set_trajectory(case["X"], case["U"])                       # NaN beyond n: the policy may read none of it
        s.publish()
        got = s.wbc_update(q["t_now"], q["rbd"], walk_flag=q["walk"])
    finally:
        s.close()
    worst = tw.check_policy(got, want, q["what"])
    print(f"policy, device: worst interpolation error / bound {worst:.3f}")


def test_tick_path_shifts_per_range(params):
    """hb_tick_resident on three instance ranges: every range keeps its own grid (launch_grid_save on a view of the batch) and brings its own
    slice of the iterate onto its new tables, on its own stream."""
    from hunter_bipedal_control_amd import abi, workload
    from hunter_bipedal_control_amd.solver import HunterSolver
    B, N = 7, 20
    nmax = N + 6
    rng = np.random.default_rng(21)
    s = HunterSolver(params, batch=B, max_nodes=nmax, sqp_iterations=0)
    try:
        w = workload.device_trot_batch(s, params, n_intervals=N)
        s.set_resident_inputs(w["x0"], w["t_now"], w["rbd"])
        s.set_chunks(3)
        xh0 = np.zeros((B, 18))
        xh0[:, 0:3] = w["rbd"][:, 3:6]
        xh0[:, 6:18] = np.asarray(s.eval_foot_kinematics(w["x0"], np.zeros((B, 22)))[0]).reshape(B, 12)
        s.estimator_reset(abi.make_estimator_config(params), xh0)

        def tick(t_now):
            quat = np.tile([0.0, 0.0, 0.0, 1.0], (B, 1)) + 0.01 * rng.standard_normal((B, 4))
            quat /= np.linalg.norm(quat, axis=1, keepdims=True)
            wl, al = 0.05 * rng.standard_normal((B, 3)), np.tile([0.0, 0.0, 9.81], (B, 1)) + 0.1 * rng.standard_normal((B, 3))
            qj, qdj = w["rbd"][:, 6:16] + 0.01 * rng.standard_normal((B, 10)), 0.1 * rng.standard_normal((B, 10))
            s.tick_resident(0.002, quat, wl, al, qj, qdj, np.ones((B, 4), dtype=np.int32), t_now, w["horizon"], w["cmd"])
            assert s.refgen_status().max() == 0
            return s.get_references()

        t1 = w["t_now"] + 0.01 + 0.003 * np.arange(B)                  # every instance on a grid of its own
        T1 = tick(t1)
        X = np.array(params["config"]["initial_state"], dtype=float) + 0.05 * rng.standard_normal((B, nmax + 1, 22))
        U = tw.weight_compensation(T1["mode"], tw.robot_weight(params)) + rng.standard_normal((B, nmax, 22))
        for b in range(B):
            X[b, T1["n_nodes"][b] + 1:] = np.nan
            U[b, T1["n_nodes"][b]:] = np.nan
        s.set_trajectory(X, U)
        T2 = tick(t1 + 0.048)
        got_X, got_U = s.get_solution()
    finally:
        s.close()
    assert not np.array_equal(T1["t"], T2["t"])
    everyone = np.ones(B, dtype=np.int32)
    want_X, want_U, plan = tw.warm_shift(T1, X, U, T2, everyone, tw.robot_weight(params))
    worst = tw.check_shift(got_X, got_U, want_X, want_U, plan, T2, everyone, "tick")
    used = plan["bx"] == tw.INTERP
    assert used.sum() > 0 and (plan["bx"] == tw.BEYOND).sum() > 0, "the second grid must overlap the first and reach beyond it"
    print(f"tick path: worst interpolation error / bound {worst:.3f}")
