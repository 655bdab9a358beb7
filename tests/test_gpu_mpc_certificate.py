"""-m gpu: the on-demand KKT certificate of the MPC's stage QP (hb_mpc_get_certificate: k_mpc_cert_nodes + k_mpc_cert_sweep) and the
stage-QP export (hb_mpc_get_lq) on the eight ragged all-mode instances of test_ragged_horizons_all_modes_and_off_grid_events, against
the dense KKT system of the exported QP in numpy (tests/_mpc_cert.py; bounds as in tests/test_mpc_certificate_host.py).

Measured on an MI355X, maxima over the eight instances after one hb_mpc_solve from the cold start (host twin in brackets):
R_DYN 2.2e-16 (1.1e-16); R_STAT / SCALE 5.0e-14 (7.5e-14); dx / u~ / lambda against the dense solve 1.7e-13 / 1.5e-10 / 1.7e-11
(1.5e-13 / 1.5e-10 / 4.4e-11).  With sqp_iterations = 3 (third iteration): 1.4e-17; 5.3e-14; 3.1e-13 / 1.5e-10 / 2.9e-11."""
import numpy as np
import pytest

import _mpc_cert as mc
from hunter_bipedal_control_amd import abi, workload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def problem(params):
    return mc.ragged_problem(params)


def _ctx(params, refs, x0, **kw):
    from hunter_bipedal_control_amd.solver import HunterSolver
    s = HunterSolver(params, batch=x0.shape[0], max_nodes=mc.NMAX, **kw)
    s.set_references(refs)
    s.reset(x0)
    return s


def _row(c, i):
    return {name: c[name][i] for name in mc.FIELDS}


def _riccati_u(lq, n, dx):
    """u~ = K~ dx + k~ with the gains of numpy's own backward recursion on the exported QP (S_n = 0)."""
    S, s = np.zeros((22, 22)), np.zeros(22)
    K, kk = [None] * n, [None] * n
    for k in range(n - 1, -1, -1):
        A, B, b, Q, P, R, q, r = (lq[key][k] for key in mc.LQ_KEYS)
        Huu, Hux, hu = R + B.T @ S @ B, P + B.T @ S @ A, r + B.T @ (S @ b + s)
        K[k], kk[k] = -np.linalg.solve(Huu, Hux), -np.linalg.solve(Huu, hu)
        s = q + A.T @ (S @ b + s) + Hux.T @ kk[k]
        S = Q + A.T @ S @ A + Hux.T @ K[k]
        S = 0.5 * (S + S.T)
    return np.stack([K[k] @ dx[k] + kk[k] for k in range(n)])


def _check_instances(s, refs, which, tag):
    """Tests 1-3 of the certificate for the instances `which` of a solved context; -> the worst figures."""
    dx, _ = s.get_step()
    c = s.mpc_certificate()
    worst = {}
    for i in which:
        n = int(refs["n_nodes"][i])
        lq = s.mpc_lq(i)
        assert lq["A"].shape[0] == n and c["n_nodes"][i] == n
        u, lam = c["u_til"][i], c["costate"][i]
        m = mc.check_against_numpy(lq, n, dx[i, :n + 1], u[:n], lam[:n + 1], _row(c, i), tag=f"{tag}[{i}]")
        # u~ and the costates against numpy's recursions on the exported data; rows behind the horizon are zero
        un, ln = _riccati_u(lq, n, dx[i]), mc.costate_recursion(lq, n, dx[i], u)
        assert np.abs(u[:n] - un).max() <= 1e-9 * max(1.0, np.abs(un).max()), (i, np.abs(u[:n] - un).max())
        assert np.abs(lam[:n + 1] - ln).max() <= 1e-9 * max(1.0, np.abs(ln).max()), (i, np.abs(lam[:n + 1] - ln).max())
        assert not u[n:].any() and not lam[n:].any()
        assert np.array_equal(lq["Q"], lq["Q"].transpose(0, 2, 1)) and (lq["n_til"] >= 6).all()
        for k, v in m.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"{tag}: worst over {len(which)} instances: " + " ".join(f"{k}={v:.3e}" for k, v in worst.items()))
    return worst


def test_certificate_matches_numpy(params, problem):
    """GPU test 1: one hb_mpc_solve, then hb_mpc_get_lq + hb_mpc_get_step + hb_mpc_get_certificate against numpy as CPU tests 1-3."""
    refs, x0 = problem
    s = _ctx(params, refs, x0)
    try:
        s.mpc_solve(x0)
        assert s.mpc_status().max() == 0
        _check_instances(s, refs, range(len(mc.SPECS)), "device")
    finally:
        s.close()


def test_read_only_and_sub_ranges(params, problem):
    """GPU test 2: two contexts, three MPC calls each on the same inputs; one reads the certificate and the stage QP after every call.
    Solutions, steps, performance and status are bit-identical; a sub-range call equals the rows of the whole-batch call."""
    refs, x0 = problem
    a, b = _ctx(params, refs, x0), _ctx(params, refs, x0)
    try:
        for it in range(3):
            a.mpc_solve(x0)
            b.mpc_solve(x0)
            c = a.mpc_certificate()
            a.mpc_lq(it)
            sub = a.mpc_certificate(2, 3)
            for key in ("cert", "costate", "u_til"):
                assert np.array_equal(sub[key], c[key][2:5]), (it, key)
            one = a.mpc_certificate(7, 1)
            assert np.array_equal(one["cert"], c["cert"][7:8]) and np.array_equal(one["costate"], c["costate"][7:8])
            assert np.array_equal(a.mpc_certificate()["cert"], c["cert"])
            for ga, gb in zip(a.get_solution() + a.get_step() + (a.get_performance(), a.mpc_status()),
                              b.get_solution() + b.get_step() + (b.get_performance(), b.mpc_status())):
                assert np.array_equal(ga, gb), it
        assert (c["n_nodes"] == refs["n_nodes"]).all()
    finally:
        a.close()
        b.close()


def test_resident_path_with_ranges(params, problem):
    """GPU test 3: two instance ranges, hb_step_resident x 2: the certificate afterwards equals the certificate after the same two steps
    through hb_mpc_solve bit for bit (the getter joins the range streams)."""
    refs, x0 = problem
    rbd = np.stack([workload.rbd_from_state(x0[i], i) for i in range(x0.shape[0])])
    a, b = _ctx(params, refs, x0), _ctx(params, refs, x0)
    try:
        a.set_resident_inputs(x0, refs["t"][:, 0].copy(), rbd)
        a.set_chunks(2)
        for _ in range(2):
            a.step_resident()
            b.mpc_solve(x0)
        ca, cb = a.mpc_certificate(), b.mpc_certificate()
        for key in ("cert", "costate", "u_til"):
            assert np.array_equal(ca[key], cb[key]), key
        assert (ca["n_nodes"] == refs["n_nodes"]).all()
        la, lb = a.mpc_lq(6), b.mpc_lq(6)
        for key in la:
            assert np.array_equal(la[key], lb[key]), key
    finally:
        a.close()
        b.close()


def test_certificate_refers_to_the_last_sqp_iteration(params, problem):
    """GPU test 4: sqp_iterations = 3: the exported QP, the step and the certificate are those of the third iteration."""
    refs, x0 = problem
    s = _ctx(params, refs, x0, sqp_iterations=3)
    one = _ctx(params, refs, x0)
    try:
        s.mpc_solve(x0)
        one.mpc_solve(x0)
        _check_instances(s, refs, range(len(mc.SPECS)), "third iteration")
        assert not np.array_equal(s.mpc_certificate()["obj"], one.mpc_certificate()["obj"])
    finally:
        s.close()
        one.close()


def test_nan_instance_is_not_certified(params, problem):
    """GPU test 5 (the contained failure of test_gpu_failure_surface.py: a NaN in one instance's observation): that instance has
    N_NODES = 0, NaN fields, zero costate and u~; its neighbours are certified as in test 1."""
    refs, x0 = problem
    s = _ctx(params, refs, x0)
    try:
        bad = x0.copy()
        bad[2, 7] = np.nan
        s.mpc_solve(bad)
        st = s.mpc_status()
        assert st[2] == abi.HB_INST_NAN and (np.delete(st, 2) == 0).all(), st
        c = s.mpc_certificate()
        assert c["n_nodes"][2] == 0 and np.isnan(c["cert"][2, :7]).all()
        assert not c["costate"][2].any() and not c["u_til"][2].any()
        _check_instances(s, refs, [i for i in range(len(mc.SPECS)) if i != 2], "neighbours")
    finally:
        s.close()


def test_refusals(params, problem):
    """GPU test 6: HB_ERR_STATE before any solve and after new references; HB_ERR_ARG on a bad range; a second solve makes it valid."""
    from hunter_bipedal_control_amd.solver import HunterHipError
    refs, x0 = problem
    s = _ctx(params, refs, x0)
    try:
        with pytest.raises(HunterHipError, match=r"failed \(-3\).*no MPC call has completed"):
            s.mpc_certificate()
        with pytest.raises(HunterHipError, match=r"failed \(-3\).*no MPC call has completed"):
            s.mpc_lq(0)
        s.mpc_solve(x0)
        first = s.mpc_certificate()
        for rng in ((-1, 2), (7, 2), (8, 1), (0, 0), (0, 9)):
            with pytest.raises(HunterHipError, match=r"failed \(-1\)"):
                s.mpc_certificate(*rng)
        for inst in (-1, 8):
            with pytest.raises(HunterHipError, match=r"failed \(-1\)"):
                s.mpc_lq(inst)
        s.set_references(refs)
        with pytest.raises(HunterHipError, match=r"failed \(-3\).*replaced since the last MPC call"):
            s.mpc_certificate()
        with pytest.raises(HunterHipError, match=r"failed \(-3\).*replaced since the last MPC call"):
            s.mpc_lq(0)
        s.mpc_solve(x0)
        again = s.mpc_certificate()
        assert (again["n_nodes"] == refs["n_nodes"]).all() and np.isfinite(again["cert"]).all() and np.isfinite(first["cert"]).all()
        s.reset(x0)
        with pytest.raises(HunterHipError, match=r"failed \(-3\)"):
            s.mpc_certificate()
    finally:
        s.close()
