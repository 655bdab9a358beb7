"""-m gpu: every block of the LQ stage record the device writes (k_lq_trip / k_lq, read back with hb_mpc_get_lq + hb_mpc_get_recovery), node
by node, against the oracle's unprojected node LQ lifted through the record's own change of input variables (tests/_lqrec.py; the host
twin: tests/test_lq_record_host.py) — on the eight ragged all-mode instances (268 nodes) at the cold start (a) and at the seeded generic
iterate with planted barrier arguments (b), for the product's choice of form, trips of 16 nodes and the one-node kernel — and the
recovery identity of the forward sweep, du = T u~ + K dx + k, for its row and its wave form.

Bounds: structure exactly; 1e-12 per block relative to max(1, max |expected block|) (200 x the host twin's measured floor, two decades
under the model tolerance 1e-10); the identity 1e-12 max(1, |du|_inf of the instance).
Measured on an MI355X, maxima over the 268 nodes, (a) / (b); trips (the product's choice and trips of 16 give identical figures), then
the one-node kernel where it differs; the host twin's figures stand in tests/test_lq_record_host.py, all in the same decade:
  D T 4.1e-16 / 1.3e-15 (one node 3.8e-16 / 8.1e-16)   Dt(D K + C) 2.4e-15 / 4.6e-15 (2.7e-15 / 3.9e-15)   Dt(D k + e) 8.9e-16 / 3.9e-15 (1.3e-15 / 3.7e-15)
  A~ 6.5e-16 / 8.4e-16 (5.6e-16 / 8.2e-16)   B~ 8.7e-18 / 6.9e-18   b~ 5.6e-17 / 4.4e-16 (8.3e-17 / 5.3e-16)   Q~ 1.2e-15 / 2.2e-15 (1.1e-15 / 4.4e-15)
  P~ 1.9e-15 / 3.0e-15 (1.7e-15 / 2.1e-15)   R~ 1.0e-16 / 5.8e-16 (9.7e-17 / 6.0e-16)   q~ 1.3e-15 / 3.2e-15 (1.6e-15 / 3.5e-15)   r~ 6.7e-16 / 1.6e-15 (3.9e-16 / 1.7e-15)
  qf 1.9e-15 / 4.4e-15 (2.3e-15 / 5.9e-15)   rf 2.8e-16 / 1.8e-15 (3.1e-16 / 1.1e-15)   cost dt 1.9e-15 / 6.1e-15 (2.2e-15 / 3.7e-15)
  dyn_sse dt 1.9e-19 / 2.8e-17   eq_sse dt 3.3e-16 / 2.2e-15 (4.7e-16 / 2.7e-15)   dq 0 / 2.2e-16
The largest figure of any block, form and point is 6.1e-15 (cost dt, trips, (b), instance 6 node 43): no bound is raised.
Forward sweep, |du - (T u~ + K dx + k)| / max(1, |du|_inf): 1.0e-16 at (a), 1.3e-16 at (b), row and wave form alike.
"""
import ctypes as C

import numpy as np
import pytest

import _lqrec as lr
import _mpc_cert as mc
from hunter_bipedal_control_amd import abi

pytestmark = pytest.mark.gpu

BOUND = 1e-12
BLOCK_BOUNDS = {}   # {check: raised bound (<= 1e-10, never a structural check)}: none is raised
LQ_FORMS = {"product": abi.FORM.NONE, "trip16": abi.FORM_RANGES["LQ_TRIP_LEN"][0] + 15, "one_node": abi.FORM.LQ_ONE_NODE}
FWD_FORMS = {"row": abi.FORM.RIC_FWD_ROW, "wave": abi.FORM.RIC_FWD_WAVE}


@pytest.fixture(scope="module")
def problem(params, oracle):
    return lr.iterates(params, oracle)


@pytest.fixture(scope="module")
def nodes(problem):
    """The node inputs per point and instance; the oracle's LQ of a node is computed once and kept with it."""
    refs, _, points = problem
    return {name: [lr.instance_nodes(refs, x, u, i) for i in range(len(mc.SPECS))] for name, (x, u) in points.items()}


def _solved(params, refs, x, u, reserved):
    """One context of batch 8, max_nodes 64: the iterate set, one SQP iteration from x0 = x[:, 0]."""
    from hunter_bipedal_control_amd.solver import HunterSolver
    s = HunterSolver(params, batch=x.shape[0], max_nodes=mc.NMAX, sqp_iterations=1, reserved=reserved)
    try:
        s.set_references(refs)
        s.set_trajectory(x, u)
        s.mpc_solve(np.ascontiguousarray(x[:, 0]))
    except Exception:
        s.close()
        raise
    return s


def _records(s, i):
    rec = s.mpc_lq(i)
    rec.update(s.mpc_recovery(i))
    return rec


@pytest.mark.parametrize("point", ["a", "b"])
@pytest.mark.parametrize("form", list(LQ_FORMS))
def test_device_record_matches_the_lifted_oracle(params, oracle, problem, nodes, form, point):
    refs, _, points = problem
    x, u = points[point]
    s = _solved(params, refs, x, u, LQ_FORMS[form])
    try:
        worst, widths = {}, set()
        for i in range(len(mc.SPECS)):
            rec = _records(s, i)
            assert len(rec["dt"]) == len(rec["A"]) == int(refs["n_nodes"][i])
            fig = lr.check_record(oracle, nodes[point][i], rec, BOUND, tag=f"device {form} ({point})[{i}]", bounds=BLOCK_BOUNDS)
            lr.merge(worst, fig, i)
            widths |= set(rec["n_til"].tolist())
        print(f"device {form} ({point}), worst per check (figure, instance, node): " + " ".join(f"{k}={v:.2e}@{i}/{n}" for k, (v, i, n) in worst.items()))
        assert widths == {6, 9, 12}
    finally:
        s.close()


@pytest.mark.parametrize("form", list(FWD_FORMS))
def test_forward_sweep_recovers_the_input_step(params, problem, form):
    """hb_mpc_get_step's du against T u~ + K dx + k formed in numpy from the exported record, u~ of hb_mpc_get_certificate and the
    device's own dx, at both points: the first direct check of the device's input recovery (hb_riccati_solve's forward pass runs on
    the host).  The norm of the bound is that of the instance, as the certificate's U_MAX."""
    refs, _, points = problem
    for point, (x, u) in points.items():
        s = _solved(params, refs, x, u, FWD_FORMS[form])
        try:
            dx, du = s.get_step()
            u_til = s.mpc_certificate()["u_til"]
            assert np.isfinite(dx).all() and np.isfinite(du).all() and np.isfinite(u_til).all(), (point, s.mpc_status())
            worst = 0.0
            for i in range(len(mc.SPECS)):
                n = int(refs["n_nodes"][i])
                rec = s.mpc_recovery(i)
                want = np.stack([lr.recovered_du(int(refs["mode"][i, k]), {key: rec[key][k] for key in rec}, u_til[i, k], dx[i, k])
                                 for k in range(n)])
                err, scale = np.abs(du[i, :n] - want).max(), max(1.0, np.abs(want).max())
                worst = max(worst, err / scale)
                assert err <= 1e-12 * scale, (form, point, i, err, scale)
                assert not du[i, n:].any()
            print(f"forward sweep {form} ({point}): max |du - (T u~ + K dx + k)| / max(1, |du|_inf) = {worst:.2e}")
        finally:
            s.close()


def test_recovery_getter_refusals_and_rows_behind_the_horizon(params, problem):
    """hb_mpc_get_recovery refuses as hb_mpc_get_lq does (HB_ERR_STATE before a solve and after new tables, HB_ERR_ARG outside the batch),
    accepts null pointers, leaves the rows behind n zero and reads without changing anything."""
    from hunter_bipedal_control_amd.solver import HunterHipError, HunterSolver
    refs, x0, _ = problem
    s = HunterSolver(params, batch=x0.shape[0], max_nodes=mc.NMAX)
    try:
        s.set_references(refs)
        s.reset(x0)
        with pytest.raises(HunterHipError, match=r"failed \(-3\).*no MPC call has completed"):
            s.mpc_recovery(0)
        s.mpc_solve(x0)
        for inst in (-1, 8):
            with pytest.raises(HunterHipError, match=r"failed \(-1\).*hb_mpc_get_recovery: instance outside the batch"):
                s.mpc_recovery(inst)
        i = int(np.argmin(refs["n_nodes"]))    # n = 1
        Kx, dt = np.full((mc.NMAX, 10, 22), 7.0), np.full(mc.NMAX, 7.0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        assert s.lib.hb_mpc_get_recovery(s.ctx, C.c_int32(i), p(Kx), None, None, None, None, None, None, p(dt), None) == 0
        assert Kx[0].any() and dt[0] == refs["t"][i, 1] - refs["t"][i, 0] and not Kx[1:].any() and not dt[1:].any()
        before = s.get_solution() + s.get_step()
        first = s.mpc_recovery(6)
        again = s.mpc_recovery(6)
        assert all(np.array_equal(first[k], again[k]) for k in first)
        assert all(np.array_equal(a, b) for a, b in zip(before, s.get_solution() + s.get_step()))
        s.set_references(refs)
        with pytest.raises(HunterHipError, match=r"failed \(-3\).*replaced since the last MPC call"):
            s.mpc_recovery(0)
    finally:
        s.close()
