"""GPU: the per-level certificate of the HierarchicalWbc cascade (k_hwbc_cert, hb_hwbc_set_certificate / hb_hwbc_get_certificate).
The numpy twin (tests/_hwbc_cert.py) recomputes every field from the oracle's task rows at the device's x_levels / slack0 / dual; an
instance is certified against the oracle's OWN cascade on the same input set (10 x its worst per level and figure); the certificate
kernel leaves sol / status bit-identical to k_hwbc on every launch path.

Measured on an MI355X (worst over the set, r_stat / r_comp / r_dual relative to scale, levels 0 / 1 / 2): see DESIGN.md §5 item 14."""
import numpy as np
import pytest

import _hwbc_cert as H
from hunter_bipedal_control_amd import workload
from test_hwbc_certificate_host import check_against_twin

pytestmark = pytest.mark.gpu

ARRAYS = ("cert", "x_levels", "slack0", "dual")


def _run_direct(params, inputs, cert, **cfg):
    from hunter_bipedal_control_amd.solver import HunterSolver
    xd, ud, rbd, mode, stance = inputs
    s = HunterSolver(params, batch=xd.shape[0], max_nodes=4, wbc_type=1, **cfg)
    try:
        if cert:
            s.hwbc_set_certificate(True)
        sol, status = s.wbc_update_direct(xd, ud, rbd, mode, stance)
        c = s.hwbc_certificate() if cert else None
        c2 = s.hwbc_certificate(10, 5) if cert else None
    finally:
        s.close()
    return sol, status, c, c2


def _instance(c, i):
    return {k: c[k][i] for k in ARRAYS}


@pytest.mark.parametrize("inputs", ["mixed", "fast"])
def test_direct_certificate_matches_numpy_and_is_certified(params, oracle, inputs):
    """hb_wbc_update_direct on the 64-instance mix of every mode and on the 24 fast-motion instances (violated level 0, non-empty working
    sets): every instance certified against the oracle's cascade, every field within 1e-9 * scale of the twin, a sub-range read equal
    to the slice of the full read."""
    ref = H.reference(oracle, params, inputs)
    sol, status, c, c2 = _run_direct(params, ref["inputs"], True)
    print(inputs, "oracle", H.worst_table(ref["cert"]), "device", H.worst_table(c["cert"]))
    assert status.max() == 0
    assert np.array_equal(c["x_levels"][:, 2], sol)
    for k in ARRAYS + tuple(s for s in ("r_stat", "n_free", "n_active", "scale")):
        assert np.array_equal(c2[k], c[k][10:15]), k
    for i in range(len(status)):
        check_against_twin(ref["tasks"][i], _instance(c, i))
    ok = H.certified(c["cert"], ref["bounds"])
    assert ok.all(), (np.flatnonzero(~ok), H.worst_table(c["cert"]), ref["bounds"])
    if inputs == "fast":
        assert c["n_active"][:, 1:].sum() > 0 and (c["slack0"] > 0.0).any()


def test_certificate_leaves_the_solution_bit_identical_direct(params, oracle):
    for name in ("mixed", "fast"):
        inp = H.reference(oracle, params, name)["inputs"]
        a = _run_direct(params, inp, False)
        b = _run_direct(params, inp, True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name


def _trot_ctx(params, B, N, cert, chunks):
    from hunter_bipedal_control_amd.solver import HunterSolver
    s = HunterSolver(params, batch=B, max_nodes=N + 4, wbc_type=1)
    w = workload.device_trot_batch(s, params, n_intervals=N)
    s.set_resident_inputs(w["x0"], w["t_now"], w["rbd"])
    s.set_chunks(chunks)
    if cert:
        s.hwbc_set_certificate(True)
    return s, w


def test_certificate_leaves_the_solution_bit_identical_resident_ranges(params, oracle):
    """hb_step_resident with 4 instance ranges on the hierarchical shape of tests/test_gpu_timed_path.py (256 x N = 40): sol / status
    bit-identical with the certificate on and off over steps that replay captured range graphs; switching it on mid-run re-captures
    them, and the certificates of the switched context equal those of a context that had it on all along.  Every instance is
    certified against the oracle's cascade on the WBC inputs of the last step."""
    B, N = 256, 40
    on, w = _trot_ctx(params, B, N, True, 4)
    off, _ = _trot_ctx(params, B, N, False, 4)
    try:
        # (no read-back between steps: a read joins the ranges and the next step forks again, without graphs)
        for _ in range(5):
            on.step_resident()
            off.step_resident()
        a, b = on.get_wbc_solution(), off.get_wbc_solution()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        with pytest.raises(Exception, match=r"failed \(-3\)"):
            off.hwbc_certificate()
        assert off.chunk_counters()["graph_launches"] > 0 and on.chunk_counters()["graph_launches"] > 0, "graph replays must be covered"
        captures_before = off.chunk_counters()["captures"]
        off.hwbc_set_certificate(True)
        for _ in range(5):
            on.step_resident()
            off.step_resident()
        assert off.chunk_counters()["captures"] > captures_before, "switching must re-capture the range graphs"
        ca, cb = on.hwbc_certificate(), off.hwbc_certificate()
        for k in ARRAYS:
            assert np.array_equal(ca[k], cb[k]), k
        a, b = on.get_wbc_solution(), off.get_wbc_solution()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[1].max() == 0 and np.array_equal(ca["x_levels"][:, 2], a[0])
        # the last step's policy inputs: one more WBC call on the same resident inputs (same policy, same time, same rbd)
        r = on.wbc_update()
        c2 = on.hwbc_certificate()
    finally:
        on.close()
        off.close()
    assert np.array_equal(r["sol"], a[0])
    for k in ARRAYS:
        assert np.array_equal(c2[k], ca[k]), k
    eps = params["config"].get("wbc_eps_reg", 1e-8)
    oc = []
    for i in range(B):
        t = H.tasks_of(oracle, r["x_des"][i], r["u_des"][i], w["rbd"][i], r["mode"][i])
        cert_o, _, sts = H.oracle_certificate(oracle, t, eps, 1)
        assert max(sts) == 0
        oc.append(cert_o)
    bounds = H.bounds_from_oracle(np.array(oc))
    print("resident 256 x 40: oracle", H.worst_table(np.array(oc)), "device", H.worst_table(ca["cert"]))
    ok = H.certified(ca["cert"], bounds)
    assert ok.all(), (np.flatnonzero(~ok), H.worst_table(ca["cert"]), bounds)


def test_refusals(params):
    from hunter_bipedal_control_amd.solver import HunterHipError, HunterSolver
    s = HunterSolver(params, batch=4, max_nodes=4)
    try:
        with pytest.raises(HunterHipError, match=r"failed \(-1\).*HierarchicalWbc"):
            s.hwbc_set_certificate(True)
    finally:
        s.close()
    s = HunterSolver(params, batch=4, max_nodes=4, wbc_type=1)
    try:
        with pytest.raises(HunterHipError, match=r"failed \(-3\)"):
            s.hwbc_certificate()
        s.hwbc_set_certificate(True)
        with pytest.raises(HunterHipError, match=r"failed \(-3\)"):   # enabled, but no WBC call since
            s.hwbc_certificate()
        with pytest.raises(HunterHipError, match=r"failed \(-1\)"):
            s.hwbc_certificate(2, 3)
    finally:
        s.close()


def test_iteration_limit_instances_are_reported_finite(params, oracle):
    """wbc_max_iter = 2 on the fast-motion set (the oracle leaves 10 of 24 at status 1): some instance stops on the limit, every field
    is finite, every instance that finished is certified."""
    ref = H.reference(oracle, params, "fast")
    sol, status, c, _ = _run_direct(params, ref["inputs"], True, wbc_max_iter=2)
    assert (status != 0).any(), status
    assert all(np.isfinite(c[k]).all() for k in ARRAYS)
    ok = H.certified(c["cert"], ref["bounds"])
    assert ok[status == 0].all(), (np.flatnonzero(~ok & (status == 0)), H.worst_table(c["cert"][status == 0]))
