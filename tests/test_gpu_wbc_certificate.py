"""GPU: the KKT certificate and dual solution of the WeightedWbc QP (k_wbc_cert, hb_wbc_set_certificate / hb_wbc_get_certificate).
numpy recomputes the residuals from the oracle's rows (oracle.wbc_problem, the reference's constraint order), the device's sol and the
device's dual; the certificate kernel leaves sol / status / iterations bit-identical to k_wbc on every launch path."""
import numpy as np
import pytest

from hunter_bipedal_control_amd import workload
from test_wbc_certificate_host import _fast_inputs, _mixed_inputs, numpy_certificate

pytestmark = pytest.mark.gpu

NAMES = ("r_eq", "r_in", "r_stat", "r_dual", "r_comp")
# bounds of a certified instance: primal rows 1e-9 absolute, the rest relative to `scale` as measured;
# r_stat / scale <= 1e-8 is SURVEY.md §8d's KKT bound
BOUND_EQ, BOUND_IN, BOUND_STAT, BOUND_DUAL, BOUND_COMP = 1e-9, 1e-9, 1e-8, 1e-7, 1e-9


def _certified(c, idx=slice(None)):
    s = c["scale"][idx]
    return ((c["r_eq"][idx] <= BOUND_EQ) & (c["r_in"][idx] <= BOUND_IN) & (c["r_stat"][idx] <= BOUND_STAT * s)
            & (c["r_dual"][idx] <= BOUND_DUAL * s) & (c["r_comp"][idx] <= BOUND_COMP * s))


def _check_against_numpy(oracle, c, sol, xd, ud, rbd, mode, stance, idx):
    for r, i in enumerate(idx):
        pr = oracle.wbc_problem(xd[r], ud[r], rbd[r], int(mode[r]), bool(stance[r]))
        ref = numpy_certificate(pr, sol[i], c["dual"][i])
        scale = c["scale"][i]
        assert abs(scale - ref["scale"]) <= 1e-12 * ref["scale"], i
        for name in NAMES:
            assert abs(c[name][i] - ref[name]) <= 1e-9 * scale, (i, name, c[name][i], ref[name])
        n = pr["Aeq"].shape[0] + pr["D"].shape[0]
        assert not c["dual"][i, n:].any()
        assert pr["Aeq"].shape[0] <= c["n_active"][i] <= 38


def test_direct_mix_certificate_matches_numpy(params, oracle):
    """hb_wbc_update_direct on the 64-instance mix of modes 3 / 3 / 2 / 1 / 0 with stance: every instance certified, and numpy's
    residuals at the device's sol and dual agree with the device's certificate within 1e-9 * scale."""
    from hunter_bipedal_control_amd.solver import HunterSolver
    B = 64
    xd, ud, rbd, mode, stance = _mixed_inputs(params, B, 7)
    s = HunterSolver(params, batch=B, max_nodes=4)
    try:
        s.wbc_set_certificate(True)
        sol, status = s.wbc_update_direct(xd, ud, rbd, mode, stance)
        c = s.wbc_certificate()
        c2 = s.wbc_certificate(10, 5)
    finally:
        s.close()
    assert status.max() == 0
    assert _certified(c).all(), {k: float(np.max(c[k] / (1.0 if k in ("r_eq", "r_in") else c["scale"]))) for k in NAMES}
    assert (c["eps"] == 1e-8).all() and (c["scale"] >= 1.0).all()
    for k in NAMES + ("dual", "scale", "n_active"):
        assert np.array_equal(c2[k], c[k][10:15]), k
    _check_against_numpy(oracle, c, sol, xd, ud, rbd, mode, stance, range(B))
    print("direct mix: r_stat / scale median %.1e max %.1e, r_eq max %.1e" % (np.median(c["r_stat"] / c["scale"]),
                                                                                (c["r_stat"] / c["scale"]).max(), c["r_eq"].max()))


def _run_direct(params, xd, ud, rbd, mode, stance, cert, **cfg):
    from hunter_bipedal_control_amd.solver import HunterSolver
    s = HunterSolver(params, batch=xd.shape[0], max_nodes=4, **cfg)
    try:
        if cert:
            s.wbc_set_certificate(True)
        sol, status = s.wbc_update_direct(xd, ud, rbd, mode, stance)
        it = s.get_wbc_iterations()
        c = s.wbc_certificate() if cert else None
    finally:
        s.close()
    return sol, status, it, c


def test_certificate_leaves_the_solution_bit_identical_direct(params):
    xd, ud, rbd, mode, stance = _mixed_inputs(params, 64, 7)
    xf, uf, rf, mf, sf = _fast_inputs(params, 24, 5)
    for inp in ((xd, ud, rbd, mode, stance), (xf, uf, rf, mf, sf)):
        a = _run_direct(params, *inp, cert=False)
        b = _run_direct(params, *inp, cert=True)
        for k in range(3):
            assert np.array_equal(a[k], b[k]), k


def _trot_ctx(params, B, N, cert, chunks):
    from hunter_bipedal_control_amd.solver import HunterSolver
    s = HunterSolver(params, batch=B, max_nodes=N)
    w = workload.device_trot_batch(s, params, n_intervals=N)
    s.set_resident_inputs(w["x0"], w["t_now"], w["rbd"])
    s.set_chunks(chunks)
    if cert:
        s.wbc_set_certificate(True)
    return s, w


def test_certificate_leaves_the_solution_bit_identical_resident_ranges(params):
    """hb_step_resident with 4 instance ranges on a 512-instance trot batch: sol / status / iterations bit-identical with the certificate
    on and off over steps that replay captured range graphs; switching it on mid-run re-captures them (the certificate of the switched
    context equals that of a context that had it on all along)."""
    B, N = 512, 50
    on, _ = _trot_ctx(params, B, N, True, 4)
    off, _ = _trot_ctx(params, B, N, False, 4)
    try:
        # (no read-back between steps: a read joins the ranges and the next step forks again, without graphs)
        for _ in range(5):
            on.step_resident()
            off.step_resident()
        a = on.get_wbc_solution() + (on.get_wbc_iterations(),)
        b = off.get_wbc_solution() + (off.get_wbc_iterations(),)
        for k in range(3):
            assert np.array_equal(a[k], b[k]), k
        with pytest.raises(Exception, match=r"failed \(-3\)"):
            off.wbc_certificate()
        assert off.chunk_counters()["graph_launches"] > 0 and on.chunk_counters()["graph_launches"] > 0, "graph replays must be covered"
        captures_before = off.chunk_counters()["captures"]
        off.wbc_set_certificate(True)
        for _ in range(5):
            on.step_resident()
            off.step_resident()
        assert off.chunk_counters()["captures"] > captures_before, "switching must re-capture the range graphs"
        ca, cb = on.wbc_certificate(), off.wbc_certificate()
        for k in NAMES + ("dual", "n_active", "scale"):
            assert np.array_equal(ca[k], cb[k]), k
        a = on.get_wbc_solution() + (on.get_wbc_iterations(),)
        b = off.get_wbc_solution() + (off.get_wbc_iterations(),)
        for k in range(3):
            assert np.array_equal(a[k], b[k]), k
        assert (ca["n_active"] >= 16).all() and _certified(ca).all()
    finally:
        on.close()
        off.close()


def test_configs2_batch_certified(params, oracle):
    """BASELINE configs[2] (4096 x N = 100, workload.device_trot_batch), one chunked resident step: every instance within the bounds;
    a strided 64-instance sample recomputed in numpy (the WBC inputs of the step read back by one more resident WBC call)."""
    B, N = 4096, 100
    s, w = _trot_ctx(params, B, N, True, 4)   # (bench.py's ranges for this batch)
    try:
        s.step_resident()
        sol, status = s.get_wbc_solution()
        c = s.wbc_certificate()
        # the step's policy inputs: one more WBC call on the same resident inputs (same policy, same time, same rbd)
        r = s.wbc_update()
        c2 = s.wbc_certificate()
    finally:
        s.close()
    assert status.max() == 0 and np.array_equal(r["sol"], sol) and np.array_equal(r["status"], status)
    for k in NAMES + ("dual",):
        assert np.array_equal(c2[k], c[k]), k
    rel = c["r_stat"] / c["scale"]
    print("configs[2]: r_stat / scale median %.2e p99 %.2e max %.2e; r_dual / scale max %.2e; r_comp / scale max %.2e; r_eq max %.2e; "
          "r_in max %.2e; n_active median %d" % (np.median(rel), np.percentile(rel, 99), rel.max(), (c["r_dual"] / c["scale"]).max(),
                                                 (c["r_comp"] / c["scale"]).max(), c["r_eq"].max(), c["r_in"].max(), np.median(c["n_active"])))
    assert _certified(c).all(), int((~_certified(c)).sum())
    idx = np.arange(0, B, B // 64)
    _check_against_numpy(oracle, c, sol, r["x_des"][idx], r["u_des"][idx], w["rbd"][idx], r["mode"][idx], np.zeros(B, dtype=np.int32)[idx],
                         idx)


def test_certificate_sees_the_tikhonov_bias(params):
    """wbc_reg_steps = 0 (the eps-regularised minimiser) against 1 (the reference's rule) on the same inputs: the stationarity residual
    of the unregularised problem is the regulariser's bias, median at least 10x larger without the step."""
    xd, ud, rbd, mode, stance = _mixed_inputs(params, 64, 7)
    med = {}
    for reg in (0, 1):
        c = _run_direct(params, xd, ud, rbd, mode, stance, cert=True, wbc_reg_steps=reg)[3]
        med[reg] = np.median(c["r_stat"] / c["scale"])
    assert med[0] >= 10.0 * med[1], med


def test_maxiter_instances_are_not_certified(params):
    """An iteration budget at the median of the fast-motion inputs' needs: the MAXITER instances keep their previous solution (zero in a
    fresh context) and their certificate shows it (residuals > 1e-6 * scale); the instances that finished are certified."""
    xd, ud, rbd, mode, stance = _fast_inputs(params, 24, 5)
    it = _run_direct(params, xd, ud, rbd, mode, stance, cert=False)[2]
    budget = int(np.median(it))
    sol, status, _, c = _run_direct(params, xd, ud, rbd, mode, stance, cert=True, wbc_max_iter=budget)
    bad, ok = status == 1, status == 0
    assert bad.any() and ok.any(), status
    assert not sol[bad].any()
    worst = np.maximum(np.maximum(c["r_stat"], c["r_in"]), c["r_eq"])
    assert (worst[bad] > 1e-6 * c["scale"][bad]).all()
    assert _certified(c, ok).all()
    # every instance fails with a budget below the equality rows
    sol, status, _, c = _run_direct(params, xd, ud, rbd, mode, stance, cert=True, wbc_max_iter=2)
    assert (status == 1).all() and (np.maximum(np.maximum(c["r_stat"], c["r_in"]), c["r_eq"]) > 1e-6 * c["scale"]).all()


def test_refusals(params):
    from hunter_bipedal_control_amd.solver import HunterHipError, HunterSolver
    s = HunterSolver(params, batch=4, max_nodes=4, wbc_type=1)
    try:
        with pytest.raises(HunterHipError, match=r"failed \(-1\).*HierarchicalWbc"):
            s.wbc_set_certificate(True)
    finally:
        s.close()
    s = HunterSolver(params, batch=4, max_nodes=4)
    try:
        with pytest.raises(HunterHipError, match=r"failed \(-3\)"):
            s.wbc_certificate()
        s.wbc_set_certificate(True)
        with pytest.raises(HunterHipError, match=r"failed \(-3\)"):   # enabled, but no WBC call since
            s.wbc_certificate()
        with pytest.raises(HunterHipError, match=r"failed \(-1\)"):
            s.wbc_certificate(2, 3)
    finally:
        s.close()
