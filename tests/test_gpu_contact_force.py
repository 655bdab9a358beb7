"""k_contact_force (one thread per instance, 32 threads per block, a CfLegWork slab per thread carved out of one LDS array) across threads and
blocks, through estimator_contact_force(dt, tau, rbd) with rbd handed in, against oracle.contact_force.

B = 67: two full blocks and a last block with three live threads.  Six ticks with the observer state kept on the device (it is not read back:
the disturbance torque of tick k carries it), dt 0.001 / 0.002 / 0.005, wide states (tests/_cfcases.py).  Bounds, from the algorithm:
  * dist <= 1e-13 max(1, |dist|): sums of a few hundred products, no solve;
  * each leg's wrench and its two norms <= eps cond(A)^2 max(1, |cf|), A the leg's 5 x 6 block and |cf| the largest entry of the instance's
    16 outputs: the device solves the normal equations A A'.  A leg with cond(A) > 1e6 is left out; at most 5 % may be.  (With these states
    cond(A) stays below 1e2, and what the wrench carries is the rounding of dist over the smallest singular value of A: the emulator sits at
    0.6 of the bound.)
The first test is the same comparison on the host emulator (no GPU): it holds the bounds to the algorithm before the device is asked."""
import ctypes as C

import numpy as np
import pytest

import _cfcases as cc
from hunter_bipedal_control_amd import abi

EPS = float(np.finfo(np.float64).eps)
B, TICKS, DTS = 67, 6, (0.001, 0.002, 0.005)
_REF = {}


def _reference(params, oracle, dt):
    """-> rbd, tau, the oracle's dist[T][B][16] and cf[T][B][16], cond[T][B][2]; computed once per dt."""
    if dt not in _REF:
        cutoff = params["config"]["kalman"]["contact_force_cutoff_frequency"]
        rbd, tau = cc.wide_states(params, B, TICKS)
        if "cond" not in _REF:
            _REF["cond"] = np.array([[cc.leg_blocks(oracle, rbd[k, i])[1] for i in range(B)] for k in range(TICKS)])
        z = np.zeros((B, 16))
        out = [oracle.contact_force(cutoff, dt, z, rbd[k], tau[k]) for k in range(TICKS)]
        _REF[dt] = (rbd, tau, np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), _REF["cond"])
    return _REF[dt]


def _check(dist, cf, ref, label):
    rbd, tau, dist_o, cf_o, cond = ref
    e_dist = (np.abs(dist - dist_o).max(axis=2) / np.maximum(1.0, np.abs(dist_o).max(axis=2))).max()
    live = cond <= cc.COND_LIMIT
    worst = 0.0
    for leg in range(2):
        w_o = cf_o[..., 6 * leg:6 * leg + 6]
        d = np.maximum(np.abs(cf[..., 6 * leg:6 * leg + 6] - w_o).max(axis=2), np.abs(cf[..., [12 + leg, 14 + leg]] - cf_o[..., [12 + leg, 14 + leg]]).max(axis=2))
        ratio = d / (EPS * cond[..., leg] ** 2 * np.maximum(1.0, np.abs(cf_o).max(axis=2)))
        worst = max(worst, float(ratio[live[..., leg]].max()))
    print("\n%s: dist %.1e, wrench %.3f of eps cond^2 (cond up to %.1e), %d of %d legs left out" % (label, e_dist, worst, cond[live].max(),
                                                                                                     (~live).sum(), live.size))
    assert (~live).mean() <= 0.05
    assert e_dist <= 1e-13 and worst <= 1.0, (label, e_dist, worst)


def _device(params, rbd, tau, dt, rows=None):
    from hunter_bipedal_control_amd.solver import HunterSolver
    rows = np.arange(rbd.shape[1]) if rows is None else np.asarray(rows)
    s = HunterSolver(params, batch=len(rows), max_nodes=4)
    try:
        s.estimator_reset(abi.make_estimator_config(params))
        out = [s.estimator_contact_force(dt, np.ascontiguousarray(tau[k][rows]), np.ascontiguousarray(rbd[k][rows])) for k in range(rbd.shape[0])]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    finally:
        s.close()


@pytest.mark.parametrize("dt", DTS)
def test_host_emulator_holds_the_bounds(params, oracle, dt):
    import _hostemu
    lib, mdl = C.CDLL(str(_hostemu.build())), abi.make_model(params)
    ref = _reference(params, oracle, dt)
    rbd, tau = ref[0], ref[1]
    gama = np.exp(-params["config"]["kalman"]["contact_force_cutoff_frequency"] * dt)
    beta = (1 - gama) / (gama * dt)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    z, dist, cf = np.zeros((B, 16)), np.zeros((TICKS, B, 16)), np.zeros((TICKS, B, 16))
    for k in range(TICKS):
        for i in range(B):
            lib.emu_contact_force(C.byref(mdl), C.c_double(gama), C.c_double(beta), p(rbd[k, i]), p(tau[k, i]), p(z[i]), p(dist[k, i]), p(cf[k, i]))
    _check(dist, cf, ref, "emulator dt %g" % dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_device_matches_the_oracle_across_blocks(params, oracle, dt):
    ref = _reference(params, oracle, dt)
    dist, cf = _device(params, ref[0], ref[1], dt)
    _check(dist, cf, ref, "device dt %g" % dt)


@pytest.mark.gpu
def test_rows_do_not_depend_on_their_thread_or_block(params):
    """The same 67 states in reversed instance order give the same rows bit for bit; a batch of 33 (one thread in block 1) equals the first 33."""
    rbd, tau = cc.wide_states(params, B, TICKS)
    dist, cf = _device(params, rbd, tau, 0.002)
    dist_r, cf_r = _device(params, rbd, tau, 0.002, rows=np.arange(B)[::-1])
    assert np.array_equal(dist_r[:, ::-1], dist) and np.array_equal(cf_r[:, ::-1], cf)
    dist_33, cf_33 = _device(params, rbd, tau, 0.002, rows=np.arange(33))
    assert np.array_equal(dist_33, dist[:, :33]) and np.array_equal(cf_33, cf[:, :33])


@pytest.mark.gpu
def test_device_stays_finite_at_leg_singularities(params, oracle):
    """The 40 configurations of tests/test_ref_kf.py test_device_contact_force_algorithm_stays_finite_at_leg_singularities as one batch of 40:
    everything finite, agreement with the oracle where the leg rows are well conditioned, as on the host."""
    rbd, tau = cc.singular_leg_cases()
    dist, cf = _device(params, rbd[None], tau[None], 0.002)
    dist, cf = dist[0], cf[0]
    assert np.isfinite(dist).all() and np.isfinite(cf).all()
    n_checked = 0
    for i in range(len(rbd)):
        conds = cc.leg_blocks(oracle, rbd[i])[1]
        do, co = oracle.contact_force(250.0, 0.002, np.zeros((1, 16)), rbd[i], tau[i])
        assert np.abs(dist[i] - do[0]).max() < 1e-8 * max(1.0, np.abs(do).max()), i
        for leg in range(2):
            if conds[leg] < cc.COND_LIMIT:
                assert np.abs(cf[i, 6 * leg:6 * leg + 6] - co[0][6 * leg:6 * leg + 6]).max() < 1e-6 * max(1.0, np.abs(co).max()), (i, leg, conds)
                n_checked += 1
    assert n_checked >= 20
