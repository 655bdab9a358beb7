"""The plant's sensor model on the device (hb_plant_sense, k_plant_sense) and the estimator entries that consume its arrays in place
(hb_estimator_update_resident, hb_estimator_contact_force_resident), up to ResidentLoop(use_estimator=True).

Sizes are small on purpose: B = 65 has one instance past a 64-wide workgroup of k_plant_sense, B = 3 is a partial one.  The numpy twin
(tests/_sensemu.py) is held to oracle.plant.Plant.imu and to the published Philox vectors by tests/test_sensors_host.py.
"""
import numpy as np
import pytest

import _sensemu as se
from hunter_bipedal_control_amd import abi

pytestmark = pytest.mark.gpu

SIGMAS = dict(orientation_noise=0.02, gyro_noise=0.05, accel_noise=0.3, joint_pos_noise=0.01, joint_vel_noise=0.2, joint_torque_noise=1.0)
# the loop tests run the controller on the noisy estimate: sensor-grade noise, not the unit-scale one of the comparisons
LOOP_SIGMAS = dict(orientation_noise=2e-3, gyro_noise=5e-3, accel_noise=5e-2, joint_pos_noise=4e-4, joint_vel_noise=2e-2, joint_torque_noise=0.1)
SEED = 0xC0FFEE1234567


def _solver(params, B):
    from hunter_bipedal_control_amd.solver import HunterSolver
    return HunterSolver(params, batch=B, max_nodes=108)


def _start(params, s, rng):
    """q0 / v0 inside the attitude box around the standing configuration."""
    from hunter_bipedal_control_amd.rollout import standing_configuration
    q0 = standing_configuration(params, s.B, s)
    q0[:, 3] = rng.uniform(-2.5, 2.5, s.B)
    q0[:, 4:6] = rng.uniform(-0.6, 0.6, (s.B, 2))
    v0 = 0.3 * rng.standard_normal((s.B, 16))
    return q0, v0


def _twin_of_state(s, tau, contact, **kw):
    st = s.plant_state()
    return se.twin_sense(st["q"], st["v"], st["vdot"], tau, contact, **kw)


def test_plant_sense_matches_the_numpy_formulas_on_the_device_state(params):
    B = 65
    rng = np.random.default_rng(11)
    gb, ab = rng.uniform(-0.1, 0.1, (B, 3)), rng.uniform(-0.5, 0.5, (B, 3))
    s, s2, s4 = _solver(params, B), _solver(params, B), _solver(params, 4)
    try:
        q0, v0 = _start(params, s, rng)
        for c in (s, s2):
            c.plant_reset(q0, v0)
        s4.plant_reset(q0[2:6], v0[2:6])
        # ---- before the first step: accel = R' g e_z, torque 0, contact all 1 (vdot, torque count as zero)
        got = s.plant_sense(want_outputs=True)
        st = s.plant_state()
        assert np.array_equal(st["q"], q0) and np.array_equal(st["vdot"], np.zeros((B, 16))) and np.array_equal(st["lam"], np.zeros((B, 12)))
        want = se.twin_sense(q0, v0, np.zeros((B, 16)), np.zeros((B, 10)), np.ones((B, 4), dtype=np.int32))
        se.assert_close_sensors(got, want, quat_tol=1e-13, vec_tol=1e-12, joint_tol=0.0, vec_relative=True)
        assert np.array_equal(got["joint_torque"], np.zeros((B, 10))) and (got["contact_flag"] == 1).all()
        g_body = np.array([se._rot(q0[i, 3:6]).T @ [0.0, 0.0, se.GRAVITY] for i in range(B)])
        assert np.abs(got["lin_acc_local"] - g_body).max() < 1e-12 * se.GRAVITY
        # ---- four steps with host torques, all four contacts down, then [0, 1, 0, 1]
        cfg = abi.make_sensor_config(seed=SEED, **SIGMAS)
        for c in (s, s2):
            c.plant_set_sensor_model(cfg, gb, ab)
        s4.plant_set_sensor_model(abi.make_sensor_config(seed=SEED, instance_offset=2, **SIGMAS), gb[2:6], ab[2:6])
        count = 0
        for tick in range(4):
            contact = np.tile([1, 1, 1, 1] if tick < 2 else [0, 1, 0, 1], (B, 1)).astype(np.int32)
            tau = 3.0 * rng.standard_normal((B, 10))
            for c in (s, s2):
                c.plant_step(tau, contact, 0.002, 4)
            s4.plant_step(tau[2:6], contact[2:6], 0.002, 4)
            # noisy reading: against the twin on the device's own state (plant integration error does not enter)
            got = s.plant_sense(want_outputs=True)
            want = _twin_of_state(s, tau, contact, sigmas=SIGMAS, seed=SEED, gyro_bias=gb, accel_bias=ab, count=count)
            se.assert_close_sensors(got, want, quat_tol=1e-12, vec_tol=1e-12, joint_tol=1e-12, vec_relative=False)
            assert np.abs(got["joint_torque"] - tau).max() > 0.5
            # two contexts with the same seed: identical bits; instance_offset: the slice of the larger batch, bit for bit
            twin_ctx, part = s2.plant_sense(want_outputs=True), s4.plant_sense(want_outputs=True)
            for k in se.OUT_KEYS:
                assert np.array_equal(got[k], twin_ctx[k]), k
                assert np.array_equal(got[k][2:6], part[k]), k
            count += 1
        # ---- the next reading of the same state differs: sense_count advanced
        again = s.plant_sense(want_outputs=True)
        want = _twin_of_state(s, tau, contact, sigmas=SIGMAS, seed=SEED, gyro_bias=gb, accel_bias=ab, count=count)
        se.assert_close_sensors(again, want, quat_tol=1e-12, vec_tol=1e-12, joint_tol=1e-12, vec_relative=False)
        for k in se.OUT_KEYS[:6]:
            assert not np.array_equal(again[k], got[k]), k
        assert np.array_equal(again["contact_flag"], contact)
        # ---- only the torque channel noisy: everything else is the ideal reading bit for bit
        s.plant_set_sensor_model(None)
        ideal = s.plant_sense(want_outputs=True)
        se.assert_close_sensors(ideal, _twin_of_state(s, tau, contact), quat_tol=1e-13, vec_tol=1e-12, joint_tol=0.0, vec_relative=True)
        s.plant_set_sensor_model(abi.make_sensor_config(seed=SEED, joint_torque_noise=1.0))
        one = s.plant_sense(want_outputs=True)
        for k in se.OUT_KEYS:
            assert np.array_equal(one[k], ideal[k]) == (k != "joint_torque"), k
        # setting the model restarted the count: the torque noise is that of count 0
        want = _twin_of_state(s, tau, contact, sigmas=dict(joint_torque_noise=1.0), seed=SEED, count=0)
        assert np.abs(one["joint_torque"] - want["joint_torque"]).max() <= 1e-12
    finally:
        for c in (s, s2, s4):
            c.close()


def _contact_trot(tick):
    return [1, 1, 1, 1] if tick < 3 else [0, 1, 0, 1]


def test_resident_estimator_equals_the_host_fed_one_bit_for_bit(params):
    B = 3
    rng = np.random.default_rng(5)
    a, b = _solver(params, B), _solver(params, B)
    try:
        q0, v0 = _start(params, a, rng)
        q0[:, 3:6] *= 0.1
        xh0 = np.zeros((B, 18))
        xh0[:, 0:3] = q0[:, 0:3]
        a.plant_reset(q0, 0.1 * v0)
        a.plant_set_sensor_model(abi.make_sensor_config(seed=SEED, **LOOP_SIGMAS))
        for c in (a, b):
            c.estimator_reset(abi.make_estimator_config(params), xh0)
        for tick in range(6):
            contact = np.tile(_contact_trot(tick), (B, 1)).astype(np.int32)
            a.plant_step(3.0 * rng.standard_normal((B, 10)), contact, 0.002, 4)
            sens = a.plant_sense(want_outputs=True)
            rbd_a, x_a = a.estimator_update_resident(0.002, want_outputs=True)
            rbd_b, x_b = b.estimator_update(0.002, sens["quat"], sens["ang_vel_local"], sens["lin_acc_local"], sens["joint_pos"],
                                            sens["joint_vel"], sens["contact_flag"])
            assert np.array_equal(rbd_a, rbd_b) and np.array_equal(x_a, x_b), tick
            (xh_a, P_a), (xh_b, P_b) = a.estimator_filter(), b.estimator_filter()
            assert np.array_equal(xh_a, xh_b) and np.array_equal(P_a, P_b), tick
            dist_a, cf_a = a.estimator_contact_force_resident(0.002)
            dist_b, cf_b = b.estimator_contact_force(0.002, sens["joint_torque"])
            assert np.array_equal(dist_a, dist_b) and np.array_equal(cf_a, cf_b), tick
            assert np.isfinite(rbd_a).all() and np.isfinite(cf_a).all() and np.abs(dist_a).max() > 0.0
    finally:
        a.close()
        b.close()


class _HostFedLoop:
    """ResidentLoop(use_estimator=True) written out on the existing entries plus plant_sense: the sensor arrays come to the host and go
    back in through hb_estimator_update."""

    def __init__(self, s, params, gaits, cmd, sensor_config):
        from hunter_bipedal_control_amd import gait
        from hunter_bipedal_control_amd.rollout import standing_configuration
        self.s, self.B, self.cmd = s, s.B, np.ascontiguousarray(cmd, dtype=float)
        self.horizon, self.dt, self.t, self.tick, self.started = 100 * params["config"]["dt"], 0.002, 0.0, 0, False
        self.gains = abi.make_joint_gains()
        s.refgen_reset(abi.make_refgen_config(params, joint_ik=True))
        self.schedules = [gait.gait_schedule(params, g, 0.3, 1.0e3 if g == "stance" else 60.0) for g in gaits]
        q0 = standing_configuration(params, self.B, s)
        s.plant_reset(q0)
        rbd = np.zeros((self.B, 32))
        rbd[:, 0:3], rbd[:, 3:6], rbd[:, 6:16] = q0[:, 3:6], q0[:, 0:3], q0[:, 6:]
        s.set_resident_inputs(s.centroidal_state_from_rbd(rbd), np.zeros(self.B), rbd)
        x = np.zeros((self.B, 22))
        x[:, 6:9], x[:, 9:12], x[:, 12:] = q0[:, 0:3], q0[:, 3:6], q0[:, 6:]
        xh0 = np.zeros((self.B, 18))
        xh0[:, 0:3] = q0[:, 0:3]
        xh0[:, 6:18] = np.asarray(s.eval_foot_kinematics(x, np.zeros((self.B, 22)))[0]).reshape(self.B, 12)
        s.estimator_reset(abi.make_estimator_config(params), xh0)
        s.plant_set_sensor_model(sensor_config)

    def step(self, want_outputs=True):
        from hunter_bipedal_control_amd.rollout import schedule_window
        s = self.s
        z = s.plant_sense(want_outputs=True)
        s.estimator_update(self.dt, z["quat"], z["ang_vel_local"], z["lin_acc_local"], z["joint_pos"], z["joint_vel"], z["contact_flag"],
                           to_resident=True)
        s.set_resident_time(np.full(self.B, self.t))
        if self.tick % 8 == 0:
            s.refgen_set_schedule([schedule_window(ms, self.t - 1.0, self.t + self.horizon + 1.5) for ms in self.schedules])
            assert s.refgen_update(np.full(self.B, self.t), self.horizon, None, self.cmd).max() == 0
            if not self.started:
                s.reset_resident()
                self.started = True
            s.mpc_solve(None)
            s.publish()
        self.last = dict(out=s.wbc_update(None, None, dt=self.dt), cmd=s.joint_command(self.gains, self.dt))
        s.plant_step(None, None, self.dt, 4, to_resident=False)
        self.t += self.dt
        self.tick += 1


class _ParentLoop(_HostFedLoop):
    """ResidentLoop() with default arguments as the parent commit ran it: none of the new entries."""

    def __init__(self, s, params, gaits, cmd):
        from hunter_bipedal_control_amd import gait
        from hunter_bipedal_control_amd.rollout import standing_configuration
        self.s, self.B, self.cmd = s, s.B, np.ascontiguousarray(cmd, dtype=float)
        self.horizon, self.dt, self.t, self.tick, self.started = 100 * params["config"]["dt"], 0.002, 0.0, 0, False
        self.gains = abi.make_joint_gains()
        s.refgen_reset(abi.make_refgen_config(params, joint_ik=True))
        self.schedules = [gait.gait_schedule(params, g, 0.3, 1.0e3 if g == "stance" else 60.0) for g in gaits]
        q0 = standing_configuration(params, self.B, s)
        s.plant_reset(q0)
        rbd = np.zeros((self.B, 32))
        rbd[:, 0:3], rbd[:, 3:6], rbd[:, 6:16] = q0[:, 3:6], q0[:, 0:3], q0[:, 6:]
        s.set_resident_inputs(s.centroidal_state_from_rbd(rbd), np.zeros(self.B), rbd)

    def step(self, want_outputs=True):
        from hunter_bipedal_control_amd.rollout import schedule_window
        s = self.s
        if self.tick % 8 == 0:
            s.refgen_set_schedule([schedule_window(ms, self.t - 1.0, self.t + self.horizon + 1.5) for ms in self.schedules])
            assert s.refgen_update(np.full(self.B, self.t), self.horizon, None, self.cmd).max() == 0
            if not self.started:
                s.reset_resident()
                self.started = True
            s.mpc_solve(None)
            s.publish()
        self.last = dict(out=s.wbc_update(None, None, dt=self.dt), cmd=s.joint_command(self.gains, self.dt))
        s.plant_step(None, None, self.dt, 4, to_resident=True)
        self.t += self.dt
        self.tick += 1


GAITS = ["trot", "trot", "stance"]
CMDS = np.array([[0.2, 0.0, 0.0, 0.0], [0.15, 0.0, 0.0, 0.3], [0.0, 0.0, 0.0, 0.0]])   # trot, trot with a turn, stance


def _run_pair(params, make_a, make_b, ticks=40):
    """Two loops on two contexts side by side: plant q, v and the joint torques equal with == at every tick."""
    a, b = _solver(params, 3), _solver(params, 3)
    try:
        la, lb = make_a(a), make_b(b)
        for tick in range(ticks):
            la.step(want_outputs=True)      # (the WBC result and the joint command of the tick come to the host; the loop is the same)
            lb.step(want_outputs=True)
            sa, sb = a.plant_state(), b.plant_state()
            assert np.array_equal(sa["q"], sb["q"]) and np.array_equal(sa["v"], sb["v"]), tick
            ta, tb = la.last["cmd"]["torque"], lb.last["cmd"]["torque"]
            assert np.array_equal(ta, tb) and np.isfinite(ta).all(), tick
            assert la.last["out"]["status"].max() == 0 and lb.last["out"]["status"].max() == 0, tick
        assert np.isfinite(sa["q"]).all() and (np.abs(sa["q"][:, 2] - 0.63) < 0.04).all()
        return sa
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("noisy", [False, True], ids=["ideal", "noisy"])
def test_resident_loop_with_the_estimator_equals_the_host_fed_loop_bit_for_bit(params, noisy):
    from hunter_bipedal_control_amd.rollout import ResidentLoop
    cfg = (lambda: abi.make_sensor_config(seed=SEED, **LOOP_SIGMAS)) if noisy else (lambda: None)
    _run_pair(params, lambda s: ResidentLoop(s, params, GAITS, CMDS, use_estimator=True, sensor_config=cfg()),
              lambda s: _HostFedLoop(s, params, GAITS, CMDS, cfg()))


def test_resident_loop_defaults_equal_the_loop_without_the_new_entries(params):
    from hunter_bipedal_control_amd.rollout import ResidentLoop
    _run_pair(params, lambda s: ResidentLoop(s, params, GAITS, CMDS), lambda s: _ParentLoop(s, params, GAITS, CMDS))


def test_resident_loop_with_the_estimator_trots_and_the_filter_tracks(params):
    """Trot at 0.2 m/s and stance, 250 ticks (0.5 s: 0.3 s of stance, then the first steps), ideal sensors, with the bounds
    test_device_closed_loop_with_the_state_estimator_in_the_loop asserts for the host-plant loop: upright, the filter within 0.03 m /
    0.15 m/s of the plant after tick 100, every WBC status 0; the x bound of that test with this test's 0.2 s of gait."""
    from hunter_bipedal_control_amd.rollout import ResidentLoop
    s = _solver(params, 2)
    try:
        loop = ResidentLoop(s, params, ["trot", "stance"], np.array([[0.2, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]]), use_estimator=True)
        err_p, err_v = 0.0, 0.0
        for k in range(250):
            loop.step(want_outputs=True)
            assert loop.last["out"]["status"].max() == 0, k
            if k > 100:
                st = s.plant_state()
                xh, _ = s.estimator_filter()
                err_p = max(err_p, np.abs(xh[:, 0:3] - st["q"][:, 0:3]).max())
                err_v = max(err_v, np.abs(xh[:, 3:6] - st["v"][:, 0:3]).max())
        q = s.plant_state()["q"]
    finally:
        s.close()
    print(f"filter error: position {err_p:.4f} m, velocity {err_v:.4f} m/s; final x {q[:, 0]}")
    assert np.isfinite(q).all() and (np.abs(q[:, 2] - 0.63) < 0.04).all() and np.abs(q[:, 4:6]).max() < 0.15
    assert abs(q[0, 0] - 0.2 * 0.2) < 0.1 and abs(q[1, 0]) < 0.05
    assert err_p < 0.03 and err_v < 0.15, (err_p, err_v)


def test_failure_surface_of_the_sensor_entries(params):
    from hunter_bipedal_control_amd.rollout import standing_configuration
    s = _solver(params, 3)
    lib, ctx = s.lib, s.ctx
    import ctypes as C

    def refused(rc, code):
        assert rc == code, (rc, code)
        assert len(lib.hb_last_error(ctx)) > 0

    try:
        q0 = standing_configuration(params, 3, s)
        ok = abi.make_sensor_config(seed=1, gyro_noise=0.1)
        # before hb_plant_reset
        refused(lib.hb_plant_set_sensor_model(ctx, C.byref(ok), None, None), abi.HB_ERR_STATE)
        refused(lib.hb_plant_sense(ctx, *[None] * 7), abi.HB_ERR_STATE)
        refused(lib.hb_estimator_update_resident(ctx, C.c_double(0.002), C.c_int32(0), None, None), abi.HB_ERR_STATE)
        refused(lib.hb_estimator_contact_force_resident(ctx, C.c_double(0.002), None, None), abi.HB_ERR_STATE)
        s.plant_reset(q0)
        # before hb_estimator_reset
        s.plant_sense()
        refused(lib.hb_estimator_update_resident(ctx, C.c_double(0.002), C.c_int32(0), None, None), abi.HB_ERR_STATE)
        refused(lib.hb_estimator_contact_force_resident(ctx, C.c_double(0.002), None, None), abi.HB_ERR_STATE)
        s.estimator_reset(abi.make_estimator_config(params))
        # before any hb_plant_sense of this plant
        s.plant_reset(q0)
        refused(lib.hb_estimator_update_resident(ctx, C.c_double(0.002), C.c_int32(0), None, None), abi.HB_ERR_STATE)
        refused(lib.hb_estimator_contact_force_resident(ctx, C.c_double(0.002), None, None), abi.HB_ERR_STATE)
        # bad sensor models
        for k in se.CHANNELS:
            for bad in (-0.1, float("nan"), float("inf")):
                refused(lib.hb_plant_set_sensor_model(ctx, C.byref(abi.make_sensor_config(**{k: bad})), None, None), abi.HB_ERR_ARG)
        r = abi.make_sensor_config()
        r.reserved = 7
        refused(lib.hb_plant_set_sensor_model(ctx, C.byref(r), None, None), abi.HB_ERR_ARG)
        refused(lib.hb_estimator_update_resident(ctx, C.c_double(-1.0), C.c_int32(0), None, None), abi.HB_ERR_ARG)
        # after the refused calls the context still steps, with ideal sensors (no refused model was taken)
        s.plant_step(np.zeros((3, 10)), np.ones((3, 4), dtype=np.int32), 0.002, 4)
        z = s.plant_sense(want_outputs=True)
        st = s.plant_state()
        assert np.array_equal(z["joint_pos"], st["q"][:, 6:]) and np.array_equal(z["joint_vel"], st["v"][:, 6:])
        rbd, x = s.estimator_update_resident(0.002, want_outputs=True)
        dist, cf = s.estimator_contact_force_resident(0.002)
        assert np.isfinite(rbd).all() and np.isfinite(x).all() and np.isfinite(dist).all() and np.isfinite(cf).all()
        assert np.abs(rbd[:, 6:16] - st["q"][:, 6:]).max() == 0.0
    finally:
        s.close()
