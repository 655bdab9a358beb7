"""The hybrid step on the device (hb_plant_step_hybrid: k_plant_hybrid, k_plant_contact_hybrid, k_plant_joints_hybrid) against the
composition identity of tests/_actemu.py, with the device's own held-torque step as the reference: a hybrid step of S substeps equals S
hb_plant_step calls of ONE substep of length dt / S, each with the law's torque computed in numpy from hb_plant_get_state.  All three plant
forms, passes of B = 4 instances, 10 ticks x 4 substeps; the same cases, commands and tolerances as tests/test_actuator_plant_host.py, and
the host build of that test as a second reference.  Then the device-resident command, ResidentLoop(actuator=...) and the error surface."""
import ctypes as C

import numpy as np
import pytest

import _actemu as ae
import _contactemu as ce
import _jointemu as je
from hunter_bipedal_control_amd import abi

pytestmark = pytest.mark.gpu

B = 4
PASSES = ("stub", "c", "r", "l")
KIND = dict(stub="stub", c="contact", r="joints", l="joints")
CHECK = dict(stub=ae.check_stub, contact=ae.check_contact, joints=ae.check_joints)
TOL_V = dict(stub=ae.STUB_TOL_V, contact=ce.TOL_V, joints=je.TOL_V)


def _solver(params, batch=B):
    from hunter_bipedal_control_amd.solver import HunterSolver
    return HunterSolver(params, batch=batch, max_nodes=108)


def _device_fns(s):
    def foot_fn(q):
        q = np.atleast_2d(q)
        x = np.zeros((q.shape[0], 22))
        x[:, 6:9], x[:, 9:12], x[:, 12:] = q[:, 0:3], q[:, 3:6], q[:, 6:]
        return s.eval_foot_kinematics(x, np.zeros((q.shape[0], 22)))[0]

    def qv_fn(q, v):
        pl = ce.GroundPlant(None, foot_fn, q[None], v[None])
        return tuple(a[0] for a in s.eval_rbd(pl.rbd()))

    return foot_fn, qv_fn


class DevicePlant:
    """The device's plant with the interface ae.compose drives a twin through: q, v from hb_plant_get_state, step = hb_plant_step."""

    def __init__(self, s, kind):
        self.s, self.kind = s, kind

    @property
    def q(self):
        return self.s.plant_state()["q"]

    @property
    def v(self):
        return self.s.plant_state()["v"]

    def step(self, tau, contact, dt, substeps):
        self.s.plant_step(tau, contact, dt, substeps)

    def outputs(self, sense=False):
        """Everything the getters return, with the keys of the emu_* records ([B][...])."""
        s, st = self.s, self.s.plant_state()
        o = dict(q=st["q"], v=st["v"], lam=st["lam"], vdot=st["vdot"])
        if self.kind != "stub":
            con = s.plant_contact()
            o.update(gap=con["gap"], point_vel=con["point_vel"].reshape(-1, 12), residual=con["residual"], touching=con["touching"], status=con["status"])
        if self.kind == "joints":
            jo = s.plant_get_joints()
            o.update(tau_applied=jo["tau_applied"], friction_torque=jo["friction_torque"], limit_torque=jo["limit_torque"],
                     jresidual=jo["residual"], jstatus=jo["status"])
        if sense:
            act = s.plant_get_actuator()
            o.update(tau_first=act["tau_first"], tau_mean=act["tau_mean"], tau_last=s.plant_sense(want_outputs=True)["joint_torque"])
        return o


def _row(o, i):
    r = {k: x[i] for k, x in o.items()}
    for k in ("residual", "jresidual"):
        if k in r:
            r[k] = float(r[k])
    for k in ("status", "jstatus"):
        if k in r:
            r[k] = int(r[k])
    return r


def _cases(name, params, q_stand, qv_fn, foot_fn):
    """-> (cases[B], rngs[B], flags[B][4], contact config or None, joint model or None)."""
    if name == "stub":
        names = ("stance", "left", "stance", "left")
        rngs = [np.random.default_rng(ae.SEEDS[n] + (i // 2)) for i, n in enumerate(names)]
        cases = [ae.stub_case(n, q_stand, qv_fn, r) for n, r in zip(names, rngs)]
        return cases, rngs, np.array([c["contact"] for c in cases], dtype=np.int32), None, None
    rngs = [np.random.default_rng(ae.SEEDS[name] + i) for i in range(B)]
    flags = np.ones((B, 4), dtype=np.int32)
    if name == "c":
        cases = [ce.make_case("c", q_stand, qv_fn, r) for r in rngs]
        return cases, rngs, flags, abi.make_contact_config(params, mu=cases[0]["mu"], ground_z=0.0, erp=ce.ERP, sweeps=ce.SWEEPS), None
    cases = [je.make_case(name, params, q_stand, qv_fn, foot_fn, r) for r in rngs]
    return cases, rngs, flags, je.contact_cfg(params, cases[0]), cases[0]["jm"]


def _reset(s, cases, cfg, jm):
    s.plant_reset(np.array([c["q0"] for c in cases]), np.array([c["v0"] for c in cases]), baumgarte=ae.BAUM, eps=ae.EPS)
    s.plant_set_contact_model(cfg)
    if cfg is not None:
        s.plant_set_external_wrench(None)
        s.plant_set_joint_model(jm)


@pytest.fixture(scope="module")
def passes(params):
    """Every pass once: the hybrid run, then from a second hb_plant_reset of the same context the composed run with the commands of the
    first, then the held-torque tick 0 -> {name: dict(kind, cases, flags, cfg, jm, rec[tick] = dict(cmds, start, dev, comp, ref), held)}.
    Shared by the tests below and left unchanged."""
    from hunter_bipedal_control_amd.rollout import standing_configuration
    s = _solver(params)
    out = {}
    try:
        foot_fn, qv_fn = _device_fns(s)
        q_stand = standing_configuration(params, 1, s)[0]
        for name in PASSES:
            kind = KIND[name]
            cases, rngs, flags, cfg, jm = _cases(name, params, q_stand, qv_fn, foot_fn)
            limit = je.model_dict(jm)["torque_limit"] if jm is not None else None
            dp = DevicePlant(s, kind)
            _reset(s, cases, cfg, jm)
            act = s.plant_get_actuator()
            assert not act["tau_first"].any() and not act["tau_mean"].any() and not act["last_timestamp"].any()
            rec = []
            for tick in range(ae.TICKS):
                start = dp.outputs()
                cmds = [ae.make_command(c["tau_fn"](tick), start["q"][i], rngs[i], ae.stance_of(flags[i])) for i, c in enumerate(cases)]
                s.plant_step_hybrid(ae.stack(cmds), flags, ae.DT, ae.SUBSTEPS)
                rec.append(dict(cmds=cmds, start=start, dev=dp.outputs(sense=True)))
            _reset(s, cases, cfg, jm)
            assert not s.plant_get_actuator()["tau_first"].any(), "hb_plant_reset clears the record of the last hybrid step"
            for r in rec:
                r["ref"] = ae.compose(dp, ae.stack(r["cmds"]), flags, ae.DT, ae.SUBSTEPS, limit)
                r["comp"] = dp.outputs()
            assert not s.plant_get_actuator()["tau_first"].any(), "hb_plant_step leaves the record of the last hybrid step alone"
            _reset(s, cases, cfg, jm)
            bc = ae.stack(rec[0]["cmds"])
            s.plant_step(ae.law(bc, rec[0]["start"]["q"], rec[0]["start"]["v"]), flags, ae.DT, ae.SUBSTEPS)
            anchors = np.asarray(foot_fn(np.array([c["q0"] for c in cases]))).reshape(B, 12)   # (the stub pins a foot where it is at q0)
            out[name] = dict(kind=kind, cases=cases, flags=flags, cfg=cfg, jm=jm, rec=rec, held=dp.outputs(), anchors=anchors)
    finally:
        s.close()
    return out


@pytest.mark.parametrize("name", PASSES)
def test_hybrid_step_equals_the_composition_of_held_torque_steps(passes, name):
    """After every tick, every instance: the outputs of the hybrid run against those of the composed run at the tolerances of
    tests/_actemu.py; the joint status word with the saturation bits ORed over the composed steps."""
    p, worst = passes[name], {}
    for tick, r in enumerate(p["rec"]):
        tw = ae.Snapshot(r["comp"])
        for i in range(B):
            for k, e in CHECK[p["kind"]](_row(r["dev"], i), tw, r["ref"], i, r["cmds"][i], (name, tick, i)).items():
                worst[k] = max(worst.get(k, 0.0), e)
    print(name, {k: f"{e:.2e}" for k, e in worst.items()})


@pytest.mark.parametrize("name", PASSES)
def test_the_device_cases_can_fail(passes, name):
    """Tick 0: the device's own held-torque tick with tau_0 over the 4 substeps differs from the composed run in v by at least 100 x the
    tolerance used for v, on every instance."""
    p = passes[name]
    gap = ae.assert_can_fail(ae.Snapshot(p["held"]), ae.Snapshot(p["rec"][0]["comp"]), TOL_V[p["kind"]], name)
    print(name, "held against composed, |dv| per instance:", gap)


@pytest.mark.parametrize("name", PASSES)
def test_device_equals_the_host_build(passes, params, name):
    """Every tick, every instance: the host build of tests/test_actuator_plant_host.py from the device's state at the start of the tick
    (impulses = forces x h; the stub's anchors = the pinned feet at q0) against the device's outputs, same tolerances."""
    p, kind = passes[name], passes[name]["kind"]
    lib, mdl, h = C.CDLL(str(ae.build())), abi.make_model(params), ae.DT / ae.SUBSTEPS
    anchors = p["anchors"]
    for tick, r in enumerate(p["rec"]):
        st = r["start"]
        for i in range(B):
            if kind == "stub":
                pinned = p["flags"][i] if tick else np.zeros(4, dtype=np.int32)
                o = ae.emu_stub(lib, mdl, st["q"][i], st["v"][i], anchors[i], pinned, r["cmds"][i], p["flags"][i])
            elif kind == "contact":
                o = ae.emu_contact(lib, mdl, p["cfg"], st["q"][i], st["v"][i], st["lam"][i] * h, r["cmds"][i], None, int(st["status"][i]))
            else:
                jimp = np.concatenate([st["friction_torque"][i], st["limit_torque"][i]]) * h
                o = ae.emu_joints(lib, mdl, p["cfg"], p["jm"], st["q"][i], st["v"][i], st["lam"][i] * h, jimp, r["cmds"][i], None, int(st["status"][i]))
            tw, ref = ae.batched(o)
            CHECK[kind](_row(r["dev"], i), tw, ref, 0, r["cmds"][i], (name, tick, i, "host build"))


def test_sticky_saturation_bit_on_the_device(params):
    """ae.sticky_case on the device: the knee is saturated in the substeps 0 - 2 and not in the last; bit 13 is set, tau_applied is the last
    substep's (inside the limit) and is what hb_plant_sense reports, tau_first is the law before saturation."""
    from hunter_bipedal_control_amd.rollout import standing_configuration
    s = _solver(params, 2)
    try:
        foot_fn, qv_fn = _device_fns(s)
        case, cmd = ae.sticky_case(params, standing_configuration(params, 1, s)[0], qv_fn, foot_fn)
        cases, flags = [case, case], np.ones((2, 4), dtype=np.int32)
        cfg, limit, j = je.contact_cfg(params, case), je.model_dict(case["jm"])["torque_limit"], je.KNEE
        dp = DevicePlant(s, "joints")
        _reset(s, cases, cfg, case["jm"])
        s.plant_step_hybrid(ae.stack([cmd, cmd]), flags, ae.DT, ae.SUBSTEPS)
        dev = dp.outputs(sense=True)
        _reset(s, cases, cfg, case["jm"])
        ref = ae.compose(dp, ae.stack([cmd, cmd]), flags, ae.DT, ae.SUBSTEPS, limit)
        ss = ref["sat_steps"][:, 0, j]
        assert ss[:-1].any() and not ss[-1], ("the case does not have the property on the device", ss)
        tw = ae.Snapshot(dp.outputs())
        for i in range(2):
            d = _row(dev, i)
            ae.check_joints(d, tw, ref, i, cmd, ("sticky", i))
            assert d["jstatus"] & (1 << (10 + j)) and abs(d["tau_applied"][j]) < 2.0 and abs(d["tau_first"][j]) > 2.0
            assert np.array_equal(d["tau_applied"], d["tau_last"])
    finally:
        s.close()


@pytest.fixture(scope="module")
def standing(params):
    """B = 2 standing on the pinned stub, one tick of the resident loop, then a real hb_wbc_update + hb_joint_command on the state the
    plant published -> (solver, command dict, q, v); the solver is closed by the fixture."""
    from hunter_bipedal_control_amd.rollout import ResidentLoop
    s = _solver(params, 2)
    try:
        loop = ResidentLoop(s, params, ["stance", "stance"], np.zeros((2, 4)))
        loop.step()
        s.wbc_update_resident(loop.dt)
        cmd = s.joint_command(loop.gains, loop.dt)
        st = s.plant_state()
        yield s, cmd, st["q"].copy(), st["v"].copy()
    finally:
        s.close()


def test_resident_command_equals_the_command_given_as_arrays(standing):
    """hb_plant_step_hybrid with all-NULL arrays = hb_plant_step_hybrid on the five arrays hb_joint_command returned, bit for bit (each from
    a hb_plant_reset at the same state); tau_first = the torque output of hb_joint_command within 4 ulp of |ff| + |kp (pos - q)| +
    |kd (vel - qd)| (the plant state is the state the command was computed from; the two kernels may contract the expression differently)."""
    s, cmd, q, v = standing
    runs = []
    for command in (None, cmd):
        s.plant_reset(q, v)
        s.plant_step_hybrid(command, None, 0.002, 4)
        st, act = s.plant_state(), s.plant_get_actuator()
        runs.append((st["q"], st["v"], st["lam"], st["vdot"], act["tau_first"], act["tau_mean"], s.plant_sense(want_outputs=True)["joint_torque"]))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    size = np.abs(cmd["tau_ff"]) + np.abs(cmd["kp"] * (cmd["pos_des"] - q[:, 6:])) + np.abs(cmd["kd"] * (cmd["vel_des"] - v[:, 6:]))
    err = np.abs(runs[0][4] - cmd["torque"])
    print("tau_first against the joint command's torque, in ulp of the sum of magnitudes:", (err / np.spacing(size)).max())
    assert (err <= 4.0 * np.spacing(size)).all()


def test_error_surface(params, standing):
    from hunter_bipedal_control_amd.solver import HunterHipError
    s, cmd, q, v = standing
    fresh = _solver(params, 2)
    try:
        for call in (lambda: fresh.plant_step_hybrid(cmd, np.ones((2, 4), dtype=np.int32)), lambda: fresh.plant_get_actuator(),
                     lambda: fresh.plant_sense_lcm(1), lambda: fresh.plant_step_lcm(np.zeros((2, 496), dtype=np.uint8), np.ones((2, 4), dtype=np.int32))):
            with pytest.raises(HunterHipError, match=r"\(-3\).*hb_plant_reset"):      # HB_ERR_STATE before hb_plant_reset
                call()
        fresh.plant_reset(q, v)
        with pytest.raises(HunterHipError, match=r"hb_plant_step_hybrid failed \(-3\).*hb_joint_command"):   # no resident command yet
            fresh.plant_step_hybrid(None, np.ones((2, 4), dtype=np.int32))
    finally:
        fresh.close()
    before = s.plant_state()
    with pytest.raises(HunterHipError, match=r"hb_plant_step_hybrid failed \(-1\).*all five"):
        s.plant_step_hybrid({k: x for k, x in cmd.items() if k != "kd"}, None)
    with pytest.raises(HunterHipError, match=r"hb_plant_step_hybrid failed \(-1\)"):
        s.plant_step_hybrid(cmd, None, substeps=0)
    with pytest.raises(HunterHipError, match=r"hb_plant_sense_lcm failed \(-1\)"):
        s.plant_sense_lcm(1, low_state=False, full_state=False)
    after = s.plant_state()
    assert np.array_equal(before["q"], after["q"]) and np.array_equal(before["v"], after["v"])


def test_resident_loop_substep_actuator_stands_and_held_is_todays_loop(params):
    """ResidentLoop(contact_config={fall_height 0.3}, joint_model={}, actuator="substep"), 2 robots standing, 100 ticks; on every tick: no
    non-finite or fallen bit, WBC status 0, gaps >= -1e-3 m, no stop bit and no saturation bit.  actuator="held" is the loop built
    without the argument, bit for bit (25 ticks)."""
    from hunter_bipedal_control_amd.rollout import ResidentLoop
    with pytest.raises(ValueError, match="actuator"):
        ResidentLoop(None, params, ["stance"] * 2, np.zeros((2, 4)), actuator="per-substep")
    s = _solver(params, 2)
    try:
        loop = ResidentLoop(s, params, ["stance", "stance"], np.zeros((2, 4)), contact_config=dict(fall_height=0.3), joint_model={}, actuator="substep")
        for k in range(100):
            loop.step(want_outputs=True)
            jo, con = s.plant_get_joints(), s.plant_contact()
            assert (con["status"] & (ce.NONFINITE | ce.FALLEN) == 0).all(), (k, con["status"])
            assert (loop.last["out"]["status"] == 0).all(), (k, loop.last["out"]["status"])
            assert (con["gap"] >= -1e-3).all(), (k, con["gap"])
            assert (jo["status"] & 0xFFFFF == 0).all(), (k, jo["status"])
        st, act = s.plant_state(), s.plant_get_actuator()
        print("standing with the actuator loop per substep, tick 100: base height", st["q"][:, 2], "tilt", np.abs(st["q"][:, 4:6]).max(axis=1),
              "largest |tau_mean - tau_first|", np.abs(act["tau_mean"] - act["tau_first"]).max())
    finally:
        s.close()
    ends = []
    for kw in (dict(), dict(actuator="held")):
        s = _solver(params, 2)
        try:
            loop = ResidentLoop(s, params, ["stance", "stance"], np.zeros((2, 4)), contact_config={}, joint_model={}, **kw)
            for k in range(25):
                loop.step()
            st = s.plant_state()
            ends.append((st["q"], st["v"], st["lam"], s.plant_get_joints()["tau_applied"]))
        finally:
            s.close()
    for a, b in zip(*ends):
        assert np.array_equal(a, b)
