"""Per-instance terrain of the ground-contact plant on the device (hb_plant_set_terrain; k_plant_terrain, k_plant_terrain_joints and their
hybrid forms) against the numpy twin of the definition (tests/_terrainemu.py) with the device's own rigid-body terms, up to
ResidentLoop(terrain=...).  B = 5: one scenario of te.scenarios per instance, so one batch holds a level floor, two slopes, four different
friction coefficients under one robot, a slider and a landing."""
import numpy as np
import pytest

import _contactemu as ce
import _jointemu as je
import _terrainemu as te
from hunter_bipedal_control_amd import abi

pytestmark = pytest.mark.gpu

B = te.B
NTICKS = max(te.TICKS)


def _solver(params, batch=B):
    from hunter_bipedal_control_amd.solver import HunterSolver
    return HunterSolver(params, batch=batch, max_nodes=108)


def _device_fns(s):
    def foot_fn(q):
        q = np.atleast_2d(q)
        x = np.zeros((q.shape[0], 22))
        x[:, 6:9], x[:, 9:12], x[:, 12:] = q[:, 0:3], q[:, 3:6], q[:, 6:]
        return s.eval_foot_kinematics(x, np.zeros((q.shape[0], 22)))[0]

    def qv_fn(q, v):   # one instance, through the rbd packing of the plant
        pl = ce.GroundPlant(None, foot_fn, q[None], v[None])
        return tuple(a[0] for a in s.eval_rbd(pl.rbd()))

    return foot_fn, qv_fn


def _cfg(params, **kw):
    # (mu and ground_z are NOT those of any scenario: a step on a terrain must not read them)
    return abi.make_contact_config(params, **{**dict(mu=0.31, ground_z=0.123, erp=te.ERP, sweeps=te.SWEEPS), **kw})


def _outputs(s, joints):
    st, con = s.plant_state(), s.plant_contact()
    o = dict(q=st["q"], v=st["v"], lam=st["lam"], vdot=st["vdot"], rbd=st["rbd"], gap=con["gap"], point_vel=con["point_vel"].reshape(-1, 12),
             residual=con["residual"], touching=con["touching"], status=con["status"])
    if joints:
        jo = s.plant_get_joints()
        o.update(tau_applied=jo["tau_applied"], friction_torque=jo["friction_torque"], limit_torque=jo["limit_torque"], jresidual=jo["residual"],
                 jstatus=jo["status"])
    return o


def _row(o, i):
    return {k: (float(a[i]) if k in ("residual", "jresidual") else a[i]) for k, a in o.items()}


def _arrays(scen):
    return (np.array([c["q0"] for c in scen]), np.array([c["v0"] for c in scen]), np.array([c["plane"] for c in scen]),
            np.array([c["mu"] for c in scen]))


def _start(s, params, scen, joints, terrain=True, **cfg):
    q0, v0, plane, mu = _arrays(scen)
    s.plant_reset(q0, v0, eps=te.EPS)
    s.plant_set_contact_model(_cfg(params, **cfg))
    s.plant_set_joint_model(abi.make_joint_model(params) if joints else None)
    if terrain:
        s.plant_set_terrain(plane, mu)
    else:
        s.plant_set_terrain(None, None)


def _command(q, tau):
    return dict(pos_des=q[:, 6:].copy(), vel_des=np.zeros((len(q), 10)), kp=np.full((len(q), 10), 5.0), kd=np.full((len(q), 10), 0.05), tau_ff=tau)


@pytest.fixture(scope="module")
def dev(params):
    """One context, B = 5.  passes[joints][tick] = dict(dev, twin, tau, start): the device on the five terrains and the twin re-seeded with
    the device's (q, v, p) before every tick; momentum[joints]: ticks of one substep from states of the passes; rolled: the batch with the
    scenarios and inputs rolled by one instance.  Shared by the tests below and left unchanged."""
    from hunter_bipedal_control_amd.rollout import standing_configuration
    s = _solver(params)
    out = dict(passes={}, momentum={}, rolled={}, flat={})
    try:
        foot_fn, qv_fn = _device_fns(s)
        q_stand = standing_configuration(params, 1, s)[0]
        scen = te.scenarios(q_stand, qv_fn, foot_fn)
        q0, v0, plane, mu = _arrays(scen)
        flags = np.ones((B, 4), dtype=np.int32)
        jmd = je.model_dict(abi.make_joint_model(params))
        for joints in (False, True):
            _start(s, params, scen, joints)
            tw = te.TerrainPlant(qv_fn, foot_fn, q0, v0, plane, mu, jmd if joints else None)
            rec, o = [], _outputs(s, joints)
            for tick in range(NTICKS):
                tau = np.array([c["tau_fn"](tick) for c in scen])
                tw.q, tw.v, tw.p = o["q"].copy(), o["v"].copy(), te.to_frame(o["lam"] * te.H, plane).reshape(B, 12)
                if joints:
                    tw.jp = np.concatenate([o["friction_torque"], o["limit_torque"]], axis=1) * te.H
                start = o
                tw.step(tau)
                s.plant_step(tau, flags, te.DT, te.SUBSTEPS)
                o = _outputs(s, joints)
                rec.append(dict(dev=o, twin=tw.record(), tau=tau, start=start))
            out["passes"][joints] = rec
            # ticks of ONE substep from three states of the pass, with a base force on the odd ones
            mom = []
            for k, r in enumerate(rec[2:12:3]):
                st = r["start"]
                s.plant_reset(st["q"], st["v"], eps=te.EPS)      # (the terrain survives; the impulses start from zero)
                wrench = np.tile([12.0, -7.0, 3.0, 0.0, 0.0, 0.0], (B, 1)) if k % 2 else None
                s.plant_set_external_wrench(wrench)
                s.plant_step(r["tau"], flags, te.H, 1)
                terms = [qv_fn(st["q"][i], st["v"][i])[:2] for i in range(B)]
                mom.append(dict(dev=_outputs(s, joints), v_in=st["v"], terms=terms, wrench=wrench))
            s.plant_set_external_wrench(None)
            out["momentum"][joints] = mom
            # the scenarios and every input rolled by one instance: instance i + 1 of this run is instance i of the pass
            rolled = [scen[(i - 1) % B] for i in range(B)]
            _start(s, params, rolled, joints)
            rr = []
            for tick in range(12):
                s.plant_step(np.roll(rec[tick]["tau"], 1, axis=0), flags, te.DT, te.SUBSTEPS)
                rr.append(_outputs(s, joints))
            out["rolled"][joints] = rr
            # level terrain with the configuration's own mu and ground_z against no terrain, held and hybrid form
            for hybrid in (False, True):
                runs = []
                for terrain in (False, True):
                    _start(s, params, scen, joints, terrain=False, mu=0.4, ground_z=0.001)
                    if terrain:
                        s.plant_set_terrain(np.tile([0.0, 0.0, 1.0, 0.001], (B, 1)), np.full((B, 4), 0.4))
                    ticks = []
                    for tick in range(8):
                        tau = rec[tick]["tau"]
                        if hybrid:
                            s.plant_step_hybrid(_command(s.plant_state()["q"], tau), flags, te.DT, te.SUBSTEPS)
                        else:
                            s.plant_step(tau, flags, te.DT, te.SUBSTEPS)
                        o2 = _outputs(s, joints)
                        if hybrid:
                            o2.update({k: a for k, a in s.plant_get_actuator().items() if k != "last_timestamp"})
                        ticks.append(o2)
                    runs.append(ticks)
                out["flat"][joints, hybrid] = runs
        out.update(scen=scen, plane=plane, mu=mu)
    finally:
        s.close()
    return out


@pytest.mark.parametrize("joints", [False, True])
def test_device_matches_the_twin_tick_by_tick(dev, joints):
    """q 1e-10; v, lambda and with the joint model friction / limit torque 10 x the twin's measured sensitivity (tests/_terrainemu.py), every
    instance on every tick of its scenario."""
    worst = {}
    for tick, r in enumerate(dev["passes"][joints]):
        for i in range(B):
            if tick < te.TICKS[i]:
                for k, e in te.check_against_twin(_row(r["dev"], i), {k: a[i] for k, a in r["twin"].items()}, joints).items():
                    worst[k] = max(worst.get(k, 0.0), e)
    print("joint model", joints, "worst against the twin:", {k: f"{e:.2e}" for k, e in worst.items()})


@pytest.mark.parametrize("joints", [False, True])
def test_the_properties_hold_on_every_tick(dev, joints):
    """lambda . n >= 0, the cone of the point's own mu, touching == (lambda . n > 0), sliding points on their cone opposing their velocity in
    the plane, no non-finite bit; the slider (instance 3) slides and the level stander (instance 0) does not."""
    sliding = np.zeros(B, dtype=int)
    for r in dev["passes"][joints]:
        for i in range(B):
            o = r["dev"]
            sliding[i] += te.check_properties(o["lam"][i], o["point_vel"][i], o["touching"][i], dev["plane"][i], dev["mu"][i])
        assert (r["dev"]["status"] & ce.NONFINITE == 0).all()
    assert sliding[3] >= 1 and sliding[0] == 0


@pytest.mark.parametrize("joints", [False, True])
def test_base_momentum_rows_pin_lambda_as_world_forces(dev, joints):
    """Ticks of one substep: (M dv / h + nle)[0:3] = sum_c lambda_c + F_ext to 64 roundings with M, nle from eval_rbd at the start state."""
    loaded = 0
    for m in dev["momentum"][joints]:
        for i in range(B):
            M, nle = m["terms"][i]
            te.check_base_momentum(m["dev"]["lam"][i], m["dev"]["v"][i], m["v_in"][i], M, nle, te.H, None if m["wrench"] is None else m["wrench"][i])
            loaded += int(np.abs(m["dev"]["lam"][i]).max() > 1.0)
    assert loaded >= B


@pytest.mark.parametrize("hybrid", [False, True])
@pytest.mark.parametrize("joints", [False, True])
def test_flat_terrain_is_no_terrain(dev, joints, hybrid):
    """plane = (0, 0, 1, ground_z), mu = cfg.mu on every instance: every output == the run without a terrain (other kernels), 8 ticks."""
    without, with_terrain = dev["flat"][joints, hybrid]
    for tick, (a, b) in enumerate(zip(without, with_terrain)):
        for k in a:
            assert np.array_equal(a[k], b[k]), (k, tick)
    assert any(np.abs(a["lam"]).max() > 1.0 for a in without)


@pytest.mark.parametrize("joints", [False, True])
def test_scenarios_rolled_by_one_instance(dev, joints):
    """Instance i of the pass == instance i + 1 of the run with scenarios and inputs rolled by one, on every output of 12 ticks."""
    for tick, rolled in enumerate(dev["rolled"][joints]):
        o = dev["passes"][joints][tick]["dev"]
        for k in o:
            assert np.array_equal(np.roll(o[k], 1, axis=0), rolled[k]), (k, tick)
    o = dev["passes"][joints][11]["dev"]
    assert not np.array_equal(o["lam"][0], o["lam"][1]) and not np.array_equal(o["lam"][1], o["lam"][3])   # (the scenarios do differ)


def test_stick_and_slide_on_the_slope(params):
    """B = 2 on the 0.2 rad slope under the statics torque, 20 ticks: mu = 2 tan (instance 0) sticks, mu = tan / 2 (instance 1) slides; the
    bounds are the CPU twin's figures with a factor 2 (te.STICK_BOUND, te.SLIDE_BOUND, te.FEET_BOUND)."""
    from hunter_bipedal_control_amd.rollout import standing_configuration
    s = _solver(params, 2)
    try:
        foot_fn, qv_fn = _device_fns(s)
        q_stand = standing_configuration(params, 1, s)[0]
        scen = [te.slope_scenario(q_stand, qv_fn, foot_fn, f) for f in (2.0, 0.5)]
        _start(s, params, scen, False)
        recs = [[], []]
        for tick in range(20):
            s.plant_step(np.array([c["tau_fn"](tick) for c in scen]), np.ones((2, 4), dtype=np.int32), te.DT, te.SUBSTEPS)
            o = _outputs(s, False)
            for i in range(2):
                recs[i].append(_row(o, i))
        stick, slide = (te.stick_slide_figures(recs[i], scen[i]["plane"], scen[i]["mu"]) for i in range(2))
        print("stick:", stick, "slide:", slide)
        te.check_stick_slide(stick, slide)
    finally:
        s.close()


def test_api_behaviour(params):
    """Error codes (the terrain in force is kept after a refused call), hb_plant_get_terrain with and without a terrain, the terrain survives
    hb_plant_reset and a second hb_plant_set_contact_model, leaving model 1 clears it, setting one clears the impulses, FALLEN along n."""
    from hunter_bipedal_control_amd.rollout import standing_configuration
    from hunter_bipedal_control_amd.solver import HunterHipError
    s = _solver(params, 3)
    try:
        foot_fn, qv_fn = _device_fns(s)
        flags = np.ones((3, 4), dtype=np.int32)
        n = te.normal_of(0.15, -0.1)
        plane = np.array([[0.0, 0.0, 1.0, 0.0], np.concatenate([te.normal_of(te.SLOPE), [0.0]]), np.concatenate([n, [0.01]])])
        mu = np.array([[0.7] * 4, [0.6, 0.5, 0.4, 0.3], [0.9, 0.5, 0.3, 0.05]])
        for call in (lambda: s.plant_set_terrain(plane, mu), s.plant_get_terrain):
            with pytest.raises(HunterHipError, match=r"\(-3\)"):          # HB_ERR_STATE before hb_plant_reset
                call()
        q_stand = standing_configuration(params, 1, s)[0]
        q0 = np.array([te.place_on_terrain(q_stand, foot_fn, pl) for pl in plane])
        s.plant_reset(q0, eps=te.EPS)
        for call in (lambda: s.plant_set_terrain(plane, mu), s.plant_get_terrain):
            with pytest.raises(HunterHipError, match=r"\(-3\)"):          # ... and in model 0
                call()
        cfg = _cfg(params)
        s.plant_set_contact_model(cfg)
        t = s.plant_get_terrain()                                         # no terrain: what the model amounts to
        assert np.array_equal(t["plane"], np.tile([0.0, 0.0, 1.0, 0.123], (3, 1))) and (t["mu"] == 0.31).all()
        assert np.array_equal(t["frame"], np.tile(np.eye(3), (3, 1, 1)))
        s.plant_set_terrain(plane * np.array([1.0 + 5e-10] * 3 + [1.0]), mu)   # (within 1e-9 of unit length: normalised on the host)
        t = s.plant_get_terrain()
        assert np.abs(t["plane"] - plane).max() <= 1e-15 and np.array_equal(t["mu"], mu)
        assert np.abs(np.linalg.norm(t["plane"][:, :3], axis=1) - 1.0).max() <= 2.3e-16
        for i in range(3):
            assert np.abs(t["frame"][i] - te.frame_of(t["plane"][i, :3])).max() <= 4e-16
        assert np.array_equal(t["frame"][0], np.eye(3))
        bad = []
        for i, (col, val) in enumerate([(0, np.nan), (3, np.inf), (2, 0.4)]):
            p = plane.copy()
            p[i, col] = val
            bad.append((i, p, mu))
        p = plane.copy()
        p[1, :3] *= 1.0 + 1e-8
        m = mu.copy()
        m[2, 3] = -1e-3
        m2 = mu.copy()
        m2[0, 1] = np.nan
        lean = plane.copy()
        lean[1, :3] = te.normal_of(1.1)                                  # n_z = 0.45
        bad += [(1, p, mu), (2, plane, m), (0, None, m2), (1, lean, None)]
        for i, p, m in bad:
            with pytest.raises(HunterHipError, match=rf"\(-1\).*instance {i}\b"):     # HB_ERR_ARG, the first offending instance named
                s.plant_set_terrain(p, m)
            assert np.array_equal(s.plant_get_terrain()["mu"], mu)                     # the terrain in force is kept
        tau = np.array([ce.statics_torque(*qv_fn(q0[i], np.zeros(16))[:3]) for i in range(3)])
        s.plant_step(tau, flags, te.DT, te.SUBSTEPS)
        lam = s.plant_state()["lam"]
        assert (te.to_frame(lam, plane)[:, :, 2] > 1.0).any(axis=1).all()           # every robot stands on ITS plane
        s.plant_set_terrain(None, mu)                                     # plane NULL: the configuration's level ground, a snapshot
        assert np.array_equal(s.plant_get_terrain()["plane"], np.tile([0.0, 0.0, 1.0, 0.123], (3, 1)))
        s.plant_set_terrain(plane, None)                                  # mu NULL: the configuration's mu
        assert (s.plant_get_terrain()["mu"] == 0.31).all()
        s.plant_set_terrain(plane, mu)
        st = s.plant_state()
        s.plant_reset(st["q"], st["v"], eps=te.EPS)                       # the terrain survives hb_plant_reset
        assert np.array_equal(s.plant_get_terrain()["plane"], t["plane"]) and np.array_equal(s.plant_get_terrain()["mu"], mu)
        s.plant_set_contact_model(cfg)                                    # a second mode-1 call keeps the terrain
        assert np.array_equal(s.plant_get_terrain()["mu"], mu)
        # FALLEN along n: a fall height between the base's height along n and its vertical height, on the slope (instance 1)
        along, vertical = q0[1, :3] @ plane[1, :3] - plane[1, 3], q0[1, 2]
        assert along < vertical - 5e-3
        s.plant_set_contact_model(_cfg(params, fall_height=0.5 * (along + vertical), ground_z=0.0))
        s.plant_reset(q0, eps=te.EPS)
        s.plant_step(tau, flags, te.DT, te.SUBSTEPS)
        assert s.plant_contact()["status"][1] & ce.FALLEN
        s.plant_set_terrain(None, None)                                   # off: the same place over level ground is high enough
        s.plant_reset(q0, eps=te.EPS)
        s.plant_step(tau, flags, te.DT, te.SUBSTEPS)
        assert not s.plant_contact()["status"][1] & ce.FALLEN
        # leaving model 1 switches the terrain off
        s.plant_set_terrain(plane, mu)
        s.plant_set_contact_model(None)
        s.plant_set_contact_model(cfg)
        assert (s.plant_get_terrain()["mu"] == 0.31).all() and np.array_equal(s.plant_get_terrain()["frame"][2], np.eye(3))
    finally:
        s.close()


def test_setting_a_terrain_clears_the_impulses(params):
    """After hb_plant_set_terrain the next step equals the step from the same (q, v) with zero impulses, and differs from the warm-started one."""
    from hunter_bipedal_control_amd.rollout import standing_configuration
    s = _solver(params, 2)
    try:
        foot_fn, qv_fn = _device_fns(s)
        q_stand = standing_configuration(params, 1, s)[0]
        scen = [te.slope_scenario(q_stand, qv_fn, foot_fn, f) for f in (2.0, 3.0)]
        flags = np.ones((2, 4), dtype=np.int32)
        tau = np.array([c["tau_fn"](0) for c in scen])
        _, _, plane, mu = _arrays(scen)
        ends = {}
        for how in ("warm", "set_again", "reset"):
            _start(s, params, scen, False)
            for _ in range(3):
                s.plant_step(tau, flags, te.DT, te.SUBSTEPS)
            st = s.plant_state()
            if how == "set_again":
                s.plant_set_terrain(plane, mu)
                assert np.array_equal(s.plant_state()["q"], st["q"]) and np.array_equal(s.plant_state()["v"], st["v"])
            if how == "reset":
                s.plant_reset(st["q"], st["v"], eps=te.EPS)
            s.plant_step(tau, flags, te.DT, te.SUBSTEPS)
            ends[how] = s.plant_state()
        for k in ("q", "v", "lam"):
            assert np.array_equal(ends["set_again"][k], ends["reset"][k]), k
        assert not np.array_equal(ends["warm"]["lam"], ends["reset"]["lam"])
    finally:
        s.close()


def test_resident_loop_keeps_the_scenarios_apart(params):
    """ResidentLoop(terrain=...), B = 4, 30 ticks of the whole closed loop: the run with terrains, gaits and commands rolled by one instance
    gives instance i + 1 what the first run gives instance i, on q, v, lambda and the contact outputs."""
    from hunter_bipedal_control_amd.rollout import ResidentLoop
    normals = np.array([te.normal_of(), te.normal_of(0.05), te.normal_of(0.03, -0.04), te.normal_of()])
    mu = np.array([[0.7] * 4, [0.7] * 4, [0.9, 0.5, 0.3, 0.2], [0.1] * 4])
    cmds = np.array([[0.0, 0.0, 0.0, 0.0], [0.2, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.1], [0.3, 0.0, 0.0, 0.0]])
    gaits = ["stance", "trot", "stance", "trot"]
    hist = []
    for shift in (0, 1):
        s = _solver(params, 4)
        try:
            loop = ResidentLoop(s, params, list(np.roll(gaits, shift)), np.roll(cmds, shift, axis=0), contact_config=dict(fall_height=0.3),
                                terrain=dict(plane=np.roll(normals, shift, axis=0), mu=np.roll(mu, shift, axis=0)))
            t = s.plant_get_terrain()
            assert np.array_equal(t["mu"], np.roll(mu, shift, axis=0)) and np.abs(t["plane"][:, :3] - np.roll(normals, shift, axis=0)).max() <= 3e-16
            ticks = []
            for _ in range(30):
                loop.step()
                ticks.append(_outputs(s, False))
            hist.append(ticks)
        finally:
            s.close()
    for tick, (a, b) in enumerate(zip(*hist)):
        for k in a:
            assert np.array_equal(np.roll(a[k], 1, axis=0), b[k]), (k, tick)
    last = hist[0][-1]
    assert not np.array_equal(last["lam"][0], last["lam"][1])
