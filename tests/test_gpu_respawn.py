"""Respawn of ended instances on the device (hb_plant_set_respawn / hb_plant_respawn / hb_plant_get_respawn; k_plant_respawn) against the
numpy twin of the definition (tests/_respawnemu.py), against the device's own getters, and against exact twins on the device: a context
without a respawn configuration (nobody else is touched) and a context that starts where the respawn put the instance (nothing of the past
survives).  Tolerances: decision, totals and the new episode record exact; the drawn state 1e-12 (the tolerance of the Box-Muller normals
between builds, tests/test_sensors_host.py); what goes through the leg kinematics (placement, anchors, the filter's contact points) 1e-10
(the bound tests/_terrainemu.py holds positions and gaps to)."""
import numpy as np
import pytest

import _contactemu as ce
import _respawnemu as rs
import _terrainemu as te
from hunter_bipedal_control_amd import abi

pytestmark = pytest.mark.gpu

NSTEPS, TILT = 12, 0.2
PUSH_FORCE, TILT_LIMIT = 250.0, 0.12      # test 5 of tests/test_gpu_episode.py: under this push the robot passes this tilt on tick 36


def _solver(params, batch):
    from hunter_bipedal_control_amd.solver import HunterSolver
    return HunterSolver(params, batch=batch, max_nodes=108)


def _foot_fn(s):
    def foot_fn(q):
        q = np.atleast_2d(q)
        x = np.zeros((q.shape[0], 22))
        x[:, 6:9], x[:, 9:12], x[:, 12:] = q[:, 0:3], q[:, 3:6], q[:, 6:]
        return s.eval_foot_kinematics(x, np.zeros((q.shape[0], 22)))[0]
    return foot_fn


def _qv_fn(s, foot_fn):
    def qv_fn(q, v):
        pl = ce.GroundPlant(None, foot_fn, q[None], v[None])
        return tuple(a[0] for a in s.eval_rbd(pl.rbd()))
    return qv_fn


# ---- tests 1 and 2: open loop ------------------------------------------------------------------------------------------------------------
def _open_loop_setup(params, s):
    """B = 6: the five terrain scenarios and a sixth on the level plane; instances 4 and 5 start rolled beyond the tilt limit and are spawned
    upright."""
    from hunter_bipedal_control_amd.rollout import standing_configuration
    foot_fn = _foot_fn(s)
    q_stand = standing_configuration(params, 1, s)[0]
    scen = te.scenarios(q_stand, _qv_fn(s, foot_fn), foot_fn)
    scen.append(dict(scen[0]))
    q_spawn = np.array([c["q0"] for c in scen])
    q0 = q_spawn.copy()
    q0[4, 5], q0[5, 5] = 0.3, -0.35
    v_spawn = np.zeros((6, 16))
    v_spawn[:, 0] = 0.01 * np.arange(6)
    return scen, q0, np.array([c["v0"] for c in scen]), q_spawn, v_spawn


RESPAWN = dict(hold_ticks=2, place=1, clearance=0.002, yaw_range=0.3, joint_pos_sigma=0.01, base_vel_sigma=0.05, seed=0xABCDEF0123, instance_offset=7)


def _getters(s):
    st, con, jo, act, sens = s.plant_state(), s.plant_contact(), s.plant_get_joints(), s.plant_get_actuator(), s.plant_sense(want_outputs=True)
    ep = s.plant_episode(want_trace=True)
    xh, P = s.estimator_filter()
    out = dict(st)
    out.update({"c_" + k: a for k, a in con.items()})
    out.update({"j_" + k: a for k, a in jo.items()})
    out.update({"a_" + k: a for k, a in act.items()})
    out.update({"s_" + k: a for k, a in sens.items()})
    out.update({"e_" + k: a for k, a in ep.items()})
    out.update(xhat=xh, P=P, latch=s.joint_emergency_stop())
    return out


def _open_loop_run(params, respawn):
    """12 open-loop hybrid steps under the joint model with an episode (tilt limit, stop_on_fall, a trace); respawn: None, or the fields of
    the configuration, with hb_plant_respawn after every step.  -> per step dict(before, after) of every getter (and the totals)."""
    s = _solver(params, 6)
    try:
        scen, q0, v0, q_spawn, v_spawn = _open_loop_setup(params, s)
        s.plant_reset(q0, v0, eps=te.EPS)
        s.plant_set_contact_model(abi.make_contact_config(params, mu=0.31, ground_z=0.123, erp=te.ERP, sweeps=te.SWEEPS))
        s.plant_set_joint_model(abi.make_joint_model(params))
        s.plant_set_terrain(np.array([c["plane"] for c in scen]), np.array([c["mu"] for c in scen]))
        planes = s.plant_get_terrain()["plane"]                      # (the unit normals as the device holds them)
        s.plant_set_episode(abi.make_episode_config(tilt_limit=TILT, stop_on_fall=1, trace_every=1, trace_capacity=4))
        xh0 = np.zeros((6, 18))
        xh0[:, 0:3] = q0[:, 0:3]
        s.estimator_reset(abi.make_estimator_config(params), xh0)
        cfg = None
        if respawn is not None:
            cfg = abi.make_respawn_config(**respawn)
            s.plant_set_respawn(cfg, q_spawn, v_spawn)
        flags = np.ones((6, 4), dtype=np.int32)
        steps = []
        for tick in range(NSTEPS):
            q = s.plant_state()["q"]
            tau = np.array([c["tau_fn"](tick) for c in scen])
            s.plant_step_hybrid(dict(pos_des=q[:, 6:].copy(), vel_des=np.zeros((6, 10)), kp=np.full((6, 10), 5.0), kd=np.full((6, 10), 0.05), tau_ff=tau),
                                flags, te.DT, te.SUBSTEPS)
            rec = dict(before=_getters(s))
            if respawn is not None:
                s.plant_respawn()
                rec.update(after=_getters(s), totals=s.plant_respawn_totals(want_state=True))
            steps.append(rec)
        return dict(steps=steps, cfg=cfg, planes=planes, q_spawn=q_spawn, v_spawn=v_spawn)
    finally:
        s.close()


@pytest.fixture(scope="module")
def open_loop(params):
    """The same 12 steps three times: without a respawn configuration, with max_ticks = 5 and with max_ticks = 0.  Shared, left unchanged."""
    return dict(none=_open_loop_run(params, None), timeout=_open_loop_run(params, dict(RESPAWN, max_ticks=5)),
                hold=_open_loop_run(params, dict(RESPAWN, max_ticks=0)))


def _episode_of(g, i):
    return {k[2:]: a[i] for k, a in g.items() if k.startswith("e_") and k != "e_trace"}


def test_open_loop_who_and_what(open_loop, params):
    """B = 6 on the terrain scenarios, contact model 1 with the joint model, hybrid steps; tilt limit 0.2, hold_ticks 2, max_ticks 5 (one
    value for the batch: every instance still up times out with its fifth tick), hb_plant_respawn after each of 12 steps.  Instances 4 and
    5 start rolled beyond the limit, end on step 0 and are put back after step 2.  Per step: who is respawned, the totals and the new record
    == the twin; the spawned state within the draw's / the kinematics' tolerance; the getters of a respawned instance."""
    run = open_loop["timeout"]
    cfg, planes = run["cfg"], run["planes"]
    s = _solver(params, 1)
    try:
        foot_fn = _foot_fn(s)
        twin = [rs.totals_init() for _ in range(6)]
        who_by_step = []
        for tick, step in enumerate(run["steps"]):
            b, a, tot = step["before"], step["after"], step["totals"]
            who = []
            for i in range(6):
                rec = _episode_of(b, i)
                cause = rs.decide(cfg, rec)
                if cause:
                    who.append(i)
                    twin[i] = rs.fold(twin[i], rec, cause)
                for name in abi.RESPAWN_INT_FIELDS + abi.RESPAWN_DOUBLE_FIELDS:
                    assert tot[name][i] == twin[i][name], (tick, i, name, tot[name][i], twin[i][name])
                if not cause:
                    for k in b:
                        assert np.array_equal(a[k][i], b[k][i]), (tick, i, k)
                    continue
                # the last spawned state against the twin's draw and placement
                e = int(twin[i]["EPISODE_INDEX"])
                qd, vd = rs.spawn_state(cfg, cfg.instance_offset + i, e, run["q_spawn"][i], run["v_spawn"][i])
                qt = rs.place(cfg, qd, foot_fn, planes[i])
                ql, vl = tot["q_last"][i], tot["v_last"][i]
                assert np.abs(ql[3:] - qt[3:]).max() <= rs.NORMAL_TOL and np.abs(vl - vd).max() <= rs.NORMAL_TOL, (tick, i)
                assert np.abs(ql[:3] - qt[:3]).max() <= te.TOL_Q and abs(rs.lowest_gap(ql, foot_fn, planes[i]) - cfg.clearance) <= te.TOL_Q
                # the new episode record: exact, from the returned state
                want = rs.init_record(ql, planes[i])
                got = _episode_of(a, i)
                for name, _, _ in abi.EPISODE_INT_FIELDS + abi.EPISODE_DOUBLE_FIELDS:
                    assert np.array_equal(got[name], want[name]), (tick, i, name, got[name], want[name])
                assert not a["e_trace"][i].any() and (b["e_trace"][i].any() or b["e_TICKS"][i] == 0)
                # the device's own getters
                assert np.array_equal(a["q"][i], ql) and np.array_equal(a["v"][i], vl)
                assert not a["lam"][i].any() and not a["vdot"][i].any()
                for k in a:
                    if k[:2] in ("c_", "j_", "a_"):
                        assert not np.asarray(a[k][i]).any(), (tick, i, k)
                assert a["latch"][i] == 0 and not (a["c_status"][i] & abi.HB_CONTACT_FALLEN)
                assert np.array_equal(a["P"][i], 100.0 * np.eye(18)) and np.array_equal(a["xhat"][i, 0:3], ql[0:3]) and not a["xhat"][i, 3:6].any()
                assert np.abs(a["xhat"][i, 6:18] - np.asarray(foot_fn(ql[None]))[0].reshape(12)).max() <= te.TOL_Q
                rbd = a["rbd"][i]
                assert np.array_equal(rbd[0:3], ql[3:6]) and np.array_equal(rbd[3:6], ql[0:3]) and np.array_equal(rbd[6:16], ql[6:])
                assert np.array_equal(a["s_joint_pos"][i], ql[6:]) and not a["s_joint_torque"][i].any() and a["s_contact_flag"][i].tolist() == [1] * 4
                # something was there to clear
                assert b["j_tau_applied"][i].any() and b["a_tau_first"][i].any()
            who_by_step.append(who)
        print("respawned per step:", who_by_step)
        # the rolled two end on step 0 and wait two steps; everybody else times out with TICKS = 5; then again five ticks after the spawn
        assert who_by_step == [[], [], [4, 5], [], [0, 1, 2, 3], [], [], [4, 5], [], [0, 1, 2, 3], [], []]
        b2 = run["steps"][2]["before"]
        assert b2["latch"][4] == 1 and b2["latch"][5] == 1 and b2["e_END_TICK"][4] == 0 and b2["e_STEPS"][4] == 3   # stop_on_fall had latched
        last = run["steps"][-1]["totals"]
        assert last["N_FALLEN"].tolist() == [0, 0, 0, 0, 1, 1] and last["N_TIMEOUT"].tolist() == [2, 2, 2, 2, 1, 1]
        assert (last["STEPS_SUM"] + run["steps"][-1]["after"]["e_STEPS"] == NSTEPS).all()
    finally:
        s.close()


def test_nobody_else_is_touched(open_loop):
    """Every array the getters return, bit for bit against the context without a respawn configuration: with max_ticks = 0 instances 0 - 3
    are never respawned (all 12 steps); with max_ticks = 5 every instance up to the step of its first respawn."""
    ref = open_loop["none"]["steps"]
    for name, never in (("hold", [0, 1, 2, 3]), ("timeout", [])):
        run = open_loop[name]["steps"]
        seen = set()
        for tick in range(NSTEPS):
            for i in range(6):
                if i in seen:
                    continue
                for k, want in ref[tick]["before"].items():
                    assert np.array_equal(run[tick]["before"][k][i], want[i]), (name, tick, i, k)
                if run[tick]["totals"]["EPISODES"][i] > 0:
                    seen.add(i)
                else:
                    for k, want in ref[tick]["before"].items():
                        assert np.array_equal(run[tick]["after"][k][i], want[i]), (name, tick, i, k)
        if never:
            assert seen == {4, 5} and (open_loop[name]["steps"][-1]["totals"]["EPISODES"][never] == 0).all()
        else:
            assert seen == set(range(6))


# ---- test 3: the closed-loop twin ----------------------------------------------------------------------------------------------------------
LOOP = dict(gaits=["stance", "trot", "stance", "trot"], cmds=np.array([[0.0, 0.0, 0.0, 0.0], [0.2, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.1], [0.3, 0.0, 0.0, 0.0]]))
EVERY = 8


def _make_loop(s, params, respawn, device_gait=False, use_estimator=True):
    from hunter_bipedal_control_amd.rollout import ResidentLoop
    return ResidentLoop(s, params, LOOP["gaits"], LOOP["cmds"], mpc_every=EVERY, contact_config={}, use_estimator=use_estimator,
                        device_gait=device_gait, episode=dict(tilt_limit=TILT), respawn=respawn)


def _tilt_instance_1(s, params):
    """The plant restarted with instance 1 rolled beyond the tilt limit (contact model, episode and respawn configuration survive)."""
    from hunter_bipedal_control_amd.rollout import standing_configuration
    q0 = standing_configuration(params, 4, s)
    q0[1, 5] = 0.3
    s.plant_reset(q0)
    return q0


def _closed_tick(loop, s):
    """One tick with the outputs on the host -> what the twin is compared on."""
    mpc_tick = loop.tick % loop.mpc_every == 0
    loop.step(want_outputs=True)
    st = s.plant_state()
    out = dict(q=st["q"], v=st["v"], torque=loop.last["cmd"]["torque"], wbc_sol=loop.last["out"]["sol"], wbc_status=loop.last["out"]["status"])
    if mpc_tick:
        x, u = s.get_solution()
        out.update(mpc_x=x, mpc_u=u, mpc_status=s.mpc_status())
    return out


def test_closed_loop_twin_nothing_of_the_past_survives(params):
    after = 2 * EVERY + 1
    runs = {}
    s = _solver(params, 4)
    try:                                            # the run with the respawn
        loop = _make_loop(s, params, dict(place=0))
        _tilt_instance_1(s, params)
        pre = [_closed_tick(loop, s) for _ in range(EVERY)]           # the respawn is enqueued behind the plant step of the eighth tick
        tot = s.plant_respawn_totals(want_state=True)
        xhat = s.estimator_filter()[0]
        assert tot["EPISODES"].tolist() == [0, 1, 0, 0] and tot["LAST_CAUSE"][1] == abi.HB_EP_FALLEN and tot["LAST_TICKS"][1] == 0
        assert np.array_equal(s.plant_state()["q"][1], tot["q_last"][1])
        t0, tick0 = loop.t, loop.tick
        runs["respawn"] = dict(pre=pre, post=[_closed_tick(loop, s) for _ in range(after)])
    finally:
        s.close()
    s = _solver(params, 4)
    try:                                            # the twin: starts where the respawn put instance 1, cold
        loop = _make_loop(s, params, None)
        s.plant_reset(tot["q_last"], tot["v_last"])
        s.estimator_reset(abi.make_estimator_config(params), xhat)
        loop.t, loop.tick = t0, tick0
        runs["twin"] = dict(post=[_closed_tick(loop, s) for _ in range(after)])
    finally:
        s.close()
    s = _solver(params, 4)
    try:                                            # the same run without a respawn configuration
        loop = _make_loop(s, params, None)
        _tilt_instance_1(s, params)
        runs["none"] = dict(pre=[_closed_tick(loop, s) for _ in range(EVERY)], post=[_closed_tick(loop, s) for _ in range(after)])
    finally:
        s.close()
    keys = set()
    for tick in range(after):
        a, b = runs["respawn"]["post"][tick], runs["twin"]["post"][tick]
        assert a.keys() == b.keys()
        for k in a:
            same = np.array_equal(a[k][1], b[k][1])
            if not same:
                print("instance 1 differs from its twin:", k, "tick", tick, np.abs(np.asarray(a[k][1], dtype=float) - np.asarray(b[k][1], dtype=float)).max())
            assert same, (k, tick)
            keys.add(k)
    assert keys == {"q", "v", "torque", "wbc_sol", "wbc_status", "mpc_x", "mpc_u", "mpc_status"}
    assert np.isfinite(runs["respawn"]["post"][-1]["q"]).all() and np.abs(runs["respawn"]["post"][-1]["torque"][1]).max() > 0.0
    for part in ("pre", "post"):
        for tick, (a, b) in enumerate(zip(runs["respawn"][part], runs["none"][part])):
            for k in a:
                for i in (0, 2, 3):
                    assert np.array_equal(a[k][i], b[k][i]), ("against the run without respawn", part, tick, k, i)
    # and the respawn did something: the fallen instance of the run without it is somewhere else
    assert not np.array_equal(runs["respawn"]["post"][0]["q"][1], runs["none"]["post"][0]["q"][1])


# ---- test 4: the device gait manager -------------------------------------------------------------------------------------------------------
def test_device_gait_state_of_a_respawned_instance(params):
    s = _solver(params, 4)
    try:
        loop = _make_loop(s, params, dict(place=0), device_gait=True, use_estimator=False)
        _tilt_instance_1(s, params)
        for _ in range(EVERY - 1):
            loop.step()
        before = s.gait_state()
        loop.step()                                 # the eighth tick: no MPC call in it, the respawn behind its plant step
        after = s.gait_state()
        assert s.plant_respawn_totals()["EPISODES"].tolist() == [0, 1, 0, 0]
    finally:
        s.close()
    s = _solver(params, 4)
    try:                                            # the same eight ticks without a respawn configuration, then hb_gait_reset with a mask
        loop = _make_loop(s, params, None, device_gait=True, use_estimator=False)
        _tilt_instance_1(s, params)
        for _ in range(EVERY):
            loop.step()
        s.gait_reset(abi.make_gait_config(params), mask=np.array([0, 1, 0, 0], dtype=np.uint8))
        fresh = s.gait_state()
    finally:
        s.close()
    changed = False
    for k in after:
        assert np.array_equal(after[k], fresh[k]), k   # (slots behind n_events keep what they held, in both)
        n_ev = int(fresh["n_events"][1])
        assert n_ev == abi.make_gait_config(params).n_init_events and fresh["level"][1] == 0 and not fresh["cmd"][1].any()
        changed = changed or not np.array_equal(before[k][1], after[k][1])
        for i in (0, 2, 3):
            assert np.array_equal(after[k][i], before[k][i]), (k, i)
    assert changed                                  # the trotting instance's gait object had moved on before


# ---- test 5: no read-back, many episodes ---------------------------------------------------------------------------------------------------
def test_run_without_read_back_many_episodes(params):
    from hunter_bipedal_control_amd.rollout import ResidentLoop, respawn_summary
    n = 17 * EVERY
    s = _solver(params, 2)
    try:
        loop = ResidentLoop(s, params, ["stance", "stance"], np.zeros((2, 4)), mpc_every=EVERY, contact_config={}, episode=dict(tilt_limit=TILT_LIMIT),
                            respawn=dict(hold_ticks=4, max_ticks=64))
        wrench = np.zeros((2, 6))
        wrench[1, 1] = PUSH_FORCE
        s.plant_set_external_wrench(wrench)
        loop.run(n)
        tot, rec = loop.respawn_totals(), loop.episode()
        print({k: a.tolist() for k, a in tot.items()}, "current STEPS", rec["STEPS"].tolist())
        assert tot["EPISODES"][1] >= 1 and tot["N_FALLEN"][1] >= 1 and tot["N_TIMEOUT"][0] >= 1 and tot["N_FALLEN"][0] == 0
        assert np.array_equal(tot["N_FALLEN"] + tot["N_NONFINITE"] + tot["N_TIMEOUT"], tot["EPISODES"])
        assert (tot["TICKS_MIN"] <= tot["LAST_TICKS"]).all() and (tot["LAST_TICKS"] <= tot["TICKS_MAX"]).all()
        assert np.array_equal(tot["EPISODE_INDEX"], tot["EPISODES"])
        assert (tot["STEPS_SUM"] + rec["STEPS"] == n).all()          # the identity of the header
        summ = respawn_summary(tot, loop.dt)
        assert np.array_equal(summ["episodes"], tot["EPISODES"]) and summ["fall_rate"][0] == 0.0 and summ["fall_rate"][1] > 0.0
        assert np.allclose(summ["mean_ticks"] * tot["EPISODES"], tot["TICKS_SUM"], rtol=1e-14, atol=0.0)
    finally:
        s.close()


# ---- test 6: shards ------------------------------------------------------------------------------------------------------------------------
def test_a_shard_spawns_the_states_of_its_slice(params):
    from hunter_bipedal_control_amd.rollout import standing_configuration
    fields = dict(max_ticks=1, place=1, clearance=0.01, yaw_range=0.4, joint_pos_sigma=0.02, base_vel_sigma=0.1, seed=31337)
    states = {}
    for name, B, offset in (("whole", 4, 0), ("shard", 2, 2)):
        s = _solver(params, B)
        try:
            q0 = standing_configuration(params, 4, s)
            q0[:, 0] = 0.1 * np.arange(4)
            q0 = q0[offset:offset + B]
            s.plant_reset(q0)
            s.plant_set_episode(abi.make_episode_config())
            s.plant_set_respawn(abi.make_respawn_config(instance_offset=offset, **fields), q0, None)
            out = []
            for _ in range(3):                      # every instance times out after every step: three episodes each
                s.plant_step(np.zeros((B, 10)), np.ones((B, 4), dtype=np.int32), 0.002, 4)
                s.plant_respawn()
                tot = s.plant_respawn_totals(want_state=True)
                out.append((tot["q_last"], tot["v_last"], tot["EPISODE_INDEX"]))
            states[name] = out
        finally:
            s.close()
    for (qw, vw, ew), (qs, vs, es) in zip(states["whole"], states["shard"]):
        assert np.array_equal(qw[2:4], qs) and np.array_equal(vw[2:4], vs) and np.array_equal(ew[2:4], es)
    assert states["whole"][2][2].tolist() == [3] * 4
    assert not np.array_equal(states["whole"][0][0][2], states["whole"][1][0][2]) and not np.array_equal(states["whole"][0][0][2, 6:], states["whole"][0][0][3, 6:])


# ---- test 7: refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(params):
    from hunter_bipedal_control_amd import workload
    from hunter_bipedal_control_amd.rollout import standing_configuration
    from hunter_bipedal_control_amd.solver import HunterHipError
    s = _solver(params, 4)
    try:
        w = workload.device_trot_batch(s, params, n_intervals=20)
        s.set_resident_inputs(w["x0"], w["t_now"], w["rbd"])
        s.step_resident()
        q0 = standing_configuration(params, 4, s)
        cfg = abi.make_respawn_config(max_ticks=3)
        for call in (lambda: s.plant_set_respawn(cfg, q0), s.plant_respawn, s.plant_respawn_totals):
            with pytest.raises(HunterHipError, match=r"\(-3\)"):           # before hb_plant_reset
                call()
        s.plant_reset(q0)
        with pytest.raises(HunterHipError, match=r"\(-3\).*episode"):      # no episode in force
            s.plant_set_respawn(cfg, q0)
        s.plant_set_episode(abi.make_episode_config())
        with pytest.raises(HunterHipError, match=r"\(-3\)"):               # no configuration in force yet
            s.plant_respawn()
        with pytest.raises(HunterHipError, match=r"\(-1\).*q_spawn"):
            s.plant_set_respawn(cfg, None)
        s.plant_set_respawn(cfg, q0)
        for call, name in ((s.step_resident, "hb_step_resident"), (lambda: _tick(s, w), "hb_tick_resident")):
            with pytest.raises(HunterHipError, match=r"\(-3\).*respawn configuration"):
                call()
        flags, tau = np.ones((4, 4), dtype=np.int32), np.zeros((4, 10))
        for _ in range(3):
            s.plant_step(tau, flags, 0.002, 4)
        s.plant_respawn()
        assert s.plant_respawn_totals()["N_TIMEOUT"].tolist() == [1] * 4
        for bad in (dict(clearance=-1.0), dict(yaw_range=float("nan")), dict(joint_pos_sigma=float("inf")), dict(base_vel_sigma=-0.1), dict(hold_ticks=-1),
                    dict(max_ticks=-2), dict(place=3)):
            with pytest.raises(HunterHipError, match=r"\(-1\).*" + next(iter(bad))):
                s.plant_set_respawn(abi.make_respawn_config(**bad), q0)
            assert s.plant_respawn_totals()["N_TIMEOUT"].tolist() == [1] * 4          # the configuration in force (and its totals) is kept
        for _ in range(3):
            s.plant_step(tau, flags, 0.002, 4)
        s.plant_respawn()                                                   # max_ticks = 3 is still the rule
        assert s.plant_respawn_totals()["N_TIMEOUT"].tolist() == [2] * 4
        s.plant_reset(q0)                                                   # the configuration survives, the totals restart
        assert s.plant_respawn_totals()["EPISODES"].tolist() == [0] * 4
        s.plant_set_respawn(None)
        s.step_resident()                                                   # and the range paths work again
        s.plant_set_respawn(cfg, q0)
        s.plant_set_episode(None)                                           # turning the episode off turns respawn off
        with pytest.raises(HunterHipError, match=r"\(-3\)"):
            s.plant_respawn()
        s.step_resident()
    finally:
        s.close()


def _tick(s, w):
    B = s.B
    quat = np.tile([0.0, 0.0, 0.0, 1.0], (B, 1))
    s.tick_resident(0.002, quat, np.zeros((B, 3)), np.tile([0.0, 0.0, 9.81], (B, 1)), np.zeros((B, 10)), np.zeros((B, 10)), np.ones((B, 4), dtype=np.int32),
                    w["t_now"], 1.0, np.zeros((B, 4)))
