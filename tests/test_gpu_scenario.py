"""Scenario draw at respawn on the device (hb_plant_set_scenario / hb_plant_get_scenario / hb_plant_get_scenario_log; k_plant_scenario,
k_plant_push) against the exact twin of the definition (tests/_scenarioemu.py), against the device's own getters, and against exact
twins on the device: a context without a scenario (nobody else is touched), a fresh context given the drawn scenario through the host
setters (the drawn records are the host's, bit for bit) and a run whose host sets the push.  The draw has no transcendental function in
it, so every comparison of a drawn quantity is ==; the one tolerance is the placement's 1e-10, the bound tests/test_gpu_respawn.py holds
quantities that go through the leg kinematics to.  The open-loop setup is that file's: B = 6, the five terrain scenarios plus one level,
instances 4 and 5 start beyond the tilt limit, hold_ticks = 2, 12 hybrid steps, max_ticks = 5 in one run and 0 in another."""
import numpy as np
import pytest

import _contactemu as ce
import _respawnemu as rs
import _scenarioemu as sc
import _terrainemu as te
from hunter_bipedal_control_amd import abi

pytestmark = pytest.mark.gpu

NSTEPS, TILT, GROUND_Z, MU0 = 12, 0.2, 0.123, 0.31
RESPAWN = dict(hold_ticks=2, place=1, clearance=0.002, yaw_range=0.3, joint_pos_sigma=0.01, base_vel_sigma=0.05, seed=0xABCDEF0123, instance_offset=7)
SCENARIO = dict(channels=abi.HB_SC_ALL, mu_per_point=1, grade_max=0.2, mu_lo=0.05, mu_hi=0.8, payload_mass_max=2.0, payload_center=(0.0, 0.0, 0.15),
                payload_half_extent=(0.08, 0.04, 0.02), mass_scale_range=0.15, push_force_max=5.0, push_start_lo=1, push_start_hi=3, push_ticks=2,
                seed=0x5CE7A210F00D, log_capacity=2)
NO_PUSH = abi.HB_SC_ALL & ~abi.HB_SC_PUSH


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


def _setup(params, s):
    """B = 6: the five terrain scenarios and a sixth on the level plane; instances 4 and 5 start rolled beyond the tilt limit and are spawned
    upright (tests/test_gpu_respawn.py)."""
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


def _getters(s, scenario):
    st, con, jo, act = s.plant_state(), s.plant_contact(), s.plant_get_joints(), s.plant_get_actuator()
    out = dict(st)
    out.update({"c_" + k: a for k, a in con.items()})
    out.update({"j_" + k: a for k, a in jo.items()})
    out.update({"a_" + k: a for k, a in act.items()})
    out.update({"e_" + k: a for k, a in s.plant_episode(want_trace=True).items()})
    out.update({"t_" + k: a for k, a in s.plant_get_terrain().items()})
    out.update({"m_" + k: a for k, a in s.plant_model_variation().items()})
    out.update(latch=s.joint_emergency_stop())
    if scenario:
        log = s.plant_scenario_log()
        out.update(scen=s.plant_scenario(), log=log["log"], count=log["count"])
    return out


def _command(s, scen, tick, rows=slice(None)):
    q = s.plant_state()["q"]
    n = q.shape[0]
    tau = np.array([c["tau_fn"](tick) for c in scen])[rows]
    return dict(pos_des=q[:, 6:].copy(), vel_des=np.zeros((n, 10)), kp=np.full((n, 10), 5.0), kd=np.full((n, 10), 0.05), tau_ff=tau)


def _run(params, respawn, scenario, joints=True, rows=slice(None), host_push=None):
    """12 open-loop hybrid steps (under the joint model if `joints`) with an episode (tilt limit, stop_on_fall, a trace); respawn / scenario:
    None, or the fields of the configurations, with hb_plant_respawn after every step.  rows: the instances of the setup this context holds.
    host_push: a scenario configuration whose push the HOST applies through hb_plant_set_external_wrench, from the twin's draw.
    -> per step dict(before, after) of every getter (and the totals)."""
    B = len(range(6)[rows])
    s = _solver(params, B)
    try:
        scen, q0, v0, q_spawn, v_spawn = _setup(params, s)
        scen_rows = scen[rows]
        s.plant_reset(q0[rows], v0[rows], eps=te.EPS)
        s.plant_set_contact_model(abi.make_contact_config(params, mu=MU0, ground_z=GROUND_Z, erp=te.ERP, sweeps=te.SWEEPS))
        if joints:
            s.plant_set_joint_model(abi.make_joint_model(params))
        s.plant_set_terrain(np.array([c["plane"] for c in scen_rows]), np.array([c["mu"] for c in scen_rows]))
        s.plant_set_episode(abi.make_episode_config(tilt_limit=TILT, stop_on_fall=1, trace_every=1, trace_capacity=4))
        cfg = scfg = None
        if respawn is not None:
            cfg = abi.make_respawn_config(**respawn)
            s.plant_set_respawn(cfg, q_spawn[rows], v_spawn[rows])
        if scenario is not None:
            scfg = abi.make_scenario_config(**scenario)
            s.plant_set_scenario(scfg)
        push = np.tile([-1.0, 0.0, 0.0], (B, 1))          # the host's copy of the push records (host_push)
        flags = np.ones((B, 4), dtype=np.int32)
        steps = []
        for tick in range(NSTEPS):
            wrench = None
            if host_push is not None:
                now = s.plant_episode()["STEPS"]
                wrench = np.array([sc.push_wrench(host_push, push[i], int(now[i])) for i in range(B)])
                s.plant_set_external_wrench(wrench)
            s.plant_step_hybrid(_command(s, scen, tick, rows), flags, te.DT, te.SUBSTEPS)
            rec = dict(before=_getters(s, scenario is not None), wrench=wrench)
            if respawn is not None:
                s.plant_respawn()
                rec.update(after=_getters(s, scenario is not None), totals=s.plant_respawn_totals(want_state=True))
                if host_push is not None:
                    for i in range(B):
                        if rec["totals"]["EPISODE_INDEX"][i] != (steps[-1]["totals"]["EPISODE_INDEX"][i] if steps else 0):
                            push[i] = sc.draw(host_push, cfg.instance_offset + i, int(rec["totals"]["EPISODE_INDEX"][i]), (0.0, 0.0), 0.0, None,
                                              np.zeros(14), None)["push"]
            steps.append(rec)
        return dict(steps=steps, cfg=cfg, scfg=scfg, q_spawn=q_spawn[rows], v_spawn=v_spawn[rows], scen=scen)
    finally:
        s.close()


@pytest.fixture(scope="module")
def runs(params):
    """Shared, left unchanged: the two respawn runs without a scenario and the two with all five channels."""
    return dict(timeout0=_run(params, dict(RESPAWN, max_ticks=5), None), hold0=_run(params, dict(RESPAWN, max_ticks=0), None),
                timeout=_run(params, dict(RESPAWN, max_ticks=5), SCENARIO), hold=_run(params, dict(RESPAWN, max_ticks=0), SCENARIO))


def _episode_of(g, i):
    return {k[2:]: a[i] for k, a in g.items() if k.startswith("e_") and k != "e_trace"}


def _model_of(g, i):
    return dict(mass=g["m_mass"][i], com=g["m_com"][i], inertia=g["m_inertia"][i], total_mass=g["m_total_mass"][i])


def _ter_of(g, i):
    return np.concatenate([g["t_frame"][i].reshape(9), [g["t_plane"][i, 3]], g["t_mu"][i]])


def _who(run):
    """Per step the instances the twin of the decision respawns, from the `before` getters."""
    return [[i for i in range(len(step["before"]["q"])) if rs.decide(run["cfg"], _episode_of(step["before"], i))] for step in run["steps"]]


# ---- test 1 --------------------------------------------------------------------------------------------------------------------------------
def test_records_and_log(runs):
    nominal = _model_of(runs["timeout0"]["steps"][0]["before"], 0)      # (no variation in force: the nominal model)
    for name in ("timeout", "hold"):
        run = runs[name]
        cfg, scfg = run["cfg"], run["scfg"]
        who_by_step = _who(run)
        episodes, logged = [0] * 6, [[] for _ in range(6)]
        for tick, step in enumerate(run["steps"]):
            b, a = step["before"], step["after"]
            for i in range(6):
                if i not in who_by_step[tick]:
                    for k in b:
                        assert np.array_equal(a[k][i], b[k][i]), (name, tick, i, k)       # stayed: not one byte
                    continue
                rec = _episode_of(b, i)
                if len(logged[i]) < scfg.log_capacity:
                    logged[i].append(sc.log_row(episodes[i], rs.decide(cfg, rec), rec, b["scen"][i]))
                episodes[i] += 1
                tw = sc.draw(scfg, cfg.instance_offset + i, episodes[i], run["q_spawn"][i, 0:2], GROUND_Z, nominal, _ter_of(b, i), _model_of(b, i))
                assert np.array_equal(a["scen"][i], tw["scen"]), (name, tick, i, a["scen"][i] - tw["scen"])
                assert np.array_equal(_ter_of(a, i), tw["ter"]), (name, tick, i, _ter_of(a, i) - tw["ter"])
                assert np.array_equal(a["t_plane"][i, 0:3], tw["ter"][[2, 5, 8]])
                got = _model_of(a, i)
                for k in ("mass", "com", "inertia", "total_mass"):
                    assert np.array_equal(got[k], tw["model"][k]), (name, tick, i, k, got[k] - tw["model"][k])
                assert a["count"][i] == len(logged[i]) and step["totals"]["EPISODE_INDEX"][i] == episodes[i]
                for j in range(scfg.log_capacity):
                    want = logged[i][j] if j < len(logged[i]) else np.zeros(abi.HB_SC_LOG_W)
                    assert np.array_equal(a["log"][i, j], want), (name, tick, i, j)
                # the drawn parameters are inside their ranges and are something
                p = abi.split_scenario(a["scen"][i])
                assert np.abs(p["GRADE"]).max() <= 0.2 and p["GRADE"].all() and 0.05 <= p["MUS"].min() and p["MUS"].max() <= 0.8
                assert 0.0 < p["PAYLOAD_M"] < 2.0 and np.abs(p["SCALE"] - 1.0).max() <= 0.15 and 1 <= p["PUSH_START"] <= 3
        print(name, "respawned per step:", who_by_step, "logged", [len(x) for x in logged])
        assert sum(len(w) for w in who_by_step) >= 2 and any(len(w) < 6 for w in who_by_step)
        if name == "timeout":
            assert max(episodes) >= 2 and max(len(x) for x in logged) == 2       # somebody respawns more than once, and a log is full
        # an instance that never respawns: every getter == the same run without a scenario (and its scen is that of episode 0)
        never = [i for i in range(6) if episodes[i] == 0]
        ref = runs[name + "0"]["steps"]
        for i in never:
            for tick in range(NSTEPS):
                for part in ("before", "after"):
                    for k, want in ref[tick][part].items():
                        assert np.array_equal(run["steps"][tick][part][k][i], want[i]), (name, "never", tick, i, k)
                    assert np.array_equal(run["steps"][tick][part]["scen"][i], sc.init_row()[0]) and run["steps"][tick][part]["count"][i] == 0
        if name == "hold":
            assert never == [0, 1, 2, 3]
    # every instance up to its first respawn, too
    for name in ("timeout", "hold"):
        seen = set()
        for tick in range(NSTEPS):
            for i in range(6):
                if i in seen:
                    continue
                for k, want in runs[name + "0"]["steps"][tick]["before"].items():
                    assert np.array_equal(runs[name]["steps"][tick]["before"][k][i], want[i]), (name, tick, i, k)
                if runs[name]["steps"][tick]["totals"]["EPISODES"][i] > 0:
                    seen.add(i)


# ---- test 2 --------------------------------------------------------------------------------------------------------------------------------
def test_placement_on_the_drawn_plane(runs, params):
    s = _solver(params, 1)
    try:
        foot_fn = _foot_fn(s)
        n = 0
        for name in ("timeout", "hold"):
            run = runs[name]
            for tick, who in enumerate(_who(run)):
                a, tot = run["steps"][tick]["after"], run["steps"][tick]["totals"]
                for i in who:
                    plane = a["t_plane"][i]
                    assert not np.array_equal(plane, run["steps"][tick]["before"]["t_plane"][i])       # a new plane
                    gap = rs.lowest_gap(tot["q_last"][i], foot_fn, plane)
                    assert abs(gap - run["cfg"].clearance) <= 1e-10, (name, tick, i, gap)
                    assert np.array_equal(a["q"][i], tot["q_last"][i])
                    n += 1
        assert n >= 6
    finally:
        s.close()


# ---- test 3 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("joints", [False, True], ids=["contact", "joints"])
def test_exact_device_twin_through_the_host_setters(params, joints):
    """Instances 4 and 5 respawn after step 2 (hold_ticks = 2).  A fresh context given the drawn (n0, d), mu, scales and payload through
    hb_plant_set_terrain / hb_plant_set_model_variation and started from the spawned state steps == them for the following three ticks."""
    scenario = dict(SCENARIO, channels=NO_PUSH)
    run = _run(params, dict(RESPAWN, max_ticks=0), scenario, joints=joints)
    assert _who(run)[2] == [4, 5] and all(not w for t, w in enumerate(_who(run)[:6]) if t != 2)
    cfg, scfg = run["cfg"], run["scfg"]
    tot = run["steps"][2]["totals"]
    planes, mus, scales, payloads = np.tile([0.0, 0.0, 1.0, 0.0], (6, 1)), np.full((6, 4), 0.7), np.ones((6, abi.NBODY)), np.zeros((6, abi.HB_PAYLOAD_SIZE))
    for i in (4, 5):
        tw = sc.draw(scfg, cfg.instance_offset + i, 1, run["q_spawn"][i, 0:2], GROUND_Z, _model_of(run["steps"][0]["before"], 0), np.zeros(14), None)
        planes[i], mus[i], scales[i], payloads[i] = tw["plane"], tw["scen"][2:6], tw["scale"], tw["payload"]
    s = _solver(params, 6)
    try:
        s.plant_reset(tot["q_last"], tot["v_last"], eps=te.EPS)
        s.plant_set_contact_model(abi.make_contact_config(params, mu=MU0, ground_z=GROUND_Z, erp=te.ERP, sweeps=te.SWEEPS))
        if joints:
            s.plant_set_joint_model(abi.make_joint_model(params))
        s.plant_set_terrain(planes, mus)
        s.plant_set_model_variation(scales, payloads)
        ter, mod = s.plant_get_terrain(), s.plant_model_variation()
        a = run["steps"][2]["after"]
        for i in (4, 5):                          # the records the device drew are the ones the host setters store
            for k in ter:
                assert np.array_equal(ter[k][i], a["t_" + k][i]), (i, k)
            for k in mod:
                assert np.array_equal(mod[k][i], a["m_" + k][i]), (i, k)
        flags = np.ones((6, 4), dtype=np.int32)
        keys = set()
        for tick in (3, 4, 5):
            s.plant_step_hybrid(_command(s, run["scen"], tick), flags, te.DT, te.SUBSTEPS)
            got = _getters_twin(s)
            want = run["steps"][tick]["before"]
            for k, x in got.items():
                for i in (4, 5):
                    assert np.array_equal(x[i], want[k][i]), (joints, tick, i, k, np.abs(np.asarray(x[i], dtype=float) - want[k][i]).max())
                keys.add(k)
        assert {"q", "v", "lam", "c_gap", "c_point_vel", "c_residual", "c_touching", "c_status", "j_tau_applied"} <= keys
        assert np.isfinite(run["steps"][5]["before"]["q"]).all() and not np.array_equal(run["steps"][5]["before"]["q"][4:6], tot["q_last"][4:6])
        if not joints:
            assert not run["steps"][5]["before"]["j_tau_applied"].any()
    finally:
        s.close()


def _getters_twin(s):
    out = dict(s.plant_state())
    out.update({"c_" + k: a for k, a in s.plant_contact().items()})
    out.update({"j_" + k: a for k, a in s.plant_get_joints().items()})
    out.update({"a_" + k: a for k, a in s.plant_get_actuator().items()})
    return out


# ---- test 4 --------------------------------------------------------------------------------------------------------------------------------
def test_push_is_the_hosts_wrench(runs, params):
    from hunter_bipedal_control_amd.solver import HunterHipError
    push = dict(channels=abi.HB_SC_PUSH, push_force_max=5.0, push_start_lo=1, push_start_hi=1, push_ticks=2, seed=77)
    dev = _run(params, dict(RESPAWN, max_ticks=5), push)
    host = _run(params, dict(RESPAWN, max_ticks=5), None, host_push=abi.make_scenario_config(**push))
    pushed = 0
    for tick in range(NSTEPS):
        for part in ("before", "after"):
            for k, want in host["steps"][tick][part].items():
                assert np.array_equal(dev["steps"][tick][part][k], want), (tick, part, k)
        w = host["steps"][tick]["wrench"]
        steps_before = host["steps"][tick - 1]["after"]["e_STEPS"] if tick else np.zeros(6, dtype=int)
        episodes = host["steps"][tick - 1]["totals"]["EPISODES"] if tick else np.zeros(6, dtype=int)
        for i in range(6):                       # the host pushed on exactly the steps 1 and 2 of every episode but the first
            on = episodes[i] > 0 and 1 <= steps_before[i] < 3
            assert bool(w[i, 0:2].all()) == on and not w[i, 2:].any() and np.abs(w[i]).max() <= 5.0, (tick, i, w[i])
            assert not on or np.array_equal(w[i, 0:2], dev["steps"][tick - 1]["after"]["scen"][i, 22:24])
            pushed += on
    assert pushed >= 8
    # ... and the push did something: the same run without it is somewhere else afterwards
    assert not np.array_equal(dev["steps"][-1]["before"]["q"], runs["timeout0"]["steps"][-1]["before"]["q"])
    s = _solver(params, 2)
    try:
        _minimal(s, params)
        s.plant_set_scenario(abi.make_scenario_config(**push))
        with pytest.raises(HunterHipError, match=r"\(-3\).*owns the wrench"):
            s.plant_set_external_wrench(np.zeros((2, 6)))
        s.plant_set_scenario(None)
        s.plant_set_external_wrench(np.zeros((2, 6)))
    finally:
        s.close()


def _minimal(s, params, respawn=True):
    from hunter_bipedal_control_amd.rollout import standing_configuration
    q0 = standing_configuration(params, s.B, s)
    s.plant_reset(q0)
    s.plant_set_contact_model(abi.make_contact_config(params))
    s.plant_set_episode(abi.make_episode_config())
    if respawn:
        s.plant_set_respawn(abi.make_respawn_config(max_ticks=1), q0)
    return q0


# ---- test 5 --------------------------------------------------------------------------------------------------------------------------------
def test_reproducible_and_a_shard_draws_the_scenarios_of_its_slice(runs, params):
    again = _run(params, dict(RESPAWN, max_ticks=5), SCENARIO)
    for tick in range(NSTEPS):
        for part in ("before", "after"):
            for k, want in runs["timeout"]["steps"][tick][part].items():
                assert np.array_equal(again["steps"][tick][part][k], want), (tick, part, k)
    shard = _run(params, dict(RESPAWN, max_ticks=5, instance_offset=RESPAWN["instance_offset"] + 4), SCENARIO, rows=slice(4, 6))
    drawn = 0
    for tick in range(NSTEPS):
        whole = runs["timeout"]["steps"][tick]["after"]
        assert np.array_equal(shard["steps"][tick]["after"]["scen"], whole["scen"][4:6]), tick
        assert np.array_equal(shard["steps"][tick]["totals"]["EPISODE_INDEX"], runs["timeout"]["steps"][tick]["totals"]["EPISODE_INDEX"][4:6])
        drawn = max(drawn, int(shard["steps"][tick]["totals"]["EPISODE_INDEX"].min()))
    assert drawn >= 2 and shard["steps"][-1]["after"]["scen"].all(axis=1).all()


# ---- test 6 --------------------------------------------------------------------------------------------------------------------------------
def test_every_channel_off_is_the_run_without_a_scenario(runs, params):
    off = _run(params, dict(RESPAWN, max_ticks=5), dict(channels=0, log_capacity=0, seed=5))
    for tick in range(NSTEPS):
        for part in ("before", "after"):
            for k, want in runs["timeout0"]["steps"][tick][part].items():
                assert np.array_equal(off["steps"][tick][part][k], want), (tick, part, k)
            g = off["steps"][tick][part]
            assert not np.delete(g["scen"], 21, axis=1).any() and not g["count"].any() and g["log"].shape == (6, 0, abi.HB_SC_LOG_W)
    assert off["steps"][-1]["totals"]["EPISODES"].min() >= 2


# ---- test 7 --------------------------------------------------------------------------------------------------------------------------------
def test_closed_loop_log_and_table(params):
    from hunter_bipedal_control_amd.rollout import ResidentLoop, scenario_table
    every, max_ticks = 8, 40
    n = 17 * every                               # (the tick count of the closed-loop test of tests/test_gpu_respawn.py)
    fields = dict(channels=abi.HB_SC_SLOPE | abi.HB_SC_MU | abi.HB_SC_PAYLOAD, grade_max=0.03, mu_lo=0.05, mu_hi=0.8, payload_mass_max=0.5,
                  payload_center=(0.0, 0.0, 0.1), payload_half_extent=(0.02, 0.02, 0.0), seed=2024, log_capacity=2)
    s = _solver(params, 4)
    try:
        loop = ResidentLoop(s, params, ["stance", "trot", "stance", "trot"], np.array([[0.0] * 4, [0.2, 0, 0, 0], [0.0] * 4, [0.3, 0, 0, 0]]), mpc_every=every,
                            contact_config={}, episode=dict(tilt_limit=TILT), respawn=dict(max_ticks=max_ticks, place=1, instance_offset=3),
                            scenario=fields)
        nominal = {k: a[0] for k, a in s.plant_model_variation().items()}
        q_spawn = s.plant_respawn_totals(want_state=True)["q_last"]
        ground_z, mu0 = abi.make_contact_config(params).ground_z, abi.make_contact_config(params).mu
        loop.run(n)
        tot, rec, log, scen = loop.respawn_totals(), loop.episode(), loop.scenario_log(), loop.scenario()
        print({k: a.tolist() for k, a in tot.items()}, "count", log["count"].tolist())
        assert (tot["EPISODES"] >= 2).all()
        assert np.array_equal(log["count"], np.minimum(tot["EPISODES"], 2))
        assert np.array_equal(tot["N_FALLEN"] + tot["N_NONFINITE"] + tot["N_TIMEOUT"], tot["EPISODES"]) and np.array_equal(tot["EPISODE_INDEX"], tot["EPISODES"])
        assert (tot["STEPS_SUM"] + rec["STEPS"] == n).all()
        cfg = abi.make_scenario_config(**fields)
        level = np.concatenate([np.eye(3).reshape(9), [ground_z], [mu0] * 4])
        for i in range(4):
            assert np.array_equal(log["log"][i, 0, 6:], sc.init_row()[0]) and log["log"][i, 0, 0] == 0.0 and log["log"][i, 1, 0] == 1.0
            tw = sc.draw(cfg, 3 + i, 1, q_spawn[i, 0:2], ground_z, nominal, level, nominal)
            assert np.array_equal(log["log"][i, 1, 6:], tw["scen"]), (i, log["log"][i, 1, 6:] - tw["scen"])
            now = sc.draw(cfg, 3 + i, int(tot["EPISODES"][i]), q_spawn[i, 0:2], ground_z, nominal, level, nominal)
            assert np.array_equal(scen[i], now["scen"]), i
        table = scenario_table(log)
        assert len(table["EPISODE"]) == int(log["count"].sum()) == 8 and table["INSTANCE"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
        assert table["EPISODE"].tolist() == [0, 1] * 4 and table["MUS"].shape == (8, 4) and table["SCALE"].shape == (8, abi.NBODY)
        assert (table["TICKS"] > 0).all() and set(table["CAUSE"].tolist()) <= {abi.HB_EP_FALLEN, abi.HB_EP_NONFINITE, abi.HB_RS_TIMEOUT}
        assert np.array_equal(table["MUS"][1::2, 0], log["log"][:, 1, 6 + 2]) and (table["MUS"][1::2] >= 0.05).all() and (table["MUS"][1::2] <= 0.8).all()
        with pytest.raises(ValueError):
            ResidentLoop(s, params, ["stance"] * 4, np.zeros((4, 4)), contact_config={}, episode={}, scenario=fields)      # needs respawn=
    finally:
        s.close()


# ---- test 8 --------------------------------------------------------------------------------------------------------------------------------
def test_error_surface(params):
    from hunter_bipedal_control_amd.rollout import standing_configuration
    from hunter_bipedal_control_amd.solver import HunterHipError
    s = _solver(params, 2)
    try:
        cfg = abi.make_scenario_config(channels=abi.HB_SC_ALL, grade_max=0.1, mu_lo=0.1, mu_hi=0.5, payload_mass_max=1.0, payload_center=(0.01, 0.01, 0.1),
                                       mass_scale_range=0.1, push_force_max=1.0, push_start_lo=1, push_start_hi=2, push_ticks=1, log_capacity=1)
        q0 = standing_configuration(params, 2, s)
        with pytest.raises(HunterHipError, match=r"\(-3\)"):               # before hb_plant_reset
            s.plant_set_scenario(cfg)
        for call in (s.plant_scenario, s.plant_scenario_log):
            with pytest.raises(HunterHipError, match=r"\(-3\)"):           # no scenario in force
                call()
        s.plant_set_scenario(None)                                          # off is off, anywhere
        s.plant_reset(q0)
        s.plant_set_episode(abi.make_episode_config())
        s.plant_set_respawn(abi.make_respawn_config(max_ticks=1), q0)
        with pytest.raises(HunterHipError, match=r"\(-3\).*ground-contact"):     # outside contact model 1
            s.plant_set_scenario(cfg)
        s.plant_set_respawn(None)
        s.plant_set_contact_model(abi.make_contact_config(params))
        with pytest.raises(HunterHipError, match=r"\(-3\).*respawn"):      # no respawn configuration in force
            s.plant_set_scenario(cfg)
        s.plant_set_respawn(abi.make_respawn_config(max_ticks=1), q0)
        s.plant_set_scenario(cfg)
        assert np.array_equal(s.plant_scenario(), np.tile(sc.init_row()[0], (2, 1))) and not s.plant_scenario_log()["count"].any()
        for bad in (dict(grade_max=1.5), dict(mu_lo=0.5, mu_hi=0.4), dict(mass_scale_range=1.0), dict(push_force_max=float("nan")), dict(log_capacity=-1),
                    dict(channels=64), dict(channels=abi.HB_SC_PUSH, push_ticks=0)):
            with pytest.raises(HunterHipError, match=r"\(-1\).*kept"):
                s.plant_set_scenario(abi.make_scenario_config(**bad))
        flags, tau = np.ones((2, 4), dtype=np.int32), np.zeros((2, 10))
        s.plant_step(tau, flags, 0.002, 4)
        s.plant_respawn()                                                   # the configuration in force is kept: everybody draws
        assert s.plant_scenario().all(axis=1).all() and s.plant_scenario_log()["count"].tolist() == [1, 1]
        with pytest.raises(HunterHipError, match=r"\(-3\).*scenario in force"):
            s.plant_set_terrain(None, None)
        with pytest.raises(HunterHipError, match=r"\(-3\).*scenario in force"):
            s.plant_set_model_variation(None, None)
        drawn = s.plant_get_terrain()
        s.plant_reset(q0)                                                   # the log is empty again, terrain and scen stay as last drawn
        assert not s.plant_scenario_log()["count"].any() and not s.plant_scenario_log()["log"].any() and s.plant_scenario().all(axis=1).all()
        assert all(np.array_equal(a, drawn[k]) for k, a in s.plant_get_terrain().items())
        s.plant_set_scenario(None)                                          # off: the records stay in force, the host image follows the device
        assert all(np.array_equal(a, drawn[k]) for k, a in s.plant_get_terrain().items()) and not np.array_equal(drawn["plane"][0], [0.0, 0.0, 1.0, 0.0])
        s.plant_set_scenario(cfg)
        s.plant_set_respawn(None)                                           # turning respawn off turns the scenario off
        with pytest.raises(HunterHipError, match=r"\(-3\)"):
            s.plant_scenario()
        s.plant_set_respawn(abi.make_respawn_config(max_ticks=1), q0)
        s.plant_set_scenario(cfg)
        s.plant_set_episode(None)                                           # ... and so does turning the episode off
        with pytest.raises(HunterHipError, match=r"\(-3\)"):
            s.plant_scenario()
        s.plant_set_episode(abi.make_episode_config())
        s.plant_set_respawn(abi.make_respawn_config(max_ticks=1), q0)
        s.plant_set_scenario(cfg)
        s.plant_set_contact_model(None)                                     # leaving model 1 turns the scenario off
        with pytest.raises(HunterHipError, match=r"\(-3\)"):
            s.plant_scenario()
        s.plant_set_contact_model(abi.make_contact_config(params))
        with pytest.raises(HunterHipError, match=r"\(-3\)"):
            s.plant_scenario()
        s.plant_set_external_wrench(np.zeros((2, 6)))                       # the wrench is the caller's again
    finally:
        s.close()


# ---- test 9 --------------------------------------------------------------------------------------------------------------------------------
def test_a_smaller_log_in_a_larger_allocation(params):
    """log_capacity 3 and then 2 in one context (the device rows keep the pitch of 3) against a fresh context with 2 alone: the draw is
    stateless per seed, instance and episode, so count and log are equal array for array."""
    logs = []
    for capacities in ((3, 2), (2,)):
        s = _solver(params, 3)
        try:
            _minimal(s, params)
            for cap in capacities:
                s.plant_set_scenario(abi.make_scenario_config(**dict(SCENARIO, log_capacity=cap)))
            flags, tau = np.ones((3, 4), dtype=np.int32), np.zeros((3, 10))
            for _ in range(3):                                              # max_ticks = 1: every instance ends an episode with every tick
                s.plant_step(tau, flags, 0.002, 4)
                s.plant_respawn()
            logs.append(s.plant_scenario_log())
        finally:
            s.close()
    grown, fresh = logs
    assert grown["log"].shape == fresh["log"].shape == (3, 2, abi.HB_SC_LOG_W)
    assert fresh["count"].tolist() == [2] * 3 and fresh["log"][:, :, 0].tolist() == [[0.0, 1.0]] * 3
    assert np.array_equal(grown["count"], fresh["count"]) and np.array_equal(grown["log"], fresh["log"])
