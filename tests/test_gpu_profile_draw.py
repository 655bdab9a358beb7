"""Profile draw at respawn on the device (hb_plant_set_profile_draw / hb_plant_get_profile_draw / hb_plant_get_profile_draw_log;
k_plant_profile_draw and the profile path of k_plant_respawn) against the exact twin of the definition (tests/_profiledrawemu.py), against
the device's own getters, and against exact twins on the device: a fresh context given the drawn knots through the host setters (the drawn
records are the host's, bit for bit) and a context with the same respawn and no ground feature (a level draw changes nothing).  The draw
has no transcendental function in it, so every comparison of a drawn quantity is ==; what goes through the leg kinematics (the placed
state) is held to the 1e-10 tests/test_gpu_respawn.py holds a placed state on a plane to, the drawn spawn state to its 1e-12."""
import numpy as np
import pytest

import _profiledrawemu as pd
import _respawnemu as rs
from hunter_bipedal_control_amd import abi

pytestmark = pytest.mark.gpu

B = 8
MU0, DT, SUBSTEPS, TOL_Q = 0.31, 0.002, 4, 1e-10
OFFSET = 0xFFFFFFFA                    # the global instance index wraps inside the batch
RESPAWN = dict(hold_ticks=0, max_ticks=1, place=1, clearance=0.002, yaw_range=0.3, joint_pos_sigma=0.01, base_vel_sigma=0.05, seed=0xABCDEF0123,
               instance_offset=OFFSET)
KMAX = abi.HB_PROFILE_MAX_KNOTS
EPISODE = abi.make_episode_config(tilt_limit=0.2)


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


def _start(params, s, batch):
    """-> (q0, ground_z): the standing configuration, the instances apart in x and y so that every s0 is another."""
    from hunter_bipedal_control_amd.rollout import lowest_contact_point, standing_configuration
    q0 = standing_configuration(params, batch, s)
    q0[:, 0] += 0.37 * np.arange(batch) - 1.0
    q0[:, 1] += 0.11 * np.arange(batch)
    return q0, lowest_contact_point(s, q0)


def _open(params, batch, respawn, draw=None, follow=False, joints=False, q_tilt=()):
    """A context in contact model 1 with an episode, the respawn configuration and, if given, the draw (with `follow`, behind the zero map)."""
    s = _solver(params, batch)
    q0, gz = _start(params, s, batch)
    q_spawn = q0.copy()
    for i in q_tilt:
        q0[i, 5] = 0.3
    s.plant_reset(q0)
    s.plant_set_contact_model(abi.make_contact_config(params, mu=MU0, ground_z=gz))
    if joints:
        s.plant_set_joint_model(abi.make_joint_model(params))
    s.plant_set_episode(EPISODE)
    rcfg = abi.make_respawn_config(**respawn)
    v_spawn = np.zeros((batch, 16))
    v_spawn[:, 0] = 0.01 * np.arange(batch)
    s.plant_set_respawn(rcfg, q_spawn, v_spawn)
    cfg = None
    if draw is not None:
        cfg = abi.make_profile_draw_config(**dict(draw, follow_map=1 if follow else 0))
        if follow:
            s.ground_set_profile(np.full(batch, 2), np.tile(np.array(cfg.dir[:]), (batch, 1)), np.tile([[-1.0, 0.0], [1.0, 0.0]], (batch, 1, 1)))
        s.plant_set_profile_draw(cfg)
    return s, dict(q0=q0, gz=gz, q_spawn=q_spawn, v_spawn=v_spawn, rcfg=rcfg, cfg=cfg)


def _episode_of(ep, i):
    return {k: a[i] for k, a in ep.items() if k != "trace"}


def _state(s, draw=True, ground=False):
    out = dict(s.plant_state())
    out.update({"c_" + k: a for k, a in s.plant_contact().items()})
    out.update({"e_" + k: a for k, a in s.plant_episode().items()})
    if draw:
        out.update({"p_" + k: a for k, a in s.plant_get_terrain_profile().items()})
        log = s.plant_profile_draw_log()
        out.update(row=s.plant_profile_draw(), log=log["log"], count=log["count"])
    if ground:
        out.update({"g_" + k: a for k, a in s.ground_get_profile().items()})
    return out


# ---- the draw, the records, the placed state, the log ------------------------------------------------------------------------------------------
def _draw_run(params, name, rounds=3):
    """max_ticks = 1: every instance times out with its first tick, so each of `rounds` respawns redraws the whole batch."""
    s, ctx = _open(params, B, RESPAWN, pd.CONFIGS[name], follow=True)
    try:
        tau, flags = np.zeros((B, 10)), np.ones((B, 4), dtype=np.int32)
        steps = [dict(after=_state(s, ground=True))]                         # the state of the set call: level ground, rows zero
        for _ in range(rounds):
            s.plant_step(tau, flags, DT, SUBSTEPS)
            before = _state(s, ground=True)
            s.plant_respawn()
            steps.append(dict(before=before, after=_state(s, ground=True), totals=s.plant_respawn_totals(want_state=True)))
        # ProfileBatch::base has no getter: the record hb_plant_set_episode starts right after the last respawn is measured against it
        s.plant_set_episode(EPISODE)
        return dict(ctx, steps=steps, reinit=s.plant_episode())
    finally:
        s.close()


@pytest.fixture(scope="module")
def draw_runs(params):
    """Shared, left unchanged: three rounds under every kind with a direction not of unit length, and under curbs and stairs alone."""
    return {name: _draw_run(params, name) for name in ("gpu_draw", "gpu_steps")}


def test_rows_knots_records_map_and_log_are_the_twins(draw_runs, params):
    """B = 8, instance_offset 0xFFFFFFFA, max_ticks = 1, three respawns.  Parameter rows and knots == the twin; the records of
    hb_plant_get_terrain_profile == those of a second context given the twin's knots through hb_plant_set_terrain_profile, the map of
    hb_ground_get_profile == that of the second context given the relative knots through hb_ground_set_profile; log rows == the twin."""
    kinds = set()
    s2, _ = _open(params, B, RESPAWN)
    try:
        s2.plant_set_respawn(None)                                           # (the frozen rule: no profile next to a respawn configuration)
        for name, run in draw_runs.items():
            cfg, gz = run["cfg"], run["gz"]
            a = np.array(pd.direction(cfg))
            first = run["steps"][0]["after"]
            assert not first["row"].any() and not first["count"].any() and (first["p_n_knots"] == 2).all() and (first["p_mu"] == MU0).all()
            for i in range(B):
                assert np.array_equal(first["p_knots"][i], pd.padded(pd.flat(cfg, run["q_spawn"][i], gz)[1]))
            logged = [[] for _ in range(B)]
            for e, step in enumerate(run["steps"][1:], start=1):
                bfr, aft = step["before"], step["after"]
                assert (step["totals"]["EPISODE_INDEX"] == e).all()
                tw = [pd.draw(cfg, OFFSET + i, e, run["q_spawn"][i], gz) for i in range(B)]
                kinds |= {t["kind"] for t in tw}
                nk = np.array([len(t["knots"]) for t in tw], dtype=np.int32)
                knots, rel = np.array([pd.padded(t["knots"]) for t in tw]), np.array([pd.padded(t["rel"]) for t in tw])
                assert np.array_equal(aft["row"], np.array([t["row"] for t in tw])), (name, e)
                assert np.array_equal(aft["p_n_knots"], nk) and np.array_equal(aft["p_knots"], knots) and np.array_equal(aft["p_mu"], np.array([t["mu"] for t in tw]))
                assert np.array_equal(aft["p_dir"], np.tile(a, (B, 1)))
                dirs = np.tile(np.array(cfg.dir[:]), (B, 1))                  # (as given: the setter normalises by the same division)
                s2.plant_set_terrain_profile(nk, dirs, knots, np.array([t["mu"] for t in tw]))
                want = s2.plant_get_terrain_profile()
                for k in ("n_knots", "dir", "knots", "mu", "records"):
                    assert np.array_equal(aft["p_" + k], want[k]), (name, e, k)
                s2.ground_set_profile(nk, dirs, rel)
                wantg = s2.ground_get_profile()
                for k in ("n_knots", "dir", "knots", "slopes"):
                    assert np.array_equal(aft["g_" + k], wantg[k]), (name, e, k)
                for i in range(B):
                    cause = rs.decide(run["rcfg"], _episode_of({k[2:]: v for k, v in bfr.items() if k.startswith("e_")}, i))
                    assert cause == abi.HB_RS_TIMEOUT
                    if len(logged[i]) < cfg.log_capacity:
                        logged[i].append(pd.log_row(e - 1, cause, _episode_of({k[2:]: v for k, v in bfr.items() if k.startswith("e_")}, i), bfr["row"][i], a))
                    assert aft["count"][i] == len(logged[i]) and np.array_equal(aft["log"][i, :len(logged[i])], np.array(logged[i])), (name, e, i)
                    assert not aft["log"][i, len(logged[i]):].any()
    finally:
        s2.close()
    assert kinds == {abi.HB_PD_FLAT, abi.HB_PD_CURB, abi.HB_PD_STAIRS}


def test_placed_state_segments_and_the_new_record(draw_runs, params):
    """On every drawn ground (level, curbs, stairs): the spawned state against the twin's draw (1e-12) and vertical placement (1e-10), the
    lowest gap over the facets of the returned records == clearance (1e-10) and no point below it; `segment` == the twin's locate with the
    device kinematics; the new episode record measures its height against the facet under the base origin, exactly."""
    s = _solver(params, 1)
    try:
        foot_fn = _foot_fn(s)
        straddled = off_level = 0
        for name, run in draw_runs.items():
            cfg, rcfg, gz = run["cfg"], run["rcfg"], run["gz"]
            a = np.array(pd.direction(cfg))
            for e, step in enumerate(run["steps"][1:], start=1):
                aft, tot = step["after"], step["totals"]
                for i in range(B):
                    tw = pd.draw(cfg, OFFSET + i, e, run["q_spawn"][i], gz)
                    qd, vd = rs.spawn_state(rcfg, OFFSET + i, e, run["q_spawn"][i], run["v_spawn"][i])
                    qt = pd.place(rcfg, qd, foot_fn, a, tw["knots"])
                    ql, vl = tot["q_last"][i], tot["v_last"][i]
                    assert np.array_equal(aft["q"][i], ql) and np.array_equal(aft["v"][i], vl)
                    assert np.abs(ql[3:] - qt[3:]).max() <= rs.NORMAL_TOL and np.abs(vl - vd).max() <= rs.NORMAL_TOL, (name, e, i)
                    assert np.abs(ql[:3] - qt[:3]).max() <= TOL_Q, (name, e, i, ql[:3] - qt[:3])
                    seg = aft["p_segment"][i]
                    assert seg.tolist() == pd.locate(a, tw["knots"], ql, foot_fn).tolist(), (name, e, i)
                    feet = np.asarray(foot_fn(ql[None]))[0].reshape(4, 3)
                    recs = aft["p_records"][i]
                    gaps = np.array([recs[seg[c]][[2, 5, 8]] @ feet[c] - recs[seg[c]][9] for c in range(4)])
                    assert abs(gaps.min() - rcfg.clearance) <= TOL_Q and (gaps >= rcfg.clearance - TOL_Q).all(), (name, e, i, gaps)
                    straddled += len(set(seg[:4].tolist())) > 1
                    r = recs[seg[4]]
                    want = rs.init_record(ql, np.array([r[2], r[5], r[8], r[9]]))
                    got = _episode_of({k[2:]: v for k, v in aft.items() if k.startswith("e_")}, i)
                    for field, _, _ in abi.EPISODE_INT_FIELDS + abi.EPISODE_DOUBLE_FIELDS:
                        assert np.array_equal(got[field], want[field]), (name, e, i, field, got[field], want[field])
            # the base record k_plant_respawn stored (the facet under the base origin of the placed state): the record that
            # k_plant_episode_init starts from it right after the last respawn == the initial record over the twin's base record, exactly
            e, last = len(run["steps"]) - 1, run["steps"][-1]
            for i in range(B):
                tw = pd.draw(cfg, OFFSET + i, e, run["q_spawn"][i], gz)
                ql = last["totals"]["q_last"][i]
                base = pd.base_record(a, tw["knots"], ql, last["after"]["p_records"][i], tw["mu"])
                off_level += int(pd.segment(a, tw["knots"], ql) != 0)
                want = rs.init_record(ql, base[[2, 5, 8, 9]])
                got = _episode_of(run["reinit"], i)
                for field, _, _ in abi.EPISODE_INT_FIELDS + abi.EPISODE_DOUBLE_FIELDS:
                    assert np.array_equal(got[field], want[field]), (name, "base", i, field, got[field], want[field])
        print("placed states whose contact points stand on more than one facet:", straddled, "; base origins beyond the first segment:", off_level)
        assert straddled > 0 and off_level > 0
    finally:
        s.close()


# ---- nobody else is touched ----------------------------------------------------------------------------------------------------------------------
def test_an_instance_that_stays_is_not_written(params):
    """B = 6, hold_ticks 2, no time-out: instances 4 and 5 start rolled beyond the tilt limit, end on step 0 and are put back after step 2;
    everybody else stays in every call.  Every array the getters return of an instance that stays — plant, contact, episode, profile
    record, knots, segment, draw row, log, map — is byte-identical across hb_plant_respawn; the two that respawn get a new ground."""
    s, ctx = _open(params, 6, dict(RESPAWN, hold_ticks=2, max_ticks=0), pd.CONFIGS["gpu_draw"], follow=True, q_tilt=(4, 5))
    try:
        tau, flags = np.zeros((6, 10)), np.ones((6, 4), dtype=np.int32)
        who, index = [], np.zeros(6, dtype=np.int32)
        for tick in range(4):
            s.plant_step(tau, flags, DT, SUBSTEPS)
            bfr = _state(s, ground=True)
            s.plant_respawn()
            aft, tot = _state(s, ground=True), s.plant_respawn_totals()
            moved = [i for i in range(6) if tot["EPISODE_INDEX"][i] != index[i]]
            who.append(moved)
            index = tot["EPISODE_INDEX"].copy()
            for i in range(6):
                if i in moved:
                    assert aft["row"][i, 0] in (1.0, 2.0, 4.0) and aft["count"][i] == 1
                    continue
                for k in bfr:
                    assert np.asarray(aft[k][i]).tobytes() == np.asarray(bfr[k][i]).tobytes(), (tick, i, k)
        assert who == [[], [], [4, 5], []]
    finally:
        s.close()
    # ProfileBatch::base has no getter.  Two contexts run the same three steps; one of them calls hb_plant_respawn after the third (4 and 5
    # are put back), then both restart the episode record, which k_plant_episode_init measures against `base`: the records of the four
    # that stay are the same bits with and without the call, those of the two that moved start over the base record of their new ground.
    recs = {}
    for call in (True, False):
        s, ctx = _open(params, 6, dict(RESPAWN, hold_ticks=2, max_ticks=0), pd.CONFIGS["gpu_steps"], follow=True, q_tilt=(4, 5))
        try:
            for tick in range(3):
                s.plant_step(tau, flags, DT, SUBSTEPS)
                if call or tick < 2:
                    s.plant_respawn()
            q, prof = s.plant_state()["q"], s.plant_get_terrain_profile()
            s.plant_set_episode(EPISODE)
            recs[call] = dict(ep=s.plant_episode(), q=q, prof=prof, cfg=ctx["cfg"], q_spawn=ctx["q_spawn"], gz=ctx["gz"])
        finally:
            s.close()
    for i in range(4):
        for k in recs[True]["ep"]:
            assert np.asarray(recs[True]["ep"][k][i]).tobytes() == np.asarray(recs[False]["ep"][k][i]).tobytes(), (i, k)
    r = recs[True]
    a = np.array(pd.direction(r["cfg"]))
    for i in (4, 5):
        tw = pd.draw(r["cfg"], OFFSET + i, 1, r["q_spawn"][i], r["gz"])
        base = pd.base_record(a, tw["knots"], r["q"][i], r["prof"]["records"][i], tw["mu"])
        want, got = rs.init_record(r["q"][i], base[[2, 5, 8, 9]]), _episode_of(r["ep"], i)
        for field, _, _ in abi.EPISODE_INT_FIELDS + abi.EPISODE_DOUBLE_FIELDS:
            assert np.array_equal(got[field], want[field]), (i, field, got[field], want[field])
        assert not np.array_equal(recs[False]["ep"]["HEIGHT_LAST"][i], got["HEIGHT_LAST"])


# ---- a level draw changes nothing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("joints", [False, True])
@pytest.mark.parametrize("hybrid", [False, True])
def test_flat_draw_is_the_run_without_a_ground_feature(params, joints, hybrid):
    """kinds = HB_PD_FLAT, mu_lo = mu_hi = cfg.mu, 12 plant ticks with max_ticks = 5 (two respawns of everybody): q, v, lambda, the
    episode records, the totals and q_last == those of a context with the same respawn and no ground feature, bit for bit."""
    flat = dict(pd.CONFIGS["gpu_draw"], kinds=abi.HB_PD_FLAT, mu_lo=MU0, mu_hi=MU0)
    runs = []
    for draw in (flat, None):
        s, ctx = _open(params, 4, dict(RESPAWN, max_ticks=5), draw, joints=joints)
        try:
            flags, out = np.ones((4, 4), dtype=np.int32), []
            qj = ctx["q0"][:, 6:].copy()
            for tick in range(12):
                tau = 0.3 * np.sin(0.7 * tick + np.arange(10))[None, :] * np.ones((4, 1))
                if hybrid:
                    s.plant_step_hybrid(dict(pos_des=qj, vel_des=np.zeros((4, 10)), kp=np.full((4, 10), 40.0), kd=np.full((4, 10), 1.0), tau_ff=tau), flags, DT, SUBSTEPS)
                else:
                    s.plant_step(tau, flags, DT, SUBSTEPS)
                s.plant_respawn()
                st = _state(s, draw=False)
                st.update({"t_" + k: v for k, v in s.plant_respawn_totals(want_state=True).items()})
                out.append(st)
            runs.append(out)
        finally:
            s.close()
    assert (runs[0][-1]["t_EPISODES"] >= 2).all()
    for tick in range(12):
        for k, want in runs[1][tick].items():
            assert np.array_equal(runs[0][tick][k], want, equal_nan=True), (tick, k)


# ---- states ------------------------------------------------------------------------------------------------------------------------------------
def test_api_behaviour(params):
    """Every state refusal, in both orders where there are two; the two frozen refusals; the getters without a draw; what survives
    hb_plant_reset; the off-rules."""
    from hunter_bipedal_control_amd.solver import HunterHipError
    state, arg = r"\(-3\)", r"\(-1\)"
    draw = dict(pd.CONFIGS["gpu_draw"])
    cfg = abi.make_profile_draw_config(**draw)
    s = _solver(params, 4)
    try:
        q0, gz = _start(params, s, 4)
        tau, flags = np.zeros((4, 10)), np.ones((4, 4), dtype=np.int32)
        zero_map = (np.full(4, 2), np.tile(np.array(cfg.dir[:]), (4, 1)), np.tile([[-1.0, 0.0], [1.0, 0.0]], (4, 1, 1)))
        s.plant_set_profile_draw(None)                                       # off while off: nothing to do, anywhere
        for call in (lambda: s.plant_set_profile_draw(cfg), s.plant_profile_draw, s.plant_profile_draw_log):
            with pytest.raises(HunterHipError, match=state):                 # before hb_plant_reset
                call()
        s.plant_reset(q0)
        with pytest.raises(HunterHipError, match=state):                     # outside contact model 1
            s.plant_set_profile_draw(cfg)
        s.plant_set_contact_model(abi.make_contact_config(params, mu=MU0, ground_z=gz))
        s.plant_set_episode(abi.make_episode_config(tilt_limit=0.2))
        with pytest.raises(HunterHipError, match=state + ".*respawn"):       # without a respawn configuration
            s.plant_set_profile_draw(cfg)
        rcfg = abi.make_respawn_config(**RESPAWN)
        s.plant_set_respawn(rcfg, q0)
        for call in (s.plant_profile_draw, s.plant_profile_draw_log):
            with pytest.raises(HunterHipError, match=state):                 # the getters while the draw is off
                call()
        with pytest.raises(HunterHipError, match=arg + ".*riser_slope.*kept"):
            s.plant_set_profile_draw(abi.make_profile_draw_config(**dict(draw, riser_slope=1.74)))
        with pytest.raises(HunterHipError, match=state + ".*follow_map"):    # follow_map without a map: the caller sets the zero map first
            s.plant_set_profile_draw(abi.make_profile_draw_config(**dict(draw, follow_map=1)))
        far = q0.copy()
        far[2, 0] = 2000.0
        s.plant_set_respawn(rcfg, far)
        with pytest.raises(HunterHipError, match=state + ".*instance 2"):    # a spawn point outside the reach of the validity argument
            s.plant_set_profile_draw(cfg)
        s.plant_set_respawn(rcfg, q0)
        # a scenario with the slope or the friction channel, in both orders; the other channels combine freely
        s.plant_set_scenario(abi.make_scenario_config(channels=abi.HB_SC_MU, mu_lo=0.2, mu_hi=0.5))
        with pytest.raises(HunterHipError, match=state + ".*scenario"):
            s.plant_set_profile_draw(cfg)
        s.plant_set_scenario(None)
        s.plant_set_profile_draw(cfg)                                        # (replaces the terrain the scenario had turned on)
        for ch in (abi.HB_SC_SLOPE, abi.HB_SC_MU):
            with pytest.raises(HunterHipError, match=state):
                s.plant_set_scenario(abi.make_scenario_config(channels=ch, grade_max=0.1, mu_lo=0.2, mu_hi=0.5))
        s.plant_set_scenario(abi.make_scenario_config(channels=abi.HB_SC_PAYLOAD | abi.HB_SC_MASS | abi.HB_SC_PUSH, payload_mass_max=1.0, mass_scale_range=0.1,
                                                      push_force_max=5.0, push_start_lo=1, push_start_hi=2, push_ticks=1))
        s.plant_set_scenario(None)
        # while the draw is in force
        assert not s.plant_profile_draw().any() and (s.plant_get_terrain_profile()["n_knots"] == 2).all()
        with pytest.raises(HunterHipError, match=state + ".*profile draw"):
            s.plant_set_terrain(np.tile([0.0, 0.0, 1.0, gz], (4, 1)), None)
        with pytest.raises(HunterHipError, match=state):
            s.plant_set_terrain(None, None)
        n2, k2 = np.full(4, 2), np.tile([[-1.0, gz], [1.0, gz]], (4, 1, 1))
        with pytest.raises(HunterHipError, match=state):                     # frozen: no profile of the host's next to respawn
            s.plant_set_terrain_profile(n2, zero_map[1], k2)
        with pytest.raises(HunterHipError, match=state + ".*profile draw"):  # nor may the host switch the drawn profile off
            s.plant_set_terrain_profile()
        assert (s.plant_get_terrain_profile()["n_knots"] == 2).all() and not s.plant_profile_draw().any()
        with pytest.raises(HunterHipError, match=state):                     # frozen: no respawn configuration next to a profile
            s.plant_set_respawn(rcfg, q0)
        with pytest.raises(HunterHipError, match=arg + ".*ground_z"):
            s.plant_set_contact_model(abi.make_contact_config(params, mu=MU0, ground_z=2000.0))
        # the map follows once it is there; a draw, then hb_plant_reset: records and rows stay, the log is empty
        s.ground_set_profile(*zero_map)
        s.plant_set_profile_draw(abi.make_profile_draw_config(**dict(draw, follow_map=1)))
        s.plant_step(tau, flags, DT, SUBSTEPS)
        s.plant_respawn()
        drawn, gmap, rows, log = s.plant_get_terrain_profile(), s.ground_get_profile(), s.plant_profile_draw(), s.plant_profile_draw_log()
        assert (rows[:, 0] > 0).all() and log["count"].tolist() == [1] * 4
        s.plant_reset(q0)
        after = s.plant_get_terrain_profile()
        for k in ("n_knots", "dir", "knots", "mu", "records"):
            assert np.array_equal(after[k], drawn[k]), k
        assert np.array_equal(s.plant_profile_draw(), rows) and not s.plant_profile_draw_log()["count"].any() and not s.plant_profile_draw_log()["log"].any()
        foot_fn = _foot_fn(s)
        a = np.array(pd.direction(cfg))
        # set again while in force with follow_map: plant and map go back to level ground together, rows and log restart
        s.plant_set_profile_draw(abi.make_profile_draw_config(**dict(draw, follow_map=1)))
        level, levelg = s.plant_get_terrain_profile(), s.ground_get_profile()
        assert (level["n_knots"] == 2).all() and (levelg["n_knots"] == 2).all() and not levelg["slopes"].any() and not levelg["knots"][:, :, 1].any()
        assert np.array_equal(levelg["knots"][:, :2, 0], level["knots"][:, :2, 0]) and np.array_equal(levelg["dir"], level["dir"])
        assert not s.plant_profile_draw().any() and not s.plant_profile_draw_log()["count"].any()
        s.plant_step(tau, flags, DT, SUBSTEPS)
        s.plant_respawn()
        drawn, gmap, rows = s.plant_get_terrain_profile(), s.ground_get_profile(), s.plant_profile_draw()
        s.plant_reset(q0)
        after = s.plant_get_terrain_profile()
        for i in range(4):                                                   # located at the reset state, on the drawn ground
            assert after["segment"][i].tolist() == pd.locate(a, drawn["knots"][i, :drawn["n_knots"][i]], q0[i], foot_fn).tolist()
        # off: profile and map stay in force as last drawn, respawn keeps placing on them, the getters of the draw are gone
        s.plant_set_profile_draw(None)
        for call in (s.plant_profile_draw, s.plant_profile_draw_log):
            with pytest.raises(HunterHipError, match=state):
                call()
        kept, keptg = s.plant_get_terrain_profile(), s.ground_get_profile()
        for k in ("n_knots", "dir", "knots", "mu", "records"):
            assert np.array_equal(kept[k], drawn[k]), k
        for k in gmap:
            assert np.array_equal(keptg[k], gmap[k]), k
        s.plant_step(tau, flags, DT, SUBSTEPS)
        s.plant_respawn()
        tot = s.plant_respawn_totals(want_state=True)
        assert (tot["EPISODES"] == 1).all()
        placed = s.plant_get_terrain_profile()
        assert np.array_equal(placed["records"], drawn["records"])
        for i in range(4):
            seg, feet = placed["segment"][i], np.asarray(foot_fn(tot["q_last"][i][None]))[0].reshape(4, 3)
            gaps = np.array([placed["records"][i][seg[c]][[2, 5, 8]] @ feet[c] - placed["records"][i][seg[c]][9] for c in range(4)])
            assert abs(gaps.min() - rcfg.clearance) <= TOL_Q
        # respawn off turns the draw off; so does the episode; so does leaving model 1 (and the profile with it)
        offs = (lambda: s.plant_set_respawn(None), lambda: s.plant_set_episode(None), lambda: s.plant_set_contact_model(None))
        for n, off in enumerate(offs):
            s.plant_set_terrain(None, None)                                  # (allowed again: the draw is off; the profile it left goes,
            s.plant_set_episode(abi.make_episode_config(tilt_limit=0.2))     #  so that respawn can come back)
            s.plant_set_respawn(rcfg, q0)
            s.plant_set_profile_draw(cfg)
            s.plant_profile_draw()
            off()
            with pytest.raises(HunterHipError, match=state):
                s.plant_profile_draw()
            if n < 2:
                assert (s.plant_get_terrain_profile()["n_knots"] == 2).all()  # the profile stays in force
        s.plant_set_contact_model(abi.make_contact_config(params, mu=MU0, ground_z=gz))
        with pytest.raises(HunterHipError, match=state):                     # leaving model 1 had switched the profile off too
            s.plant_get_terrain_profile()
    finally:
        s.close()


def test_a_smaller_log_in_a_larger_allocation(params):
    """log_capacity 3 and then 2 in one context (the device rows keep the pitch of 3) against a fresh context with 2 alone: the draw is
    stateless per seed, instance and episode, so count and log are equal array for array."""
    draw = pd.CONFIGS["gpu_draw"]
    logs = []
    for capacities in ((3, 2), (2,)):
        s, _ = _open(params, 3, RESPAWN, dict(draw, log_capacity=capacities[0]))
        try:
            for cap in capacities[1:]:
                s.plant_set_profile_draw(abi.make_profile_draw_config(**dict(draw, log_capacity=cap)))
            tau, flags = np.zeros((3, 10)), np.ones((3, 4), dtype=np.int32)
            for _ in range(3):                                               # max_ticks = 1: every instance ends an episode with every tick
                s.plant_step(tau, flags, DT, SUBSTEPS)
                s.plant_respawn()
            logs.append(s.plant_profile_draw_log())
        finally:
            s.close()
    grown, fresh = logs
    assert grown["log"].shape == fresh["log"].shape == (3, 2, abi.HB_PD_LOG_W)
    assert fresh["count"].tolist() == [2] * 3
    assert np.array_equal(grown["count"], fresh["count"]) and np.array_equal(grown["log"], fresh["log"])


# ---- the closed loop ----------------------------------------------------------------------------------------------------------------------------
LOOP_B, LOOP_TICKS, EVERY = 4, 30, 6


def _flat_offset(cfg, episodes, base=1000):
    """The first instance_offset from `base` on whose instance 1 and the shifted run's instance 0 draw level ground in every episode."""
    off = base
    while not all(pd.draw(cfg, off + 1, e, (0.0, 0.0), 0.0)["kind"] == abi.HB_PD_FLAT for e in range(1, episodes + 1)):
        off += 1
    return off


def _loop_run(params, respawn, draw):
    from hunter_bipedal_control_amd.rollout import ResidentLoop
    s = _solver(params, LOOP_B)
    try:
        loop = ResidentLoop(s, params, ["trot"] * LOOP_B, np.tile([0.2, 0.0, 0.0, 0.0], (LOOP_B, 1)), mpc_every=EVERY, contact_config={},
                            episode=dict(tilt_limit=0.3), respawn=respawn, profile_draw=draw, ground_map="draw" if draw is not None else None)
        loop.run(LOOP_TICKS)
        out = dict(s.plant_state())
        out.update({"e_" + k: a for k, a in loop.episode().items()})
        out.update({"t_" + k: a for k, a in loop.respawn_totals(want_state=True).items()})
        if draw is not None:
            log = loop.profile_draw_log()
            out.update(row=loop.profile_draw(), log=log["log"], count=log["count"], knots=s.plant_get_terrain_profile()["knots"],
                       gknots=s.ground_get_profile()["knots"])
        return out
    finally:
        s.close()


def test_closed_loop_is_reproducible_per_global_instance_and_level_ground_is_no_ground(params):
    """ResidentLoop(profile_draw=..., ground_map="draw"), B = 4, 30 ticks, max_ticks = 6 (a respawn of everybody at every MPC boundary).
    The run with instance_offset shifted by one gives its instance i what the first run gave instance i + 1 (the same global instance):
    rows, knots, map, log, state, record and totals, bit for bit.  The instance that draws level ground in every episode == the same
    instance of the same loop built without the draw."""
    draw = dict(pd.CONFIGS["gpu_loop"], mu_lo=params["config"]["friction_mu"], mu_hi=params["config"]["friction_mu"])
    cfg = abi.make_profile_draw_config(**draw)
    off = _flat_offset(cfg, LOOP_TICKS // EVERY)
    respawn = dict(hold_ticks=0, max_ticks=6, place=1, clearance=0.0, yaw_range=0.05, joint_pos_sigma=0.005, seed=77)
    first = _loop_run(params, dict(respawn, instance_offset=off), draw)
    shifted = _loop_run(params, dict(respawn, instance_offset=off + 1), draw)
    plain = _loop_run(params, dict(respawn, instance_offset=off), None)
    assert (first["t_EPISODES"] == LOOP_TICKS // EVERY).all() and (first["count"] == min(LOOP_TICKS // EVERY, cfg.log_capacity)).all()
    assert len({tuple(r) for r in first["row"].tolist()}) > 1               # not everybody on the same ground
    for k in first:
        assert np.array_equal(shifted[k][:-1], first[k][1:], equal_nan=True), k
    assert (first["log"][1, :first["count"][1], 5] == [0.0] + [float(abi.HB_PD_FLAT)] * (first["count"][1] - 1)).all() and first["row"][1, 0] == abi.HB_PD_FLAT
    for k in plain:
        assert np.array_equal(first[k][1], plain[k][1], equal_nan=True), k
