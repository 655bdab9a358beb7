"""-m gpu: the controller's FIELD map on the device (hb_ground_set_field; k_refgen_gfield, k_estimator_gfield, k_ground_field_eval) against
the host routine, against its numpy twin (tests/_groundfieldtwin.py), against contexts without a map, through the instance-range path and in
the closed loop.  The cases and the twin's tables are those of tests/test_groundfield_host.py, computed once.

Closed loop (test g), measured on an MI355X (pytest -s prints the figures): planes rising 0.03 along the walk with a cross slope of +0.015 /
-0.015 on a grid turned by atan(0.75) (blind robots fall from a rise of 0.04 on; item 20's downhill sweep lost them at
0.05), 2400 ticks.  Map height under the base at the end 2.91 / 2.88 cm; z estimate - z plant over the last 100 ticks: level robots +0.02441
(with the zero map and without one: the same bits), mapped +0.02566 / +0.02724, blind -0.00114 / -0.00105 — the blind filter has sunk by the
height climbed, the mapped one has not."""
import numpy as np
import pytest

import _groundfieldemu as gfe
import _groundfieldtwin as gft
import _groundtwin as gt
from _cmp import maxdiff_nan
from hunter_bipedal_control_amd import abi, workload
from oracle import refgen

pytestmark = pytest.mark.gpu
NMAX = gt.N + 8


def _solver(params, batch, max_nodes=NMAX, **kw):
    from hunter_bipedal_control_amd.solver import HunterSolver
    return HunterSolver(params, batch=batch, max_nodes=max_nodes, **kw)


def _quat_from_zyx(zyx):
    R = refgen.zyx_to_rotation(zyx)
    w = 0.5 * np.sqrt(max(1e-300, 1 + np.trace(R)))
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def _sensors(rng, params, n):
    qj0 = np.array(params["config"]["default_joint_state"])
    return dict(quat=np.array([_quat_from_zyx(0.2 * rng.standard_normal(3)) for _ in range(n)]), w=0.5 * rng.standard_normal((n, 3)),
                a=np.array([0, 0, 9.81]) + 0.5 * rng.standard_normal((n, 3)), qj=qj0 + 0.1 * rng.standard_normal((n, 10)),
                qdj=rng.standard_normal((n, 10)), contact=(rng.uniform(size=(n, 4)) < 0.7).astype(np.int32))


def _flat(o):
    return list(o.values()) if isinstance(o, dict) else list(o)


def _all_equal(a, b, what=None):
    for u, v in zip(_flat(a), _flat(b)):
        assert np.array_equal(np.asarray(u), np.asarray(v), equal_nan=np.asarray(u).dtype.kind == "f"), what


# ---- a. the height function -----------------------------------------------------------------------------------------------------------------
def test_ground_eval_under_a_field_map_equals_the_host_routine(params):
    """Height bit for bit and facet id, on the grids and points of the CPU test (which holds the host routine == the twin on them); the
    32 x 32 grid is the one that exercises pitch and index range."""
    maps = gft.height_maps()
    rng = np.random.default_rng(32)
    s = _solver(params, len(maps))
    try:
        s.ground_set_field(*gft.pack(maps))
        inst, xy, want_h, want_f = [], [], [], []
        for i, m in enumerate(maps):
            pts, _ = gft.height_points(m, rng)
            h, f = gfe.height(gfe.record_of(m), pts)
            inst += [i] * len(pts)
            xy.append(pts)
            want_h.append(h)
            want_f.append(f)
        h, facet = s.ground_eval(inst, np.concatenate(xy))
        assert np.array_equal(h, np.concatenate(want_h), equal_nan=True)
        assert np.array_equal(facet, np.concatenate(want_f))
        big = np.concatenate(want_f)[np.array(inst) == 2]
        assert big.max() >= 2 * 31 * 30 and len(set(big.tolist())) >= 100 and np.isnan(h).sum() == 2 * len(maps)
    finally:
        s.close()


# ---- b. the zero map is no map ------------------------------------------------------------------------------------------------------------
def _run_b(params, inputs, with_map):
    c = params["config"]
    s = _solver(params, gt.B)
    try:
        if with_map == "zero":
            s.ground_set_field(*gft.pack([gft.zero_field_map() if i & 1 else gft.level_field_map() for i in range(gt.B)]))
        elif with_map == "cleared":
            s.ground_set_field(*gft.pack(gft.cases(params)[1]))
            s.ground_set_field()
        s.refgen_reset(abi.make_refgen_config(params, joint_ik=True))
        s.refgen_set_schedule([case["sched"] for case in inputs])
        cmd = np.stack([case["cmd"] for case in inputs])
        out = []
        for call in range(2):
            t0 = np.array([case["calls"][call][0] for case in inputs])
            x = np.stack([case["calls"][call][1] for case in inputs])
            assert s.refgen_update(t0, gt.N * c["dt"], x, cmd).max() == 0
            out.append(s.get_references())
        xh0 = np.zeros((gt.B, 18))
        xh0[:, 0:3] = x[:, 6:9]
        xh0[:, 6:18] = np.stack([refgen.foot_positions(params["model"], xi) for xi in x]).reshape(gt.B, 12)
        s.estimator_reset(abi.make_estimator_config(params), xh0)
        rng = np.random.default_rng(2)
        for tick in range(3):
            v = _sensors(rng, params, gt.B)
            out.append(s.estimator_update(0.002, v["quat"], v["w"], v["a"], v["qj"], v["qdj"], v["contact"]))
            out.append(s.estimator_filter())
        s.reset(x)
        s.mpc_solve(x)
        out.append(s.get_solution())
        return out
    finally:
        s.close()


def test_zero_field_map_and_cleared_field_map_equal_no_map(params):
    inputs = gt.case_inputs(params)
    base = _run_b(params, inputs, None)
    for mode in ("zero", "cleared"):
        for a, b in zip(base, _run_b(params, inputs, mode)):
            _all_equal(a, b, mode)
    assert any(np.isnan(o["swing"]).any() for o in base[:2])       # the NaN window at gait start was part of it


# ---- c. the cases of the host test through the C ABI ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("joint_ik", [False, True])
def test_planner_on_the_device_matches_the_twin(params, joint_ik):
    """Tolerances of tests/test_gpu_refgen.py: grid 1e-12, modes ==, x_ref 1e-12 (1e-9 with the IK joint references), swing 1e-10."""
    inputs, maps, tabs, swings = gft.cases(params)
    assert min(m.margin for m in maps) > gft.MARGIN and max(abs(td[2] - to[2]) for sw in swings for _, to, td in sw) >= gft.MIN_STEP
    assert all({f & 1 for _, _, f in m.log} == {0, 1} for m in maps)
    idx = [i for i, case in enumerate(inputs) if case["joint_ik"] == joint_ik]
    assert len({gft.KINDS[i] for i in range(gt.B)}) == 6 and len(idx) == gt.B // 2
    c = params["config"]
    s = _solver(params, len(idx))
    try:
        s.ground_set_field(*gft.pack([maps[i] for i in idx]))
        s.refgen_reset(abi.make_refgen_config(params, joint_ik=joint_ik),
                       latest_stance=np.stack([refgen.foot_positions(params["model"], inputs[i]["calls"][0][1]) for i in idx]))
        s.refgen_set_schedule([inputs[i]["sched"] for i in idx])
        cmd = np.stack([inputs[i]["cmd"] for i in idx])
        for call in range(2):
            t0 = np.array([inputs[i]["calls"][call][0] for i in idx])
            x = np.stack([inputs[i]["calls"][call][1] for i in idx])
            assert s.refgen_update(t0, gt.N * c["dt"], x, cmd).max() == 0
            got = s.get_references()
            for j, i in enumerate(idx):
                ref = tabs[i][call]
                assert got["n_nodes"][j] == ref["n_nodes"] and np.array_equal(got["mode"][j], ref["mode"]), (call, i)
                assert np.abs(got["t"][j] - ref["t"]).max() < 1e-12
                assert np.abs(got["x_ref"][j][:, :12] - ref["x_ref"][:, :12]).max() < 1e-12, (call, i)
                assert np.abs(got["x_ref"][j] - ref["x_ref"]).max() < (1e-9 if joint_ik else 1e-12), (call, i)
                assert maxdiff_nan(got["swing"][j], ref["swing"]) < 1e-10, (call, i)
    finally:
        s.close()


def test_filter_on_the_device_matches_the_twin(params):
    """Tolerances of tests/test_gpu_estimator.py: rbd, x, xhat 1e-10, P 1e-9 relative.  Ten ticks per map from the feet of a standing robot."""
    inputs, maps, _, _ = gft.cases(params)
    ecfg = abi.make_estimator_config(params)
    tw_maps = [gft.FieldMap(m.dir_given, m.origin, m.spacing, m.g) for m in maps]
    x0 = np.stack([case["calls"][0][1] for case in inputs])
    xh0 = np.zeros((gt.B, 18))
    xh0[:, 0:3] = x0[:, 6:9]
    xh0[:, 6:18] = np.stack([refgen.foot_positions(params["model"], xi) for xi in x0]).reshape(gt.B, 12)
    xh0[:, 3] = 0.3
    s = _solver(params, gt.B)
    try:
        s.ground_set_field(*gft.pack(maps))
        s.estimator_reset(ecfg, xh0)
        tw = [dict(xhat=xh0[i].copy(), P=100.0 * np.eye(18)) for i in range(gt.B)]
        rng = np.random.default_rng(41)
        for tick in range(10):
            v = _sensors(rng, params, gt.B)
            rbd, x = s.estimator_update(0.002, v["quat"], v["w"], v["a"], v["qj"], v["qdj"], v["contact"])
            xh, P = s.estimator_filter()
            for i in range(gt.B):
                gt.numpy_kf(params, ecfg, tw[i], 0.002, v["quat"][i], v["w"][i], v["a"][i], v["qj"][i], v["qdj"][i], v["contact"][i], tw_maps[i])
                assert np.abs(xh[i] - tw[i]["xhat"]).max() < 1e-10, (tick, i)
                assert np.abs(rbd[i, 3:6] - tw[i]["xhat"][0:3]).max() < 1e-10 and np.abs(x[i, 6:9] - tw[i]["xhat"][0:3]).max() < 1e-10
                assert np.abs(P[i] - tw[i]["P"]).max() < 1e-9 * max(1.0, np.abs(tw[i]["P"]).max())
        assert min(m.margin for m in tw_maps) > gft.MARGIN
        assert all(np.abs(m.g).max() > 0.0 for m in tw_maps)
    finally:
        s.close()


# ---- d. the tick on instance ranges --------------------------------------------------------------------------------------------------------
TB, TN = 8, 40


def _tick_fields():
    """One field per instance under the start of the trot workload: a cross slope with a ridge ahead, different for every instance"""
    uu, ww = np.meshgrid(np.arange(9) * 0.11, np.arange(7) * 0.13, indexing="ij")
    return [gft.FieldMap([0.96, 0.28], [-0.31, -0.37], [0.11, 0.13], 0.05 * ww + (0.01 + 0.002 * i) * np.minimum(uu, 0.4)) for i in range(TB)]


def _tick_run(params, mode, field=True, pre_profile=False):
    """Seven ticks through the separate calls (mode "calls") or hb_tick_resident on `mode` instance ranges, under the field map; pre_profile:
    seven ticks under a PROFILE map first, in the same mode, and the field map then replaces it in the same context."""
    horizon = TN * params["config"]["dt"]
    knots = [[[-1.0, 0.0], [0.02 + 0.005 * i, 0.0], [0.04 + 0.005 * i, 0.03], [3.0, 0.03 + 0.02 * i]] for i in range(TB)]
    s = _solver(params, TB, TN + 6)
    try:
        if pre_profile:
            s.ground_set_profile(np.full(TB, 4, dtype=np.int32), np.tile([1.0, 0.0], (TB, 1)), np.array(knots))
        elif field:
            s.ground_set_field(*gft.pack(_tick_fields()))
        w = workload.device_trot_batch(s, params, n_intervals=TN)
        s.set_resident_inputs(w["x0"], w["t_now"], w["rbd"])
        s.set_chunks(mode if isinstance(mode, int) else 1)
        xh0 = np.zeros((TB, 18))
        xh0[:, 0:3] = w["rbd"][:, 3:6]
        xh0[:, 6:18] = np.asarray(s.eval_foot_kinematics(w["x0"], np.zeros((TB, 22)))[0]).reshape(TB, 12)
        s.estimator_reset(abi.make_estimator_config(params), xh0)
        srng = np.random.default_rng(6)
        for k in range(14 if pre_profile else 7):
            if pre_profile and k == 7:
                s.ground_set_field(*gft.pack(_tick_fields()))          # profile -> field: what a range enqueues changes
                assert s.ground_get_field()["n_nodes"].tolist() == [[9, 7]] * TB
            tk = w["t_now"] + 0.01 * (k + 1)
            quat = np.tile([0.0, 0.0, 0.0, 1.0], (TB, 1)) + 0.01 * srng.standard_normal((TB, 4))
            quat /= np.linalg.norm(quat, axis=1, keepdims=True)
            wl, al = 0.05 * srng.standard_normal((TB, 3)), np.tile([0.0, 0.0, 9.81], (TB, 1)) + 0.1 * srng.standard_normal((TB, 3))
            qj, qdj = w["rbd"][:, 6:16] + 0.01 * srng.standard_normal((TB, 10)), 0.1 * srng.standard_normal((TB, 10))
            contact = np.ones((TB, 4), dtype=np.int32)
            cmd = w["cmd"] + 0.02 * srng.standard_normal(w["cmd"].shape)
            if isinstance(mode, str):
                s.set_resident_time(tk)
                s.estimator_update(0.002, quat, wl, al, qj, qdj, contact, to_resident=True)
                assert s.refgen_update(tk, horizon, None, cmd).max() == 0
                s.step_resident()
            else:
                s.tick_resident(0.002, quat, wl, al, qj, qdj, contact, tk, horizon, cmd)
        assert s.refgen_status().max() == 0
        return (s.get_references(), s.get_solution(), s.get_wbc_solution(), s.mpc_status(), s.estimator_filter())
    finally:
        s.close()


def test_tick_resident_with_a_field_map_equals_the_separate_calls(params):
    """hb_tick_resident on one stream and on two instance ranges (the MPC part replayed as graphs once steady) against hb_set_resident_time /
    hb_estimator_update / hb_refgen_update / hb_step_resident: identical tables, iterate, WBC solution and filter state — and not those
    of the run without a map."""
    ref = _tick_run(params, "calls")
    for mode in (1, 2):
        for a, b in zip(ref, _tick_run(params, mode)):
            _all_equal(a, b, mode)
    blind = _tick_run(params, "calls", field=False)
    assert not np.array_equal(ref[0]["x_ref"], blind[0]["x_ref"]) and not np.array_equal(ref[4][0], blind[4][0])


def test_ranges_that_ticked_under_a_profile_map_tick_on_the_field_map_once_it_replaces_it(params):
    """The epoch bump of profile -> field: a context whose two ranges captured their graphs under a profile map must enqueue the field forms
    from the tick after hb_ground_set_field on.  Same history through the separate calls, then ==; and the end differs from that of a
    context which kept the profile map's history only in its first half, i.e. the field map did act."""
    ref = _tick_run(params, "calls", pre_profile=True)
    for a, b in zip(ref, _tick_run(params, 2, pre_profile=True)):
        _all_equal(a, b)
    only_field = _tick_run(params, "calls")
    assert not np.array_equal(ref[4][0], only_field[4][0])


# ---- e. the entry points ----------------------------------------------------------------------------------------------------------------------
def test_set_get_round_trip_refusals_and_one_map_at_a_time(params):
    from hunter_bipedal_control_amd.solver import HunterHipError
    inputs, maps, _, _ = gft.cases(params)
    d, o, sp, hts = gft.pack(maps)
    pn, pd, pk = gt.pack(gt.cases(params)[1])
    s = _solver(params, gt.B)

    def same_map(g):
        g2 = s.ground_get_field()
        assert all(np.array_equal(g[key], g2[key]) for key in g)

    try:
        for call in (s.ground_get_field, lambda: s.ground_eval([0], [[0.0, 0.0]])):
            with pytest.raises(HunterHipError, match="no (field|ground) map in force"):
                call()
        s.ground_set_field(d, o, sp, hts)                              # legal right after hb_create
        g = s.ground_get_field()
        assert np.array_equal(g["n_nodes"], np.array([m.g.shape for m in maps])) and np.array_equal(g["dir"], np.stack([m.a for m in maps]))
        assert np.array_equal(g["origin"], o) and np.array_equal(g["spacing"], sp)
        assert np.array_equal(g["heights"], np.stack([gft.padded(m.g) for m in maps]))
        # refusals: field_record's reasons, the first offending instance named, the map in force kept
        for what, inst in (("count", 3), ("count_high", 6), ("spacing", 0), ("steep", 7), ("dir", 5), ("nan", 2), ("origin", 4)):
            d2, o2, sp2, h2 = d.copy(), o.copy(), sp.copy(), [h.copy() for h in hts]
            if what == "count":
                h2[inst] = h2[inst][:1]
            elif what == "count_high":
                h2[inst] = np.zeros((2, 33))
            elif what == "spacing":
                sp2[inst, 1] = 0.0
            elif what == "steep":
                h2[inst][1, 1] = h2[inst][0, 0] + 2.0 * sp2[inst].max()
            elif what == "dir":
                d2[inst] = 0.0
            elif what == "nan":
                h2[inst][0, 1] = np.nan
            else:
                o2[inst, 0] = np.inf
            with pytest.raises(HunterHipError, match="the map in force is kept") as e:
                s.ground_set_field(d2, o2, sp2, h2)
            assert f"instance {inst} " in str(e.value), (what, str(e.value))
            same_map(g)
        with pytest.raises(HunterHipError, match="the map in force is kept"):
            s._check(s.lib.hb_ground_set_field(s.ctx, None, d.ctypes.data, None, None, None), "hb_ground_set_field")
        same_map(g)
        with pytest.raises(HunterHipError):
            s.ground_eval([gt.B], [[0.0, 0.0]])
        # the map survives the resets of its consumers and of the plant
        s.refgen_reset(abi.make_refgen_config(params))
        s.estimator_reset(abi.make_estimator_config(params))
        s.plant_reset(np.tile(np.concatenate([[0, 0, 0.62, 0, 0, 0], params["config"]["default_joint_state"]]), (gt.B, 1)))
        same_map(g)
        # one map at a time: each getter refuses while the other kind is in force, each setter replaces the other's map
        with pytest.raises(HunterHipError, match="field map"):
            s.ground_get_profile()
        s.ground_set_profile(pn, pd, pk)
        assert np.array_equal(s.ground_get_profile()["knots"], pk)
        with pytest.raises(HunterHipError, match="profile map"):
            s.ground_get_field()
        h, seg = s.ground_eval([1], [[0.3, 0.1]])                      # hb_ground_eval under a profile map: the profile's segment, as ever
        want = gt.GroundMap(pd[1], pk[1, :pn[1]]).height(0.3, 0.1)
        assert h[0] == want[0] and seg[0] == want[1]
        s.ground_set_field(d, o, sp, hts)
        same_map(g)
        with pytest.raises(HunterHipError, match="field map"):
            s.ground_get_profile()
        s.ground_set_field()
        for call in (s.ground_get_field, s.ground_get_profile):
            with pytest.raises(HunterHipError, match="no (field|ground) map in force"):
                call()
        s.ground_set_field()                                           # clearing twice is fine
        s.ground_set_field(d, o, sp, hts)
        s.ground_set_profile()                                         # all-NULL in either setter switches the map in force off
        with pytest.raises(HunterHipError, match="no field map in force"):
            s.ground_get_field()
    finally:
        s.close()


def test_a_following_profile_draw_and_a_field_map_refuse_one_another(params):
    """Either order, HB_ERR_STATE (the draw writes profile records); what is in force stays."""
    import _profiledrawemu as pd
    from hunter_bipedal_control_amd.rollout import lowest_contact_point, standing_configuration
    from hunter_bipedal_control_amd.solver import HunterHipError
    B = 4
    m = gft.level_field_map()
    fld = gft.pack([m] * B)
    follow = abi.make_profile_draw_config(**dict(pd.CONFIGS["gpu_draw"], follow_map=1))
    s = _solver(params, B, 108)
    try:
        q0 = standing_configuration(params, B, s)
        q0[:, 0] += 0.37 * np.arange(B) - 1.0
        s.plant_reset(q0)
        s.plant_set_contact_model(abi.make_contact_config(params, mu=0.31, ground_z=lowest_contact_point(s, q0)))
        s.plant_set_episode(abi.make_episode_config(tilt_limit=0.2))
        s.plant_set_respawn(abi.make_respawn_config(hold_ticks=0, max_ticks=1, place=1, clearance=0.002, seed=5), q0)
        s.ground_set_field(*fld)
        with pytest.raises(HunterHipError, match="HB_ERR_STATE.*field map|field map") as e:
            s.plant_set_profile_draw(follow)
        assert "hb_plant_set_profile_draw" in str(e.value)
        assert np.array_equal(s.ground_get_field()["heights"][0], m.g)
        with pytest.raises(HunterHipError):                            # (no draw came into force)
            s.plant_profile_draw()
        s.ground_set_profile(np.full(B, 2, dtype=np.int32), np.tile(np.array(follow.dir[:]), (B, 1)), np.tile([[-1.0, 0.0], [1.0, 0.0]], (B, 1, 1)))
        s.plant_set_profile_draw(follow)                               # the zero profile map first: legal, as before
        with pytest.raises(HunterHipError, match="profile draw") as e:
            s.ground_set_field(*fld)
        assert "hb_ground_set_field" in str(e.value)
        assert s.ground_get_profile()["n_knots"].min() >= 2             # the profile map is still in force
        with pytest.raises(HunterHipError, match="profile map"):
            s.ground_get_field()
        s.plant_set_profile_draw(None)
        s.ground_set_field(*fld)                                       # without the draw the field map goes in
        assert s.ground_get_field()["n_nodes"].tolist() == [[32, 32]] * B
    finally:
        s.close()


# ---- g. the closed loop -----------------------------------------------------------------------------------------------------------------------
SLOPES = ((0.0, 0.0), (0.03, 0.015), (0.03, -0.015))       # (rise along the walk, cross slope) of the plane of each pair of robots
LOOP_TICKS = 2400


def _plane_field(p, r):
    """A 32 x 32 field over the walk whose heights are the plane z = p x + r y, on a grid turned against both (the gradient lies along no
    grid axis), zero at the world origin where the robots start."""
    a = np.array([0.8, 0.6])
    b = np.array([-a[1], a[0]])
    sp, org = np.array([0.06, 0.06]), np.array([-0.7, -0.9])
    uu, ww = np.meshgrid(org[0] + np.arange(32) * sp[0], org[1] + np.arange(32) * sp[1], indexing="ij")
    x, y = uu * a[0] + ww * b[0], uu * a[1] + ww * b[1]
    return dict(dir=a, origin=org, spacing=sp, heights=p * x + r * y)


def _closed_loop(params, with_map):
    """B = 6 robots trot at (0.2, 0), ground plant, joint model, estimator in the loop: robots 0, 1 on a level field, 2, 3 and 4, 5 on the two
    oblique planes; the even ones are given their
    field as the controller's map, the odd ones the zero field map (blind).  with_map False: the same loop built without ground_map."""
    from hunter_bipedal_control_amd.rollout import ResidentLoop
    B = 6
    fields = [_plane_field(*SLOPES[i // 2]) for i in range(B)]
    gm = None
    if with_map:
        gm = dict(field=[f if i % 2 == 0 else dict(f, heights=np.zeros((32, 32))) for i, f in enumerate(fields)])
    s = _solver(params, B, 108)
    try:
        loop = ResidentLoop(s, params, ["trot"] * B, np.tile([0.2, 0.0, 0.0, 0.0], (B, 1)), contact_config=dict(fall_height=0.2), joint_model={},
                            use_estimator=True, terrain=dict(field=fields, relative=True), episode=dict(slip_speed=0.05), ground_map=gm)
        facet0 = s.plant_get_terrain_field()["facet"].copy()
        loop.run(LOOP_TICKS - 100)
        err = []
        for _ in range(100):
            loop.step(check_refgen=False)
            err.append(s.estimator_filter()[0][:, 2] - s.plant_state()["q"][:, 2])
        st = s.plant_state()
        return dict(err=np.array(err), q=st["q"], v=st["v"], ep=loop.episode(), xhat=s.estimator_filter()[0], facet0=facet0,
                    facet=s.plant_get_terrain_field()["facet"])
    finally:
        s.close()


def test_closed_loop_on_oblique_planes_with_and_without_the_field_map(params):
    blind = _closed_loop(params, False)
    mixed = _closed_loop(params, True)
    # asserted first: the level robot with the map is the same robot in a loop built without ground_map, bit for bit (and so is every blind one)
    for k in ("q", "v", "xhat"):
        assert np.array_equal(mixed[k][0], blind[k][0]), k
        assert np.array_equal(mixed[k][1::2], blind[k][1::2]), k
    assert np.array_equal(mixed["err"][:, 0], blind["err"][:, 0])
    # all six ended upright, and the ground under them changed
    for run in (blind, mixed):
        assert np.isfinite(run["q"]).all() and np.isfinite(run["v"]).all() and (run["ep"]["END_CAUSE"] == abi.HB_EP_RUNNING).all(), run["ep"]["END_CAUSE"]
    assert (mixed["facet"] != mixed["facet0"]).all(), (mixed["facet0"], mixed["facet"])
    e = mixed["err"].mean(axis=0)                                       # [6]: z estimate - z plant over the last 100 ticks
    hs = []
    for pair in (1, 2):
        i = 2 * pair
        pf = _plane_field(*SLOPES[pair])
        f = gft.FieldMap(pf["dir"], pf["origin"], pf["spacing"], pf["heights"])
        h = f.G(mixed["q"][i, 0], mixed["q"][i, 1])
        hs.append(h)
        print(f"  plane {SLOPES[pair]}: map height under the base {h:+.4f} m; z estimate - z plant: level {e[0]:+.5f}, mapped {e[i]:+.5f}, blind {e[i + 1]:+.5f}")
    assert min(hs) >= 0.02, hs                                          # asserted first: the robots climbed 2 cm
    for pair, h in zip((1, 2), hs):
        i = 2 * pair
        assert abs(e[i] - e[0]) <= 0.5 * h, (pair, e[i], e[0], h)       # item 26's assertion
        assert abs(e[i + 1] - e[0]) > abs(e[i] - e[0]), (pair, e)        # the blind robot's error is further from the level robot's
