"""-m gpu: the controller's ground map on the device (hb_ground_set_profile; k_refgen_ground, k_estimator_ground, k_ground_eval) against its
numpy twin (tests/_groundtwin.py), against contexts without a map, through the instance-range path and in the closed loop.  The cases and
the twin's tables are those of tests/test_groundmap_host.py, computed once.

Closed loop (test f), measured on an MI355X (pytest -s prints the figures): every robot is beyond the riser after 700 ticks; over the next
100 ticks z estimate - z plant is +0.0246 .. +0.0282 on level ground, +0.0271 .. +0.0344 / +0.0247 .. +0.0282 for the robots that know their
2 cm step up / 1 cm step down (asserted: within h/2 of the level robot's) and +0.0137 .. +0.0190 / +0.0329 .. +0.0366 for the blind ones
(a finding, not asserted).  DESIGN.md §5 item 26."""
import numpy as np
import pytest

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


# ---- a. the height function -----------------------------------------------------------------------------------------------------------------
def test_ground_eval_equals_the_twin(params):
    inputs, maps, _, _ = gt.cases(params)
    rng = np.random.default_rng(5)
    s = _solver(params, gt.B)
    try:
        s.ground_set_profile(*gt.pack(maps))
        inst, xy = [], []
        for i, m in enumerate(maps):
            pts = rng.uniform(-1.5, 2.5, (70, 2))
            if abs(m.a[0]) == 1.0 and len(m.knots) > 2:       # points exactly on the breakpoints, and one ulp-scale step to either side
                on = np.stack([m.knots[:, 0], rng.uniform(-1, 1, len(m.knots))], axis=1)
                pts = np.concatenate([pts, on, on + [2.0 ** -40, 0.0], on - [2.0 ** -40, 0.0]])
            pts = np.concatenate([pts, [[np.nan, 0.0]]])
            inst += [i] * len(pts)
            xy.append(pts)
        xy = np.concatenate(xy)
        h, seg = s.ground_eval(inst, xy)
        want = [gt.GroundMap(maps[i].dir_given, maps[i].knots).height(x, y) for i, (x, y) in zip(inst, xy)]
        assert np.array_equal(h, np.array([w[0] for w in want]), equal_nan=True)
        assert np.array_equal(seg, np.array([w[1] for w in want]))
        assert len(set(seg.tolist())) >= 8
    finally:
        s.close()


# ---- b. the zero map is no map ------------------------------------------------------------------------------------------------------------
def _run_b(params, inputs, with_map):
    c = params["config"]
    s = _solver(params, gt.B)
    try:
        if with_map == "zero":
            s.ground_set_profile(np.full(gt.B, 2, dtype=np.int32), np.tile([1.0, 0.0], (gt.B, 1)), np.tile([[0.0, 0.0], [1.0, 0.0]], (gt.B, 1, 1)))
        elif with_map == "cleared":
            s.ground_set_profile(*gt.pack(gt.cases(params)[1]))
            s.ground_set_profile()
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


def _flat(o):
    return list(o.values()) if isinstance(o, dict) else list(o)


def test_zero_map_and_cleared_map_equal_no_map(params):
    inputs = gt.case_inputs(params)
    base = _run_b(params, inputs, None)
    for mode in ("zero", "cleared"):
        for a, b in zip(base, _run_b(params, inputs, mode)):
            for u, v in zip(_flat(a), _flat(b)):
                assert np.array_equal(np.asarray(u), np.asarray(v), equal_nan=np.asarray(u).dtype.kind == "f"), mode
    assert any(np.isnan(o["swing"]).any() for o in base[:2])       # the NaN window at gait start was part of it


# ---- c. the cases of the host test through the C ABI ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("joint_ik", [False, True])
def test_planner_on_the_device_matches_the_twin(params, joint_ik):
    """Tolerances of tests/test_gpu_refgen.py: grid 1e-12, modes ==, x_ref 1e-12 (1e-9 with the IK joint references), swing 1e-10."""
    inputs, maps, tabs, swings = gt.cases(params)
    assert min(m.margin for m in maps) > gt.MARGIN and max(abs(td[2] - to[2]) for sw in swings for _, to, td in sw) >= gt.MIN_STEP
    idx = [i for i, case in enumerate(inputs) if case["joint_ik"] == joint_ik]
    c = params["config"]
    s = _solver(params, len(idx))
    try:
        s.ground_set_profile(*gt.pack([maps[i] for i in idx]))
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
    inputs, maps, _, _ = gt.cases(params)
    ecfg = abi.make_estimator_config(params)
    tw_maps = [gt.GroundMap(m.dir_given, m.knots) for m in maps]
    x0 = np.stack([case["calls"][0][1] for case in inputs])
    xh0 = np.zeros((gt.B, 18))
    xh0[:, 0:3] = x0[:, 6:9]
    xh0[:, 6:18] = np.stack([refgen.foot_positions(params["model"], xi) for xi in x0]).reshape(gt.B, 12)
    xh0[:, 3] = 0.3
    s = _solver(params, gt.B)
    try:
        s.ground_set_profile(*gt.pack(maps))
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
        assert min(m.margin for m in tw_maps) > gt.MARGIN
        assert max(abs(h) for m in tw_maps for h in m.knots[:, 1]) > 0.0
    finally:
        s.close()


# ---- d. the tick on instance ranges --------------------------------------------------------------------------------------------------------
def test_tick_resident_with_a_map_equals_the_separate_calls(params):
    """Seven ticks with a map set: hb_tick_resident on one stream and on two instance ranges (set_chunks(2): estimator and reference
    generation per range, the MPC part replayed as graphs once steady) against hb_set_resident_time / hb_estimator_update /
    hb_refgen_update / hb_step_resident: identical tables, iterate, WBC solution and filter state — and not those of the run without a map."""
    B, N = 10, 40
    horizon = N * params["config"]["dt"]
    knots = [[[-1.0, 0.0], [0.02 + 0.005 * i, 0.0], [0.04 + 0.005 * i, 0.03], [3.0, 0.03 + 0.02 * i]] for i in range(B)]
    out = []
    for mode in ("calls", 1, 2, "calls, no map"):
        s = _solver(params, B, N + 6)
        try:
            if mode != "calls, no map":
                s.ground_set_profile(np.full(B, 4, dtype=np.int32), np.tile([1.0, 0.0], (B, 1)), np.array(knots))
            w = workload.device_trot_batch(s, params, n_intervals=N)
            s.set_resident_inputs(w["x0"], w["t_now"], w["rbd"])
            s.set_chunks(mode if isinstance(mode, int) else 1)
            xh0 = np.zeros((B, 18))
            xh0[:, 0:3] = w["rbd"][:, 3:6]
            xh0[:, 6:18] = np.asarray(s.eval_foot_kinematics(w["x0"], np.zeros((B, 22)))[0]).reshape(B, 12)
            s.estimator_reset(abi.make_estimator_config(params), xh0)
            srng = np.random.default_rng(6)
            for k in range(7):
                tk = w["t_now"] + 0.01 * (k + 1)
                quat = np.tile([0.0, 0.0, 0.0, 1.0], (B, 1)) + 0.01 * srng.standard_normal((B, 4))
                quat /= np.linalg.norm(quat, axis=1, keepdims=True)
                wl, al = 0.05 * srng.standard_normal((B, 3)), np.tile([0.0, 0.0, 9.81], (B, 1)) + 0.1 * srng.standard_normal((B, 3))
                qj, qdj = w["rbd"][:, 6:16] + 0.01 * srng.standard_normal((B, 10)), 0.1 * srng.standard_normal((B, 10))
                contact = np.ones((B, 4), dtype=np.int32)
                cmd = w["cmd"] + 0.02 * srng.standard_normal(w["cmd"].shape)
                if isinstance(mode, str):
                    s.set_resident_time(tk)
                    s.estimator_update(0.002, quat, wl, al, qj, qdj, contact, to_resident=True)
                    assert s.refgen_update(tk, horizon, None, cmd).max() == 0
                    s.step_resident()
                else:
                    s.tick_resident(0.002, quat, wl, al, qj, qdj, contact, tk, horizon, cmd)
            assert s.refgen_status().max() == 0
            out.append((s.get_references(), s.get_solution(), s.get_wbc_solution(), s.mpc_status(), s.estimator_filter()))
        finally:
            s.close()
    ref = out[0]
    for other in out[1:3]:
        for a, b in zip(ref, other):
            for u, v in zip(_flat(a), _flat(b)):
                assert np.array_equal(np.asarray(u), np.asarray(v), equal_nan=np.asarray(u).dtype.kind == "f")
    assert not np.array_equal(ref[0]["x_ref"], out[3][0]["x_ref"]) and not np.array_equal(ref[4][0], out[3][4][0])


# ---- e. the entry points ----------------------------------------------------------------------------------------------------------------------
def test_set_get_round_trip_and_refusals(params):
    from hunter_bipedal_control_amd.solver import HunterHipError
    inputs, maps, _, _ = gt.cases(params)
    n, d, k = gt.pack(maps)
    s = _solver(params, gt.B)
    try:
        for call in (s.ground_get_profile, lambda: s.ground_eval([0], [[0.0, 0.0]])):
            with pytest.raises(HunterHipError, match="no ground map in force"):
                call()
        s.ground_set_profile(n, d, k)                                  # legal right after hb_create
        g = s.ground_get_profile()
        assert np.array_equal(g["n_knots"], n) and np.array_equal(g["knots"], k)
        assert np.array_equal(g["dir"], np.stack([m.a for m in maps]))
        for i, m in enumerate(maps):
            assert np.array_equal(g["slopes"][i, :len(m.slopes)], m.slopes) and not g["slopes"][i, len(m.slopes):].any()
        bad = []
        for what, inst in (("knots", 3), ("spacing", 0), ("steep", 7), ("dir", 5), ("nan", 2), ("count", 6)):
            n2, d2, k2 = n.copy(), d.copy(), k.copy()
            if what == "knots":
                n2[inst] = 1
            elif what == "count":
                n2[inst] = 17
            elif what == "spacing":
                k2[inst, 1, 0] = k2[inst, 0, 0]
            elif what == "steep":
                k2[inst, 1, 1] = k2[inst, 0, 1] + 1.8 * (k2[inst, 1, 0] - k2[inst, 0, 0])
            elif what == "dir":
                d2[inst] = 0.0
            else:
                k2[inst, 0, 1] = np.nan
            bad.append((inst, (n2, d2, k2)))
        bad.append((None, (n, None, k)))
        for inst, args in bad:
            with pytest.raises(HunterHipError, match="the map in force is kept") as e:
                s.ground_set_profile(*args)
            assert inst is None or f"instance {inst} " in str(e.value)
            g2 = s.ground_get_profile()
            assert all(np.array_equal(g[key], g2[key]) for key in g)                       # every refusal leaves the stored map unchanged
        with pytest.raises(HunterHipError):
            s.ground_eval([gt.B], [[0.0, 0.0]])                        # an instance outside the batch is refused on the host
        # the map survives the resets of its consumers and of the plant
        s.refgen_reset(abi.make_refgen_config(params))
        s.estimator_reset(abi.make_estimator_config(params))
        s.plant_reset(np.tile(np.concatenate([[0, 0, 0.62, 0, 0, 0], params["config"]["default_joint_state"]]), (gt.B, 1)))
        g2 = s.ground_get_profile()
        assert all(np.array_equal(g[key], g2[key]) for key in g)
        s.ground_set_profile()
        with pytest.raises(HunterHipError, match="no ground map in force"):
            s.ground_get_profile()
        s.ground_set_profile()                                         # clearing twice is fine
    finally:
        s.close()


# ---- f. the closed loop -----------------------------------------------------------------------------------------------------------------------
STEPS = (0.0, 0.02, -0.01)
RISER_AT = 0.08


def _closed_loop(params, ground_map):
    """B = 6 robots trot at (0.2, 0) over a level profile, a 2 cm step up and a 1 cm step down whose riser starts 8 cm ahead; instances
    0 - 2 know the profile, 3 - 5 do not (the zero map).  ground_map False: the same loop built without one (every robot blind).  Runs until
    the segment word shows all four contact points and the base of every robot beyond the riser, then 100 ticks more -> dict."""
    from hunter_bipedal_control_amd.rollout import ResidentLoop, curb_profile
    B = 6
    knots = [curb_profile(h, RISER_AT) for h in STEPS] * 2
    level = curb_profile(0.0, RISER_AT)
    gm = dict(dir=np.tile([1.0, 0.0], (B, 1)), knots=knots[:3] + [level] * 3) if ground_map else None
    s = _solver(params, B, 108)
    try:
        loop = ResidentLoop(s, params, ["trot"] * B, np.tile([0.2, 0.0, 0.0, 0.0], (B, 1)), contact_config=dict(fall_height=0.2), joint_model={},
                            use_estimator=True, terrain=dict(profile=dict(dir=np.tile([1.0, 0.0], (B, 1)), knots=knots), relative=True),
                            episode=dict(slip_speed=0.05), ground_map=gm)
        ticks, beyond = 0, False
        while ticks < 2000 and not beyond:
            loop.run(50)
            ticks += 50
            beyond = bool((s.plant_get_terrain_profile()["segment"] == 2).all())
        err = []
        for _ in range(100 if beyond else 0):
            loop.step(check_refgen=False)
            err.append(s.estimator_filter()[0][:, 2] - s.plant_state()["q"][:, 2])
        st = s.plant_state()
        return dict(beyond=beyond, ticks=ticks, err=np.array(err), q=st["q"], v=st["v"], ep=loop.episode(), xhat=s.estimator_filter()[0])
    finally:
        s.close()


def test_closed_loop_over_a_step_with_and_without_the_map(params):
    blind = _closed_loop(params, False)
    mixed = _closed_loop(params, True)
    # asserted first: the zero-map robots are the robots of a loop without a map, and the blind robots got across upright
    assert blind["beyond"] and mixed["beyond"], (blind["ticks"], mixed["ticks"])
    for k in ("q", "v", "xhat"):
        assert np.array_equal(mixed[k][3:], blind[k][3:]), k
    assert mixed["ticks"] == blind["ticks"] and np.array_equal(mixed["err"][:, 3:], blind["err"][:, 3:])
    assert np.isfinite(blind["q"]).all() and np.isfinite(blind["v"]).all() and (blind["ep"]["END_CAUSE"] == abi.HB_EP_RUNNING).all(), blind["ep"]["END_CAUSE"]
    # then: so did the robots that know the step
    assert np.isfinite(mixed["q"]).all() and np.isfinite(mixed["v"]).all() and (mixed["ep"]["END_CAUSE"] == abi.HB_EP_RUNNING).all(), mixed["ep"]["END_CAUSE"]
    e = mixed["err"]                                                   # [100][6]: z estimate - z plant
    print("closed loop, ticks to get beyond the riser:", mixed["ticks"])
    for i, h in enumerate(STEPS):
        print(f"  step {h:+.3f}: aware error {e[:, i].min():+.5f} .. {e[:, i].max():+.5f}, blind error {e[:, 3 + i].min():+.5f} .. {e[:, 3 + i].max():+.5f}")
    for i, h in enumerate(STEPS[1:], start=1):
        dev = np.abs(e[:, i] - e[:, 0]).max()
        assert dev <= 0.5 * abs(h), (h, dev)
