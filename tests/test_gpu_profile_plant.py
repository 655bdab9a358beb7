"""Per-instance terrain profile of the ground-contact plant on the device (hb_plant_set_terrain_profile; k_plant_profile,
k_plant_profile_joints and their hybrid forms) against the numpy twin of the definition (tests/_profileemu.py) with the device's own
rigid-body terms, the exact identities with the other plant forms, the API surface and ResidentLoop(terrain=dict(profile=...)).  B = 6: one
scenario of pe.scenarios per instance, so one batch holds a slope, a kink under each foot, a step down, a lateral step, a slider that
crosses a breakpoint and level ground."""
import numpy as np
import pytest

import _contactemu as ce
import _jointemu as je
import _profileemu as pe
import _terrainemu as te
from hunter_bipedal_control_amd import abi

pytestmark = pytest.mark.gpu

B = pe.B


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
    return abi.make_contact_config(params, **{**dict(mu=pe.CFG_MU, ground_z=pe.CFG_GROUND, erp=pe.ERP, sweeps=pe.SWEEPS), **kw})


def _outputs(s, joints, profile=True):
    st, con = s.plant_state(), s.plant_contact()
    o = dict(q=st["q"], v=st["v"], lam=st["lam"], vdot=st["vdot"], rbd=st["rbd"], gap=con["gap"], point_vel=con["point_vel"].reshape(-1, 12),
             residual=con["residual"], touching=con["touching"], status=con["status"])
    if joints:
        jo = s.plant_get_joints()
        o.update(tau_applied=jo["tau_applied"], friction_torque=jo["friction_torque"], limit_torque=jo["limit_torque"], jresidual=jo["residual"],
                 jstatus=jo["status"])
    if profile:
        o["segment"] = s.plant_get_terrain_profile()["segment"]
    return o


def _row(o, i):
    return {k: (float(a[i]) if k in ("residual", "jresidual") else a[i]) for k, a in o.items()}


def _start(s, params, scen, joints, ground="profile", **cfg):
    """ground: "profile", "none", or (plane[B][4], mu[B][4]) for hb_plant_set_terrain."""
    s.plant_reset(np.array([c["q0"] for c in scen]), np.array([c["v0"] for c in scen]), eps=pe.EPS)
    s.plant_set_contact_model(_cfg(params, **cfg))
    s.plant_set_joint_model(abi.make_joint_model(params) if joints else None)
    if isinstance(ground, str) and ground == "profile":
        s.plant_set_terrain_profile(*pe.pack(scen))
    elif isinstance(ground, str):
        s.plant_set_terrain(None, None)
    else:
        s.plant_set_terrain(*ground)


def _command(q, tau):
    return dict(pos_des=q[:, 6:].copy(), vel_des=np.zeros((len(q), 10)), kp=np.full((len(q), 10), 5.0), kd=np.full((len(q), 10), 0.05), tau_ff=tau)


def _facet_p(lam, planes):
    """World forces lam[B][12] -> each point's components in the frame of its facet planes[B][4][4], times h: the twin's impulses."""
    return np.array([pe.facet_components(lam[i], planes[i]).reshape(12) for i in range(len(lam))]) * pe.H


def _run(s, joints, tau, flags, ticks, hybrid, profile):
    out = []
    for _ in range(ticks):
        if hybrid:
            s.plant_step_hybrid(_command(s.plant_state()["q"], tau), flags, pe.DT, pe.SUBSTEPS)
        else:
            s.plant_step(tau, flags, pe.DT, pe.SUBSTEPS)
        o = _outputs(s, joints, profile)
        o.pop("segment", None)
        if hybrid:
            o.update({k: a for k, a in s.plant_get_actuator().items() if k != "last_timestamp"})
        out.append(o)
    return out


@pytest.fixture(scope="module")
def dev(params):
    """One context, B = 6.  passes[joints][tick] = dict(dev, twin, start): the device on the six profiles and the twin re-seeded with the
    device's (q, v, p) before every tick; momentum[joints]: ticks of one substep from states of the passes; rolled[joints]: the batch with
    scenarios and inputs rolled by one instance; same[joints, hybrid] = (profile run, run without a terrain, run on the plane terrain of
    each instance's first segment, and the last two again under a model variation).  Shared by the tests below and left unchanged."""
    from hunter_bipedal_control_amd.rollout import standing_configuration
    s = _solver(params)
    out = dict(passes={}, momentum={}, rolled={}, same={})
    try:
        foot_fn, qv_fn = _device_fns(s)
        q_stand = standing_configuration(params, 1, s)[0]
        scen = pe.scenarios(q_stand, qv_fn, foot_fn)
        q0, v0 = np.array([c["q0"] for c in scen]), np.array([c["v0"] for c in scen])
        tau = np.array([c["tau"] for c in scen])
        flags = np.ones((B, 4), dtype=np.int32)
        jmd = je.model_dict(abi.make_joint_model(params))
        for joints in (False, True):
            _start(s, params, scen, joints)
            got = s.plant_get_terrain_profile()
            tw = pe.ProfilePlant(qv_fn, foot_fn, q0, v0, scen, jmd if joints else None)
            rec, o, planes = [], _outputs(s, joints), None
            for tick in range(pe.TICKS):
                tw.q, tw.v = o["q"].copy(), o["v"].copy()
                tw.p = np.zeros((B, 12)) if planes is None else _facet_p(o["lam"], planes)
                if joints:
                    tw.jp = np.concatenate([o["friction_torque"], o["limit_torque"]], axis=1) * pe.H
                start = o
                tw.step(tau)
                planes = tw.last_planes
                s.plant_step(tau, flags, pe.DT, pe.SUBSTEPS)
                o = _outputs(s, joints)
                rec.append(dict(dev=o, twin=tw.record(), start=start))
            out["passes"][joints] = rec
            # ticks of ONE substep from four states of the pass, with a base force on the odd ones
            mom = []
            for k, r in enumerate(rec[2:18:5]):
                st = r["start"]
                s.plant_reset(st["q"], st["v"], eps=pe.EPS)      # (the profile survives; the impulses start from zero)
                wrench = np.tile([12.0, -7.0, 3.0, 0.0, 0.0, 0.0], (B, 1)) if k % 2 else None
                s.plant_set_external_wrench(wrench)
                s.plant_step(tau, flags, pe.H, 1)
                terms = [qv_fn(st["q"][i], st["v"][i])[:2] for i in range(B)]
                mom.append(dict(dev=_outputs(s, joints), v_in=st["v"], terms=terms, wrench=wrench))
            s.plant_set_external_wrench(None)
            out["momentum"][joints] = mom
            # the scenarios and every input rolled by one instance: instance i + 1 of this run is instance i of the pass
            _start(s, params, pe.rolled(scen), joints)
            rr = []
            for tick in range(12):
                s.plant_step(np.roll(tau, 1, axis=0), flags, pe.DT, pe.SUBSTEPS)
                rr.append(_outputs(s, joints))
            out["rolled"][joints] = rr
            # the other plant forms: no terrain (for instance 5) and the plane terrain of every instance's first segment (for instance 0)
            first = got["records"][:, 0]
            plane = np.concatenate([first[:, [2, 5, 8]], first[:, 9:10]], axis=1)
            mu = np.array([c["mu"] for c in scen])
            scale = np.tile(np.linspace(0.9, 1.2, 11), (B, 1))
            for hybrid in (False, True):
                runs = {}
                for name, ground, vary in (("profile", "profile", False), ("none", "none", False), ("plane", (plane, mu), False),
                                           ("profile_varied", "profile", True), ("plane_varied", (plane, mu), True)):
                    _start(s, params, scen, joints, ground)
                    s.plant_set_model_variation(scale if vary else None, None)
                    runs[name] = _run(s, joints, tau, flags, 8, hybrid, ground == "profile")
                s.plant_set_model_variation(None, None)
                out["same"][joints, hybrid] = runs
            if not joints:
                s.plant_set_terrain(plane, mu)
                out["getter"] = dict(profile=got, terrain=s.plant_get_terrain())
        out.update(scen=scen, mu=np.array([c["mu"] for c in scen]))
    finally:
        s.close()
    return out


@pytest.mark.parametrize("joints", [False, True])
def test_device_matches_the_twin_tick_by_tick(dev, joints):
    """The margin first, then q 1e-10; v, lambda and with the joint model friction / limit torque 10 x the twin's measured sensitivity
    (tests/_profileemu.py); the segments of hb_plant_get_terrain_profile == the twin's.  Every instance on every tick."""
    worst, margin, crossings = {}, np.inf, 0
    for r in dev["passes"][joints]:
        for i in range(B):
            for k, e in pe.check_against_twin(_row(r["dev"], i), {k: a[i] for k, a in r["twin"].items()}, joints).items():
                worst[k] = max(worst.get(k, 0.0), e)
        margin = min(margin, r["twin"]["margin"].min())
        crossings += int(not np.array_equal(r["dev"]["segment"], dev["passes"][joints][0]["dev"]["segment"]))
    assert crossings >= 1
    print("joint model", joints, "smallest margin", margin, "worst against the twin:", {k: f"{e:.2e}" for k, e in worst.items()})


@pytest.mark.parametrize("joints", [False, True])
def test_forces_lie_in_the_cone_of_their_own_facet(dev, joints):
    """Every touching point's force in the cone of its own facet, no force on a point that does not touch, no non-finite bit; scenario (2)
    touches down heels first; scenario (4) slides, on its cone (the bounds of tests/_profileemu.py, a factor 2 from the twin's figures)."""
    slow, off = np.inf, 0.0
    for tick, r in enumerate(dev["passes"][joints]):
        for i in range(B):
            pe.check_cone(r["dev"]["lam"][i], r["dev"]["touching"][i], r["twin"]["last_planes"][i], dev["mu"][i])
        assert (r["dev"]["status"] & ce.NONFINITE == 0).all()
        if tick >= 5:
            s, o = pe.slide_figures(_row(r["dev"], 4), r["twin"]["last_planes"][4], dev["mu"][4])
            slow, off = min(slow, s), max(off, o)
    order = [2, 3, 0, 1]                       # (device order: the two front points, then the two rear ones; checked on the gaps below)
    first, front = pe.check_late_touchdown(np.array([r["dev"]["touching"][2] for r in dev["passes"][joints]])[:, order])
    gap0 = dev["passes"][joints][0]["dev"]["gap"][2]
    assert gap0[order[:2]].max() < gap0[order[2:]].min()                      # the rear points start closer to their ground
    print("joint model", joints, "(2) first touch rear / front:", first, front, " (4) slowest touching point", slow, "off its cone", off)
    assert slow >= pe.SLIDE4_BOUND and off <= pe.ON_CONE4_BOUND


@pytest.mark.parametrize("joints", [False, True])
def test_base_momentum_rows_pin_lambda_as_world_forces(dev, joints):
    """Ticks of one substep, scenarios 1, 2, 3 (tests/test_profile_plant_host.py says why not 4): (M dv / h + nle)[0:3] = sum_c lambda_c +
    F_ext to 64 roundings with M, nle from eval_rbd at the start state."""
    loaded = 0
    for m in dev["momentum"][joints]:
        for i in (1, 2, 3):
            M, nle = m["terms"][i]
            pe.check_base_momentum(m["dev"]["lam"][i], m["dev"]["v"][i], m["v_in"][i], M, nle, pe.H, None if m["wrench"] is None else m["wrench"][i])
            loaded += int(np.abs(m["dev"]["lam"][i]).max() > 1.0)
    assert loaded >= 4


@pytest.mark.parametrize("hybrid", [False, True])
@pytest.mark.parametrize("joints", [False, True])
def test_the_other_plant_forms_give_the_same_values(dev, joints, hybrid):
    """== on every output of 8 ticks: instance 5 (level at ground_z, cfg.mu) against the kernels without a terrain; instance 0 (one segment)
    against the terrain kernels on the plane of its stored record; instance 0 under a model variation against the varied kernels."""
    runs = dev["same"][joints, hybrid]
    for name, other, i in (("profile", "none", 5), ("profile", "plane", 0), ("profile_varied", "plane_varied", 0)):
        for tick, (a, b) in enumerate(zip(runs[name], runs[other])):
            for k in a:
                assert np.array_equal(a[k][i], b[k][i]), (name, k, tick)
    assert any(np.abs(a["lam"][[0, 5]]).max() > 1.0 for a in runs["profile"])
    assert not np.array_equal(runs["profile"][-1]["v"][0], runs["profile_varied"][-1]["v"][0])      # (the variation does change the step)


@pytest.mark.parametrize("joints", [False, True])
def test_scenarios_rolled_by_one_instance(dev, joints):
    """Instance i of the pass == instance i + 1 of the run with scenarios and inputs rolled by one, on every output of 12 ticks."""
    for tick, rolled in enumerate(dev["rolled"][joints]):
        o = dev["passes"][joints][tick]["dev"]
        for k in o:
            assert np.array_equal(np.roll(o[k], 1, axis=0), rolled[k]), (k, tick)
    o = dev["passes"][joints][11]["dev"]
    assert not np.array_equal(o["lam"][0], o["lam"][1]) and not np.array_equal(o["lam"][1], o["lam"][3])   # (the scenarios do differ)


def test_the_getter_returns_the_records_of_the_same_planes(dev):
    """records[i][0] of hb_plant_get_terrain_profile == frame and d of hb_plant_get_terrain after hb_plant_set_terrain on that plane; the
    profile comes back as stored (direction normalised), records beyond the last segment are zero."""
    g, t = dev["getter"]["profile"], dev["getter"]["terrain"]
    assert np.array_equal(g["records"][:, 0, :9].reshape(B, 3, 3), t["frame"]) and np.array_equal(g["records"][:, 0, 9], t["plane"][:, 3])
    n, d, k, mu = pe.pack(dev["scen"])
    assert np.array_equal(g["n_knots"], n) and np.array_equal(g["knots"], k) and np.array_equal(g["mu"], mu)
    assert np.abs(g["dir"] - d / np.linalg.norm(d, axis=1, keepdims=True)).max() <= 2.3e-16
    for i in range(B):
        assert (g["records"][i, n[i] - 1:] == 0.0).all() and np.abs(g["records"][i, :n[i] - 1, 9]).max() < 1.0
        planes = pe.segment_planes(dev["scen"][i]["dir"], dev["scen"][i]["knots"])
        assert np.abs(g["records"][i, :n[i] - 1][:, [2, 5, 8, 9]] - planes).max() <= 1e-15


def test_api_behaviour(params):
    """Each validation error names the instance and keeps the profile in force; HB_ERR_STATE before hb_plant_reset, outside model 1 and next
    to respawn or a scenario with the slope / friction channel, in either order; the last setter of plane and profile wins and both clear
    the impulses; the profile survives hb_plant_reset and ends on leaving model 1."""
    from hunter_bipedal_control_amd.rollout import standing_configuration
    from hunter_bipedal_control_amd.solver import HunterHipError
    s = _solver(params, 3)
    try:
        foot_fn, qv_fn = _device_fns(s)
        flags = np.ones((3, 4), dtype=np.int32)
        q_stand = standing_configuration(params, 1, s)[0]
        scen = pe.scenarios(q_stand, qv_fn, foot_fn)[:3]
        n, d, k, mu = pe.pack(scen)
        mu = np.array([[0.7] * 4, [0.6, 0.5, 0.4, 0.3], [0.9, 0.5, 0.3, 0.05]])
        q0 = np.array([c["q0"] for c in scen])
        for call in (lambda: s.plant_set_terrain_profile(n, d, k, mu), s.plant_get_terrain_profile):
            with pytest.raises(HunterHipError, match=r"\(-3\)"):          # HB_ERR_STATE before hb_plant_reset
                call()
        s.plant_reset(q0, eps=pe.EPS)
        for call in (lambda: s.plant_set_terrain_profile(n, d, k, mu), s.plant_get_terrain_profile):
            with pytest.raises(HunterHipError, match=r"\(-3\)"):          # ... and in model 0
                call()
        cfg = _cfg(params)
        s.plant_set_contact_model(cfg)
        with pytest.raises(HunterHipError, match=r"\(-3\)"):              # no profile in force: nothing to report
            s.plant_get_terrain_profile()
        s.plant_set_terrain_profile(n, d, k, mu)
        assert np.array_equal(s.plant_get_terrain_profile()["segment"], [[0] * 5, [1, 1, 0, 0, 1], [2, 2, 0, 0, 2]])   # located at the set call
        bad = []
        for i, change in enumerate(("count", "dir", "knot")):
            n2, d2, k2 = n.copy(), d.copy(), k.copy()
            if change == "count":
                n2[i] = 1
            elif change == "dir":
                d2[i] = 0.0
            else:
                k2[i, 1, 0] = np.nan
            bad.append((i, n2, d2, k2, mu))
        k2 = k.copy()
        k2[1, 2, 0] = k2[1, 1, 0]                                        # spacing 0
        k3 = k.copy()
        k3[2, 2, 1] -= 0.01                                              # the riser steeper than sqrt(3)
        m = mu.copy()
        m[2, 3] = -1e-3
        n17 = n.copy()
        n17[0] = 17
        bad += [(1, n, d, k2, mu), (2, n, d, k3, mu), (2, n, d, k, m), (0, n17, d, k, mu)]
        for i, n2, d2, kk, m2 in bad:
            with pytest.raises(HunterHipError, match=rf"\(-1\).*instance {i}\b"):     # HB_ERR_ARG, the first offending instance named
                s.plant_set_terrain_profile(n2, d2, kk, m2)
            assert np.array_equal(s.plant_get_terrain_profile()["mu"], mu)            # the profile in force is kept
        # one ground at a time, the last setter wins, and each setter clears the impulses
        tau = np.array([c["tau"] for c in scen])
        ends = {}
        for how in ("warm", "set_again", "reset"):
            s.plant_reset(q0, eps=pe.EPS)
            for _ in range(3):
                s.plant_step(tau, flags, pe.DT, pe.SUBSTEPS)
            st = s.plant_state()
            if how == "set_again":                                        # (state kept, impulses cleared)
                s.plant_set_terrain_profile(n, d, k, mu)
                assert np.array_equal(s.plant_state()["q"], st["q"]) and np.array_equal(s.plant_state()["v"], st["v"])
            if how == "reset":
                s.plant_reset(st["q"], st["v"], eps=pe.EPS)
            s.plant_step(tau, flags, pe.DT, pe.SUBSTEPS)
            ends[how] = s.plant_state()
        for key in ("q", "v", "lam"):
            assert np.array_equal(ends["set_again"][key], ends["reset"][key]), key
        assert not np.array_equal(ends["warm"]["lam"], ends["reset"]["lam"])
        s.plant_reset(q0, eps=pe.EPS)                                     # the profile survives hb_plant_reset
        assert np.array_equal(s.plant_get_terrain_profile()["knots"], k)
        s.plant_set_contact_model(cfg)                                    # ... and a second mode-1 call
        assert np.array_equal(s.plant_get_terrain_profile()["mu"], mu)
        plane = np.tile([0.0, 0.0, 1.0, 0.0], (3, 1))
        s.plant_set_terrain(plane, mu)                                    # the plane replaces the profile
        with pytest.raises(HunterHipError, match=r"\(-3\)"):
            s.plant_get_terrain_profile()
        s.plant_step(tau, flags, pe.DT, pe.SUBSTEPS)
        on_plane = s.plant_state()["lam"]
        s.plant_set_terrain_profile(n, d, k, mu)                          # the profile replaces the plane: the getter of the plane reads level
        assert np.array_equal(s.plant_get_terrain()["plane"], np.tile([0.0, 0.0, 1.0, pe.CFG_GROUND], (3, 1)))
        s.plant_reset(q0, eps=pe.EPS)
        s.plant_step(tau, flags, pe.DT, pe.SUBSTEPS)
        assert not np.array_equal(s.plant_state()["lam"][1], on_plane[1])
        # respawn and the slope / friction scenario, in either order
        s.plant_set_episode(abi.make_episode_config())
        with pytest.raises(HunterHipError, match=r"\(-3\).*profile"):
            s.plant_set_respawn(abi.make_respawn_config(), q0, None)
        s.plant_set_terrain_profile(None, None, None, None)               # off
        s.plant_set_respawn(abi.make_respawn_config(), q0, None)
        with pytest.raises(HunterHipError, match=r"\(-3\).*respawn"):
            s.plant_set_terrain_profile(n, d, k, mu)
        s.plant_set_respawn(None, None, None)
        s.plant_set_terrain_profile(n, d, k, mu)
        # leaving model 1 switches the profile off
        s.plant_set_contact_model(None)
        s.plant_set_contact_model(cfg)
        with pytest.raises(HunterHipError, match=r"\(-3\)"):
            s.plant_get_terrain_profile()
    finally:
        s.close()


def test_resident_loop_on_profiles(params):
    """ResidentLoop(terrain=dict(profile=...), episode={...}), B = 4, 30 ticks of the whole closed loop: the run with profiles, gaits and
    commands rolled by one instance gives instance i + 1 what the first run gives instance i; the instance on the level profile == the same
    instance of a loop without a terrain; the episode record's height is n . q - d of the facet the getter reports under the base."""
    from hunter_bipedal_control_amd.rollout import ResidentLoop, curb_profile, stairs_profile
    knots = [curb_profile(0.0, 0.1), curb_profile(0.005, -0.01), stairs_profile(-0.01, 0.08, 3, 0.05), curb_profile(-0.01, 0.04)]
    dirs = np.array([[1.0, 0.0], [1.0, 0.0], [1.0, 0.0], [0.8, 0.6]])
    cmds = np.array([[0.0, 0.0, 0.0, 0.0], [0.2, 0.0, 0.0, 0.0], [0.3, 0.0, 0.0, 0.0], [0.2, 0.0, 0.0, 0.1]])
    gaits = ["stance", "trot", "trot", "trot"]
    hist, heights = [], None
    for shift, profile in ((0, True), (1, True), (0, False)):
        s = _solver(params, 4)
        try:
            roll = lambda a: [a[(i - shift) % 4] for i in range(4)]  # noqa: E731
            terrain = dict(profile=dict(dir=np.array(roll(list(dirs))), knots=roll(knots)), relative=True) if profile else None
            loop = ResidentLoop(s, params, roll(gaits), np.array(roll(list(cmds))), contact_config=dict(fall_height=0.3), terrain=terrain,
                                episode={})
            ticks = []
            for _ in range(30):
                loop.step()
                ticks.append(_outputs(s, False, False))
            hist.append(ticks)
            if profile and shift == 0:
                g, q = s.plant_get_terrain_profile(), s.plant_state()["q"]
                rec = np.array([g["records"][i, g["segment"][i, 4]] for i in range(4)])
                heights = (np.einsum("bx,bx->b", rec[:, [2, 5, 8]], q[:, :3]) - rec[:, 9], loop.episode())
        finally:
            s.close()
    for tick, (a, b, c) in enumerate(zip(*hist)):
        for k in a:
            assert np.array_equal(np.roll(a[k], 1, axis=0), b[k]), (k, tick)
            assert np.array_equal(a[k][0], c[k][0]), (k, tick)               # the level profile against no terrain
    last = hist[0][-1]
    assert not np.array_equal(last["lam"][1], hist[2][-1]["lam"][1])          # (a curb does change the run)
    want, ep = heights
    assert np.abs(ep["HEIGHT_LAST"] - want).max() <= 1e-12
