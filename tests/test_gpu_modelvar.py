"""Per-instance model variation of the ground-contact plant on the device (hb_plant_set_model_variation; k_plant_varied, k_plant_varied_joints
and their hybrid forms) against the numpy twin of tests/_terrainemu.py on Oracle(params_i) — the twins of tests/test_modelvar_host.py — up to
ResidentLoop(model_variation=...).  B = 6: one scenario of mv.scenarios per instance, so one batch holds the nominal robot, two payloads, two
sets of mass scales and a landing, on a level floor, a slope and a tilted plane with four friction coefficients.

Measured on the MI355X (-s), worst over the six instances against the twin — ideal joints, held / hybrid: q 7.1e-15 / 4.3e-15, v 9.5e-12 /
8.2e-12, lambda 1.6e-11 / 2.9e-11; joint model: q 6.3e-14 / 3.3e-14, v 1.3e-10 / 6.7e-11, lambda 5.3e-09 / 2.8e-09, friction torque 1.0e-07 /
5.2e-08, limit torque 0 — every instance far inside the tolerance of its own model (tests/_modelvaremu.py).  The resident observation
against the oracle on the nominal model: 2.8e-17; against the oracle on the 10 kg robot's own model: 5.4e-03."""
import ctypes as C

import numpy as np
import pytest

import _actemu as ae
import _modelvaremu as mv
import _terrainemu as te
from hunter_bipedal_control_amd import abi

pytestmark = pytest.mark.gpu

B = mv.B
NTICKS = 14          # the landing (instance 5) touches down on tick 10


def _solver(params, batch=B):
    from hunter_bipedal_control_amd.solver import HunterSolver
    return HunterSolver(params, batch=batch, max_nodes=108)


def _cfg(params, **kw):
    # (mu and ground_z are NOT those of any scenario: a step on a terrain must not read them)
    return abi.make_contact_config(params, **{**dict(mu=0.31, ground_z=0.123, erp=te.ERP, sweeps=te.SWEEPS), **kw})


def _outputs(s, joints, hybrid=False):
    st, con = s.plant_state(), s.plant_contact()
    o = dict(q=st["q"], v=st["v"], lam=st["lam"], vdot=st["vdot"], rbd=st["rbd"], gap=con["gap"], point_vel=con["point_vel"].reshape(-1, 12),
             residual=con["residual"], touching=con["touching"], status=con["status"])
    if joints:
        jo = s.plant_get_joints()
        o.update(tau_applied=jo["tau_applied"], friction_torque=jo["friction_torque"], limit_torque=jo["limit_torque"], jresidual=jo["residual"],
                 jstatus=jo["status"])
    if hybrid:
        o.update({k: a for k, a in s.plant_get_actuator().items() if k != "last_timestamp"})
    return o


def _row(o, i):
    return {k: (float(a[i]) if k in ("residual", "jresidual") else a[i]) for k, a in o.items()}


def _arrays(scen):
    return {k: np.array([c[k] for c in scen]) for k in ("q0", "v0", "plane", "mu", "scale", "payload")}


def _start(s, params, a, joints, terrain=True, variation="given", **cfg):
    """variation: "given" — the scenarios'; "identity" — scales 1, payloads 0; None — none."""
    s.plant_reset(a["q0"], a["v0"], eps=te.EPS)
    s.plant_set_contact_model(_cfg(params, **cfg))
    s.plant_set_joint_model(abi.make_joint_model(params) if joints else None)
    s.plant_set_terrain(*((a["plane"], a["mu"]) if terrain else (None, None)))
    if variation == "given":
        s.plant_set_model_variation(a["scale"], a["payload"])
    elif variation == "identity":
        s.plant_set_model_variation(np.ones_like(a["scale"]), np.zeros_like(a["payload"]))
    else:
        s.plant_set_model_variation(None, None)


def _command(q, tau):
    return dict(pos_des=q[:, 6:].copy(), vel_des=np.zeros((len(q), 10)), kp=np.full((len(q), 10), 5.0), kd=np.full((len(q), 10), 0.05), tau_ff=tau)


def _step(s, hybrid, tau, flags):
    if hybrid:
        s.plant_step_hybrid(_command(s.plant_state()["q"], tau), flags, te.DT, te.SUBSTEPS)
    else:
        s.plant_step(tau, flags, te.DT, te.SUBSTEPS)


@pytest.fixture(scope="module")
def scen(params):
    return mv.scenarios(params)


@pytest.fixture(scope="module")
def dev(params, scen):
    """One context, B = 6.  passes[joints, hybrid][tick] = dict(dev, twin): the device on the six scenarios and the six twins (one per model),
    re-seeded with the device's (q, v, p) before every tick; a hybrid tick of the twin is `substeps` steps of one substep with the law
    evaluated from the twin's own state before each.  identity[terrain, joints, hybrid] = (without, with): the context without a variation
    and with the identity variation over 10 ticks.  Shared by the tests below and left unchanged."""
    s = _solver(params)
    out = dict(passes={}, identity={})
    try:
        a = _arrays(scen)
        flags = np.ones((B, 4), dtype=np.int32)
        for joints in (False, True):
            for hybrid in (False, True):
                _start(s, params, a, joints)
                if not out.get("image"):
                    out["image"] = s.plant_model_variation()
                twins = [mv.twin_of(c, joints, params) for c in scen]
                rec, o = [], _outputs(s, joints, hybrid)
                for tick in range(NTICKS):
                    tau = np.array([c["tau_fn"](tick) for c in scen])
                    cmd = _command(o["q"], tau)
                    p = te.to_frame(o["lam"] * te.H, a["plane"]).reshape(B, 12)
                    rows = []
                    for i, tw in enumerate(twins):
                        tw.q[0], tw.v[0], tw.p[0] = o["q"][i], o["v"][i], p[i]
                        if joints:
                            tw.jp[0] = np.concatenate([o["friction_torque"][i], o["limit_torque"][i]]) * te.H
                        if hybrid:
                            for _ in range(te.SUBSTEPS):
                                tw.step(ae.law({k: x[i:i + 1] for k, x in cmd.items()}, tw.q, tw.v), te.H, 1)
                        else:
                            tw.step(tau[i:i + 1])
                        rows.append({k: x[0] for k, x in tw.record().items()})
                    _step(s, hybrid, tau, flags)
                    o = _outputs(s, joints, hybrid)
                    rec.append(dict(dev=o, twin=rows, tau=tau))
                out["passes"][joints, hybrid] = rec
                for terrain in (False, True):
                    runs = []
                    for variation in (None, "identity"):
                        _start(s, params, a, joints, terrain=terrain, variation=variation, mu=0.4, ground_z=0.001)
                        ticks = []
                        for tick in range(10):
                            _step(s, hybrid, rec[tick]["tau"], flags)
                            ticks.append(_outputs(s, joints, hybrid))
                        runs.append(ticks)
                    out["identity"][terrain, joints, hybrid] = runs
        out.update(arrays=a)
    finally:
        s.close()
    return out


@pytest.mark.parametrize("hybrid", [False, True])
@pytest.mark.parametrize("joints", [False, True])
def test_device_matches_the_twin_of_each_model(dev, joints, hybrid):
    """q 1e-10; v, lambda and with the joint model friction / limit torque 10 x the sensitivity of the twin on the instance's own model, every
    instance on every tick, in the four forms."""
    worst = {}
    for r in dev["passes"][joints, hybrid]:
        for i in range(B):
            for k, e in mv.check_against_twin(_row(r["dev"], i), r["twin"][i], joints, i).items():
                worst[k] = max(worst.get(k, 0.0), e)
    assert any(np.abs(r["dev"]["lam"]).max() > 1.0 for r in dev["passes"][joints, hybrid])
    print("joint model", joints, "hybrid", hybrid, "worst against the twin:", {k: f"{e:.2e}" for k, e in worst.items()})


def test_the_getter_returns_the_host_composition(params, dev, scen):
    """hb_plant_get_model_variation == csrc/hb_modelvar.hpp compiled for the host, entry for entry (the host builds the image); instance 0 is
    the nominal model."""
    a = dev["arrays"]
    got = mv.emu_compose(C.CDLL(str(mv.build())), abi.make_model(params), a["scale"], a["payload"])
    img = dev["image"]
    for i in range(B):
        mass, com, inertia = mv.arrays_of(got["model"][i])
        assert np.array_equal(img["mass"][i], mass) and np.array_equal(img["com"][i], com) and np.array_equal(img["inertia"][i], inertia)
    assert np.array_equal(img["total_mass"], got["total_mass"])
    assert np.array_equal(img["mass"][0], np.array(params["model"]["mass"])) and img["total_mass"][1] > img["total_mass"][0] + 4.9


@pytest.mark.parametrize("hybrid", [False, True])
@pytest.mark.parametrize("joints", [False, True])
@pytest.mark.parametrize("terrain", [False, True])
def test_the_identity_variation_is_no_variation(dev, terrain, joints, hybrid):
    """Scales 1 and zero payloads on every instance: every output of hb_plant_step / hb_plant_step_hybrid == the context without a variation
    (other kernels), with and without a terrain and the joint model, 10 ticks."""
    without, with_variation = dev["identity"][terrain, joints, hybrid]
    for tick, (x, y) in enumerate(zip(without, with_variation)):
        for k in x:
            assert np.array_equal(x[k], y[k]), (k, tick)
    assert any(np.abs(x["lam"]).max() > 1.0 for x in without)


def test_scenarios_tiled_and_rolled_by_one_instance(params, scen):
    """B = 65, the six scenarios tiled: the run with scenarios and inputs rolled by one instance gives instance i + 1 what instance i had, on
    every output of 8 ticks; ideal joints with the held torque and the joint model with the hybrid step."""
    n = 65
    tiled = [scen[i % B] for i in range(n)]
    flags = np.ones((n, 4), dtype=np.int32)
    s = _solver(params, n)
    try:
        for joints, hybrid in ((False, False), (True, True)):
            hist = []
            for shift in (0, 1):
                order = [tiled[(i - shift) % n] for i in range(n)]
                _start(s, params, _arrays(order), joints)
                ticks = []
                for tick in range(8):
                    _step(s, hybrid, np.array([c["tau_fn"](tick) for c in order]), flags)
                    ticks.append(_outputs(s, joints, hybrid))
                hist.append(ticks)
            for tick, (x, y) in enumerate(zip(*hist)):
                for k in x:
                    assert np.array_equal(np.roll(x[k], 1, axis=0), y[k]), (k, tick)
            last = hist[0][-1]
            assert not np.array_equal(last["lam"][0], last["lam"][1]) and np.array_equal(last["lam"][0], last["lam"][B])
    finally:
        s.close()


def test_resident_loop_keeps_the_nominal_robot_and_the_nominal_view(params, oracle):
    """ResidentLoop(model_variation=...), B = 4, ground, joint model, payloads (0, 2, 5, 10) kg on the base, 30 ticks of the whole closed loop:
    instance 0's plant_state, plant_contact and WBC solution == the loop without a variation; run(30) == 30 x step(); and the resident
    observation the last step wrote is Oracle(nominal).centroidal_state_from_rbd of the returned rbd (1e-12, the tolerance of
    tests/test_oracle_estimator.py) for every instance — the controller's view keeps the nominal model — while the centroidal state on
    the payload robot's own model is somewhere else."""
    from hunter_bipedal_control_amd.rollout import ResidentLoop, payload_on_base
    from oracle.pyoracle import Oracle
    payload = payload_on_base([0.0, 2.0, 5.0, 10.0], [0.0, 0.0, 0.10])
    cmds = np.tile([0.2, 0.0, 0.0, 0.0], (4, 1))
    hist, ends = {}, {}
    for how in ("without", "stepped", "run"):
        s = _solver(params, 4)
        try:
            loop = ResidentLoop(s, params, ["trot"] * 4, cmds, contact_config=dict(fall_height=0.3), joint_model={},
                                model_variation=None if how == "without" else dict(payload=payload))
            if how == "run":
                loop.run(30)
            else:
                ticks = []
                for _ in range(30):
                    loop.step()
                    ticks.append(dict(state=s.plant_state(), contact=s.plant_contact(), wbc=s.get_wbc_solution()[0]))
                hist[how] = ticks
            ends[how] = dict(state=s.plant_state(), contact=s.plant_contact(), wbc=s.get_wbc_solution()[0])
            if how == "stepped":
                assert (np.diff(s.plant_model_variation()["total_mass"]) > 1.9).all()
                s.reset_resident()                        # the cold start copies the resident observation into node 0
                x0 = s.get_solution()[0][:, 0]
                rbd = ends[how]["state"]["rbd"]
                assert np.abs(x0 - oracle.centroidal_state_from_rbd(rbd)).max() <= 1e-12
                model_3, _, _ = mv.compose_numpy(params["model"], None, payload[3])
                own = Oracle(mv.params_of(params, model_3)).centroidal_state_from_rbd(rbd[3:4])[0]
                print("resident observation against the oracle on the nominal model:", np.abs(x0 - oracle.centroidal_state_from_rbd(rbd)).max(),
                      "instance 3 against the oracle on its own model:", np.abs(x0[3] - own).max())
                assert np.abs(x0[3] - own).max() > 1e-9
        finally:
            s.close()
    for tick, (x, y) in enumerate(zip(hist["without"], hist["stepped"])):
        for grp in ("state", "contact"):
            for k in x[grp]:
                assert np.array_equal(x[grp][k][0], y[grp][k][0]), (grp, k, tick)
        assert np.array_equal(x["wbc"][0], y["wbc"][0]), tick
    last = hist["stepped"][-1]["state"]
    assert not np.array_equal(last["q"][0], last["q"][3])                 # (the payload does change the run)
    for grp in ("state", "contact"):
        for k in ends["run"][grp]:
            assert np.array_equal(ends["run"][grp][k], ends["stepped"][grp][k]), (grp, k)
    assert np.array_equal(ends["run"]["wbc"], ends["stepped"]["wbc"])


def test_api_behaviour(params, scen):
    """Error codes (the variation in force is kept after a refused call), the getter with and without a variation, survival over
    hb_plant_reset and a second hb_plant_set_contact_model, off by leaving model 1 and by NULL / NULL, nothing cleared by a set call: the
    impulses stay a warm start and an episode record is not restarted."""
    from hunter_bipedal_control_amd.solver import HunterHipError
    n = 3
    s = _solver(params, n)
    try:
        a = {k: x[[1, 2, 3]] for k, x in _arrays(scen).items()}
        flags = np.ones((n, 4), dtype=np.int32)
        calls = (lambda: s.plant_set_model_variation(a["scale"], a["payload"]), s.plant_model_variation)
        for call in calls:
            with pytest.raises(HunterHipError, match=r"\(-3\)"):          # HB_ERR_STATE before hb_plant_reset
                call()
        s.plant_reset(a["q0"], a["v0"], eps=te.EPS)
        for call in calls:
            with pytest.raises(HunterHipError, match=r"\(-3\)"):          # ... and in model 0: the pinned stub has no varied form
                call()
        cfg = _cfg(params)
        s.plant_set_contact_model(cfg)
        nominal = s.plant_model_variation()                               # no variation: the nominal model repeated
        model = params["model"]
        for i in range(n):
            assert np.array_equal(nominal["mass"][i], np.array(model["mass"])) and np.array_equal(nominal["com"][i], np.array(model["com"]))
            assert np.array_equal(nominal["inertia"][i], np.array(model["inertia"]))
        total = 0.0
        for m in model["mass"]:
            total += m
        assert (nominal["total_mass"] == total).all()
        s.plant_set_model_variation(a["scale"], a["payload"])
        inforce = s.plant_model_variation()
        assert not np.array_equal(inforce["mass"], nominal["mass"])
        bad = []
        for i, (which, col, val) in enumerate([("scale", 4, np.nan), ("payload", 2, np.inf), ("scale", 0, 0.0)]):
            x = {k: a[k].copy() for k in ("scale", "payload")}
            x[which][i:, col] = val                                        # (instance i and every later one offend: the first is named)
            bad.append((i, x["scale"], x["payload"]))
        for i, col, val in ((1, 0, -1e-3), (0, 4, -1e-6)):                 # m_p < 0; a negative diagonal entry of I_p
            p = a["payload"].copy()
            p[i, col] = val
            bad.append((i, a["scale"], p))
        p = a["payload"].copy()
        p[2, 0], p[2, 4:10] = 0.0, [0.01, 0.0, 0.0, 0.01, 0.0, 0.01]      # an inertia without a mass
        bad.append((2, None, p))
        p = a["payload"].copy()
        p[0, 4:10] = [1.0, 0.9, 0.9, 1.0, -0.9, 1.0]                       # every 2 x 2 minor positive, det < 0
        bad.append((0, a["scale"], p))
        neg = a["scale"].copy()
        neg[1, 7] = -1.1
        bad.append((1, neg, None))
        for i, sc, pl in bad:
            with pytest.raises(HunterHipError, match=rf"\(-1\).*instance {i}\b"):     # HB_ERR_ARG, the first offending instance named
                s.plant_set_model_variation(sc, pl)
            now = s.plant_model_variation()
            assert all(np.array_equal(now[k], inforce[k]) for k in now)                # the variation in force is kept
        tau = np.array([c["tau_fn"](0) for c in (scen[1], scen[2], scen[3])])
        s.plant_set_terrain(a["plane"], a["mu"])
        s.plant_step(tau, flags, te.DT, te.SUBSTEPS)
        st = s.plant_state()
        s.plant_reset(st["q"], st["v"], eps=te.EPS)                       # the variation survives hb_plant_reset
        s.plant_set_contact_model(cfg)                                    # ... and a second mode-1 call
        now = s.plant_model_variation()
        assert all(np.array_equal(now[k], inforce[k]) for k in now)
        s.plant_set_model_variation(None, None)                           # off by NULL / NULL
        assert np.array_equal(s.plant_model_variation()["mass"], nominal["mass"])
        s.plant_set_model_variation(None, a["payload"])                   # either argument alone
        assert np.array_equal(s.plant_model_variation()["mass"][:, 1:], nominal["mass"][:, 1:])
        s.plant_set_contact_model(None)                                   # leaving model 1 switches it off
        s.plant_set_contact_model(cfg)
        assert np.array_equal(s.plant_model_variation()["mass"], nominal["mass"])
        # a set call clears nothing: after three ticks, setting the identity variation leaves the next tick what it is without the call
        # (a cold start differs), and the episode record goes on counting
        ends = {}
        for how in ("plain", "set", "reset"):
            s.plant_reset(a["q0"], a["v0"], eps=te.EPS)
            s.plant_set_terrain(a["plane"], a["mu"])
            s.plant_set_model_variation(None, None)
            s.plant_set_episode(abi.make_episode_config())
            for _ in range(3):
                s.plant_step(tau, flags, te.DT, te.SUBSTEPS)
            if how == "set":
                s.plant_set_model_variation(np.ones((n, abi.NBODY)), np.zeros((n, abi.HB_PAYLOAD_SIZE)))
                assert (s.plant_episode()["STEPS"] == 3).all()
            if how == "reset":
                st = s.plant_state()
                s.plant_reset(st["q"], st["v"], eps=te.EPS)
            s.plant_step(tau, flags, te.DT, te.SUBSTEPS)
            ends[how] = (s.plant_state(), s.plant_episode()["STEPS"].copy())
        for k in ("q", "v", "lam"):
            assert np.array_equal(ends["plain"][0][k], ends["set"][0][k]), k
        assert not np.array_equal(ends["plain"][0]["lam"], ends["reset"][0]["lam"])
        assert (ends["set"][1] == 4).all() and (ends["reset"][1] == 1).all()
        s.plant_set_episode(None)
    finally:
        s.close()
