"""The joint model of the ground-contact plant on the device (hb_plant_set_joint_model, k_plant_joints) against the numpy twin of the
definition (tests/_jointemu.py) with the device's own rigid-body terms (eval_rbd / eval_foot_kinematics), up to
ResidentLoop(joint_model=...).

The model belongs to the context, so the cases run as passes of B = 4 distinct instances on one solver, 40 ticks each:
  "s": the default model on the plane — (s), and (s) turned about the vertical and moved on the plane (three more poses);
  "r": torque limit 2 N m — (r) with four torque sequences;
  "f": free fall, friction only, 60 sweeps — (f1), (f2), and both with the torque reversed;
  "l": free fall, damping 1, stops on — (l); the knee driven into its LOWER stop by -60 N m; the right knee; 6 N m (does not arrive);
  "o": a model with everything off on the cases (a), (b), (c) and the pushed robot of the contact tests, against no model at all.
Every instance of the first four passes is held to the twin on every tick."""
import numpy as np
import pytest

import _contactemu as ce
import _jointemu as je
from hunter_bipedal_control_amd import abi

pytestmark = pytest.mark.gpu

B = 4


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

    return (lambda rbd: s.eval_rbd(rbd)), foot_fn, qv_fn


def _dev(st, con, jo, i):
    """One instance's outputs in the shape the checks of tests/_jointemu.py take."""
    return dict(q=st["q"][i], v=st["v"][i], lam=st["lam"][i], touching=con["touching"][i], status=int(con["status"][i]),
                tau_applied=jo["tau_applied"][i], friction_torque=jo["friction_torque"][i], limit_torque=jo["limit_torque"][i],
                jresidual=float(jo["residual"][i]), jstatus=int(jo["status"][i]))


def _pass_cases(name, params, q_stand, qv_fn, foot_fn):
    mk = lambda n, seed=7: je.make_case(n, params, q_stand, qv_fn, foot_fn, np.random.default_rng(seed))  # noqa: E731
    if name == "s":
        cases = [mk("s") for _ in range(4)]
        for c, (x, y, yaw) in zip(cases[1:], ((1.0, -2.0, 0.4), (0.0, 0.0, -1.1), (3.0, 1.0, 0.0))):
            c["q0"] = c["q0"] + np.array([x, y, 0.0, yaw] + [0.0] * 12)     # (the statics torque does not change)
        return cases
    if name == "r":
        return [mk("r", seed) for seed in (7, 8, 9, 10)]
    if name == "f":
        cases = [mk("f1"), mk("f2"), mk("f1"), mk("f2")]
        for c in cases[2:]:
            tau = -c["tau_fn"](0)
            c["tau_fn"] = lambda tick, tau=tau: tau
        for c in cases:
            c["sweeps"] = je.SWEEPS["f1"]
        return cases
    cases = [mk("l") for _ in range(4)]
    for c, (joint, torque) in zip(cases, ((je.KNEE, je.L_TORQUE), (je.KNEE, -je.L_TORQUE), (8, je.L_TORQUE), (je.KNEE, 0.1 * je.L_TORQUE))):
        tau = np.zeros(10)
        tau[joint] = torque
        c["tau_fn"] = lambda tick, tau=tau: tau
    return cases


@pytest.fixture(scope="module")
def passes(params):
    """All passes, tick by tick: the device outputs and the twin's, the twin re-seeded with the device's (q, v, p) before every tick.
    Computed once, shared by the tests below and left unchanged."""
    from hunter_bipedal_control_amd.rollout import standing_configuration
    s = _solver(params)
    out = {}
    try:
        rbd_fn, foot_fn, qv_fn = _device_fns(s)
        q_stand = standing_configuration(params, 1, s)[0]
        commanded = np.ones((B, 4), dtype=np.int32)
        for name in ("s", "r", "f", "l"):
            cases = _pass_cases(name, params, q_stand, qv_fn, foot_fn)
            c0 = cases[0]
            q0, v0 = np.array([c["q0"] for c in cases]), np.array([c["v0"] for c in cases])
            s.plant_reset(q0, v0, eps=ce.EPS)
            s.plant_set_contact_model(je.contact_cfg(params, c0))
            s.plant_set_external_wrench(None)
            s.plant_set_joint_model(c0["jm"])
            tw = je.JointPlant(c0["jm"], rbd_fn, foot_fn, q0, v0, mu=c0["mu"], ground_z=c0["ground_z"], sweeps=c0["sweeps"])
            st, jo = s.plant_state(), s.plant_get_joints()
            assert not jo["status"].any() and not jo["tau_applied"].any()
            rec = []
            for tick in range(je.TICKS):
                tau = np.array([c["tau_fn"](tick) for c in cases])
                tw.q, tw.v, tw.p = st["q"].copy(), st["v"].copy(), st["lam"] * je.H
                tw.jp = np.hstack([jo["friction_torque"], jo["limit_torque"]]) * je.H
                tw.step(tau, commanded, je.DT, je.SUBSTEPS)
                s.plant_step(tau, commanded, je.DT, je.SUBSTEPS)
                st, con, jo = s.plant_state(), s.plant_contact(), s.plant_get_joints()
                twin = tw.record()
                rec.append(dict(tau=tau, dev=[_dev(st, con, jo, i) for i in range(B)], twin=[{k: x[i] for k, x in twin.items()} for i in range(B)]))
            out[name] = dict(cases=cases, rec=rec)
            if name == "r":
                out["sense"] = (s.plant_sense(want_outputs=True), jo["tau_applied"].copy(), tau)
        # (o): the contact tests' cases without a joint model and with the all-off one
        cases = [ce.make_case(n, q_stand, qv_fn, np.random.default_rng(7)) for n in "abcd"]
        q0, v0 = np.array([c["q0"] for c in cases]), np.array([c["v0"] for c in cases])
        wrench = np.array([np.zeros(6) if c["wrench"] is None else c["wrench"] for c in cases])
        cfg = abi.make_contact_config(params, mu=0.7, ground_z=0.0, erp=ce.ERP, sweeps=ce.SWEEPS)
        runs = {}
        for model in (None, je.all_off_model(params)):
            s.plant_reset(q0, v0, eps=ce.EPS)
            s.plant_set_contact_model(cfg)
            s.plant_set_external_wrench(wrench)
            s.plant_set_joint_model(model)
            rec = []
            for tick in range(40):
                tau = np.array([c["tau_fn"](tick) for c in cases])
                s.plant_step(tau, commanded, ce.DT, ce.SUBSTEPS)
                rec.append((s.plant_state(), s.plant_contact(), s.plant_get_joints(), tau))
            runs[model is not None] = rec
        out["o"] = runs
    finally:
        s.close()
    return out


@pytest.mark.parametrize("name", ["s", "r", "f", "l"])
def test_device_matches_the_twin_and_keeps_the_exact_properties(passes, name):
    """Every tick of every instance: q 1e-10; v, lambda, friction torque, limit torque 10 x the twin's measured sensitivity
    (tests/_jointemu.py); |friction torque| <= frictionloss (1 + 1e-14), s limit torque >= 0, tau_applied == numpy's clip bit for bit,
    the status bits against the arrays they summarise, the contact properties."""
    cases, worst = passes[name]["cases"], {}
    jm = je.model_dict(cases[0]["jm"])
    for tick, r in enumerate(passes[name]["rec"]):
        for i in range(B):
            d, t = r["dev"][i], r["twin"][i]
            for k, e in je.check_against_twin(d, t).items():
                worst[k] = max(worst.get(k, 0.0), e)
            je.check_exact_properties(d, r["tau"][i], jm, cases[i]["mu"])
            je.check_stop_sign(d, t["side"])
            je.check_status_bits(d, r["tau"][i], jm)
            assert np.array_equal(d["touching"], t["touching"]) and d["jstatus"] & 0xFFFFF == t["jstatus"] & 0xFFFFF, (tick, i)
    print(name, {k: f"{e:.2e}" for k, e in worst.items()})


def test_physics_on_the_device(passes):
    """(f1), (f2), (l), (r) as on the host (tests/_jointemu.py check_f1 / check_f2 / check_l / check_r_bits), on the instances that are
    those cases; the knee driven the other way ends on its lower stop with a positive limit torque."""
    rec, cases = passes["f"]["rec"], passes["f"]["cases"]
    jm = je.model_dict(cases[0]["jm"])
    for i in (0, 2):
        je.check_f1([r["dev"][i] for r in rec], [r["twin"][i] for r in rec], rec[0]["tau"][i][je.KNEE], jm)
    for i in (1, 3):
        je.check_f2([r["dev"][i] for r in rec], rec[0]["tau"][i][je.KNEE], jm)
    rec = passes["l"]["rec"]
    jm = je.model_dict(passes["l"]["cases"][0]["jm"])
    je.check_l([r["dev"][0] for r in rec], [r["twin"][0] for r in rec], jm)
    low, right, slow = (rec[-1]["dev"][i] for i in (1, 2, 3))
    assert low["jstatus"] & 0x3FF == 1 << je.KNEE and low["limit_torque"][je.KNEE] > 0.0 and abs(low["q"][6 + je.KNEE]) <= 1e-9
    assert right["jstatus"] & 0x3FF == 1 << 8 and right["limit_torque"][8] < 0.0
    assert slow["jstatus"] & 0x3FF == 0 and not slow["limit_torque"].any()
    clamped = 0
    for r in passes["r"]["rec"]:
        for i in range(B):
            je.check_r_bits(r["dev"][i], r["tau"][i])
            clamped += int((np.abs(r["tau"][i]) > 2.0).any())
    assert clamped == B * je.TICKS


def test_at_rest_the_limit_torque_cancels_the_applied_torque_on_the_device(params):
    """The (l) pass for 1250 ticks (5 sweeps, no read-back in between): the left knee on its upper stop, the right knee on its upper stop
    and the knee driven by 6 N m are at rest, and limit torque + applied torque is within the bound of tests/_jointemu.py check_l_rest
    (mass matrix of the end state from eval_rbd).  The knee driven into its lower stop swings further and still turns at 1.0e-6 rad/s on
    a base rotating at 4e-3 rad/s: it is not at rest by the check's definition and is left out."""
    from hunter_bipedal_control_amd.rollout import standing_configuration
    s = _solver(params)
    try:
        rbd_fn, foot_fn, qv_fn = _device_fns(s)
        cases = _pass_cases("l", params, standing_configuration(params, 1, s)[0], qv_fn, foot_fn)
        c0 = dict(cases[0], sweeps=je.SWEEPS["l_rest"])
        s.plant_reset(np.array([c["q0"] for c in cases]), np.array([c["v0"] for c in cases]), eps=ce.EPS)
        s.plant_set_contact_model(je.contact_cfg(params, c0))
        s.plant_set_joint_model(c0["jm"])
        tau, commanded = np.array([c["tau_fn"](0) for c in cases]), np.ones((B, 4), dtype=np.int32)
        for _ in range(je.REST_TICKS):
            s.plant_step(tau, commanded, je.DT, je.SUBSTEPS)
        st, con, jo = s.plant_state(), s.plant_contact(), s.plant_get_joints()
        for i, joint in ((0, je.KNEE), (2, 8), (3, je.KNEE)):
            d = _dev(st, con, jo, i)
            miss, bound = je.check_l_rest(d, qv_fn(d["q"], d["v"])[0], je.model_dict(c0["jm"]), joint)
            print(f"instance {i}: limit + applied {miss:.3e} N m, bound {bound:.3e}")
    finally:
        s.close()


@pytest.mark.parametrize("name", ["s", "r", "l"])
def test_momentum_rows_and_integration_on_ticks_of_one_substep(params, name):
    """160 ticks of one substep h of a pass: on every tick of every instance q+ = q + h v+ to 2 ulp and, on every joint row, limit +
    applied + friction torque = (Mh dv / h + nle + damping o v - J' lambda) with the device's own v+, lambda and torques and M, nle, J of
    eval_rbd at the start of the tick — without the twin (tests/_jointemu.py check_integration / check_momentum_row)."""
    from hunter_bipedal_control_amd.rollout import standing_configuration
    s = _solver(params)
    try:
        rbd_fn, foot_fn, qv_fn = _device_fns(s)
        cases = _pass_cases(name, params, standing_configuration(params, 1, s)[0], qv_fn, foot_fn)
        c0, jm = cases[0], je.model_dict(cases[0]["jm"])
        s.plant_reset(np.array([c["q0"] for c in cases]), np.array([c["v0"] for c in cases]), eps=ce.EPS)
        s.plant_set_contact_model(je.contact_cfg(params, c0))
        s.plant_set_joint_model(c0["jm"])
        commanded = np.ones((B, 4), dtype=np.int32)
        st = s.plant_state()
        for k in range(4 * je.TICKS):
            q, v = st["q"].copy(), st["v"].copy()
            M, nle, J = rbd_fn(ce.GroundPlant(None, foot_fn, q, v).rbd())[:3]
            s.plant_step(np.array([c["tau_fn"](k // 4) for c in cases]), commanded, je.H, 1)
            st, con, jo = s.plant_state(), s.plant_contact(), s.plant_get_joints()
            for i in range(B):
                d = _dev(st, con, jo, i)
                je.check_integration(d, q[i], je.H)
                je.check_momentum_row(d, v[i], M[i], nle[i], J[i], jm, je.H)
    finally:
        s.close()


def test_a_model_with_everything_off_is_no_model_at_all(passes):
    """(o): 40 ticks, each run on its own trajectory, within TOL_Q, TOL_V, TOL_LAM_REL of tests/_contactemu.py."""
    for (a, ca, ja, tau), (b, cb, jb, _) in zip(passes["o"][False], passes["o"][True]):
        scale = np.maximum(1.0, np.abs(a["lam"]).max(axis=1))
        errs = (np.abs(a["q"] - b["q"]).max(), np.abs(a["v"] - b["v"]).max(), (np.abs(a["lam"] - b["lam"]).max(axis=1) / scale).max())
        assert errs[0] <= ce.TOL_Q and errs[1] <= ce.TOL_V and errs[2] <= ce.TOL_LAM_REL, errs
        assert np.array_equal(ca["touching"], cb["touching"]) and np.array_equal(ca["status"], cb["status"])
        assert not jb["friction_torque"].any() and not jb["limit_torque"].any() and not jb["status"].any()
        assert np.array_equal(jb["tau_applied"], tau) and not ja["tau_applied"].any()     # (without a model the outputs stay zero)


def test_sense_reports_the_saturated_torque(passes):
    sense, tau_applied, tau = passes["sense"]
    assert np.array_equal(sense["joint_torque"], tau_applied) and np.array_equal(tau_applied, np.clip(tau, -2.0, 2.0))
    assert not np.array_equal(tau_applied, tau)


def test_error_codes_and_the_model_in_force_is_kept(params):
    from hunter_bipedal_control_amd.rollout import standing_configuration
    from hunter_bipedal_control_amd.solver import HunterHipError
    s = _solver(params, 2)
    try:
        good = abi.make_joint_model(params, torque_limit=2.0)
        for call in (lambda: s.plant_set_joint_model(good), lambda: s.plant_set_joint_model(None), s.plant_get_joints):
            with pytest.raises(HunterHipError, match=r"\(-3\)"):          # HB_ERR_STATE before hb_plant_reset
                call()
        q0 = standing_configuration(params, 2, s)
        s.plant_reset(q0)
        for call in (lambda: s.plant_set_joint_model(good), s.plant_get_joints):
            with pytest.raises(HunterHipError, match=r"\(-3\)"):          # ... and in contact model 0
                call()
        s.plant_set_contact_model(abi.make_contact_config(params))
        s.plant_set_joint_model(good)
        tau = np.full((2, 10), 5.0)
        bad = abi.make_joint_model(params)
        bad.reserved = 3
        refused = [bad] + [abi.make_joint_model(params, **kw) for kw in (dict(armature=-1.0), dict(damping=np.nan), dict(frictionloss=np.inf),
                                                                         dict(lower=3.0), dict(torque_limit=0.0), dict(torque_limit=np.nan),
                                                                         dict(limit_erp=1.5), dict(tol=-1.0), dict(limits=2))]
        for model in refused:
            with pytest.raises(HunterHipError, match=r"\(-1\)"):          # HB_ERR_ARG
                s.plant_set_joint_model(model)
            s.plant_step(tau, np.ones((2, 4), dtype=np.int32), 0.002, 4)  # the model in force is kept: the torque limit of 2 still clips
            assert (s.plant_get_joints()["tau_applied"] == 2.0).all()
        jo = s.plant_get_joints()
        assert (jo["status"] >> 10 & 0x3FF == 0x3FF).all() and jo["friction_torque"].any()
        s.plant_reset(q0)                                                 # the model survives hb_plant_reset, which clears the outputs
        jo = s.plant_get_joints()
        assert not any(jo[k].any() for k in jo)
        s.plant_step(tau, np.ones((2, 4), dtype=np.int32), 0.002, 4)
        assert (s.plant_get_joints()["tau_applied"] == 2.0).all()
        s.plant_set_joint_model(abi.make_joint_model(params, torque_limit=np.inf))   # +inf is allowed
        s.plant_step(tau, np.ones((2, 4), dtype=np.int32), 0.002, 4)
        assert (s.plant_get_joints()["tau_applied"] == 5.0).all()
        s.plant_set_joint_model(good)
        s.plant_set_contact_model(None)                                   # leaving contact model 1 switches the joint model off
        with pytest.raises(HunterHipError, match=r"\(-3\)"):
            s.plant_get_joints()
        s.plant_set_contact_model(abi.make_contact_config(params))
        s.plant_reset(q0)
        s.plant_step(tau, np.ones((2, 4), dtype=np.int32), 0.002, 4)
        assert not s.plant_get_joints()["tau_applied"].any()              # (no joint model: its outputs stay zero)
        assert np.array_equal(s.plant_sense(want_outputs=True)["joint_torque"], tau)
    finally:
        s.close()


def test_resident_loop_stands_with_the_default_joint_model(params):
    """ResidentLoop(contact_config={}, joint_model={}), 2 robots standing, 100 ticks: no HB_CONTACT_NONFINITE; no stop bit (the standing
    posture is >= 0.3 rad inside every range); tau_applied equals the commanded torque on every tick."""
    from hunter_bipedal_control_amd.rollout import ResidentLoop
    with pytest.raises(ValueError, match="contact_config"):
        ResidentLoop(None, params, ["stance"] * 2, np.zeros((2, 4)), joint_model={})
    s = _solver(params, 2)
    try:
        loop = ResidentLoop(s, params, ["stance", "stance"], np.zeros((2, 4)), contact_config={}, joint_model={})
        q = s.plant_state()["q"][:, 6:]
        m = params["model"]
        assert (q - np.array(m["q_lower"]) >= 0.3).all() and (np.array(m["q_upper"]) - q >= 0.3).all()
        for k in range(100):
            loop.step(want_outputs=True)
            jo, con = s.plant_get_joints(), s.plant_contact()
            assert (con["status"] & ce.NONFINITE == 0).all(), (k, con["status"])
            assert (jo["status"] & 0x3FF == 0).all(), (k, jo["status"])
            assert np.array_equal(jo["tau_applied"], loop.last["cmd"]["torque"]), k
            assert (jo["status"] >> 10 & 0x3FF == 0).all()
        st = s.plant_state()
        print("standing with the default joint model, tick 100: base height", st["q"][:, 2], "tilt", np.abs(st["q"][:, 4:6]).max(axis=1),
              "joint residual", jo["residual"], "friction torque", np.abs(jo["friction_torque"]).max())
    finally:
        s.close()
