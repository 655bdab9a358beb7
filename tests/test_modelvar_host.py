"""CPU: the per-instance model variation of the ground-contact plant (hb_plant_set_model_variation).  The composition of csrc/hb_modelvar.hpp
(compiled for the host, tests/host_emu/modelvaremu.cpp) against a second composition in numpy (tests/_modelvaremu.py compose_numpy), and the
host build of the plant's step routines on the composed model against the numpy twin of tests/_terrainemu.py on Oracle(params_i).  Six
scenarios, one instance each (mv.scenarios): 0 no variation; 1 point payload 5 kg; 2 payload 10 kg with an inertia on the pitch / roll plane
with four friction coefficients; 3 base x 0.9, links x 1.2; 4 seeded per-body scales and 3 kg on the 0.2 rad slope; 5 instance 1's payload,
landing from 2 mm.  20 ticks of 4 substeps, 30 sweeps, ideal joints and the default joint model.

Measured (this file, -s): host build against the twin, worst over the six scenarios — ideal joints q 5.3e-15, v 7.6e-12, lambda 3.2e-11;
joint model q 6.0e-14, v 1.2e-10, lambda 5.1e-09, friction torque 9.6e-08, limit torque 0.  Against the twin on the NOMINAL model, largest
|dv| over the ticks of scenarios 1 - 5 [m/s]: ideal joints 7.9e-02, 3.6e-01, 9.1e-03, 3.5e-02, 1.4e-01 (100 x the tolerance: 6.7e-05, 2.4e-03,
1.9e-05, 1.9e-05, 6.7e-05); joint model 2.1e-02, 2.6e-01, 8.5e-05, 1.4e-02, 1.6e-01 (1.8e-05, 7.9e-05, 5.3e-06, 8.5e-05, 1.8e-05); scenario 0
3.8e-12 / 3.9e-12.  Weight after 40 substeps, sum f_z / (total_mass_i g) - 1, scenarios 0 / 1 / 3: ideal joints twin -6.4e-09 / -4.9e-09 /
-6.5e-09 and the host build the same to these digits; joint model -2.7e-05 / +2.5e-05 / -6.1e-05 on both (the friction rows carry the rest)."""
import ctypes as C

import numpy as np
import pytest

import _modelvaremu as mv
import _terrainemu as te
from hunter_bipedal_control_amd import abi

EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def env(params):
    lib = C.CDLL(str(mv.build()))
    scen = mv.scenarios(params)
    mdl = abi.make_model(params)
    scale, payload = mv.variations()
    return dict(lib=lib, telib=C.CDLL(str(te.build())), mdl=mdl, params=params, scen=scen, scale=scale, payload=payload,
                composed=mv.emu_compose(lib, mdl, scale, payload), jm=abi.make_joint_model(params))


def _cfg(params, **kw):
    # (mu and ground_z are NOT those of any scenario: the varied forms are terrain forms and must not read them)
    return abi.make_contact_config(params, **{**dict(mu=0.31, ground_z=0.123, erp=te.ERP, sweeps=te.SWEEPS), **kw})


def _compare(lib, mdl, model, scale, payload):
    """The host build of the composition against compose_numpy on one instance: every entry within 16 roundings of the largest term of
    its own sum -> the composed abi.HbModel."""
    got = mv.emu_compose(lib, mdl, scale, payload)
    want, total, terms = mv.compose_numpy(model, scale, payload)
    mass, com, inertia = mv.arrays_of(got["model"][0])
    wm, wc, wi = (np.array(want[k]) for k in ("mass", "com", "inertia"))
    tm, tc, ti = np.abs(wm), np.abs(wc), np.abs(wi)              # links: one product, the entry is its own term
    tm[0], tc[0], ti[0] = terms["mass0"], terms["com0"], terms["inertia0"]
    assert (np.abs(mass - wm) <= 16 * EPS * tm).all(), ("mass", np.abs(mass - wm) / (EPS * tm))
    assert (np.abs(com - wc) <= 16 * EPS * tc).all(), ("com", np.abs(com - wc))
    assert (np.abs(inertia - wi) <= 16 * EPS * ti).all(), ("inertia", np.abs(inertia - wi), EPS * ti)
    assert abs(got["total_mass"][0] - total) <= 16 * EPS * wm.max()
    for k in ("joint_origin", "joint_axis", "q_lower", "q_upper", "qd_limit", "contact_offset"):
        assert np.array_equal(np.array([list(np.atleast_1d(r)) for r in getattr(got["model"][0], k)]).ravel(), np.array(model[k], dtype=float).ravel()), k
    assert got["model"][0].gravity == model["gravity"]
    return got


def test_composition_matches_the_second_implementation(env):
    """The six scenarios and 20 seeded random variations (scales in [0.5, 1.5], payloads up to 10 kg within 0.15 m of the base origin per axis
    with a random positive semidefinite inertia; a quarter each without scales / without a payload)."""
    model = env["params"]["model"]
    for i in range(mv.B):
        _compare(env["lib"], env["mdl"], model, env["scale"][i], env["payload"][i])
    rng = np.random.default_rng(2201)
    for k in range(20):
        scale = rng.uniform(0.5, 1.5, abi.NBODY)
        a = 0.1 * rng.standard_normal((3, 3))
        ip = a @ a.T
        payload = np.concatenate([[rng.uniform(0.1, 10.0)], rng.uniform(-0.15, 0.15, 3), mv._six(ip)])
        _compare(env["lib"], env["mdl"], model, None if k % 4 == 1 else scale, None if k % 4 == 2 else payload)


def test_the_unvaried_instance_is_a_byte_copy(env):
    """Scales 1.0 and no payload mass (whatever the payload's position says): the composed model is abi.make_model(params) byte for byte,
    the device record the nominal record byte for byte (total_mass is not summed again), also inside a batch of varied instances."""
    nominal = bytes(abi.make_model(env["params"]))
    c = env["composed"]
    assert bytes(c["model"][0]) == nominal and c["record"][0] == c["nominal"]
    for i in range(1, mv.B):
        assert bytes(c["model"][i]) != nominal and c["record"][i] != c["nominal"]
    moved = np.zeros(abi.HB_PAYLOAD_SIZE)
    moved[1:4] = [0.1, -0.2, 0.3]
    for scale, payload in ((np.ones(abi.NBODY), None), (None, moved), (np.ones(abi.NBODY), moved)):
        got = mv.emu_compose(env["lib"], env["mdl"], scale, payload)
        assert bytes(got["model"][0]) == nominal and got["record"][0] == got["nominal"]


def test_every_refusal_names_the_first_offending_instance(env):
    """B = 4 with instance 2 (and instance 3) offending: non-finite scale / payload entry, s_b <= 0, m_p < 0, a massless inertia, I_p with a
    negative diagonal entry, a negative 2 x 2 minor, a negative determinant.  Rank-deficient inertias within the slack are accepted."""
    ok_s, ok_p = np.ones((4, abi.NBODY)), np.zeros((4, abi.HB_PAYLOAD_SIZE))
    ok_p[:, 0] = 1.0

    def bad(which, col, val):
        s, p = ok_s.copy(), ok_p.copy()
        (s if which == "s" else p)[2, col] = val
        (s if which == "s" else p)[3, col] = val
        return s, p

    cases = [bad("s", 4, np.nan), bad("s", 0, np.inf), bad("p", 2, np.nan), bad("p", 7, -np.inf), bad("s", 3, 0.0), bad("s", 10, -1.2), bad("p", 0, -1e-3),
             bad("p", 4, -1e-6)]
    s, p = ok_s.copy(), ok_p.copy()
    p[2:, 0], p[2:, 4:10] = 0.0, [0.01, 0.0, 0.0, 0.01, 0.0, 0.01]         # inertia without mass
    cases.append((s, p))
    p = ok_p.copy()
    p[2:, 4:10] = [0.01, 0.02, 0.0, 0.01, 0.0, 0.01]                        # xx yy - xy^2 < 0
    cases.append((ok_s, p))
    p = ok_p.copy()
    p[2:, 4:10] = [1.0, 0.9, 0.9, 1.0, -0.9, 1.0]                           # every 2 x 2 minor positive, det < 0
    cases.append((ok_s, p))
    for s, p in cases:
        with pytest.raises(mv.Refused) as e:
            mv.emu_compose(env["lib"], env["mdl"], s, p)
        assert e.value.instance == 2, e.value
    with pytest.raises(mv.Refused) as e:                                    # scales alone / payload alone
        mv.emu_compose(env["lib"], env["mdl"], bad("s", 1, -1.0)[0], None)
    assert e.value.instance == 2
    with pytest.raises(mv.Refused) as e:
        mv.emu_compose(env["lib"], env["mdl"], None, bad("p", 0, -2.0)[1])
    assert e.value.instance == 2
    v = np.array([0.3, -0.2, 0.1])
    for ip in (np.zeros((3, 3)), np.outer(v, v), np.outer(v, v) + np.outer([0.0, 0.1, 0.2], [0.0, 0.1, 0.2])):   # rank 0, 1, 2
        p = ok_p.copy()
        p[:, 4:10] = mv._six(ip)
        mv.emu_compose(env["lib"], env["mdl"], ok_s, p)


@pytest.fixture(scope="module")
def runs(env):
    """{joints: [per scenario: list of dict(dev, twin, nominal, tau, q, v, p, jp) per tick]}: the host build of the plant on the composed
    model over 20 ticks of every scenario; the twin on Oracle(params_i) and the twin on the nominal model, both re-seeded with the host
    build's (q, v, p) before every tick.  Shared by the tests below and left unchanged."""
    out = {}
    nominal_qv = env["scen"][0]["qv_fn"]
    for joints in (False, True):
        jm = env["jm"] if joints else None
        out[joints] = []
        for i, sc in enumerate(env["scen"]):
            rec = te.record_of(sc["plane"], sc["mu"])
            twins = [mv.twin_of(sc, joints, env["params"]), mv.twin_of(sc, joints, env["params"], nominal_qv)]
            q, v, p, jp, st, ticks = sc["q0"].copy(), sc["v0"].copy(), np.zeros(12), np.zeros(20), 0, []
            for tick in range(mv.TICKS):
                tau = sc["tau_fn"](tick)
                o = te.emu_step(env["telib"], env["composed"]["model"][i], _cfg(env["params"]), rec, q, v, p, tau, None, st, jm, jp)
                recs = []
                for tw in twins:
                    tw.q[0], tw.v[0], tw.p[0], tw.jp[0] = q, v, p, jp
                    tw.step(tau[None])
                    recs.append({k: a[0] for k, a in tw.record().items()})
                ticks.append(dict(dev=o, twin=recs[0], nominal=recs[1], tau=tau, q=q, v=v, p=p, jp=jp))
                q, v, p, st = o["q"], o["v"], o["p"], o["status"]
                jp = o["jp"] if joints else jp
            out[joints].append(ticks)
    return out


@pytest.mark.parametrize("joints", [False, True])
def test_host_build_on_the_varied_model_matches_its_twin(env, runs, joints):
    """q 1e-10; v, lambda and with the joint model friction / limit torque 10 x the twin's measured sensitivity (tests/_modelvaremu.py)."""
    worst = {}
    for i, ticks in enumerate(runs[joints]):
        for t in ticks:
            for k, e in mv.check_against_twin(t["dev"], t["twin"], joints, i).items():
                worst[k] = max(worst.get(k, 0.0), e)
    print("joint model", joints, "worst against the twin:", {k: f"{e:.2e}" for k, e in worst.items()})


@pytest.mark.parametrize("joints", [False, True])
def test_the_nominal_twin_turns_the_comparison_red(env, runs, joints):
    """The comparison can tell a varied robot from the nominal one: on each of the scenarios 1 - 5 the twin on the nominal model differs
    from the code by more than 100 x the tolerance in v; on scenario 0 it is the same twin."""
    worst = [max(mv.errors_against_twin(t["dev"], t["nominal"])["v"] for t in ticks) for ticks in runs[joints]]
    print("joint model", joints, "largest |dv| against the nominal twin per scenario:", [f"{w:.2e}" for w in worst])
    assert worst[0] <= mv.tol_of(joints, 0)["v"]
    for i in range(1, mv.B):
        assert worst[i] > 100 * mv.tol_of(joints, i)["v"], (i, worst[i])


@pytest.mark.parametrize("joints", [False, True])
def test_base_momentum_rows_hold_on_the_instance_model(env, runs, joints):
    """A tick of ONE substep from the start state of every tick of every scenario (a base force on the odd ticks): (M_i dv / h + nle_i)[0:3]
    = sum lambda_c + F_ext to 64 roundings with M_i, nle_i from Oracle(params_i); on the loaded ticks of scenarios 1 - 5 the nominal M, nle
    miss it."""
    jm = env["jm"] if joints else None
    nominal_qv, red = env["scen"][0]["qv_fn"], np.zeros(mv.B, dtype=int)
    for i, sc in enumerate(env["scen"]):
        rec = te.record_of(sc["plane"], sc["mu"])
        for k, t in enumerate(runs[joints][i]):
            wrench = np.array([12.0, -7.0, 3.0, 0.0, 0.0, 0.0]) if k % 2 else None
            o = te.emu_step(env["telib"], env["composed"]["model"][i], _cfg(env["params"]), rec, t["q"], t["v"], t["p"], t["tau"], wrench, 0, jm, t["jp"],
                            dt=te.H, substeps=1)
            M, nle = sc["qv_fn"](t["q"], t["v"])[:2]
            te.check_base_momentum(o["lam"], o["v"], t["v"], M, nle, te.H, wrench)
            try:
                te.check_base_momentum(o["lam"], o["v"], t["v"], *nominal_qv(t["q"], t["v"])[:2], te.H, wrench)
            except AssertionError:
                red[i] += 1
    assert red[0] == 0 and (red[1:] >= 1).all(), red


@pytest.mark.parametrize("joints", [False, True])
def test_the_ground_carries_the_instance_weight(env, runs, joints):
    """Scenarios 0, 1, 3 stand on their plane under the statics torque of their own model: after 40 substeps | sum f_z / (total_mass_i g) - 1 |
    <= 1e-3 (the bound of the ground-contact plant's own weight check) — on the free-running twin first, then on the host build; against the
    nominal total mass the payload and the heavier legs show."""
    g = env["params"]["model"]["gravity"]
    for i in mv.STANDING:
        sc = env["scen"][i]
        tw = mv.twin_of(sc, joints, env["params"])
        for tick in range(10):
            tw.step(sc["tau_fn"](tick)[None])
        twin = mv.weight_ratio(tw.lam[0], sc["total_mass"], g) - 1.0
        assert abs(twin) <= 1e-3, ("twin", i, twin)
        dev = mv.weight_ratio(runs[joints][i][9]["dev"]["lam"], env["composed"]["total_mass"][i], g) - 1.0
        print(f"joint model {joints} scenario {i}: weight ratio - 1: twin {twin:.2e} host build {dev:.2e}")
        assert abs(dev) <= 1e-3, (i, dev)
        if i:
            assert abs(mv.weight_ratio(runs[joints][i][9]["dev"]["lam"], env["composed"]["total_mass"][0], g) - 1.0) > 1e-2


def test_the_resident_loop_argument_and_the_payload_helper():
    """ResidentLoop refuses a model variation without the ground-contact plant before it touches the solver; payload_on_base packs [B][10]."""
    from hunter_bipedal_control_amd.rollout import ResidentLoop, payload_on_base
    with pytest.raises(ValueError):
        ResidentLoop(None, {}, ["stance"], np.zeros((1, 4)), model_variation=dict(payload=np.zeros((1, 10))))
    p = payload_on_base([0.0, 2.0], [0.1, 0.0, 0.15])
    assert p.shape == (2, abi.HB_PAYLOAD_SIZE) and np.array_equal(p[1], [2.0, 0.1, 0.0, 0.15, 0, 0, 0, 0, 0, 0]) and p[0, 0] == 0.0
    p = payload_on_base(3.0, [[0.0, 0.0, 0.1]], inertia=[0.05, 0.01, -0.005, 0.08, 0.002, 0.04])
    assert np.array_equal(p, [[3.0, 0.0, 0.0, 0.1, 0.05, 0.01, -0.005, 0.08, 0.002, 0.04]])
