"""Helpers of the actuator-loop tests of the plant (tests/test_actuator_plant_host.py, tests/test_gpu_actuator_plant.py):

  * build() of tests/host_emu/libactemu.so — the hybrid forms of plant_step / contact_step / joints_step and the per-item routines of the
    wire kernels of the simulator end compiled for the host behind a tiny C API (actemu.cpp), under the file lock of tests/_hostemu.py;
  * the yardstick, a composition identity and not a new model: a hybrid step of S substeps equals S held-torque steps of ONE substep of
    length dt / S, each with the law's torque computed HERE, in numpy, from the state at its start (compose).  The held-torque steps are
    those of the independent numpy twins the earlier tests hold the plant to: oracle.plant.Plant (pinned stub), tests/_contactemu.GroundPlant
    (contact model 1), tests/_jointemu.JointPlant (joint model).  Exact because the warm starts carry over from step to step, the stub
    re-anchors only when a contact switches on, and lambda = p / h has the same h;
  * the cases and commands both test files share, and the checks at the tolerances the twins' helpers define.

Tolerances.  Contact model 1: ce.TOL_Q, ce.TOL_V, ce.TOL_LAM_REL; joint model: je.TOL_Q, je.TOL_V, je.TOL_LAM_REL, je.TOL_FRICTION,
je.TOL_LIMIT ("code against twin, one tick from the same state": the twin is re-seeded with the state of the code under test before every
tick).  Pinned stub: q 1e-10, v 1e-8, lambda 1e-6 max(1, |lambda|), the bounds tests/test_host_emu.py and tests/test_closed_loop.py hold
the stub to.  Torques (tau_first, tau_mean, tau_applied, the sensed torque): the law is linear in the state, so two evaluations at states
that agree to (tol_q, tol_v) differ by at most max(kp) tol_q + max(kd) tol_v; substep s > 0 starts from states that already differ by
up to the tick's tolerance, so that bound holds for every substep and for their mean (torque_tol)."""
import copy
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import _contactemu as ce
import _jointemu as je
from hunter_bipedal_control_amd import abi
from oracle.plant import Plant

HERE, CSRC = ce.HERE, ce.CSRC
DT, SUBSTEPS, TICKS, EPS, BAUM = ce.DT, ce.SUBSTEPS, 10, ce.EPS, 30.0
STUB_TOL_Q, STUB_TOL_V, STUB_TOL_LAM_REL = 1e-10, 1e-8, 1e-6
KEYS = ("pos_des", "vel_des", "kp", "kd", "tau_ff")
SAT_BITS = 0x3FF << 10

_p = ce._p


def build():
    so = HERE / "libactemu.so"
    deps = [HERE / "actemu.cpp", CSRC.parents[1] / "include" / "hunter_hip.h", CSRC.parents[1] / "include" / "hunter_lcm.h", *CSRC.glob("*.hpp")]
    with open(HERE / ".hostemu.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            tmp = HERE / f"libactemu.{os.getpid()}.so"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", str(tmp), str(HERE / "actemu.cpp")])
            os.replace(tmp, so)
    return so


# ---- the law and the commands --------------------------------------------------------------------------------------------------------
def law(cmd, q, v):
    """tau = ff + kp (pos_des - q_joint) + kd (vel_des - v_joint), operand order of k_joint_command; q, v [..., 16]."""
    return cmd["tau_ff"] + cmd["kp"] * (cmd["pos_des"] - q[..., 6:]) + cmd["kd"] * (cmd["vel_des"] - v[..., 6:])


def make_command(ff, q, rng, stance=(True, True)):
    """The command of a tick for one instance: ff = the case's torque, gains = abi.make_joint_gains() by joint as k_joint_command assigns
    them, pos_des = q_joint + U(-0.05, 0.05), vel_des = U(-0.5, 0.5)."""
    kp, kd = abi.hybrid_gains(abi.make_joint_gains(), stance)
    return dict(pos_des=q[6:] + rng.uniform(-0.05, 0.05, 10), vel_des=rng.uniform(-0.5, 0.5, 10), kp=kp, kd=kd, tau_ff=np.array(ff, dtype=float))


def stack(cmds):
    """list of per-instance commands -> one batched command ([B][10] each)."""
    return {k: np.array([c[k] for c in cmds]) for k in KEYS}


def pack(cmd):
    """One instance's command as the [5][10] block actemu.cpp takes."""
    return np.ascontiguousarray(np.concatenate([cmd[k] for k in KEYS]), dtype=float)


def torque_tol(cmd, tol_q, tol_v):
    return float(np.max(cmd["kp"]) * tol_q + np.max(cmd["kd"]) * tol_v)


# ---- the composition -----------------------------------------------------------------------------------------------------------------
def compose(twin, cmd, contact, dt, substeps, limit=None):
    """`substeps` held-torque steps of one substep of length dt / substeps on the twin (Plant, GroundPlant or JointPlant, batched), the
    torque of each computed here from the twin's (q, v) at its start.  limit: the joint model's torque limit [10] (JointPlant) or None.
    -> dict(tau_first, tau_mean, tau_last [B][10] and, with a limit, sat[B] = the saturation bits 10 + j ORed over the steps,
    sat_steps[substeps][B][10] = saturated in that step)."""
    taus, applied, sat_steps = [], [], []
    for _ in range(substeps):
        tau = law(cmd, twin.q, twin.v)
        twin.step(tau, contact, dt / substeps, 1)
        taus.append(tau)
        ta = tau if limit is None else np.clip(tau, -limit, limit)
        applied.append(ta)
        sat_steps.append(ta != tau)
    out = dict(tau_first=taus[0], tau_mean=np.mean(applied, axis=0), tau_last=applied[-1], sat_steps=np.array(sat_steps))
    out["sat"] = (np.any(out["sat_steps"], axis=0) << (10 + np.arange(10))).sum(axis=-1).astype(np.int32)
    return out


def held(twin, cmd, contact, dt, substeps):
    """The held-torque tick with tau_0 over `substeps` substeps on a COPY of the twin -> the copy.  What a build that evaluates the law
    once per step would compute."""
    tw = copy.deepcopy(twin)
    tw.step(law(cmd, tw.q, tw.v), contact, dt, substeps)
    return tw


def assert_can_fail(twin_held, twin_composed, tol_v, who):
    """The held-torque tick differs from the composed reference in v by at least 100 x the tolerance used for v."""
    gap = np.abs(twin_held.v - twin_composed.v).max(axis=-1)
    assert (gap >= 100.0 * tol_v).all(), (who, "the case cannot tell the hybrid step from a held torque", gap, 100.0 * tol_v)
    return gap


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
STUB_CASES = {"stance": (1, 1, 1, 1), "left": (1, 0, 1, 0)}   # contact i sits on leg i & 1
# seeds chosen on the CPU with the twins alone (test_actuator_plant_host.py test_the_cases_can_fail) so that every tick of every case
# tells the hybrid step from the held one
SEEDS = {"stance": 7, "left": 7, "c": 7, "r": 7, "l": 7}


def stub_case(name, q_stand, terms_fn, rng):
    """Pinned stub: the standing configuration, small rates, the statics torque; contact flags of STUB_CASES."""
    M, nle, J = terms_fn(np.array(q_stand, dtype=float), np.zeros(16))[:3]
    tau_s = ce.statics_torque(M, nle, J)
    return dict(q0=np.array(q_stand, dtype=float), v0=0.05 * rng.standard_normal(16), contact=np.array(STUB_CASES[name], dtype=np.int32),
                tau_fn=lambda tick: tau_s)


STICKY_TAU0 = 2.03   # N m on the knee: found with the twin alone — saturated in the substeps 0, 1, 2, at 1.988 N m in the last


def sticky_case(params, q_stand, terms_fn, foot_fn):
    """-> ((r) of the joint tests: torque limit 2 N m; a command with ff = 0 whose knee torque starts at STICKY_TAU0)."""
    rng = np.random.default_rng(7)
    case = je.make_case("r", params, q_stand, terms_fn, foot_fn, rng)
    cmd = make_command(np.zeros(10), case["q0"], rng)
    j = je.KNEE
    cmd["pos_des"][j] = case["q0"][6 + j] + (STICKY_TAU0 - cmd["kd"][j] * (cmd["vel_des"][j] - case["v0"][6 + j])) / cmd["kp"][j]
    return case, cmd


def stance_of(contact):
    return (bool(contact[0]), bool(contact[1]))


# ---- the host build ------------------------------------------------------------------------------------------------------------------
def emu_stub(lib, mdl, q, v, anchor, pinned, cmd, contact, dt=DT, substeps=SUBSTEPS, eps=EPS, baum=BAUM):
    o = dict(q=np.array(q, dtype=float), v=np.array(v, dtype=float), anchor=np.array(anchor, dtype=float).reshape(12),
             pinned=np.array(pinned, dtype=np.int32), lam=np.zeros(12), vdot=np.zeros(16), tau_first=np.zeros(10), tau_mean=np.zeros(10),
             tau_last=np.zeros(10))
    c, fl = pack(cmd), np.ascontiguousarray(contact, dtype=np.int32)
    lib.ae_stub_step(C.byref(mdl), _p(o["q"]), _p(o["v"]), _p(o["anchor"]), _p(o["pinned"]), _p(c), _p(fl), C.c_double(baum), C.c_double(eps),
                     C.c_double(dt), C.c_int(substeps), _p(o["lam"]), _p(o["vdot"]), _p(o["tau_first"]), _p(o["tau_mean"]), _p(o["tau_last"]))
    return o


def emu_stub_held(lib, mdl, q, v, anchor, pinned, tau, contact, dt=DT, substeps=SUBSTEPS, eps=EPS, baum=BAUM):
    o = dict(q=np.array(q, dtype=float), v=np.array(v, dtype=float), anchor=np.array(anchor, dtype=float).reshape(12),
             pinned=np.array(pinned, dtype=np.int32), lam=np.zeros(12), vdot=np.zeros(16))
    t, fl = np.ascontiguousarray(tau, dtype=float), np.ascontiguousarray(contact, dtype=np.int32)
    lib.ae_stub_step_held(C.byref(mdl), _p(o["q"]), _p(o["v"]), _p(o["anchor"]), _p(o["pinned"]), _p(t), _p(fl), C.c_double(baum), C.c_double(eps),
                          C.c_double(dt), C.c_int(substeps), _p(o["lam"]), _p(o["vdot"]))
    return o


def emu_contact(lib, mdl, cfg, q, v, imp, cmd, wrench=None, status=0, dt=DT, substeps=SUBSTEPS, eps=EPS):
    o = dict(q=np.array(q, dtype=float), v=np.array(v, dtype=float), p=np.array(imp, dtype=float), lam=np.zeros(12), vdot=np.zeros(16),
             gap=np.zeros(4), point_vel=np.zeros(12), residual=np.zeros(1), touching=np.zeros(4, dtype=np.int32),
             status=np.array([status], dtype=np.int32), tau_first=np.zeros(10), tau_mean=np.zeros(10), tau_last=np.zeros(10))
    c = pack(cmd)
    w = None if wrench is None else np.ascontiguousarray(wrench, dtype=float)
    lib.ae_contact_step(C.byref(mdl), C.byref(cfg), _p(o["q"]), _p(o["v"]), _p(o["p"]), _p(c), _p(w), C.c_double(eps), C.c_double(dt),
                        C.c_int(substeps), _p(o["lam"]), _p(o["vdot"]), _p(o["gap"]), _p(o["point_vel"]), _p(o["residual"]), _p(o["touching"]),
                        _p(o["status"]), _p(o["tau_first"]), _p(o["tau_mean"]), _p(o["tau_last"]))
    o["residual"], o["status"] = float(o["residual"][0]), int(o["status"][0])
    return o


def emu_joints(lib, mdl, cfg, jm, q, v, imp, jimp, cmd, wrench=None, status=0, dt=DT, substeps=SUBSTEPS, eps=EPS):
    o = dict(q=np.array(q, dtype=float), v=np.array(v, dtype=float), p=np.array(imp, dtype=float), jp=np.array(jimp, dtype=float),
             lam=np.zeros(12), vdot=np.zeros(16), gap=np.zeros(4), point_vel=np.zeros(12), residual=np.zeros(1),
             touching=np.zeros(4, dtype=np.int32), status=np.array([status], dtype=np.int32), tau_applied=np.zeros(10),
             friction_torque=np.zeros(10), limit_torque=np.zeros(10), jresidual=np.zeros(1), jstatus=np.zeros(1, dtype=np.int32),
             tau_last=np.zeros(10), tau_first=np.zeros(10), tau_mean=np.zeros(10))
    c = pack(cmd)
    w = None if wrench is None else np.ascontiguousarray(wrench, dtype=float)
    lib.ae_joints_step(C.byref(mdl), C.byref(cfg), C.byref(jm), _p(o["q"]), _p(o["v"]), _p(o["p"]), _p(o["jp"]), _p(c), _p(w), C.c_double(eps),
                       C.c_double(dt), C.c_int(substeps), _p(o["lam"]), _p(o["vdot"]), _p(o["gap"]), _p(o["point_vel"]), _p(o["residual"]),
                       _p(o["touching"]), _p(o["status"]), _p(o["tau_applied"]), _p(o["friction_torque"]), _p(o["limit_torque"]),
                       _p(o["jresidual"]), _p(o["jstatus"]), _p(o["tau_last"]), _p(o["tau_first"]), _p(o["tau_mean"]))
    for k in ("residual", "jresidual"):
        o[k] = float(o[k][0])
    o["status"], o["jstatus"] = int(o["status"][0]), int(o["jstatus"][0])
    return o


# ---- the checks: dev = one instance's outputs of the code under test, tw = the composed twin, i its instance, ref = compose()'s record ------
def check_torques(dev, ref, i, tol, who):
    for k in ("tau_first", "tau_mean", "tau_last"):
        e = np.abs(dev[k] - ref[k][i]).max()
        assert e <= tol, (who, k, e, tol)


def check_stub(dev, tw, ref, i, cmd, who):
    """q 1e-10, v 1e-8, lambda 1e-6 max(1, |lambda|), vdot 1e-8 / h (vdot = dv / h of the last substep); the three torques."""
    h = DT / SUBSTEPS
    errs = dict(q=np.abs(dev["q"] - tw.q[i]).max(), v=np.abs(dev["v"] - tw.v[i]).max(),
                lam=np.abs(dev["lam"] - tw.last_lambda[i]).max() / max(1.0, np.abs(tw.last_lambda[i]).max()),
                vdot=np.abs(dev["vdot"] - tw.last_vdot[i]).max() * h)
    tol = dict(q=STUB_TOL_Q, v=STUB_TOL_V, lam=STUB_TOL_LAM_REL, vdot=2.0 * STUB_TOL_V)
    for k, e in errs.items():
        assert e <= tol[k], (who, k, e, tol[k])
    check_torques(dev, ref, i, torque_tol(cmd, STUB_TOL_Q, STUB_TOL_V), who)
    return errs


def check_contact(dev, tw, ref, i, cmd, who):
    """ce.TOL_Q, ce.TOL_V, ce.TOL_LAM_REL; vdot = (v+ - v) / h of the last substep, both rates within TOL_V: 2 TOL_V / h; gap TOL_Q x the
    lever of the kinematics (1 m: 1e-10 of q moves a point by no more); point velocity J v+: TOL_V x the row sums of J (< 4); touching
    and status equal."""
    h = DT / SUBSTEPS
    lam_scale = max(1.0, np.abs(tw.last_lambda[i]).max())
    errs = dict(q=np.abs(dev["q"] - tw.q[i]).max(), v=np.abs(dev["v"] - tw.v[i]).max(),
                lam=np.abs(dev["lam"] - tw.last_lambda[i]).max() / lam_scale, vdot=np.abs(dev["vdot"] - tw.last_vdot[i]).max() * h,
                gap=np.abs(dev["gap"] - tw.gap[i]).max(), point_vel=np.abs(np.ravel(dev["point_vel"]) - np.ravel(tw.point_vel[i])).max())
    tol = dict(q=ce.TOL_Q, v=ce.TOL_V, lam=ce.TOL_LAM_REL, vdot=2.0 * ce.TOL_V, gap=10.0 * ce.TOL_Q, point_vel=4.0 * ce.TOL_V)
    for k, e in errs.items():
        assert e <= tol[k], (who, k, e, tol[k])
    assert np.array_equal(dev["touching"], tw.touching[i]) and int(dev["status"]) == int(tw.status[i]), (who, "touching / status")
    check_torques(dev, ref, i, torque_tol(cmd, ce.TOL_Q, ce.TOL_V), who)
    return errs


def check_joints(dev, tw, ref, i, cmd, who):
    """je.check_against_twin (q, v, lambda, friction and limit torque, joint residual) on the composed twin; touching and the contact
    status equal; the joint status word: stop bits and HB_JOINT_UNCONVERGED of the last composed step, saturation bits ORed over the
    composed steps; tau_applied and the three torques of the step within the law's bound."""
    rec = {k: x[i] for k, x in tw.record().items()}
    errs = je.check_against_twin(dev, rec)
    assert np.array_equal(dev["touching"], rec["touching"]) and int(dev["status"]) == int(rec["status"]), (who, "touching / status")
    want = (int(rec["jstatus"]) & ~SAT_BITS) | int(ref["sat"][i])
    assert int(dev["jstatus"]) & 0xFFFFF == want & 0xFFFFF, (who, "joint status", hex(int(dev["jstatus"])), hex(want))
    tol = torque_tol(cmd, je.TOL_Q, je.TOL_V)
    check_torques(dev, ref, i, tol, who)
    assert np.abs(dev["tau_applied"] - ref["tau_last"][i]).max() <= tol, (who, "tau_applied")
    return errs


# ---- reference adaptors of the device tests ----------------------------------------------------------------------------------------------
class Snapshot:
    """Batched outputs (dict of [B][...] arrays with the keys of the emu_* records) in the shape the checks take a twin in."""

    def __init__(self, rec):
        self.rec = {k: np.array(x) for k, x in rec.items()}
        self.q, self.v = self.rec["q"], self.rec["v"]
        self.last_lambda, self.last_vdot = self.rec["lam"], self.rec["vdot"]
        for k in ("gap", "point_vel", "touching", "status"):
            if k in self.rec:
                setattr(self, k, self.rec[k])

    def record(self):
        return self.rec


def batched(o):
    """One instance's emu_* record -> a Snapshot of batch 1 and the reference record of its torques."""
    snap = Snapshot({k: np.asarray(x)[None] for k, x in o.items()})
    ref = {k: np.asarray(o[k])[None] for k in ("tau_first", "tau_mean", "tau_last")}
    ref["sat"] = np.array([int(o.get("jstatus", 0)) & SAT_BITS], dtype=np.int32)
    return snap, ref
