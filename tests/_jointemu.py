"""Helpers of the joint-model tests of the ground-contact plant (tests/test_joint_plant_host.py, tests/test_gpu_joint_plant.py):

  * build() of tests/host_emu/libjointemu.so — csrc/hb_joints.hpp compiled for the host behind a tiny C API (jointemu.cpp), under the
    file lock of tests/_hostemu.py, installed atomically, rebuilt when a source it includes is newer;
  * an independent numpy twin of the joint model as include/hunter_hip.h defines it (JointPlant): dense 32 rows, Jh, Mh and
    W = Jh Mh^-1 Jh' formed in full, g = W p + c recomputed from scratch before every update, rigid-body terms from outside
    (tests/_contactemu.oracle_fns on the CPU, the device's eval_rbd on the GPU);
  * the cases (s), (r), (f1), (f2), (l), (o), the checks the tests share (check_against_twin, check_exact_properties,
    check_status_bits, check_momentum_row, check_l_rest ...: each names what it holds, so that the self-test can require the named check to fail), and the measurement
    behind the tolerances (measure_sensitivity; run this file to print it).

Tolerances of "device code against twin, one tick from the same (q, v, p)".  q: 1e-10, the plant's.  v, lambda / max(1, |lambda|),
friction torque and limit torque: 10 x the twin's OWN sensitivity, the largest change of its outputs over 40 ticks of the cases (s), (r),
(f2), (l) when q, v, the 32 warm-start impulses and every M, nle, J are perturbed by relative 1e-12 (measure_sensitivity, 3 draws per
tick, oracle rigid-body terms; the method of tests/_contactemu.py):
    measured |dv| [m/s, rad/s]:                 (s) 4.47e-09  (r) 7.50e-10  (f2) 3.61e-12  (l) 2.75e-10   -> 4.47e-09
    measured |dlambda| / max(1, |lambda|):      (s) 7.16e-06  (r) 0         (f2) 0         (l) 0          -> 7.16e-06
    measured |d friction torque| [N m]:         (s) 2.51e-05  (r) 8.22e-12  (f2) 2.01e-12  (l) 0          -> 2.51e-05
    measured |d limit torque| [N m]:            (s) 0         (r) 0         (f2) 0         (l) 1.48e-08   -> 1.48e-08
((s) dominates lambda and the friction torque: standing, the ten friction rows are inside their boxes and share the load with the
contact rows, so the split between them is as ill-conditioned as the contact problem; in (r) the robot leaves the ground in the first
tick — the 5 mm penetration of the tilted start is pushed out at erp * 5 mm / h = 2 m/s — and stays in the air, so lambda is zero there.)
The tolerances of tests/_contactemu.py (TOL_Q, TOL_V, TOL_LAM_REL) are used as they are where a test compares against the model
without joints (case (o)).
"""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import _contactemu as ce
from hunter_bipedal_control_amd import abi

HERE, CSRC = ce.HERE, ce.CSRC
DT, SUBSTEPS, EPS, H = ce.DT, ce.SUBSTEPS, ce.EPS, ce.H
UNCONVERGED = 1 << 30
KNEE = 3                       # joint 3 = q[9]: range 0 .. 1.5

TOL_Q = 1e-10
TOL_V = 10 * 4.47e-9
TOL_LAM_REL = 10 * 7.16e-6
TOL_FRICTION = 10 * 2.51e-5
TOL_LIMIT = 10 * 1.48e-8


def build():
    so = HERE / "libjointemu.so"
    deps = [HERE / "jointemu.cpp", CSRC.parents[1] / "include" / "hunter_hip.h", *CSRC.glob("*.hpp")]
    with open(HERE / ".hostemu.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            tmp = HERE / f"libjointemu.{os.getpid()}.so"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", str(tmp), str(HERE / "jointemu.cpp")])
            os.replace(tmp, so)
    return so


_p = ce._p


def emu_step(lib, mdl, cfg, jm, q, v, imp, jimp, tau, wrench=None, status=0, eps=EPS, dt=DT, substeps=SUBSTEPS):
    """One tick of hb_joints.hpp joints_step on the host for one instance -> dict like the twin's record (new arrays)."""
    o = dict(q=np.array(q, dtype=float), v=np.array(v, dtype=float), p=np.array(imp, dtype=float), jp=np.array(jimp, dtype=float),
             lam=np.zeros(12), vdot=np.zeros(16), gap=np.zeros(4), point_vel=np.zeros(12), residual=np.zeros(1),
             touching=np.zeros(4, dtype=np.int32), status=np.array([status], dtype=np.int32), tau_applied=np.zeros(10),
             friction_torque=np.zeros(10), limit_torque=np.zeros(10), jresidual=np.zeros(1), jstatus=np.zeros(1, dtype=np.int32),
             tau_last=np.zeros(10))
    tau = np.ascontiguousarray(tau, dtype=float)
    w = None if wrench is None else np.ascontiguousarray(wrench, dtype=float)
    lib.je_step(C.byref(mdl), C.byref(cfg), C.byref(jm), _p(o["q"]), _p(o["v"]), _p(o["p"]), _p(o["jp"]), _p(tau), _p(w), C.c_double(eps),
                C.c_double(dt), C.c_int(substeps), _p(o["lam"]), _p(o["vdot"]), _p(o["gap"]), _p(o["point_vel"]), _p(o["residual"]),
                _p(o["touching"]), _p(o["status"]), _p(o["tau_applied"]), _p(o["friction_torque"]), _p(o["limit_torque"]), _p(o["jresidual"]),
                _p(o["jstatus"]), _p(o["tau_last"]))
    for k in ("residual", "jresidual"):
        o[k] = float(o[k][0])
    o["status"], o["jstatus"] = int(o["status"][0]), int(o["jstatus"][0])
    return o


# ---- numpy twin ------------------------------------------------------------------------------------------------------------------------
def model_dict(jm):
    """abi.HbJointModel -> dict of numpy arrays / scalars."""
    d = {k: np.array(getattr(jm, k), dtype=float) for k in ("armature", "damping", "frictionloss", "lower", "upper", "torque_limit")}
    d.update(limit_erp=float(jm.limit_erp), tol=float(jm.tol), limits=int(jm.limits))
    return d


def twin_substep(q, v, p32, M, nle, J, foot_z, tau_a, wrench, jm, mu, ground_z, erp, sweeps, eps, h):
    """Steps 1 - 5 of the definition for one instance; p32 = contact impulses | friction impulses | signed stop impulses u.
    -> (q+, v+, p32 (stops as u again), contact residual, joint residual, s, diagonal of W on the friction rows)."""
    Mh = np.array(M, dtype=float)
    Mh[6:, 6:] += np.diag(jm["armature"] + h * jm["damping"])
    rhs = -np.asarray(nle, dtype=float).copy()
    rhs[6:] += tau_a - jm["damping"] * v[6:]
    if wrench is not None:
        rhs[0:3] += wrench[0:3]
        rhs[3:6] += ce._E1(q[3:6]).T @ wrench[3:6]
    vf = v + h * np.linalg.solve(Mh, rhs)
    lo, up = q[6:] - jm["lower"], jm["upper"] - q[6:]
    s = np.where(lo <= up, 1.0, -1.0)
    phi_j = np.where(lo <= up, lo, up)
    Jh = np.zeros((32, 16))
    Jh[:12] = J
    for j in range(10):
        Jh[12 + j, 6 + j] = 1.0
        Jh[22 + j, 6 + j] = s[j]
    MiJt = np.linalg.solve(Mh, Jh.T)
    W = Jh @ MiJt
    W[:12, :12] += eps * np.trace(W[:12, :12]) * np.eye(12)
    b = np.zeros(32)
    phi = foot_z - ground_z
    b[2:12:3] = (np.maximum(phi, 0.0) + erp * np.minimum(phi, 0.0)) / h
    b[22:] = (np.maximum(phi_j, 0.0) + jm["limit_erp"] * np.minimum(phi_j, 0.0)) / h
    c = Jh @ vf + b
    p = np.array(p32, dtype=float)
    p[22:] = np.maximum(0.0, s * p[22:]) if jm["limits"] else 0.0
    res = jres = 0.0
    for _ in range(sweeps):
        res = jres = 0.0
        for pt in range(4):
            a, n = 3 * pt, 3 * pt + 2
            g = W @ p + c
            new = max(0.0, p[n] - g[n] / W[n, n])
            res = max(res, abs(W[n, n] * (new - p[n])))
            p[n] = new
            g = W @ p + c
            t = np.array([p[a] - g[a] / W[a, a], p[a + 1] - g[a + 1] / W[a + 1, a + 1]])
            nrm, lim = np.hypot(t[0], t[1]), mu * p[n]
            if nrm > lim:
                t = t * (lim / nrm) if p[n] > 0.0 else np.zeros(2)
            res = max(res, abs(W[a, a] * (t[0] - p[a])), abs(W[a + 1, a + 1] * (t[1] - p[a + 1])))
            p[a:a + 2] = t
        for j in range(10):
            r, lim = 12 + j, jm["frictionloss"][j] * h
            g = W @ p + c
            new = min(max(p[r] - g[r] / W[r, r], -lim), lim)
            jres = max(jres, abs(W[r, r] * (new - p[r])))
            p[r] = new
        if jm["limits"]:
            for j in range(10):
                r = 22 + j
                g = W @ p + c
                new = max(0.0, p[r] - g[r] / W[r, r])
                jres = max(jres, abs(W[r, r] * (new - p[r])))
                p[r] = new
    vn = vf + MiJt @ p
    p[22:] = s * p[22:]
    return q + h * vn, vn, p, res, jres, s, np.diag(W)[12:22].copy()


class JointPlant(ce.GroundPlant):
    """Contact model 1 with the joint model in numpy, batched: ce.GroundPlant plus jp[B][20] (friction impulses | signed stop impulses),
    tau_applied, friction_torque, limit_torque [B][10], jresidual[B], jstatus[B], side[B][10] (s of the last substep) and wdiag[B][10]
    ((Mh^-1)_jj of the last substep)."""

    def __init__(self, jm, *args, **kw):
        super().__init__(*args, **kw)
        self.jm = jm if isinstance(jm, dict) else model_dict(jm)
        self.jp = np.zeros((self.B, 20))
        self.tau_applied, self.friction_torque, self.limit_torque = (np.zeros((self.B, 10)) for _ in range(3))
        self.jresidual, self.jstatus = np.zeros(self.B), np.zeros(self.B, dtype=np.int32)
        self.side, self.wdiag = np.ones((self.B, 10)), np.ones((self.B, 10))

    def step(self, tau, contact, dt, substeps=4):
        h = dt / substeps
        tau = np.asarray(tau, dtype=float).reshape(self.B, 10)
        self.tau_applied = np.clip(tau, -self.jm["torque_limit"], self.jm["torque_limit"])
        for _ in range(substeps):
            M, nle, J = self._terms()
            feet = np.asarray(self.foot_fn(self.q)).reshape(self.B, 4, 3)
            v_old = self.v.copy()
            for i in range(self.B):
                w = None if self.wrench is None else self.wrench[i]
                self.q[i], self.v[i], p32, self.residual[i], self.jresidual[i], self.side[i], self.wdiag[i] = twin_substep(
                    self.q[i], self.v[i], np.concatenate([self.p[i], self.jp[i]]), M[i], nle[i], J[i], feet[i, :, 2], self.tau_applied[i], w,
                    self.jm, self.mu, self.ground_z, self.erp, self.sweeps, self.eps, h)
                self.p[i], self.jp[i] = p32[:12], p32[12:]
                self.point_vel[i] = J[i] @ self.v[i]
            self.last_vdot = (self.v - v_old) / h
        self.last_lambda = self.p / h
        self.friction_torque, self.limit_torque = self.jp[:, :10] / h, self.jp[:, 10:] / h
        self.touching = (self.p[:, 2::3] > 0.0).astype(np.int32)
        self.gap = np.asarray(self.foot_fn(self.q)).reshape(self.B, 4, 3)[:, :, 2] - self.ground_z
        finite = np.isfinite(self.q).all(axis=1) & np.isfinite(self.v).all(axis=1)
        fallen = (self.q[:, 2] - self.ground_z < self.fall_height) if self.fall_height > 0.0 else np.zeros(self.B, dtype=bool)
        self.status = ((self.status & ce.FALLEN) | np.where(finite, 0, ce.NONFINITE) | np.where(fallen, ce.FALLEN, 0) |
                       np.where(self.residual <= self.tol, 0, ce.UNCONVERGED)).astype(np.int32)
        self.jstatus = status_word(self.limit_torque, self.tau_applied, tau, self.jresidual, self.jm["tol"])
        return self.q, self.v

    def record(self):
        return dict(q=self.q.copy(), v=self.v.copy(), lam=self.last_lambda.copy(), vdot=self.last_vdot.copy(), gap=self.gap.copy(),
                    point_vel=self.point_vel.copy(), residual=self.residual.copy(), touching=self.touching.copy(), status=self.status.copy(),
                    tau_applied=self.tau_applied.copy(), friction_torque=self.friction_torque.copy(), limit_torque=self.limit_torque.copy(),
                    jresidual=self.jresidual.copy(), jstatus=self.jstatus.copy(), side=self.side.copy(), wdiag=self.wdiag.copy())


def status_word(limit_torque, tau_applied, tau, jres, tol):
    """The status word of the definition from the arrays it summarises ([B][10] each, jres[B])."""
    bits = np.arange(10)
    st = ((np.asarray(limit_torque) != 0.0) << bits).sum(axis=-1) + ((np.asarray(tau_applied) != np.asarray(tau)) << (10 + bits)).sum(axis=-1)
    return (st + np.where(np.asarray(jres) <= tol, 0, UNCONVERGED)).astype(np.int32)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
# name -> sweeps.  (s), (r): the 30 of the contact tests.  The physics bounds of (f1), (f2), (l) are met by the twin alone on the CPU with
# these counts (tests/test_joint_plant_host.py test_the_twin_alone_meets_the_physics_bounds).
SWEEPS = dict(s=30, r=30, f1=60, f2=30, l=30, l_rest=5)
TICKS = 40
L_TORQUE = 60.0                # (l): the knee reaches its upper stop from 0.93 rad within the 40 ticks
REST_TICKS = 1250              # (l) at rest: the other joints lose the rates of the swing and the impact through damping alone (see check_l_rest)


def make_case(name, params, q_stand, terms_fn, foot_fn, rng):
    """-> dict(q0[16], v0[16], mu, ground_z, wrench, tau_fn(tick) -> [10], jm = abi.HbJointModel, sweeps)."""
    free = dict(armature=0.0, damping=0.0, frictionloss=0.0, torque_limit=np.inf, limits=0)
    if name == "s":
        q_on = ce.place_on_plane(q_stand, foot_fn)
        M, nle, J = terms_fn(q_on, np.zeros(16))[:3]
        tau_s = ce.statics_torque(M, nle, J)
        case = dict(q0=q_on, v0=np.zeros(16), mu=0.7, wrench=None, tau_fn=lambda tick: tau_s, jm=abi.make_joint_model(params))
    elif name == "r":
        case = ce.make_case("c", q_stand, terms_fn, rng)
        case["jm"] = abi.make_joint_model(params, frictionloss=0.2, armature=0.1, damping=1.0, torque_limit=2.0)
    elif name in ("f1", "f2", "l", "l_rest"):
        tau = np.zeros(10)
        if name in ("l", "l_rest"):
            tau[KNEE] = L_TORQUE
            jm = abi.make_joint_model(params, frictionloss=0.0, damping=1.0, limits=1)
        else:
            tau[KNEE] = (0.5 if name == "f1" else 3.0) * 0.2
            jm = abi.make_joint_model(params, **{**free, "frictionloss": 0.2})
        case = dict(q0=np.array(q_stand, dtype=float), v0=np.zeros(16), mu=0.7, wrench=None, tau_fn=lambda tick: tau, jm=jm, ground_z=-100.0)
    else:
        raise ValueError(name)
    case.setdefault("ground_z", 0.0)
    case["sweeps"] = SWEEPS[name]
    return case


def all_off_model(params):
    """Case (o): a joint model with everything off."""
    return abi.make_joint_model(params, armature=0.0, damping=0.0, frictionloss=0.0, torque_limit=np.inf, limits=0)


def contact_cfg(params, case, **kw):
    return abi.make_contact_config(params, **{**dict(mu=case["mu"], ground_z=case["ground_z"], erp=ce.ERP, sweeps=case["sweeps"]), **kw})


def twin_for(case, rbd_fn, foot_fn, qv_fn=None, batch=1):
    return JointPlant(case["jm"], rbd_fn, foot_fn, np.tile(case["q0"], (batch, 1)), np.tile(case["v0"], (batch, 1)), mu=case["mu"],
                      ground_z=case["ground_z"], sweeps=case["sweeps"], qv_fn=qv_fn)


# ---- the checks (one instance: dev = outputs of the code under test, twin = JointPlant.record() row) ----------------------------------------
def check_against_twin(dev, twin):
    """Point 1: q 1e-10; v, lambda / max(1, |lambda|), friction torque, limit torque 10 x the twin's sensitivity; tau_applied bit-equal."""
    lam_scale = max(1.0, np.abs(twin["lam"]).max())
    errs = dict(q=np.abs(dev["q"] - twin["q"]).max(), v=np.abs(dev["v"] - twin["v"]).max(),
                lam=np.abs(dev["lam"] - twin["lam"]).max() / lam_scale,
                friction_torque=np.abs(dev["friction_torque"] - twin["friction_torque"]).max(),
                limit_torque=np.abs(dev["limit_torque"] - twin["limit_torque"]).max())
    tol = dict(q=TOL_Q, v=TOL_V, lam=TOL_LAM_REL, friction_torque=TOL_FRICTION, limit_torque=TOL_LIMIT)
    for k, e in errs.items():
        assert e <= tol[k], ("against the twin", k, e, tol[k])
    assert abs(dev["jresidual"] - twin["jresidual"]) <= TOL_V, ("against the twin", "jresidual", dev["jresidual"], twin["jresidual"])
    return errs


def check_exact_properties(dev, tau, jm, mu):
    """Point 2 on one instance (jm = model_dict): the friction bound, tau_applied against numpy's clip, the contact properties; the sign
    of the stop torques and the status bits are check_stop_sign / check_status_bits."""
    assert (np.abs(dev["friction_torque"]) <= jm["frictionloss"] * (1.0 + 1e-14)).all(), "friction bound"
    assert np.array_equal(dev["tau_applied"], np.clip(tau, -jm["torque_limit"], jm["torque_limit"])), "tau_applied is not numpy's clip"
    ce.assert_exact_properties(dev["lam"] * H, dev["touching"], dev["status"], mu)


def check_impulse_identities(dev):
    """lambda = p / h, friction torque = p / h, limit torque = u / h, bit for bit (the host build hands the impulses out)."""
    assert np.array_equal(dev["lam"], dev["p"] / H), "lambda = p / h"
    assert np.array_equal(dev["friction_torque"], dev["jp"][:10] / H), "friction torque = p / h"
    assert np.array_equal(dev["limit_torque"], dev["jp"][10:] / H), "limit torque = u / h"


def check_integration(dev, q_in, h):
    """q+ = q + h v+ of a tick of ONE substep, to two units in the last place of the largest of |q|, |h v+|, |q+| (the device fuses the
    product into the sum, numpy rounds it first: one rounding of h v+ apart, and where q and h v+ cancel the sum is smaller than both)."""
    hv = h * dev["v"]
    ulp = np.spacing(np.maximum(np.maximum(np.abs(q_in), np.abs(hv)), np.abs(dev["q"])))
    assert (np.abs(dev["q"] - (q_in + hv)) <= 2.0 * ulp).all(), "q+ = q + h v+"


# ---- physics (point 3), on one instance's records over a run: devs[tick], twins[tick] -----------------------------------------------------
ROUND = 64 * np.finfo(float).eps   # a joint rate is v_f + Mh^-1 Jh' p: two 16-term triangular solves and a 32-term sum, 64 roundings


def check_f1(devs, twins, tau3, jm):
    """(f1): every joint rate within the joint residual of zero, friction_torque[3] = -tau, the others 0.  The residual of a converged
    run is exactly 0 while the rate is a rounded sum of terms of size h tau (Mh^-1)_jj that cancel, so the rate bound is the joint
    residual + ROUND * h |tau| max_j (Mh^-1)_jj, and the torque bound of joint j that rate bound / ((Mh^-1)_jj h)."""
    for d, t in zip(devs, twins):
        rate = d["jresidual"] + ROUND * H * abs(tau3) * t["wdiag"].max()
        assert (np.abs(d["v"][6:]) <= rate).all(), ("(f1) joint rates", np.abs(d["v"][6:]).max(), rate)
        want = np.zeros(10)
        want[KNEE] = -tau3
        assert (np.abs(d["friction_torque"] - want) <= rate / (t["wdiag"] * H)).all(), "(f1) friction torque"


def check_f2(devs, tau3, jm):
    """(f2): friction_torque[3] = -sign(tau) frictionloss to 1e-14 relative on every tick once the joint moves."""
    moved = 0
    for d in devs:
        if d["v"][6 + KNEE] != 0.0:
            moved += 1
            want = -np.sign(tau3) * jm["frictionloss"][KNEE]
            assert abs(d["friction_torque"][KNEE] - want) <= 1e-14 * abs(want), "(f2) friction torque"
    assert moved >= len(devs) - 1, "(f2) the joint moves"


def check_l(devs, twins, jm):
    """(l) over the 40 ticks: q[9] <= upper + the penetration of the twin's run (+ TOL_Q, to which the two agree); no stop bit but the
    knee's on any tick, and the knee's set at the end with a negative limit torque (an upper stop pushes back)."""
    upper = jm["upper"][KNEE]
    pen = max(0.0, max(t["q"][6 + KNEE] - upper for t in twins))
    for d in devs:
        assert d["q"][6 + KNEE] <= upper + pen + TOL_Q, ("(l) penetration", d["q"][6 + KNEE] - upper, pen)
        assert d["jstatus"] & 0x3FF & ~(1 << KNEE) == 0, ("(l) another stop bit", hex(d["jstatus"]))
    assert devs[-1]["jstatus"] & (1 << KNEE) and devs[-1]["limit_torque"][KNEE] < 0.0, "(l) the knee rests on its stop"


REST_RATE, REST_SPIN, REST_TIME = 1e-6, 3e-3, 0.1


def check_l_rest(dev, M, jm, joint=KNEE):
    """(l) at rest, after REST_TICKS ticks: the limit torque cancels the applied torque within joint residual / ((Mh^-1)_jj h) + what
    the motion that is left can put on the joint's row of M vdot + nle + damping o v.  "At rest" is asserted: every joint rate <=
    REST_RATE = 1e-6 rad/s, every base angular rate <= REST_SPIN = 3e-3 rad/s (nothing damps the free-floating base: the integrator
    leaves it a rigid rotation of 8.8e-4 rad/s, which puts a centrifugal torque on the joint for good).  What that motion can add, with
    R = sum_k |Mh[joint][k]| (M: the mass matrix at the end state, from the oracle / the device's eval_rbd, not from the code under test):
    inertial and damping terms of rates that decay in REST_TIME = armature / damping = 0.1 s, <= R REST_RATE / REST_TIME + damping
    REST_RATE; centrifugal and Coriolis terms, <= R REST_SPIN^2.  With R = 0.4 kg m^2 that is 9e-6 N m against 60 N m applied."""
    rates, spin = np.abs(dev["v"][6:]).max(), np.abs(dev["v"][3:6]).max()
    assert rates <= REST_RATE and spin <= REST_SPIN, ("(l) not at rest", rates, spin)
    assert dev["jstatus"] & (1 << joint), "(l) at rest: the stop is not active"
    Mh = np.array(M, dtype=float)
    Mh[6:, 6:] += np.diag(jm["armature"] + H * jm["damping"])
    Mh_row, wjj = np.abs(Mh[6 + joint]).sum(), np.linalg.inv(Mh)[6 + joint, 6 + joint]
    bound = dev["jresidual"] / (wjj * H) + Mh_row * (REST_RATE / REST_TIME + REST_SPIN ** 2) + jm["damping"][joint] * REST_RATE
    miss = dev["limit_torque"][joint] + dev["tau_applied"][joint]
    assert abs(miss) <= bound, ("(l) limit torque at rest", miss, bound)
    return miss, bound


def check_momentum_row(dev, v_in, M, nle, J, jm, h):
    """A tick of ONE substep from v_in: on every joint row, limit torque + applied torque + friction torque = (Mh (v+ - v) / h + nle +
    damping o v - J' lambda), with v+, lambda and the three torques the outputs of the code under test and M, nle, J from outside it
    (oracle / eval_rbd at the start of the tick).  Bound: ROUND x the sum of the magnitudes of the terms, the inertial term taken as
    the Cholesky solve leaves it: the residual of L L' x = b in row i is of the size eps (|L| |L'| |x|)_i, and |L| |L'| <= sqrt(m_ii m_jj)
    entry by entry, so the heavy base rows reach the light joint rows through sqrt(m_ii m_jj), not through the small m_ij.  nle enters
    with its largest entry on every row: a joint row of nle is a sum over the bodies of forces of the size of the base rows (m g = 136 N)
    times lever arms below 1 m that cancel, so its rounding is that of the largest term, not of the small result."""
    Mh = np.array(M, dtype=float)
    Mh[6:, 6:] += np.diag(jm["armature"] + h * jm["damping"])
    dv = (dev["v"] - v_in) / h
    row = (Mh @ dv + nle)[6:] + jm["damping"] * v_in[6:] - (J.T @ dev["lam"])[6:]
    lhs = dev["limit_torque"] + dev["tau_applied"] + dev["friction_torque"]
    root = np.sqrt(np.diag(Mh))
    scale = (root * (root @ np.abs(dv)))[6:] + np.abs(nle).max() + jm["damping"] * np.abs(v_in[6:]) + (np.abs(J.T) @ np.abs(dev["lam"]))[6:] + np.abs(lhs)
    assert (np.abs(lhs - row) <= ROUND * scale).all(), ("momentum row", np.abs(lhs - row).max(), (ROUND * scale).min())


def check_r_bits(dev, tau):
    """(r): bits 10..19 are set exactly where |tau| > 2."""
    assert (dev["jstatus"] >> 10) & 0x3FF == int(((np.abs(tau) > 2.0) << np.arange(10)).sum()), "(r) saturation bits"


def check_stop_sign(dev, side):
    """s_j * limit_torque_j >= 0 with s of the last substep (the twin's)."""
    assert (side * dev["limit_torque"] >= 0.0).all(), "stop sign"


def check_status_bits(dev, tau, jm):
    assert dev["jstatus"] == status_word(dev["limit_torque"], dev["tau_applied"], tau, dev["jresidual"], jm["tol"]), "status bits"


def measure_sensitivity(params, q_stand, qv_fn, foot_fn, ticks=TICKS, draws=3, rel=1e-12):
    """Largest change of the twin's v, lambda / max(1, |lambda|), friction torque and limit torque after one tick when q, v, the 32
    impulses and every M, nle, J are perturbed by relative `rel` (uniform in [-rel, rel] per entry), over `ticks` ticks of the cases
    (s), (r), (f2), (l) -> {case: (dv, dlam_rel, dfriction, dlimit)}."""
    out = {}
    for name in ("s", "r", "f2", "l"):
        rng = np.random.default_rng(7)
        case = make_case(name, params, q_stand, qv_fn, foot_fn, rng)
        base = twin_for(case, None, foot_fn, qv_fn)
        worst = np.zeros(4)
        for tick in range(ticks):
            tau = case["tau_fn"](tick)
            q, v, p, jp = base.q.copy(), base.v.copy(), base.p.copy(), base.jp.copy()
            base.step(tau[None], None, DT, SUBSTEPS)
            for _ in range(draws):
                pert = lambda x: x * (1.0 + rel * rng.uniform(-1.0, 1.0, np.shape(x)))  # noqa: E731
                tw = twin_for(case, None, foot_fn, lambda qq, vv: tuple(pert(np.asarray(x)) for x in qv_fn(qq, vv)[:3]))
                tw.q, tw.v, tw.p, tw.jp = pert(q), pert(v), pert(p), pert(jp)
                tw.step(tau[None], None, DT, SUBSTEPS)
                worst = np.maximum(worst, [np.abs(tw.v - base.v).max(),
                                           np.abs(tw.last_lambda - base.last_lambda).max() / max(1.0, np.abs(base.last_lambda).max()),
                                           np.abs(tw.friction_torque - base.friction_torque).max(),
                                           np.abs(tw.limit_torque - base.limit_torque).max()])
        out[name] = tuple(worst)
    return out


if __name__ == "__main__":
    from hunter_bipedal_control_amd import ingest   # (run with the repository root and tests/ on PYTHONPATH)
    prm = ingest.load_packaged()
    qv, foot, qs = ce.oracle_fns(prm)
    for k, w in measure_sensitivity(prm, qs, qv, foot).items():
        print(f"sensitivity ({k}): |dv| {w[0]:.2e}   |dlambda| rel {w[1]:.2e}   |d friction torque| {w[2]:.2e}   |d limit torque| {w[3]:.2e}")
