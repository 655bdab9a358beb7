"""Helpers of the terrain tests of the ground-contact plant (tests/test_terrain_plant_host.py, tests/test_gpu_terrain_plant.py):

  * build() of tests/host_emu/libterrainemu.so — the terrain forms of csrc/hb_contact.hpp / hb_joints.hpp compiled for the host behind a
    tiny C API (terrainemu.cpp), under the file lock of tests/_hostemu.py, installed atomically, rebuilt when a source it includes is newer;
  * an independent numpy twin of the terrain as include/hunter_hip.h defines it (TerrainPlant): the frame from the normal, J~ =
    blockdiag(T') J built FIRST, W = J~ M^-1 J~' from it with np.linalg.solve, g = W p + c recomputed from scratch before every update,
    lambda = T p / h; with a joint model the dense 32 rows of tests/_jointemu.py on J~.  It shares no route with the device code, which
    rotates Jc, the contact columns of X and A after they are formed;
  * the five scenarios of the issue, one per instance, the checks the tests share, and the measurement behind the tolerances
    (measure_sensitivity; run this file to print it, together with the stick / slide figures).

Tolerances of "device code against twin, one tick from the same (q, v, p)".  q: 1e-10, the plant's.  v, lambda / max(1, |lambda|) and,
with the joint model, friction and limit torque: 10 x the twin's OWN sensitivity, the largest change of its outputs over the ticks of
the five scenarios when q, v, the warm-start impulses and every M, nle, J are perturbed by relative 1e-12 (measure_sensitivity, 3 draws per
tick, oracle rigid-body terms; the method of tests/_contactemu.py):
    ideal joints    |dv| [m/s, rad/s]          (0) 1.74e-09  (1) 1.43e-10  (2) 1.84e-08  (3) 1.58e-08  (4) 1.37e-08   -> 1.84e-08
                    |dlambda| / max(1, |lambda|)  (0) 4.51e-09  (1) 4.25e-10  (2) 1.92e-09  (3) 6.78e-11  (4) 1.10e-08   -> 1.10e-08
    joint model     |dv|                       (0) 4.47e-09  (1) 4.43e-10  (2) 5.92e-09  (3) 4.96e-10  (4) 5.03e-09   -> 5.92e-09
                    |dlambda| / max(1, |lambda|)  (0) 7.16e-06  (1) 1.37e-07  (2) 2.54e-07  (3) 6.90e-10  (4) 2.71e-08   -> 7.16e-06
                    |d friction torque| [N m]  (0) 2.51e-05  (1) 5.27e-07  (2) 3.11e-07  (3) 5.43e-09  (4) 5.39e-08   -> 2.51e-05
                    |d limit torque| [N m]     0 in every scenario: no stop is reached, the torque is exactly zero        -> 0
(scenario 0 with the joint model is case (s) of tests/_jointemu.py and repeats its figures: standing, the friction rows share the load
with the contact rows.)
"""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import _contactemu as ce
import _jointemu as je
from hunter_bipedal_control_amd import abi

HERE, CSRC = ce.HERE, ce.CSRC
DT, SUBSTEPS, EPS, H, SWEEPS, ERP = ce.DT, ce.SUBSTEPS, ce.EPS, ce.H, ce.SWEEPS, ce.ERP
B = 5
TICKS = (40, 40, 40, 50, 40)      # per scenario; a batch runs max(TICKS)

TOL_Q = 1e-10
TOL = {False: dict(v=10 * 1.84e-8, lam=10 * 1.10e-8),
       True: dict(v=10 * 5.92e-9, lam=10 * 7.16e-6, friction_torque=10 * 2.51e-5, limit_torque=0.0)}

# Stick and slide on a 0.2 rad slope (point 5 of the issue's test list): the robot of slope_scenario under its statics torque, 20 ticks,
# ideal joints.  The twin's own figures on the CPU (run this file) and the bounds the tests hold the code to (a factor 2 each):
#   mu = 2 tan:  largest tangential speed of a touching point over the run 6.62e-9 m/s                 -> at most 2 x that
#   mu = tan / 2: every touching point on its cone; downslope speed of the base at the end -7.23e-3 m/s -> above 2 x that
#                 smallest downslope speed of a touching point at the end 0.411 m/s                     -> above half of that
# The base speed is NEGATIVE: the open-loop robot does not slide down as a block; its feet slip out downhill under torques that count on
# the friction of statics (0.41 m/s after 40 ms, a rigid block would have 0.039) and the base recoils uphill, nearly twice as fast as the
# sticking robot's base tips (-3.86e-3 m/s).  So the base bound is kept as the issue words it and says little; what tells sliding from
# sticking is the speed of the feet, which the third bound holds.
SLOPE = 0.2
STICK_TWIN, SLIDE_BASE_TWIN, SLIDE_FEET_TWIN = 6.62e-9, -7.23e-3, 0.411
STICK_BOUND, SLIDE_BOUND, FEET_BOUND = 2.0 * STICK_TWIN, 2.0 * SLIDE_BASE_TWIN, 0.5 * SLIDE_FEET_TWIN


def build():
    so = HERE / "libterrainemu.so"
    deps = [HERE / "terrainemu.cpp", CSRC.parents[1] / "include" / "hunter_hip.h", *CSRC.glob("*.hpp")]
    with open(HERE / ".hostemu.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            tmp = HERE / f"libterrainemu.{os.getpid()}.so"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", str(tmp), str(HERE / "terrainemu.cpp")])
            os.replace(tmp, so)
    return so


_p = ce._p


# ---- the definition, in numpy ----------------------------------------------------------------------------------------------------------
def normal_of(pitch=0.0, roll=0.0):
    """Ry(pitch) Rx(roll) e_z."""
    return np.array([np.sin(pitch) * np.cos(roll), -np.sin(roll), np.cos(pitch) * np.cos(roll)])


def frame_of(n):
    """T = [t1 t2 n] (columns) of a unit normal."""
    n = np.asarray(n, dtype=float)
    t1 = np.array([1.0, 0.0, 0.0]) - n[0] * n
    t1 /= np.linalg.norm(t1)
    return np.stack([t1, np.cross(n, t1), n], axis=1)


def record_of(plane, mu):
    """The record the kernels stage for one instance: T row-major | d | mu[4] (plane = unit normal and d)."""
    return np.concatenate([frame_of(plane[:3]).reshape(9), [plane[3]], np.asarray(mu, dtype=float).reshape(4)])


def heights(foot_fn, q, plane):
    """n . x_c - d of the four contact points of q[16]."""
    return np.asarray(foot_fn(np.asarray(q)[None]))[0] @ plane[:3] - plane[3]


def place_on_terrain(q, foot_fn, plane):
    """ce.place_on_plane for a plane n . x = d, with the base left upright: base height and the ten joints changed (Gauss-Newton on the
    four heights along n, the least-norm step of each iteration) so that all four contact points lie on the plane.  The ankles take the
    slope; tilting the base with the plane instead puts the centre of mass behind the feet and the robot falls over backwards at once."""
    q = np.array(q, dtype=float)
    idx = [2] + list(range(6, 16))
    for _ in range(12):
        z = heights(foot_fn, q, plane)
        jac = np.zeros((4, len(idx)))
        for k, i in enumerate(idx):
            d = np.zeros(16)
            d[i] = 1e-6
            jac[:, k] = (heights(foot_fn, q + d, plane) - z) / 1e-6
        q[idx] += np.linalg.lstsq(jac, -z, rcond=None)[0]
    return q


def twin_substep(q, v, p, M, nle, J, feet, tau, wrench, plane, mu4, erp, sweeps, eps, h, jm=None, transposed=False):
    """One substep of one instance on a terrain.  p: 12 contact impulses in (t1, t2, n), then with jm the 20 joint impulses of
    tests/_jointemu.py.  feet[4][3] world.  -> (q+, v+, p, contact residual, joint residual).  transposed: the self-test's wrong frame."""
    T = frame_of(plane[:3])
    if transposed:
        T = T.T
    Jt = np.zeros((12, 16))
    for c in range(4):
        Jt[3 * c:3 * c + 3] = T.T @ J[3 * c:3 * c + 3]
    phi = np.asarray(feet) @ plane[:3] - plane[3]
    nr = 12 if jm is None else 32
    Mh = np.array(M, dtype=float)
    rhs = -np.asarray(nle, dtype=float).copy()
    rhs[6:] += tau
    p = np.array(p, dtype=float)
    Jh = np.zeros((nr, 16))
    Jh[:12] = Jt
    b = np.zeros(nr)
    b[2:12:3] = (np.maximum(phi, 0.0) + erp * np.minimum(phi, 0.0)) / h
    s = np.ones(10)
    if jm is not None:
        Mh[6:, 6:] += np.diag(jm["armature"] + h * jm["damping"])
        rhs[6:] -= jm["damping"] * v[6:]
        lo, up = q[6:] - jm["lower"], jm["upper"] - q[6:]
        s = np.where(lo <= up, 1.0, -1.0)
        phi_j = np.where(lo <= up, lo, up)
        for j in range(10):
            Jh[12 + j, 6 + j] = 1.0
            Jh[22 + j, 6 + j] = s[j]
        b[22:] = (np.maximum(phi_j, 0.0) + jm["limit_erp"] * np.minimum(phi_j, 0.0)) / h
        p[22:] = np.maximum(0.0, s * p[22:]) if jm["limits"] else 0.0
    if wrench is not None:
        rhs[0:3] += wrench[0:3]
        rhs[3:6] += ce._E1(q[3:6]).T @ wrench[3:6]
    vf = v + h * np.linalg.solve(Mh, rhs)
    MiJt = np.linalg.solve(Mh, Jh.T)
    W = Jh @ MiJt
    W[:12, :12] += eps * np.trace(W[:12, :12]) * np.eye(12)
    c = Jh @ vf + b
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
            nrm, lim = np.hypot(t[0], t[1]), mu4[pt] * p[n]
            if nrm > lim:
                t = t * (lim / nrm) if p[n] > 0.0 else np.zeros(2)
            res = max(res, abs(W[a, a] * (t[0] - p[a])), abs(W[a + 1, a + 1] * (t[1] - p[a + 1])))
            p[a:a + 2] = t
        if jm is not None:
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
    if jm is not None:
        p[22:] = s * p[22:]
    return q + h * vn, vn, p, res, jres


class TerrainPlant:
    """The terrain in numpy, batched: plane[B][4] (unit normal, d), mu[B][4]; jm = je.model_dict(...) or None.  State q, v, p[B][12]
    (components in the instance's frame), jp[B][20]; outputs as hb_plant_get_state / _get_contact / _get_joints.  qv_fn(q, v) -> (M, nle,
    J, ...) of one instance, foot_fn(q[B][16]) -> [B][4][3]."""

    def __init__(self, qv_fn, foot_fn, q0, v0, plane, mu, jm=None, wrench=None, sweeps=SWEEPS, erp=ERP, eps=EPS, tol=1e-3, fall_height=0.0,
                 transposed=False, shared_mu=False):
        self.qv_fn, self.foot_fn, self.jm = qv_fn, foot_fn, jm
        self.q, self.v = np.array(q0, dtype=float), np.array(v0, dtype=float)
        self.B = self.q.shape[0]
        self.plane, self.mu = np.array(plane, dtype=float), np.array(mu, dtype=float)
        if shared_mu:                                   # the self-test's wrong model: every point gets the first point's coefficient
            self.mu = np.repeat(self.mu[:, :1], 4, axis=1)
        self.transposed = transposed
        self.wrench, self.sweeps, self.erp, self.eps, self.tol, self.fall_height = wrench, sweeps, erp, eps, tol, fall_height
        self.p, self.jp = np.zeros((self.B, 12)), np.zeros((self.B, 20))
        self.status = np.zeros(self.B, dtype=np.int32)

    def frames(self):
        return np.array([frame_of(pl[:3]) for pl in self.plane])

    def step(self, tau, dt=DT, substeps=SUBSTEPS):
        h = dt / substeps
        tau = np.asarray(tau, dtype=float).reshape(self.B, 10)
        if self.jm is not None:
            tau = np.clip(tau, -self.jm["torque_limit"], self.jm["torque_limit"])
        self.tau_applied = tau
        self.residual, self.jresidual = np.zeros(self.B), np.zeros(self.B)
        self.point_vel = np.zeros((self.B, 12))
        for _ in range(substeps):
            feet = np.asarray(self.foot_fn(self.q)).reshape(self.B, 4, 3)
            v_old = self.v.copy()
            for i in range(self.B):
                M, nle, J = self.qv_fn(self.q[i], self.v[i])[:3]
                p = self.p[i] if self.jm is None else np.concatenate([self.p[i], self.jp[i]])
                self.q[i], self.v[i], p, self.residual[i], self.jresidual[i] = twin_substep(
                    self.q[i], self.v[i], p, M, nle, J, feet[i], tau[i], None if self.wrench is None else self.wrench[i], self.plane[i],
                    self.mu[i], self.erp, self.sweeps, self.eps, h, self.jm, self.transposed)
                self.p[i], self.jp[i] = p[:12], (p[12:] if self.jm is not None else self.jp[i])
                self.point_vel[i] = np.asarray(J) @ self.v[i]
            self.vdot = (self.v - v_old) / h
        T = self.frames()
        if self.transposed:
            T = T.transpose(0, 2, 1)
        self.lam = np.einsum("bak,bck->bca", T, self.p.reshape(self.B, 4, 3)).reshape(self.B, 12) / h
        self.friction_torque, self.limit_torque = self.jp[:, :10] / h, self.jp[:, 10:] / h
        self.touching = (self.p[:, 2::3] > 0.0).astype(np.int32)
        feet = np.asarray(self.foot_fn(self.q)).reshape(self.B, 4, 3)
        self.gap = np.einsum("bcx,bx->bc", feet, self.plane[:, :3]) - self.plane[:, 3:4]
        finite = np.isfinite(self.q).all(axis=1) & np.isfinite(self.v).all(axis=1)
        height = np.einsum("bx,bx->b", self.q[:, :3], self.plane[:, :3]) - self.plane[:, 3]
        fallen = (height < self.fall_height) if self.fall_height > 0.0 else np.zeros(self.B, dtype=bool)
        self.status = ((self.status & ce.FALLEN) | np.where(finite, 0, ce.NONFINITE) | np.where(fallen, ce.FALLEN, 0) |
                       np.where(self.residual <= self.tol, 0, ce.UNCONVERGED)).astype(np.int32)

    def record(self):
        keys = ("q", "v", "lam", "vdot", "gap", "point_vel", "residual", "touching", "status", "friction_torque", "limit_torque", "jresidual", "p")
        return {k: np.array(getattr(self, k)).copy() for k in keys}


def to_frame(lam, plane):
    """World forces lam[B][12] -> components in each instance's (t1, t2, n): [B][4][3]."""
    T = np.array([frame_of(pl[:3]) for pl in np.atleast_2d(plane)])
    return np.einsum("bak,bca->bck", T, np.asarray(lam).reshape(len(T), 4, 3))


# ---- the host build -----------------------------------------------------------------------------------------------------------------------
def emu_step(lib, mdl, cfg, rec, q, v, imp, tau, wrench=None, status=0, jm=None, jimp=None, cmd=None, eps=EPS, dt=DT, substeps=SUBSTEPS):
    """One tick of one instance on the host build.  rec: the terrain record or None (the routines without a terrain); jm: an
    abi.HbJointModel or None; cmd[5][10]: the hybrid form with this command (tau is not read).  -> dict of new arrays."""
    o = dict(q=np.array(q, dtype=float), v=np.array(v, dtype=float), p=np.array(imp, dtype=float), lam=np.zeros(12), vdot=np.zeros(16),
             gap=np.zeros(4), point_vel=np.zeros(12), residual=np.zeros(1), touching=np.zeros(4, dtype=np.int32),
             status=np.array([status], dtype=np.int32))
    j = dict(tau_applied=np.zeros(10), friction_torque=np.zeros(10), limit_torque=np.zeros(10), jresidual=np.zeros(1),
             jstatus=np.zeros(1, dtype=np.int32), tau_last=np.zeros(10))
    h = dict(tau_first=np.zeros(10), tau_mean=np.zeros(10))
    rec = None if rec is None else np.ascontiguousarray(rec, dtype=float)
    drive = np.ascontiguousarray(tau if cmd is None else cmd, dtype=float)
    w = None if wrench is None else np.ascontiguousarray(wrench, dtype=float)
    tail = [C.c_double(eps), C.c_double(dt), C.c_int(substeps)] + [_p(o[k]) for k in ("lam", "vdot", "gap", "point_vel", "residual", "touching", "status")]
    if jm is None:
        head = [C.byref(mdl), C.byref(cfg), _p(rec), _p(o["q"]), _p(o["v"]), _p(o["p"]), _p(drive), _p(w)]
        if cmd is None:
            lib.te_step(*head, *tail)
        else:
            lib.te_step_hybrid(*head, *tail, _p(h["tau_first"]), _p(h["tau_mean"]), _p(j["tau_last"]))
    else:
        o["jp"] = np.array(np.zeros(20) if jimp is None else jimp, dtype=float)
        head = [C.byref(mdl), C.byref(cfg), C.byref(jm), _p(rec), _p(o["q"]), _p(o["v"]), _p(o["p"]), _p(o["jp"]), _p(drive), _p(w)]
        jt = [_p(j[k]) for k in ("tau_applied", "friction_torque", "limit_torque", "jresidual", "jstatus", "tau_last")]
        if cmd is None:
            lib.te_joints_step(*head, *tail, *jt)
        else:
            lib.te_joints_step_hybrid(*head, *tail, *jt, _p(h["tau_first"]), _p(h["tau_mean"]))
    o.update(j)
    o.update(h)
    for k in ("residual", "jresidual"):
        o[k] = float(o[k][0])
    o["status"], o["jstatus"] = int(o["status"][0]), int(o["jstatus"][0])
    return o


# ---- the five scenarios -------------------------------------------------------------------------------------------------------------------
def scenarios(q_stand, qv_fn, foot_fn, rng=None):
    """The issue's table, one dict per instance: plane[4], mu[4], q0, v0, tau_fn(tick) -> [10].  Starts and torques in the style of the
    cases (a) - (d) of ce.make_case, placed on the instance's plane: 0 (a) flat; 1 (a) on a pitch slope of 0.2 rad; 2 (c) tilted, moving,
    random torques on a plane of pitch 0.15, roll -0.1 with four different coefficients; 3 (a) on the 0.2 rad slope with mu = 0.05: it
    slides; 4 (b) flat, the plane 2 mm under the feet: landing."""
    rng = np.random.default_rng(7) if rng is None else rng
    normals = [normal_of(), normal_of(SLOPE), normal_of(0.15, -0.1), normal_of(SLOPE), normal_of()]
    mus = [[0.7] * 4, [0.7] * 4, [0.9, 0.5, 0.3, 0.05], [0.05] * 4, [0.7] * 4]
    out = []
    for i, (n, mu) in enumerate(zip(normals, mus)):
        plane = np.concatenate([n, [0.0]])
        q0, v0 = place_on_terrain(q_stand, foot_fn, plane), np.zeros(16)
        M, nle, J = qv_fn(q0, v0)[:3]
        tau_s = ce.statics_torque(M, nle, J)
        tau_fn = lambda tick, t=tau_s: t  # noqa: E731
        if i == 2:
            q0[3:6] += [0.05, -0.02, 0.03]
            q0 = q0 + 0.0
            q0[0:3] += (0.0 - heights(foot_fn, q0, plane).min()) * n     # lowest point back onto the plane
            v0 = 0.05 * rng.standard_normal(16)
            taus = 3.0 * rng.standard_normal((max(TICKS), 10))
            tau_fn = lambda tick, t=taus: t[tick]  # noqa: E731
        if i == 4:
            plane[3] = -0.002
        out.append(dict(plane=plane, mu=np.array(mu), q0=q0, v0=v0, tau_fn=tau_fn))
    return out


def slope_scenario(q_stand, qv_fn, foot_fn, factor):
    """Point 5: standing on the 0.2 rad slope under the statics torque with mu = factor * tan(slope) on every point."""
    plane = np.concatenate([normal_of(SLOPE), [0.0]])
    q0 = place_on_terrain(q_stand, foot_fn, plane)
    M, nle, J = qv_fn(q0, np.zeros(16))[:3]
    tau = ce.statics_torque(M, nle, J)
    return dict(plane=plane, mu=np.full(4, factor * np.tan(SLOPE)), q0=q0, v0=np.zeros(16), tau_fn=lambda tick: tau)


def stick_slide_figures(recs, plane, mu):
    """From the records of a run of ONE instance (each: lam[12], point_vel[12], touching[4], v[16]) -> dict(speed = largest tangential speed
    of a touching point over the run, base_down = downslope base speed at the end (t1 points down a pitch slope), feet_down = smallest
    downslope speed of a touching point at the end, on_cone = all touching points of the last record on their cone to 1e-9 relative)."""
    T = frame_of(plane[:3])
    worst, on_cone, feet_down = 0.0, True, np.inf
    for r in recs:
        vel = np.asarray(r["point_vel"]).reshape(4, 3) @ T
        for c in range(4):
            if r["touching"][c]:
                worst = max(worst, np.hypot(vel[c, 0], vel[c, 1]))
    p = to_frame(np.asarray(recs[-1]["lam"])[None], plane[None])[0]
    for c in range(4):
        if recs[-1]["touching"][c]:
            on_cone = on_cone and abs(np.hypot(p[c, 0], p[c, 1]) - mu[c] * p[c, 2]) <= 1e-9 * mu[c] * p[c, 2]
            feet_down = min(feet_down, vel[c, 0])
    return dict(speed=float(worst), base_down=float(np.asarray(recs[-1]["v"])[:3] @ T[:, 0]), feet_down=float(feet_down), on_cone=bool(on_cone))


def check_stick_slide(stick, slide):
    """Point 5 on the figures of the two runs (stick_slide_figures)."""
    assert stick["speed"] <= STICK_BOUND, ("mu = 2 tan: a touching point moves", stick["speed"])
    assert slide["on_cone"], "mu = tan / 2: a touching point is inside its cone"
    assert slide["base_down"] >= SLIDE_BOUND, ("mu = tan / 2: downslope speed of the base", slide["base_down"])
    assert slide["feet_down"] >= FEET_BOUND, ("mu = tan / 2: the feet do not slide down", slide["feet_down"])


# ---- the checks (one instance: dev = outputs of the code under test, twin = a row of TerrainPlant.record()) ----------------------------------
def check_against_twin(dev, twin, joints):
    """Point 1: q 1e-10; v, lambda / max(1, |lambda|) and with the joint model friction / limit torque at 10 x the twin's sensitivity; the
    other outputs of hb_plant_get_contact at the tolerances of tests/test_gpu_contact_plant.py."""
    tol = TOL[joints]
    errs = dict(q=np.abs(dev["q"] - twin["q"]).max(), v=np.abs(dev["v"] - twin["v"]).max(),
                lam=np.abs(dev["lam"] - twin["lam"]).max() / max(1.0, np.abs(twin["lam"]).max()))
    assert errs["q"] <= TOL_Q and errs["v"] <= tol["v"] and errs["lam"] <= tol["lam"], ("against the twin", errs)
    if joints:
        for k in ("friction_torque", "limit_torque"):
            errs[k] = np.abs(dev[k] - twin[k]).max()
            assert errs[k] <= tol[k], ("against the twin", k, errs[k])
    assert np.abs(dev["vdot"] - twin["vdot"]).max() <= tol["v"] / H
    assert np.abs(dev["gap"] - twin["gap"]).max() <= TOL_Q
    assert np.abs(np.ravel(dev["point_vel"]) - twin["point_vel"]).max() <= 10 * tol["v"]
    assert abs(dev["residual"] - twin["residual"]) <= tol["v"] and np.array_equal(dev["touching"], twin["touching"])
    return errs


def check_properties(lam, point_vel, touching, plane, mu):
    """Point 4, independent of the twin, one instance: lambda . n >= 0; |lambda - (lambda . n) n| <= mu_c (lambda . n) (1 + 1e-12);
    touching == (lambda . n > 0); a sliding point (tangential speed > 1e-3 m/s in the plane) lies on its cone to 1e-9 relative and its
    tangential force opposes its tangential velocity.  -> number of sliding points."""
    n = plane[:3]
    lam, vel = np.asarray(lam).reshape(4, 3), np.asarray(point_vel).reshape(4, 3)
    fn = lam @ n
    ft = lam - fn[:, None] * n
    assert (fn >= 0.0).all(), ("lambda . n", fn)
    assert (np.linalg.norm(ft, axis=1) <= mu * fn * (1.0 + 1e-12)).all(), ("cone", np.linalg.norm(ft, axis=1) - mu * fn)
    assert np.array_equal(np.asarray(touching) != 0, fn > 0.0)
    vt = vel - (vel @ n)[:, None] * n
    sliding = 0
    for c in range(4):
        if touching[c] and np.linalg.norm(vt[c]) > 1e-3:
            sliding += 1
            assert abs(np.linalg.norm(ft[c]) - mu[c] * fn[c]) <= 1e-9 * mu[c] * fn[c], ("a sliding point is off its cone", c)
            assert ft[c] @ vt[c] < 0.0 or mu[c] == 0.0, ("friction does not oppose the sliding", c)
    return sliding


ROUND = je.ROUND


def check_base_momentum(lam, v_out, v_in, M, nle, h, f_ext=None):
    """A tick of ONE substep from v_in: the three base-linear rows (M dv / h + nle)[0:3] = sum_c lambda_c + F_ext, with M, nle from outside
    the code under test at the start of the tick.  Bound: 64 roundings of the terms (je.check_momentum_row: the inertial term as the
    Cholesky solve leaves it, nle with its largest entry).  Pins lambda as WORLD forces."""
    dv = (np.asarray(v_out) - v_in) / h
    row = (np.asarray(M) @ dv + nle)[0:3]
    lam = np.asarray(lam).reshape(4, 3)
    rhs = lam.sum(axis=0) + (0.0 if f_ext is None else np.asarray(f_ext)[:3])
    root = np.sqrt(np.diag(M))
    scale = (root * (root @ np.abs(dv)))[0:3] + np.abs(nle).max() + np.abs(lam).sum(axis=0) + np.abs(rhs)
    assert (np.abs(row - rhs) <= ROUND * scale).all(), ("base momentum rows", np.abs(row - rhs), ROUND * scale)


def measure_sensitivity(params, q_stand, qv_fn, foot_fn, joints, draws=3, rel=1e-12):
    """Largest change of the twin's v, lambda / max(1, |lambda|), friction torque and limit torque after one tick when q, v, the warm-start
    impulses and every M, nle, J are perturbed by relative `rel`, over the ticks of the five scenarios -> [(dv, dlam, dfriction, dlimit)]."""
    jm = je.model_dict(abi.make_joint_model(params)) if joints else None
    out = []
    for i, sc in enumerate(scenarios(q_stand, qv_fn, foot_fn)):
        rng = np.random.default_rng(7)
        mk = lambda fn: TerrainPlant(fn, foot_fn, sc["q0"][None], sc["v0"][None], sc["plane"][None], sc["mu"][None], jm)  # noqa: E731
        base, worst = mk(qv_fn), np.zeros(4)
        for tick in range(TICKS[i]):
            tau = sc["tau_fn"](tick)
            q, v, p, jp = base.q.copy(), base.v.copy(), base.p.copy(), base.jp.copy()
            base.step(tau[None])
            for _ in range(draws):
                pert = lambda x: x * (1.0 + rel * rng.uniform(-1.0, 1.0, np.shape(x)))  # noqa: E731
                tw = mk(lambda qq, vv: tuple(pert(np.asarray(x)) for x in qv_fn(qq, vv)[:3]))
                tw.q, tw.v, tw.p, tw.jp = pert(q), pert(v), pert(p), pert(jp)
                tw.step(tau[None])
                worst = np.maximum(worst, [np.abs(tw.v - base.v).max(), np.abs(tw.lam - base.lam).max() / max(1.0, np.abs(base.lam).max()),
                                           np.abs(tw.friction_torque - base.friction_torque).max(),
                                           np.abs(tw.limit_torque - base.limit_torque).max()])
        out.append(tuple(worst))
    return out


def twin_stick_slide(q_stand, qv_fn, foot_fn, factor, ticks=20):
    sc = slope_scenario(q_stand, qv_fn, foot_fn, factor)
    tw = TerrainPlant(qv_fn, foot_fn, sc["q0"][None], sc["v0"][None], sc["plane"][None], sc["mu"][None])
    recs = []
    for tick in range(ticks):
        tw.step(sc["tau_fn"](tick)[None])
        recs.append({k: a[0] for k, a in tw.record().items()})
    return stick_slide_figures(recs, sc["plane"], sc["mu"])


if __name__ == "__main__":
    from hunter_bipedal_control_amd import ingest   # (run with the repository root and tests/ on PYTHONPATH)
    prm = ingest.load_packaged()
    qv, foot, qs = ce.oracle_fns(prm)
    for joints in (False, True):
        for i, w in enumerate(measure_sensitivity(prm, qs, qv, foot, joints)):
            print(f"joint model {joints} scenario {i}: |dv| {w[0]:.2e}  |dlambda| rel {w[1]:.2e}  |d friction| {w[2]:.2e}  |d limit| {w[3]:.2e}")
    print("stick (mu = 2 tan): largest tangential speed of a touching point, downslope base speed, on cone:", twin_stick_slide(qs, qv, foot, 2.0))
    print("slide (mu = tan / 2):", twin_stick_slide(qs, qv, foot, 0.5))
