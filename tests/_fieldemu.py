"""Helpers of the height-field tests of the ground-contact plant (tests/test_field_plant_host.py, tests/test_gpu_field_plant.py):

  * build() of tests/host_emu/libfieldemu.so — the field forms of csrc/hb_contact.hpp / hb_joints.hpp (TERRAIN 3) compiled for the host
    behind a tiny C API (fieldemu.cpp), under the file lock of tests/_hostemu.py, installed atomically, rebuilt when a source is newer;
  * an independent numpy twin of the field as include/hunter_hip.h defines it: facet() is new code for the selection and the plane
    (np.floor / np.clip, the plane from the triangle's two slopes), the substep is tests/_profileemu.py twin_substep, which takes a plane
    per point.  The twin also keeps the smallest distance, in metres in (u, w), of any contact point and of the base origin from any
    interior node line and from the diagonal of its cell (margin): a comparison is valid only where both sides chose the same facets;
  * the six scenarios of the issue, one per instance, the checks the tests share, and the measurement behind the tolerances
    (measure_sensitivity; run this file to print it together with the twin's own figures).

Tolerances of "code under test against twin, one tick from the same (q, v, p)".  q: 1e-10, the plant's.  v, lambda / max(1, |lambda|) and,
with the joint model, friction and limit torque: 10 x the twin's OWN sensitivity, the largest change of its outputs over the ticks of the
six scenarios when q, v, the warm-start impulses and every M, nle, J are perturbed by relative 1e-12 (the method of
_profileemu.measure_sensitivity: 3 draws per tick, oracle rigid-body terms).  The figures are in SENS below.
"""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import _contactemu as ce
import _jointemu as je
import _profileemu as pe
import _terrainemu as te
from hunter_bipedal_control_amd import abi, rollout

HERE, CSRC = ce.HERE, ce.CSRC
DT, SUBSTEPS, EPS, H, SWEEPS, ERP = ce.DT, ce.SUBSTEPS, ce.EPS, ce.H, ce.SWEEPS, ce.ERP
B = 6
TICKS = 20
MARGIN = 1e-6                      # [m] in (u, w): every point and the base origin stay this far from every node line and diagonal
CFG_MU, CFG_GROUND = 0.6, 0.004    # the contact configuration of the batch: what scenario (0) is level at; no other scenario reads them
NMAX = abi.HB_FIELD_MAX_NODES
twin_substep = pe.twin_substep

# measure_sensitivity on the CPU oracle (run this file), per scenario (0) .. (5) and the largest:
SENS = {
    False: dict(v=(3.35e-9, 1.84e-9, 4.13e-8, 1.85e-9, 6.45e-10, 1.75e-9),                  # |dv| [m/s, rad/s]             -> 4.13e-08
                lam=(1.14e-8, 3.27e-11, 6.17e-8, 2.30e-8, 8.49e-8, 5.46e-9)),               # |dlambda| / max(1, |lambda|)  -> 8.49e-08
    True: dict(v=(4.49e-9, 2.70e-9, 5.62e-9, 1.43e-8, 3.91e-9, 3.77e-9),                    #                               -> 1.43e-08
               lam=(7.20e-6, 1.79e-7, 6.11e-8, 7.83e-6, 2.00e-7, 6.84e-6),                  #                               -> 7.83e-06
               friction_torque=(2.52e-5, 1.36e-6, 1.06e-8, 2.53e-5, 1.29e-7, 2.20e-5),      # [N m]                         -> 2.53e-05
               limit_torque=(0.0,) * 6),                                                    # no stop is reached: exactly zero
}
TOL_Q = 1e-10


def tol(joints):
    return {k: 10.0 * max(v) for k, v in SENS[joints].items()}


def build():
    so = HERE / "libfieldemu.so"
    deps = [HERE / "fieldemu.cpp", CSRC.parents[1] / "include" / "hunter_hip.h", *CSRC.glob("*.hpp")]
    with open(HERE / ".hostemu.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            tmp = HERE / f"libfieldemu.{os.getpid()}.so"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", str(tmp), str(HERE / "fieldemu.cpp")])
            os.replace(tmp, so)
    return so


_p = ce._p


# ---- the definition, in numpy ----------------------------------------------------------------------------------------------------------
def facet(fld, x, mutant=None):
    """The facet under the world points x[N][3] of one field dict(dir, origin, spacing, heights[nu][nw]): ids[N], planes[N][4] = (n, d),
    dist[N] = the distance in metres in (u, w) from the nearest interior node line or the diagonal of the cell.  mutant: "swap" chooses the
    triangles the other way round (the upper one where fu > fw), "wrong_edge" takes r of the lower triangle from the edge i instead of
    i + 1: the self-test's wrong definitions."""
    a = np.asarray(fld["dir"], dtype=float)
    a = a / np.linalg.norm(a)
    b = np.array([-a[1], a[0]])
    z = np.asarray(fld["heights"], dtype=float)
    nu, nw = z.shape
    (u0, w0), (du, dw) = fld["origin"], fld["spacing"]
    x = np.atleast_2d(np.asarray(x, dtype=float))
    ids, planes, dist = np.zeros(len(x), dtype=np.int32), np.zeros((len(x), 4)), np.zeros(len(x))
    for k, pt in enumerate(x):
        u, w = a @ pt[:2] - u0, b @ pt[:2] - w0
        i, j = int(np.clip(np.floor(u / du), 0, nu - 2)), int(np.clip(np.floor(w / dw), 0, nw - 2))
        fu, fw = u / du - i, w / dw - j
        lower = (fu >= fw) != (mutant == "swap")
        if lower:
            p, r = (z[i + 1, j] - z[i, j]) / du, (z[i + 1, j + 1] - z[i + 1, j]) / dw
            if mutant == "wrong_edge":
                r = (z[i, j + 1] - z[i, j]) / dw
        else:
            r, p = (z[i, j + 1] - z[i, j]) / dw, (z[i + 1, j + 1] - z[i, j + 1]) / du
        n = np.array([-(p * a[0] + r * b[0]), -(p * a[1] + r * b[1]), 1.0]) / np.sqrt(1.0 + p * p + r * r)
        node = np.array([*(a * (u0 + i * du) + b * (w0 + j * dw)), z[i, j]])
        ids[k] = 2 * (i * (nw - 1) + j) + (0 if lower else 1)
        planes[k] = [*n, n @ node]
        lines = [abs(u - m * du) for m in range(1, nu - 1)] + [abs(w - m * dw) for m in range(1, nw - 1)]
        dist[k] = min(lines + [abs(fu - fw) / np.hypot(1.0 / du, 1.0 / dw)])
    return ids, planes, dist


def surface_height(fld, x):
    """n_c . x - d_c of the world points x[N][3] over the facet under each."""
    pl = facet(fld, x)[1]
    return np.einsum("cx,cx->c", np.atleast_2d(x), pl[:, :3]) - pl[:, 3]


def place_on_field(q, foot_fn, fld, lift=0.0):
    """pe.place_on_profile for a field: base height and the ten joints changed (Gauss-Newton, least-norm steps) so that each contact point
    lies `lift` above the facet under it; the base stays upright."""
    q = np.array(q, dtype=float)
    idx = [2] + list(range(6, 16))
    hts = lambda qq: surface_height(fld, np.asarray(foot_fn(qq[None])).reshape(4, 3)) - lift  # noqa: E731
    for _ in range(12):
        z = hts(q)
        jac = np.zeros((4, len(idx)))
        for k, i in enumerate(idx):
            d = np.zeros(16)
            d[i] = 1e-6
            jac[:, k] = (hts(q + d) - z) / 1e-6
        q[idx] += np.linalg.lstsq(jac, -z, rcond=None)[0]
    return q


class FieldPlant:
    """The field in numpy, batched: fields = [B] dicts(dir[2], origin[2], spacing[2], heights[nu][nw], mu[4]); jm = je.model_dict(...) or
    None.  State and outputs as pe.ProfilePlant, with facet[B][5] (hb_plant_get_terrain_field) in the place of segment and margin = the
    smallest distance of a point or the base origin from a node line or a diagonal over every selection of the last step()."""

    def __init__(self, qv_fn, foot_fn, q0, v0, fields, jm=None, wrench=None, sweeps=SWEEPS, erp=ERP, eps=EPS, tol=1e-3, fall_height=0.0,
                 mutant=None):
        self.qv_fn, self.foot_fn, self.jm = qv_fn, foot_fn, jm
        self.q, self.v = np.array(q0, dtype=float), np.array(v0, dtype=float)
        self.B = self.q.shape[0]
        self.fields, self.mutant = fields, mutant
        self.wrench, self.sweeps, self.erp, self.eps, self.tol, self.fall_height = wrench, sweeps, erp, eps, tol, fall_height
        self.p, self.jp = np.zeros((self.B, 12)), np.zeros((self.B, 20))
        self.status = np.zeros(self.B, dtype=np.int32)
        self.margin = np.inf

    def _pick(self, i, x):
        ids, planes, dist = facet(self.fields[i], x, self.mutant)
        self.margin = min(self.margin, float(np.min(dist)))
        return ids, planes

    def step(self, tau, dt=DT, substeps=SUBSTEPS):
        h = dt / substeps
        tau = np.asarray(tau, dtype=float).reshape(self.B, 10)
        if self.jm is not None:
            tau = np.clip(tau, -self.jm["torque_limit"], self.jm["torque_limit"])
        self.tau_applied = tau
        self.residual, self.jresidual = np.zeros(self.B), np.zeros(self.B)
        self.point_vel = np.zeros((self.B, 12))
        self.margin = np.inf
        last = [None] * self.B
        for _ in range(substeps):
            feet = np.asarray(self.foot_fn(self.q)).reshape(self.B, 4, 3)
            v_old = self.v.copy()
            for i in range(self.B):
                M, nle, J = self.qv_fn(self.q[i], self.v[i])[:3]
                p = self.p[i] if self.jm is None else np.concatenate([self.p[i], self.jp[i]])
                w = None if self.wrench is None else self.wrench[i]
                self._pick(i, self.q[i, None, :3])                                   # (the base origin counts for the margin)
                pl = self._pick(i, feet[i])[1]
                self.q[i], self.v[i], p, self.residual[i], self.jresidual[i] = twin_substep(
                    self.q[i], self.v[i], p, M, nle, J, feet[i], tau[i], w, pl, self.fields[i]["mu"], self.erp, self.sweeps, self.eps, h, self.jm)
                self.p[i], self.jp[i] = p[:12], (p[12:] if self.jm is not None else self.jp[i])
                self.point_vel[i] = np.asarray(J) @ self.v[i]
                last[i] = pl
            self.vdot = (self.v - v_old) / h
        self.lam = np.zeros((self.B, 12))
        for i in range(self.B):
            for c in range(4):
                self.lam[i, 3 * c:3 * c + 3] = te.frame_of(last[i][c][:3]) @ self.p[i, 3 * c:3 * c + 3] / h
        self.last_planes = np.array(last)
        self.friction_torque, self.limit_torque = self.jp[:, :10] / h, self.jp[:, 10:] / h
        self.touching = (self.p[:, 2::3] > 0.0).astype(np.int32)
        feet = np.asarray(self.foot_fn(self.q)).reshape(self.B, 4, 3)
        self.facet = np.zeros((self.B, 5), dtype=np.int32)
        self.gap, height = np.zeros((self.B, 4)), np.zeros(self.B)
        self.base_plane = np.zeros((self.B, 4))
        for i in range(self.B):
            ids, pl = self._pick(i, feet[i])
            bid, bpl = self._pick(i, self.q[i, None, :3])
            self.facet[i] = [*ids, bid[0]]
            self.gap[i] = np.einsum("cx,cx->c", feet[i], pl[:, :3]) - pl[:, 3]
            height[i] = self.q[i, :3] @ bpl[0, :3] - bpl[0, 3]
            self.base_plane[i] = bpl[0]
        finite = np.isfinite(self.q).all(axis=1) & np.isfinite(self.v).all(axis=1)
        fallen = (height < self.fall_height) if self.fall_height > 0.0 else np.zeros(self.B, dtype=bool)
        self.status = ((self.status & ce.FALLEN) | np.where(finite, 0, ce.NONFINITE) | np.where(fallen, ce.FALLEN, 0) |
                       np.where(self.residual <= self.tol, 0, ce.UNCONVERGED)).astype(np.int32)

    def record(self):
        keys = ("q", "v", "lam", "vdot", "gap", "point_vel", "residual", "touching", "status", "friction_torque", "limit_torque", "jresidual", "p",
                "facet", "last_planes", "base_plane")
        out = {k: np.array(getattr(self, k)).copy() for k in keys}
        out["margin"] = np.full(self.B, self.margin)
        return out


# ---- the host build -----------------------------------------------------------------------------------------------------------------------
def padded(heights):
    z = np.zeros((NMAX, NMAX))
    h = np.asarray(heights, dtype=float)
    z[:h.shape[0], :h.shape[1]] = h
    return z


def emu_record(lib, fld, cfg_mu=CFG_MU, n=None):
    """(hdr, z[32][32]) of one field by the host setter's routine (raises ValueError with its refusal); n overrides the node counts."""
    z = padded(np.asarray(fld["heights"], dtype=float)[:NMAX, :NMAX])
    nn = np.array(np.shape(fld["heights"]) if n is None else n, dtype=np.int32)
    hdr, why = np.zeros(lib.fe_stored_size()), C.create_string_buffer(128)
    mu = None if fld.get("mu") is None else np.ascontiguousarray(fld["mu"], dtype=float)
    f64 = lambda k: np.ascontiguousarray(fld[k], dtype=float)  # noqa: E731
    if lib.fe_record(_p(nn), _p(f64("dir")), _p(f64("origin")), _p(f64("spacing")), _p(z), _p(mu), C.c_double(cfg_mu), _p(hdr), why):
        raise ValueError(why.value.decode())
    return hdr, z


def emu_facet(lib, rec, x):
    """field_facet of the host build on x[N][3] -> (ids[N], records[N][10])."""
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=float)
    ids, recs = np.zeros(len(x), dtype=np.int32), np.zeros((len(x), 10))
    lib.fe_facet(_p(rec[0]), _p(rec[1]), C.c_int(len(x)), _p(x), _p(ids), _p(recs))
    return ids, recs


def record_of_plane(pl):
    """The twin's 10-double record (T row-major, d) of a plane (n, d)."""
    return np.concatenate([te.frame_of(pl[:3]).reshape(9), [pl[3]]])


def emu_step(lib, mdl, cfg, rec, q, v, imp, tau, wrench=None, status=0, jm=None, jimp=None, cmd=None, eps=EPS, dt=DT, substeps=SUBSTEPS):
    """One tick of one instance on the host build, rec = (hdr, z) of emu_record; otherwise pe.emu_step.  -> dict of new arrays, with facet[5]
    and base[14]."""
    o = dict(q=np.array(q, dtype=float), v=np.array(v, dtype=float), p=np.array(imp, dtype=float), lam=np.zeros(12), vdot=np.zeros(16),
             gap=np.zeros(4), point_vel=np.zeros(12), residual=np.zeros(1), touching=np.zeros(4, dtype=np.int32),
             status=np.array([status], dtype=np.int32))
    j = dict(tau_applied=np.zeros(10), friction_torque=np.zeros(10), limit_torque=np.zeros(10), jresidual=np.zeros(1),
             jstatus=np.zeros(1, dtype=np.int32), tau_last=np.zeros(10))
    hy = dict(tau_first=np.zeros(10), tau_mean=np.zeros(10))
    pr = dict(facet=np.zeros(5, dtype=np.int32), base=np.zeros(14))
    hdr, z = (np.ascontiguousarray(a, dtype=float) for a in rec)
    drive = np.ascontiguousarray(tau if cmd is None else cmd, dtype=float)
    w = None if wrench is None else np.ascontiguousarray(wrench, dtype=float)
    tail = [C.c_double(eps), C.c_double(dt), C.c_int(substeps)] + [_p(o[k]) for k in ("lam", "vdot", "gap", "point_vel", "residual", "touching", "status")]
    end = [_p(pr["facet"]), _p(pr["base"])]
    if jm is None:
        head = [C.byref(mdl), C.byref(cfg), _p(hdr), _p(z), _p(o["q"]), _p(o["v"]), _p(o["p"]), _p(drive), _p(w)]
        if cmd is None:
            lib.fe_step(*head, *tail, *end)
        else:
            lib.fe_step_hybrid(*head, *tail, _p(hy["tau_first"]), _p(hy["tau_mean"]), _p(j["tau_last"]), *end)
    else:
        o["jp"] = np.array(np.zeros(20) if jimp is None else jimp, dtype=float)
        head = [C.byref(mdl), C.byref(cfg), C.byref(jm), _p(hdr), _p(z), _p(o["q"]), _p(o["v"]), _p(o["p"]), _p(o["jp"]), _p(drive), _p(w)]
        jt = [_p(j[k]) for k in ("tau_applied", "friction_torque", "limit_torque", "jresidual", "jstatus", "tau_last")]
        if cmd is None:
            lib.fe_joints_step(*head, *tail, *jt, *end)
        else:
            lib.fe_joints_step_hybrid(*head, *tail, *jt, _p(hy["tau_first"]), _p(hy["tau_mean"]), *end)
    o.update(j)
    o.update(hy)
    o.update(pr)
    for k in ("residual", "jresidual"):
        o[k] = float(o[k][0])
    o["status"], o["jstatus"] = int(o["status"][0]), int(o["jstatus"][0])
    return o


# ---- the six scenarios --------------------------------------------------------------------------------------------------------------------
PITCH1, ROLL1, STEP2, LIFT2, CROSS3, RAMP3, MU4, SPEED4 = 0.2, 0.1, 0.01, 0.002, 0.15, 0.1, 0.3, 0.1
PROFILE2_DU = 0.02


def profile2(q_stand, foot_fn):
    """The curb of scenario (2) as a terrain profile: level at the standing height of the contact points, a riser down STEP2 over one grid
    step PROFILE2_DU (slope 0.5) that starts 5 mm ahead of the heel points, level again; knots on a grid of PROFILE2_DU."""
    f0 = np.asarray(foot_fn(np.asarray(q_stand)[None])).reshape(4, 3)
    riser, z0 = np.sort(f0[:, 0])[:2].mean() + 0.005, f0[:, 2].min()
    return dict(dir=np.array([1.0, 0.0]), mu=np.full(4, 0.7),
                knots=np.array([[riser - 15 * PROFILE2_DU, z0], [riser, z0], [riser + PROFILE2_DU, z0 - STEP2], [riser + 15 * PROFILE2_DU, z0 - STEP2]]))


def plane1():
    """The oblique plane of scenario (1): unit normal and offset (through the origin)."""
    n = np.array([np.tan(PITCH1), -np.tan(ROLL1), 1.0])
    return np.concatenate([n / np.linalg.norm(n), [0.0]])


def scenarios(q_stand, qv_fn, foot_fn):
    """The issue's table, one dict per instance: dir[2], origin[2], spacing[2], heights[nu][nw], mu[4], q0, v0, tau[10] (held; the statics
    torque of the start unless said).  Contact points: per foot a heel and a toe point; heel / toe = mean x of the two rear / front points
    of the standing configuration, right / left = mean y of the two with the smaller / larger y.
      (0) level at CFG_GROUND with CFG_MU, 5 x 4 nodes on a grid along (0.6, 0.8); the robot stands on it.
      (1) the plane plane1() (pitch 0.2, roll 0.1 rad) sampled on a 6 x 5 grid along (0.8, 0.6); every point placed on it.
      (2) profile2() through rollout.field_from_profile: the robot starts LIFT2 above the upper level with zero torque and drops, the toe
          points hang over the lower level.
      (3) right foot: facets that rise along u and twist along w; left foot: a pure cross slope of CROSS3 rad along w.  Every point placed
          on its facet.  No profile has these two grounds side by side.
      (4) a bump: one cell per foot, heel and toe point of a foot on the two triangles of its cell, node heights up to 2 cm, mu MU4; the
          robot is placed on the four facets and starts with SPEED4 along x, so it slides or rocks over the bump.
      (5) a 3 x 3 grid that ends between the heel and the toe points: the toe points stand beyond the border on the continued planes of
          the last cells."""
    f0 = np.asarray(foot_fn(np.asarray(q_stand)[None])).reshape(4, 3)
    xs, ys = np.sort(f0[:, 0]), np.sort(f0[:, 1])
    heel, toe, right, left = xs[:2].mean(), xs[2:].mean(), ys[:2].mean(), ys[2:].mean()
    z0, length, gap = f0[:, 2].min(), toe - heel, left - right
    pl1 = plane1()
    a1 = np.array([0.8, 0.6])
    b1 = np.array([-0.6, 0.8])
    g1 = np.array([[-(pl1[:2] @ (a1 * (-0.6 + 0.25 * i) + b1 * (-0.55 + 0.3 * j))) / pl1[2] for j in range(5)] for i in range(6)])
    du4, dw4 = length / 0.6, gap
    u3 = heel - 0.23
    flds = [
        dict(dir=[0.6, 0.8], origin=[-0.31, -0.27], spacing=[0.17, 0.19], heights=np.full((5, 4), CFG_GROUND), mu=[CFG_MU] * 4),
        dict(dir=a1, origin=[-0.6, -0.55], spacing=[0.25, 0.3], heights=g1, mu=[0.7] * 4),
        rollout.field_from_profile(**{k: v for k, v in profile2(q_stand, foot_fn).items() if k != "dir"}, direction=[1.0, 0.0], du=PROFILE2_DU),
        dict(dir=[1.0, 0.0], origin=[u3, -0.3 + 0.5 * (left + right)], spacing=[0.6, 0.3],
             heights=z0 + np.array([[RAMP3 * 0.0, 0.0, 0.3 * np.tan(CROSS3)], [RAMP3 * 0.6, 0.0, 0.3 * np.tan(CROSS3)], [RAMP3 * 1.2, 0.0, 0.3 * np.tan(CROSS3)]]),
             mu=[0.7] * 4),
        dict(dir=[1.0, 0.0], origin=[heel - 0.2 * du4 - du4, right - 0.5 * dw4 - dw4], spacing=[du4, dw4],
             heights=z0 + 0.02 * np.array([[0.1, 0.5, 0.3, 0.2], [0.4, 0.0, 0.6, 0.1], [0.2, 0.8, 0.2, 0.9], [0.5, 0.3, 0.7, 0.4]]), mu=[MU4] * 4),
        dict(dir=[1.0, 0.0], origin=[0.5 * (heel + toe) - 0.4, -0.4 + 0.5 * (left + right)], spacing=[0.2, 0.4],
             heights=z0 + np.array([[0.0, 0.002, 0.001], [0.004, 0.006, 0.003], [0.012, 0.010, 0.013]]), mu=[0.7] * 4),
    ]
    out = []
    for i, fl in enumerate(flds):
        fl = {k: np.asarray(v, dtype=float) for k, v in fl.items()}
        if i == 2:
            q0 = np.array(q_stand, dtype=float)
            q0[2] += LIFT2
        else:
            q0 = place_on_field(q_stand, foot_fn, fl)
        M, nle, J = qv_fn(q0, np.zeros(16))[:3]
        tau = ce.statics_torque(M, nle, J) if i != 2 else np.zeros(10)   # (2): limp, the robot drops as it stands
        v0 = np.zeros(16)
        if i == 4:
            v0[0] = SPEED4
        out.append(dict(fl, q0=q0, v0=v0, tau=tau))
    return out


def pack(scen):
    """-> the arguments of HunterSolver.plant_set_terrain_field."""
    return rollout.pack_fields(scen)


# ---- the checks (one instance: dev = outputs of the code under test, twin = a row of FieldPlant.record()) ---------------------------------
def check_against_twin(dev, twin, joints):
    """The margin first: the comparison is valid only where both sides chose the same facets.  Then q 1e-10; v, lambda / max(1, |lambda|) and
    with the joint model friction / limit torque at 10 x the twin's sensitivity; the other outputs as pe.check_against_twin; the facet ids
    under the points and the base ==."""
    assert twin["margin"] >= MARGIN, ("a point or the base origin within 1e-6 m of a node line or a diagonal", twin["margin"])
    t = tol(joints)
    errs = dict(q=np.abs(dev["q"] - twin["q"]).max(), v=np.abs(dev["v"] - twin["v"]).max(),
                lam=np.abs(dev["lam"] - twin["lam"]).max() / max(1.0, np.abs(twin["lam"]).max()))
    print("against the twin:", {k: f"{e:.3e}" for k, e in errs.items()}, "bounds", TOL_Q, t["v"], t["lam"])
    assert errs["q"] <= TOL_Q and errs["v"] <= t["v"] and errs["lam"] <= t["lam"], ("against the twin", errs)
    if joints:
        for k in ("friction_torque", "limit_torque"):
            errs[k] = np.abs(dev[k] - twin[k]).max()
            assert errs[k] <= t[k], ("against the twin", k, errs[k])
    assert np.abs(dev["vdot"] - twin["vdot"]).max() <= t["v"] / H
    assert np.abs(dev["gap"] - twin["gap"]).max() <= TOL_Q
    assert np.abs(np.ravel(dev["point_vel"]) - twin["point_vel"]).max() <= 10 * t["v"]
    assert abs(dev["residual"] - twin["residual"]) <= t["v"] and np.array_equal(dev["touching"], twin["touching"])
    assert np.array_equal(dev["facet"], twin["facet"]), ("facets", dev["facet"], twin["facet"])
    return errs


# every touching point's force lies in the cone of its own facet: the profile's bound (rounding of T' T p)
CONE_BOUND = pe.CONE_BOUND
check_cone = pe.check_cone
check_base_momentum = te.check_base_momentum


def measure_sensitivity(params, q_stand, qv_fn, foot_fn, joints, draws=3, rel=1e-12):
    """pe.measure_sensitivity on the six field scenarios -> [(dv, dlam, dfriction, dlimit)].  A draw that changes a facet choice would
    measure the discontinuity, not the sensitivity: it is asserted not to happen."""
    jm = je.model_dict(abi.make_joint_model(params)) if joints else None
    out = []
    for i, sc in enumerate(scenarios(q_stand, qv_fn, foot_fn)):
        rng = np.random.default_rng(7)
        mk = lambda fn: FieldPlant(fn, foot_fn, sc["q0"][None], sc["v0"][None], [sc], jm)  # noqa: E731
        base, worst = mk(qv_fn), np.zeros(4)
        for tick in range(TICKS):
            q, v, p, jp = base.q.copy(), base.v.copy(), base.p.copy(), base.jp.copy()
            base.step(sc["tau"][None])
            assert base.margin >= MARGIN, (i, tick, base.margin)
            for _ in range(draws):
                pert = lambda x: x * (1.0 + rel * rng.uniform(-1.0, 1.0, np.shape(x)))  # noqa: E731
                tw = mk(lambda qq, vv: tuple(pert(np.asarray(x)) for x in qv_fn(qq, vv)[:3]))
                tw.q, tw.v, tw.p, tw.jp = pert(q), pert(v), pert(p), pert(jp)
                tw.step(sc["tau"][None])
                assert np.array_equal(tw.facet, base.facet)
                worst = np.maximum(worst, [np.abs(tw.v - base.v).max(), np.abs(tw.lam - base.lam).max() / max(1.0, np.abs(base.lam).max()),
                                           np.abs(tw.friction_torque - base.friction_torque).max(),
                                           np.abs(tw.limit_torque - base.limit_torque).max()])
        out.append(tuple(worst))
    return out


def twin_figures(q_stand, qv_fn, foot_fn):
    """The twin's own run of the six scenarios: margin, the cone figure, the facets at the first and the last tick, touching by tick."""
    scen = scenarios(q_stand, qv_fn, foot_fn)
    tw = FieldPlant(qv_fn, foot_fn, np.array([c["q0"] for c in scen]), np.array([c["v0"] for c in scen]), scen)
    tau = np.array([c["tau"] for c in scen])
    margin, cone, facets, touch = np.inf, -np.inf, [], []
    for tick in range(TICKS):
        tw.step(tau)
        r = tw.record()
        margin = min(margin, tw.margin)
        for i in range(B):
            cone = max(cone, pe.cone_figures(r["lam"][i], r["touching"][i], r["last_planes"][i], scen[i]["mu"])[1])
        facets.append(r["facet"].copy())
        touch.append(r["touching"].copy())
    return dict(margin=margin, cone=cone, facets=np.array(facets), touching=np.array(touch))


if __name__ == "__main__":
    from hunter_bipedal_control_amd import ingest   # (run with the repository root and tests/ on PYTHONPATH)
    prm = ingest.load_packaged()
    qv, foot, qs = ce.oracle_fns(prm)
    f = twin_figures(qs, qv, foot)
    print("margin", f["margin"], "cone", f["cone"])
    print("facets at the first / last tick:\n", f["facets"][0], "\n", f["facets"][-1])
    print("touching at the last tick:\n", f["touching"][-1])
    for joints in (False, True):
        for i, w in enumerate(measure_sensitivity(prm, qs, qv, foot, joints)):
            print(f"joint model {joints} scenario {i}: |dv| {w[0]:.2e}  |dlambda| rel {w[1]:.2e}  |d friction| {w[2]:.2e}  |d limit| {w[3]:.2e}")
