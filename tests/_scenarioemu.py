"""Helpers of the scenario tests (tests/test_scenario_host.py, tests/test_gpu_scenario.py):

  * build() of tests/host_emu/libscenarioemu.so — csrc/hb_scenario.hpp compiled for the host behind a tiny C API (scenarioemu.cpp), under
    the file lock of tests/_hostemu.py, installed atomically, rebuilt when a source it includes is newer;
  * an independent twin of the procedure as include/hunter_hip.h defines it above hb_plant_set_scenario: the draw (Philox4x32-10 of
    tests/_sensemu.py, the counter layout and the word table of the header), the terrain record and the model composition the header
    defines above hb_plant_set_terrain / hb_plant_set_model_variation, the push and the log row.  Written from the header text in Python
    floats (IEEE doubles), one operation per rounding in the order written, so it is EXACT; it shares no route with the C++.
"""
import fcntl
import math
import os
import subprocess

import numpy as np

import _contactemu as ce
import _sensemu as se
from hunter_bipedal_control_amd import abi

HERE, CSRC = ce.HERE, ce.CSRC
_p = ce._p
NBLOCKS = 7


def build():
    so = HERE / "libscenarioemu.so"
    deps = [HERE / "scenarioemu.cpp", CSRC.parents[1] / "include" / "hunter_hip.h", *CSRC.glob("*.hpp")]
    with open(HERE / ".hostemu.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            tmp = HERE / f"libscenarioemu.{os.getpid()}.so"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", str(tmp), str(HERE / "scenarioemu.cpp")])
            os.replace(tmp, so)
    return so


# ---- the twin -----------------------------------------------------------------------------------------------------------------------------
def block_words(cfg, inst, episode, block):
    seed = int(cfg.seed)
    return se.philox4x32_10([inst & 0xFFFFFFFF, episode, abi.HB_SC_STREAM, block], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])


def uniform(word) -> float:
    return (float(word) + 0.5) * 2.0 ** -32


def block_channel(block) -> int:
    return (abi.HB_SC_SLOPE, abi.HB_SC_MU, abi.HB_SC_PAYLOAD, abi.HB_SC_MASS, abi.HB_SC_MASS, abi.HB_SC_MASS, abi.HB_SC_PUSH)[block]


def terrain_record(plane):
    """What hb_plant_set_terrain stores for plane = (n, d): (T[9] row-major = [t1 t2 n] in columns, d), n normalised first."""
    a, b, c, d = (float(x) for x in plane)
    ln = math.sqrt(a * a + b * b + c * c)
    n = [a / ln, b / ln, c / ln]
    t1 = [1.0 - n[0] * n[0], -(n[0] * n[1]), -(n[0] * n[2])]
    l1 = math.sqrt(t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2])
    t1 = [x / l1 for x in t1]
    t2 = [n[1] * t1[2] - n[2] * t1[1], n[2] * t1[0] - n[0] * t1[2], n[0] * t1[1] - n[1] * t1[0]]
    T = np.zeros(9)
    for k in range(3):
        T[3 * k], T[3 * k + 1], T[3 * k + 2] = t1[k], t2[k], n[k]
    return T, d


def _shift(m, d):
    dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return [m * (dd - d[0] * d[0]), m * (0.0 - d[0] * d[1]), m * (0.0 - d[0] * d[2]), m * (dd - d[1] * d[1]), m * (0.0 - d[1] * d[2]),
            m * (dd - d[2] * d[2])]


def model_compose(nominal, scale=None, payload=None):
    """The composition above hb_plant_set_model_variation.  nominal / result: dict(mass[11], com[11][3], inertia[11][6], total_mass)."""
    mass, com, inertia = (np.array(nominal[k], dtype=float) for k in ("mass", "com", "inertia"))
    s = [1.0] * abi.NBODY if scale is None else [float(x) for x in scale]
    pl = [0.0] * abi.HB_PAYLOAD_SIZE if payload is None else [float(x) for x in payload]
    if pl[0] == 0.0 and all(x == 1.0 for x in s):
        return dict(mass=mass, com=com, inertia=inertia, total_mass=float(nominal["total_mass"]))
    for b in range(1, abi.NBODY):
        mass[b] = s[b] * float(nominal["mass"][b])
        for k in range(6):
            inertia[b, k] = s[b] * float(nominal["inertia"][b][k])
    c0, I0 = [float(x) for x in nominal["com"][0]], [float(x) for x in nominal["inertia"][0]]
    mp, r, Ip = pl[0], pl[1:4], pl[4:10]
    ms = s[0] * float(nominal["mass"][0])
    m0 = ms + mp
    cn = [(ms * c0[a] + mp * r[a]) / m0 for a in range(3)]
    P1, P2 = _shift(ms, [c0[a] - cn[a] for a in range(3)]), _shift(mp, [r[a] - cn[a] for a in range(3)])
    mass[0], com[0] = m0, cn
    for k in range(6):
        inertia[0, k] = ((s[0] * I0[k] + P1[k]) + Ip[k]) + P2[k]
    total = 0.0
    for b in range(abi.NBODY):
        total += float(mass[b])
    return dict(mass=mass, com=com, inertia=inertia, total_mass=total)


def init_row():
    """scen before the first draw and the push record "none"."""
    scen = np.zeros(abi.HB_SC_N)
    scen[21] = -1.0
    return scen, np.array([-1.0, 0.0, 0.0])


def draw(cfg, inst, episode, spawn_xy, ground_z, nominal, ter, model):
    """The draw of episode `episode` of global instance `inst` -> dict(scen[HB_SC_N], ter[14] = T | d | mu, model = dict as model_compose's,
    push[3], plane = the (n0, d) the slope channel hands to the terrain record, or None, scale / payload = what the model channels hand to
    the composition, or None).  ter / model: the records in place; a channel that is off leaves its part."""
    ch = int(cfg.channels)
    u = {b: [uniform(w) for w in block_words(cfg, inst, episode, b)] for b in range(NBLOCKS) if ch & block_channel(b)}
    scen, ter = np.zeros(abi.HB_SC_N), np.array(ter, dtype=float)
    out = dict(plane=None, scale=None, payload=None)
    if ch & abi.HB_SC_SLOPE:
        gx, gy = cfg.grade_max * (2.0 * u[0][0] - 1.0), cfg.grade_max * (2.0 * u[0][1] - 1.0)
        ln = math.sqrt((gx * gx + gy * gy) + 1.0)
        n0 = [(-gx) / ln, (-gy) / ln, 1.0 / ln]
        d = (n0[0] * float(spawn_xy[0]) + n0[1] * float(spawn_xy[1])) + n0[2] * float(ground_z)
        ter[0:9], ter[9] = terrain_record(n0 + [d])
        scen[0:2] = gx, gy
        out["plane"] = np.array(n0 + [d])
    if ch & abi.HB_SC_MU:
        for c in range(4):
            ter[10 + c] = scen[2 + c] = cfg.mu_lo + (cfg.mu_hi - cfg.mu_lo) * u[1][c if cfg.mu_per_point else 0]
    if ch & (abi.HB_SC_PAYLOAD | abi.HB_SC_MASS):
        if ch & abi.HB_SC_PAYLOAD:
            pl = np.zeros(abi.HB_PAYLOAD_SIZE)
            pl[0] = cfg.payload_mass_max * u[2][0]
            for a in range(3):
                pl[1 + a] = cfg.payload_center[a] + cfg.payload_half_extent[a] * (2.0 * u[2][1 + a] - 1.0)
            scen[6:10] = pl[0:4]
            out["payload"] = pl
        if ch & abi.HB_SC_MASS:
            out["scale"] = np.array([1.0 + cfg.mass_scale_range * (2.0 * u[3 + b // 4][b % 4] - 1.0) for b in range(abi.NBODY)])
            scen[10:21] = out["scale"]
        model = model_compose(nominal, out["scale"], out["payload"])
    push = np.array([-1.0, 0.0, 0.0])
    if ch & abi.HB_SC_PUSH:
        start = cfg.push_start_lo + int(u[6][0] * float(cfg.push_start_hi - cfg.push_start_lo + 1))
        push = np.array([float(start), cfg.push_force_max * (2.0 * u[6][1] - 1.0), cfg.push_force_max * (2.0 * u[6][2] - 1.0)])
        scen[21:24] = push
    out.update(scen=scen, ter=ter, model=model, push=push)
    return out


def push_wrench(cfg, push, steps):
    on = push[0] >= 0 and push[0] <= steps < push[0] + cfg.push_ticks
    return np.array([push[1], push[2], 0.0, 0.0, 0.0, 0.0]) if on else np.zeros(6)


def log_row(episode_index, cause, rec, scen):
    """The row of a finished episode from its record (a dict of abi.split_episode_record of ONE instance) and the scen it ran under."""
    return np.concatenate([[float(episode_index), float(cause), float(rec["TICKS"]), rec["LAST_BASE"][0] - rec["START_POS"][0],
                            rec["LAST_BASE"][1] - rec["START_POS"][1], rec["TILT_MAX"]], scen])
