"""Helpers of the episode-record tests (tests/test_episode_host.py, tests/test_gpu_episode.py):

  * build() of tests/host_emu/libepisodeemu.so — csrc/hb_episode.hpp compiled for the host behind a tiny C API (episodeemu.cpp), under the
    file lock of tests/_hostemu.py, installed atomically, rebuilt when a source it includes is newer; host_record() runs it over a stream;
  * an independent numpy twin of the record as include/hunter_hip.h defines it (twin_record): it takes the per-tick outputs of a run STACKED
    over the ticks and reduces them with np.max / np.min / np.sum / np.bitwise_or over the ticks before the end.  It has no per-tick loop
    and shares no route with the header;
  * the comparison rules (compare) and the check that no threshold test sits on the fence (assert_off_the_fence).

A stream is a dict of arrays stacked over T ticks, the outputs of the getters after every plant step: q[T][16], v[T][16], tau_last[T][10]
(what hb_plant_sense reports as joint_torque); wbc_status[T] or None (no WBC call has run); the contact group gap[T][4], lam[T][12],
point_vel[T][12], residual[T], touching[T][4], status[T], all None outside contact model 1; the joint group jresidual[T], jstatus[T], None
without a joint model.

Comparison rules.  Every count, latch, OR, copy, minimum and maximum of a stored value: ==.  height and the tangential speed over a tilted
plane (three products and their sums, which a compiler may contract into fused multiply-adds): 8 roundings of the largest term; on the
level plane (n = e_z) == as well.  The two work sums: |a - b| <= (TICKS + 21) 2^-53 WORK_ABS: 21 roundings for a term of ten products, ten
additions and the multiplication by dt, one rounding per accumulation.
"""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import _contactemu as ce
from hunter_bipedal_control_amd import abi

HERE, CSRC = ce.HERE, ce.CSRC
_p = ce._p
U = 2.0 ** -53
CONTACT_KEYS = ("gap", "lam", "point_vel", "residual", "touching", "status")
JOINT_KEYS = ("jresidual", "jstatus")
EXACT_DOUBLES = ("START_POS", "LAST_BASE", "TILT_MAX", "TAU_MAX", "GAP_MIN", "FN_MAX", "RES_MAX", "JRES_MAX")
HEIGHTS = ("HEIGHT_LAST", "HEIGHT_MIN", "HEIGHT_MAX")


def build():
    so = HERE / "libepisodeemu.so"
    deps = [HERE / "episodeemu.cpp", CSRC.parents[1] / "include" / "hunter_hip.h", *CSRC.glob("*.hpp")]
    with open(HERE / ".hostemu.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            tmp = HERE / f"libepisodeemu.{os.getpid()}.so"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", str(tmp), str(HERE / "episodeemu.cpp")])
            os.replace(tmp, so)
    return so


def stack(ticks):
    """A list of per-tick dicts (one instance) -> a stream; a key that is None on the first tick stays None."""
    return {k: (None if ticks[0][k] is None else np.array([t[k] for t in ticks])) for k in ticks[0]}


def instance(stream, i):
    """Instance i of a stream whose arrays are [T][B][...]."""
    return {k: (None if a is None else np.ascontiguousarray(a[:, i])) for k, a in stream.items()}


# ---- the host build ---------------------------------------------------------------------------------------------------------------------
def host_record(lib, cfg, plane, q_start, st, dt):
    """ee_init at q_start, then ee_update over the ticks of the stream -> (record dict of one instance, trace[capacity][8], latch)."""
    plane = np.ascontiguousarray(plane, dtype=float)
    irec, drec = np.zeros((1, abi.HB_EP_NI), dtype=np.int32), np.zeros((1, abi.HB_EP_ND))
    trace = np.zeros((max(int(cfg.trace_capacity), 1), abi.HB_EP_TRACE_W))
    estop = np.zeros(1, dtype=np.int32)
    lib.ee_init(_p(np.ascontiguousarray(q_start, dtype=float)), _p(plane), _p(irec), _p(drec))
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=float)          # noqa: E731
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)       # noqa: E731
    for t in range(len(st["q"])):
        row = {k: (None if a is None else a[t]) for k, a in st.items()}
        args = [f64(row["q"]), f64(row["v"]), f64(row["tau_last"]), plane, i32(row["wbc_status"]), f64(row["gap"]), f64(row["lam"]),
                f64(row["point_vel"]), f64(row["residual"]), i32(row["touching"]), i32(row["status"]), f64(row["jresidual"]), i32(row["jstatus"])]
        lib.ee_update(C.byref(cfg), *[_p(a) for a in args], C.c_double(dt), _p(irec), _p(drec), _p(trace), _p(estop))
    rec = {k: a[0] for k, a in abi.split_episode_record(irec, drec).items()}
    return rec, trace[:int(cfg.trace_capacity)], int(estop[0])


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------
def _dot3(n, x):
    """n . x over the last axis, summed in the order x, y, z, every product and sum rounded on its own."""
    return (n[0] * x[..., 0] + n[1] * x[..., 1]) + n[2] * x[..., 2]


def tangential_speed(n, pv):
    """|pv - (n . pv) n| of point velocities pv[..., 3]."""
    t = pv - _dot3(n, pv)[..., None] * n
    return np.sqrt((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2])


def twin_record(cfg, plane, q_start, st, dt, wrong=None):
    """The record and the trace of one instance from its stacked stream.  wrong: None, or one of the three wrong twins of the self-test —
    "slip_untouched" counts slipping on points that do not touch, "fall_tick" accumulates the tick of the fall, "no_freeze" goes on
    accumulating every later tick that is not itself an end."""
    n, d = np.asarray(plane[:3], dtype=float), float(plane[3])
    q, v, tau = st["q"], st["v"], st["tau_last"]
    T = len(q)
    ground, joints = st["status"] is not None, st["jstatus"] is not None
    finite = np.isfinite(q).all(axis=1) & np.isfinite(v).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        height = _dot3(n, q[:, 0:3]) - d
        tilt = np.maximum(np.abs(q[:, 4]), np.abs(q[:, 5]))
        fallen = (cfg.tilt_limit > 0.0) & (tilt > cfg.tilt_limit)
    if ground:
        fallen = fallen | ((st["status"] & abi.HB_CONTACT_FALLEN) != 0)
    ended = ~finite | fallen
    end = int(np.argmax(ended)) if ended.any() else -1
    up = np.ones(T, dtype=bool) if end < 0 else np.arange(T) < end
    if wrong == "fall_tick" and end >= 0 and finite[end]:
        up = np.arange(T) <= end
    if wrong == "no_freeze":
        up = ~ended
    k = np.flatnonzero(up)
    height0 = float(_dot3(n, np.asarray(q_start, dtype=float)[0:3]) - d)
    r = dict(STEPS=T, TICKS=len(k), END_TICK=end, END_CAUSE=abi.HB_EP_RUNNING if end < 0 else (abi.HB_EP_FALLEN if finite[end] else abi.HB_EP_NONFINITE),
             FIRST_NONFINITE=int(np.argmax(~finite)) if (~finite).any() else -1, START_POS=np.array(q_start[0:3], dtype=float),
             LAST_BASE=q[k[-1], 0:6] if len(k) else np.array(q_start[0:6], dtype=float), HEIGHT_LAST=height[k[-1]] if len(k) else height0,
             HEIGHT_MIN=height[k].min(initial=np.inf), HEIGHT_MAX=height[k].max(initial=-np.inf), TILT_MAX=tilt[k].max(initial=0.0),
             TAU_MAX=np.abs(tau[k]).max(axis=0, initial=0.0))
    power = tau[k] * v[k, 6:]
    r["WORK_ABS"], r["WORK_NET"] = np.sum(dt * np.abs(power).sum(axis=1)), np.sum(dt * power.sum(axis=1))
    wbc = st["wbc_status"]
    fails = np.flatnonzero(wbc[k] != 0) if wbc is not None else np.zeros(0, dtype=int)
    r.update(WBC_STATUS_OR=int(np.bitwise_or.reduce(wbc[k], initial=0)) if wbc is not None else 0, WBC_FAIL_TICKS=len(fails),
             FIRST_WBC_FAIL=int(k[fails[0]]) if len(fails) else -1)
    r.update(CONTACT_TICKS=np.zeros(4, dtype=int), TOUCHDOWNS=np.zeros(4, dtype=int), PREV_TOUCHING=np.zeros(4, dtype=int), SLIP_TICKS=0, FIRST_SLIP=-1,
             UNCONVERGED_TICKS=0, CONTACT_STATUS_OR=0, GAP_MIN=np.inf, FN_MAX=np.zeros(4), SLIP_SPEED_MAX=0.0, RES_MAX=0.0)
    n_touching = np.zeros(T)
    if ground:
        touch = st["touching"][k] != 0
        before = np.concatenate([np.zeros((1, 4), dtype=bool), touch[:-1]]) if len(k) else touch
        speed = tangential_speed(n, st["point_vel"][k].reshape(-1, 4, 3))
        counted = speed if wrong == "slip_untouched" else np.where(touch, speed, 0.0)
        slipping = np.flatnonzero((counted > cfg.slip_speed).any(axis=1))
        n_touching = (st["touching"] != 0).sum(axis=1)
        r.update(CONTACT_TICKS=touch.sum(axis=0), TOUCHDOWNS=(touch & ~before).sum(axis=0), PREV_TOUCHING=touch[-1].astype(int) if len(k) else np.zeros(4, dtype=int),
                 SLIP_TICKS=len(slipping), FIRST_SLIP=int(k[slipping[0]]) if len(slipping) else -1,
                 UNCONVERGED_TICKS=int(((st["status"][k] & abi.HB_CONTACT_UNCONVERGED) != 0).sum()),
                 CONTACT_STATUS_OR=int(np.bitwise_or.reduce(st["status"][k], initial=0)), GAP_MIN=st["gap"][k].min(initial=np.inf),
                 FN_MAX=_dot3(n, st["lam"][k].reshape(-1, 4, 3)).max(axis=0, initial=0.0), SLIP_SPEED_MAX=counted.max(initial=0.0),
                 RES_MAX=st["residual"][k].max(initial=0.0))
    r.update(JRES_MAX=0.0, JOINT_STATUS_OR=0, CLAMP_TICKS=0, STOP_TICKS=0)
    if joints:
        js = st["jstatus"][k]
        r.update(JRES_MAX=st["jresidual"][k].max(initial=0.0), JOINT_STATUS_OR=int(np.bitwise_or.reduce(js, initial=0)),
                 CLAMP_TICKS=int(((js & 0xffc00) != 0).sum()), STOP_TICKS=int(((js & 0x3ff) != 0).sum()))
    sampled = k[k % cfg.trace_every == 0][:cfg.trace_capacity] if cfg.trace_every > 0 else k[:0]
    trace = np.stack([sampled.astype(float), q[sampled, 0], q[sampled, 1], height[sampled], q[sampled, 3], q[sampled, 4], q[sampled, 5],
                      n_touching[sampled].astype(float)], axis=1)
    r["N_TRACE"] = len(sampled)
    return r, trace


def assert_off_the_fence(cfg, plane, st, rel=1e-9):
    """No tangential speed of a touching point within relative `rel` of slip_speed and no tilt within that distance of tilt_limit, on any
    finite tick of the stream: a rounding cannot decide a threshold test."""
    n = np.asarray(plane[:3], dtype=float)
    ok = np.isfinite(st["q"]).all(axis=1) & np.isfinite(st["v"]).all(axis=1)
    if cfg.tilt_limit > 0.0:
        tilt = np.maximum(np.abs(st["q"][ok, 4]), np.abs(st["q"][ok, 5]))
        assert (np.abs(tilt - cfg.tilt_limit) > rel * cfg.tilt_limit).all(), "a tilt sits on tilt_limit"
    if st["status"] is not None:
        speed = tangential_speed(n, st["point_vel"][ok].reshape(-1, 4, 3))[st["touching"][ok] != 0]
        assert (np.abs(speed - cfg.slip_speed) > rel * cfg.slip_speed).all(), "a tangential speed sits on slip_speed"


def compare(dev, dev_trace, tw, tw_trace, plane, st):
    """The record and trace of the code under test against the twin's, under the rules at the top of this file."""
    n, d = np.asarray(plane[:3], dtype=float), float(plane[3])
    level = np.array_equal(n, [0.0, 0.0, 1.0])
    for name, _, _ in abi.EPISODE_INT_FIELDS:
        assert np.array_equal(dev[name], tw[name]), (name, dev[name], tw[name])
    for name in EXACT_DOUBLES:
        assert np.array_equal(dev[name], tw[name]), (name, dev[name], tw[name])
    ok = np.isfinite(st["q"]).all(axis=1) & np.isfinite(st["v"]).all(axis=1)
    h_tol = 0.0 if level else 8 * U * max(np.abs(n * st["q"][ok, 0:3]).max(initial=0.0), abs(d))
    s_tol = 0.0 if level or st["status"] is None else 8 * U * np.abs(st["point_vel"][ok]).max(initial=0.0)
    for name in HEIGHTS:
        assert dev[name] == tw[name] or abs(dev[name] - tw[name]) <= h_tol, (name, dev[name], tw[name], h_tol)
    assert abs(dev["SLIP_SPEED_MAX"] - tw["SLIP_SPEED_MAX"]) <= s_tol, ("SLIP_SPEED_MAX", dev["SLIP_SPEED_MAX"], tw["SLIP_SPEED_MAX"], s_tol)
    w_tol = (tw["TICKS"] + 21) * U * tw["WORK_ABS"]
    for name in ("WORK_ABS", "WORK_NET"):
        assert abs(dev[name] - tw[name]) <= w_tol, (name, dev[name], tw[name], w_tol)
    m = tw["N_TRACE"]
    assert dev_trace.shape[0] >= m and not dev_trace[m:].any(), "samples behind N_TRACE are zero"
    if m:
        cols = [c for c in range(abi.HB_EP_TRACE_W) if c != 3]
        assert np.array_equal(dev_trace[:m][:, cols], tw_trace[:, cols]), "trace"
        assert (np.abs(dev_trace[:m, 3] - tw_trace[:, 3]) <= h_tol).all(), "trace height"
