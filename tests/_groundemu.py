"""Host emulator of the controller's ground map (tests/host_emu/groundemu.cpp: hb_ground.hpp and the planner, IK, node-table and filter
routines that read it, compiled with g++) for tests/test_groundmap_host.py: build() under the file lock of tests/_hostemu.py, installed
atomically, rebuilt when a source is newer; thin ctypes wrappers."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import _hostemu
from hunter_bipedal_control_amd import abi

HERE, CSRC = _hostemu.HERE, _hostemu.CSRC
KMAX = abi.HB_PROFILE_MAX_KNOTS
MAX_EVENTS, RG_PHASE, RG_MAX_KNOTS = 64, 8, 24

_lib = None


def build():
    so = HERE / "libgroundemu.so"
    deps = [HERE / "groundemu.cpp", CSRC.parents[1] / "include" / "hunter_hip.h", *CSRC.glob("*.hpp")]
    with open(HERE / ".hostemu.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            tmp = HERE / f"libgroundemu.{os.getpid()}.so"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", str(tmp), str(HERE / "groundemu.cpp")])
            os.replace(tmp, so)
    return so


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(str(build()))
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def record(direction, knots):
    """The stored record of a map (what hb_ground_set_profile stores) -> array, or raises ValueError with the refusal."""
    k = np.ascontiguousarray(knots, dtype=np.float64).reshape(-1, 2)
    d = np.ascontiguousarray(direction, dtype=np.float64)
    rec = np.zeros(lib().ge_record_size())
    why = C.create_string_buffer(128)
    if lib().ge_record(C.c_int(len(k)), _p(d), _p(k), _p(rec), why) != 0:
        raise ValueError(why.value.decode())
    return rec


def slopes(rec):
    at = lib().ge_slopes_at()
    return rec[at:at + KMAX - 1]


def height(rec, xy):
    p = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    h, seg = np.zeros(len(p)), np.zeros(len(p), dtype=np.int32)
    lib().ge_height(_p(rec), C.c_int(len(p)), _p(p), _p(h), _p(seg))
    return h, seg


def refgen(mdl, rcfg, rec, sched, t0, horizon, x_now, cmd_vel, latest_stance, nmax):
    """One pass of one instance (rec None: the base forms); latest_stance [4][3] is updated in place.  -> (status, dict of EVERY output:
    the node tables, the phase records, the knots and the stance memory)."""
    ev = np.ascontiguousarray(sched.event_times, dtype=np.float64)
    modes = np.ascontiguousarray(sched.modes, dtype=np.int32)
    n, nk = C.c_int(), C.c_int()
    t, mode = np.zeros(nmax + 1), np.zeros(nmax, dtype=np.int32)
    xref, swing = np.zeros((nmax, 22)), np.zeros((nmax, 4, 6))
    phases = np.zeros((4, MAX_EVENTS + 1, RG_PHASE))
    knot_t, knot_x = np.zeros(RG_MAX_KNOTS), np.zeros((RG_MAX_KNOTS, 22))
    st = lib().ge_refgen(C.byref(mdl), C.byref(rcfg), _p(rec), C.c_int(len(ev)), _p(ev) if len(ev) else None, _p(modes), C.c_double(t0),
                         C.c_double(horizon), _p(np.ascontiguousarray(x_now, dtype=np.float64)), _p(np.ascontiguousarray(cmd_vel, dtype=np.float64)),
                         _p(latest_stance), C.c_int(nmax), C.byref(n), _p(t), _p(mode), _p(xref), _p(swing), _p(phases), C.byref(nk), _p(knot_t),
                         _p(knot_x))
    return st, dict(n_nodes=n.value, t=t, mode=mode, x_ref=xref, swing=swing, phases=phases, n_knots=nk.value, knot_t=knot_t, knot_x=knot_x,
                    stance=latest_stance.copy())


def kf_update(mdl, ecfg, rec, dt, xhat, P, yaw, quat, w_local, a_local, qj, qdj, contact):
    """One filter tick (rec None: the base form); xhat[18], P[18][18], yaw[1] are updated in place.  -> (rbd[32], x[22])"""
    rbd, x = np.zeros(32), np.zeros(22)
    lib().ge_kf_update(C.byref(mdl), C.byref(ecfg), _p(rec), C.c_double(dt), _p(xhat), _p(P), _p(yaw), _p(np.ascontiguousarray(quat)),
                       _p(np.ascontiguousarray(w_local)), _p(np.ascontiguousarray(a_local)), _p(np.ascontiguousarray(qj)),
                       _p(np.ascontiguousarray(qdj)), _p(np.ascontiguousarray(contact, dtype=np.int32)), _p(rbd), _p(x))
    return rbd, x
