"""Host emulator of the controller's field map (tests/host_emu/groundfieldemu.cpp: hb_ground.hpp's field part and the planner, IK,
node-table and filter routines in their field forms, compiled with g++) for tests/test_groundfield_host.py and the GPU test's host side:
build() under the file lock of tests/_hostemu.py, installed atomically, rebuilt when a source is newer; thin ctypes wrappers."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import _hostemu
from _groundemu import MAX_EVENTS, RG_MAX_KNOTS, RG_PHASE

HERE, CSRC = _hostemu.HERE, _hostemu.CSRC

_lib = None


def build():
    so = HERE / "libgroundfieldemu.so"
    deps = [HERE / "groundfieldemu.cpp", CSRC.parents[1] / "include" / "hunter_hip.h", *CSRC.glob("*.hpp")]
    with open(HERE / ".hostemu.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            tmp = HERE / f"libgroundfieldemu.{os.getpid()}.so"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", str(tmp), str(HERE / "groundfieldemu.cpp")])
            os.replace(tmp, so)
    return so


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(str(build()))
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def record(direction, origin, spacing, heights, n=None, into=None):
    """The stored map (header[8], heights [32][32] with zero beyond the grid) of one instance, what hb_ground_set_field stores -> (hdr, z),
    or raises ValueError with the refusal.  n overrides the node counts; into: the header array the routine writes (left as it is by a
    refusal)."""
    N = lib().gfe_max_nodes()
    h = np.asarray(heights, dtype=np.float64)
    z = np.zeros((N, N))
    z[:min(N, h.shape[0]), :min(N, h.shape[1])] = 0.0 + h[:N, :N]
    nn = np.array(h.shape if n is None else n, dtype=np.int32)
    hdr = np.zeros(lib().gfe_header_size()) if into is None else into
    why = C.create_string_buffer(128)
    f64 = lambda v: np.ascontiguousarray(v, dtype=np.float64)  # noqa: E731
    if lib().gfe_record(_p(nn), _p(f64(direction)), _p(f64(origin)), _p(f64(spacing)), _p(z), _p(hdr), why) != 0:
        raise ValueError(why.value.decode())
    return hdr, z


def record_of(m):
    """record() of a twin FieldMap"""
    return record(m.dir_given, m.origin, m.spacing, m.g)


def height(rec, xy):
    p = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    h, facet = np.zeros(len(p)), np.zeros(len(p), dtype=np.int32)
    lib().gfe_height(_p(rec[0]), _p(rec[1]), C.c_int(len(p)), _p(p), _p(h), _p(facet))
    return h, facet


def ground_form(profile_on, field_on=None):
    """use_ground_forms of hb_forms.hpp -> 0 none, 1 profile, 2 field; field_on None: the one-argument call"""
    if field_on is None:
        return lib().gfe_ground_form_profile_only(C.c_int(int(profile_on)))
    return lib().gfe_ground_form(C.c_int(int(profile_on)), C.c_int(int(field_on)))


def refgen(mdl, rcfg, rec, sched, t0, horizon, x_now, cmd_vel, latest_stance, nmax):
    """One pass of one instance (rec None: the base forms); latest_stance [4][3] is updated in place.  -> (status, dict of EVERY output), as
    _groundemu.refgen."""
    ev = np.ascontiguousarray(sched.event_times, dtype=np.float64)
    modes = np.ascontiguousarray(sched.modes, dtype=np.int32)
    n, nk = C.c_int(), C.c_int()
    t, mode = np.zeros(nmax + 1), np.zeros(nmax, dtype=np.int32)
    xref, swing = np.zeros((nmax, 22)), np.zeros((nmax, 4, 6))
    phases = np.zeros((4, MAX_EVENTS + 1, RG_PHASE))
    knot_t, knot_x = np.zeros(RG_MAX_KNOTS), np.zeros((RG_MAX_KNOTS, 22))
    hdr, z = (None, None) if rec is None else rec
    st = lib().gfe_refgen(C.byref(mdl), C.byref(rcfg), _p(hdr), _p(z), C.c_int(len(ev)), _p(ev) if len(ev) else None, _p(modes), C.c_double(t0),
                          C.c_double(horizon), _p(np.ascontiguousarray(x_now, dtype=np.float64)), _p(np.ascontiguousarray(cmd_vel, dtype=np.float64)),
                          _p(latest_stance), C.c_int(nmax), C.byref(n), _p(t), _p(mode), _p(xref), _p(swing), _p(phases), C.byref(nk), _p(knot_t),
                          _p(knot_x))
    return st, dict(n_nodes=n.value, t=t, mode=mode, x_ref=xref, swing=swing, phases=phases, n_knots=nk.value, knot_t=knot_t, knot_x=knot_x,
                    stance=latest_stance.copy())


def kf_update(mdl, ecfg, rec, dt, xhat, P, yaw, quat, w_local, a_local, qj, qdj, contact):
    """One filter tick (rec None: the base form); xhat[18], P[18][18], yaw[1] are updated in place.  -> (rbd[32], x[22])"""
    rbd, x = np.zeros(32), np.zeros(22)
    hdr, z = (None, None) if rec is None else rec
    lib().gfe_kf_update(C.byref(mdl), C.byref(ecfg), _p(hdr), _p(z), C.c_double(dt), _p(xhat), _p(P), _p(yaw), _p(np.ascontiguousarray(quat)),
                        _p(np.ascontiguousarray(w_local)), _p(np.ascontiguousarray(a_local)), _p(np.ascontiguousarray(qj)),
                        _p(np.ascontiguousarray(qdj)), _p(np.ascontiguousarray(contact, dtype=np.int32)), _p(rbd), _p(x))
    return rbd, x
