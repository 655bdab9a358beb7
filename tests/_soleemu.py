"""Host emulator of the planner's sole mode (tests/host_emu/soleemu.cpp: refgen_plan<MAP, 1> of hb_refgen.hpp on both kinds of map, compiled
with g++) for tests/test_sole_host.py: build() under the file lock of tests/_hostemu.py, installed atomically, rebuilt when a source is
newer; thin ctypes wrappers.  Maps are given as tests/_groundemu.py record() (an array) or tests/_groundfieldemu.py record() (hdr, z)."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import _hostemu
from _groundemu import MAX_EVENTS, RG_MAX_KNOTS, RG_PHASE
from hunter_bipedal_control_amd import abi

HERE, CSRC = _hostemu.HERE, _hostemu.CSRC

_lib = None


def build():
    so = HERE / "libsoleemu.so"
    deps = [HERE / "soleemu.cpp", CSRC.parents[1] / "include" / "hunter_hip.h", *CSRC.glob("*.hpp")]
    with open(HERE / ".hostemu.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            tmp = HERE / f"libsoleemu.{os.getpid()}.so"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", str(tmp), str(HERE / "soleemu.cpp")])
            os.replace(tmp, so)
    return so


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(str(build()))
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _map(rec):
    return (rec, None) if isinstance(rec, np.ndarray) else rec


def no_foothold():
    return lib().se_no_foothold()


def sole_form(profile_on, field_on, mode=None):
    """use_sole_forms of hb_forms.hpp on use_ground_forms(profile_on, field_on); mode None: the defaulted call"""
    return lib().se_sole_form(C.c_int(int(profile_on)), C.c_int(int(field_on)), C.c_int(-1 if mode is None else int(mode)))


def refused(fcfg):
    """the argument check hb_ground_set_foothold applies to a configuration with mode != 0"""
    return bool(lib().se_refused(C.byref(fcfg)))


def sample(rec, t_xy, h_xy):
    """S(cT, cH) -> (delta, top)"""
    gnd, gz = _map(rec)
    out = np.zeros(2)
    lib().se_sample(_p(gnd), _p(gz), _p(np.ascontiguousarray(t_xy, dtype=np.float64)), _p(np.ascontiguousarray(h_xy, dtype=np.float64)), _p(out))
    return out[0], out[1]


def refgen(mdl, rcfg, rec, fcfg, sched, t0, horizon, x_now, cmd_vel, latest_stance, nmax):
    """One pass of one instance on the map rec; fcfg: an abi.FootholdConfig or None (the per-point forms).  latest_stance [4][3] is updated
    in place.  -> (status, dict of EVERY output of _groundemu.refgen plus the choice read-back shift[2], defect[2], level[2])."""
    gnd, gz = _map(rec)
    ev = np.ascontiguousarray(sched.event_times, dtype=np.float64)
    modes = np.ascontiguousarray(sched.modes, dtype=np.int32)
    n, nk = C.c_int(), C.c_int()
    t, mode = np.zeros(nmax + 1), np.zeros(nmax, dtype=np.int32)
    xref, swing = np.zeros((nmax, 22)), np.zeros((nmax, 4, 6))
    phases = np.zeros((4, MAX_EVENTS + 1, RG_PHASE))
    knot_t, knot_x = np.zeros(RG_MAX_KNOTS), np.zeros((RG_MAX_KNOTS, 22))
    shift, defect, level = np.full(2, -7, dtype=np.int32), np.full(2, -7.0), np.full(2, -7, dtype=np.int32)
    st = lib().se_refgen(C.byref(mdl), C.byref(rcfg), _p(gnd), _p(gz), None if fcfg is None else C.byref(fcfg), C.c_int(len(ev)),
                         _p(ev) if len(ev) else None, _p(modes), C.c_double(t0), C.c_double(horizon),
                         _p(np.ascontiguousarray(x_now, dtype=np.float64)), _p(np.ascontiguousarray(cmd_vel, dtype=np.float64)), _p(latest_stance),
                         C.c_int(nmax), C.byref(n), _p(t), _p(mode), _p(xref), _p(swing), _p(phases), C.byref(nk), _p(knot_t), _p(knot_x),
                         _p(shift), _p(defect), _p(level))
    return st, dict(n_nodes=n.value, t=t, mode=mode, x_ref=xref, swing=swing, phases=phases, n_knots=nk.value, knot_t=knot_t, knot_x=knot_x,
                    stance=latest_stance.copy(), shift=shift, defect=defect, level=level)


def foothold_config(mode=1, n_shift=3, shift_step=0.02, flat_tol=0.005):
    return abi.make_foothold_config(mode=mode, n_shift=n_shift, shift_step=shift_step, flat_tol=flat_tol)
