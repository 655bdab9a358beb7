"""ctypes binding of libhunter_hip.so (the C-ABI in include/hunter_hip.h).

This is the host-side mirror of the reference's solver surface for the hot path:
``MPC_MRT_Interface::{advanceMpc, updatePolicy, evaluatePolicy}`` and ``WbcBase::update``
(legged_controllers/src/LeggedController.cpp:144-185).  There is no CPU fallback: importing works anywhere
(so the ABI can be inspected), but creating a solver without the HIP library or without a GPU raises.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import abi

_LIB_PATH = Path(__file__).resolve().parent / "libhunter_hip.so"
_lib = None

# every symbol include/hunter_hip.h declares
ABI_SYMBOLS = [
    "hb_create", "hb_destroy", "hb_last_error", "hb_mpc_set_references", "hb_mpc_reset", "hb_mpc_set_trajectory",
    "hb_mpc_solve", "hb_mpc_publish", "hb_mpc_get_solution", "hb_mpc_get_performance", "hb_mpc_get_step",
    "hb_wbc_update", "hb_wbc_update_direct", "hb_set_resident_inputs", "hb_step_resident", "hb_set_resident_x0_sequence",
    "hb_get_wbc_solution", "hb_set_chunks",
    "hb_sync", "hb_get_stats", "hb_get_input_cost", "hb_version", "hb_eval_flow_map", "hb_eval_foot_kinematics",
    "hb_eval_rbd", "hb_riccati_solve", "hb_riccati_gains", "hb_estimator_reset", "hb_estimator_update", "hb_estimator_get_filter", "hb_estimator_contact_force",
    "hb_refgen_reset", "hb_refgen_set_schedule", "hb_refgen_update", "hb_mpc_get_references", "hb_joint_command", "hb_centroidal_state_from_rbd", "hb_plant_reset", "hb_plant_step",
    "hb_plant_get_state", "hb_hoqp_solve", "hb_mpc_reset_masked", "hb_mpc_get_status", "hb_joint_set_flags",
    "hb_joint_get_emergency_stop", "hb_set_resident_time", "hb_get_wbc_iterations", "hb_ik_solve", "hb_debug_chunk_counters", "hb_debug_graph_state", "hb_refgen_get_status", "hb_tick_resident",
    "hb_wbc_set_certificate", "hb_wbc_get_certificate", "hb_hwbc_set_certificate", "hb_hwbc_get_certificate",
    "hb_mpc_get_certificate", "hb_mpc_get_lq", "hb_mpc_get_recovery", "hb_mpc_get_linesearch", "hb_mpc_get_linesearch_refused",
    "hb_refgen_get_schedule", "hb_gait_reset", "hb_gait_disable", "hb_gait_insert_template", "hb_gait_get_state",
    "hb_plant_set_sensor_model", "hb_plant_sense", "hb_estimator_update_resident", "hb_estimator_contact_force_resident",
    "hb_plant_set_contact_model", "hb_plant_set_external_wrench", "hb_plant_get_contact",
    "hb_plant_set_joint_model", "hb_plant_get_joints", "hb_plant_step_hybrid", "hb_plant_get_actuator",
    "hb_plant_set_terrain", "hb_plant_get_terrain",
    "hb_plant_set_terrain_profile", "hb_plant_get_terrain_profile",
    "hb_plant_set_terrain_field", "hb_plant_get_terrain_field", "hb_plant_field_eval",
    "hb_plant_set_model_variation", "hb_plant_get_model_variation",
    "hb_plant_set_episode", "hb_plant_get_episode",
    "hb_plant_set_respawn", "hb_plant_respawn", "hb_plant_get_respawn",
    "hb_plant_set_scenario", "hb_plant_get_scenario", "hb_plant_get_scenario_log",
    "hb_plant_set_profile_draw", "hb_plant_get_profile_draw", "hb_plant_get_profile_draw_log",
    "hb_plant_set_field_draw", "hb_plant_get_field_draw", "hb_plant_get_field_draw_log",
    "hb_plant_set_height_scan", "hb_plant_scan", "hb_plant_get_height_scan",
    "hb_ground_set_profile", "hb_ground_get_profile", "hb_ground_set_field", "hb_ground_get_field", "hb_ground_eval",
    "hb_ground_set_foothold", "hb_ground_get_foothold", "hb_ground_get_foothold_choice",
]
# include/hunter_lcm.h
LCM_SYMBOLS = ["hb_lcm_fingerprint", "hb_lcm_encoded_size", "hb_lcm_field_count", "hb_lcm_encode", "hb_lcm_decode", "hb_lcm_frame", "hb_lcm_unframe",
               "hb_joint_command_lcm", "hb_estimator_update_lcm", "hb_plant_step_lcm", "hb_plant_sense_lcm"]


LCM_LOW_CMD, LCM_LOW_STATE, LCM_FULL_STATE = 0, 1, 2


def lcm_encode(msg_type: int, timestamp, fields) -> np.ndarray:
    """Host codec of include/hunter_lcm.h: fields[n][60|40|56] -> wire images [n][496|336|464] (uint8)."""
    lib = load_library()
    nf, sz = lib.hb_lcm_field_count(msg_type), lib.hb_lcm_encoded_size(msg_type)
    f = np.ascontiguousarray(fields, dtype=np.float64).reshape(-1, nf)
    ts = np.ascontiguousarray(np.broadcast_to(np.asarray(timestamp, dtype=np.int64), (f.shape[0],)))
    out = np.zeros((f.shape[0], sz), dtype=np.uint8)
    rc = lib.hb_lcm_encode(C.c_int32(msg_type), C.c_int32(f.shape[0]), _p(ts), _p(f), _p(out))
    if rc != 0:
        raise ValueError(f"hb_lcm_encode failed ({rc})")
    return out


def lcm_decode(msg_type: int, wire):
    """-> (timestamp[n], fields[n][60|40|56]); raises if a message carries a foreign fingerprint."""
    lib = load_library()
    nf, sz = lib.hb_lcm_field_count(msg_type), lib.hb_lcm_encoded_size(msg_type)
    w = np.ascontiguousarray(wire, dtype=np.uint8).reshape(-1, sz)
    ts, f = np.zeros(w.shape[0], dtype=np.int64), np.zeros((w.shape[0], nf))
    rc = lib.hb_lcm_decode(C.c_int32(msg_type), C.c_int32(w.shape[0]), _p(w), _p(ts), _p(f))
    if rc != 0:
        raise ValueError(f"hb_lcm_decode failed ({rc}): fingerprint mismatch")
    return ts, f


class HunterHipError(RuntimeError):
    pass


def load_library() -> C.CDLL:
    """Load the in-tree HIP library; raises if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is None:
        if not _LIB_PATH.exists():
            raise HunterHipError(f"{_LIB_PATH} not found: build it with hunter_bipedal_control_amd/csrc/build.sh "
                                 "(the solver has no CPU fallback)")
        _lib = C.CDLL(str(_LIB_PATH))
        _lib.hb_last_error.restype = C.c_char_p
        _lib.hb_last_error.argtypes = [C.c_void_p]
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        assert a.shape == tuple(shape), (a.shape, shape)
    return a


def _i32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.int32)
    if shape is not None:
        assert a.shape == tuple(shape), (a.shape, shape)
    return a


class HunterSolver:
    """Batched NMPC + WBC solver bound to one GPU."""

    def __init__(self, params: dict, batch: int, max_nodes: int, device: int = 0, **cfg_overrides):
        self.lib = load_library()
        self.model = abi.make_model(params)
        self.config = abi.make_config(params, **cfg_overrides)
        self.B, self.N = int(batch), int(max_nodes)
        self.ctx = C.c_void_p()
        rc = self.lib.hb_create(C.byref(self.model), C.byref(self.config), C.c_int32(self.B), C.c_int32(self.N),
                                C.c_int32(device), C.byref(self.ctx))
        if rc != 0:
            raise HunterHipError(f"hb_create failed ({rc}): {self.lib.hb_last_error(None).decode()}")

    def close(self):
        if getattr(self, "ctx", None) is not None and self.ctx.value:
            self.lib.hb_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise HunterHipError(f"{what} failed ({rc}): {self.lib.hb_last_error(self.ctx).decode()}")

    # ---- MPC ------------------------------------------------------------------------------------
    def set_references(self, refs: dict, inst_begin: int = 0):
        n_nodes = _i32(refs["n_nodes"])
        cnt = n_nodes.shape[0]
        t = _f64(refs["t"], (cnt, self.N + 1))
        mode = _i32(refs["mode"], (cnt, self.N))
        x_ref = _f64(refs["x_ref"], (cnt, self.N, 22))
        swing = _f64(refs["swing"], (cnt, self.N, 4, 6))
        self._check(self.lib.hb_mpc_set_references(self.ctx, C.c_int32(inst_begin), C.c_int32(cnt), _p(n_nodes), _p(t),
                                                   _p(mode), _p(x_ref), _p(swing)), "hb_mpc_set_references")

    def reset(self, x0):
        self._check(self.lib.hb_mpc_reset(self.ctx, _p(_f64(x0, (self.B, 22)))), "hb_mpc_reset")

    def set_trajectory(self, x, u):
        self._check(self.lib.hb_mpc_set_trajectory(self.ctx, _p(_f64(x, (self.B, self.N + 1, 22))),
                                                   _p(_f64(u, (self.B, self.N, 22)))), "hb_mpc_set_trajectory")

    def mpc_solve(self, x0=None):
        x0 = None if x0 is None else _f64(x0, (self.B, 22))
        self._check(self.lib.hb_mpc_solve(self.ctx, _p(x0)), "hb_mpc_solve")

    def publish(self):
        self._check(self.lib.hb_mpc_publish(self.ctx), "hb_mpc_publish")

    def get_solution(self):
        x = np.zeros((self.B, self.N + 1, 22))
        u = np.zeros((self.B, self.N, 22))
        self._check(self.lib.hb_mpc_get_solution(self.ctx, C.c_int32(0), C.c_int32(self.B), _p(x), _p(u)), "hb_mpc_get_solution")
        return x, u

    def get_step(self):
        dx = np.zeros((self.B, self.N + 1, 22))
        du = np.zeros((self.B, self.N, 22))
        self._check(self.lib.hb_mpc_get_step(self.ctx, _p(dx), _p(du)), "hb_mpc_get_step")
        return dx, du

    def get_performance(self):
        perf = np.zeros((self.B, 4))
        self._check(self.lib.hb_mpc_get_performance(self.ctx, _p(perf)), "hb_mpc_get_performance")
        return perf

    # ---- WBC ------------------------------------------------------------------------------------
    def wbc_update(self, t_now=None, rbd=None, walk_flag=None, dt=0.002):
        """t_now / rbd None: the device-resident time and rbd state."""
        t_now = None if t_now is None else _f64(t_now, (self.B,))
        rbd = None if rbd is None else _f64(rbd, (self.B, 32))
        walk = None if walk_flag is None else _i32(walk_flag, (self.B,))
        sol, xd, ud = np.zeros((self.B, 38)), np.zeros((self.B, 22)), np.zeros((self.B, 22))
        mode, status = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.hb_wbc_update(self.ctx, _p(t_now), _p(rbd), _p(walk), C.c_double(dt), _p(sol), _p(xd), _p(ud),
                                           _p(mode), _p(status)), "hb_wbc_update")
        return dict(sol=sol, x_des=xd, u_des=ud, mode=mode, status=status)

    def wbc_update_direct(self, x_des, u_des, rbd, mode, stance_flag=None, dt=0.002):
        x_des, u_des, rbd = _f64(x_des, (self.B, 22)), _f64(u_des, (self.B, 22)), _f64(rbd, (self.B, 32))
        mode = _i32(mode, (self.B,))
        stance = None if stance_flag is None else _i32(stance_flag, (self.B,))
        sol, status = np.zeros((self.B, 38)), np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.hb_wbc_update_direct(self.ctx, _p(x_des), _p(u_des), _p(rbd), _p(mode), _p(stance), C.c_double(dt),
                                                  _p(sol), _p(status)), "hb_wbc_update_direct")
        return sol, status

    def joint_command(self, gains: "abi.HbJointGains", dt=0.002):
        """Joint command law of LeggedController::update on the last WBC result -> dict of [B][10] arrays."""
        out = {k: np.zeros((self.B, 10)) for k in ("pos_des", "vel_des", "kp", "kd", "tau_ff", "torque")}
        self._check(self.lib.hb_joint_command(self.ctx, C.byref(gains), C.c_double(dt), *[_p(out[k]) for k in
                                              ("pos_des", "vel_des", "kp", "kd", "tau_ff", "torque")]), "hb_joint_command")
        return out

    def wbc_update_resident(self, dt=0.002):
        """hb_wbc_update on the device-resident time / rbd, results left on the device."""
        self._check(self.lib.hb_wbc_update(self.ctx, None, None, None, C.c_double(dt), None, None, None, None, None), "hb_wbc_update")

    def joint_command_resident(self, gains: "abi.HbJointGains", dt=0.002):
        self._check(self.lib.hb_joint_command(self.ctx, C.byref(gains), C.c_double(dt), None, None, None, None, None, None), "hb_joint_command")

    def reset_masked(self, mask, x0=None):
        """Cold start of the instances with mask[i] != 0 (hb_mpc_reset_masked)."""
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(self.B)
        x = None if x0 is None else _f64(x0, (self.B, 22))
        self._check(self.lib.hb_mpc_reset_masked(self.ctx, _p(m), _p(x)), "hb_mpc_reset_masked")

    def mpc_status(self):
        st = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.hb_mpc_get_status(self.ctx, _p(st)), "hb_mpc_get_status")
        return st

    def joint_set_flags(self, controller_loaded=None, emergency_stop=None):
        a = None if controller_loaded is None else _i32(controller_loaded, (self.B,))
        b = None if emergency_stop is None else _i32(emergency_stop, (self.B,))
        self._check(self.lib.hb_joint_set_flags(self.ctx, _p(a), _p(b)), "hb_joint_set_flags")

    def joint_emergency_stop(self):
        st = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.hb_joint_get_emergency_stop(self.ctx, _p(st)), "hb_joint_get_emergency_stop")
        return st

    def reset_resident(self):
        """Cold start of the MPC iterate from the device-resident observation (hb_mpc_reset with x0 = NULL)."""
        self._check(self.lib.hb_mpc_reset(self.ctx, None), "hb_mpc_reset")

    # ---- plant stub (closed-loop rollouts) -----------------------------------------------------------------------------
    def plant_reset(self, q0, v0=None, baumgarte=30.0, eps=1e-8):
        v = None if v0 is None else _f64(v0, (self.B, 16))
        self._check(self.lib.hb_plant_reset(self.ctx, _p(_f64(q0, (self.B, 16))), _p(v), C.c_double(baumgarte), C.c_double(eps)), "hb_plant_reset")

    def plant_step(self, tau=None, contact=None, dt=0.002, substeps=4, to_resident=False):
        tau = None if tau is None else _f64(tau, (self.B, 10))
        contact = None if contact is None else _i32(contact, (self.B, 4))
        self._check(self.lib.hb_plant_step(self.ctx, _p(tau), _p(contact), C.c_double(dt), C.c_int32(substeps), C.c_int32(1 if to_resident else 0)),
                    "hb_plant_step")

    # ---- actuator loop per substep (hb_plant_step_hybrid) and the simulator end of the LCM link ---------------------------------
    def plant_step_hybrid(self, command=None, contact=None, dt=0.002, substeps=4, to_resident=False):
        """A hybrid step: the law ff + kp (pos_des - q) + kd (vel_des - qd) evaluated before every substep from the plant's own state.
        command: dict(pos_des, vel_des, kp, kd, tau_ff) of [B][10] arrays (what joint_command returns), or None for the command the
        last joint_command left on the device.  A missing key is passed as NULL (the library refuses a partly given command)."""
        keys = ("pos_des", "vel_des", "kp", "kd", "tau_ff")
        arrs = [None] * 5 if command is None else [None if command.get(k) is None else _f64(command[k], (self.B, 10)) for k in keys]
        contact = None if contact is None else _i32(contact, (self.B, 4))
        self._check(self.lib.hb_plant_step_hybrid(self.ctx, *[_p(a) for a in arrs], _p(contact), C.c_double(dt), C.c_int32(substeps),
                                                  C.c_int32(1 if to_resident else 0)), "hb_plant_step_hybrid")

    def plant_step_lcm(self, low_cmd, contact=None, dt=0.002, substeps=4, to_resident=False):
        """hb_plant_step_lcm: low_cmd[B][496] wire images of low_cmd_t through the simulator's timestamp filter, then a hybrid step on the
        received commands -> accepted[B] int32."""
        wire = np.ascontiguousarray(low_cmd, dtype=np.uint8)
        assert wire.shape == (self.B, 496)
        contact = None if contact is None else _i32(contact, (self.B, 4))
        accepted = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.hb_plant_step_lcm(self.ctx, _p(wire), _p(contact), C.c_double(dt), C.c_int32(substeps),
                                               C.c_int32(1 if to_resident else 0), _p(accepted)), "hb_plant_step_lcm")
        return accepted

    def plant_sense_lcm(self, timestamp_ns: int, low_state=True, full_state=True):
        """hb_plant_sense_lcm: one plant_sense, packed on the device -> (low_state_t wire images [B][336] or None, full_state_t [B][464] or
        None)."""
        low = np.zeros((self.B, 336), dtype=np.uint8) if low_state else None
        full = np.zeros((self.B, 464), dtype=np.uint8) if full_state else None
        self._check(self.lib.hb_plant_sense_lcm(self.ctx, C.c_int64(timestamp_ns), _p(low), _p(full)), "hb_plant_sense_lcm")
        return low, full

    def plant_get_actuator(self):
        """-> dict(tau_first[B][10], tau_mean[B][10] of the last hybrid step, last_timestamp[B] int64: the stored bits of the timestamp
        filter of plant_step_lcm)."""
        out = dict(tau_first=np.zeros((self.B, 10)), tau_mean=np.zeros((self.B, 10)), last_timestamp=np.zeros(self.B, dtype=np.int64))
        self._check(self.lib.hb_plant_get_actuator(self.ctx, *[_p(a) for a in out.values()]), "hb_plant_get_actuator")
        return out

    def plant_state(self):
        out = dict(q=np.zeros((self.B, 16)), v=np.zeros((self.B, 16)), rbd=np.zeros((self.B, 32)), lam=np.zeros((self.B, 12)),
                   vdot=np.zeros((self.B, 16)))
        self._check(self.lib.hb_plant_get_state(self.ctx, _p(out["q"]), _p(out["v"]), _p(out["rbd"]), _p(out["lam"]), _p(out["vdot"])),
                    "hb_plant_get_state")
        return out

    # ---- contact model of the plant (hb_plant_set_contact_model) ---------------------------------------------------------------
    def plant_set_contact_model(self, contact_cfg: "abi.HbContactConfig" = None):
        """contact_cfg None: the pinned stub (model 0); abi.make_contact_config(params, ...): ground with unilateral frictional contact."""
        self._check(self.lib.hb_plant_set_contact_model(self.ctx, None if contact_cfg is None else C.byref(contact_cfg)),
                    "hb_plant_set_contact_model")

    def plant_set_external_wrench(self, wrench=None):
        """wrench [B][6] = world force, world moment at the base origin, applied by every later step of the ground model; None clears."""
        w = None if wrench is None else _f64(wrench, (self.B, 6))
        self._check(self.lib.hb_plant_set_external_wrench(self.ctx, _p(w)), "hb_plant_set_external_wrench")

    def plant_contact(self):
        """Contact outputs of the last step of the ground model -> dict(gap[B][4], point_vel[B][4][3], residual[B], touching[B][4] int32,
        status[B] int32: bits abi.HB_CONTACT_*)."""
        out = dict(gap=np.zeros((self.B, 4)), point_vel=np.zeros((self.B, 4, 3)), residual=np.zeros(self.B),
                   touching=np.zeros((self.B, 4), dtype=np.int32), status=np.zeros(self.B, dtype=np.int32))
        self._check(self.lib.hb_plant_get_contact(self.ctx, *[_p(a) for a in out.values()]), "hb_plant_get_contact")
        return out

    # ---- joint model of the ground-contact plant (hb_plant_set_joint_model) ---------------------------------------------------
    def plant_set_joint_model(self, joint_model: "abi.HbJointModel" = None):
        """joint_model None: ideal joints; abi.make_joint_model(params, ...): rotor inertia, damping, dry friction, stops and torque
        saturation in the ground-contact model (plant_set_contact_model first)."""
        self._check(self.lib.hb_plant_set_joint_model(self.ctx, None if joint_model is None else C.byref(joint_model)),
                    "hb_plant_set_joint_model")

    def plant_get_joints(self):
        """Joint outputs of the last step under the joint model -> dict(tau_applied[B][10], friction_torque[B][10], limit_torque[B][10],
        residual[B], status[B] int32: bit j = stop of joint j active, bit 10 + j = torque of joint j saturated, abi.HB_JOINT_UNCONVERGED)."""
        out = dict(tau_applied=np.zeros((self.B, 10)), friction_torque=np.zeros((self.B, 10)), limit_torque=np.zeros((self.B, 10)),
                   residual=np.zeros(self.B), status=np.zeros(self.B, dtype=np.int32))
        self._check(self.lib.hb_plant_get_joints(self.ctx, *[_p(a) for a in out.values()]), "hb_plant_get_joints")
        return out

    # ---- per-instance terrain of the ground-contact plant (hb_plant_set_terrain) ---------------------------------------------------
    def plant_set_terrain(self, plane=None, mu=None):
        """plane [B][4] = unit normal and offset of the instance's ground plane n . x = d (None: (0, 0, 1, ground_z)); mu [B][4] = friction
        coefficient per contact point (None: the contact model's mu).  Both None: no terrain.  Clears the contact impulses."""
        pl = None if plane is None else _f64(plane, (self.B, 4))
        m = None if mu is None else _f64(mu, (self.B, 4))
        self._check(self.lib.hb_plant_set_terrain(self.ctx, _p(pl), _p(m)), "hb_plant_set_terrain")

    def plant_get_terrain(self):
        """-> dict(plane[B][4], mu[B][4], frame[B][3][3] = T = [t1 t2 n] with the axes in columns) of the terrain in force; without one,
        what the contact model amounts to."""
        out = dict(plane=np.zeros((self.B, 4)), mu=np.zeros((self.B, 4)), frame=np.zeros((self.B, 3, 3)))
        self._check(self.lib.hb_plant_get_terrain(self.ctx, *[_p(a) for a in out.values()]), "hb_plant_get_terrain")
        return out

    # ---- per-instance terrain profile of the ground-contact plant (hb_plant_set_terrain_profile) ------------------------------------
    def plant_set_terrain_profile(self, n_knots=None, direction=None, knots=None, mu=None):
        """Piecewise-planar ground per instance: n_knots [B]; direction [B][2] = the horizontal direction s is measured along; knots
        [B][K][2] = (s_k, z_k) with K <= abi.HB_PROFILE_MAX_KNOTS (rows from n_knots[i] on are not read); mu [B][4] per contact point (None:
        the contact model's mu).  All None: no profile.  Replaces a terrain of plant_set_terrain; clears the contact impulses."""
        if n_knots is None and direction is None and knots is None and mu is None:
            self._check(self.lib.hb_plant_set_terrain_profile(self.ctx, None, None, None, None), "hb_plant_set_terrain_profile")
            return
        nk = _i32(n_knots, (self.B,))
        d = _f64(direction, (self.B, 2))
        k = np.asarray(knots, dtype=np.float64)
        assert k.ndim == 3 and k.shape[0] == self.B and k.shape[1] <= abi.HB_PROFILE_MAX_KNOTS and k.shape[2] == 2, k.shape
        kk = np.zeros((self.B, abi.HB_PROFILE_MAX_KNOTS, 2))
        kk[:, :k.shape[1]] = k
        m = None if mu is None else _f64(mu, (self.B, 4))
        self._check(self.lib.hb_plant_set_terrain_profile(self.ctx, _p(nk), _p(d), _p(kk), _p(m)), "hb_plant_set_terrain_profile")

    def plant_get_terrain_profile(self):
        """-> dict(n_knots[B], dir[B][2], knots[B][16][2], mu[B][4], records[B][15][10] = (T_j row-major, d_j) per segment, segment[B][5] =
        the segment under the four contact points and under the base origin at the end of the last step) of the profile in force."""
        K = abi.HB_PROFILE_MAX_KNOTS
        out = dict(n_knots=np.zeros(self.B, dtype=np.int32), dir=np.zeros((self.B, 2)), knots=np.zeros((self.B, K, 2)), mu=np.zeros((self.B, 4)),
                   records=np.zeros((self.B, K - 1, abi.HB_PROFILE_RECORD)), segment=np.zeros((self.B, 5), dtype=np.int32))
        self._check(self.lib.hb_plant_get_terrain_profile(self.ctx, *[_p(a) for a in out.values()]), "hb_plant_get_terrain_profile")
        return out

    # ---- per-instance height field of the ground-contact plant (hb_plant_set_terrain_field) ------------------------------------------
    def plant_set_terrain_field(self, direction=None, origin=None, spacing=None, heights=None, mu=None):
        """Triangulated height field per instance: direction [B][2] = the first grid axis a (the second is b = (-a_y, a_x)); origin [B][2]
        = grid coordinates (u0, w0) of node (0, 0); spacing [B][2] = (du, dw); heights = a [B][nu][nw] array, or a list of B arrays
        [nu_i][nw_i], 2 <= nu, nw <= abi.HB_FIELD_MAX_NODES; mu [B][4] per contact point (None: the contact model's mu).  All None: no
        field.  Replaces a terrain or a profile; clears the contact impulses."""
        if direction is None and origin is None and spacing is None and heights is None and mu is None:
            self._check(self.lib.hb_plant_set_terrain_field(self.ctx, None, None, None, None, None, None), "hb_plant_set_terrain_field")
            return
        N = abi.HB_FIELD_MAX_NODES
        assert len(heights) == self.B, len(heights)
        n, z = np.zeros((self.B, 2), dtype=np.int32), np.zeros((self.B, N, N))
        for i, h in enumerate(heights):
            h = np.asarray(h, dtype=np.float64)
            assert h.ndim == 2, h.shape
            n[i] = h.shape
            z[i, :min(N, h.shape[0]), :min(N, h.shape[1])] = h[:N, :N]
        m = None if mu is None else _f64(mu, (self.B, 4))
        self._check(self.lib.hb_plant_set_terrain_field(self.ctx, _p(n), _p(_f64(direction, (self.B, 2))), _p(_f64(origin, (self.B, 2))),
                                                        _p(_f64(spacing, (self.B, 2))), _p(z), _p(m)), "hb_plant_set_terrain_field")

    def plant_get_terrain_field(self):
        """-> dict(n_nodes[B][2], dir[B][2] as stored, origin[B][2], spacing[B][2], heights[B][32][32], mu[B][4], facet[B][5] = the facet id
        under the four contact points and under the base origin at the end of the last step) of the field in force."""
        N = abi.HB_FIELD_MAX_NODES
        out = dict(n_nodes=np.zeros((self.B, 2), dtype=np.int32), dir=np.zeros((self.B, 2)), origin=np.zeros((self.B, 2)), spacing=np.zeros((self.B, 2)),
                   heights=np.zeros((self.B, N, N)), mu=np.zeros((self.B, 4)), facet=np.zeros((self.B, 5), dtype=np.int32))
        self._check(self.lib.hb_plant_get_terrain_field(self.ctx, *[_p(a) for a in out.values()]), "hb_plant_get_terrain_field")
        return out

    def plant_field_eval(self, xyz):
        """The device facet selection of the field in force: xyz [B][n][3] world points per instance -> (facet_id[B][n],
        records[B][n][10] = (T row-major, d), height[B][n] = n . x - d)."""
        x = np.ascontiguousarray(xyz, dtype=np.float64)
        assert x.ndim == 3 and x.shape[0] == self.B and x.shape[2] == 3, x.shape
        n = x.shape[1]
        fid, rec, h = np.zeros((self.B, n), dtype=np.int32), np.zeros((self.B, n, abi.HB_PROFILE_RECORD)), np.zeros((self.B, n))
        self._check(self.lib.hb_plant_field_eval(self.ctx, C.c_int32(n), _p(x), _p(fid), _p(rec), _p(h)), "hb_plant_field_eval")
        return fid, rec, h

    # ---- ground map of the controller (hb_ground_set_profile) -----------------------------------------------------------------------
    def ground_set_profile(self, n_knots=None, direction=None, knots=None):
        """Height profile the planner, the command target and the filter take for the ground, per instance: n_knots [B]; direction
        [B][2]; knots [B][K][2] = (s_k, g_k) with K <= abi.HB_PROFILE_MAX_KNOTS (rows from n_knots[i] on are not read), heights relative
        to the level ground of a controller without a map.  All None: no map.  Independent of the plant's ground."""
        nk = None if n_knots is None else _i32(n_knots, (self.B,))
        d = None if direction is None else _f64(direction, (self.B, 2))
        kk = None
        if knots is not None:
            k = np.asarray(knots, dtype=np.float64)
            assert k.ndim == 3 and k.shape[0] == self.B and k.shape[1] <= abi.HB_PROFILE_MAX_KNOTS and k.shape[2] == 2, k.shape
            kk = np.zeros((self.B, abi.HB_PROFILE_MAX_KNOTS, 2))
            kk[:, :k.shape[1]] = k
        self._check(self.lib.hb_ground_set_profile(self.ctx, _p(nk), _p(d), _p(kk)), "hb_ground_set_profile")

    def ground_get_profile(self):
        """-> dict(n_knots[B], dir[B][2] as stored, knots[B][16][2], slopes[B][15]) of the map in force."""
        K = abi.HB_PROFILE_MAX_KNOTS
        out = dict(n_knots=np.zeros(self.B, dtype=np.int32), dir=np.zeros((self.B, 2)), knots=np.zeros((self.B, K, 2)), slopes=np.zeros((self.B, K - 1)))
        self._check(self.lib.hb_ground_get_profile(self.ctx, *[_p(a) for a in out.values()]), "hb_ground_get_profile")
        return out

    def ground_set_field(self, direction=None, origin=None, spacing=None, heights=None):
        """Two-dimensional height field the planner, the command target and the filter take for the ground, per instance — the grid of
        plant_set_terrain_field without its friction: direction [B][2] = the first grid axis a (the second is b = (-a_y, a_x)); origin
        [B][2]; spacing [B][2]; heights = a [B][nu][nw] array or a list of B arrays [nu_i][nw_i], relative to the level ground of a
        controller without a map.  All None: no map.  Replaces a profile map (ground_set_profile); independent of the plant's ground."""
        if direction is None and origin is None and spacing is None and heights is None:
            self._check(self.lib.hb_ground_set_field(self.ctx, None, None, None, None, None), "hb_ground_set_field")
            return
        N = abi.HB_FIELD_MAX_NODES
        assert len(heights) == self.B, len(heights)
        n, z = np.zeros((self.B, 2), dtype=np.int32), np.zeros((self.B, N, N))
        for i, h in enumerate(heights):
            h = np.asarray(h, dtype=np.float64)
            assert h.ndim == 2, h.shape
            n[i] = h.shape
            z[i, :min(N, h.shape[0]), :min(N, h.shape[1])] = h[:N, :N]
        self._check(self.lib.hb_ground_set_field(self.ctx, _p(n), _p(_f64(direction, (self.B, 2))), _p(_f64(origin, (self.B, 2))),
                                                 _p(_f64(spacing, (self.B, 2))), _p(z)), "hb_ground_set_field")

    def ground_get_field(self):
        """-> dict(n_nodes[B][2], dir[B][2] as stored, origin[B][2], spacing[B][2], heights[B][32][32]) of the field map in force."""
        N = abi.HB_FIELD_MAX_NODES
        out = dict(n_nodes=np.zeros((self.B, 2), dtype=np.int32), dir=np.zeros((self.B, 2)), origin=np.zeros((self.B, 2)), spacing=np.zeros((self.B, 2)),
                   heights=np.zeros((self.B, N, N)))
        self._check(self.lib.hb_ground_get_field(self.ctx, *[_p(a) for a in out.values()]), "hb_ground_get_field")
        return out

    # ---- foothold mode on the ground map (hb_ground_set_foothold) ------------------------------------------------------------------
    def ground_set_foothold(self, cfg=None, **fields):
        """cfg: an abi.HbFootholdConfig, or None with fields of abi.make_foothold_config (mode="sole" or "point" must be among them; n_shift,
        shift_step, flat_tol); no argument at all: off.  Mode 1 plans the toe and the heel of a foot as one sole on the map in force."""
        if cfg is None and fields:
            cfg = abi.make_foothold_config(**fields)
        self._check(self.lib.hb_ground_set_foothold(self.ctx, None if cfg is None else C.byref(cfg)), "hb_ground_set_foothold")

    def ground_get_foothold(self):
        """-> dict(mode, n_shift, shift_step, flat_tol) of the configuration in force (all zero while off)."""
        out = abi.HbFootholdConfig()
        self._check(self.lib.hb_ground_get_foothold(self.ctx, C.byref(out)), "hb_ground_get_foothold")
        return dict(mode=out.mode, n_shift=out.n_shift, shift_step=out.shift_step, flat_tol=out.flat_tol)

    def ground_get_foothold_choice(self, inst_begin=0, inst_count=None):
        """What the last planner pass in sole mode decided for the first foothold of every foot -> dict(shift[count][2] int32
        (abi.HB_NO_FOOTHOLD: none planned), defect[count][2], level[count][2] int32)."""
        cnt = self.B - inst_begin if inst_count is None else inst_count
        out = dict(shift=np.zeros((cnt, 2), dtype=np.int32), defect=np.zeros((cnt, 2)), level=np.zeros((cnt, 2), dtype=np.int32))
        self._check(self.lib.hb_ground_get_foothold_choice(self.ctx, C.c_int32(inst_begin), C.c_int32(cnt), *[_p(a) for a in out.values()]),
                    "hb_ground_get_foothold_choice")
        return out

    def ground_eval(self, inst, xy):
        """The device height function of the map in force at n points: inst [n] = the instance whose map a point is put to, xy [n][2]
        -> (height[n], segment[n]); under a field map segment is the facet id."""
        ii = _i32(inst)
        n = ii.shape[0]
        p = _f64(xy, (n, 2))
        h, seg = np.zeros(n), np.zeros(n, dtype=np.int32)
        self._check(self.lib.hb_ground_eval(self.ctx, C.c_int32(n), _p(ii), _p(p), _p(h), _p(seg)), "hb_ground_eval")
        return h, seg

    # ---- per-instance model variation of the ground-contact plant (hb_plant_set_model_variation) -------------------------------------
    def plant_set_model_variation(self, mass_scale=None, payload=None):
        """mass_scale [B][11] = a scale of mass and inertia per body (None: 1); payload [B][10] = mass, position[3] in the base frame,
        inertia[6] = xx xy xz yy yz zz about its own centre of mass, of a payload on the base (None: none; rollout.payload_on_base packs
        it).  Both None: no variation.  The plant steps on the varied model, the controller keeps the nominal one."""
        sc = None if mass_scale is None else _f64(mass_scale, (self.B, abi.NBODY))
        pl = None if payload is None else _f64(payload, (self.B, abi.HB_PAYLOAD_SIZE))
        self._check(self.lib.hb_plant_set_model_variation(self.ctx, _p(sc), _p(pl)), "hb_plant_set_model_variation")

    def plant_model_variation(self):
        """-> dict(mass[B][11], com[B][11][3], inertia[B][11][6], total_mass[B]) of the model every instance steps on; without a
        variation the nominal model repeated."""
        out = dict(mass=np.zeros((self.B, abi.NBODY)), com=np.zeros((self.B, abi.NBODY, 3)), inertia=np.zeros((self.B, abi.NBODY, 6)),
                   total_mass=np.zeros(self.B))
        self._check(self.lib.hb_plant_get_model_variation(self.ctx, *[_p(a) for a in out.values()]), "hb_plant_get_model_variation")
        return out

    # ---- per-instance episode record and stop-on-fall (hb_plant_set_episode) -----------------------------------------------------
    def plant_set_episode(self, cfg: "abi.HbEpisodeConfig" = None):
        """cfg None: no episode; abi.make_episode_config(...): the record of every instance (re)starts from the plant's present state and
        is updated on the device after every plant step."""
        self._check(self.lib.hb_plant_set_episode(self.ctx, None if cfg is None else C.byref(cfg)), "hb_plant_set_episode")
        self._episode_capacity = 0 if cfg is None else int(cfg.trace_capacity)

    def plant_episode(self, want_trace=False):
        """The episode records -> dict of named arrays (abi.EPISODE_INT_FIELDS / EPISODE_DOUBLE_FIELDS: [B] or [B][n]); want_trace adds
        trace[B][trace_capacity][8] (columns abi.EPISODE_TRACE_COLUMNS; the first N_TRACE samples of an instance are valid)."""
        irec, drec = np.zeros((self.B, abi.HB_EP_NI), dtype=np.int32), np.zeros((self.B, abi.HB_EP_ND))
        cap = getattr(self, "_episode_capacity", 0)
        trace = np.zeros((self.B, cap, abi.HB_EP_TRACE_W)) if want_trace else None
        self._check(self.lib.hb_plant_get_episode(self.ctx, _p(irec), _p(drec), _p(trace) if cap else None), "hb_plant_get_episode")
        out = abi.split_episode_record(irec, drec)
        if want_trace:
            out["trace"] = trace
        return out

    # ---- respawn of ended instances (hb_plant_set_respawn) ---------------------------------------------------------------------------
    def plant_set_respawn(self, cfg: "abi.HbRespawnConfig" = None, q_spawn=None, v_spawn=None):
        """cfg None: off; abi.make_respawn_config(...) with q_spawn[B][16] (v_spawn[B][16] or None = zero): plant_respawn() puts every
        instance whose episode is over back to a state drawn from it.  Needs plant_set_episode; starts the totals."""
        q = None if q_spawn is None else _f64(q_spawn, (self.B, 16))
        v = None if v_spawn is None else _f64(v_spawn, (self.B, 16))
        self._check(self.lib.hb_plant_set_respawn(self.ctx, None if cfg is None else C.byref(cfg), _p(q), _p(v)), "hb_plant_set_respawn")

    def plant_respawn(self):
        """Enqueue-only: the device respawns the instances whose episode record says so (hb_plant_respawn)."""
        self._check(self.lib.hb_plant_respawn(self.ctx), "hb_plant_respawn")

    def plant_respawn_totals(self, want_state=False):
        """The totals of the finished episodes -> dict of [B] arrays keyed by field name (abi.RESPAWN_INT_FIELDS / RESPAWN_DOUBLE_FIELDS);
        want_state adds q_last / v_last [B][16], the last spawned state."""
        itot, dtot = np.zeros((self.B, abi.HB_RS_NI), dtype=np.int32), np.zeros((self.B, abi.HB_RS_ND))
        q, v = (np.zeros((self.B, 16)), np.zeros((self.B, 16))) if want_state else (None, None)
        self._check(self.lib.hb_plant_get_respawn(self.ctx, _p(itot), _p(dtot), _p(q), _p(v)), "hb_plant_get_respawn")
        out = abi.split_respawn_totals(itot, dtot)
        if want_state:
            out["q_last"], out["v_last"] = q, v
        return out

    # ---- scenario draw at respawn (hb_plant_set_scenario) -----------------------------------------------------------------------------
    def plant_set_scenario(self, cfg: "abi.HbScenarioConfig" = None):
        """cfg None: off; abi.make_scenario_config(...): every plant_respawn() draws terrain, friction, payload, link masses and a push
        (the channels of cfg) for the instances it respawns.  Needs contact model 1 and plant_set_respawn."""
        self._check(self.lib.hb_plant_set_scenario(self.ctx, None if cfg is None else C.byref(cfg)), "hb_plant_set_scenario")
        self._scenario_log_capacity = 0 if cfg is None else int(cfg.log_capacity)

    def plant_scenario(self):
        """-> scen[B][HB_SC_N], the parameters every instance's current episode runs under (abi.split_scenario names them)."""
        scen = np.zeros((self.B, abi.HB_SC_N))
        self._check(self.lib.hb_plant_get_scenario(self.ctx, _p(scen)), "hb_plant_get_scenario")
        return scen

    def plant_scenario_log(self):
        """-> dict(count[B] int32, log[B][log_capacity][HB_SC_LOG_W]): the finished episodes of every instance in order, each row
        abi.SCENARIO_LOG_HEAD and then the HB_SC_N parameters it ran under; rows behind count are zero."""
        cap = getattr(self, "_scenario_log_capacity", 0)
        count, log = np.zeros(self.B, dtype=np.int32), np.zeros((self.B, cap, abi.HB_SC_LOG_W))
        self._check(self.lib.hb_plant_get_scenario_log(self.ctx, _p(count), _p(log) if cap else None), "hb_plant_get_scenario_log")
        return dict(count=count, log=log)

    # ---- profile draw at respawn (hb_plant_set_profile_draw) --------------------------------------------------------------------------
    def plant_set_profile_draw(self, cfg: "abi.HbProfileDrawConfig" = None):
        """cfg None: off; abi.make_profile_draw_config(...): every plant_respawn() draws level ground, a curb / step-down or a flight of
        stairs (the kinds of cfg) for the instances it respawns and places them on it.  Needs contact model 1 and plant_set_respawn; with
        follow_map a ground map in force (ground_set_profile), which then follows the drawn ground."""
        self._check(self.lib.hb_plant_set_profile_draw(self.ctx, None if cfg is None else C.byref(cfg)), "hb_plant_set_profile_draw")
        self._profile_draw_log_capacity = 0 if cfg is None else int(cfg.log_capacity)

    def plant_profile_draw(self):
        """-> row[B][HB_PD_N], the parameters every instance's current ground was drawn with (abi.split_profile_draw names them)."""
        row = np.zeros((self.B, abi.HB_PD_N))
        self._check(self.lib.hb_plant_get_profile_draw(self.ctx, _p(row)), "hb_plant_get_profile_draw")
        return row

    def plant_profile_draw_log(self):
        """-> dict(count[B] int32, log[B][log_capacity][HB_PD_LOG_W]): the finished episodes of every instance in order, each row
        abi.PROFILE_DRAW_LOG_HEAD and then the HB_PD_N parameters it ran under; rows behind count are zero."""
        cap = getattr(self, "_profile_draw_log_capacity", 0)
        count, log = np.zeros(self.B, dtype=np.int32), np.zeros((self.B, cap, abi.HB_PD_LOG_W))
        self._check(self.lib.hb_plant_get_profile_draw_log(self.ctx, _p(count), _p(log) if cap else None), "hb_plant_get_profile_draw_log")
        return dict(count=count, log=log)

    # ---- field draw at respawn (hb_plant_set_field_draw) ------------------------------------------------------------------------------
    def plant_set_field_draw(self, cfg: "abi.HbFieldDrawConfig" = None):
        """cfg None: off; abi.make_field_draw_config(...): every plant_respawn() composes a height field (level, rough, tilted or both: the
        kinds of cfg) on the device for the instances it respawns and places them on it.  Needs contact model 1 and plant_set_respawn;
        with follow_map a field map in force (ground_set_field), which then follows the drawn field."""
        self._check(self.lib.hb_plant_set_field_draw(self.ctx, None if cfg is None else C.byref(cfg)), "hb_plant_set_field_draw")
        self._field_draw_log_capacity = 0 if cfg is None else int(cfg.log_capacity)

    def plant_get_field_draw(self):
        """-> row[B][HB_FD_N], the parameters every instance's current ground was drawn with (abi.split_field_draw names them)."""
        row = np.zeros((self.B, abi.HB_FD_N))
        self._check(self.lib.hb_plant_get_field_draw(self.ctx, _p(row)), "hb_plant_get_field_draw")
        return row

    def plant_get_field_draw_log(self):
        """-> dict(count[B] int32, log[B][log_capacity][HB_FD_LOG_W]): the finished episodes of every instance in order, each row
        abi.FIELD_DRAW_LOG_HEAD and then the HB_FD_N parameters it ran under; rows behind count are zero."""
        cap = getattr(self, "_field_draw_log_capacity", 0)
        count, log = np.zeros(self.B, dtype=np.int32), np.zeros((self.B, cap, abi.HB_FD_LOG_W))
        self._check(self.lib.hb_plant_get_field_draw_log(self.ctx, _p(count), _p(log) if cap else None), "hb_plant_get_field_draw_log")
        return dict(count=count, log=log)

    # ---- height scan (hb_plant_set_height_scan) ----------------------------------------------------------------------------------------
    def plant_set_height_scan(self, cfg: "abi.HbHeightScanConfig" = None):
        """cfg None: off (the map last written stays in force); abi.make_height_scan_config(...): plant_scan() writes the controller's field
        map from the plant's ground.  Needs contact model 1 and a field map in force (ground_set_field: the zero map over the scan grid)."""
        self._check(self.lib.hb_plant_set_height_scan(self.ctx, None if cfg is None else C.byref(cfg)), "hb_plant_set_height_scan")

    def plant_scan(self):
        """One scan of every instance; enqueue-only."""
        self._check(self.lib.hb_plant_scan(self.ctx), "hb_plant_scan")

    def plant_get_height_scan(self):
        """-> dict(cfg: the configuration in force (dir as stored), origin_index[B][2] int32, n_returns[B] int32 (-1: the last scan skipped
        the instance), returned[B][32][32] uint8 (1: the node had a return)), as the last scan left them."""
        cfg = abi.HbHeightScanConfig()
        org, n = np.zeros((self.B, 2), dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        ret = np.zeros((self.B, abi.HB_FIELD_MAX_NODES, abi.HB_FIELD_MAX_NODES), dtype=np.uint8)
        self._check(self.lib.hb_plant_get_height_scan(self.ctx, C.byref(cfg), _p(org), _p(n), _p(ret)), "hb_plant_get_height_scan")
        return dict(cfg=cfg, origin_index=org, n_returns=n, returned=ret)

    # ---- sensors from the plant (hb_plant_sense) and the estimator on them ------------------------------------------------
    def plant_set_sensor_model(self, sensor_cfg: "abi.HbSensorConfig" = None, gyro_bias=None, accel_bias=None):
        """sensor_cfg None: ideal sensors; gyro_bias / accel_bias [B][3] or None (zero).  Restarts the noise counter."""
        gb = None if gyro_bias is None else _f64(gyro_bias, (self.B, 3))
        ab = None if accel_bias is None else _f64(accel_bias, (self.B, 3))
        self._check(self.lib.hb_plant_set_sensor_model(self.ctx, None if sensor_cfg is None else C.byref(sensor_cfg), _p(gb), _p(ab)),
                    "hb_plant_set_sensor_model")

    def plant_sense(self, want_outputs=False):
        """One sensor reading of every instance, left on the device for estimator_update_resident.  want_outputs: -> dict(quat[B][4],
        ang_vel_local[B][3], lin_acc_local[B][3], joint_pos / joint_vel / joint_torque [B][10], contact_flag[B][4] int32); otherwise
        the call is enqueue-only and returns None."""
        out = None
        if want_outputs:
            out = dict(quat=np.zeros((self.B, 4)), ang_vel_local=np.zeros((self.B, 3)), lin_acc_local=np.zeros((self.B, 3)),
                       joint_pos=np.zeros((self.B, 10)), joint_vel=np.zeros((self.B, 10)), joint_torque=np.zeros((self.B, 10)),
                       contact_flag=np.zeros((self.B, 4), dtype=np.int32))
        ptrs = [None] * 7 if out is None else [_p(a) for a in out.values()]
        self._check(self.lib.hb_plant_sense(self.ctx, *ptrs), "hb_plant_sense")
        return out

    def estimator_update_resident(self, dt, to_resident=False, want_outputs=False):
        """hb_estimator_update on the arrays the last plant_sense left on the device -> (rbd[B][32], x_state[B][22]), or (None, None)
        for the enqueue-only form."""
        rbd, x = (np.zeros((self.B, 32)), np.zeros((self.B, 22))) if want_outputs else (None, None)
        self._check(self.lib.hb_estimator_update_resident(self.ctx, C.c_double(dt), C.c_int32(1 if to_resident else 0), _p(rbd), _p(x)),
                    "hb_estimator_update_resident")
        return rbd, x

    def estimator_contact_force_resident(self, dt, want_outputs=True):
        """hb_estimator_contact_force(rbd = None) on the sensed joint torque -> (estDisturbancetorque_ [B][16], estContactforce_ [B][16])."""
        dist, cf = (np.zeros((self.B, 16)), np.zeros((self.B, 16))) if want_outputs else (None, None)
        self._check(self.lib.hb_estimator_contact_force_resident(self.ctx, C.c_double(dt), _p(dist), _p(cf)),
                    "hb_estimator_contact_force_resident")
        return dist, cf

    # ---- device-resident stepping -----------------------------------------------------------------
    def set_resident_inputs(self, x0, t_now, rbd, walk_flag=None):
        walk = None if walk_flag is None else _i32(walk_flag, (self.B,))
        self._check(self.lib.hb_set_resident_inputs(self.ctx, _p(_f64(x0, (self.B, 22))), _p(_f64(t_now, (self.B,))),
                                                    _p(_f64(rbd, (self.B, 32))), _p(walk)), "hb_set_resident_inputs")

    def set_resident_time(self, t_now):
        self._check(self.lib.hb_set_resident_time(self.ctx, _p(_f64(t_now, (self.B,)))), "hb_set_resident_time")

    def set_resident_x0_sequence(self, x0_seq):
        if x0_seq is None:  # back to the single device-resident observation
            self._check(self.lib.hb_set_resident_x0_sequence(self.ctx, C.c_int32(0), None), "hb_set_resident_x0_sequence")
            return
        x0_seq = _f64(x0_seq)
        assert x0_seq.ndim == 3 and x0_seq.shape[1:] == (self.B, 22)
        self._check(self.lib.hb_set_resident_x0_sequence(self.ctx, C.c_int32(x0_seq.shape[0]), _p(x0_seq)), "hb_set_resident_x0_sequence")

    def tick_resident(self, dt_est, quat, ang_vel_local, lin_acc_local, joint_pos, joint_vel, contact_flag, t_now, horizon, cmd_vel, dt=0.002):
        """Controller time + estimator + reference generation + MPC iteration + publish + policy + WBC on the resident state,
        enqueue-only (hb_tick_resident); per instance range when set_chunks(n > 1)."""
        self._check(self.lib.hb_tick_resident(
            self.ctx, C.c_double(dt_est), _p(_f64(quat, (self.B, 4))), _p(_f64(ang_vel_local, (self.B, 3))), _p(_f64(lin_acc_local, (self.B, 3))),
            _p(_f64(joint_pos, (self.B, 10))), _p(_f64(joint_vel, (self.B, 10))), _p(_i32(contact_flag, (self.B, 4))), _p(_f64(t_now, (self.B,))),
            C.c_double(horizon), _p(_f64(cmd_vel, (self.B, 4))), C.c_double(dt)), "hb_tick_resident")

    def set_chunks(self, n_chunks: int):
        self._check(self.lib.hb_set_chunks(self.ctx, C.c_int32(n_chunks)), "hb_set_chunks")

    def step_resident(self, dt=0.002):
        self._check(self.lib.hb_step_resident(self.ctx, C.c_double(dt)), "hb_step_resident")

    def get_wbc_solution(self):
        sol, status = np.zeros((self.B, 38)), np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.hb_get_wbc_solution(self.ctx, _p(sol), _p(status)), "hb_get_wbc_solution")
        return sol, status

    def get_wbc_iterations(self):
        """Active-set iterations of the last WBC solve per instance."""
        it = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.hb_get_wbc_iterations(self.ctx, _p(it)), "hb_get_wbc_iterations")
        return it

    # field order of hunter_hip.h's HB_WBC_CERT_* (the certificate of one instance)
    WBC_CERT_FIELDS = ("r_eq", "r_in", "r_stat", "r_dual", "r_comp", "n_active", "eps", "scale")

    def wbc_set_certificate(self, enable: bool = True):
        """KKT certificate + dual solution of the WeightedWbc QP on every later WBC call (hb_wbc_set_certificate)."""
        self._check(self.lib.hb_wbc_set_certificate(self.ctx, C.c_int32(1 if enable else 0)), "hb_wbc_set_certificate")

    def wbc_certificate(self, inst_begin: int = 0, count: int | None = None) -> dict:
        """Certificates of instances [inst_begin, inst_begin + count) from the last WBC call: the named fields of hunter_hip.h
        (r_eq, r_in, r_stat, r_dual, r_comp, n_active, eps, scale; [count] each, n_active as int) and dual [count][60]."""
        count = self.B - inst_begin if count is None else int(count)
        cert, dual = np.zeros((max(count, 0), 8)), np.zeros((max(count, 0), 60))
        self._check(self.lib.hb_wbc_get_certificate(self.ctx, C.c_int32(inst_begin), C.c_int32(count), _p(cert), _p(dual)),
                    "hb_wbc_get_certificate")
        out = {name: cert[:, k].copy() for k, name in enumerate(self.WBC_CERT_FIELDS)}
        out["n_active"] = out["n_active"].astype(np.int32)
        out["dual"] = dual
        return out

    # field order of hunter_hip.h's HB_HWBC_CERT_* (the certificate of one level of one instance)
    HWBC_CERT_FIELDS = ("res_own", "res_final", "r_hier", "r_in", "r_stat", "r_dual", "r_comp", "n_free", "n_active", "scale")

    def hwbc_set_certificate(self, enable: bool = True):
        """Per-level certificate of the HierarchicalWbc cascade on every later WBC call (hb_hwbc_set_certificate)."""
        self._check(self.lib.hb_hwbc_set_certificate(self.ctx, C.c_int32(1 if enable else 0)), "hb_hwbc_set_certificate")

    def hwbc_certificate(self, inst_begin: int = 0, count: int | None = None) -> dict:
        """Per-level certificates of instances [inst_begin, inst_begin + count) from the last WBC call: the named fields of hunter_hip.h
        (res_own, res_final, r_hier, r_in, r_stat, r_dual, r_comp, n_free, n_active, scale; [count][3] each, the two counts as int),
        cert [count][3][10] (the same, as one array), x_levels [count][3][38], slack0 [count][40] and dual [count][3][40]."""
        count = self.B - inst_begin if count is None else int(count)
        n = max(count, 0)
        cert, xl, s0, dual = np.zeros((n, 3, 10)), np.zeros((n, 3, 38)), np.zeros((n, 40)), np.zeros((n, 3, 40))
        self._check(self.lib.hb_hwbc_get_certificate(self.ctx, C.c_int32(inst_begin), C.c_int32(count), _p(cert), _p(xl), _p(s0), _p(dual)),
                    "hb_hwbc_get_certificate")
        out = {name: cert[:, :, k].copy() for k, name in enumerate(self.HWBC_CERT_FIELDS)}
        out["n_free"], out["n_active"] = out["n_free"].astype(np.int32), out["n_active"].astype(np.int32)
        out.update(cert=cert, x_levels=xl, slack0=s0, dual=dual)
        return out

    # field order of hunter_hip.h's HB_MPC_CERT_* (the certificate of one instance's stage QP)
    MPC_CERT_FIELDS = abi.MPC_CERT_FIELDS

    def mpc_certificate(self, inst_begin: int = 0, count: int | None = None) -> dict:
        """KKT certificate of the stage QP of the last MPC call for instances [inst_begin, inst_begin + count), computed on demand
        (hb_mpc_get_certificate): the named fields of hunter_hip.h (r_dyn, r_stat, obj, step_max, u_max, lambda_max, scale, n_nodes;
        [count] each, n_nodes as int; r_stat is read relative to scale), cert [count][8] (the same, as one array),
        costate [count][max_nodes+1][22] and u_til [count][max_nodes][12]."""
        count = self.B - inst_begin if count is None else int(count)
        n = max(count, 0)
        cert, costate, u_til = np.zeros((n, 8)), np.zeros((n, self.N + 1, 22)), np.zeros((n, self.N, 12))
        self._check(self.lib.hb_mpc_get_certificate(self.ctx, C.c_int32(inst_begin), C.c_int32(count), _p(cert), _p(costate), _p(u_til)),
                    "hb_mpc_get_certificate")
        out = {name: cert[:, k].copy() for k, name in enumerate(self.MPC_CERT_FIELDS)}
        out["n_nodes"] = out["n_nodes"].astype(np.int32)
        out.update(cert=cert, costate=costate, u_til=u_til)
        return out

    def mpc_lq(self, inst: int) -> dict:
        """The stage QP of instance `inst` as the last MPC call left it (hb_mpc_get_lq), dense and trimmed to its n intervals, in the
        OCP-QP layout: A [n][22][22], B [n][22][12], b [n][22], Q [n][22][22], P [n][12][22] (the cross term S), R [n][12][12],
        q [n][22], r [n][12], n_til [n] (projected inputs per stage; the columns behind them are padding)."""
        N = self.N
        out = dict(A=np.zeros((N, 22, 22)), B=np.zeros((N, 22, 12)), b=np.zeros((N, 22)), Q=np.zeros((N, 22, 22)), P=np.zeros((N, 12, 22)),
                   R=np.zeros((N, 12, 12)), q=np.zeros((N, 22)), r=np.zeros((N, 12)), n_til=np.zeros(N, dtype=np.int32))
        self._check(self.lib.hb_mpc_get_lq(self.ctx, C.c_int32(inst), *[_p(out[k]) for k in ("A", "B", "b", "Q", "P", "R", "q", "r", "n_til")]),
                    "hb_mpc_get_lq")
        n = int(np.count_nonzero(out["n_til"]))   # every stage has at least the six kernel coordinates
        return {k: v[:n].copy() for k, v in out.items()}

    RECOVERY_KEYS = ("Kx", "ke", "Z", "dF", "qf", "rf", "meta", "dt", "dq")

    def mpc_recovery(self, inst: int) -> dict:
        """The rest of the records of instance `inst` (hb_mpc_get_recovery), trimmed to its n intervals: what recovers the full input
        step du = T u~ + K dx + k (hunter_hip.h) and what the line search reads.  Kx [n][10][22], ke [n][10], Z [n][10][6], dF [n][12],
        qf [n][22], rf [n][22], meta [n][6] (n_f, n_z, mode, cost dt, dyn_sse dt, eq_sse dt), dt [n], dq [n][10]."""
        N = self.N
        out = dict(Kx=np.zeros((N, 10, 22)), ke=np.zeros((N, 10)), Z=np.zeros((N, 10, 6)), dF=np.zeros((N, 12)), qf=np.zeros((N, 22)),
                   rf=np.zeros((N, 22)), meta=np.zeros((N, 6)), dt=np.zeros(N), dq=np.zeros((N, 10)))
        self._check(self.lib.hb_mpc_get_recovery(self.ctx, C.c_int32(inst), *[_p(out[k]) for k in self.RECOVERY_KEYS]), "hb_mpc_get_recovery")
        n = int(np.count_nonzero(out["meta"][:, 0] + out["meta"][:, 1]))   # every stage has at least the six kernel coordinates
        return {k: v[:n].copy() for k, v in out.items()}

    LINESEARCH_KEYS = ("acc", "partial", "ls_tail", "ls_norm", "accepted", "ric_fail")

    def mpc_linesearch(self, inst_begin: int = 0, count: int | None = None) -> dict:
        """The state of the filter line search of the last SQP iteration of the last MPC call (hb_mpc_get_linesearch), read only, as the
        kernels left it: acc [count][4] (Armijo term, baseline merit, dyn_sse, eq_sse), partial [count][max_nodes][3] (per-node values at
        step size 1), ls_tail [count][16][max_nodes][3] (the same for the last evaluated window of the backtracking tail; hunter_hip.h says
        which rows are stale), ls_norm [count][2] (|dx|, |du|), accepted [count] (0 / 1 / 2 = stopped on deltaTol), ric_fail [count]."""
        count = self.B - inst_begin if count is None else int(count)
        n = max(count, 0)
        out = dict(acc=np.zeros((n, 4)), partial=np.zeros((n, self.N, 3)), ls_tail=np.zeros((n, abi.HB_LS_TAIL_MAX, self.N, 3)),
                   ls_norm=np.zeros((n, 2)), accepted=np.zeros(n, dtype=np.int32), ric_fail=np.zeros(n, dtype=np.int32))
        self._check(self.lib.hb_mpc_get_linesearch(self.ctx, C.c_int32(inst_begin), C.c_int32(count), *[_p(out[k]) for k in self.LINESEARCH_KEYS]),
                    "hb_mpc_get_linesearch")
        return out

    def mpc_linesearch_refused(self) -> int:
        """How many instances the last SQP iteration of the last MPC call handed to the backtracking tail (hb_mpc_get_linesearch_refused)."""
        n = C.c_int32(0)
        self._check(self.lib.hb_mpc_get_linesearch_refused(self.ctx, C.byref(n)), "hb_mpc_get_linesearch_refused")
        return int(n.value)

    def sync(self):
        self._check(self.lib.hb_sync(self.ctx), "hb_sync")

    def stats(self) -> dict:
        st = abi.HbStats()
        self._check(self.lib.hb_get_stats(self.ctx, C.byref(st)), "hb_get_stats")
        return {k: (list(getattr(st, k)) if k == "n_status" else getattr(st, k)) for k, _ in abi.HbStats._fields_}

    def input_cost(self):
        R = np.zeros((22, 22))
        self._check(self.lib.hb_get_input_cost(self.ctx, _p(R)), "hb_get_input_cost")
        return R

    # ---- reference generation on the device (SwitchedModelReferenceManager::modifyReferences) -----------------------
    def refgen_reset(self, rg_cfg: "abi.RefgenConfig", latest_stance=None):
        ls = None if latest_stance is None else _f64(latest_stance, (self.B, 4, 3))
        self._check(self.lib.hb_refgen_reset(self.ctx, C.byref(rg_cfg), _p(ls)), "hb_refgen_reset")

    def refgen_set_schedule(self, schedules, inst_begin: int = 0):
        """schedules: list of gait.ModeSchedule (event_times, modes), one per instance."""
        cnt = len(schedules)
        n_ev = np.array([len(s.event_times) for s in schedules], dtype=np.int32)
        if n_ev.max(initial=0) > abi.HB_MAX_EVENTS:
            raise ValueError("mode schedule longer than HB_MAX_EVENTS")
        ev = np.zeros((cnt, abi.HB_MAX_EVENTS))
        modes = np.full((cnt, abi.HB_MAX_EVENTS + 1), 3, dtype=np.int32)
        for i, s in enumerate(schedules):
            ev[i, :n_ev[i]] = s.event_times
            modes[i, :n_ev[i] + 1] = s.modes
        self._check(self.lib.hb_refgen_set_schedule(self.ctx, C.c_int32(inst_begin), C.c_int32(cnt), _p(n_ev), _p(ev), _p(modes)),
                    "hb_refgen_set_schedule")

    def refgen_update(self, t0, horizon, x_now, cmd_vel, want_status=True):
        """want_status=False: the enqueue-only form (no device synchronisation; status later through refgen_status()).
        With joint_ik in the configuration the horizon must stay below 3.3 s (22 joint-reference knots, one every 0.15 s): a longer
        one raises HunterHipError (HB_ERR_ARG), here and in tick_resident, instead of tables resampled onto fewer knots."""
        status = np.zeros(self.B, dtype=np.int32) if want_status else None
        x = None if x_now is None else _f64(x_now, (self.B, 22))
        self._check(self.lib.hb_refgen_update(self.ctx, _p(_f64(t0, (self.B,))), C.c_double(horizon), _p(x), _p(_f64(cmd_vel, (self.B, 4))),
                                              _p(status)), "hb_refgen_update")
        return status

    def refgen_status(self):
        status = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.hb_refgen_get_status(self.ctx, _p(status)), "hb_refgen_get_status")
        return status

    def refgen_schedule(self, inst_begin: int = 0, count: int | None = None):
        """The mode-schedule windows the last reference-generation pass read (hb_refgen_get_schedule) -> list of gait.ModeSchedule."""
        from .gait import ModeSchedule
        count = self.B - inst_begin if count is None else int(count)
        n = np.zeros(count, dtype=np.int32)
        ev, modes = np.zeros((count, abi.HB_MAX_EVENTS)), np.zeros((count, abi.HB_MAX_EVENTS + 1), dtype=np.int32)
        self._check(self.lib.hb_refgen_get_schedule(self.ctx, C.c_int32(inst_begin), C.c_int32(count), _p(n), _p(ev), _p(modes)), "hb_refgen_get_schedule")
        return [ModeSchedule(ev[i, :n[i]].tolist(), modes[i, :n[i] + 1].tolist()) for i in range(count)]

    # ---- device-resident gait manager (GaitSchedule + walkGait + the cmd_vel rate limiter per instance) -----------------
    def gait_reset(self, gait_cfg: "abi.HbGaitConfig", mask=None):
        """Enable the device gait manager and (re)initialise every instance, or those with mask[i] != 0 (hb_gait_reset)."""
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(self.B)
        self._check(self.lib.hb_gait_reset(self.ctx, C.byref(gait_cfg), _p(m)), "hb_gait_reset")

    def gait_disable(self):
        self._check(self.lib.hb_gait_disable(self.ctx), "hb_gait_disable")

    def gait_insert_template(self, switching_times, modes, start, final, inst_begin: int = 0):
        """insertModeSequenceTemplate(template, start[i], final[i]) for instances [inst_begin, inst_begin + len(start))."""
        sw, md = _f64(switching_times), _i32(modes)
        assert sw.ndim == 1 and md.shape == (sw.shape[0] - 1,)
        start = _f64(np.atleast_1d(start))
        final = _f64(np.broadcast_to(np.asarray(final, dtype=np.float64), start.shape))
        self._check(self.lib.hb_gait_insert_template(self.ctx, C.c_int32(inst_begin), C.c_int32(start.shape[0]), C.c_int32(sw.shape[0]), _p(sw), _p(md),
                                                     _p(start), _p(final)), "hb_gait_insert_template")

    def gait_state(self, inst_begin: int = 0, count: int | None = None) -> dict:
        """hb_gait_get_state: level, vel_abs, vel_avg, cmd [count][4] (filtered), the persistent schedule (n_events, event_times, modes) and
        status, per instance."""
        n = self.B - inst_begin if count is None else int(count)
        out = dict(level=np.zeros(n, dtype=np.int32), vel_abs=np.zeros(n), vel_avg=np.zeros(n), cmd=np.zeros((n, 4)),
                   n_events=np.zeros(n, dtype=np.int32), event_times=np.zeros((n, abi.HB_MAX_EVENTS)),
                   modes=np.zeros((n, abi.HB_MAX_EVENTS + 1), dtype=np.int32), status=np.zeros(n, dtype=np.int32))
        self._check(self.lib.hb_gait_get_state(self.ctx, C.c_int32(inst_begin), C.c_int32(n), *[_p(out[k]) for k in (
            "level", "vel_abs", "vel_avg", "cmd", "n_events", "event_times", "modes", "status")]), "hb_gait_get_state")
        return out

    def get_references(self):
        n = np.zeros(self.B, dtype=np.int32)
        t, mode = np.zeros((self.B, self.N + 1)), np.zeros((self.B, self.N), dtype=np.int32)
        x_ref, swing = np.zeros((self.B, self.N, 22)), np.zeros((self.B, self.N, 4, 6))
        self._check(self.lib.hb_mpc_get_references(self.ctx, C.c_int32(0), C.c_int32(self.B), _p(n), _p(t), _p(mode), _p(x_ref), _p(swing)),
                    "hb_mpc_get_references")
        return dict(n_nodes=n, t=t, mode=mode, x_ref=x_ref, swing=swing)

    # ---- state estimator (KalmanFilterEstimate, legged_estimation/src/LinearKalmanFilter.cpp) ------------------------
    def estimator_reset(self, est_cfg: "abi.HbEstimatorConfig", x_hat0=None):
        x0 = None if x_hat0 is None else _f64(x_hat0, (self.B, 18))
        self._est_cfg = est_cfg
        self._check(self.lib.hb_estimator_reset(self.ctx, C.byref(est_cfg), _p(x0)), "hb_estimator_reset")

    def estimator_update(self, dt, quat, ang_vel_local, lin_acc_local, joint_pos, joint_vel, contact_flag, to_resident=False,
                         want_outputs=True):
        """-> rbd[B][32], x_state[B][22] (what WbcBase::update and the MPC observation take).  want_outputs=False: the enqueue-only
        form (results stay on the device, no synchronisation) -> (None, None)."""
        rbd, x = (np.zeros((self.B, 32)), np.zeros((self.B, 22))) if want_outputs else (None, None)
        self._check(self.lib.hb_estimator_update(
            self.ctx, C.c_double(dt), _p(_f64(quat, (self.B, 4))), _p(_f64(ang_vel_local, (self.B, 3))),
            _p(_f64(lin_acc_local, (self.B, 3))), _p(_f64(joint_pos, (self.B, 10))), _p(_f64(joint_vel, (self.B, 10))),
            _p(_i32(contact_flag, (self.B, 4))), C.c_int32(1 if to_resident else 0), _p(rbd), _p(x)), "hb_estimator_update")
        return rbd, x

    def estimator_update_lcm(self, dt, low_state, contact_flag, to_resident=False):
        """hb_estimator_update_lcm: low_state[B][336] wire images of low_state_t -> rbd, x_state, timestamps."""
        rbd, x, ts = np.zeros((self.B, 32)), np.zeros((self.B, 22)), np.zeros(self.B, dtype=np.int64)
        wire = np.ascontiguousarray(low_state, dtype=np.uint8)
        assert wire.shape == (self.B, 336)
        self._check(self.lib.hb_estimator_update_lcm(self.ctx, C.c_double(dt), _p(wire), _p(_i32(contact_flag, (self.B, 4))),
                                                     C.c_int32(1 if to_resident else 0), _p(rbd), _p(x), _p(ts)), "hb_estimator_update_lcm")
        return rbd, x, ts

    def joint_command_lcm(self, gains: "abi.HbJointGains", dt, timestamp_ns: int):
        """hb_joint_command_lcm: the joint command of the last WBC result as low_cmd_t wire images [B][496]."""
        wire = np.zeros((self.B, 496), dtype=np.uint8)
        self._check(self.lib.hb_joint_command_lcm(self.ctx, C.byref(gains), C.c_double(dt), C.c_int64(timestamp_ns), _p(wire)), "hb_joint_command_lcm")
        return wire

    def estimator_contact_force(self, dt, joint_torque, rbd=None):
        """hb_estimator_contact_force (StateEstimateBase::estContactForce): -> estDisturbancetorque_ [B][16], estContactforce_ [B][16].
        rbd = None: the state the last estimator_update left on the device."""
        dist, cf = np.zeros((self.B, 16)), np.zeros((self.B, 16))
        self._check(self.lib.hb_estimator_contact_force(self.ctx, C.c_double(dt), _p(None if rbd is None else _f64(rbd, (self.B, 32))),
                                                        _p(_f64(joint_torque, (self.B, 10))), _p(dist), _p(cf)), "hb_estimator_contact_force")
        return dist, cf

    def estimator_filter(self):
        xh, P = np.zeros((self.B, 18)), np.zeros((self.B, 18, 18))
        self._check(self.lib.hb_estimator_get_filter(self.ctx, _p(xh), _p(P)), "hb_estimator_get_filter")
        return xh, P

    # ---- unit-level ---------------------------------------------------------------------------------
    def eval_flow_map(self, x, u, jac=False):
        x, u = _f64(np.atleast_2d(x)), _f64(np.atleast_2d(u))
        n = x.shape[0]
        f = np.zeros((n, 22))
        A = np.zeros((n, 22, 22)) if jac else None
        Bm = np.zeros((n, 22, 22)) if jac else None
        self._check(self.lib.hb_eval_flow_map(self.ctx, C.c_int32(n), _p(x), _p(u), _p(f), _p(A), _p(Bm)), "hb_eval_flow_map")
        return (f, A, Bm) if jac else f

    def eval_foot_kinematics(self, x, u):
        x, u = _f64(np.atleast_2d(x)), _f64(np.atleast_2d(u))
        n = x.shape[0]
        pos, vel = np.zeros((n, 4, 3)), np.zeros((n, 4, 3))
        self._check(self.lib.hb_eval_foot_kinematics(self.ctx, C.c_int32(n), _p(x), _p(u), _p(pos), _p(vel)), "hb_eval_foot_kinematics")
        return pos, vel

    def eval_rbd(self, rbd):
        rbd = _f64(np.atleast_2d(rbd))
        n = rbd.shape[0]
        M, nle, J, dJv = np.zeros((n, 16, 16)), np.zeros((n, 16)), np.zeros((n, 12, 16)), np.zeros((n, 12))
        self._check(self.lib.hb_eval_rbd(self.ctx, C.c_int32(n), _p(rbd), _p(M), _p(nle), _p(J), _p(dJv)), "hb_eval_rbd")
        return M, nle, J, dJv

    def centroidal_state_from_rbd(self, rbd):
        rbd = _f64(np.atleast_2d(rbd))
        x = np.zeros((rbd.shape[0], 22))
        self._check(self.lib.hb_centroidal_state_from_rbd(self.ctx, C.c_int32(rbd.shape[0]), _p(rbd), _p(x)), "hb_centroidal_state_from_rbd")
        return x

    def hoqp_solve(self, tasks_batch):
        """Generic hierarchical QP cascade (hb_hoqp_solve).  tasks_batch: list of problems, each a list (highest priority
        first) of dicts A, b, D, f with the same row counts per level across the batch.  -> x [P][L][n], slack list per
        level [P][m_in[l]], status [P]."""
        P, L = len(tasks_batch), len(tasks_batch[0])
        n = tasks_batch[0][0]["A"].shape[1]
        m_eq = np.array([tasks_batch[0][l]["A"].shape[0] for l in range(L)], dtype=np.int32)
        m_in = np.array([tasks_batch[0][l]["D"].shape[0] for l in range(L)], dtype=np.int32)
        A, D = np.zeros((P, 3, 8, 8)), np.zeros((P, 3, 8, 8))
        b, f = np.zeros((P, 3, 8)), np.zeros((P, 3, 8))
        for p, tasks in enumerate(tasks_batch):
            for l, t in enumerate(tasks):
                A[p, l, :m_eq[l], :n], b[p, l, :m_eq[l]] = t["A"], t["b"]
                D[p, l, :m_in[l], :n], f[p, l, :m_in[l]] = t["D"], t["f"]
        x, slack, status = np.zeros((P, 3, 8)), np.zeros((P, 3, 8)), np.zeros(P, dtype=np.int32)
        self._check(self.lib.hb_hoqp_solve(self.ctx, C.c_int32(P), C.c_int32(n), C.c_int32(L), _p(m_eq), _p(m_in), _p(A), _p(b), _p(D), _p(f),
                                           _p(x), _p(slack), _p(status)), "hb_hoqp_solve")
        return x[:, :L, :n], [slack[:, l, :m_in[l]] for l in range(L)], status

    def chunk_counters(self):
        out = np.zeros(4, dtype=np.int64)
        self._check(self.lib.hb_debug_chunk_counters(self.ctx, _p(out)), "hb_debug_chunk_counters")
        g = np.zeros(2, dtype=np.int64)
        self._check(self.lib.hb_debug_graph_state(self.ctx, _p(g)), "hb_debug_graph_state")
        return dict(graph_launches=int(out[0]), direct=int(out[1]), forks=int(out[2]), captures=int(out[3]),
                    capture_failures=int(g[0]), graphs_disabled=int(g[1]))

    def ik_solve(self, q16, leg, des_pos, R_des):
        """n independent InverseKinematics::computeIK problems on the device (hb_ik_solve) -> joint angles [n][5]."""
        q16, des_pos, R_des = _f64(np.atleast_2d(q16)), _f64(np.atleast_2d(des_pos)), _f64(np.asarray(R_des).reshape(-1, 9))
        leg = np.ascontiguousarray(np.atleast_1d(leg), dtype=np.int32)
        n = q16.shape[0]
        out = np.zeros((n, 5))
        self._check(self.lib.hb_ik_solve(self.ctx, C.c_int32(n), _p(q16), _p(leg), _p(des_pos), _p(R_des), _p(out)), "hb_ik_solve")
        return out

    def riccati_solve(self, A, Bm, b, Q, R, P, q, r, dx0):
        A, Bm, b, Q, R, P, q, r, dx0 = map(_f64, (A, Bm, b, Q, R, P, q, r, dx0))
        n, N, nu = A.shape[0], A.shape[1], Bm.shape[3]
        dx, du = np.zeros((n, N + 1, 22)), np.zeros((n, N, nu))
        self._check(self.lib.hb_riccati_solve(self.ctx, C.c_int32(n), C.c_int32(N), C.c_int32(nu), _p(A), _p(Bm), _p(b), _p(Q), _p(R),
                                              _p(P), _p(q), _p(r), _p(dx0), _p(dx), _p(du)), "hb_riccati_solve")
        return dx, du

    def riccati_gains(self, N, n_f, n_z, A, Bm, b, Q, R, P, q, r):
        """The gains of the backward sweep alone (hb_riccati_gains): N [n] stages per instance, n_f, n_z [n][max_nodes] widths per stage, stage
        data [n][max_nodes][...] padded to 12 inputs -> K [n][max_nodes][12][22], k [n][max_nodes][12], ric_fail [n].  Slots the sweep did not
        write hold abi.RIC_GAINS_SENTINEL_BITS."""
        N = _i32(np.atleast_1d(N))
        n, M = N.shape[0], self.N
        n_f, n_z = _i32(n_f, (n, M)), _i32(n_z, (n, M))
        A, Q = _f64(A, (n, M, 22, 22)), _f64(Q, (n, M, 22, 22))
        Bm, R, P = _f64(Bm, (n, M, 22, 12)), _f64(R, (n, M, 12, 12)), _f64(P, (n, M, 12, 22))
        b, q, r = _f64(b, (n, M, 22)), _f64(q, (n, M, 22)), _f64(r, (n, M, 12))
        K, k, fail = np.zeros((n, M, 12, 22)), np.zeros((n, M, 12)), np.zeros(n, dtype=np.int32)
        self._check(self.lib.hb_riccati_gains(self.ctx, C.c_int32(n), _p(N), _p(n_f), _p(n_z), _p(A), _p(Bm), _p(b), _p(Q), _p(R), _p(P), _p(q),
                                              _p(r), _p(K), _p(k), _p(fail)), "hb_riccati_gains")
        return K, k, fail
