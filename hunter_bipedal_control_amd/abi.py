"""ctypes mirror of include/hunter_hip.h (hb_model / hb_config / hb_stats) and builders from flattened params."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

NX, NU, NV, NJ, NC, NBODY, NWBC, NRBD, SWING_REF = 22, 22, 16, 10, 4, 11, 38, 32, 6
FLY, MODE_R, MODE_L, STANCE = 0, 1, 2, 3
HB_PAYLOAD_SIZE = 10   # hb_plant_set_model_variation: m_p, r[3], I_p[6] = xx xy xz yy yz zz
HB_PROFILE_MAX_KNOTS = 16   # hb_plant_set_terrain_profile, hb_ground_set_profile: knots per instance at most
HB_PROFILE_RECORD = 10      # hb_plant_get_terrain_profile: doubles per segment record, T row-major | d
HB_FIELD_MAX_NODES = 32     # hb_plant_set_terrain_field: nodes per grid axis at most (a facet record has HB_PROFILE_RECORD doubles too)


class HbModel(C.Structure):
    _fields_ = [
        ("parent", C.c_int32 * NJ),
        ("joint_origin", (C.c_double * 3) * NJ),
        ("joint_axis", (C.c_double * 3) * NJ),
        ("q_lower", C.c_double * NJ), ("q_upper", C.c_double * NJ),
        ("qd_limit", C.c_double * NJ), ("effort", C.c_double * NJ),
        ("mass", C.c_double * NBODY),
        ("com", (C.c_double * 3) * NBODY),
        ("inertia", (C.c_double * 6) * NBODY),
        ("contact_body", C.c_int32 * NC),
        ("contact_offset", (C.c_double * 3) * NC),
        ("gravity", C.c_double),
    ]


class HbConfig(C.Structure):
    _fields_ = [
        ("dt", C.c_double),
        ("sqp_iterations", C.c_int32), ("wbc_type", C.c_int32),
        ("g_max", C.c_double), ("g_min", C.c_double),
        ("alpha_decay", C.c_double), ("alpha_min", C.c_double), ("gamma_c", C.c_double), ("armijo_factor", C.c_double),
        ("Q_diag", C.c_double * NX),
        ("R_task_diag", C.c_double * 24),
        ("initial_state", C.c_double * NX),
        ("friction_mu", C.c_double), ("friction_reg", C.c_double), ("friction_gripper", C.c_double),
        ("friction_hess_shift", C.c_double),
        ("friction_barrier_mu", C.c_double), ("friction_barrier_delta", C.c_double),
        ("soft_swing_weight", C.c_double),
        ("pos_limit_barrier", C.c_double * 2), ("vel_limit_barrier", C.c_double * 2),
        ("force_limit_barrier", C.c_double * 2), ("force_limit", C.c_double * 2),
        ("position_error_gain", C.c_double),
        ("zero_vel_z_gain", C.c_double), ("zero_vel_z_offset", C.c_double),
        ("xy_ref_gain", C.c_double),
        ("torque_limits", C.c_double * 5),
        ("wbc_friction_mu", C.c_double),
        ("swing_kp", C.c_double), ("swing_kd", C.c_double),
        ("base_height_kp", C.c_double), ("base_height_kd", C.c_double),
        ("base_angular_kp", C.c_double), ("base_angular_kd", C.c_double),
        ("weight_swing_leg", C.c_double), ("weight_base_accel", C.c_double), ("weight_contact_force", C.c_double),
        ("wbc_eps_reg", C.c_double),
        ("wbc_max_iter", C.c_int32), ("reserved", C.c_int32),
        ("default_joint_state", C.c_double * NJ),
        ("delta_tol", C.c_double),
        ("wbc_reg_steps", C.c_int32), ("wbc_eps_mode", C.c_int32),
    ]


# Values of hb_config.reserved: hand-written mirror of csrc/hb_forms.hpp (there and in DESIGN.md 3.0: the meaning of every code; held together by
# tests/test_forms_host.py).  The stops of a kernel (profiling build) stand in code order, as the tools walk them: each includes the phases before it.
_LQ = dict(LQ_LOADS=10, LQ_LEG_VALUES=6, LQ_VALUE_PREPASS=7, LQ_DIRECTIONS=9, LQ_COMPOSE=1, LQ_FACTOR=2, LQ_SOLVES=3, LQ_DEFECT=30,
           LQ_B_COLUMNS=31, LQ_COST=4, LQ_SOFT_ROWS=5, LQ_Q=32, LQ_P=33, LQ_R=34)
_WBC = dict(WBC_A_BASE=13, WBC_A_LEGS=14, WBC_A_FINISH=15, WBC_A=11, WBC_B=12)
_RIC1 = dict(RIC1_STAGING=20, RIC1_GEMM1=21, RIC1_GEMM2=22, RIC1_FACTOR=23)    # k_ric_bwd
_RIC4 = dict(RIC4_STAGING=24, RIC4_GEMM1=25, RIC4_GEMM2=26, RIC4_FACTOR=27)    # k_ric_bwd4
_HWBC = dict(HWBC_LEVEL0=41, HWBC_KERNEL0=43, HWBC_QP1=44, HWBC_LEVEL1=42)
FORMS = dict(NONE=0, **_LQ, **_WBC, **_RIC1, **_RIC4, **_HWBC, RIC_BWD_ONE=101, RIC_BWD_FOUR=104, RIC_FWD_ROW=111, RIC_FWD_WAVE=114,
             LQT_ONE_RECORD=117, LQT_TRACE=118, LQT_PARK_NOTHING=119, LQT_VALUES_ONCE=125, LQT_VALUES=126, LQT_VALUES_FWD=127,
             LQT_VALUES_LEGS=128, LQ_ONE_NODE=129, LS_EVAL_NODE=151, RIC1_TRACE=197, WBC_TRACE=198, RIC4_TRACE=199)
FORM_RANGES = dict(LQ_TRIP_POW2=(120, 124), LQ_TRIP_LEN=(131, 146))   # LQ trips of 2^(value - first) / of value - first + 1 nodes
FORM = SimpleNamespace(**FORMS)
LQ_STOPS, WBC_STOPS, RIC1_STOPS, RIC4_STOPS, HWBC_STOPS = (tuple(d.values()) for d in (_LQ, _WBC, _RIC1, _RIC4, _HWBC))


class HbStats(C.Structure):
    _fields_ = [
        ("ms_lq", C.c_double), ("ms_riccati_bwd", C.c_double), ("ms_riccati_fwd", C.c_double),
        ("ms_linesearch", C.c_double), ("ms_mpc_total", C.c_double), ("ms_wbc", C.c_double),
        ("n_mpc_solves", C.c_int64), ("n_wbc_solves", C.c_int64),
        ("n_status", C.c_int32 * 4),
    ]


def _fill(arr, values):
    a = np.asarray(values)
    if a.ndim == 1:
        for i, v in enumerate(a):
            arr[i] = v.item()
    else:
        for i in range(a.shape[0]):
            for j in range(a.shape[1]):
                arr[i][j] = a[i, j].item()


def make_model(params: dict) -> HbModel:
    m = params["model"]
    out = HbModel()
    for name in ("parent", "joint_origin", "joint_axis", "q_lower", "q_upper", "qd_limit", "effort", "mass", "com",
                 "inertia", "contact_body", "contact_offset"):
        _fill(getattr(out, name), m[name])
    out.gravity = m["gravity"]
    return out


def make_config(params: dict, **overrides) -> HbConfig:
    c = params["config"]
    out = HbConfig()
    out.dt = c["dt"]
    out.sqp_iterations = c["sqp_iterations"]
    out.wbc_type = 0
    out.g_max, out.g_min = c["g_max"], c["g_min"]
    # OCS2 FilterLinesearch defaults
    out.alpha_decay, out.alpha_min, out.gamma_c, out.armijo_factor = 0.5, 1e-4, 1e-6, 1e-4
    _fill(out.Q_diag, c["Q_diag"])
    _fill(out.R_task_diag, c["R_task_diag"])
    _fill(out.initial_state, c["initial_state"])
    out.friction_mu = c["friction_mu"]
    # FrictionConeConstraint::Config defaults (FrictionConeConstraint.h:77-83)
    out.friction_reg, out.friction_gripper, out.friction_hess_shift = 25.0, 0.0, 1e-6
    out.friction_barrier_mu, out.friction_barrier_delta = c["friction_barrier_mu"], c["friction_barrier_delta"]
    out.soft_swing_weight = c["soft_swing_weight"]
    # LeggedInterface.cpp:337-339,352
    _fill(out.pos_limit_barrier, [1.0, 0.1])
    _fill(out.vel_limit_barrier, [1.0, 0.1])
    _fill(out.force_limit_barrier, [0.1, 1.0])
    _fill(out.force_limit, [0.0, 350.0])
    out.position_error_gain = c["position_error_gain"]
    # LeggedInterface.cpp:436-444: Ax(2,2) = 3, b(2) = -3*0.02
    out.zero_vel_z_gain, out.zero_vel_z_offset = 3.0, -0.06
    out.xy_ref_gain = 3.0  # LeggedRobotPreComputation.cpp:113-116
    _fill(out.torque_limits, c["torque_limits"])
    out.wbc_friction_mu = c["wbc_friction_mu"]
    out.swing_kp, out.swing_kd = c["swing_kp"], c["swing_kd"]
    out.base_height_kp, out.base_height_kd = c["base_height_kp"], c["base_height_kd"]
    out.base_angular_kp, out.base_angular_kd = c["base_angular_kp"], c["base_angular_kd"]
    out.weight_swing_leg, out.weight_base_accel = c["weight_swing_leg"], c["weight_base_accel"]
    out.weight_contact_force = c["weight_contact_force"]
    out.wbc_eps_reg = 1e-8    # the regularised-minimiser rule (why not qpOASES's 5e3 * EPS, with measurements)
    out.wbc_max_iter = 120
    _fill(out.default_joint_state, c["default_joint_state"])
    out.delta_tol = c["delta_tol"]
    out.wbc_reg_steps = 1     # qpOASES setToMPC(): numRegularisationSteps = 1 (WeightedWbc.cpp:47-48, HoQp.cpp:175-176)
    for k, v in overrides.items():
        if isinstance(v, (list, tuple)):
            _fill(getattr(out, k), v)
        else:
            setattr(out, k, v)
    return out


class HbEstimatorConfig(C.Structure):
    _fields_ = [(k, C.c_double) for k in (
        "foot_radius", "imu_process_noise_position", "imu_process_noise_velocity", "foot_process_noise_position",
        "foot_sensor_noise_position", "foot_sensor_noise_velocity", "foot_height_sensor_noise",
        "contact_force_cutoff_frequency", "contact_threshold")]


def make_estimator_config(params: dict, **overrides) -> HbEstimatorConfig:
    out = HbEstimatorConfig()
    for k, _ in HbEstimatorConfig._fields_:
        setattr(out, k, overrides.get(k, params["config"]["kalman"][k]))
    return out


class HbSensorConfig(C.Structure):
    """hb_sensor_config (include/hunter_hip.h): noise of the plant's sensor model, hb_plant_set_sensor_model."""
    _fields_ = [(k, C.c_double) for k in ("orientation_noise", "gyro_noise", "accel_noise", "joint_pos_noise", "joint_vel_noise",
                                          "joint_torque_noise")] + [("seed", C.c_uint64), ("instance_offset", C.c_uint32),
                                                                    ("reserved", C.c_int32)]


def make_sensor_config(seed: int = 0, instance_offset: int = 0, **sigmas) -> HbSensorConfig:
    """Standard deviations by channel name (orientation_noise [rad], gyro_noise, accel_noise, joint_pos_noise, joint_vel_noise,
    joint_torque_noise; default 0 = ideal channel), the 64-bit seed and the global index of the context's instance 0."""
    out = HbSensorConfig()
    names = [k for k, _ in HbSensorConfig._fields_[:6]]
    for k, v in sigmas.items():
        if k not in names:
            raise TypeError(f"make_sensor_config: unknown channel {k!r} (one of {names})")
        setattr(out, k, float(v))
    out.seed, out.instance_offset, out.reserved = int(seed) & 0xFFFFFFFFFFFFFFFF, int(instance_offset), 0
    return out


class HbContactConfig(C.Structure):
    """hb_contact_config (include/hunter_hip.h): contact model of the plant, hb_plant_set_contact_model."""
    _fields_ = [("mode", C.c_int32), ("sweeps", C.c_int32), ("mu", C.c_double), ("ground_z", C.c_double), ("erp", C.c_double),
                ("tol", C.c_double), ("fall_height", C.c_double), ("reserved", C.c_int32 * 2)]


HB_CONTACT_NONFINITE, HB_CONTACT_FALLEN, HB_CONTACT_UNCONVERGED = 1, 2, 4
# Default sweep count of make_contact_config, from the residual decay of the numpy twin of the definition (with
# the table): standing levels off at 1e-8 m/s by 20 sweeps, landing by 30, a tilted start under random torques reaches 1e-8 at 30; a foot
# sliding under a push is still at 5e-6 there and decays slowly.  Convergence is NOT promised: HB_CONTACT_UNCONVERGED reports the
# residual of every step against `tol`.
CONTACT_DEFAULT_SWEEPS = 30


def make_contact_config(params: dict, **overrides) -> HbContactConfig:
    """The ground-contact model (mode 1) with mu = frictionCoefficient of the task file, ground at z = 0, erp 0.2, 30 sweeps, residual
    tolerance 1e-3 m/s and no fall detection; any field by name overrides."""
    d = dict(mode=1, sweeps=CONTACT_DEFAULT_SWEEPS, mu=params["config"]["friction_mu"], ground_z=0.0, erp=0.2, tol=1e-3, fall_height=0.0)
    for k in overrides:
        if k not in d:
            raise TypeError(f"make_contact_config: unknown field {k!r} (one of {sorted(d)})")
    d.update(overrides)
    out = HbContactConfig()
    out.mode, out.sweeps = int(d["mode"]), int(d["sweeps"])
    for k in ("mu", "ground_z", "erp", "tol", "fall_height"):
        setattr(out, k, float(d[k]))
    return out


class HbJointModel(C.Structure):
    """hb_joint_model (include/hunter_hip.h): joint model of the ground-contact plant, hb_plant_set_joint_model."""
    _fields_ = [(k, C.c_double * NJ) for k in ("armature", "damping", "frictionloss", "lower", "upper", "torque_limit")] + [
        ("limit_erp", C.c_double), ("tol", C.c_double), ("limits", C.c_int32), ("reserved", C.c_int32)]


HB_JOINT_UNCONVERGED = 1 << 30


def make_joint_model(params: dict, **overrides) -> HbJointModel:
    """The joints of the reference's MuJoCo model: armature 0.1 kg m^2 and damping 1 N m s/rad (mujoco/model/hunter/hunter.xml:6),
    frictionloss 0.2 N m and the ranges (hunter.xml:59-124; the ranges are params["model"]["q_lower"] / ["q_upper"], the same numbers
    as hunter.urdf:93-556), torque limit 100 N m (ctrlrange of every motor, hunter.xml:25), stops on (limits = 1), limit_erp 0.2,
    joint-residual tolerance 1e-3 rad/s.  Any field by name overrides; a per-joint field takes a scalar or ten values.

    The URDF's `effort` of 23.7 N m (params["model"]["effort"]) is NOT the default: it lies below the WBC's own torque rows of 28 / 60
    N m (task.info torqueLimitsTask), so a plant saturating there clips torques the controller considers admissible.  It is a choice by
    override: make_joint_model(params, torque_limit=params["model"]["effort"])."""
    m = params["model"]
    d = dict(armature=0.1, damping=1.0, frictionloss=0.2, lower=m["q_lower"], upper=m["q_upper"], torque_limit=100.0, limit_erp=0.2,
             tol=1e-3, limits=1)
    for k in overrides:
        if k not in d:
            raise TypeError(f"make_joint_model: unknown field {k!r} (one of {sorted(d)})")
    d.update(overrides)
    out = HbJointModel()
    for k in ("armature", "damping", "frictionloss", "lower", "upper", "torque_limit"):
        _fill(getattr(out, k), np.broadcast_to(np.asarray(d[k], dtype=float), (NJ,)))
    out.limit_erp, out.tol, out.limits, out.reserved = float(d["limit_erp"]), float(d["tol"]), int(d["limits"]), 0
    return out


class HbEpisodeConfig(C.Structure):
    """hb_episode_config (include/hunter_hip.h): per-instance episode record of the plant and stop-on-fall, hb_plant_set_episode."""
    _fields_ = [("slip_speed", C.c_double), ("tilt_limit", C.c_double), ("stop_on_fall", C.c_int32), ("trace_every", C.c_int32),
                ("trace_capacity", C.c_int32), ("reserved", C.c_int32 * 3)]


HB_EP_RUNNING, HB_EP_FALLEN, HB_EP_NONFINITE = 0, 1, 2
HB_EP_TRACE_W, HB_EP_TRACE_MAX = 8, 4096
# The fields of the two records, (name, first index, length), in the order of the HB_EP_I_* / HB_EP_D_* indices of the header; the trace
# sample's columns.
EPISODE_INT_FIELDS = (("STEPS", 0, 1), ("TICKS", 1, 1), ("END_TICK", 2, 1), ("END_CAUSE", 3, 1), ("FIRST_NONFINITE", 4, 1), ("N_TRACE", 5, 1),
                      ("WBC_STATUS_OR", 6, 1), ("WBC_FAIL_TICKS", 7, 1), ("FIRST_WBC_FAIL", 8, 1), ("CONTACT_TICKS", 9, 4), ("TOUCHDOWNS", 13, 4),
                      ("PREV_TOUCHING", 17, 4), ("SLIP_TICKS", 21, 1), ("FIRST_SLIP", 22, 1), ("UNCONVERGED_TICKS", 23, 1),
                      ("CONTACT_STATUS_OR", 24, 1), ("JOINT_STATUS_OR", 25, 1), ("CLAMP_TICKS", 26, 1), ("STOP_TICKS", 27, 1))
EPISODE_DOUBLE_FIELDS = (("START_POS", 0, 3), ("LAST_BASE", 3, 6), ("HEIGHT_LAST", 9, 1), ("HEIGHT_MIN", 10, 1), ("HEIGHT_MAX", 11, 1),
                         ("TILT_MAX", 12, 1), ("TAU_MAX", 13, 10), ("WORK_ABS", 23, 1), ("WORK_NET", 24, 1), ("GAP_MIN", 25, 1), ("FN_MAX", 26, 4),
                         ("SLIP_SPEED_MAX", 30, 1), ("RES_MAX", 31, 1), ("JRES_MAX", 32, 1))
HB_EP_NI, HB_EP_ND = 28, 33
EPISODE_TRACE_COLUMNS = ("tick", "x", "y", "height", "yaw", "pitch", "roll", "n_touching")


def make_episode_config(**fields) -> HbEpisodeConfig:
    """slip_speed 0.05 m/s, no tilt limit, no stop on a fall, no trace; any field by name overrides."""
    d = dict(slip_speed=0.05, tilt_limit=0.0, stop_on_fall=0, trace_every=0, trace_capacity=0)
    for k in fields:
        if k not in d:
            raise TypeError(f"make_episode_config: unknown field {k!r} (one of {sorted(d)})")
    d.update(fields)
    out = HbEpisodeConfig()
    out.slip_speed, out.tilt_limit = float(d["slip_speed"]), float(d["tilt_limit"])
    out.stop_on_fall, out.trace_every, out.trace_capacity = int(d["stop_on_fall"]), int(d["trace_every"]), int(d["trace_capacity"])
    return out


def split_episode_record(irec, drec) -> dict:
    """irec[B][HB_EP_NI], drec[B][HB_EP_ND] -> dict of named arrays ([B] for a scalar field, [B][n] otherwise)."""
    out = {}
    for table, rec in ((EPISODE_INT_FIELDS, irec), (EPISODE_DOUBLE_FIELDS, drec)):
        for name, at, n in table:
            out[name] = rec[:, at].copy() if n == 1 else rec[:, at:at + n].copy()
    return out


class HbRespawnConfig(C.Structure):
    """hb_respawn_config (include/hunter_hip.h): respawn of ended instances, hb_plant_set_respawn."""
    _fields_ = [("clearance", C.c_double), ("yaw_range", C.c_double), ("joint_pos_sigma", C.c_double), ("base_vel_sigma", C.c_double),
                ("seed", C.c_uint64), ("instance_offset", C.c_uint32), ("hold_ticks", C.c_int32), ("max_ticks", C.c_int32),
                ("place", C.c_int32), ("reserved", C.c_int32 * 2)]


HB_RS_TIMEOUT, HB_RS_STREAM = 3, 0x52535031
# The totals, (name, index), in the order of the HB_RS_I_* / HB_RS_D_* indices of the header.
RESPAWN_INT_FIELDS = ("EPISODES", "N_FALLEN", "N_NONFINITE", "N_TIMEOUT", "TICKS_SUM", "TICKS_MIN", "TICKS_MAX", "SLIP_TICKS_SUM",
                      "WBC_FAIL_TICKS_SUM", "LAST_CAUSE", "LAST_TICKS", "EPISODE_INDEX", "STEPS_SUM")
RESPAWN_DOUBLE_FIELDS = ("DIST_X_SUM", "DIST_Y_SUM", "WORK_ABS_SUM", "TILT_MAX", "TAU_MAX")
HB_RS_NI, HB_RS_ND = len(RESPAWN_INT_FIELDS), len(RESPAWN_DOUBLE_FIELDS)


def make_respawn_config(**fields) -> HbRespawnConfig:
    """No hold, no time-out, no placement, no perturbation, seed 0; any field by name overrides."""
    d = dict(clearance=0.0, yaw_range=0.0, joint_pos_sigma=0.0, base_vel_sigma=0.0, seed=0, instance_offset=0, hold_ticks=0, max_ticks=0,
             place=0)
    for k in fields:
        if k not in d:
            raise TypeError(f"make_respawn_config: unknown field {k!r} (one of {sorted(d)})")
    d.update(fields)
    out = HbRespawnConfig()
    for k in ("clearance", "yaw_range", "joint_pos_sigma", "base_vel_sigma"):
        setattr(out, k, float(d[k]))
    for k in ("seed", "instance_offset", "hold_ticks", "max_ticks", "place"):
        setattr(out, k, int(d[k]))
    return out


def split_respawn_totals(itot, dtot) -> dict:
    """itot[B][HB_RS_NI], dtot[B][HB_RS_ND] -> dict of [B] arrays keyed by field name."""
    out = {name: itot[:, k].copy() for k, name in enumerate(RESPAWN_INT_FIELDS)}
    out.update({name: dtot[:, k].copy() for k, name in enumerate(RESPAWN_DOUBLE_FIELDS)})
    return out


class HbScenarioConfig(C.Structure):
    """hb_scenario_config (include/hunter_hip.h): scenario draw at respawn, hb_plant_set_scenario."""
    _fields_ = [("seed", C.c_uint64), ("channels", C.c_int32), ("mu_per_point", C.c_int32), ("grade_max", C.c_double), ("mu_lo", C.c_double),
                ("mu_hi", C.c_double), ("payload_mass_max", C.c_double), ("payload_center", C.c_double * 3),
                ("payload_half_extent", C.c_double * 3), ("mass_scale_range", C.c_double), ("push_force_max", C.c_double),
                ("push_start_lo", C.c_int32), ("push_start_hi", C.c_int32), ("push_ticks", C.c_int32), ("log_capacity", C.c_int32),
                ("reserved", C.c_int32 * 2)]


HB_SC_STREAM = 0x53434E31
HB_SC_SLOPE, HB_SC_MU, HB_SC_PAYLOAD, HB_SC_MASS, HB_SC_PUSH = 1, 2, 4, 8, 16
HB_SC_ALL = HB_SC_SLOPE | HB_SC_MU | HB_SC_PAYLOAD | HB_SC_MASS | HB_SC_PUSH
# scen[HB_SC_N], (name, first index, count), in the order of the HB_SC_* indices of the header.
SCENARIO_FIELDS = (("GRADE", 0, 2), ("MUS", 2, 4), ("PAYLOAD_M", 6, 1), ("PAYLOAD_R", 7, 3), ("SCALE", 10, 11), ("PUSH_START", 21, 1), ("PUSH_F", 22, 2))
HB_SC_N = 24
# a log row: these six, then the HB_SC_N parameters
SCENARIO_LOG_HEAD = ("EPISODE", "CAUSE", "TICKS", "DIST_X", "DIST_Y", "TILT_MAX")
HB_SC_LOG_W, HB_SC_LOG_MAX = len(SCENARIO_LOG_HEAD) + HB_SC_N, 1024


def make_scenario_config(**fields) -> HbScenarioConfig:
    """No channel, no log, seed 0, mu in [0, 0], push_ticks 0; any field by name overrides (payload_center / payload_half_extent: 3 values)."""
    d = dict(seed=0, channels=0, mu_per_point=0, grade_max=0.0, mu_lo=0.0, mu_hi=0.0, payload_mass_max=0.0, payload_center=(0.0, 0.0, 0.0),
             payload_half_extent=(0.0, 0.0, 0.0), mass_scale_range=0.0, push_force_max=0.0, push_start_lo=0, push_start_hi=0, push_ticks=0,
             log_capacity=0)
    for k in fields:
        if k not in d:
            raise TypeError(f"make_scenario_config: unknown field {k!r} (one of {sorted(d)})")
    d.update(fields)
    out = HbScenarioConfig()
    for k in ("grade_max", "mu_lo", "mu_hi", "payload_mass_max", "mass_scale_range", "push_force_max"):
        setattr(out, k, float(d[k]))
    for k in ("seed", "channels", "mu_per_point", "push_start_lo", "push_start_hi", "push_ticks", "log_capacity"):
        setattr(out, k, int(d[k]))
    for k in ("payload_center", "payload_half_extent"):
        for a in range(3):
            getattr(out, k)[a] = float(d[k][a])
    return out


def split_scenario(scen) -> dict:
    """scen[...][HB_SC_N] -> dict of [...] / [...][n] arrays keyed by field name."""
    scen = np.asarray(scen)
    return {name: (scen[..., at].copy() if n == 1 else scen[..., at:at + n].copy()) for name, at, n in SCENARIO_FIELDS}


class HbProfileDrawConfig(C.Structure):
    """hb_profile_draw_config (include/hunter_hip.h): profile draw at respawn, hb_plant_set_profile_draw."""
    _fields_ = [("seed", C.c_uint64), ("kinds", C.c_int32), ("mu_per_point", C.c_int32), ("dir", C.c_double * 2), ("height_lo", C.c_double),
                ("height_hi", C.c_double), ("at_lo", C.c_double), ("at_hi", C.c_double), ("riser_slope", C.c_double), ("steps_lo", C.c_int32),
                ("steps_hi", C.c_int32), ("run_lo", C.c_double), ("run_hi", C.c_double), ("mu_lo", C.c_double), ("mu_hi", C.c_double),
                ("follow_map", C.c_int32), ("log_capacity", C.c_int32), ("reserved", C.c_int32 * 2)]


HB_PD_STREAM = 0x50444431
HB_PD_FLAT, HB_PD_CURB, HB_PD_STAIRS = 1, 2, 4
HB_PD_ALL = HB_PD_FLAT | HB_PD_CURB | HB_PD_STAIRS
# row[HB_PD_N], (name, first index, count), in the order of the HB_PD_* indices of the header.
PROFILE_DRAW_FIELDS = (("KIND", 0, 1), ("HEIGHT", 1, 1), ("AT", 2, 1), ("STEPS", 3, 1), ("RUN", 4, 1), ("MUS", 5, 4))
HB_PD_N = 9
# a log row: these five, then the HB_PD_N parameters
PROFILE_DRAW_LOG_HEAD = ("EPISODE", "CAUSE", "TICKS", "PROGRESS", "TILT_MAX")
HB_PD_LOG_W, HB_PD_LOG_MAX = len(PROFILE_DRAW_LOG_HEAD) + HB_PD_N, 1024


def make_profile_draw_config(**fields) -> HbProfileDrawConfig:
    """Level ground only along x, risers of slope 1.7 one metre ahead, one step of run 0.3 m, mu in [0, 0], no map, no log, seed 0; any
    field by name overrides (dir: 2 values)."""
    d = dict(seed=0, kinds=HB_PD_FLAT, mu_per_point=0, dir=(1.0, 0.0), height_lo=0.0, height_hi=0.0, at_lo=1.0, at_hi=1.0, riser_slope=1.7,
             steps_lo=1, steps_hi=1, run_lo=0.3, run_hi=0.3, mu_lo=0.0, mu_hi=0.0, follow_map=0, log_capacity=0)
    for k in fields:
        if k not in d:
            raise TypeError(f"make_profile_draw_config: unknown field {k!r} (one of {sorted(d)})")
    d.update(fields)
    out = HbProfileDrawConfig()
    for k in ("height_lo", "height_hi", "at_lo", "at_hi", "riser_slope", "run_lo", "run_hi", "mu_lo", "mu_hi"):
        setattr(out, k, float(d[k]))
    for k in ("seed", "kinds", "mu_per_point", "steps_lo", "steps_hi", "follow_map", "log_capacity"):
        setattr(out, k, int(d[k]))
    out.dir[0], out.dir[1] = float(d["dir"][0]), float(d["dir"][1])
    return out


def split_profile_draw(row) -> dict:
    """row[...][HB_PD_N] -> dict of [...] / [...][n] arrays keyed by field name."""
    row = np.asarray(row)
    return {name: (row[..., at].copy() if n == 1 else row[..., at:at + n].copy()) for name, at, n in PROFILE_DRAW_FIELDS}


class HbFieldDrawConfig(C.Structure):
    """hb_field_draw_config (include/hunter_hip.h): field draw at respawn, hb_plant_set_field_draw."""
    _fields_ = [("seed", C.c_uint64), ("kinds", C.c_int32), ("mu_per_point", C.c_int32), ("dir", C.c_double * 2), ("n_nodes", C.c_int32 * 2),
                ("spacing", C.c_double * 2), ("centre", C.c_double * 2), ("calm", C.c_double), ("amp_lo", C.c_double), ("amp_hi", C.c_double),
                ("slope_u_lo", C.c_double), ("slope_u_hi", C.c_double), ("slope_w_lo", C.c_double), ("slope_w_hi", C.c_double),
                ("mu_lo", C.c_double), ("mu_hi", C.c_double), ("follow_map", C.c_int32), ("log_capacity", C.c_int32), ("reserved", C.c_int32 * 2)]


HB_FD_STREAM = 0x46444431
HB_FD_FLAT, HB_FD_ROUGH, HB_FD_TILT, HB_FD_TILT_ROUGH = 1, 2, 4, 8
HB_FD_ALL = HB_FD_FLAT | HB_FD_ROUGH | HB_FD_TILT | HB_FD_TILT_ROUGH
# row[HB_FD_N], (name, first index, count), in the order of the HB_FD_* indices of the header.
FIELD_DRAW_FIELDS = (("KIND", 0, 1), ("AMPLITUDE", 1, 1), ("SLOPE_U", 2, 1), ("SLOPE_W", 3, 1), ("MUS", 4, 4))
HB_FD_N = 8
# a log row: the profile draw's five leading entries, then the HB_FD_N parameters
FIELD_DRAW_LOG_HEAD = PROFILE_DRAW_LOG_HEAD
HB_FD_LOG_W, HB_FD_LOG_MAX = len(FIELD_DRAW_LOG_HEAD) + HB_FD_N, 1024


def make_field_draw_config(**fields) -> HbFieldDrawConfig:
    """Level ground only: a 32 x 32 grid along x with 0.1 m spacing and the spawn point at its middle, no bumps, no tilt, mu in [0, 0], no
    map, no log, seed 0; any field by name overrides (dir, n_nodes, spacing, centre: 2 values each; centre None: the middle of the grid)."""
    d = dict(seed=0, kinds=HB_FD_FLAT, mu_per_point=0, dir=(1.0, 0.0), n_nodes=(HB_FIELD_MAX_NODES, HB_FIELD_MAX_NODES), spacing=(0.1, 0.1),
             centre=None, calm=0.0, amp_lo=0.0, amp_hi=0.0, slope_u_lo=0.0, slope_u_hi=0.0, slope_w_lo=0.0, slope_w_hi=0.0, mu_lo=0.0, mu_hi=0.0,
             follow_map=0, log_capacity=0)
    for k in fields:
        if k not in d:
            raise TypeError(f"make_field_draw_config: unknown field {k!r} (one of {sorted(d)})")
    d.update(fields)
    out = HbFieldDrawConfig()
    for k in ("calm", "amp_lo", "amp_hi", "slope_u_lo", "slope_u_hi", "slope_w_lo", "slope_w_hi", "mu_lo", "mu_hi"):
        setattr(out, k, float(d[k]))
    for k in ("seed", "kinds", "mu_per_point", "follow_map", "log_capacity"):
        setattr(out, k, int(d[k]))
    for j in (0, 1):
        out.dir[j], out.n_nodes[j], out.spacing[j] = float(d["dir"][j]), int(d["n_nodes"][j]), float(d["spacing"][j])
        out.centre[j] = 0.5 * float(out.n_nodes[j] - 1) * out.spacing[j] if d["centre"] is None else float(d["centre"][j])
    return out


def split_field_draw(row) -> dict:
    """row[...][HB_FD_N] -> dict of [...] / [...][n] arrays keyed by field name."""
    row = np.asarray(row)
    return {name: (row[..., at].copy() if n == 1 else row[..., at:at + n].copy()) for name, at, n in FIELD_DRAW_FIELDS}


class HbHeightScanConfig(C.Structure):
    """hb_height_scan_config (include/hunter_hip.h): the controller's field map perceived from the plant's ground, hb_plant_set_height_scan."""
    _fields_ = [("n_nodes", C.c_int32 * 2), ("back", C.c_int32 * 2), ("dir", C.c_double * 2), ("spacing", C.c_double * 2), ("range", C.c_double),
                ("noise", C.c_double), ("dropout", C.c_double), ("register_mode", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64),
                ("instance_offset", C.c_uint32), ("pad", C.c_int32)]


HB_HS_STREAM = 0x48535331


def make_height_scan_config(**fields) -> HbHeightScanConfig:
    """An ideal sensor: a 32 x 32 grid along x with 0.1 m spacing, the registration point in its middle cell (back None: (n - 1) // 2), no
    range limit, no noise, no dropout, registered with the plant's position, seed 0; any field by name overrides (n_nodes, back, dir,
    spacing: 2 values each)."""
    d = dict(n_nodes=(HB_FIELD_MAX_NODES, HB_FIELD_MAX_NODES), back=None, dir=(1.0, 0.0), spacing=(0.1, 0.1), range=0.0, noise=0.0, dropout=0.0,
             register_mode=0, reserved=0, seed=0, instance_offset=0, pad=0)
    for k in fields:
        if k not in d:
            raise TypeError(f"make_height_scan_config: unknown field {k!r} (one of {sorted(d)})")
    d.update(fields)
    out = HbHeightScanConfig()
    for k in ("range", "noise", "dropout"):
        setattr(out, k, float(d[k]))
    for k in ("register_mode", "reserved", "seed", "instance_offset", "pad"):
        setattr(out, k, int(d[k]))
    for j in (0, 1):
        out.n_nodes[j], out.dir[j], out.spacing[j] = int(d["n_nodes"][j]), float(d["dir"][j]), float(d["spacing"][j])
        out.back[j] = (out.n_nodes[j] - 1) // 2 if d["back"] is None else int(d["back"][j])
    return out


HB_FOOTHOLD_MAX_SHIFT = 8   # hb_ground_set_foothold: candidates to either side of the nominal foothold at most
HB_NO_FOOTHOLD = -2 ** 31   # hb_ground_get_foothold_choice: the shift of a foot the pass planned no foothold for


class HbFootholdConfig(C.Structure):
    """hb_foothold_config (include/hunter_hip.h): the planner's foothold mode on the ground map, hb_ground_set_foothold."""
    _fields_ = [("mode", C.c_int32), ("n_shift", C.c_int32), ("shift_step", C.c_double), ("flat_tol", C.c_double)]


FOOTHOLD_MODES = {"point": 0, "sole": 1}


def make_foothold_config(mode, n_shift=3, shift_step=0.02, flat_tol=0.005) -> HbFootholdConfig:
    """mode (always given by the caller): 0 / "point" (per contact point) or 1 / "sole"; the other defaults are placeholders nobody has
    measured."""
    out = HbFootholdConfig()
    out.mode = FOOTHOLD_MODES[mode] if isinstance(mode, str) else int(mode)
    out.n_shift, out.shift_step, out.flat_tol = int(n_shift), float(shift_step), float(flat_tol)
    return out


class HbJointGains(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("kp_big_stance", "kp_big_swing", "kd_big", "kp_small_stance", "kp_small_swing", "kd_small",
                                          "kd_feet", "kp_position", "kd_position")]


def make_joint_gains(**overrides) -> HbJointGains:
    """Defaults of legged_controllers/cfg/Tutorials.cfg:6-16 (dynamic_reconfigure)."""
    d = dict(kp_big_stance=40.0, kp_big_swing=30.0, kd_big=2.0, kp_small_stance=30.0, kp_small_swing=20.0, kd_small=2.0, kd_feet=0.01,
             kp_position=10.0, kd_position=3.0)
    d.update(overrides)
    out = HbJointGains()
    for k, v in d.items():
        setattr(out, k, v)
    return out


def hybrid_gains(gains: HbJointGains, stance=(True, True)):
    """-> (kp[10], kd[10]) by joint, as k_joint_command assigns them with the controller loaded (LeggedController.cpp:222-244): joints 0, 1
    and 4 of a leg take the small gains (4: kd_feet), 2 and 3 the big ones; stance[leg] selects the stance or the swing kp."""
    kp, kd = np.zeros(NJ), np.zeros(NJ)
    for j in range(NJ):
        k, on = j % 5, bool(stance[j // 5])
        small = k in (0, 1, 4)
        kp[j] = (gains.kp_small_stance if on else gains.kp_small_swing) if small else (gains.kp_big_stance if on else gains.kp_big_swing)
        kd[j] = gains.kd_feet if k == 4 else (gains.kd_small if small else gains.kd_big)
    return kp, kd


HB_MAX_EVENTS = 64
# field order of hunter_hip.h's HB_MPC_CERT_* (HunterSolver.mpc_certificate)
MPC_CERT_FIELDS = ("r_dyn", "r_stat", "obj", "step_max", "u_max", "lambda_max", "scale", "n_nodes")
RIC_GAINS_SENTINEL_BITS = 0x7ff85e471e100001   # HB_RIC_GAINS_SENTINEL_BITS: what hb_riccati_gains leaves in a gain slot the sweep did not write
HB_LS_TAIL_MAX = 16  # step sizes one window of the backtracking tail evaluates side by side (hb_mpc_get_linesearch: ls_tail rows)
# hb_status / per-instance status words (include/hunter_hip.h)
HB_OK, HB_ERR_ARG, HB_ERR_DEVICE, HB_ERR_STATE, HB_ERR_NO_GPU = 0, -1, -2, -3, -4
HB_INST_OK, HB_INST_MAXITER, HB_INST_INFEASIBLE, HB_INST_NAN = 0, 1, 2, 3


class RefgenConfig(C.Structure):
    """hb_refgen_config (include/hunter_hip.h)."""
    _fields_ = [("dt", C.c_double), ("com_height", C.c_double), ("next_position_z", C.c_double), ("swing_height", C.c_double),
                ("swing_time_scale", C.c_double), ("feet_bias", (C.c_double * 3) * 4), ("default_joints", C.c_double * 10),
                ("joint_ik", C.c_int32), ("reserved", C.c_int32)]


def make_refgen_config(params: dict, joint_ik: bool = True) -> RefgenConfig:
    c = params["config"]
    sw = c["swing"]
    out = RefgenConfig()
    out.dt, out.com_height = c["dt"], c["com_height"]
    out.next_position_z, out.swing_height, out.swing_time_scale = sw["next_position_z"], sw["swing_height"], sw["swing_time_scale"]
    bias = [[sw["feet_bias_x1"], sw["feet_bias_y"], sw["feet_bias_z"]], [sw["feet_bias_x1"], -sw["feet_bias_y"], sw["feet_bias_z"]],
            [sw["feet_bias_x2"], sw["feet_bias_y"], sw["feet_bias_z"]], [sw["feet_bias_x2"], -sw["feet_bias_y"], sw["feet_bias_z"]]]
    _fill(out.feet_bias, bias)
    _fill(out.default_joints, c["default_joint_state"])
    out.joint_ik = 1 if joint_ik else 0
    return out


PARAMS_BLOB_MAGIC = 0x48423032  # "HB02"


def write_params_blob(params: dict, path) -> None:
    """Binary image of everything a C++ host needs at LeggedController::init, version 2 (include/hunter_ingest.hpp
    loadParametersBlob / writeParametersBlob write and read the same bytes): header {magic, sizeof of the five structs, number of
    initial event times, number of template switching times}, hb_model, hb_config (defaults of make_config: WeightedWbc),
    hb_estimator_config, hb_refgen_config, hb_joint_gains, {timeHorizon, mpcDesiredFrequency, phaseTransitionStanceTime}, the
    initial mode schedule and the default mode-sequence template of reference.info."""
    import struct
    c = params["config"]
    model, config = make_model(params), make_config(params)
    est, rg, gains = make_estimator_config(params), make_refgen_config(params), make_joint_gains()
    ev, modes = c["initial_mode_schedule"]["event_times"], c["initial_mode_schedule"]["modes"]
    tt, tm = c["default_mode_template"]["switching_times"], c["default_mode_template"]["modes"]
    assert len(modes) == len(ev) + 1 and len(tm) == len(tt) - 1
    with open(path, "wb") as f:
        f.write(struct.pack("<8I", PARAMS_BLOB_MAGIC, C.sizeof(HbModel), C.sizeof(HbConfig), C.sizeof(HbEstimatorConfig), C.sizeof(RefgenConfig),
                            C.sizeof(HbJointGains), len(ev), len(tt)))
        for st in (model, config, est, rg, gains):
            f.write(bytes(st))
        f.write(struct.pack("<3d", c["time_horizon"], c["mpc_frequency"], c["phase_transition_stance_time"]))
        f.write(struct.pack(f"<{len(ev)}d", *ev))
        f.write(struct.pack(f"<{len(modes)}i", *modes))
        f.write(struct.pack(f"<{len(tt)}d", *tt))
        f.write(struct.pack(f"<{len(tm)}i", *tm))


HB_GAIT_MAX_INIT_EVENTS, HB_GAIT_MAX_PHASES = 8, 8


class HbGaitConfig(C.Structure):
    """hb_gait_config (include/hunter_hip.h): the device-resident gait manager."""
    _fields_ = [("phase_transition_stance_time", C.c_double), ("init_event_times", C.c_double * HB_GAIT_MAX_INIT_EVENTS),
                ("template_switching_times", C.c_double * (HB_GAIT_MAX_PHASES + 1)), ("n_init_events", C.c_int32),
                ("init_modes", C.c_int32 * (HB_GAIT_MAX_INIT_EVENTS + 1)), ("n_template_phases", C.c_int32),
                ("template_modes", C.c_int32 * HB_GAIT_MAX_PHASES), ("filter_cmd", C.c_int32), ("reserved", C.c_int32)]


def make_gait_config(params: dict, filter_cmd: bool = False) -> HbGaitConfig:
    """initialModeSchedule / defaultModeSequenceTemplate / phaseTransitionStanceTime as ingest.read_config gives them.
    filter_cmd: cmd_vel arguments are raw requests, rate-limited on the device once per pass."""
    c = params["config"]
    ev, modes = c["initial_mode_schedule"]["event_times"], c["initial_mode_schedule"]["modes"]
    tt, tm = c["default_mode_template"]["switching_times"], c["default_mode_template"]["modes"]
    if not (1 <= len(ev) <= HB_GAIT_MAX_INIT_EVENTS and len(modes) == len(ev) + 1):
        raise ValueError("initial mode schedule: 1..8 event times and one more mode")
    if not (1 <= len(tm) <= HB_GAIT_MAX_PHASES and len(tt) == len(tm) + 1):
        raise ValueError("default mode-sequence template: 1..8 phases and one more switching time")
    out = HbGaitConfig()
    out.phase_transition_stance_time = c["phase_transition_stance_time"]
    out.n_init_events, out.n_template_phases = len(ev), len(tm)
    _fill(out.init_event_times, ev)
    _fill(out.init_modes, modes)
    _fill(out.template_switching_times, tt)
    _fill(out.template_modes, tm)
    out.filter_cmd = 1 if filter_cmd else 0
    return out
