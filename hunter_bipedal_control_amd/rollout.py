"""Closed-loop batched rollouts through the C ABI: plant -> observation -> references -> MPC ->
policy -> WBC -> joint command -> plant, the loop of LeggedController::update (legged_controllers/src/LeggedController.cpp:
137-278) and its MPC thread (:396-412), for every instance of a HunterSolver.

Everything between the plant's state and the joint torque runs on the device (reference generation, SQP, policy
evaluation, WBC, joint command law); the plant stub integrates either on the device (ResidentLoop, hb_plant_step) or on the host (DeviceLoop, with a plant object the
caller injects — the tests pass the numpy twin oracle/plant.py)  with the device's rigid-body
terms.  The observation is the plant's true state by default; with use_estimator it is the state estimator's output on the plant's
sensors — host arrays in DeviceLoop (ideal sensors), device arrays in ResidentLoop (hb_plant_sense + hb_estimator_update_resident: no
sensor crosses PCIe; optional biases and seeded noise, hb_plant_set_sensor_model).
"""
from __future__ import annotations

import numpy as np

from . import abi, gait
from . import solver as _solver
from .gait import schedule_window  # noqa: F401  (re-exported: the tests address it as rollout.schedule_window)


def standing_configuration(params: dict, batch: int, solver) -> np.ndarray:
    """q[B][16]: initialState of task.info with the base lowered so that the mean contact-point height is zero (contact
    points from the device kinematics, hb_eval_foot_kinematics)."""
    x0 = np.array(params["config"]["initial_state"], dtype=float)
    q = np.zeros((batch, 16))
    q[:, 0:3], q[:, 3:6], q[:, 6:] = x0[6:9], x0[9:12], x0[12:]
    feet = solver.eval_foot_kinematics(x0[None, :], np.zeros((1, 22)))[0]
    q[:, 2] -= np.asarray(feet).reshape(4, 3)[:, 2].mean()
    return q


def lowest_contact_point(solver, q) -> float:
    """Height of the lowest contact point over the batch q[B][16] (device kinematics): the ground of a rollout that starts there."""
    x = np.zeros((q.shape[0], 22))
    x[:, 6:9], x[:, 9:12], x[:, 12:] = q[:, 0:3], q[:, 3:6], q[:, 6:]
    feet = np.asarray(solver.eval_foot_kinematics(x, np.zeros((q.shape[0], 22)))[0]).reshape(q.shape[0], 4, 3)
    return float(feet[:, :, 2].min())


def plane_under_contact_points(solver, q, normals) -> np.ndarray:
    """d[B] that puts the plane n_i . x = d_i under the lowest contact point of q[i] (device kinematics), normals[B][3] (any length;
    measured along the unit normal): the terrain of a rollout that starts there.  With normals (0, 0, 1) it is the height of each
    instance's lowest contact point (lowest_contact_point is its minimum over the batch)."""
    q = np.atleast_2d(np.asarray(q, dtype=float))
    n = np.broadcast_to(np.asarray(normals, dtype=float), (q.shape[0], 3))
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    x = np.zeros((q.shape[0], 22))
    x[:, 6:9], x[:, 9:12], x[:, 12:] = q[:, 0:3], q[:, 3:6], q[:, 6:]
    feet = np.asarray(solver.eval_foot_kinematics(x, np.zeros((q.shape[0], 22)))[0]).reshape(q.shape[0], 4, 3)
    return np.einsum("bcx,bx->bc", feet, n).min(axis=1)


def curb_profile(height: float, at: float, riser_slope: float = np.sqrt(3.0)) -> np.ndarray:
    """Knots [4][2] of a curb (height > 0) or a step down (height < 0) whose riser starts at s = `at`: level at 0, a riser of slope
    riser_slope (the steepest hb_plant_set_terrain_profile takes is sqrt(3)), level at `height`.  height 0: the same four knots, level."""
    run = max(abs(height) / riser_slope, 1e-3)
    return np.array([[at - 1.0, 0.0], [at, 0.0], [at + run, height], [at + run + 1.0, height]])


def stairs_profile(rise: float, run: float, steps: int, at: float, riser_slope: float = np.sqrt(3.0)) -> np.ndarray:
    """Knots [2 + 2 steps][2] of a flight of `steps` stairs from s = `at`: treads of length `run` (riser included), risers of height `rise`
    (negative: down) and slope riser_slope.  2 + 2 steps <= abi.HB_PROFILE_MAX_KNOTS, so at most 7 steps."""
    w = abs(rise) / riser_slope
    if steps < 1 or 2 + 2 * steps > abi.HB_PROFILE_MAX_KNOTS or not run > w:
        raise ValueError("stairs_profile: 1 .. 7 steps, each tread longer than its riser is wide")
    k = [[at - 1.0, 0.0]]
    for i in range(steps):
        k += [[at + i * run, i * rise], [at + i * run + w, (i + 1) * rise]]
    k.append([at + steps * run + 1.0, steps * rise])
    return np.array(k)


def pack_profiles(profiles):
    """[B] knot arrays of different lengths -> (n_knots[B], knots[B][HB_PROFILE_MAX_KNOTS][2]) of hb_plant_set_terrain_profile."""
    n = np.array([len(k) for k in profiles], dtype=np.int32)
    out = np.zeros((len(profiles), abi.HB_PROFILE_MAX_KNOTS, 2))
    for i, k in enumerate(profiles):
        out[i, :len(k)] = k
    return n, out


FIELD_SLOPE2_MAX = 3.0   # hb_plant_set_terrain_field refuses a triangle with p^2 + r^2 above 3 (1 + 1e-12): n_z < 0.5


def field_slopes2(heights, spacing) -> np.ndarray:
    """p^2 + r^2 of both triangles of every cell of the height field heights[nu][nw] with node spacing (du, dw): [nu - 1][nw - 1][2]
    (lower triangle, upper triangle), as hb_plant_set_terrain_field cuts the cells (along the diagonal from node (i, j) to (i + 1, j + 1))."""
    z = np.asarray(heights, dtype=float)
    du, dw = float(spacing[0]), float(spacing[1])
    z00, z10, z01, z11 = z[:-1, :-1], z[1:, :-1], z[:-1, 1:], z[1:, 1:]
    low = ((z10 - z00) / du) ** 2 + ((z11 - z10) / dw) ** 2
    up = ((z11 - z01) / du) ** 2 + ((z01 - z00) / dw) ** 2
    return np.stack([low, up], axis=-1)


def field_from_profile(direction, knots, du: float, w0: float = -1.0, dw: float = 2.0, nw: int = 2, mu=None) -> dict:
    """The height field that is the terrain profile (direction, knots[K][2]) sampled on a grid: the first grid axis is the profile's
    direction with a node every du from the first knot to the last, every knot on a node (to 1e-9 du, else ValueError), the heights
    constant along the second axis (nw nodes every dw from w0).  Every cell then lies within one segment, so either triangle carries its
    segment's plane and the border cells continue the end segments as the profile does.  -> the dict of one instance of
    ResidentLoop(terrain=dict(field=...)): dir, origin, spacing, heights[nu][nw] (and mu when given)."""
    k = np.asarray(knots, dtype=float)
    at = (k[:, 0] - k[0, 0]) / du
    nu = int(round(at[-1])) + 1
    if np.abs(at - np.round(at)).max() > 1e-9 or not 2 <= nu <= abi.HB_FIELD_MAX_NODES or not 2 <= nw <= abi.HB_FIELD_MAX_NODES:
        raise ValueError("field_from_profile: every knot on a node of the grid, 2 .. HB_FIELD_MAX_NODES nodes per axis")
    z = np.interp(np.round(at[0]) + np.arange(nu), np.round(at), k[:, 1])
    out = dict(dir=np.asarray(direction, dtype=float), origin=np.array([k[0, 0], w0]), spacing=np.array([du, dw]), heights=np.repeat(z[:, None], nw, axis=1))
    if mu is not None:
        out["mu"] = np.asarray(mu, dtype=float)
    return out


def rough_field(seed: int, amplitude: float, spacing, shape=(abi.HB_FIELD_MAX_NODES, abi.HB_FIELD_MAX_NODES)) -> np.ndarray:
    """Heights [nu][nw] of seeded rough ground: independent bumps uniform in [-amplitude, amplitude] per node (numpy default_rng(seed)),
    scaled down as a whole where a triangle would break the slope bound of hb_plant_set_terrain_field (p^2 + r^2 <= 0.99 x 3 after it)."""
    z = amplitude * np.random.default_rng(seed).uniform(-1.0, 1.0, shape)
    worst = float(field_slopes2(z, spacing).max())
    if worst > 0.99 * FIELD_SLOPE2_MAX:
        z *= np.sqrt(0.99 * FIELD_SLOPE2_MAX / worst)
    return z


def pack_fields(fields):
    """[B] dicts(dir[2], origin[2], spacing[2], heights[nu_i][nw_i], mu[4] or missing) -> the arguments of
    HunterSolver.plant_set_terrain_field: (dir[B][2], origin[B][2], spacing[B][2], [B] height arrays, mu[B][4] or None).  mu: given by every
    instance or by none."""
    with_mu = [f.get("mu") is not None for f in fields]
    if any(with_mu) and not all(with_mu):
        raise ValueError("pack_fields: mu for every instance or for none")
    col = lambda k: np.array([np.asarray(f[k], dtype=float) for f in fields]).reshape(len(fields), 2)  # noqa: E731
    return (col("dir"), col("origin"), col("spacing"), [np.asarray(f["heights"], dtype=float) for f in fields],
            np.array([f["mu"] for f in fields], dtype=float) if all(with_mu) and fields else None)


def payload_on_base(mass, pos, inertia=None) -> np.ndarray:
    """The [B][10] payload array of hb_plant_set_model_variation: mass[B] (or a scalar) [kg], pos[B][3] (or [3]) = the payload's centre of
    mass in the base frame from the base origin [m], inertia[B][6] (or [6]) = xx xy xz yy yz zz about that centre in base axes (None: a
    point mass)."""
    mass = np.atleast_1d(np.asarray(mass, dtype=float))
    out = np.zeros((mass.shape[0], abi.HB_PAYLOAD_SIZE))
    out[:, 0] = mass
    out[:, 1:4] = np.broadcast_to(np.asarray(pos, dtype=float), (mass.shape[0], 3))
    if inertia is not None:
        out[:, 4:10] = np.broadcast_to(np.asarray(inertia, dtype=float), (mass.shape[0], 6))
    return out


class DeviceLoop:
    """One HunterSolver driven in closed loop.  `gait` per instance (names of gait.info), `cmd_vel` [B][4]."""

    def __init__(self, solver, params: dict, gaits, cmd_vel, n_intervals: int = 100, mpc_every: int = 8, dt: float = 0.002,
                 t_gait_start: float = 0.3, joint_ik: bool = True, use_estimator: bool = False, use_lcm: bool = False,
                 plant_factory=None):
        """use_lcm (with use_estimator): sensors and commands cross the controller boundary as LCM wire images — the
        plant side encodes low_state_t / applies the PD + feed-forward law of a decoded low_cmd_t like the MuJoCo bridge
        (mujoco/src/main.cc), the controller side uses hb_estimator_update_lcm / hb_joint_command_lcm."""
        assert not (use_lcm and not use_estimator)
        if plant_factory is None:
            raise ValueError("DeviceLoop integrates the plant on the host: pass plant_factory(rbd_fn, foot_fn, q0) "
                             "(tests: oracle.plant.Plant); ResidentLoop keeps the plant on the device")
        self.use_lcm = use_lcm
        self.tau_applied = np.zeros((solver.B, 10))
        self.s, self.params = solver, params
        self.B = solver.B
        c = params["config"]
        self.horizon = n_intervals * c["dt"]
        self.dt, self.mpc_every = dt, mpc_every
        self.cmd = np.ascontiguousarray(cmd_vel, dtype=float).reshape(self.B, 4)
        self.gains = abi.make_joint_gains()
        self.t, self.tick = 0.0, 0
        solver.refgen_reset(abi.make_refgen_config(params, joint_ik=joint_ik))
        # GaitSchedule output per instance; each MPC call hands the device the window [t - 1, t + horizon + 1.5] of it
        # (the reference asks its gait schedule for [t - T, t + 2T], SwitchedModelReferenceManager.cpp:147)
        self.schedules = [gait.gait_schedule(params, g, t_gait_start, 1.0e3 if g == "stance" else 60.0) for g in gaits]
        zeros_u = np.zeros((1, 22))

        def foot_fn(q):
            x = np.zeros((q.shape[0], 22))
            x[:, 6:9], x[:, 9:12], x[:, 12:] = q[:, 0:3], q[:, 3:6], q[:, 6:]
            return solver.eval_foot_kinematics(x, np.repeat(zeros_u, q.shape[0], axis=0))[0]

        self.plant = plant_factory(lambda rbd: solver.eval_rbd(rbd), foot_fn, standing_configuration(params, self.B, solver))
        self.started = False
        self.last = {}
        # use_estimator: the observation comes from hb_estimator_update fed with the plant's ideal IMU, joint encoders and
        # the commanded contact flags (LeggedController::updateStateEstimation) instead of the plant's true state
        self.use_estimator = use_estimator
        self.contact = np.ones((self.B, 4), dtype=np.int32)
        if use_estimator:
            q = self.plant.q
            xh0 = np.zeros((self.B, 18))
            xh0[:, 0:3] = q[:, 0:3]
            feet = self.plant.foot_fn(q)
            xh0[:, 6:18] = feet.reshape(self.B, 12)
            solver.estimator_reset(abi.make_estimator_config(params), xh0)

    def step(self):
        s, B = self.s, self.B
        if self.use_estimator:
            quat, w_loc, a_loc = self.plant.imu()
            if self.use_lcm:   # LcmInterface.cpp:54-70: quaternion (w x y z), gyroscope, accelerometer, joint pos / vel / torque
                fields = np.concatenate([quat[:, 3:4], quat[:, 0:3], w_loc, a_loc, self.plant.q[:, 6:], self.plant.v[:, 6:],
                                         self.tau_applied], axis=1)
                wire = _solver.lcm_encode(_solver.LCM_LOW_STATE, int(round(self.t * 1e9)), fields)
                rbd, x_obs, _ = s.estimator_update_lcm(self.dt, wire, self.contact)
            else:
                rbd, x_obs = s.estimator_update(self.dt, quat, w_loc, a_loc, self.plant.q[:, 6:], self.plant.v[:, 6:], self.contact)
        else:
            rbd = self.plant.rbd()
            x_obs = s.centroidal_state_from_rbd(rbd)
        if self.tick % self.mpc_every == 0:                       # MPC thread: references, one SQP iteration, publish
            s.refgen_set_schedule([schedule_window(ms, self.t - 1.0, self.t + self.horizon + 1.5) for ms in self.schedules])
            status = s.refgen_update(np.full(B, self.t), self.horizon, x_obs, self.cmd)
            if status.max() != 0:
                raise RuntimeError(f"reference generation failed: {status}")
            if not self.started:
                s.reset(x_obs)                                    # cold start (LeggedRobotInitializer)
                self.started = True
            s.mpc_solve(x_obs)
            s.publish()
        out = s.wbc_update(np.full(B, self.t), rbd, dt=self.dt)   # control thread: policy, WBC, joint command
        if self.use_lcm:
            wire = s.joint_command_lcm(self.gains, self.dt, int(round(self.t * 1e9)))
            _, f = _solver.lcm_decode(_solver.LCM_LOW_CMD, wire)      # plant side: PD + feed-forward on the decoded command
            cmd = dict(pos_des=f[:, 0:10], vel_des=f[:, 10:20], tau_ff=f[:, 30:40], kp=f[:, 40:50], kd=f[:, 50:60])
            cmd["torque"] = cmd["tau_ff"] + cmd["kp"] * (cmd["pos_des"] - self.plant.q[:, 6:]) + cmd["kd"] * (cmd["vel_des"] - self.plant.v[:, 6:])
            self.tau_applied = cmd["torque"]
        else:
            cmd = s.joint_command(self.gains, self.dt)
        contact = np.array([gait.mode_to_contact_flags(int(m)) for m in out["mode"]])
        self.plant.step(cmd["torque"], contact, self.dt)
        self.contact = contact.astype(np.int32)
        self.t += self.dt
        self.tick += 1
        self.last = dict(out=out, cmd=cmd, contact=contact, x_obs=x_obs)
        return self.plant.q, self.plant.v


class ResidentLoop:
    """The same loop with the plant stub on the device too (hb_plant_step): nothing but the reference-generation time
    stamps, the commands and the mode-schedule windows crosses PCIe — and with device_gait not even the windows: the gait
    scheduler and the command-driven gait selection (walkGait) run per instance on the device (hb_gait_reset).

    use_estimator closes the loop through the state estimator on the device as well: per tick hb_plant_sense turns the plant's state into
    IMU, encoder, effort and contact-flag arrays, hb_estimator_update_resident filters them into the resident observation, then MPC (every
    mpc_every ticks), WBC, joint command and the plant step follow as before.  sensor_config (abi.make_sensor_config) adds seeded noise,
    sensor_bias = (gyro_bias, accel_bias) [B][3] constant biases; both None: ideal sensors."""

    def __init__(self, solver, params: dict, gaits, cmd_vel, n_intervals: int = 100, mpc_every: int = 8, dt: float = 0.002,
                 t_gait_start: float = 0.3, joint_ik: bool = True, substeps: int = 4, static_schedule_until: float = 0.0,
                 device_gait: bool = False, use_estimator: bool = False, sensor_config=None, sensor_bias=None, contact_config=None,
                 joint_model=None, actuator: str = "held", terrain=None, episode=None, model_variation=None, respawn=None, scenario=None,
                 ground_map=None, profile_draw=None, field_draw=None, height_scan=None, foothold=None):
        """static_schedule_until > 0: the mode schedules are uploaded once for [-1, static_schedule_until] (at most
        HB_MAX_EVENTS events) instead of a sliding window per MPC call — no per-call host work for large batches.
        device_gait: the device gait manager produces the windows; step() builds no per-instance list and uploads no schedule, and
        the gait of every instance follows its command as in the reference (set_cmd replaces the commands between steps).  `gaits`
        other than the default "stance" go in once, at t_gait_start, through hb_gait_insert_template.
        contact_config: the plant's contact model — None: the pinned stub; a dict of abi.make_contact_config fields ({} = the defaults):
        ground with unilateral frictional contact, the plane under the lowest contact point of the start unless ground_z is among them;
        an abi.HbContactConfig is taken as it is.
        joint_model: the joint model of the ground-contact plant — None: ideal joints; a dict of abi.make_joint_model fields ({} = the
        joints of the reference's MuJoCo model); an abi.HbJointModel is taken as it is.  Needs contact_config.
        actuator: "held" — the torque of the joint command is held over the tick (hb_plant_step); "substep" — the plant evaluates the
        command's law ff + kp (pos_des - q) + kd (vel_des - qd) before every substep from its own state (hb_plant_step_hybrid on the
        device-resident command), as the reference's simulator does per simulator step (mujoco/src/main.cc:243-249).
        terrain: per-instance ground of the ground-contact plant — None: the contact model's own plane and mu; dict(plane=[B][4] = unit
        normal and offset d, or [B][3] = normals alone, the plane then goes under the lowest contact point of each instance's start
        (plane_under_contact_points); mu=[B][4] per contact point), either may be missing (hb_plant_set_terrain); or dict(profile=dict(dir=
        [B][2], knots=[B] knot arrays [K_i][2] (curb_profile, stairs_profile) or [B][K][2], mu=[B][4] or missing), relative=True):
        piecewise-planar ground per instance (hb_plant_set_terrain_profile), `relative` adds the height of the lowest contact point of each
        instance's start to the knot heights.  Needs contact_config; set after the contact model.  The controller, estimator and swing
        planner assume level ground unless ground_map tells them otherwise.  Or dict(field=dict(dir=[B][2], origin=[B][2], spacing=[B][2],
        heights=[B] arrays [nu_i][nw_i] (rough_field, field_from_profile) or [B][nu][nw], mu=[B][4] or missing) or a list of B such dicts of
        one instance each, relative=True): a triangulated height field per instance (hb_plant_set_terrain_field), `relative` as for the
        profile.  ground_map="plant" is refused beside a field (the profile map is one-dimensional: ground_map="field" hands the field over),
        and so is respawn=.
        ground_map: the ground the controller's side plans and filters on (hb_ground_set_profile, hb_ground_set_field) — None: the level
        plane; "scan": a field map perceived from the plant's ground on the device (height_scan= below); "field": the plant field's heights above the level ground of the start, as a field map (needs terrain=dict(field=...));
        dict(field=dict(dir=, origin=, spacing=, heights=), per instance as terrain's field): a field map of the caller's, beside any plant
        ground; "plant": the
        plant's terrain profile with the start offset taken out (the knots of terrain["profile"] as given when relative, less the height of
        the lowest contact point of the start otherwise), so a level relative profile is the zero map; dict(dir=[B][2], knots=[B] knot
        arrays [K_i][2] or [B][K][2]): a map of the caller's, heights relative to the level ground the controller assumes — independent of
        the plant's ground, wrong on purpose if wanted.
        model_variation: per-instance inertial parameters of the ground-contact plant — None: the nominal robot; dict(mass_scale=[B][11],
        payload=[B][10] (payload_on_base)), either may be missing (hb_plant_set_model_variation).  Needs contact_config; set after the
        contact model, the joint model and the terrain and before the episode.  The controller keeps the nominal model.
        episode: the per-instance episode record of the plant (hb_plant_set_episode) — None: none; a dict of abi.make_episode_config
        fields ({} = the defaults); an abi.HbEpisodeConfig is taken as it is.  Set after the models and the terrain, so the record starts
        from the start state over the ground of the run; episode() reads it, run(n) advances n ticks without a read-back.
        respawn: repeated episodes per instance (hb_plant_set_respawn) — None: a fallen robot stays fallen; a dict of
        abi.make_respawn_config fields plus, optionally, q_spawn / v_spawn [B][16] (default: the start configuration, at rest).  Needs
        episode= and is set after it.  step() / run() then call plant_respawn() after the plant step of every tick whose successor is an
        MPC tick, so that the policy a respawned instance is driven by is always one of its own episode; respawn_totals() reads the totals.
        scenario: a scenario drawn on the device for every respawned instance (hb_plant_set_scenario) — None: none; a dict of
        abi.make_scenario_config fields; an abi.HbScenarioConfig is taken as it is.  Needs respawn= (and contact_config=) and is set
        after it; scenario() / scenario_log() read the current parameters and the log of the finished episodes.
        profile_draw: a piecewise-planar ground (level, a curb or step-down, a flight of stairs) drawn on the device for every respawned
        instance (hb_plant_set_profile_draw) — None: none; a dict of abi.make_profile_draw_config fields; an abi.HbProfileDrawConfig is
        taken as it is.  Needs respawn= and contact_config=, excludes terrain= (the draw owns the ground) and is set after the scenario;
        ground_map="draw" sets the zero map along the draw's direction and follow_map, so the controller's map follows every drawn
        ground.  profile_draw() / profile_draw_log() read the current parameters and the log of the finished episodes.
        field_draw: a height field (level, rough, tilted or both) composed on the device for every respawned instance
        (hb_plant_set_field_draw) — None: none; a dict of abi.make_field_draw_config fields; an abi.HbFieldDrawConfig is taken as it is.
        Needs respawn= and contact_config=, excludes terrain= and profile_draw= (one draw owns the ground) and is set after the scenario;
        ground_map="draw" sets the zero field map over the draw's grid and follow_map, so the controller's map follows every drawn
        field.  field_draw() / field_draw_log() read the current parameters and the log of the finished episodes.  (A field of the
        host's, terrain=dict(field=...), stays refused beside respawn=.)
        height_scan: with ground_map="scan" the controller's field map is PERCEIVED from the plant's ground on the device
        (hb_plant_set_height_scan) — a dict of abi.make_height_scan_config fields ({} or None: the ideal 32 x 32 sensor) plus, optionally,
        every= (default mpc_every): plant_scan() runs at the top of every tick that is a multiple of it, ahead of the sensors and the
        estimator and behind a respawn of the tick before; an abi.HbHeightScanConfig is taken as it is (every = mpc_every).  The zero field
        map over the scan grid goes in first.  Needs contact_config=; composes with terrain=dict(plane= | profile= | field=) and with
        profile_draw= / field_draw= that do not follow (a draw with follow_map beside it is a ValueError: one writer of the map).
        height_scan() reads origin index, return counts and return flags of the last scan.
        foothold: the planner's foothold mode on the map (hb_ground_set_foothold) — None: the call is not made (per contact point); a dict
        of abi.make_foothold_config fields, e.g. dict(mode="sole", n_shift=3, shift_step=0.02, flat_tol=0.005): with mode "sole" the toe
        and the heel of a foot are planned as one sole, shifted along its axis off an edge or levelled on it.  These defaults are
        UNMEASURED placeholders: nobody has tuned n_shift, shift_step or flat_tol yet.  An abi.HbFootholdConfig is taken as it is.  Acts
        while a map is in force (any ground_map=); foothold_choice() reads what the last planner pass decided."""
        if height_scan is not None and not (isinstance(ground_map, str) and ground_map == "scan"):
            raise ValueError('height_scan= belongs to ground_map="scan"')
        if isinstance(ground_map, str) and ground_map == "scan":
            if contact_config is None:
                raise ValueError('ground_map="scan" scans the ground of the ground-contact plant: give contact_config= as well')
            for draw in (profile_draw, field_draw):
                follows = draw.get("follow_map", 0) if isinstance(draw, dict) else getattr(draw, "follow_map", 0)
                if draw is not None and follows:
                    raise ValueError('ground_map="scan" beside a draw with follow_map: the scan and the draw would both write the controller\'s map')
        if field_draw is not None and (respawn is None or contact_config is None):
            raise ValueError("the field is drawn at respawn, for the ground-contact plant: give respawn= and contact_config= as well")
        if field_draw is not None and (terrain is not None or profile_draw is not None):
            raise ValueError("field_draw draws the ground: no terrain= or profile_draw= beside it")
        if profile_draw is not None and (respawn is None or contact_config is None):
            raise ValueError("the profile is drawn at respawn, for the ground-contact plant: give respawn= and contact_config= as well")
        if profile_draw is not None and terrain is not None:
            raise ValueError("profile_draw draws the ground: no terrain= beside it")
        if isinstance(ground_map, str) and ground_map == "draw" and profile_draw is None and field_draw is None:
            raise ValueError('ground_map="draw" follows the drawn ground: give profile_draw= or field_draw= as well')
        if scenario is not None and (respawn is None or contact_config is None):
            raise ValueError("the scenario is drawn at respawn, for the ground-contact plant: give respawn= and contact_config= as well")
        if respawn is not None and episode is None:
            raise ValueError("respawn reads its decision from the episode record: give episode= as well")
        if model_variation is not None and contact_config is None:
            raise ValueError("model_variation belongs to the ground-contact plant: give contact_config as well")
        if terrain is not None and contact_config is None:
            raise ValueError("terrain belongs to the ground-contact plant: give contact_config as well")
        if terrain is not None and terrain.get("field") is not None:
            if terrain.get("plane") is not None or terrain.get("mu") is not None or terrain.get("profile") is not None:
                raise ValueError("terrain: a field, a profile or a plane, one ground at a time (the field's mu goes inside field=)")
            if isinstance(ground_map, str) and ground_map == "plant":
                raise ValueError('ground_map="plant" with a height field: the controller\'s map is one-dimensional (give dict(dir=..., knots=...) or None)')
            if respawn is not None:
                raise ValueError("no respawn on a height field")
        if actuator not in ("held", "substep"):
            raise ValueError('actuator is "held" or "substep"')
        self.actuator = actuator
        if joint_model is not None and contact_config is None:
            raise ValueError("joint_model belongs to the ground-contact plant: give contact_config as well")
        self.s, self.params, self.B = solver, params, solver.B
        self.horizon = n_intervals * params["config"]["dt"]
        self.dt, self.mpc_every, self.substeps = dt, mpc_every, substeps
        self.cmd = np.ascontiguousarray(cmd_vel, dtype=float).reshape(self.B, 4)
        self.gains = abi.make_joint_gains()
        self.t, self.tick = 0.0, 0
        solver.refgen_reset(abi.make_refgen_config(params, joint_ik=joint_ik))
        self.device_gait = device_gait
        if device_gait:
            if static_schedule_until > 0.0:
                raise ValueError("static_schedule_until is a host-schedule option")
            solver.gait_reset(abi.make_gait_config(params))
            gaits, named = list(gaits), params["config"]["gaits"]
            i = 0
            while i < self.B:                                  # one call per run of instances with the same named gait
                j = i
                while j < self.B and gaits[j] == gaits[i]:
                    j += 1
                if gaits[i] != "stance":
                    g = named[gaits[i]]
                    solver.gait_insert_template(g["switching_times"], g["modes"], np.full(j - i, t_gait_start),
                                                t_gait_start + self.horizon, inst_begin=i)
                i = j
            self.schedules = None
        else:
            self.schedules = [gait.gait_schedule(params, g, t_gait_start, 1.0e3 if g == "stance" else 60.0) for g in gaits]
        q0 = standing_configuration(params, self.B, solver)
        solver.plant_reset(q0)
        if contact_config is not None:
            if isinstance(contact_config, dict):   # fields of abi.make_contact_config; the plane goes under the start unless given
                fields = dict(contact_config)
                fields.setdefault("ground_z", lowest_contact_point(solver, q0))
                contact_config = abi.make_contact_config(params, **fields)
            solver.plant_set_contact_model(contact_config)
            if joint_model is not None:
                solver.plant_set_joint_model(abi.make_joint_model(params, **joint_model) if isinstance(joint_model, dict) else joint_model)
            if terrain is not None and terrain.get("field") is not None:
                fld = terrain["field"]
                flds = fld if isinstance(fld, (list, tuple)) else [{k: v[i] for k, v in fld.items() if v is not None} for i in range(self.B)]
                d, org, sp, hts, fmu = pack_fields(flds)
                z0 = plane_under_contact_points(solver, q0, [0.0, 0.0, 1.0])
                plant_field = dict(dir=d, origin=org, spacing=sp, heights=hts if terrain.get("relative", True) else [h - z0[i] for i, h in enumerate(hts)])
                if terrain.get("relative", True):
                    hts = [h + z0[i] for i, h in enumerate(hts)]
                solver.plant_set_terrain_field(d, org, sp, hts, fmu)
            elif terrain is not None and terrain.get("profile") is not None:
                if terrain.get("plane") is not None or terrain.get("mu") is not None:
                    raise ValueError("terrain: a profile or a plane, one ground at a time (the profile's mu goes inside profile=)")
                prof = terrain["profile"]
                n_knots, knots = pack_profiles([np.asarray(k, dtype=float) for k in prof["knots"]])
                z0 = plane_under_contact_points(solver, q0, [0.0, 0.0, 1.0])
                plant_map = dict(n_knots=n_knots, dir=np.asarray(prof["dir"], dtype=float).reshape(self.B, 2), knots=knots.copy())
                for i in range(self.B):
                    if terrain.get("relative", True):
                        knots[i, :n_knots[i], 1] += z0[i]
                    else:
                        plant_map["knots"][i, :n_knots[i], 1] -= z0[i]
                solver.plant_set_terrain_profile(n_knots, np.asarray(prof["dir"], dtype=float).reshape(self.B, 2), knots, prof.get("mu"))
            elif terrain is not None:
                plane = terrain.get("plane")
                if plane is not None:
                    plane = np.asarray(plane, dtype=float).reshape(self.B, -1)
                    if plane.shape[1] == 3:
                        n = plane / np.linalg.norm(plane, axis=1, keepdims=True)
                        plane = np.concatenate([n, plane_under_contact_points(solver, q0, n)[:, None]], axis=1)
                solver.plant_set_terrain(plane, terrain.get("mu"))
        if isinstance(ground_map, str) and ground_map in ("draw", "scan"):
            pass   # (the zero map goes in with the draw / the scan, below)
        elif isinstance(ground_map, str) and ground_map == "field":   # the plant field's heights above the level ground of the start
            if terrain is None or terrain.get("field") is None or contact_config is None:
                raise ValueError('ground_map="field" hands the plant\'s height field to the controller: give terrain=dict(field=...) as well')
            solver.ground_set_field(plant_field["dir"], plant_field["origin"], plant_field["spacing"], plant_field["heights"])
        elif isinstance(ground_map, str):
            if ground_map != "plant" or terrain is None or terrain.get("profile") is None:
                raise ValueError('ground_map is None, "plant" (with terrain=dict(profile=...)), "field" (with terrain=dict(field=...)), "draw" (with profile_draw= or field_draw=), "scan", dict(dir=..., knots=...) or dict(field=dict(dir=, origin=, spacing=, heights=))')
            solver.ground_set_profile(plant_map["n_knots"], plant_map["dir"], plant_map["knots"])
        elif ground_map is not None and ground_map.get("field") is not None:   # a field map of the caller's
            fld = ground_map["field"]
            flds = fld if isinstance(fld, (list, tuple)) else [{k: v[i] for k, v in fld.items() if v is not None} for i in range(self.B)]
            d, org, sp, hts, _ = pack_fields(flds)
            solver.ground_set_field(d, org, sp, hts)
        elif ground_map is not None:
            n_knots, knots = pack_profiles([np.asarray(k, dtype=float) for k in ground_map["knots"]])
            solver.ground_set_profile(n_knots, np.asarray(ground_map["dir"], dtype=float).reshape(self.B, 2), knots)
        if model_variation is not None:
            solver.plant_set_model_variation(model_variation.get("mass_scale"), model_variation.get("payload"))
        if episode is not None:
            solver.plant_set_episode(abi.make_episode_config(**episode) if isinstance(episode, dict) else episode)
        self.has_episode = episode is not None
        self.has_respawn = respawn is not None
        if respawn is not None:
            fields = dict(respawn)
            q_spawn, v_spawn = fields.pop("q_spawn", q0), fields.pop("v_spawn", None)
            solver.plant_set_respawn(abi.make_respawn_config(**fields), q_spawn, v_spawn)
        self.has_scenario = scenario is not None
        if scenario is not None:
            solver.plant_set_scenario(abi.make_scenario_config(**scenario) if isinstance(scenario, dict) else scenario)
        self.has_profile_draw = profile_draw is not None
        if profile_draw is not None:
            follow = isinstance(ground_map, str) and ground_map == "draw"
            if isinstance(profile_draw, dict):
                fields = dict(profile_draw)
                if follow:
                    fields["follow_map"] = 1
                profile_draw = abi.make_profile_draw_config(**fields)
            if follow:
                if not profile_draw.follow_map:
                    raise ValueError('ground_map="draw" needs follow_map in the configuration given')
                level = np.tile(np.array([[-1.0, 0.0], [1.0, 0.0]]), (self.B, 1, 1))
                solver.ground_set_profile(np.full(self.B, 2), np.tile(np.array(profile_draw.dir[:]), (self.B, 1)), level)
            solver.plant_set_profile_draw(profile_draw)
        self.has_field_draw = field_draw is not None
        if field_draw is not None:
            follow = isinstance(ground_map, str) and ground_map == "draw"
            if isinstance(field_draw, dict):
                fields = dict(field_draw)
                if follow:
                    fields["follow_map"] = 1
                field_draw = abi.make_field_draw_config(**fields)
            if follow:
                if not field_draw.follow_map:
                    raise ValueError('ground_map="draw" needs follow_map in the configuration given')
                nu, nw = field_draw.n_nodes[0], field_draw.n_nodes[1]
                solver.ground_set_field(np.tile(np.array(field_draw.dir[:]), (self.B, 1)), np.zeros((self.B, 2)),
                                        np.tile(np.array(field_draw.spacing[:]), (self.B, 1)), np.zeros((self.B, nu, nw)))
            solver.plant_set_field_draw(field_draw)
        self.scan_every = 0
        if isinstance(ground_map, str) and ground_map == "scan":
            self.scan_every = int(mpc_every)
            if height_scan is None or isinstance(height_scan, dict):
                fields = dict(height_scan or {})
                self.scan_every = int(fields.pop("every", mpc_every))
                height_scan = abi.make_height_scan_config(**fields)
            if self.scan_every < 1:
                raise ValueError("height_scan: every >= 1")
            nu, nw = height_scan.n_nodes[0], height_scan.n_nodes[1]
            solver.ground_set_field(np.tile(np.array(height_scan.dir[:]), (self.B, 1)), np.zeros((self.B, 2)),
                                    np.tile(np.array(height_scan.spacing[:]), (self.B, 1)), np.zeros((self.B, nu, nw)))
            solver.plant_set_height_scan(height_scan)
        self.has_foothold = foothold is not None
        if foothold is not None:
            solver.ground_set_foothold(abi.make_foothold_config(**foothold) if isinstance(foothold, dict) else foothold)
        # resident observation of the initial state
        rbd = np.zeros((self.B, 32))
        rbd[:, 0:3], rbd[:, 3:6], rbd[:, 6:16] = q0[:, 3:6], q0[:, 0:3], q0[:, 6:]
        solver.set_resident_inputs(solver.centroidal_state_from_rbd(rbd), np.zeros(self.B), rbd)
        self.started = False
        self.use_estimator = use_estimator
        if use_estimator:
            # the filter starts where DeviceLoop starts it: base position and the four contact points of q0
            x = np.zeros((self.B, 22))
            x[:, 6:9], x[:, 9:12], x[:, 12:] = q0[:, 0:3], q0[:, 3:6], q0[:, 6:]
            xh0 = np.zeros((self.B, 18))
            xh0[:, 0:3] = q0[:, 0:3]
            xh0[:, 6:18] = np.asarray(solver.eval_foot_kinematics(x, np.zeros((self.B, 22)))[0]).reshape(self.B, 12)
            solver.estimator_reset(abi.make_estimator_config(params), xh0)
            gyro_bias, accel_bias = sensor_bias if sensor_bias is not None else (None, None)
            solver.plant_set_sensor_model(sensor_config, gyro_bias, accel_bias)
        elif sensor_config is not None or sensor_bias is not None:
            raise ValueError("sensor_config / sensor_bias belong to use_estimator=True")
        self.static = static_schedule_until > 0.0
        if self.static:
            solver.refgen_set_schedule([schedule_window(ms, -1.0, static_schedule_until) for ms in self.schedules])

    def _windows(self):
        """Host schedule path: the mode-schedule window of every instance for this MPC call."""
        return [schedule_window(ms, self.t - 1.0, self.t + self.horizon + 1.5) for ms in self.schedules]

    def set_cmd(self, cmd_vel):
        """Replace the velocity commands [B][4] = (vx, vy, vz, yaw rate); they take effect at the next MPC call."""
        self.cmd = np.ascontiguousarray(cmd_vel, dtype=float).reshape(self.B, 4)

    def step(self, want_outputs: bool = False, check_refgen: bool = True):
        """want_outputs: the WBC result and the joint command of the tick come back to the host (self.last = dict(out, cmd), as
        DeviceLoop keeps them) instead of staying on the device; the loop itself is the same.  check_refgen False: the status of the
        reference generation is not read back (run)."""
        s = self.s
        if self.scan_every and self.tick % self.scan_every == 0:
            s.plant_scan()
        if self.use_estimator:
            s.plant_sense()
            s.estimator_update_resident(self.dt, to_resident=True)
            s.set_resident_time(np.full(self.B, self.t))       # (the estimator knows no clock; the plant step below leaves it alone)
        if self.tick % self.mpc_every == 0:
            if not self.static and not self.device_gait:
                s.refgen_set_schedule(self._windows())
            status = s.refgen_update(np.full(self.B, self.t), self.horizon, None, self.cmd, want_status=check_refgen)
            if check_refgen and status.max() != 0:
                raise RuntimeError(f"reference generation failed: {status}")
            if not self.started:
                s.reset_resident()
                self.started = True
            s.mpc_solve(None)
            s.publish()
        if want_outputs:
            self.last = dict(out=s.wbc_update(None, None, dt=self.dt), cmd=s.joint_command(self.gains, self.dt))
        else:
            s.wbc_update_resident(self.dt)
            s.joint_command_resident(self.gains, self.dt)
        if self.actuator == "substep":
            s.plant_step_hybrid(None, None, self.dt, self.substeps, to_resident=not self.use_estimator)
        else:
            s.plant_step(None, None, self.dt, self.substeps, to_resident=not self.use_estimator)
        self.t += self.dt
        self.tick += 1
        if self.has_respawn and self.tick % self.mpc_every == 0:   # the next tick is an MPC tick
            s.plant_respawn()

    def run(self, n: int):
        """n ticks of step() with no read-back: every call of a tick is enqueue-only (the status of the reference generation is looked at
        once, after the last tick).  What happened is in the episode record (episode())."""
        for _ in range(int(n)):
            self.step(check_refgen=False)
        status = self.s.refgen_status()
        if status.max() != 0:
            raise RuntimeError(f"reference generation failed: {status}")

    def foothold_choice(self) -> dict:
        """What the last planner pass in sole mode decided per (instance, foot) (HunterSolver.ground_get_foothold_choice)."""
        if not self.has_foothold:
            raise ValueError("ResidentLoop was built without foothold=")
        return self.s.ground_get_foothold_choice()

    def episode(self, want_trace: bool = False) -> dict:
        """The episode records of the run so far (HunterSolver.plant_episode)."""
        if not self.has_episode:
            raise ValueError("ResidentLoop was built without episode=")
        return self.s.plant_episode(want_trace)

    def respawn_totals(self, want_state: bool = False) -> dict:
        """The totals of the finished episodes (HunterSolver.plant_respawn_totals)."""
        if not self.has_respawn:
            raise ValueError("ResidentLoop was built without respawn=")
        return self.s.plant_respawn_totals(want_state)


    def scenario(self):
        """scen[B][HB_SC_N] of the episodes that are running (HunterSolver.plant_scenario)."""
        if not self.has_scenario:
            raise ValueError("ResidentLoop was built without scenario=")
        return self.s.plant_scenario()

    def scenario_log(self) -> dict:
        """The log of the finished episodes (HunterSolver.plant_scenario_log)."""
        if not self.has_scenario:
            raise ValueError("ResidentLoop was built without scenario=")
        return self.s.plant_scenario_log()


    def profile_draw(self):
        """row[B][HB_PD_N] of the grounds the running episodes stand on (HunterSolver.plant_profile_draw)."""
        if not self.has_profile_draw:
            raise ValueError("ResidentLoop was built without profile_draw=")
        return self.s.plant_profile_draw()

    def field_draw(self):
        """row[B][HB_FD_N] of the fields the running episodes stand on (HunterSolver.plant_get_field_draw)."""
        if not self.has_field_draw:
            raise ValueError("ResidentLoop was built without field_draw=")
        return self.s.plant_get_field_draw()

    def height_scan(self) -> dict:
        """Origin index, return counts and return flags of the last scan (HunterSolver.plant_get_height_scan)."""
        if not self.scan_every:
            raise ValueError('ResidentLoop was built without ground_map="scan"')
        return self.s.plant_get_height_scan()

    def field_draw_log(self) -> dict:
        """The log of the finished episodes (HunterSolver.plant_get_field_draw_log)."""
        if not self.has_field_draw:
            raise ValueError("ResidentLoop was built without field_draw=")
        return self.s.plant_get_field_draw_log()

    def profile_draw_log(self) -> dict:
        """The log of the finished episodes (HunterSolver.plant_profile_draw_log)."""
        if not self.has_profile_draw:
            raise ValueError("ResidentLoop was built without profile_draw=")
        return self.s.plant_profile_draw_log()


def field_draw_table(log: dict) -> dict:
    """The log of HunterSolver.plant_get_field_draw_log as flat arrays over all finished episodes that were logged, instance by instance in
    the order they finished: INSTANCE, the five abi.FIELD_DRAW_LOG_HEAD fields (EPISODE, CAUSE and TICKS as integers) and the parameters
    of abi.FIELD_DRAW_FIELDS ([n] or [n][4]; KIND as an integer)."""
    count, rows = np.asarray(log["count"]), np.asarray(log["log"])
    flat = np.concatenate([rows[i, :count[i]] for i in range(len(count))], axis=0) if len(count) else np.zeros((0, abi.HB_FD_LOG_W))
    flat = flat.reshape(-1, abi.HB_FD_LOG_W)
    out = dict(INSTANCE=np.repeat(np.arange(len(count)), count))
    for k, name in enumerate(abi.FIELD_DRAW_LOG_HEAD):
        out[name] = flat[:, k].astype(np.int64) if name in ("EPISODE", "CAUSE", "TICKS") else flat[:, k].copy()
    out.update(abi.split_field_draw(flat[:, len(abi.FIELD_DRAW_LOG_HEAD):]))
    out["KIND"] = out["KIND"].astype(np.int64)
    return out


def profile_draw_table(log: dict) -> dict:
    """The log of HunterSolver.plant_profile_draw_log as flat arrays over all finished episodes that were logged, instance by instance in
    the order they finished: INSTANCE, the five abi.PROFILE_DRAW_LOG_HEAD fields (EPISODE, CAUSE and TICKS as integers) and the parameters
    of abi.PROFILE_DRAW_FIELDS ([n] or [n][k]; KIND and STEPS as integers)."""
    count, rows = np.asarray(log["count"]), np.asarray(log["log"])
    inst = np.repeat(np.arange(len(count)), count)
    flat = np.concatenate([rows[i, :count[i]] for i in range(len(count))], axis=0) if len(count) else np.zeros((0, abi.HB_PD_LOG_W))
    flat = flat.reshape(-1, abi.HB_PD_LOG_W)
    out = dict(INSTANCE=inst)
    for k, name in enumerate(abi.PROFILE_DRAW_LOG_HEAD):
        out[name] = flat[:, k].astype(np.int64) if name in ("EPISODE", "CAUSE", "TICKS") else flat[:, k].copy()
    out.update(abi.split_profile_draw(flat[:, len(abi.PROFILE_DRAW_LOG_HEAD):]))
    out["KIND"], out["STEPS"] = out["KIND"].astype(np.int64), out["STEPS"].astype(np.int64)
    return out


def scenario_table(log: dict) -> dict:
    """The log of HunterSolver.plant_scenario_log as flat arrays over all finished episodes that were logged, instance by instance in the
    order they finished: INSTANCE, the six abi.SCENARIO_LOG_HEAD fields (EPISODE, CAUSE and TICKS as integers) and the parameters of
    abi.SCENARIO_FIELDS ([n] or [n][k])."""
    count, rows = np.asarray(log["count"]), np.asarray(log["log"])
    inst = np.repeat(np.arange(len(count)), count)
    flat = np.concatenate([rows[i, :count[i]] for i in range(len(count))], axis=0) if len(count) else np.zeros((0, abi.HB_SC_LOG_W))
    flat = flat.reshape(-1, abi.HB_SC_LOG_W)
    out = dict(INSTANCE=inst)
    for k, name in enumerate(abi.SCENARIO_LOG_HEAD):
        out[name] = flat[:, k].astype(np.int64) if name in ("EPISODE", "CAUSE", "TICKS") else flat[:, k].copy()
    out.update(abi.split_scenario(flat[:, len(abi.SCENARIO_LOG_HEAD):]))
    return out


def respawn_summary(totals: dict, dt: float = 0.002) -> dict:
    """Per instance, from the totals alone (HunterSolver.plant_respawn_totals): episodes finished, survival_rate = share of them that ended
    by time-out (neither fallen nor non-finite), fall_rate, mean_ticks and mean_time = mean_ticks dt of an episode, mean_distance_x /
    mean_distance_y per episode (ratios are 0 for an instance with no finished episode)."""
    n = np.asarray(totals["EPISODES"], dtype=float)
    per = np.where(n > 0, 1.0 / np.maximum(n, 1.0), 0.0)
    mean_ticks = totals["TICKS_SUM"] * per
    return dict(episodes=np.asarray(totals["EPISODES"]).copy(), survival_rate=totals["N_TIMEOUT"] * per, fall_rate=totals["N_FALLEN"] * per,
                mean_ticks=mean_ticks, mean_time=mean_ticks * dt, mean_distance_x=totals["DIST_X_SUM"] * per,
                mean_distance_y=totals["DIST_Y_SUM"] * per)


def episode_summary(record: dict, start=None, dt: float = 0.002) -> dict:
    """Per instance, from the episode record alone (HunterSolver.plant_episode): survived (no end so far), end_tick and end_cause (-1 and
    abi.HB_EP_RUNNING while it runs), distance_x / distance_y travelled from `start` ([B][3] or None: the record's START_POS) to the last
    upright tick, mean_speed = horizontal distance / (TICKS dt), slip_share = SLIP_TICKS / TICKS, duty_factor[B][4] = CONTACT_TICKS / TICKS
    (ratios are 0 for an instance with no upright tick)."""
    ticks = np.asarray(record["TICKS"], dtype=float)
    start = np.asarray(record["START_POS"] if start is None else start, dtype=float).reshape(len(ticks), 3)
    dx, dy = record["LAST_BASE"][:, 0] - start[:, 0], record["LAST_BASE"][:, 1] - start[:, 1]
    per_tick = np.where(ticks > 0, 1.0 / np.maximum(ticks, 1.0), 0.0)
    return dict(survived=np.asarray(record["END_TICK"]) < 0, end_tick=np.asarray(record["END_TICK"]).copy(),
                end_cause=np.asarray(record["END_CAUSE"]).copy(), distance_x=dx, distance_y=dy,
                mean_speed=np.hypot(dx, dy) * per_tick / dt, slip_share=record["SLIP_TICKS"] * per_tick,
                duty_factor=record["CONTACT_TICKS"] * per_tick[:, None])
