#!/usr/bin/env python3
"""Scenario sweeps of the closed loop on the device plant, one batch each, read from the per-instance episode record alone
(hb_plant_set_episode): no getter is called between the first tick and the last.

    python tools/sweep_rollout.py                       the friction sweep (B = 8) and the slope sweep (B = 4) of DESIGN.md 5 item 20, 600 ticks
    python tools/sweep_rollout.py --grid 64 64 --ticks 5000   friction x slope on a grid, one scenario per instance (4096), static schedules
    python tools/sweep_rollout.py --payload 8 5 --ticks 5000  payload mass 0 .. 15 kg x fore-aft offset -0.1 .. 0.1 m, 0.15 m above the base origin, on
                                                        level ground with mu 0.7, one pair per instance (hb_plant_set_model_variation)
    python tools/sweep_rollout.py --respawn 250 --ticks 2000  the friction sweep as repeated episodes of at most 250 ticks per instance (hb_plant_set_respawn:
                                                        a fallen robot is put back at the next MPC boundary), read from the respawn totals alone
    python tools/sweep_rollout.py --randomize 2000 --robots 4096   a robustness sweep in one run(n) and one read-back: every respawn draws slope, friction,
                                                        payload and a push on the device (hb_plant_set_scenario); survival rate and mean ticks
                                                        binned by mu, grade and payload mass, from the scenario log alone.  --host-driven: the
                                                        same sweep with the host calling the setters per respawn round and uploading a wrench
                                                        per tick, for the wall time of both
    python tools/sweep_rollout.py --curb                one curb or step-down height per robot (0 / 1 / 2 / 3 cm down and up, B = 8), the riser --curb-at
                                                        metres ahead of the base origin, trot across it (hb_plant_set_terrain_profile);
                                                        --ground-map: the controller plans and filters on the plant's profile
                                                        (hb_ground_set_profile) instead of on the level plane
    python tools/sweep_rollout.py --random-curbs 3000 --robots 256 --max-ticks 1000   repeated episodes on a ground drawn on the device per episode: level, a curb
                                                        or step-down of -3 .. 3 cm, or a flight of 1 .. 4 stairs (hb_plant_set_profile_draw);
                                                        survival, progress and tilt by kind and height bin, from one run(n) and one
                                                        read-back of the draw's log.  --ground-map: the controller's map follows every drawn
                                                        ground; --joint-model as everywhere
    python tools/sweep_rollout.py --rough 1500 --robots 64   rough ground: a seeded 32 x 32 height field of 5 cm cells per robot, bump amplitude
                                                        0 .. --rough-max metres in eight steps over the batch (hb_plant_set_terrain_field), the
                                                        controller blind; survival, tilt and slip by amplitude from one run(n) and one
                                                        read-back of the episode record.  --ground-map: the same rows once more with the
                                                        field as the controller's field map (hb_ground_set_field), next to the blind ones
    python tools/sweep_rollout.py --random-rough 3000 --robots 256 --max-ticks 1000   repeated episodes on a height field composed on the device per episode:
                                                        level, rough (bump amplitude 0 .. --rough-max), tilted (slopes up to 0.1) or both, a 32 x 32
                                                        grid of 5 cm cells around the spawn point (hb_plant_set_field_draw); survival, progress
                                                        and largest tilt by kind and amplitude bin, from one run(n) and one read-back of the
                                                        draw's log.  --ground-map: the controller's field map follows every drawn field;
                                                        --joint-model as everywhere
    python tools/sweep_rollout.py --readback            the two sweeps once more with the per-tick read-back loop the findings of items 17 - 20
                                                        were made with, for the wall time per tick of both

Every robot trots at (0.2, 0) m/s; fall_height 0.3 m, slip = tangential speed of a touching point above 0.05 m/s.  Ticks are counted
from 0: "end 263" is the 264th step."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hunter_bipedal_control_amd import abi, ingest  # noqa: E402
from hunter_bipedal_control_amd.rollout import (ResidentLoop, curb_profile, episode_summary, field_draw_table, payload_on_base,  # noqa: E402
                                                profile_draw_table, respawn_summary, rough_field, scenario_table)
from hunter_bipedal_control_amd.solver import HunterSolver  # noqa: E402

FRICTION = [0.7, 0.5, 0.4, 0.3, 0.2, 0.15, 0.1, 0.05]
SLOPES = [0.0, 0.05, 0.1, 0.2]
CURBS = [0.0, -0.01, -0.02, -0.03, 0.0, 0.01, 0.02, 0.03]
CAUSE = {abi.HB_EP_RUNNING: "-", abi.HB_EP_FALLEN: "fallen", abi.HB_EP_NONFINITE: "non-finite"}


def normals_of(pitch):
    """Unit normals of pitch slopes, downhill along +x."""
    pitch = np.asarray(pitch, dtype=float)
    return np.stack([np.sin(pitch), np.zeros_like(pitch), np.cos(pitch)], axis=1)


def make_loop(params, mu, pitch, ticks, static, joint_model, payload=None, respawn=None):
    """One batch: instance i trots on a plane of pitch[i] with friction mu[i] under all four points, carrying payload[i] ([B][10]) if given."""
    B = len(mu)
    s = HunterSolver(params, batch=B, max_nodes=108)
    cmd = np.tile([0.2, 0.0, 0.0, 0.0], (B, 1))
    horizon = 100 * params["config"]["dt"]
    loop = ResidentLoop(s, params, ["trot"] * B, cmd, contact_config=dict(fall_height=0.3), joint_model=joint_model,
                        terrain=dict(plane=normals_of(pitch), mu=np.repeat(np.asarray(mu, dtype=float)[:, None], 4, axis=1)),
                        static_schedule_until=(ticks * 0.002 + horizon + 1.5) if static else 0.0, episode=dict(slip_speed=0.05),
                        model_variation=None if payload is None else dict(payload=payload), respawn=respawn)
    return s, loop


# the sensor of --scan: 32 x 32 nodes of 5 cm along the walk, the robot in the cell 0.35 m from the rear edge and in the middle across (the
# window of --rough, carried along)
SCAN_GRID = dict(n_nodes=(32, 32), back=(7, 15), dir=(1.0, 0.0), spacing=(0.05, 0.05))


# --sole: the foothold configuration every mapped run of this process hands to ResidentLoop (None: the call is not made), and what
# run_ticks has read of the choice read-back since: planned first footholds, those accepted off the nominal place, those levelled
SOLE = None
SOLE_STATS = dict(planned=0, shifted=0, levelled=0)


def map_args(handed, scan, how):
    """ResidentLoop's ground_map / height_scan: the map perceived by the scan (scan: a dict of abi.make_height_scan_config fields), handed
    over (`how`: "plant", "field" or "draw") or none; with --sole and a map, the foothold configuration as well."""
    sole = dict(foothold=SOLE) if SOLE is not None and (scan is not None or handed) else {}
    if scan is not None:
        return dict(ground_map="scan", height_scan=dict(SCAN_GRID, **scan), **sole)
    return dict(ground_map=how if handed else None, **sole)


def run_ticks(loop, ticks):
    """loop.run(ticks); in sole mode in pieces of one MPC period, the choice read-back sampled after each (the only read-back of the run
    besides the planner's status)."""
    if not getattr(loop, "has_foothold", False):
        loop.run(ticks)
        return
    done = 0
    while done < ticks:
        n = min(loop.mpc_every, ticks - done)
        loop.run(n)
        done += n
        c = loop.foothold_choice()
        planned = c["shift"] != abi.HB_NO_FOOTHOLD
        SOLE_STATS["planned"] += int(planned.sum())
        SOLE_STATS["shifted"] += int((planned & (c["shift"] != 0) & (c["level"] == 0)).sum())
        SOLE_STATS["levelled"] += int((planned & (c["level"] == 1)).sum())


def print_sole_shares():
    if SOLE is None or SOLE_STATS["planned"] == 0:   # (a blind run beside the mapped one has none)
        return
    n = SOLE_STATS["planned"]
    print(f"   sole mode (n_shift {SOLE['n_shift']}, step {SOLE['shift_step']:g} m, tolerance {SOLE['flat_tol']:g} m): of {SOLE_STATS['planned']} first footholds "
          f"sampled once per MPC call, accepted off the nominal place {SOLE_STATS['shifted'] / n:.3f}, levelled by the fallback {SOLE_STATS['levelled'] / n:.3f}")
    SOLE_STATS.update(planned=0, shifted=0, levelled=0)


def map_label(handed, scan, told):
    if scan is not None:
        reg = "the estimate" if scan.get("register_mode") else "the plant's position"
        return f"controller on the scanned map (noise {scan.get('noise', 0.0):g} m, range {scan.get('range', 0.0):g} m, dropout {scan.get('dropout', 0.0):g}, registered with {reg})"
    return told if handed else "controller blind"


def run_curb(params, heights, at, ticks, joint_model=None, riser_slope=np.sqrt(3.0), ground_map=False, scan=None):
    """One batch: instance i trots along +x across a curb (height > 0) or a step down (< 0) of heights[i] whose riser starts `at` ahead of the
    base origin of the start; ground_map: the controller is given the profile too -> (episode record, segment under the points and the base at the end, wall seconds of the ticks)."""
    B = len(heights)
    s = HunterSolver(params, batch=B, max_nodes=108)
    try:
        # fall_height 0.2, not the 0.3 of the other sweeps: the fall test is measured along the normal of the facet under the base origin,
        # and over a riser of slope sqrt(3) (n_z = 0.5) the standing height of 0.62 m reads 0.31 m
        loop = ResidentLoop(s, params, ["trot"] * B, np.tile([0.2, 0.0, 0.0, 0.0], (B, 1)), contact_config=dict(fall_height=0.2), joint_model=joint_model,
                            terrain=dict(profile=dict(dir=np.tile([1.0, 0.0], (B, 1)), knots=[curb_profile(h, at, riser_slope) for h in heights]), relative=True),
                            episode=dict(slip_speed=0.05), **map_args(ground_map, scan, "plant"))
        s.sync()
        t0 = time.perf_counter()
        run_ticks(loop, ticks)
        rec = loop.episode()
        wall = time.perf_counter() - t0
        return rec, s.plant_get_terrain_profile()["segment"], wall
    finally:
        s.close()


ROUGH_STEPS, ROUGH_CELL = 8, 0.05


def run_rough(params, robots, ticks, amp_max, joint_model=None, ground_map=False, scan=None):
    """One batch: instance i trots along +x over a rough field of its own (seed i) with bump amplitude amp_max * (i % 8) / 7, 32 x 32 nodes of
    5 cm, from 0.35 m behind the start to 1.2 m ahead of it; ground_map: the controller is given the field too (hb_ground_set_field)
    -> (amplitude per instance, episode record, wall seconds of the ticks)."""
    B = robots
    amp = amp_max * (np.arange(B) % ROUGH_STEPS) / (ROUGH_STEPS - 1)
    fields = [dict(dir=[1.0, 0.0], origin=[-0.35, -0.775], spacing=[ROUGH_CELL, ROUGH_CELL], heights=rough_field(i, amp[i], (ROUGH_CELL, ROUGH_CELL)))
              for i in range(B)]
    s = HunterSolver(params, batch=B, max_nodes=108)
    try:
        horizon = 100 * params["config"]["dt"]
        # (fall_height 0.2 as in run_curb: the fall test is measured along the normal of the facet under the base origin)
        loop = ResidentLoop(s, params, ["trot"] * B, np.tile([0.2, 0.0, 0.0, 0.0], (B, 1)), contact_config=dict(fall_height=0.2), joint_model=joint_model,
                            terrain=dict(field=fields, relative=True), static_schedule_until=ticks * 0.002 + horizon + 1.5, episode=dict(slip_speed=0.05),
                            **map_args(ground_map, scan, "field"))
        s.sync()
        t0 = time.perf_counter()
        run_ticks(loop, ticks)
        rec = loop.episode()
        return amp, rec, time.perf_counter() - t0
    finally:
        s.close()


def print_rough(amp, rec):
    """Per amplitude: robots, how many are up at the end, median end tick of those that fell, median of the largest tilt, mean slip ticks."""
    heads = ("amplitude", "robots", "up", "survival", "end med", "tiltmax med", "slipT mean", "nonfin")
    print("   " + " ".join(f"{h:>12}" for h in heads))
    for a in np.unique(amp):
        m = amp == a
        up = rec["END_TICK"][m] < 0
        fell = rec["END_TICK"][m][~up]
        cells = (f"{a:.4f}", f"{int(m.sum())}", f"{int(up.sum())}", f"{up.mean():.3f}", f"{int(np.median(fell))}" if len(fell) else "-",
                 f"{np.median(rec['TILT_MAX'][m]):.4g}", f"{rec['SLIP_TICKS'][m].mean():.1f}", f"{int((rec['FIRST_NONFINITE'][m] >= 0).sum())}")
        print("   " + " ".join(f"{c:>12}" for c in cells))


def run_respawn(params, mu, ticks, max_ticks, joint_model=None):
    """The friction sweep as repeated episodes -> (respawn totals, wall seconds of the ticks)."""
    s, loop = make_loop(params, mu, [0.0] * len(mu), ticks, False, joint_model,
                        respawn=dict(max_ticks=max_ticks, hold_ticks=0, place=1, clearance=0.0, yaw_range=0.1, joint_pos_sigma=0.005, seed=1))
    try:
        s.sync()
        t0 = time.perf_counter()
        loop.run(ticks)
        tot = loop.respawn_totals()
        return tot, time.perf_counter() - t0
    finally:
        s.close()


RANDOMIZE = dict(grade_max=0.15, mu_lo=0.05, mu_hi=0.8, payload_mass_max=3.0, payload_center=(0.0, 0.0, 0.15), payload_half_extent=(0.1, 0.05, 0.0),
                 push_force_max=40.0, push_start_lo=50, push_start_hi=150, push_ticks=25)
RANDOMIZE_RESPAWN = dict(hold_ticks=0, place=1, clearance=0.0, yaw_range=0.1, joint_pos_sigma=0.005, seed=1)


def run_randomize(params, robots, ticks, max_ticks, joint_model=None, host_driven=False):
    """Repeated episodes with a new scenario each -> (scenario log or None, respawn totals, wall seconds of the ticks).  host_driven: the
    host draws (numpy, not the device's stream) and calls hb_plant_set_terrain / hb_plant_set_model_variation after every respawn round and
    hb_plant_set_external_wrench before every tick."""
    channels = abi.HB_SC_SLOPE | abi.HB_SC_MU | abi.HB_SC_PAYLOAD | abi.HB_SC_PUSH
    log_capacity = min(abi.HB_SC_LOG_MAX, ticks // 8 + 1)
    scenario = None if host_driven else dict(RANDOMIZE, channels=channels, seed=2, log_capacity=log_capacity)
    B = robots
    s = HunterSolver(params, batch=B, max_nodes=108)
    try:
        horizon = 100 * params["config"]["dt"]
        loop = ResidentLoop(s, params, ["trot"] * B, np.tile([0.2, 0.0, 0.0, 0.0], (B, 1)), contact_config=dict(fall_height=0.3), joint_model=joint_model,
                            static_schedule_until=ticks * 0.002 + horizon + 1.5, episode=dict(slip_speed=0.05),
                            respawn=dict(RANDOMIZE_RESPAWN, max_ticks=max_ticks), scenario=scenario)
        rng = np.random.default_rng(2)
        s.sync()
        t0 = time.perf_counter()
        if not host_driven:
            loop.run(ticks)
            log = loop.scenario_log()
        else:
            R, push, start = RANDOMIZE, np.zeros((B, 6)), np.full(B, -1)
            for tick in range(ticks):
                steps = s.plant_episode()["STEPS"]
                w = np.where(((start >= 0) & (start <= steps) & (steps < start + R["push_ticks"]))[:, None], push, 0.0)
                s.plant_set_external_wrench(w)
                loop.step()
                if loop.tick % loop.mpc_every == 0:   # a respawn round has been enqueued: the host draws for everybody and uploads the batch
                    g = R["grade_max"] * rng.uniform(-1.0, 1.0, (B, 2))
                    n = np.concatenate([-g, np.ones((B, 1))], axis=1)
                    n /= np.linalg.norm(n, axis=1)[:, None]
                    s.plant_set_terrain(np.concatenate([n, np.zeros((B, 1))], axis=1), np.repeat(rng.uniform(R["mu_lo"], R["mu_hi"], (B, 1)), 4, axis=1))
                    pl = np.zeros((B, abi.HB_PAYLOAD_SIZE))
                    pl[:, 0] = R["payload_mass_max"] * rng.uniform(0.0, 1.0, B)
                    pl[:, 1:4] = np.asarray(R["payload_center"]) + np.asarray(R["payload_half_extent"]) * rng.uniform(-1.0, 1.0, (B, 3))
                    s.plant_set_model_variation(None, pl)
                    push[:, 0:2] = R["push_force_max"] * rng.uniform(-1.0, 1.0, (B, 2))
                    start = rng.integers(R["push_start_lo"], R["push_start_hi"] + 1, B)
            log = None
        tot = loop.respawn_totals()
        return log, tot, time.perf_counter() - t0
    finally:
        s.close()


RANDOM_CURBS = dict(kinds=abi.HB_PD_ALL, dir=(1.0, 0.0), height_lo=-0.03, height_hi=0.03, at_lo=0.05, at_hi=0.25, riser_slope=1.7, steps_lo=1,
                    steps_hi=4, run_lo=0.2, run_hi=0.3, mu_lo=0.7, mu_hi=0.7, seed=3)


def run_random_curbs(params, robots, ticks, max_ticks, joint_model=None, ground_map=False, scan=None):
    """Repeated episodes on a newly drawn ground each -> (log of the draw, respawn totals, wall seconds of the ticks)."""
    B = robots
    s = HunterSolver(params, batch=B, max_nodes=108)
    try:
        horizon = 100 * params["config"]["dt"]
        # (fall_height 0.2 as in run_curb: the fall test is measured along the normal of the facet under the base origin)
        loop = ResidentLoop(s, params, ["trot"] * B, np.tile([0.2, 0.0, 0.0, 0.0], (B, 1)), contact_config=dict(fall_height=0.2), joint_model=joint_model,
                            static_schedule_until=ticks * 0.002 + horizon + 1.5, episode=dict(slip_speed=0.05),
                            respawn=dict(RANDOMIZE_RESPAWN, max_ticks=max_ticks),
                            profile_draw=dict(RANDOM_CURBS, log_capacity=min(abi.HB_PD_LOG_MAX, ticks // 8 + 1)), **map_args(ground_map, scan, "draw"))
        s.sync()
        t0 = time.perf_counter()
        run_ticks(loop, ticks)
        log = loop.profile_draw_log()
        return log, loop.respawn_totals(), time.perf_counter() - t0
    finally:
        s.close()


def print_random_curbs(log, bins=3):
    """Survival rate (episodes that ended by time-out), median progress along the direction, median of the largest tilt and mean ticks by
    kind, and for curbs and stairs by height bin, from the log alone."""
    t = profile_draw_table(log)
    drawn = t["EPISODE"] > 0                       # (episode 0 ran on the level ground of the start, not on a draw)
    print(f"   {len(t['EPISODE'])} finished episodes logged, {int(drawn.sum())} of them on a drawn ground")
    survived = t["CAUSE"] == abi.HB_RS_TIMEOUT
    heads = ("kind", "height", "episodes", "survival", "progress med", "tiltmax med", "ticks")
    print("   " + " ".join(f"{h:>16}" for h in heads))

    def row(kind, label, m):
        # (medians: a robot that is lost can leave very large values at its last finite tick)
        cells = (kind, label, f"{int(m.sum())}") + ((f"{survived[m].mean():.3f}", f"{np.median(t['PROGRESS'][m]):.4f}", f"{np.median(t['TILT_MAX'][m]):.4f}",
                                                     f"{t['TICKS'][m].mean():.1f}") if m.any() else ("-",) * 4)
        print("   " + " ".join(f"{c:>16}" for c in cells))

    row("flat", "0", drawn & (t["KIND"] == abi.HB_PD_FLAT))
    for name, kind in (("curb", abi.HB_PD_CURB), ("stairs", abi.HB_PD_STAIRS)):
        of = drawn & (t["KIND"] == kind)
        if not of.any():
            row(name, "-", of)
            continue
        edges = np.linspace(t["HEIGHT"][of].min(), t["HEIGHT"][of].max(), bins + 1)
        which = np.clip(np.searchsorted(edges, t["HEIGHT"], side="right") - 1, 0, bins - 1)
        for b in range(bins):
            row(name, "[%.3g, %.3g]" % (edges[b], edges[b + 1]), of & (which == b))


# the grid of --rough (32 x 32 nodes of 5 cm, from 0.35 m behind the spawn point to 1.2 m ahead of it, centred across), bumps under the
# feet of the start too (calm = 0), tilts of up to 0.1 either way
RANDOM_ROUGH = dict(kinds=abi.HB_FD_ALL, dir=(1.0, 0.0), n_nodes=(32, 32), spacing=(ROUGH_CELL, ROUGH_CELL), centre=(0.35, 0.775), calm=0.0,
                    amp_lo=0.0, slope_u_lo=-0.1, slope_u_hi=0.1, slope_w_lo=-0.1, slope_w_hi=0.1, mu_lo=0.7, mu_hi=0.7, seed=4)


def run_random_rough(params, robots, ticks, max_ticks, amp_max, joint_model=None, ground_map=False, scan=None):
    """Repeated episodes on a newly composed height field each -> (log of the draw, respawn totals, wall seconds of the ticks, the largest
    amplitude drawn).  amp_max is cut to what the draw's slope bound admits on this grid beside the tilt: (0.1 + 2 A / 0.05)^2 * 2 <= 2.9
    gives A <= 0.0276 m (a seeded field of --rough is scaled down as a whole instead)."""
    B = robots
    amp_max = min(amp_max, 0.999 * (np.sqrt(2.9 / 2.0) - RANDOM_ROUGH["slope_u_hi"]) * ROUGH_CELL / 2.0)
    s = HunterSolver(params, batch=B, max_nodes=108)
    try:
        horizon = 100 * params["config"]["dt"]
        # (fall_height 0.2 as in run_curb: the fall test is measured along the normal of the facet under the base origin)
        loop = ResidentLoop(s, params, ["trot"] * B, np.tile([0.2, 0.0, 0.0, 0.0], (B, 1)), contact_config=dict(fall_height=0.2), joint_model=joint_model,
                            static_schedule_until=ticks * 0.002 + horizon + 1.5, episode=dict(slip_speed=0.05),
                            respawn=dict(RANDOMIZE_RESPAWN, max_ticks=max_ticks),
                            field_draw=dict(RANDOM_ROUGH, amp_hi=amp_max, log_capacity=min(abi.HB_FD_LOG_MAX, ticks // 8 + 1)),
                            **map_args(ground_map, scan, "draw"))
        s.sync()
        t0 = time.perf_counter()
        run_ticks(loop, ticks)
        log = loop.field_draw_log()
        return log, loop.respawn_totals(), time.perf_counter() - t0, amp_max
    finally:
        s.close()


def print_random_rough(log, bins=4):
    """Survival rate (episodes that ended by time-out), median progress along the direction, median of the largest tilt and mean ticks by
    kind, and for the two rough kinds by amplitude bin, from the log alone."""
    t = field_draw_table(log)
    drawn = t["EPISODE"] > 0                       # (episode 0 ran on the level field of the start, not on a draw)
    print(f"   {len(t['EPISODE'])} finished episodes logged, {int(drawn.sum())} of them on a drawn field")
    survived = t["CAUSE"] == abi.HB_RS_TIMEOUT
    heads = ("kind", "amplitude", "episodes", "survival", "progress med", "tiltmax med", "ticks")
    print("   " + " ".join(f"{h:>16}" for h in heads))

    def row(kind, label, m):
        # (medians: a robot that is lost can leave very large values at its last finite tick)
        cells = (kind, label, f"{int(m.sum())}") + ((f"{survived[m].mean():.3f}", f"{np.median(t['PROGRESS'][m]):.4f}", f"{np.median(t['TILT_MAX'][m]):.4f}",
                                                     f"{t['TICKS'][m].mean():.1f}") if m.any() else ("-",) * 4)
        print("   " + " ".join(f"{c:>16}" for c in cells))

    row("flat", "0", drawn & (t["KIND"] == abi.HB_FD_FLAT))
    row("tilt", "0", drawn & (t["KIND"] == abi.HB_FD_TILT))
    for name, kind in (("rough", abi.HB_FD_ROUGH), ("tilt + rough", abi.HB_FD_TILT_ROUGH)):
        of = drawn & (t["KIND"] == kind)
        if not of.any():
            row(name, "-", of)
            continue
        edges = np.linspace(t["AMPLITUDE"][of].min(), t["AMPLITUDE"][of].max(), bins + 1)
        which = np.clip(np.searchsorted(edges, t["AMPLITUDE"], side="right") - 1, 0, bins - 1)
        for b in range(bins):
            row(name, "[%.3g, %.3g]" % (edges[b], edges[b + 1]), of & (which == b))


def print_randomize(log, bins=4):
    """Survival rate (episodes that ended by time-out) and mean ticks, binned by mu, |grade| and payload mass, from the log alone."""
    t = scenario_table(log)
    drawn = t["EPISODE"] > 0                       # (episode 0 ran on the terrain and the model of the start, not on a draw)
    n = int(drawn.sum())
    print(f"   {len(t['EPISODE'])} finished episodes logged, {n} of them on a drawn scenario")
    survived, ticks = (t["CAUSE"] == abi.HB_RS_TIMEOUT)[drawn], t["TICKS"][drawn]
    for name, x in (("mu", t["MUS"][drawn, 0]), ("|grade|", np.hypot(t["GRADE"][drawn, 0], t["GRADE"][drawn, 1])), ("payload kg", t["PAYLOAD_M"][drawn])):
        if n == 0:
            break
        edges = np.linspace(x.min(), x.max(), bins + 1)
        which = np.clip(np.searchsorted(edges, x, side="right") - 1, 0, bins - 1)
        print(f"   {name:>12} " + " ".join(f"{'[%.3g, %.3g]' % (edges[b], edges[b + 1]):>16}" for b in range(bins)))
        for label, val in (("episodes", lambda m: f"{int(m.sum())}"), ("survival", lambda m: f"{survived[m].mean():.3f}" if m.any() else "-"),
                           ("mean ticks", lambda m: f"{ticks[m].mean():.1f}" if m.any() else "-")):
            print(f"   {label:>12} " + " ".join(f"{val(which == b):>16}" for b in range(bins)))


def run_record(params, mu, pitch, ticks, static=False, joint_model=None, payload=None):
    """-> (episode record, wall seconds of the ticks)."""
    s, loop = make_loop(params, mu, pitch, ticks, static, joint_model, payload)
    try:
        s.sync()
        t0 = time.perf_counter()
        loop.run(ticks)
        rec = loop.episode()
        return rec, time.perf_counter() - t0
    finally:
        s.close()


def run_readback(params, mu, pitch, ticks, joint_model=None):
    """The loop of the earlier findings: three synchronising getters after every tick, reduced in numpy -> (figures, wall seconds)."""
    s, loop = make_loop(params, mu, pitch, ticks, False, joint_model)
    try:
        plane = s.plant_get_terrain()["plane"]
        B = len(mu)
        slip_ticks, first_slip, fall = np.zeros(B, dtype=int), np.full(B, -1), np.full(B, -1)
        s.sync()
        t0 = time.perf_counter()
        for tick in range(ticks):
            loop.step()
            st, con, _ = s.plant_state(), s.plant_contact(), s.plant_get_joints()
            pv = con["point_vel"]
            vn = np.einsum("bcx,bx->bc", pv, plane[:, :3])
            with np.errstate(over="ignore", invalid="ignore"):
                speed = np.linalg.norm(pv - vn[:, :, None] * plane[:, None, :3], axis=2)
            slipping = ((speed > 0.05) & (con["touching"] != 0)).any(axis=1) & (fall < 0)
            slip_ticks += slipping
            first_slip = np.where((first_slip < 0) & slipping, tick, first_slip)
            fall = np.where((fall < 0) & ((con["status"] & abi.HB_CONTACT_FALLEN) != 0), tick, fall)
        wall = time.perf_counter() - t0
        return dict(slip_ticks=slip_ticks, first_slip=first_slip, fall=fall, z=st["q"][:, 2]), wall
    finally:
        s.close()


def table(label, values, rec, dt=0.002):
    """One row per instance; %g columns, since a robot that is lost can leave very large values at its last finite tick."""
    summ = episode_summary(rec, dt=dt)
    heads = (label, "end", "cause", "nonfin", "z", "height", "tilt", "tiltmax", "dist_x", "speed", "slipT", "first", "slipmax", "wbcF", "first", "taumax", "duty")
    print(" ".join(f"{h:>10}" for h in heads))
    for i, val in enumerate(values):
        base = rec["LAST_BASE"][i]
        row = (val, int(rec["END_TICK"][i]), CAUSE[int(rec["END_CAUSE"][i])], int(rec["FIRST_NONFINITE"][i]), base[2], rec["HEIGHT_LAST"][i],
               max(abs(base[4]), abs(base[5])), rec["TILT_MAX"][i], summ["distance_x"][i], summ["mean_speed"][i], int(rec["SLIP_TICKS"][i]),
               int(rec["FIRST_SLIP"][i]), rec["SLIP_SPEED_MAX"][i], int(rec["WBC_FAIL_TICKS"][i]), int(rec["FIRST_WBC_FAIL"][i]), rec["TAU_MAX"][i].max(),
               summ["duty_factor"][i].mean())
        print(" ".join(f"{x:>10}" if isinstance(x, (str, int)) else f"{x:10.4g}" for x in row))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ticks", type=int, default=600)
    ap.add_argument("--grid", type=int, nargs=2, metavar=("N_MU", "N_SLOPE"), help="friction 0.05 .. 0.7 x pitch 0 .. 0.1 rad, one instance per pair")
    ap.add_argument("--payload", type=int, nargs=2, metavar=("N_MASS", "N_OFFSET"),
                    help="payload mass 0 .. 15 kg x fore-aft offset -0.1 .. 0.1 m at 0.15 m above the base origin, one instance per pair")
    ap.add_argument("--joint-model", action="store_true", help="the joints of the reference's MuJoCo model instead of ideal joints")
    ap.add_argument("--respawn", type=int, metavar="N_TICKS", help="the friction sweep as repeated episodes of at most N_TICKS ticks, from the respawn totals")
    ap.add_argument("--randomize", type=int, metavar="N_TICKS", help="N_TICKS ticks of repeated episodes with slope, friction, payload and a push drawn on the device per episode; one read-back")
    ap.add_argument("--random-curbs", type=int, metavar="N_TICKS", help="N_TICKS ticks of repeated episodes on level ground, a curb / step-down or stairs drawn on the device per episode; one read-back")
    ap.add_argument("--random-rough", type=int, metavar="N_TICKS", help="N_TICKS ticks of repeated episodes on a level, rough, tilted or rough and tilted height field composed on the device per episode (bump amplitude up to --rough-max); one read-back")
    ap.add_argument("--robots", type=int, default=64, help="batch of --randomize / --random-curbs / --random-rough / --rough")
    ap.add_argument("--max-ticks", type=int, default=400, help="time-out of an episode of --randomize / --random-curbs")
    ap.add_argument("--host-driven", action="store_true", help="--randomize with the host calling the setters per respawn round and uploading a wrench per tick")
    ap.add_argument("--curb", action="store_true", help="one curb / step-down height per robot (0, 1, 2, 3 cm down and up), trot across it; from the episode record alone")
    ap.add_argument("--ground-map", action="store_true", help="--curb with the controller's ground map set to the plant's profile (hb_ground_set_profile); --random-curbs with the map following every drawn ground; --rough a second time with the plant's field as the controller's field map (hb_ground_set_field)")
    ap.add_argument("--curb-at", type=float, default=0.08, help="where the riser of --curb starts, metres ahead of the base origin of the start")
    ap.add_argument("--riser-slope", type=float, default=float(np.sqrt(3.0)), help="slope of the riser of --curb (at most sqrt(3))")
    ap.add_argument("--rough", type=int, metavar="N_TICKS", help="N_TICKS ticks on a seeded rough height field per robot, bump amplitude 0 .. --rough-max over the batch (--robots); one read-back")
    ap.add_argument("--rough-max", type=float, default=0.035, help="largest bump amplitude of --rough, metres")
    ap.add_argument("--readback", action="store_true", help="also time the per-tick read-back loop on the two sweeps")
    ap.add_argument("--scan", action="store_true", help="--random-rough / --random-curbs / --rough / --curb with the controller on a field map PERCEIVED from the plant's ground on the device (hb_plant_set_height_scan: 32 x 32 nodes of 5 cm carried with the robot), between blind and --ground-map")
    ap.add_argument("--scan-noise", type=float, default=0.0, metavar="S", help="standard deviation of the height noise per return of --scan, metres")
    ap.add_argument("--scan-range", type=float, default=0.0, metavar="R", help="range of --scan, metres from the base (0: no limit)")
    ap.add_argument("--scan-dropout", type=float, default=0.0, metavar="P", help="probability that a return of --scan is lost")
    ap.add_argument("--scan-register", action="store_true", help="--scan registered with the estimated base position instead of the plant's")
    ap.add_argument("--sole", action="store_true", help="--ground-map / --scan with the toe and the heel of a foot planned as one sole (hb_ground_set_foothold); prints the shares of first footholds shifted and levelled from the choice read-back, sampled once per MPC call: every sample is a synchronising read-back, so the ms per tick printed for a --sole run includes the sampling and is not comparable with a run without --sole")
    ap.add_argument("--sole-shift", type=int, default=3, metavar="N", help="candidates of --sole to either side of the nominal foothold (unmeasured default)")
    ap.add_argument("--sole-step", type=float, default=0.02, metavar="S", help="distance between candidates of --sole, metres (unmeasured default)")
    ap.add_argument("--sole-tol", type=float, default=0.005, metavar="T", help="largest defect of a sole --sole takes for flat, metres (unmeasured default)")
    args = ap.parse_args()
    if args.sole and not (args.ground_map or args.scan):
        ap.error("--sole acts on the controller's map: give --ground-map or --scan as well")
    if args.sole:
        global SOLE
        SOLE = dict(mode="sole", n_shift=args.sole_shift, shift_step=args.sole_step, flat_tol=args.sole_tol)
    if args.scan and args.ground_map:
        ap.error("--scan and --ground-map: one source of the controller's map at a time")
    if args.scan and not (args.curb or args.rough or args.random_rough or args.random_curbs):
        ap.error("--scan goes with --random-rough, --random-curbs, --rough or --curb")
    scan = dict(noise=args.scan_noise, range=args.scan_range, dropout=args.scan_dropout, register_mode=1 if args.scan_register else 0) if args.scan else None
    params = ingest.load_packaged()
    jm = {} if args.joint_model else None
    if args.curb:
        rec, seg, wall = run_curb(params, CURBS, args.curb_at, args.ticks, joint_model=jm, riser_slope=args.riser_slope, ground_map=args.ground_map, scan=scan)
        print(f"-- curb sweep, {map_label(args.ground_map, scan, 'controller on the ground map')}, B = {len(CURBS)}, riser of slope {args.riser_slope:.3g} {args.curb_at} m ahead, {args.ticks} ticks, run(): {1e3 * wall / args.ticks:.3f} ms per tick")
        table("height", CURBS, rec)
        print("   segment under the four contact points and the base at the end (0 before the riser, 1 on it, 2 beyond):", seg.tolist())
        print_sole_shares()
        return
    for mapped in ([False, True] if args.ground_map else [False]) if args.rough else []:   # (--ground-map: the same rows next to the blind ones)
        amp, rec, wall = run_rough(params, args.robots, args.rough, args.rough_max, joint_model=jm, ground_map=mapped, scan=scan)
        print(f"-- rough ground, {map_label(mapped, scan, 'controller on the field map')}, {'joint model' if args.joint_model else 'ideal joints'}, "
              f"B = {args.robots}, {args.rough} ticks, run() and one read-back: {wall:.3f} s, {1e3 * wall / args.rough:.3f} ms per tick")
        print_rough(amp, rec)
        print_sole_shares()
    if args.rough:
        return
    if args.random_rough:
        log, tot, wall, amp = run_random_rough(params, args.robots, args.random_rough, args.max_ticks, args.rough_max, joint_model=jm, ground_map=args.ground_map, scan=scan)
        print(f"-- a height field composed per episode, {map_label(args.ground_map, scan, 'controller on the field map that follows')}, "
              f"{'joint model' if args.joint_model else 'ideal joints'}, B = {args.robots}, {args.random_rough} ticks, episodes of at most {args.max_ticks} "
              f"ticks, bump amplitude up to {amp:.4f} m, run() and one read-back: {wall:.3f} s, {1e3 * wall / args.random_rough:.3f} ms per tick")
        print(f"   episodes {int(tot['EPISODES'].sum())}: fallen {int(tot['N_FALLEN'].sum())}, non-finite {int(tot['N_NONFINITE'].sum())}, timed out {int(tot['N_TIMEOUT'].sum())}")
        print_random_rough(log)
        print_sole_shares()
        return
    if args.random_curbs:
        log, tot, wall = run_random_curbs(params, args.robots, args.random_curbs, args.max_ticks, joint_model=jm, ground_map=args.ground_map, scan=scan)
        print(f"-- a ground drawn per episode, {map_label(args.ground_map, scan, 'controller on the map that follows')}, "
              f"{'joint model' if args.joint_model else 'ideal joints'}, B = {args.robots}, {args.random_curbs} ticks, episodes of at most {args.max_ticks} "
              f"ticks, run() and one read-back: {wall:.3f} s, {1e3 * wall / args.random_curbs:.3f} ms per tick")
        print(f"   episodes {int(tot['EPISODES'].sum())}: fallen {int(tot['N_FALLEN'].sum())}, non-finite {int(tot['N_NONFINITE'].sum())}, timed out {int(tot['N_TIMEOUT'].sum())}")
        print_random_curbs(log)
        print_sole_shares()
        return
    if args.randomize:
        log, tot, wall = run_randomize(params, args.robots, args.randomize, args.max_ticks, joint_model=jm, host_driven=args.host_driven)
        print(f"-- randomised scenarios per episode, B = {args.robots}, {args.randomize} ticks, episodes of at most {args.max_ticks} ticks, "
              f"{'host-driven' if args.host_driven else 'run() and one read-back'}: {wall:.3f} s, {1e3 * wall / args.randomize:.3f} ms per tick")
        print(f"   episodes {int(tot['EPISODES'].sum())}: fallen {int(tot['N_FALLEN'].sum())}, non-finite {int(tot['N_NONFINITE'].sum())}, timed out {int(tot['N_TIMEOUT'].sum())}")
        if log is not None:
            print_randomize(log)
        return
    if args.respawn:
        tot, wall = run_respawn(params, FRICTION, args.ticks, args.respawn, joint_model=jm)
        summ = respawn_summary(tot, dt=0.002)
        print(f"-- friction sweep as repeated episodes of at most {args.respawn} ticks, B = {len(FRICTION)}, {args.ticks} ticks, run(): "
              f"{1e3 * wall / args.ticks:.3f} ms per tick")
        heads = ("mu", "episodes", "fallen", "nonfin", "timeout", "fall_rate", "mean_ticks", "mean_s", "dist_x", "tiltmax", "taumax")
        print(" ".join(f"{h:>10}" for h in heads))
        for i, m in enumerate(FRICTION):
            row = (m, int(tot["EPISODES"][i]), int(tot["N_FALLEN"][i]), int(tot["N_NONFINITE"][i]), int(tot["N_TIMEOUT"][i]), summ["fall_rate"][i],
                   summ["mean_ticks"][i], summ["mean_time"][i], summ["mean_distance_x"][i], tot["TILT_MAX"][i], tot["TAU_MAX"][i])
            print(" ".join(f"{x:>10}" if isinstance(x, int) else f"{x:10.4g}" for x in row))
        return
    if args.payload:
        n_m, n_x = args.payload
        masses, offsets = np.linspace(0.0, 15.0, n_m), np.linspace(-0.1, 0.1, n_x)
        mass, off = np.repeat(masses, n_x), np.tile(offsets, n_m)
        B = len(mass)
        pos = np.stack([off, np.zeros(B), np.full(B, 0.15)], axis=1)
        rec, wall = run_record(params, [0.7] * B, [0.0] * B, args.ticks, static=True, joint_model=jm, payload=payload_on_base(mass, pos))
        up = (rec["END_TICK"] < 0).reshape(n_m, n_x)
        print(f"payload {n_m} x {n_x} = {B} instances, {args.ticks} ticks: {wall:.2f} s wall, {1e3 * wall / args.ticks:.3f} ms per tick; "
              f"{int(up.sum())} instances up at the end, {int((rec['FIRST_NONFINITE'] >= 0).sum())} went non-finite")
        print("survivors per offset column", np.round(offsets, 3).tolist(), "(of", n_m, "masses):", up.sum(axis=0).tolist())
        print("survivors per mass row", np.round(masses, 2).tolist(), "(of", n_x, "offsets):", up.sum(axis=1).tolist())
        if B <= 64:
            table("mass/off", [f"{m:.3g}/{x:+.2g}" for m, x in zip(mass, off)], rec)
        else:   # per mass row: the figures of the instances still up, else of all
            heads = ("mass", "up", "height", "tiltmax", "taumax", "wbcF")
            print(" ".join(f"{h:>10}" for h in heads))
            for k, m in enumerate(masses):
                sel = np.arange(k * n_x, (k + 1) * n_x)
                sel = sel[up[k]] if up[k].any() else sel
                row = (m, int(up[k].sum()), np.median(rec["HEIGHT_LAST"][sel]), rec["TILT_MAX"][sel].max(), rec["TAU_MAX"][sel].max(),
                       int(rec["WBC_FAIL_TICKS"][sel].max()))
                print(" ".join(f"{x:>10}" if isinstance(x, int) else f"{x:10.4g}" for x in row))
        return
    if args.grid:
        n_mu, n_sl = args.grid
        mus, slopes = np.linspace(0.05, 0.7, n_mu), np.linspace(0.0, 0.1, n_sl)
        mu, pitch = np.repeat(mus, n_sl), np.tile(slopes, n_mu)
        rec, wall = run_record(params, mu, pitch, args.ticks, static=True, joint_model=jm)
        up = (rec["END_TICK"] < 0).reshape(n_mu, n_sl)
        end = np.where(rec["END_TICK"] < 0, args.ticks, rec["END_TICK"]).reshape(n_mu, n_sl)
        print(f"grid {n_mu} x {n_sl} = {len(mu)} instances, {args.ticks} ticks: {wall:.2f} s wall, {1e3 * wall / args.ticks:.3f} ms per tick; "
              f"{int(up.sum())} instances up at the end, {int((rec['FIRST_NONFINITE'] >= 0).sum())} went non-finite")
        print("survivors per slope column (of", n_mu, "friction values):", up.sum(axis=0).tolist())
        print("survivors per friction row (of", n_sl, "slopes):", up.sum(axis=1).tolist())
        print("median end tick per slope column:", np.median(end, axis=0).astype(int).tolist())
        print("median end tick per friction row:", np.median(end, axis=1).astype(int).tolist())
        return
    for name, mu, pitch, values in (("friction", FRICTION, [0.0] * len(FRICTION), FRICTION), ("slope", [0.7] * len(SLOPES), SLOPES, SLOPES)):
        rec, wall = run_record(params, mu, pitch, args.ticks, joint_model=jm)
        print(f"-- {name} sweep, B = {len(mu)}, {args.ticks} ticks, run(): {1e3 * wall / args.ticks:.3f} ms per tick")
        table("mu" if name == "friction" else "pitch", values, rec)
        if args.readback:
            fig, wall_rb = run_readback(params, mu, pitch, args.ticks, joint_model=jm)
            print(f"   per-tick read-back loop: {1e3 * wall_rb / args.ticks:.3f} ms per tick; slip ticks {fig['slip_ticks'].tolist()} first {fig['first_slip'].tolist()} "
                  f"fall {fig['fall'].tolist()}")


if __name__ == "__main__":
    main()
