#!/usr/bin/env python3
"""Cost of the device-resident gait manager: one JSON line per figure.

    python tools/bench_gait.py [--lib path/to/other/libhunter_hip.so] [--batch 4096] [--nodes 100] [--ticks 40] [--what tick,pass,host]

  tick  hb_tick_resident on four instance ranges, updates/s, with the manager on (`gait`) and on the schedule uploaded once (`static`).
        With --lib pointing at a build of a commit without the manager only `static` runs: the yardstick is that build on the same
        machine in the same session.
  pass  the enqueue-only hb_refgen_update with the manager on and off; the difference per pass is k_gait (rocprofv3 --kernel-trace
        --stats on this tool gives the kernel's own row).
  host  host wall time per MPC call of the host schedule path of rollout.ResidentLoop (one schedule_window per instance plus
        hb_refgen_set_schedule) at the same batch: the work the manager removes.
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np

from hunter_bipedal_control_amd import abi, gait, ingest, workload
from hunter_bipedal_control_amd import solver as _solver_mod

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--nodes", type=int, default=100)
ap.add_argument("--ticks", type=int, default=40)
ap.add_argument("--what", default="tick,pass,host")
args = ap.parse_args()
if args.lib:  # another build (tools only; the product loader has no override)
    _solver_mod._LIB_PATH = Path(args.lib).resolve()
from hunter_bipedal_control_amd.solver import HunterSolver  # noqa: E402

P = ingest.load_packaged()
B, N = args.batch, args.nodes
has_gait = hasattr(_solver_mod.load_library(), "hb_gait_reset")
what = args.what.split(",")


def _setup(estimator):
    s = HunterSolver(P, batch=B, max_nodes=N + 8)
    w = workload.device_trot_batch(s, P, n_intervals=N)
    s.set_resident_inputs(w["x0"], w["t_now"], w["rbd"])
    if estimator:
        xh0 = np.zeros((B, 18))
        xh0[:, 0:3] = w["rbd"][:, 3:6]
        xh0[:, 6:18] = np.asarray(s.eval_foot_kinematics(w["x0"], np.zeros((B, 22)))[0]).reshape(B, 12)
        s.estimator_reset(abi.make_estimator_config(P), xh0)
    return s, w


def tick(manager):
    s, w = _setup(True)
    if manager:
        s.gait_reset(abi.make_gait_config(P))
    s.set_chunks(4)
    rbd = w["rbd"]
    quat, z3, acc = np.tile([0.0, 0.0, 0.0, 1.0], (B, 1)), np.zeros((B, 3)), np.tile([0.0, 0.0, 9.81], (B, 1))
    contact = np.ones((B, 4), dtype=np.int32)
    qj, qdj = np.ascontiguousarray(rbd[:, 6:16]), np.ascontiguousarray(rbd[:, 22:32])
    t, warm = w["t_now"].copy(), 10
    for k in range(warm):
        s.tick_resident(0.002, quat, z3, acc, qj, qdj, contact, t + 0.01 * k, w["horizon"], w["cmd"])
    s.sync()
    t0 = time.perf_counter()
    for k in range(args.ticks):
        s.tick_resident(0.002, quat, z3, acc, qj, qdj, contact, t + 0.01 * (warm + k), w["horizon"], w["cmd"])
    s.sync()
    el = time.perf_counter() - t0
    out = dict(figure="tick", schedule="gait" if manager else "static", batch=B, nodes=N, ranges=4, ms_per_tick=round(1e3 * el / args.ticks, 3),
               updates_per_s=round(B * args.ticks / el), refgen_status_max=int(s.refgen_status().max()), mpc_status_max=int(s.mpc_status().max()))
    if manager:
        st = s.gait_state()
        out.update(levels=np.bincount(st["level"], minlength=4).tolist(), gait_status_max=int(st["status"].max()))
    s.close()
    return out


def refgen_pass(manager, passes=100):
    s, w = _setup(False)
    if manager:
        s.gait_reset(abi.make_gait_config(P))
    t = np.full(B, 0.1)
    for k in range(10):
        s.refgen_update(t + 0.01 * k, w["horizon"], w["x0"], w["cmd"], want_status=False)
    s.sync()
    t0 = time.perf_counter()
    for k in range(passes):
        s.refgen_update(t + 0.01 * (10 + k), w["horizon"], None, w["cmd"], want_status=False)
    s.sync()
    el = time.perf_counter() - t0
    s.close()
    return 1e3 * el / passes


def host_schedule_path(calls=5):
    s, w = _setup(False)
    schedules = [gait.gait_schedule(P, "trot", 0.3, 60.0) for _ in range(B)]   # as rollout.ResidentLoop builds them
    horizon, t, el = w["horizon"], 0.1, []
    for _ in range(calls):
        t0 = time.perf_counter()
        s.refgen_set_schedule([gait.schedule_window(ms, t - 1.0, t + horizon + 1.5) for ms in schedules])
        el.append(time.perf_counter() - t0)
        t += 0.016
    s.close()
    return dict(figure="host", batch=B, host_ms_per_mpc_call=round(1e3 * float(np.median(el)), 2))


if "tick" in what:
    print(json.dumps(dict(lib=args.lib or "default", **tick(False))), flush=True)
    if has_gait:
        print(json.dumps(dict(lib=args.lib or "default", **tick(True))), flush=True)
if "pass" in what and has_gait:
    off, on = refgen_pass(False), refgen_pass(True)
    print(json.dumps(dict(figure="pass", batch=B, nodes=N, refgen_ms_per_pass_off=round(off, 4), refgen_ms_per_pass_on=round(on, 4),
                          k_gait_ms_per_pass=round(on - off, 4))), flush=True)
if "host" in what:
    print(json.dumps(host_schedule_path()), flush=True)
