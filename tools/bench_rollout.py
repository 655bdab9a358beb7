"""Closed-loop rollout throughput: 4096 robots trotting under their own commands, everything (reference generation, SQP,
WBC, joint command, plant stub) on the device.  Run on the GPU box:  python tools/bench_rollout.py [ticks] [--estimator [--noise]]

--estimator: the observation is the state estimator's, fed by the plant's sensor model on the device (hb_plant_sense +
hb_estimator_update_resident) instead of the plant's true state; --noise adds seeded noise on every sensor channel."""
import argparse
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
from hunter_bipedal_control_amd import abi, ingest
from hunter_bipedal_control_amd.rollout import ResidentLoop
from hunter_bipedal_control_amd.solver import HunterSolver

ap = argparse.ArgumentParser()
ap.add_argument("ticks", nargs="?", type=int, default=400)
ap.add_argument("--estimator", action="store_true", help="close the loop through hb_plant_sense + hb_estimator_update_resident")
ap.add_argument("--noise", action="store_true", help="with --estimator: seeded noise on every sensor channel")
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()
if args.noise and not args.estimator:
    ap.error("--noise belongs to --estimator")

P = ingest.load_packaged()
B = 4096
ticks = args.ticks
rng = np.random.default_rng(0)
cmd = np.stack([[rng.uniform(0.05, 0.3), rng.uniform(-0.08, 0.08), 0.0, rng.uniform(-0.3, 0.3)] for _ in range(B)])
s = HunterSolver(P, batch=B, max_nodes=108)
extra = {}
if args.estimator:
    extra["use_estimator"] = True
    if args.noise:   # a consumer-grade IMU and 14-bit encoders, roughly
        extra["sensor_config"] = abi.make_sensor_config(seed=args.seed, orientation_noise=2e-3, gyro_noise=5e-3, accel_noise=5e-2,
                                                        joint_pos_noise=4e-4, joint_vel_noise=2e-2, joint_torque_noise=0.1)
loop = ResidentLoop(s, P, ["trot"] * B, cmd, static_schedule_until=12.0, **extra)
for _ in range(16):
    loop.step()
s.sync()
t0 = time.perf_counter()
for _ in range(ticks):
    loop.step()
s.sync()
el = time.perf_counter() - t0
st = s.plant_state()
q = st["q"]
up = (np.abs(q[:, 2] - 0.63) < 0.05) & (np.abs(q[:, 4:6]).max(axis=1) < 0.2)
what = "" if not args.estimator else (" [estimator in the loop, noisy sensors]" if args.noise else " [estimator in the loop, ideal sensors]")
print(f"rollout{what}: {B} robots x {ticks} control ticks (dt 2 ms, MPC every 8 ticks) in {el:.2f} s = {B * ticks / el:.0f} robot-ticks/s = "
      f"{ticks * 0.002 / el:.3f} x real time for the whole batch; upright {int(up.sum())}/{B}; mean x progress {q[:, 0].mean():.3f} m "
      f"(mean command {cmd[:, 0].mean():.3f} m/s over {loop.t - 0.3:.2f} s of gait)")
if args.estimator:
    xh, _ = s.estimator_filter()
    print(f"filter error at the end: base position max {np.abs(xh[:, 0:3] - q[:, 0:3]).max():.4f} m, "
          f"base velocity max {np.abs(xh[:, 3:6] - st['v'][:, 0:3]).max():.4f} m/s")
s.close()
