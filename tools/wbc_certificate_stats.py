#!/usr/bin/env python3
"""Distribution of the WeightedWbc KKT certificate (hb_wbc_set_certificate) over BASELINE configs[2]'s batch
(4096 distinct trotting instances, N = 100, tables generated on the device): median / p99 / max of r_stat / scale and the other
residuals after `--steps` resident steps, with the regularisation step (the rule) and without it (`--reg-steps 0`).  `--off` runs the
same steps with the certificate off (for a kernel-trace comparison of k_wbc and k_wbc_cert).
python tools/wbc_certificate_stats.py [--batch B] [--nodes N] [--steps K] [--chunks C] [--reg-steps R] [--off]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from hunter_bipedal_control_amd import ingest, workload
from hunter_bipedal_control_amd.solver import HunterSolver

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--nodes", type=int, default=100)
ap.add_argument("--steps", type=int, default=1)
ap.add_argument("--chunks", type=int, default=4)
ap.add_argument("--reg-steps", type=int, default=1)
ap.add_argument("--off", action="store_true")
args = ap.parse_args()
P = ingest.load_packaged()
s = HunterSolver(P, batch=args.batch, max_nodes=args.nodes, wbc_reg_steps=args.reg_steps)
try:
    w = workload.device_trot_batch(s, P, n_intervals=args.nodes)
    s.set_resident_inputs(w["x0"], w["t_now"], w["rbd"])
    s.set_chunks(args.chunks)
    if not args.off:
        s.wbc_set_certificate(True)
    for _ in range(args.steps):
        s.step_resident()
    _, status = s.get_wbc_solution()
    out = dict(batch=args.batch, nodes=args.nodes, steps=args.steps, chunks=args.chunks, reg_steps=args.reg_steps, certificate=not args.off,
               wbc_status_max=int(status.max()))
    if not args.off:
        c = s.wbc_certificate()
        pct = lambda a: dict(median=float(np.median(a)), p99=float(np.percentile(a, 99)), max=float(a.max()))
        out.update(r_stat_rel=pct(c["r_stat"] / c["scale"]), r_dual_rel=pct(c["r_dual"] / c["scale"]), r_comp_rel=pct(c["r_comp"] / c["scale"]),
                   r_eq=pct(c["r_eq"]), r_in=pct(c["r_in"]), scale=pct(c["scale"]), n_active=pct(c["n_active"].astype(float)),
                   above_1e8_rel=int((c["r_stat"] > 1e-8 * c["scale"]).sum()))
finally:
    s.close()
print(json.dumps(out))
