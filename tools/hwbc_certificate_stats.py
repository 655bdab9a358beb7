#!/usr/bin/env python3
"""Distribution of the per-level certificate of the HierarchicalWbc cascade (hb_hwbc_set_certificate) over one
GPU's share of BASELINE configs[4] (1024 distinct trotting instances, N = 200, tables generated on the device, bench.py's instance
ranges): per level the median / p99 / max of every figure after `--steps` resident steps, with the regularisation step (the rule) and
without it (`--reg-steps 0`).  `--oracle` adds the same figures of the CPU oracle's own cascade on the WBC inputs of the last step (the
reference values of a certified instance, tests/_hwbc_cert.py) and the number of instances outside 10 x its worst.  `--off` runs the
same steps with the certificate off (for a kernel-trace comparison of k_hwbc and k_hwbc_cert).
python tools/hwbc_certificate_stats.py [--batch B] [--nodes N] [--steps K] [--chunks C] [--reg-steps R] [--oracle] [--off]"""
import argparse, json, os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import bench
from hunter_bipedal_control_amd import ingest, workload
from hunter_bipedal_control_amd.solver import HunterSolver

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--nodes", type=int, default=200)
ap.add_argument("--steps", type=int, default=1)
ap.add_argument("--chunks", type=int, default=0, help="instance ranges (0: bench.py's choice for the batch)")
ap.add_argument("--reg-steps", type=int, default=1)
ap.add_argument("--oracle", action="store_true")
ap.add_argument("--off", action="store_true")
args = ap.parse_args()
P = ingest.load_packaged()
chunks = args.chunks or bench.default_chunks(args.batch)
s = HunterSolver(P, batch=args.batch, max_nodes=args.nodes, wbc_type=1, wbc_reg_steps=args.reg_steps)
try:
    w = workload.device_trot_batch(s, P, n_intervals=args.nodes)
    s.set_resident_inputs(w["x0"], w["t_now"], w["rbd"])
    s.set_chunks(chunks)
    if not args.off:
        s.hwbc_set_certificate(True)
    for _ in range(args.steps):
        s.step_resident()
    _, status = s.get_wbc_solution()
    out = dict(batch=args.batch, nodes=args.nodes, steps=args.steps, chunks=chunks, reg_steps=args.reg_steps, certificate=not args.off,
               wbc_status_max=int(status.max()))
    if not args.off:
        c = s.hwbc_certificate()
        pct = lambda a: [dict(median=float(np.median(a[:, k])), p99=float(np.percentile(a[:, k], 99)), max=float(a[:, k].max())) for k in range(3)]
        sc = c["scale"]
        out.update(r_stat_rel=pct(c["r_stat"] / sc), r_dual_rel=pct(c["r_dual"] / sc), r_comp_rel=pct(c["r_comp"] / sc), r_in=pct(c["r_in"]),
                   r_hier=pct(c["r_hier"]), res_own=pct(c["res_own"]), res_final=pct(c["res_final"]),
                   res_gap=pct(np.abs(c["res_final"] - c["res_own"])), scale=pct(sc), n_free=pct(c["n_free"].astype(float)),
                   n_active=pct(c["n_active"].astype(float)), level0_violated=int((c["slack0"] > 0.0).any(axis=1).sum()))
        if args.oracle:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import _hwbc_cert as H
            from oracle.pyoracle import Oracle
            o = Oracle(P, wbc_reg_steps=args.reg_steps)
            r = s.wbc_update()   # the last step's policy inputs: one more WBC call on the same resident inputs
            eps = P["config"].get("wbc_eps_reg", 1e-8)
            oc = np.array([H.oracle_certificate(o, H.tasks_of(o, r["x_des"][i], r["u_des"][i], w["rbd"][i], r["mode"][i]), eps, args.reg_steps)[0]
                           for i in range(args.batch)])
            out.update(oracle_worst=H.worst_table(oc), device_worst=H.worst_table(c["cert"]),
                       not_certified=int((~H.certified(c["cert"], H.bounds_from_oracle(oc))).sum()))
finally:
    s.close()
print(json.dumps(out))
