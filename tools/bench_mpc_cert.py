#!/usr/bin/env python3
"""Cost and distribution of the on-demand MPC certificate (hb_mpc_get_certificate) on the headline workload:
BASELINE configs[2] (4096 distinct trotting instances, N = 100, tables generated on the device, workload.device_trot_batch), one
hb_mpc_solve, then the certificate of the whole batch.  Prints one JSON line: the wall time of the call with the certificate fields
only (the two kernels, one synchronisation, a 256 KB copy) and with costates and u~ copied out as well, the MPC call next to it, and the
median / p99 / max of R_DYN and R_STAT / SCALE over the batch.  `--batch 1 --nodes 54` is the single-robot figure.
The times of the two kernels come from a kernel trace of their own, next to k_ric_fwd of the same run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_mpc_cert.py --repeat 10
python tools/bench_mpc_cert.py [--batch B] [--nodes N] [--repeat R]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
from hunter_bipedal_control_amd import ingest, workload
from hunter_bipedal_control_amd.solver import HunterSolver

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--nodes", type=int, default=100)
ap.add_argument("--repeat", type=int, default=5)
args = ap.parse_args()
P = ingest.load_packaged()
s = HunterSolver(P, batch=args.batch, max_nodes=args.nodes)
try:
    w = workload.device_trot_batch(s, P, n_intervals=args.nodes)
    t_mpc = []
    for _ in range(max(args.repeat, 1)):   # every solve continues from the last: the receding-horizon situation
        s.sync()
        t0 = time.perf_counter()
        s.mpc_solve(w["x0"])
        s.sync()
        t_mpc.append(time.perf_counter() - t0)
    cert = np.zeros((args.batch, 8))
    t_cert = []
    for _ in range(max(args.repeat, 1) + 1):   # the first call allocates the work buffers
        t0 = time.perf_counter()
        rc = s.lib.hb_mpc_get_certificate(s.ctx, C.c_int32(0), C.c_int32(args.batch), cert.ctypes.data_as(C.c_void_p), None, None)
        t_cert.append(time.perf_counter() - t0)
        assert rc == 0, s.lib.hb_last_error(s.ctx).decode()
    t0 = time.perf_counter()
    c = s.mpc_certificate()
    t_full = time.perf_counter() - t0
    status = s.mpc_status()
finally:
    s.close()
ok = c["n_nodes"] > 0
rel = c["r_stat"][ok] / c["scale"][ok]
pct = lambda a: dict(median=float(np.median(a)), p99=float(np.percentile(a, 99)), max=float(a.max()))  # noqa: E731
print(json.dumps(dict(batch=args.batch, nodes=args.nodes, repeat=args.repeat, mpc_status_max=int(status.max()), certified_instances=int(ok.sum()),
                      mpc_solve_ms=1e3 * float(np.median(t_mpc)), certificate_first_call_ms=1e3 * t_cert[0],
                      certificate_fields_only_ms=1e3 * float(np.median(t_cert[1:])), certificate_all_outputs_ms=1e3 * t_full,
                      r_dyn=pct(c["r_dyn"][ok]), r_stat_rel=pct(rel), scale=pct(c["scale"][ok]), u_max=pct(c["u_max"][ok]),
                      lambda_max=pct(c["lambda_max"][ok]), over_1e9=int((rel > 1e-9).sum()))))
