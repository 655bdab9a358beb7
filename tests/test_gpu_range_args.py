"""-m gpu: every entry point that takes an instance range (i0, cnt) rejects a range outside the batch with HB_ERR_ARG — through ONE
check (range_ok in csrc/hb_api_ctx.hpp) that cannot overflow: i0 = INT32_MAX or cnt = INT32_MAX used to pass `i0 + cnt > B` by signed
wrap-around in the older entries and go on to a wild copy.  Raw ctypes calls, valid non-null buffers (sized for four instances), one
context of B = 3 instances and 4 nodes; afterwards the context still synchronises and reads back its status."""
import ctypes as C

import numpy as np
import pytest

from hunter_bipedal_control_amd import abi
from oracle import workloads

pytestmark = pytest.mark.gpu

B, N = 3, 4
INT32_MAX = 2147483647
BAD_RANGES = [(-1, 1), (3, 1), (0, 4), (1, 3), (INT32_MAX, 1), (1, INT32_MAX)]
ENTRIES = ["hb_mpc_set_references", "hb_mpc_get_references", "hb_mpc_get_solution", "hb_refgen_set_schedule", "hb_refgen_get_schedule",
           "hb_gait_insert_template", "hb_gait_get_state", "hb_wbc_get_certificate", "hb_hwbc_get_certificate", "hb_mpc_get_certificate"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _calls(lib, ctx):
    """name -> f(i0, cnt): the raw call with buffers for four instances (one more than the batch)."""
    M, E = B + 1, abi.HB_MAX_EVENTS
    f64 = lambda *shape: np.zeros(shape, dtype=np.float64)
    i32 = lambda *shape: np.zeros(shape, dtype=np.int32)
    n_nodes, t, mode, xref, swing = np.full(M, N, dtype=np.int32), f64(M, N + 1), i32(M, N), f64(M, N, 22), f64(M, N, 24)
    x, u = f64(M, N + 1, 22), f64(M, N, 22)
    n_ev, ev, modes = i32(M), f64(M, E), i32(M, E + 1)
    sw, tpl_modes, start, final = np.array([0.0, 0.3, 0.6]), i32(2), f64(M), np.ones(M)
    level, vel_abs, vel_avg, cmd, status = i32(M), f64(M), f64(M), f64(M, 4), i32(M)
    cert, dual = f64(M, 8), f64(M, 60)
    hcert, hx, hslack, hdual = f64(M, 3, 10), f64(M, 3, 38), f64(M, 40), f64(M, 3, 40)
    mcert, costate, util = f64(M, 8), f64(M, N + 1, 22), f64(M, N, 12)
    r = lambda i0, cnt: (ctx, C.c_int32(i0), C.c_int32(cnt))
    return {
        "hb_mpc_set_references": lambda i0, cnt: lib.hb_mpc_set_references(*r(i0, cnt), _p(n_nodes), _p(t), _p(mode), _p(xref), _p(swing)),
        "hb_mpc_get_references": lambda i0, cnt: lib.hb_mpc_get_references(*r(i0, cnt), _p(n_nodes), _p(t), _p(mode), _p(xref), _p(swing)),
        "hb_mpc_get_solution": lambda i0, cnt: lib.hb_mpc_get_solution(*r(i0, cnt), _p(x), _p(u)),
        "hb_refgen_set_schedule": lambda i0, cnt: lib.hb_refgen_set_schedule(*r(i0, cnt), _p(n_ev), _p(ev), _p(modes)),
        "hb_refgen_get_schedule": lambda i0, cnt: lib.hb_refgen_get_schedule(*r(i0, cnt), _p(n_ev), _p(ev), _p(modes)),
        "hb_gait_insert_template": lambda i0, cnt: lib.hb_gait_insert_template(*r(i0, cnt), C.c_int32(3), _p(sw), _p(tpl_modes), _p(start), _p(final)),
        "hb_gait_get_state": lambda i0, cnt: lib.hb_gait_get_state(*r(i0, cnt), _p(level), _p(vel_abs), _p(vel_avg), _p(cmd), _p(n_ev), _p(ev), _p(modes),
                                                                   _p(status)),
        "hb_wbc_get_certificate": lambda i0, cnt: lib.hb_wbc_get_certificate(*r(i0, cnt), _p(cert), _p(dual)),
        "hb_hwbc_get_certificate": lambda i0, cnt: lib.hb_hwbc_get_certificate(*r(i0, cnt), _p(hcert), _p(hx), _p(hslack), _p(hdual)),
        "hb_mpc_get_certificate": lambda i0, cnt: lib.hb_mpc_get_certificate(*r(i0, cnt), _p(mcert), _p(costate), _p(util)),
    }


def test_every_instance_range_entry_rejects_ranges_outside_the_batch(params):
    from hunter_bipedal_control_amd.solver import HunterSolver
    refs, x0, _, _ = workloads.trot_batch(params, B, n_intervals=N)
    s = HunterSolver(params, batch=B, max_nodes=N)
    try:
        s.set_references(refs)
        s.reset(x0)
        calls = _calls(s.lib, s.ctx)
        assert sorted(calls) == sorted(ENTRIES)
        got = {(name, rng): calls[name](*rng) for name in ENTRIES for rng in BAD_RANGES}
        assert got == {k: abi.HB_ERR_ARG for k in got}
        assert s.lib.hb_sync(s.ctx) == abi.HB_OK
        assert s.mpc_status().tolist() == [abi.HB_INST_OK] * B   # the freshly reset context still works
    finally:
        s.close()
