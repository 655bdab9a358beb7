"""CPU: the KKT certificate of the MPC's stage QP (hb_mpccert.hpp: mpc_cert_node, mpc_cert_sweep_*) and the stage-QP export
(hb_lq.hpp rec_unpack) compiled for the host with one emulated lane, behind the host twin of one SQP iteration (lq_node ->
riccati_bwd_node -> riccati_fwd_node), against the dense KKT system of the exported QP in numpy (tests/_mpc_cert.py).

Measured on these eight instances (host twin): R_DYN <= 1.1e-16, R_STAT <= 7.5e-14 SCALE, dx / u~ / lambda against the dense solve
1.5e-13 / 1.5e-10 / 4.4e-11, numpy's own KKT residual <= 1e-11 (asserted); R_STAT / SCALE after the 1e-4 gain error >= 2.6e-8."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _mpc_cert as mc
from hunter_bipedal_control_amd import abi

HERE = Path(__file__).resolve().parent / "host_emu"


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("mpccertemu") / "libmpccertemu.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", str(so), str(HERE / "mpccertemu.cpp")])
    return C.CDLL(str(so))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def run_twin(lib, params, refs, x0, x, u, i, perturb_stage=-1, perturb_rel=0.0):
    """One SQP iteration of instance i on the host twin + its certificate -> dict(n, lq, dx, cert, costate, u_til)."""
    mdl, cfg = abi.make_model(params), abi.make_config(params)
    n = int(refs["n_nodes"][i])
    t = np.ascontiguousarray(refs["t"][i, :n + 1])
    mode = np.ascontiguousarray(refs["mode"][i, :n], dtype=np.int32)
    xref = np.ascontiguousarray(refs["x_ref"][i, :n])
    swing = np.ascontiguousarray(refs["swing"][i, :n]).reshape(n, 24)
    xi, ui = np.ascontiguousarray(x[i, :n + 1]).copy(), np.ascontiguousarray(u[i, :n]).copy()
    dx, cert, costate, u_til = np.zeros((n + 1, 22)), np.zeros(8), np.zeros((n + 1, 22)), np.zeros((n, 12))
    lq = dict(A=np.zeros((n, 22, 22)), B=np.zeros((n, 22, 12)), b=np.zeros((n, 22)), Q=np.zeros((n, 22, 22)), P=np.zeros((n, 12, 22)),
              R=np.zeros((n, 12, 12)), q=np.zeros((n, 22)), r=np.zeros((n, 12)))
    n_til = np.zeros(n, dtype=np.int32)
    lib.emu_mpc_certificate(C.byref(mdl), C.byref(cfg), C.c_int(n), _p(t), _p(mode), _p(xref), _p(swing), _p(np.ascontiguousarray(x0[i])),
                            _p(xi), _p(ui), C.c_int(perturb_stage), C.c_double(perturb_rel), _p(dx), _p(cert), _p(costate), _p(u_til),
                            *[_p(lq[k]) for k in mc.LQ_KEYS], _p(n_til))
    return dict(n=n, lq=lq, n_til=n_til, dx=dx, cert=dict(zip(mc.FIELDS, cert)), costate=costate, u_til=u_til)


@pytest.fixture(scope="module")
def problem(params, oracle):
    refs, x0 = mc.ragged_problem(params)
    x, u = mc.cold_start(oracle, refs, x0)
    return refs, x0, x, u


@pytest.fixture(scope="module")
def twin_runs(lib, params, problem):
    refs, x0, x, u = problem
    return [run_twin(lib, params, refs, x0, x, u, i) for i in range(len(mc.SPECS))]


def test_twin_matches_the_dense_kkt_solve_and_is_certified(twin_runs, problem):
    """CPU tests 1-3: (dx, u~, lambda, OBJ) against np.linalg.solve on the dense KKT system of the exported QP; every reported field
    against numpy's recomputation; R_DYN <= 1e-12 max(1, STEP_MAX) and R_STAT <= 1e-9 SCALE on all eight (SCALE has no floor: the
    standing instance's is 3.4e-3)."""
    refs = problem[0]
    widths = set()
    for i, r in enumerate(twin_runs):
        n = r["n"]
        mc.check_against_numpy(r["lq"], n, r["dx"], r["u_til"], r["costate"], r["cert"], tag=f"twin[{i}]")
        widths |= set(r["n_til"].tolist())
        for k in range(n):   # the padded input columns: R~ = I, zero elsewhere, u~ = 0
            nt = int(r["n_til"][k])
            assert np.array_equal(r["lq"]["R"][k][nt:, nt:], np.eye(12 - nt)) and not r["lq"]["B"][k][:, nt:].any()
            assert not r["u_til"][k, nt:].any()
        assert np.array_equal(r["lq"]["Q"], r["lq"]["Q"].transpose(0, 2, 1))
    assert widths == {6, 9, 12}
    assert min(r["cert"]["scale"] for r in twin_runs) < 1e-2   # the standing instance: a floor at 1 would hide 300 x


def test_detects_an_error_in_one_gain(lib, params, problem, twin_runs):
    """CPU test 4: 1e-4 (1 + |k~_0|) added to k~_0 of stage n // 2 before the forward sweep: R_STAT > 1e-9 SCALE on every instance (the
    dynamics still hold: the forward sweep is consistent with the wrong gain)."""
    refs, x0, x, u = problem
    for i in range(len(mc.SPECS)):
        n = twin_runs[i]["n"]
        c = run_twin(lib, params, refs, x0, x, u, i, perturb_stage=n // 2, perturb_rel=1e-4)["cert"]
        print(f"perturbed[{i}] n={n}: r_stat/scale={c['r_stat'] / c['scale']:.3e} (clean {twin_runs[i]['cert']['r_stat'] / twin_runs[i]['cert']['scale']:.3e})")
        assert c["r_stat"] > 1e-9 * c["scale"], (i, c)
        assert c["r_dyn"] <= 1e-12 * max(1.0, c["step_max"])


def test_unpack_round_trip(lib):
    """CPU test 5: rec_unpack agrees with the rec_A / rec_B / rec_P / rec_R / rec_b / rec_r accessors (and the packed Q~ | q~) on a record
    of distinct values; Q is symmetric; n_til = n_f + n_z."""
    size = lib.emu_rec_size()
    rec = np.arange(size, dtype=np.float64) + 0.5
    idx = lambda which, i, j=0: lib.emu_rec_index(C.c_int(which), C.c_int(i), C.c_int(j))  # noqa: E731
    rec[idx(8, 0)], rec[idx(9, 0)] = 6.0, 3.0
    A, B, b, Q, P, R, q, r = (np.zeros(s) for s in ((22, 22), (22, 12), (22,), (22, 22), (12, 22), (12, 12), (22,), (12,)))
    n_til = C.c_int()
    lib.emu_rec_unpack(_p(rec), _p(A), _p(B), _p(b), _p(Q), _p(P), _p(R), _p(q), _p(r), C.byref(n_til))
    for i in range(22):
        assert b[i] == rec[idx(2, i)] and q[i] == rec[idx(7, i)]
        for j in range(22):
            assert A[i, j] == rec[idx(0, i, j)]
            assert Q[i, j] == rec[idx(6, min(i, j), max(i, j))]
        for a in range(12):
            assert B[i, a] == rec[idx(1, i, a)] and P[a, i] == rec[idx(3, a, i)]
    for a in range(12):
        assert r[a] == rec[idx(5, a)]
        for c in range(12):
            assert R[a, c] == rec[idx(4, a, c)]
    assert np.array_equal(Q, Q.T) and n_til.value == 9
    every = np.concatenate([v.ravel() for v in (A, B, b, P, R, q, r)] + [Q[np.triu_indices(22)]])
    assert len(set(every.tolist())) == every.size, "distinct record entries map to distinct outputs"
    # null pointers are skipped
    lib.emu_rec_unpack(_p(rec), None, None, None, None, None, None, None, None, None)
