"""CPU: the KKT certificate of the WeightedWbc QP (wbc_solve's certificate instantiation, hb_wbc.hpp) compiled for the host with one
emulated lane, against numpy on the oracle's rows of the same problems (oracle.wbc_problem: the reference's constraint order)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from hunter_bipedal_control_amd import abi, gait, workload

HERE = Path(__file__).resolve().parent / "host_emu"
R_EQ, R_IN, R_STAT, R_DUAL, R_COMP, N_ACTIVE, EPS, SCALE = range(8)


@pytest.fixture(scope="module")
def cert_lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("certemu") / "libcertemu.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", str(so), str(HERE / "certemu.cpp")])
    return C.CDLL(str(so))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _run(lib, params, cfg_kw, xd, ud, rbd, mode, stance, sol_prev=None):
    mdl, cfg = abi.make_model(params), abi.make_config(params, **cfg_kw)
    sol = np.zeros(38) if sol_prev is None else np.array(sol_prev, dtype=np.float64)
    st, it = C.c_int(), C.c_int()
    cert, dual, active = np.zeros(8), np.zeros(60), np.zeros(64, dtype=np.int32)
    lib.cert_wbc(C.byref(mdl), C.byref(cfg), _p(xd), _p(ud), _p(rbd), C.c_int(int(mode)), C.c_int(int(stance)), _p(sol), C.byref(st),
                 C.byref(it), _p(cert), _p(dual), _p(active))
    return sol, st.value, it.value, cert, dual, active


def numpy_certificate(pr, x, y):
    """The five residuals of hunter_hip.h's certificate from the oracle's rows, a point x and multipliers y (row order Aeq, D)."""
    A = np.vstack([pr["Aeq"], pr["D"]])
    ne = pr["Aeq"].shape[0]
    H = pr["Aw"].T @ pr["Aw"]
    g = -pr["Aw"].T @ pr["bw"]
    s = pr["D"] @ x - pr["f"]
    yi = y[ne:A.shape[0]]
    return dict(r_eq=np.abs(pr["Aeq"] @ x - pr["beq"]).max(), r_in=max(0.0, s.max()), r_stat=np.abs(H @ x + g - A.T @ y[:A.shape[0]]).max(),
                r_dual=max(0.0, yi.max()), r_comp=np.abs(yi * s).max(), scale=max(1.0, np.abs(g).max(), np.abs(H @ x).max()))


def _mixed_inputs(params, B, seed):
    """The direct-path mix of tests/test_gpu_parity.py::test_wbc_direct_matches_oracle (modes 3 / 3 / 2 / 1 / 0, every fifth in stance)."""
    rng = np.random.default_rng(seed)
    x0 = np.array(params["config"]["initial_state"])
    mass = sum(params["model"]["mass"])
    xd, ud, rbd = np.zeros((B, 22)), np.zeros((B, 22)), np.zeros((B, 32))
    mode, stance = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for i in range(B):
        mode[i] = [3, 3, 2, 1, 0][i % 5]
        stance[i] = 1 if i % 5 == 0 else 0
        cf = gait.mode_to_contact_flags(int(mode[i]))
        for k in range(4):
            if cf[k]:
                ud[i, 3 * k:3 * k + 3] = [3 * rng.standard_normal(), 3 * rng.standard_normal(), mass * 9.81 / max(sum(cf), 1)]
        ud[i, 12:] = 0.5 * rng.standard_normal(10)
        xd[i] = x0 + 0.05 * rng.standard_normal(22)
        rbd[i] = workload.rbd_from_state(x0 + 0.03 * rng.standard_normal(22), i)
        rbd[i, 16:] = 0.3 * rng.standard_normal(16)
    return xd, ud, rbd, mode, stance


def _fast_inputs(params, B, seed):
    from test_gpu_parity import _fast_moving_wbc_inputs
    xd, ud, rbd, mode = _fast_moving_wbc_inputs(params, B, seed)
    return xd, ud, rbd, mode, np.zeros(B, dtype=np.int32)


@pytest.mark.parametrize("inputs, cfg_kw", [("mixed", {}), ("fast", {}), ("mixed", {"wbc_eps_mode": 1}), ("fast", {"wbc_eps_mode": 1})])
def test_certificate_matches_numpy(params, oracle, cert_lib, inputs, cfg_kw):
    """Every mode (incl. stance and fast motion with torque-limit / friction rows in the working set): the device routine's residuals
    against numpy's on the oracle's rows, its multipliers against numpy's least squares on the same working set, both at 1e-9; the
    solution is the oracle's and is certified."""
    from oracle.pyoracle import Oracle
    B = 20
    xd, ud, rbd, mode, stance = (_mixed_inputs if inputs == "mixed" else _fast_inputs)(params, B, 3)
    o = oracle if not cfg_kw else Oracle(params, **cfg_kw)
    so, sto, _ = o.wbc_update(xd, ud, rbd, mode, stance_flag=stance, threads=4)
    seen_ineq = 0
    for i in range(B):
        sol, st, _, cert, dual, active = _run(cert_lib, params, cfg_kw, xd[i], ud[i], rbd[i], mode[i], stance[i])
        assert st == sto[i] == 0
        assert np.abs(sol - so[i]).max() < 1e-6 * max(1.0, np.abs(so[i]).max())
        pr = o.wbc_problem(xd[i], ud[i], rbd[i], int(mode[i]), bool(stance[i]))
        ne, ni = pr["Aeq"].shape[0], pr["D"].shape[0]
        n_sw = (ne - 16) // 3
        assert ne + ni == 36 + 6 * n_sw + 5 * (4 - n_sw) and ne + ni <= 60
        ref = numpy_certificate(pr, sol, dual)
        scale = ref["scale"]
        assert abs(cert[SCALE] - scale) <= 1e-12 * scale
        for k, name in ((R_EQ, "r_eq"), (R_IN, "r_in"), (R_STAT, "r_stat"), (R_DUAL, "r_dual"), (R_COMP, "r_comp")):
            assert abs(cert[k] - ref[name]) <= 1e-9 * scale, (i, name, cert[k], ref[name])
        # multipliers: numpy least squares on the solver's working set (equalities + active inequality rows)
        W = list(range(ne)) + [c for c in range(ne, ne + ni) if active[c]]
        A = np.vstack([pr["Aeq"], pr["D"]])
        H, g = pr["Aw"].T @ pr["Aw"], -pr["Aw"].T @ pr["bw"]
        yW = np.linalg.lstsq(A[W].T, H @ sol + g, rcond=None)[0]
        y = np.zeros(60)
        y[W] = yW
        assert cert[N_ACTIVE] == len(W)
        assert np.abs(dual - y).max() <= 1e-9 * scale, (i, np.abs(dual - y).max())
        assert not dual[ne + ni:].any() and not dual[[c for c in range(60) if c not in W]].any()
        seen_ineq += len(W) - ne
        # certified: primal feasibility, stationarity of the unregularised problem (1e-8), sign and complementarity
        # (measured on these inputs: r_eq 1.8e-10 absolute, r_stat / scale 1.3e-9, r_dual / scale 7.2e-9, r_comp / scale 1e-19)
        assert cert[R_EQ] <= 1e-9 and cert[R_IN] <= 1e-9
        assert cert[R_STAT] <= 1e-8 * scale and cert[R_DUAL] <= 1e-7 * scale and cert[R_COMP] <= 1e-9 * scale
        assert cert[EPS] > 0.0 and (cfg_kw or cert[EPS] == params["config"].get("wbc_eps_reg", 1e-8))
    if inputs == "fast":
        assert seen_ineq > 0, "the fast-motion case must carry inequality rows in the working set"


def test_certificate_sees_the_tikhonov_bias(params, cert_lib):
    """Without the regularisation step the point is the eps-regularised minimiser: its stationarity residual for the unregularised
    problem is first order in eps and much larger than with the step."""
    xd, ud, rbd, mode, stance = _mixed_inputs(params, 20, 5)
    med = {}
    for reg in (0, 1):
        r = [(lambda c: c[R_STAT] / c[SCALE])(_run(cert_lib, params, {"wbc_reg_steps": reg}, xd[i], ud[i], rbd[i], mode[i], stance[i])[3])
             for i in range(20)]
        med[reg] = np.median(r)
    assert med[0] >= 10.0 * med[1], med


def test_certificate_of_a_failed_solve_is_at_the_previous_solution(params, cert_lib):
    """wbc_max_iter below the number of equality rows: MAXITER, the previous solution is kept and certified as what it is (not the
    optimum: large residuals), with the working set of the failed solve."""
    xd, ud, rbd, mode, stance = _mixed_inputs(params, 5, 9)
    prev = np.full(38, 0.5)
    sol, st, _, cert, dual, _ = _run(cert_lib, params, {"wbc_max_iter": 2}, xd[1], ud[1], rbd[1], mode[1], stance[1], sol_prev=prev)
    assert st == 1 and np.array_equal(sol, prev)
    assert max(cert[R_STAT], cert[R_IN], cert[R_EQ]) > 1e-6 * cert[SCALE]
    assert np.isfinite(cert).all() and np.isfinite(dual).all()
