"""The C++ host adapter's MPC certificate interface (include/hunter_hip.hpp, MpcMrtInterface::certificate / stageQp and ShardedSolver's
forwards): a small program built with g++ against it, checked bit for bit against the ctypes path on four of the ragged instances."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _mpc_cert as mc

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "hunter_bipedal_control_amd"
PARAMS_BIN = PKG / "data" / "hunter_params.bin"


def _build():
    lib = PKG / "libhunter_hip.so"
    assert lib.exists(), "libhunter_hip.so not built (python __graft_entry__.py build)"
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "mpc_certificate_test"
    src = ROOT / "tests" / "cpp" / "mpc_certificate_test.cpp"
    newest = max(src.stat().st_mtime, (ROOT / "include" / "hunter_hip.hpp").stat().st_mtime, (ROOT / "include" / "hunter_hip.h").stat().st_mtime,
                 lib.stat().st_mtime)
    if not exe.exists() or exe.stat().st_mtime < newest:
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-pthread", "-I", str(ROOT / "include"), str(src), "-L", str(PKG),
                               "-lhunter_hip", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    return exe


def test_mpc_certificate_program_builds():
    assert _build().exists()


@pytest.mark.gpu
def test_cpp_mpc_certificate_matches_ctypes_path(params, tmp_path):
    from hunter_bipedal_control_amd.solver import HunterSolver
    exe = _build()
    B, N = 4, mc.NMAX
    refs8, x08 = mc.ragged_problem(params)
    refs = {k: np.ascontiguousarray(v[:B]) for k, v in refs8.items()}
    x0 = np.ascontiguousarray(x08[:B])
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([B, N], dtype=np.int32).tofile(f)
        np.ascontiguousarray(refs["n_nodes"], dtype=np.int32).tofile(f)
        np.ascontiguousarray(refs["t"], dtype=np.float64).tofile(f)
        np.ascontiguousarray(refs["mode"], dtype=np.int32).tofile(f)
        np.ascontiguousarray(refs["x_ref"], dtype=np.float64).tofile(f)
        np.ascontiguousarray(refs["swing"], dtype=np.float64).tofile(f)
        x0.tofile(f)
    r = subprocess.run([str(exe), str(PARAMS_BIN), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "certificate before any solve: status -3" in r.stdout and "stage QP before any solve: status -3" in r.stdout
    assert "bad range: status -1" in r.stdout and "after new references: status -3" in r.stdout
    out = np.fromfile(tmp_path / "out.bin")
    sizes = dict(A=484, B=264, b=22, Q=484, P=264, R=144, q=22, r=12, n_til=1)
    pos = 0

    def take(n):
        nonlocal pos
        pos += n
        return out[pos - n:pos]

    cert, costate, u_til = take(B * 8).reshape(B, 8), take(B * (N + 1) * 22).reshape(B, N + 1, 22), take(B * N * 12).reshape(B, N, 12)
    s = HunterSolver(params, batch=B, max_nodes=N)
    try:
        s.set_references(refs)
        s.reset(x0)
        s.mpc_solve(x0)
        c = s.mpc_certificate()
        assert np.array_equal(cert, c["cert"], equal_nan=True) and np.array_equal(costate, c["costate"]) and np.array_equal(u_til, c["u_til"])
        assert np.array_equal(c["n_nodes"], refs["n_nodes"])
        for i in range(B):
            lq = s.mpc_lq(i)
            n = int(refs["n_nodes"][i])
            for key, w in sizes.items():
                full = take(N * w).reshape(N, -1)
                assert np.array_equal(full[:n].ravel(), lq[key].astype(np.float64).ravel()), (i, key)
                assert not full[n:].any(), (i, key)
        assert pos == out.size
    finally:
        s.close()
