"""The C++ host adapter's per-level certificate interface (include/hunter_hip.hpp, Wbc::enableLevelCertificate / levelCertificate): a
small program built with g++ against it, checked against the ctypes path on the same inputs."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_wbc_certificate_host import _mixed_inputs

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "hunter_bipedal_control_amd"
PARAMS_BIN = PKG / "data" / "hunter_params.bin"


def _build():
    lib = PKG / "libhunter_hip.so"
    assert lib.exists(), "libhunter_hip.so not built (python __graft_entry__.py build)"
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "hwbc_certificate_test"
    src = ROOT / "tests" / "cpp" / "hwbc_certificate_test.cpp"
    newest = max(src.stat().st_mtime, (ROOT / "include" / "hunter_hip.hpp").stat().st_mtime, (ROOT / "include" / "hunter_hip.h").stat().st_mtime,
                 lib.stat().st_mtime)
    if not exe.exists() or exe.stat().st_mtime < newest:
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", str(ROOT / "include"), str(src), "-L", str(PKG),
                               "-lhunter_hip", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    return exe


def test_hwbc_certificate_program_builds():
    assert _build().exists()


@pytest.mark.gpu
def test_cpp_hwbc_certificate_matches_ctypes_path(params, tmp_path):
    from hunter_bipedal_control_amd.solver import HunterSolver
    exe = _build()
    B = 16
    xd, ud, rbd, mode, _ = _mixed_inputs(params, B, 11)
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([B], dtype=np.int32).tofile(f)
        for a in (xd, ud, rbd):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
        np.ascontiguousarray(mode, dtype=np.int32).tofile(f)
    r = subprocess.run([str(exe), str(PARAMS_BIN), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "weighted refused: status -1" in r.stdout and "no update yet: status -3" in r.stdout
    out = np.fromfile(tmp_path / "out.bin")
    sizes = (B * 38, B * 30, B * 114, B * 40, B * 120)
    assert out.size == sum(sizes)
    sol, cert, xl, s0, dual = np.split(out, np.cumsum(sizes)[:-1])
    s = HunterSolver(params, batch=B, max_nodes=4, wbc_type=1)
    try:
        s.hwbc_set_certificate(True)
        sol_p, _ = s.wbc_update_direct(xd, ud, rbd, mode, np.zeros(B, dtype=np.int32))
        c = s.hwbc_certificate()
    finally:
        s.close()
    assert np.array_equal(sol.reshape(B, 38), sol_p)
    assert np.array_equal(cert.reshape(B, 3, 10), c["cert"]) and np.array_equal(xl.reshape(B, 3, 38), c["x_levels"])
    assert np.array_equal(s0.reshape(B, 40), c["slack0"]) and np.array_equal(dual.reshape(B, 3, 40), c["dual"])
