"""The field map through the C++ host adapter (include/hunter_hip.hpp: setGroundField of the ReferenceManager and of the
KalmanFilterEstimate): a small program built with g++ against it sets maps through both, reads them back with hb_ground_get_field, evaluates
one on the device, has a steep map refused, lets a profile map and a field map replace one another and switches the map off."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "hunter_bipedal_control_amd"
PARAMS_BIN = PKG / "data" / "hunter_params.bin"


def _build():
    lib = PKG / "libhunter_hip.so"
    assert lib.exists(), "libhunter_hip.so not built (python __graft_entry__.py build)"
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "groundfield_test"
    src = ROOT / "tests" / "cpp" / "groundfield_test.cpp"
    newest = max(src.stat().st_mtime, (ROOT / "include" / "hunter_hip.hpp").stat().st_mtime, (ROOT / "include" / "hunter_hip.h").stat().st_mtime,
                 lib.stat().st_mtime)
    if not exe.exists() or exe.stat().st_mtime < newest:
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", str(ROOT / "include"), str(src), "-L", str(PKG),
                               "-lhunter_hip", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    return exe


def test_groundfield_program_builds():
    assert _build().exists()


@pytest.mark.gpu
def test_cpp_field_map_round_trip():
    exe = _build()
    r = subprocess.run([str(exe), str(PARAMS_BIN)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "steep map refused" in r.stdout and "instance 1" in r.stdout
    assert "ok: field map round trip" in r.stdout
