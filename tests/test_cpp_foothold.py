"""The planner's foothold mode through the C++ host adapter (include/hunter_hip.hpp: setFootholdConfig, getFootholdConfig and
getFootholdChoice of the ReferenceManager): a small program built with g++ against it sets a configuration with and without a map in
force, reads it back with hb_ground_get_foothold, has one refused, clears it by mode 0 and by nullptr and reads the choice read-back."""
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
    exe = out / "foothold_test"
    src = ROOT / "tests" / "cpp" / "foothold_test.cpp"
    newest = max(src.stat().st_mtime, (ROOT / "include" / "hunter_hip.hpp").stat().st_mtime, (ROOT / "include" / "hunter_hip.h").stat().st_mtime,
                 lib.stat().st_mtime)
    if not exe.exists() or exe.stat().st_mtime < newest:
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", str(ROOT / "include"), str(src), "-L", str(PKG),
                               "-lhunter_hip", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    return exe


def test_foothold_program_builds():
    assert _build().exists()


@pytest.mark.gpu
def test_cpp_foothold_round_trip():
    exe = _build()
    r = subprocess.run([str(exe), str(PARAMS_BIN)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "configuration refused" in r.stdout and "n_shift" in r.stdout
    assert "ok: foothold configuration round trip" in r.stdout
