"""C++ ingest of the reference's input files (include/hunter_ingest.hpp, include/hunter_info.hpp): what LeggedController::init reads
through LeggedInterface / WbcBase::loadTasksSetting / KalmanFilterEstimate::loadSettings (LeggedInterface.cpp:55-96,
WbcBase.cpp:352-411) — task.info, reference.info, gait.info and hunter.urdf — flattened into the ABI structs by a C++14 header with
no dependency.  Held byte for byte to the Python ingest (ingest.py + abi.py) and to the packaged data/hunter_params.bin."""
import ctypes as C
import struct
import subprocess
from pathlib import Path

import pytest

from hunter_bipedal_control_amd import abi, ingest

ROOT = Path(__file__).resolve().parents[1]
PARAMS_BIN = ROOT / "hunter_bipedal_control_amd" / "data" / "hunter_params.bin"
# the reference's task.info / reference.info / gait.info and hunter.urdf, stored as test inputs
CFG = ROOT / "tests" / "golden" / "reference_input"
URDF = CFG / "hunter.urdf"


@pytest.fixture(scope="module")
def exe():
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    e = out / "ingest_test"
    src = ROOT / "tests" / "cpp" / "ingest_test.cpp"
    deps = [src, ROOT / "include" / "hunter_ingest.hpp", ROOT / "include" / "hunter_info.hpp", ROOT / "include" / "hunter_hip.h"]
    if not e.exists() or e.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(e)])
    return e


def test_packaged_blob_is_the_image_of_the_python_structs(params, tmp_path):
    """data/hunter_params.bin (HB02) = header + hb_model + hb_config + estimator / refgen / gain structs + schedules, as
    abi.write_params_blob lays them out from the packaged JSON."""
    raw = PARAMS_BIN.read_bytes()
    head = struct.unpack("<8I", raw[:32])
    assert head[0] == abi.PARAMS_BLOB_MAGIC and head[1] == C.sizeof(abi.HbModel) and head[2] == C.sizeof(abi.HbConfig)
    o = 32
    assert raw[o:o + head[1]] == bytes(abi.make_model(params)); o += head[1]
    assert raw[o:o + head[2]] == bytes(abi.make_config(params)); o += head[2]
    assert raw[o:o + head[3]] == bytes(abi.make_estimator_config(params)); o += head[3]
    assert raw[o:o + head[4]] == bytes(abi.make_refgen_config(params)); o += head[4]
    assert raw[o:o + head[5]] == bytes(abi.make_joint_gains())
    again = tmp_path / "again.bin"
    abi.write_params_blob(params, again)
    assert again.read_bytes() == raw


def test_cpp_blob_round_trip(exe, tmp_path):
    out = tmp_path / "rt.bin"
    subprocess.check_call([str(exe), "--roundtrip", str(PARAMS_BIN), str(out)])
    assert out.read_bytes() == PARAMS_BIN.read_bytes()


def test_cpp_loader_errors_like_the_reference(exe, tmp_path):
    """LeggedInterface throws std::invalid_argument on a missing file (LeggedInterface.cpp:62,73,84); the ingest does the same
    (the test program turns it into exit code 1 + message)."""
    r = subprocess.run([str(exe), str(tmp_path / "no_task.info"), "x.urdf", "r.info", "g.info", str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot open" in r.stderr
    bad = tmp_path / "bad.bin"
    bad.write_bytes(b"HB01" + bytes(100))
    r = subprocess.run([str(exe), "--roundtrip", str(bad), str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 1 and "does not match this ABI" in r.stderr


def test_cpp_ingest_of_the_reference_files_reproduces_the_packaged_blob(exe, tmp_path):
    """task.info + hunter.urdf + reference.info + gait.info read by the C++ header == the packaged image, byte for byte; and the
    Python ingest of the same files == the packaged JSON values."""
    out = tmp_path / "cpp.bin"
    r = subprocess.run([str(exe), str(CFG / "task.info"), str(URDF), str(CFG / "reference.info"), str(CFG / "gait.info"), str(out)],
                       capture_output=True, text=True, check=True)
    assert out.read_bytes() == PARAMS_BIN.read_bytes()
    assert "gaits 4" in r.stdout or "gaits" in r.stdout
    fresh = dict(model=ingest.read_urdf(URDF), config=ingest.read_config(CFG / "task.info", CFG / "reference.info", CFG / "gait.info"))
    py = tmp_path / "py.bin"
    abi.write_params_blob(fresh, py)
    assert py.read_bytes() == PARAMS_BIN.read_bytes()
