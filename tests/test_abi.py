"""CPU: the C-ABI library loads and exports every symbol include/*.h declares (no compute without a GPU)."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from hunter_bipedal_control_amd import abi, solver

ROOT = Path(__file__).resolve().parents[1]


def test_header_and_library_symbols_agree():
    header = (ROOT / "include" / "hunter_hip.h").read_text()
    declared = sorted(set(re.findall(r"\b(hb_[a-z_0-9]+)\s*\(", header)))
    assert declared == sorted(solver.ABI_SYMBOLS)
    lib = solver.load_library()
    for name in declared:
        assert hasattr(lib, name), f"libhunter_hip.so does not export {name}"
    lib.hb_version.restype = C.c_int32
    assert lib.hb_version() >= 100
    lcm_header = (ROOT / "include" / "hunter_lcm.h").read_text()
    lcm_declared = sorted(set(re.findall(r"\b(hb_[a-z_0-9]+)\s*\(", lcm_header.split("extern \"C\"", 1)[1])))
    assert lcm_declared == sorted(solver.LCM_SYMBOLS)
    for name in lcm_declared:
        assert hasattr(lib, name), f"libhunter_hip.so does not export {name}"


def test_linesearch_getter_is_declared_bound_and_sized_alike():
    """hb_mpc_get_linesearch: declared once with its nine arguments, bound by the Python wrapper key for key, and the window length the
    header, the layout description and abi.py name is one number."""
    header = (ROOT / "include" / "hunter_hip.h").read_text()
    decl = re.findall(r"int32_t hb_mpc_get_linesearch\(([^;]*)\);", header)
    assert len(decl) == 1
    args = [re.sub(r"/\*.*?\*/", "", a).split()[-1].lstrip("*") for a in decl[0].replace("\n", " ").split(",")]
    assert args == ["ctx", "inst_begin", "inst_count"] + list(solver.HunterSolver.LINESEARCH_KEYS)
    assert int(re.search(r"#define HB_LS_TAIL_MAX (\d+)", header).group(1)) == abi.HB_LS_TAIL_MAX == 16
    layout = (ROOT / "hunter_bipedal_control_amd" / "csrc" / "hb_layout.hpp").read_text()
    assert "constexpr int LS_TAIL_MAX = HB_LS_TAIL_MAX;" in layout
    assert "hb_mpc_get_linesearch" in solver.ABI_SYMBOLS and hasattr(solver.load_library(), "hb_mpc_get_linesearch")


def test_riccati_gains_entry_is_declared_bound_and_its_sentinel_is_one_number():
    """hb_riccati_gains: declared once, bound by the Python wrapper, and the bit pattern it leaves in gain slots the sweep did not write is
    the same number in the header, in abi.py and in the twin that looks for it (tests/_rictwin.py)."""
    import _rictwin
    header = (ROOT / "include" / "hunter_hip.h").read_text()
    decl = re.findall(r"int32_t hb_riccati_gains\(([^;]*)\);", header)
    assert len(decl) == 1
    args = [a.split()[-1].lstrip("*") for a in decl[0].replace("\n", " ").split(",")]
    assert args == ["ctx", "n", "N", "n_f", "n_z", "A", "B", "b", "Q", "R", "P", "q", "r", "K", "k", "ric_fail"]
    bits = int(re.search(r"#define HB_RIC_GAINS_SENTINEL_BITS (0x[0-9a-fA-F]+)ULL", header).group(1), 16)
    assert bits == abi.RIC_GAINS_SENTINEL_BITS == int(_rictwin.SENTINEL_BITS)
    assert (bits >> 51) == 0xfff and bits & ((1 << 51) - 1), "a quiet NaN with a payload: arithmetic on it cannot come out finite"
    assert "hb_riccati_gains" in solver.ABI_SYMBOLS and hasattr(solver.HunterSolver, "riccati_gains")


def test_struct_sizes_match_the_header():
    # hb_model: 10 i32 + (30+30+40) f64 + 11 + 33 + 66 f64 + 4 i32 + 12 f64 + 1 f64
    assert C.sizeof(abi.HbModel) == 40 + 8 * (30 + 30 + 40 + 11 + 33 + 66) + 16 + 8 * 13
    assert C.sizeof(abi.HbStats) == 8 * 6 + 8 * 2 + 4 * 4
    assert C.sizeof(abi.HbConfig) % 8 == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a machine without a GPU")
def test_no_cpu_fallback(params):
    with pytest.raises(solver.HunterHipError, match="no HIP device"):
        solver.HunterSolver(params, batch=1, max_nodes=4)
    lib = solver.load_library()
    out = C.c_void_p()
    rc = lib.hb_create(None, None, 1, 1, 0, C.byref(out))
    assert rc == -1        # HB_ERR_ARG, never a crash
