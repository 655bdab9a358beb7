"""CPU: csrc/hb_forms.hpp compiled for the host (tests/host_emu/formsemu.cpp).

The selection rules — decode_forms and use_ric_bwd4 / use_ric_fwd_wave / lq_trip_len — against verbatim copies of the three expressions
the launchers of hb_api_mpc.hpp held before the header existed (backward-sweep choice, trip length, one-node and forward-sweep
choice), for the release and the profiling build, over every combination of hb_config.reserved in -1 .. 260, concurrent in
{1, 511, 512, 513, 1024, 2047, 2048, 4096}, Nmax in {1, 44, 100, 108, 200} and n_cu in {64, 256}.

The plant's rule — plant_form, mapped to the kernel plant_launch launches for it — against verbatim copies of the conditions of the two
nine-rung ladders hb_plant_step and plant_launch_hybrid held, over contact mode 0 / 1, every combination of joints_on, terrain_on,
modelvar_on and profile_on, and held / hybrid drive.

The table — every code a site of the library reads, the families of selectors by their bounds — against abi.py's hand-written mirror.
(LQT_VALUES .. LQT_VALUES_LEGS, 126 .. 128, are single codes: the kernels read each of them on its own, and the first and the last
name the bounds of the one site that reads them as an interval.)"""
import subprocess
from pathlib import Path

import pytest

from hunter_bipedal_control_amd import abi

HERE = Path(__file__).resolve().parent / "host_emu"


@pytest.fixture(scope="module")
def formsemu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("formsemu") / "formsemu"
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-o", str(exe), str(HERE / "formsemu.cpp")])
    return exe


@pytest.fixture(scope="module")
def table(formsemu):
    codes, ranges = [], []
    for line in subprocess.check_output([str(formsemu), "table"], text=True).splitlines():
        kind, name, *vals = line.split()
        (codes if kind == "code" else ranges).append((name, *map(int, vals)))
    return codes, ranges


def test_selection_rules_agree_with_the_expressions_they_replace(formsemu):
    r = subprocess.run([str(formsemu), "check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip() == f"checked {262 * 2 * 8 * 5 * 2}"


def test_plant_form_agrees_with_the_ladders_it_replaces(formsemu):
    r = subprocess.run([str(formsemu), "plant"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip() == f"checked {2 * 2 ** 4 * 2}"


def test_table_equals_the_python_mirror(table):
    codes, ranges = table
    assert len({n for n, *_ in codes + ranges}) == len(codes) + len(ranges)     # (no name twice, before the dicts would hide it)
    assert dict(codes) == abi.FORMS
    assert {n: (lo, hi) for n, lo, hi in ranges} == abi.FORM_RANGES
    assert set(abi.LQ_STOPS + abi.RIC1_STOPS + abi.RIC4_STOPS + abi.WBC_STOPS + abi.HWBC_STOPS) <= set(abi.FORMS.values())


def test_values_are_unique_and_ranges_overlap_no_code(table):
    codes, ranges = table
    values = [v for _, v in codes]
    assert len(set(values)) == len(values)
    covered = [v for _, lo, hi in ranges for v in range(lo, hi + 1)]
    assert all(lo < hi for _, lo, hi in ranges) and len(set(covered)) == len(covered)    # ranges do not overlap each other
    assert not set(covered) & set(values)
