"""CPU: every block of the LQ stage record, node by node, against the oracle's unprojected node LQ lifted through the record's own change of
input variables (tests/_lqrec.py) — the host twin of the record assembly (hb_lq.hpp lq_node compiled for the host with one emulated
lane, tests/host_emu/mpccertemu.cpp emu_lq_records) on the eight ragged all-mode instances (268 nodes) at the cold start (a) and at a
seeded generic iterate with planted barrier arguments (b) — and the self-test that the checker bites.

Bound: 1e-13 per block, relative to max(1, max |expected block|).
(5.4e-15 is the largest figure measured below; the margin of about 20 is there because it is the maximum of 268 nodes of one seed.)

Measured, host twin, maxima over the 268 nodes, (a) / (b):
  D T 3.0e-16 / 1.5e-15   Dt(D K + C) 2.4e-15 / 3.6e-15   Dt(D k + e) 1.2e-15 / 3.4e-15
  A~ 7.2e-16 / 8.3e-16   B~ 7.8e-18 / 6.9e-18   b~ 8.3e-17 / 5.6e-16   Q~ 1.4e-15 / 3.5e-15   P~ 1.3e-15 / 2.2e-15   R~ 7.6e-17 / 5.8e-16
  q~ 1.7e-15 / 3.1e-15   r~ 3.3e-16 / 1.5e-15   qf 2.5e-15 / 5.4e-15   rf 3.9e-16 / 1.2e-15
  cost dt 2.7e-15 / 4.6e-15   dyn_sse dt 2.4e-19 / 2.8e-17   eq_sse dt 4.4e-16 / 2.3e-15   dq 0 / 2.2e-16
Nodes of (b) per barrier branch (log / extension): friction 247 / 84, position lower 268 / 79, upper 268 / 82, rate lower 268 / 72,
upper 268 / 72, force lower 267 / 183, upper 268 / 72; at the cold start only force-lower reaches its extension (the swing feet).
"""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _lqrec as lr
import _mpc_cert as mc
from hunter_bipedal_control_amd import abi

HERE = Path(__file__).resolve().parent / "host_emu"
BOUND = 1e-13
SHAPES = dict(A=(22, 22), B=(22, 12), b=(22,), Q=(22, 22), P=(12, 22), R=(12, 12), q=(22,), r=(12,), n_til=(), Kx=(10, 22), ke=(10,), Z=(10, 6),
              dF=(12,), qf=(22,), rf=(22,), meta=(6,), dt=(), dq=(10,))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("lqrecemu") / "libmpccertemu.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", str(so), str(HERE / "mpccertemu.cpp")])
    return C.CDLL(str(so))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def twin_records(lib, params, refs, x, u, i):
    """The records of instance i of the host twin at (x, u) -> dict of [n] stages (lr.LQ_KEYS + lr.REC_KEYS)."""
    mdl, cfg = abi.make_model(params), abi.make_config(params)
    n = int(refs["n_nodes"][i])
    t = np.ascontiguousarray(refs["t"][i, :n + 1])
    mode = np.ascontiguousarray(refs["mode"][i, :n], dtype=np.int32)
    xref = np.ascontiguousarray(refs["x_ref"][i, :n])
    swing = np.ascontiguousarray(refs["swing"][i, :n]).reshape(n, 24)
    xi, ui = np.ascontiguousarray(x[i, :n + 1]), np.ascontiguousarray(u[i, :n])
    rec = {key: np.zeros((n,) + SHAPES[key], dtype=np.int32 if key == "n_til" else np.float64) for key in lr.LQ_KEYS + lr.REC_KEYS}
    lib.emu_lq_records(C.byref(mdl), C.byref(cfg), C.c_int(n), _p(t), _p(mode), _p(xref), _p(swing), _p(xi), _p(ui),
                       *[_p(rec[key]) for key in lr.LQ_KEYS + lr.REC_KEYS])
    return rec


@pytest.fixture(scope="module")
def problem(params, oracle):
    return lr.iterates(params, oracle)


@pytest.fixture(scope="module")
def nodes(problem):
    """The node inputs per point and instance; the oracle's LQ of a node is computed once and kept with it."""
    refs, _, points = problem
    return {name: [lr.instance_nodes(refs, x, u, i) for i in range(len(mc.SPECS))] for name, (x, u) in points.items()}


@pytest.fixture(scope="module")
def twin(lib, params, problem):
    refs, _, points = problem
    return {name: [twin_records(lib, params, refs, x, u, i) for i in range(len(mc.SPECS))] for name, (x, u) in points.items()}


@pytest.mark.parametrize("point", ["a", "b"])
def test_host_twin_record_matches_the_lifted_oracle(oracle, nodes, twin, point):
    """All 268 nodes at the cold start (a) / the generic iterate (b): structure exactly, every block within 1e-13."""
    worst, widths = {}, set()
    for i in range(len(mc.SPECS)):
        fig = lr.check_record(oracle, nodes[point][i], twin[point][i], BOUND, tag=f"twin ({point})[{i}]")
        lr.merge(worst, fig, i)
        widths |= set(twin[point][i]["n_til"].tolist())
    print(f"host twin ({point}), worst per check (figure, instance, node): " + " ".join(f"{k}={v:.2e}@{i}/{n}" for k, (v, i, n) in worst.items()))
    assert widths == {6, 9, 12}
    assert set(worst) == set(lr.TOLERANCED)


def _largest(a):
    return np.unravel_index(np.abs(a).argmax(), a.shape)


# field -> (how the entry is picked, the check that must fail)
SCALED = [("A", "A"), ("B", "B"), ("b", "b"), ("P", "P"), ("R", "R"), ("q", "q"), ("r", "r"), ("Kx", "normal K"), ("ke", "normal k"), ("Z", "D T"),
          ("dF", "dF"), ("qf", "qf"), ("rf", "rf"), ("dt", "dt"), ("dq", "dq")]
META = [(0, "n_f"), (1, "n_f + n_z"), (2, "mode"), (3, "cost"), (4, "dyn_sse"), (5, "eq_sse")]


def test_the_checker_bites(oracle, problem, nodes, twin):
    """For each exported field in turn, on a copy of a passing record (the 60-node trot instance at the generic iterate): its largest entry
    scaled by 1 + 1e-9, or one padded zero set to 1e-12; the named check must fail (and the untouched record passes)."""
    inst = int(np.argmax(problem[0]["n_nodes"]))
    nodes, good = nodes["b"][inst], twin["b"][inst]
    lr.check_record(oracle, nodes, good, BOUND, tag="untouched")

    def must_fail(name, edit):
        rec = {key: v.copy() for key, v in good.items()}
        edit(rec)
        with pytest.raises(AssertionError) as err:
            lr.check_record(oracle, nodes, rec, BOUND, tag=f"edited for [{name}]", verbose=False)
        assert f"[{name}]" in str(err.value), (name, str(err.value))

    def scale(field):
        def edit(rec):
            rec[field][_largest(rec[field])] *= 1.0 + 1e-9
        return edit

    for field, name in SCALED:
        must_fail(name, scale(field))
    for col, name in META:
        def edit(rec, col=col):
            k = _largest(rec["meta"][:, col])[0]
            rec["meta"][k, col] *= 1.0 + 1e-9
        must_fail(name, edit)

    def q_pair(rec):   # both halves: the symmetric Q~ itself is wrong
        k, i, j = _largest(rec["Q"])
        rec["Q"][k, i, j] *= 1.0 + 1e-9
        rec["Q"][k, j, i] = rec["Q"][k, i, j]
    must_fail("Q", q_pair)

    def q_half(rec):
        k, i, j = _largest(rec["Q"] * (1.0 - np.eye(22)))
        rec["Q"][k, i, j] *= 1.0 + 1e-9
    must_fail("Q symmetric", q_half)

    def n_til(rec):
        rec["n_til"][3] += 1
    must_fail("n_f + n_z", n_til)
    # padded zeros: a stage of width 9 (one leg in contact) has padding in every block
    k9 = int(np.flatnonzero(good["n_til"] == 9)[0])
    n_z = int(good["meta"][k9, 1])
    assert n_z < 6
    contact_foot = lr.contact_flags(int(good["meta"][k9, 2])).index(True)
    for field, index, name in (("R", (k9, 11, 2), "R padding"), ("R", (k9, 10, 11), "R padding"), ("B", (k9, 4, 9), "B padding"),
                               ("P", (k9, 9, 0), "P padding"), ("r", (k9, 11), "r padding"), ("Z", (k9, 0, n_z), "Z padding"),
                               ("dF", (k9, 3 * contact_foot), "dF")):
        def edit(rec, field=field, index=index):
            assert rec[field][index] == 0.0
            rec[field][index] = 1e-12
        must_fail(name, edit)
    # the unit diagonal of the R~ padding
    def diag(rec):
        rec["R"][k9, 11, 11] = 1.0 + 1e-12
    must_fail("R padding", diag)
