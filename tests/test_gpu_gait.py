"""The device-resident gait manager (hb_gait_reset: k_gait ahead of the reference-generation kernels) on the GPU:

  * replay of the compiled reference manager's sequences (tests/golden/ref_refmgr.json) next to a context that gets its schedules from
    the host classes: windows, levels, velocities as the golden; node tables of the two contexts bit-identical on every call;
  * a batch of 512 with per-instance random request sequences through the enqueue-only hb_refgen_update against gait.py twins;
  * hb_tick_resident on four instance ranges against one stream: gait state, windows, tables, WBC solutions bit-identical;
  * the failure surface, and hb_gait_disable back to the host path.
"""
import json
from pathlib import Path

import numpy as np
import pytest

from _gait_twin import SEED, THRESHOLDS, HostTwin, random_passes

from hunter_bipedal_control_amd import abi, workload

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
TABLES = ("n_nodes", "t", "mode", "x_ref", "swing")


@pytest.fixture(scope="module")
def golden():
    return json.loads((HERE / "golden/ref_refmgr.json").read_text())


def _same_tables(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in TABLES)


def _request4(call):
    r = call["request"]
    return np.array([[r[0], r[1], 0.0, r[2]]])


def _persistent(st, i):
    n = int(st["n_events"][i])
    return st["event_times"][i, :n].tolist(), st["modes"][i, :n + 1].tolist()


def test_golden_replay_on_the_device_next_to_the_host_path(golden, params):
    from hunter_bipedal_control_amd.solver import HunterSolver
    levels, n_calls = set(), 0
    for seq in golden["sequences"]:
        T = seq["horizon"]
        nmax = max(call["n_nodes"] for call in seq["calls"] if call["full"]) + 6
        twin = HostTwin(params, 1, filter_cmd=True)
        host, dev = HunterSolver(params, batch=1, max_nodes=nmax), HunterSolver(params, batch=1, max_nodes=nmax)
        try:
            for s in (host, dev):
                s.refgen_reset(abi.make_refgen_config(params, joint_ik=True), latest_stance=np.zeros((1, 4, 3)))
            dev.gait_reset(abi.make_gait_config(params, filter_cmd=True))
            for call in seq["calls"]:
                t, x, o = np.array([call["t"]]), np.array([call["x"]]), call["out"]
                wins, cmd = twin.step(t, T, x, _request4(call))
                host.refgen_set_schedule(wins)
                assert host.refgen_update(t, T, x, cmd)[0] == 0, call["t"]
                assert dev.refgen_update(t, T, x, _request4(call))[0] == 0, call["t"]
                win, st = dev.refgen_schedule()[0], dev.gait_state()
                assert st["cmd"][0].tolist() == call["cmd"], call["t"]
                assert list(win.event_times) == o["ev"] and list(win.modes) == o["modes"], call["t"]
                assert abs(st["vel_abs"][0] - o["vel_abs"]) < 1e-14 and abs(st["vel_avg"][0] - o["vel_avg"]) < 1e-14, call["t"]
                assert int(st["level"][0]) == o["gait_level"] and int(st["status"][0]) == 0, call["t"]
                assert _same_tables(host.get_references(), dev.get_references()), call["t"]
                levels.add(int(st["level"][0]))
                n_calls += 1
        finally:
            host.close()
            dev.close()
    assert n_calls == 528 and levels == {0, 1, 3}


def _standing_observations(params, x_rand):
    """The random observations of _gait_twin with a sensible body: task.info's initial state, the drawn position offsets and angles."""
    x = np.tile(np.array(params["config"]["initial_state"], dtype=float), (x_rand.shape[0], 1))
    x[:, 6:8] += 0.05 * x_rand[:, 6:8]
    x[:, 9:12] = x_rand[:, 9:12]
    return x


def test_batch_of_512_follows_its_host_twins(params):
    from hunter_bipedal_control_amd.solver import HunterSolver
    B, n_pass, T = 512, 200, 1.0
    passes = random_passes(B, n_pass, SEED + 7)
    probe = HostTwin(params, B)
    margin = np.inf
    obs = [_standing_observations(params, x) for _, x, _ in passes]
    for (t0, _, req), x in zip(passes, obs):
        probe.step(t0, T, x, req)
        margin = min(margin, min(abs(s.vel_avg - th) for s in probe.sel for th in THRESHOLDS))
    assert margin > 1e-9, margin                      # no decision of the committed seed hangs on the last bit of sin / cos
    twin = HostTwin(params, B)
    s = HunterSolver(params, batch=B, max_nodes=100)
    try:
        s.refgen_reset(abi.make_refgen_config(params, joint_ik=True))
        s.gait_reset(abi.make_gait_config(params, filter_cmd=True))
        seen = set()
        for k, ((t0, _, req), x) in enumerate(zip(passes, obs)):
            wins, cmd = twin.step(t0, T, x, req)
            s.refgen_update(t0, T, x, req, want_status=False)
            if k % 10 == 9 or k == n_pass - 1:
                got, st = s.refgen_schedule(), s.gait_state()
                assert st["level"].tolist() == twin.levels, k
                assert st["cmd"].tolist() == cmd.tolist(), k
                for i in range(B):
                    assert (got[i].event_times, got[i].modes) == (list(wins[i].event_times), list(wins[i].modes)), (k, i)
                    assert _persistent(st, i) == (list(twin.gs[i].s.event_times), list(twin.gs[i].s.modes)), (k, i)
                assert not st["status"].any()
                assert s.refgen_status().max() == 0, k
                seen |= set(twin.levels)
        assert seen == {0, 1, 3} and twin.insertions > 200
    finally:
        s.close()


def _tick_run(params, ranges, n_ticks=24, n_steps=8):
    from hunter_bipedal_control_amd.solver import HunterSolver
    B, N = 64, 40
    horizon = N * params["config"]["dt"]
    s = HunterSolver(params, batch=B, max_nodes=N + 8)
    try:
        w = workload.device_trot_batch(s, params, n_intervals=N)
        s.set_resident_inputs(w["x0"], w["t_now"], w["rbd"])
        s.set_chunks(ranges)
        xh0 = np.zeros((B, 18))
        xh0[:, 0:3] = w["rbd"][:, 3:6]
        xh0[:, 6:18] = np.asarray(s.eval_foot_kinematics(w["x0"], np.zeros((B, 22)))[0]).reshape(B, 12)
        s.estimator_reset(abi.make_estimator_config(params), xh0)
        s.gait_reset(abi.make_gait_config(params, filter_cmd=True))
        srng = np.random.default_rng(6)
        req = np.zeros((B, 4))
        snaps = []
        for k in range(n_ticks):
            tk = w["t_now"] + 0.01 * (k + 1)
            quat = np.tile([0.0, 0.0, 0.0, 1.0], (B, 1)) + 0.01 * srng.standard_normal((B, 4))
            quat /= np.linalg.norm(quat, axis=1, keepdims=True)
            wl, al = 0.05 * srng.standard_normal((B, 3)), np.tile([0.0, 0.0, 9.81], (B, 1)) + 0.1 * srng.standard_normal((B, 3))
            qj, qdj = w["rbd"][:, 6:16] + 0.01 * srng.standard_normal((B, 10)), 0.1 * srng.standard_normal((B, 10))
            if k == 2:
                req[0::2, 0] = 0.3                      # every other robot is told to walk ...
            if k == 6:
                req[0::4, 0] = 1.2                      # ... half of those to run (level 3) ...
            if k == 14:
                req[0::8] = 0.0                         # ... and some to stop again
            s.tick_resident(0.002, quat, wl, al, qj, qdj, np.ones((B, 4), dtype=np.int32), tk, horizon, req)
            if k in (5, 15, n_ticks - 1):
                snaps.append((s.gait_state(), s.refgen_schedule(), s.get_references(), s.get_wbc_solution(), s.mpc_status()))
        assert s.refgen_status().max() == 0
        for _ in range(n_steps):                        # the steady state of hb_step_resident: replayed range graphs
            s.step_resident()
        snaps.append((s.gait_state(), s.refgen_schedule(), s.get_references(), s.get_wbc_solution(), s.mpc_status()))
        return snaps, s.chunk_counters()
    finally:
        s.close()


def test_tick_on_four_ranges_equals_one_stream(params):
    """The ranges of hb_tick_resident enqueue their slice of the tick directly, k_gait included, as they do without the manager; the
    hb_step_resident steps behind them replay the range graphs (captured after the manager was switched on)."""
    one, c1 = _tick_run(params, 1)
    four, c4 = _tick_run(params, 4)
    assert c1["graph_launches"] == 0 and c4["forks"] >= 1
    assert c4["graph_launches"] > 0 and c4["capture_failures"] == 0 and c4["graphs_disabled"] == 0, c4
    levels = set()
    for (ga, wa, ra, sa, ma), (gb, wb, rb, sb, mb) in zip(one, four):
        for k in ga:
            assert np.array_equal(ga[k], gb[k]), k
        assert [(w.event_times, w.modes) for w in wa] == [(w.event_times, w.modes) for w in wb]
        assert _same_tables(ra, rb)
        assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]) and np.array_equal(ma, mb)
        assert not ga["status"].any()
        levels |= set(ga["level"].tolist())
    assert levels == {0, 1, 3}, levels                  # the commands really moved robots between the gaits


def test_failure_surface_and_back_to_the_host_path(golden, params):
    from hunter_bipedal_control_amd.solver import HunterHipError, HunterSolver
    seq = golden["sequences"][1]
    T = seq["horizon"]
    calls = seq["calls"][:60]
    nmax = max(call["n_nodes"] for call in seq["calls"] if call["full"]) + 6
    twin = HostTwin(params, 1, filter_cmd=True)
    plain, dev = HunterSolver(params, batch=1, max_nodes=nmax), HunterSolver(params, batch=1, max_nodes=nmax)
    try:
        with pytest.raises(HunterHipError, match=r"\(-3\).*hb_refgen_reset"):
            dev.gait_reset(abi.make_gait_config(params))
        for s in (plain, dev):
            s.refgen_reset(abi.make_refgen_config(params, joint_ik=True), latest_stance=np.zeros((1, 4, 3)))
        dev.gait_reset(abi.make_gait_config(params, filter_cmd=True))
        with pytest.raises(HunterHipError, match=r"\(-3\)") as e:
            dev.refgen_set_schedule([twin.gs[0].s])
        assert "hb_gait_reset" in str(e.value) and "hb_gait_disable" in str(e.value)
        for k, call in enumerate(calls):
            t, x = np.array([call["t"]]), np.array([call["x"]])
            wins, cmd = twin.step(t, T, x, _request4(call))
            plain.refgen_set_schedule(wins)
            assert plain.refgen_update(t, T, x, cmd)[0] == 0
            if k == 30:
                dev.gait_disable()
                with pytest.raises(HunterHipError, match=r"\(-3\)"):
                    dev.gait_insert_template([0.0, 0.3, 0.6], [2, 1], [1.0], [2.0])
            if k < 30:
                assert dev.refgen_update(t, T, x, _request4(call))[0] == 0
            else:
                dev.refgen_set_schedule(wins)
                assert dev.refgen_update(t, T, x, cmd)[0] == 0
            assert _same_tables(plain.get_references(), dev.get_references()), k
            got = dev.refgen_schedule()[0]
            assert (got.event_times, got.modes) == (list(wins[0].event_times), list(wins[0].modes)), k
    finally:
        plain.close()
        dev.close()
