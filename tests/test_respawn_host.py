"""CPU: the respawn routines (csrc/hb_respawn.hpp, compiled for the host: what k_plant_respawn runs per instance) against the independent
numpy twin of the definition in include/hunter_hip.h (tests/_respawnemu.py).  Decision and fold: exact.  Draw: the Philox words exact, the
normals, the uniform and the perturbed state within the tolerance tests/test_sensors_host.py applies to the same Box-Muller normals between
builds (1e-12 for sigma <= 1), a channel with range / sigma 0 bit for bit.  Placement: the lowest gap equals the clearance within the
bound the terrain host tests hold gaps to (tests/_terrainemu.py TOL_Q)."""
import ctypes as C
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

import _contactemu as ce
import _episodeemu as ee
import _respawnemu as rs
import _terrainemu as te
from hunter_bipedal_control_amd import abi

_p = rs._p
Q_SPAWN = np.concatenate([[0.1, -0.2, 0.62, 0.3, 0.01, -0.02], np.linspace(-0.4, 0.5, 10)])
V_SPAWN = np.linspace(-0.1, 0.2, 16)


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(str(rs.build()))
    lib.re_config_refusal.restype = C.c_char_p
    lib.re_stream.restype = C.c_uint
    return lib


def _pack(rec):
    """A record dict of one instance -> irec[HB_EP_NI], drec[HB_EP_ND]."""
    irec, drec = np.zeros(abi.HB_EP_NI, dtype=np.int32), np.zeros(abi.HB_EP_ND)
    for table, out in ((abi.EPISODE_INT_FIELDS, irec), (abi.EPISODE_DOUBLE_FIELDS, drec)):
        for name, at, n in table:
            out[at:at + n] = rec[name]
    return irec, drec


def _rec(**kw):
    r = rs.init_record(Q_SPAWN, [0.0, 0.0, 1.0, 0.0])
    r.update(kw)
    return r


def test_decision_table(lib):
    """END_TICK in {-1, k} x steps since the end {<, =, >} hold_ticks x TICKS {<, =, >} max_ticks, and max_ticks = 0."""
    hold, k = 3, 4
    for max_ticks, end, since, dticks in itertools.product((0, 6), (-1, k), (hold - 1, hold, hold + 1), (-1, 0, 1)):
        cfg = abi.make_respawn_config(hold_ticks=hold, max_ticks=max_ticks)
        ticks = (max_ticks if max_ticks else 6) + dticks
        rec = _rec(END_TICK=end, END_CAUSE=abi.HB_EP_FALLEN if end >= 0 else abi.HB_EP_RUNNING, STEPS=(end + 1 + since) if end >= 0 else ticks,
                   TICKS=ticks)
        want = (abi.HB_EP_FALLEN if since >= hold else 0) if end >= 0 else (abi.HB_RS_TIMEOUT if max_ticks and dticks >= 0 else 0)
        irec, _ = _pack(rec)
        assert lib.re_decide(C.byref(cfg), _p(irec)) == want == rs.decide(cfg, rec), (max_ticks, end, since, dticks)
    # the cause of an ended instance is its own
    rec = _rec(END_TICK=2, END_CAUSE=abi.HB_EP_NONFINITE, STEPS=3, TICKS=99)
    assert lib.re_decide(C.byref(abi.make_respawn_config(max_ticks=5)), _p(_pack(rec)[0])) == abi.HB_EP_NONFINITE


@pytest.fixture(scope="module")
def real_records(params):
    """The records of the five terrain scenarios after 20 ticks of the host build of the ground-contact plant (as tests/test_episode_host.py
    builds them), with a tilt limit that scenario 2 starts beyond."""
    elib, tlib = C.CDLL(str(ee.build())), C.CDLL(str(te.build()))
    qv_fn, foot_fn, q_stand = ce.oracle_fns(params)
    mdl = abi.make_model(params)
    pcfg = abi.make_contact_config(params, mu=0.31, ground_z=0.123, erp=te.ERP, sweeps=te.SWEEPS)
    cfg = abi.make_episode_config(slip_speed=0.05, tilt_limit=0.025)
    out = []
    for sc in te.scenarios(q_stand, qv_fn, foot_fn):
        rec = te.record_of(sc["plane"], sc["mu"])
        q, v, p, status, ticks = sc["q0"], sc["v0"], np.zeros(12), 0, []
        for tick in range(20):
            tau = sc["tau_fn"](tick)
            o = te.emu_step(tlib, mdl, pcfg, rec, q, v, p, tau, None, status, None, np.zeros(20))
            q, v, p, status = o["q"], o["v"], o["p"], o["status"]
            ticks.append(dict(q=q, v=v, tau_last=tau, wbc_status=None, gap=o["gap"], lam=o["lam"], point_vel=o["point_vel"], residual=o["residual"],
                              touching=o["touching"], status=status, jresidual=None, jstatus=None))
        out.append(ee.host_record(elib, cfg, sc["plane"], sc["q0"], ee.stack(ticks), te.DT)[0])
    return out


def test_fold_of_real_records_three_times_over(lib, real_records):
    cfg = abi.make_respawn_config(max_ticks=10)
    causes = [rs.decide(cfg, r) for r in real_records]
    assert abi.HB_EP_FALLEN in causes and abi.HB_RS_TIMEOUT in causes and 0 not in causes
    itot, dtot = np.full(abi.HB_RS_NI, 7, dtype=np.int32), np.full(abi.HB_RS_ND, 7.0)
    lib.re_totals_init(_p(itot), _p(dtot))
    tw = rs.totals_init()
    assert not itot.any() and not dtot.any()
    for rnd in range(3):
        for rec, cause in zip(real_records, causes):
            irec, drec = _pack(rec)
            assert lib.re_decide(C.byref(cfg), _p(irec)) == cause
            lib.re_fold(C.c_int(cause), _p(irec), _p(drec), _p(itot), _p(dtot))
            itot[abi.RESPAWN_INT_FIELDS.index("EPISODE_INDEX")] += 1      # (step 5 is the caller's)
            tw = rs.fold(tw, rec, cause)
            dev = abi.split_respawn_totals(itot[None], dtot[None])
            for name in abi.RESPAWN_INT_FIELDS + abi.RESPAWN_DOUBLE_FIELDS:
                assert dev[name][0] == tw[name], (rnd, name, dev[name][0], tw[name])
    n = 3 * len(real_records)
    assert tw["EPISODES"] == tw["EPISODE_INDEX"] == n == tw["N_FALLEN"] + tw["N_NONFINITE"] + tw["N_TIMEOUT"]
    assert tw["TICKS_MIN"] == min(r["TICKS"] for r in real_records) and tw["TICKS_MAX"] == 20 and tw["STEPS_SUM"] == 20 * n
    assert tw["TAU_MAX"] > 0.0 and tw["WORK_ABS_SUM"] > 0.0


def _draw(lib, cfg, inst, episode):
    draw, words, gen = np.full(20, np.nan), np.zeros(20, dtype=np.uint32), np.zeros(5, dtype=np.int32)
    lib.re_draw(C.byref(cfg), C.c_uint32(inst), C.c_uint32(episode), _p(draw), _p(words), _p(gen))
    return draw, words, gen


def _state(lib, cfg, inst, episode, v_spawn=V_SPAWN):
    draw = _draw(lib, cfg, inst, episode)[0]
    q, v = np.zeros(16), np.zeros(16)
    lib.re_perturb(C.byref(cfg), _p(Q_SPAWN), None if v_spawn is None else _p(v_spawn), _p(draw), _p(q), _p(v))
    return q, v


def test_draw_words_normals_and_state(lib):
    assert lib.re_stream() == abi.HB_RS_STREAM
    cfg = abi.make_respawn_config(yaw_range=0.5, joint_pos_sigma=0.1, base_vel_sigma=0.3, seed=0x1234567890ABCDEF)
    for inst, episode in ((0, 1), (3, 1), (3, 2), (0xFFFFFFFF, 77)):
        draw, words, gen = _draw(lib, cfg, inst, episode)
        assert gen.tolist() == [1] * 5
        for b in range(5):
            want = rs.block_words(cfg, inst, episode, b)
            assert words[4 * b:4 * b + 4].tolist() == want, (inst, episode, b)
            if b:
                assert np.abs(draw[4 * b:4 * b + 4] - rs._normals4(want)).max() <= rs.NORMAL_TOL
        assert abs(draw[0] - (rs.block_words(cfg, inst, episode, 0)[0] + 0.5) * 2.0 ** -32) <= rs.NORMAL_TOL and 0.0 < draw[0] < 1.0
        q, v = _state(lib, cfg, inst, episode)
        qt, vt = rs.spawn_state(cfg, inst, episode, Q_SPAWN, V_SPAWN)
        assert np.abs(q - qt).max() <= rs.NORMAL_TOL and np.abs(v - vt).max() <= rs.NORMAL_TOL
        assert abs(q[3] - Q_SPAWN[3]) <= 0.5 and np.array_equal(q[[0, 1, 2, 4, 5]], Q_SPAWN[[0, 1, 2, 4, 5]]) and np.array_equal(v[3:], V_SPAWN[3:])
        assert (q[6:] != Q_SPAWN[6:]).all() and (v[:3] != V_SPAWN[:3]).all() and q[3] != Q_SPAWN[3]
    a, b = _state(lib, cfg, 3, 1), _state(lib, cfg, 3, 2)
    assert not np.array_equal(a[0], b[0])                                       # another episode: another draw


def test_a_channel_that_is_off_leaves_the_value_bit_for_bit_and_draws_no_block(lib):
    on = dict(yaw_range=0.5, joint_pos_sigma=0.1, base_vel_sigma=0.3)
    blocks = dict(yaw_range=[0], joint_pos_sigma=[1, 2, 3], base_vel_sigma=[4])
    full = _state(lib, abi.make_respawn_config(seed=5, **on), 2, 1)
    for off in on:
        cfg = abi.make_respawn_config(seed=5, **{k: (0.0 if k == off else x) for k, x in on.items()})
        draw, _, gen = _draw(lib, cfg, 2, 1)
        assert [b for b in range(5) if not gen[b]] == blocks[off]
        assert all(np.isnan(draw[4 * b:4 * b + 4]).all() for b in blocks[off])    # not generated
        q, v = _state(lib, cfg, 2, 1)
        if off == "yaw_range":
            assert q[3] == Q_SPAWN[3]
        if off == "joint_pos_sigma":
            assert np.array_equal(q[6:], Q_SPAWN[6:])
        if off == "base_vel_sigma":
            assert np.array_equal(v, V_SPAWN)
        # the channels that stay on do not depend on the one that is off
        keep_q = [a for a in range(16) if not ((off == "yaw_range" and a == 3) or (off == "joint_pos_sigma" and a >= 6))]
        assert np.array_equal(q[keep_q], full[0][keep_q])
    q, v = _state(lib, abi.make_respawn_config(seed=5), 2, 1, v_spawn=None)
    assert np.array_equal(q, Q_SPAWN) and not v.any()


def test_same_seed_and_global_instance_give_the_same_bits(lib):
    on = dict(yaw_range=0.5, joint_pos_sigma=0.1, base_vel_sigma=0.3, seed=99)
    whole, shard = abi.make_respawn_config(instance_offset=0, **on), abi.make_respawn_config(instance_offset=2, **on)
    for i in range(2):
        a = _state(lib, whole, whole.instance_offset + 2 + i, 4)
        b = _state(lib, shard, shard.instance_offset + i, 4)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(_state(lib, whole, 2, 4)[0], _state(lib, abi.make_respawn_config(**{**on, "seed": 100}), 2, 4)[0])


@pytest.mark.parametrize("normal", [(0.0, 0.0), (te.SLOPE, 0.0), (0.15, -0.1)])
def test_placement_puts_the_lowest_point_at_the_clearance(lib, params, normal):
    _, foot_fn, q_stand = ce.oracle_fns(params)
    mdl = abi.make_model(params)
    plane = np.concatenate([te.normal_of(*normal), [0.07]])
    q0 = np.array(q_stand, dtype=float)
    q0[3:6] += [0.2, 0.03, -0.04]
    q0[6:] += np.linspace(-0.05, 0.05, 10)
    for clearance in (0.0, 0.013):
        cfg = abi.make_respawn_config(place=1, clearance=clearance)
        q, feet = q0.copy(), np.zeros(12)
        lib.re_place(C.byref(mdl), C.byref(cfg), _p(plane), _p(q), _p(feet))
        assert abs(rs.lowest_gap(q, foot_fn, plane) - clearance) <= te.TOL_Q
        assert np.abs(q - rs.place(cfg, q0, foot_fn, plane)).max() <= te.TOL_Q and np.array_equal(q[3:], q0[3:])
        assert np.abs(feet.reshape(4, 3) - np.asarray(foot_fn(q[None]))[0]).max() <= te.TOL_Q    # the contact points of the placed state
    q = q0.copy()
    lib.re_place(C.byref(mdl), C.byref(abi.make_respawn_config(place=0, clearance=0.5)), _p(plane), _p(q), _p(np.zeros(12)))
    assert np.array_equal(q, q0)


def test_every_refusal_of_the_configuration(lib):
    assert lib.re_config_refusal(C.byref(abi.make_respawn_config())) is None
    assert lib.re_config_refusal(C.byref(abi.make_respawn_config(clearance=0.1, yaw_range=3.0, joint_pos_sigma=0.2, base_vel_sigma=1.0, hold_ticks=5,
                                                                 max_ticks=1000, place=1, seed=2 ** 64 - 1, instance_offset=2 ** 32 - 1))) is None
    nan, inf = float("nan"), float("inf")
    for field in ("clearance", "yaw_range", "joint_pos_sigma", "base_vel_sigma"):
        for bad in (-1e-9, nan, inf):
            why = lib.re_config_refusal(C.byref(abi.make_respawn_config(**{field: bad})))
            assert why is not None and field in why.decode(), (field, bad, why)
    for field, bad in (("hold_ticks", -1), ("max_ticks", -1), ("place", 2), ("place", -1)):
        why = lib.re_config_refusal(C.byref(abi.make_respawn_config(**{field: bad})))
        assert why is not None and field in why.decode(), (field, bad, why)
    for k in range(2):
        cfg = abi.make_respawn_config()
        cfg.reserved[k] = 1
        assert b"reserved" in lib.re_config_refusal(C.byref(cfg))
    with pytest.raises(TypeError):
        abi.make_respawn_config(hold=3)


def test_struct_and_index_tables_mirror_the_header(lib):
    header = (Path(__file__).resolve().parents[1] / "include" / "hunter_hip.h").read_text()
    for prefix, table in (("HB_RS_I_", abi.RESPAWN_INT_FIELDS), ("HB_RS_D_", abi.RESPAWN_DOUBLE_FIELDS)):
        found = {m.group(1): int(m.group(2)) for m in re.finditer(prefix + r"([A-Z_]+) = (\d+)", header)}
        assert found == {name: at for at, name in enumerate(table)}
    assert (lib.re_ni(), lib.re_nd()) == (abi.HB_RS_NI, abi.HB_RS_ND) == (13, 5)
    assert f"#define HB_RS_TIMEOUT {abi.HB_RS_TIMEOUT}" in header and f"#define HB_RS_STREAM 0x{abi.HB_RS_STREAM:X}u" in header
    assert C.sizeof(abi.HbRespawnConfig) == lib.re_config_size() == 64
    off = np.zeros(10, dtype=np.int32)
    lib.re_config_offsets(_p(off))
    names = [n for n, _ in abi.HbRespawnConfig._fields_]
    assert names == ["clearance", "yaw_range", "joint_pos_sigma", "base_vel_sigma", "seed", "instance_offset", "hold_ticks", "max_ticks", "place",
                     "reserved"]
    assert off.tolist() == [getattr(abi.HbRespawnConfig, n).offset for n in names]
    body = header[header.index("typedef struct hb_respawn_config {"):header.index("} hb_respawn_config;")]
    assert re.findall(r"(?:double|uint64_t|uint32_t|int32_t) (\w+)", body) == names   # the declaration order is the order of the table


def test_the_rows_of_a_respawned_instance(lib, params):
    """Steps 4 - 8 on rows full of sevens: what is written, and that the episode record restarts from the new state."""
    mdl = abi.make_model(params)
    _, foot_fn, q_stand = ce.oracle_fns(params)
    q, v = np.array(q_stand, dtype=float), 0.1 * V_SPAWN
    plane = np.concatenate([te.normal_of(0.15, -0.1), [0.02]])
    f = lambda n: np.full(n, 7.0)                                     # noqa: E731
    i = lambda n: np.full(n, 7, dtype=np.int32)                       # noqa: E731
    cap = 3
    a = dict(plant=f(114), iplant=i(8), last=f(32), contact=f(29), icontact=i(5), joints=f(51), jstatus=i(1), act=f(70),
             ts=np.full(1, 7, dtype=np.uint64), estop=i(1), irec=i(abi.HB_EP_NI), drec=f(abi.HB_EP_ND), trace=f(cap * 8), est=f(359), res=f(54),
             flags=i(2))
    lib.re_write(C.byref(mdl), _p(q), _p(v), _p(plane), _p(a["plant"]), _p(a["iplant"]), _p(a["last"]), _p(a["contact"]), _p(a["icontact"]),
                 _p(a["joints"]), _p(a["jstatus"]), _p(a["act"]), _p(a["ts"]), _p(a["estop"]), _p(a["irec"]), _p(a["drec"]), _p(a["trace"]),
                 C.c_int(cap), _p(a["est"]), _p(a["res"]), _p(a["flags"]))
    feet = np.asarray(foot_fn(q[None]))[0].reshape(12)
    pl = a["plant"]
    assert np.array_equal(pl[0:16], q) and np.array_equal(pl[16:32], v) and np.array_equal(a["last"], np.concatenate([q, v]))
    assert np.abs(pl[32:44] - feet).max() <= te.TOL_Q and not pl[44:82].any()                     # anchor | lambda, vdot, tau_last
    assert a["iplant"].tolist() == [0] * 4 + [1] * 4
    rbd = pl[82:114]
    assert np.array_equal(rbd[0:3], q[3:6]) and np.array_equal(rbd[3:6], q[0:3]) and np.array_equal(rbd[6:16], q[6:]) and np.array_equal(rbd[19:22], v[0:3])
    assert np.array_equal(a["res"][:32], rbd) and np.array_equal(a["res"][32 + 6:32 + 12], np.concatenate([q[0:3], q[3:6]]))
    for k in ("contact", "icontact", "joints", "jstatus", "act", "ts", "estop", "trace"):
        assert not a[k].any(), k
    est = a["est"]
    assert np.array_equal(est[0:3], q[0:3]) and not est[3:6].any() and np.array_equal(est[6:18], pl[32:44])
    assert np.array_equal(est[18:342].reshape(18, 18), 100.0 * np.eye(18)) and not est[342:].any()
    assert a["flags"].tolist() == [1, 1]
    rec = {k: x[0] for k, x in abi.split_episode_record(a["irec"][None], a["drec"][None]).items()}
    want = rs.init_record(q, plane)
    for name, _, _ in abi.EPISODE_INT_FIELDS + abi.EPISODE_DOUBLE_FIELDS:
        if name == "HEIGHT_LAST":
            assert abs(rec[name] - want[name]) <= 8 * ee.U * np.abs(plane[:3] * q[:3]).max()
        else:
            assert np.array_equal(rec[name], want[name]), name
