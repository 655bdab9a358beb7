"""CPU: the profile-draw routines (csrc/hb_profiledraw.hpp, compiled for the host: what k_plant_profile_draw runs per instance and what
k_plant_respawn runs on a profile) against the independent twin of the definition in include/hunter_hip.h (tests/_profiledrawemu.py) and
against the host setters' own records (profile_record, ground_record).  The draw uses no transcendental function, so everything up to the
records is exact: the Philox words, the uniforms, the kind, the knots, the parameter row, the log row, and the records byte for byte.  The
placement goes through the leg kinematics; its bound is derived where it is used."""
import ctypes as C

import numpy as np
import pytest

import _profiledrawemu as pd
from hunter_bipedal_control_amd import abi, rollout

_p = pd._p
EPS = 2.0 ** -52
CASES = ((0, 1), (3, 1), (3, 2), (0xFFFFFFFF, 77), (4103, 1000), (12, 5), (13, 5))
Q_SPAWN = np.array([0.31, -0.17])
GROUND_Z, CFG_MU = 0.123, 0.31
KMAX = abi.HB_PROFILE_MAX_KNOTS


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(str(pd.build()))
    lib.pd_config_refusal.restype = C.c_char_p
    lib.pd_stream.restype = C.c_uint
    return lib


@pytest.fixture(scope="module")
def mdl(params):
    return abi.make_model(params)


def _cfg(name="host_all", **over):
    return abi.make_profile_draw_config(**{**pd.CONFIGS[name], **over})


def _draw(lib, cfg, inst, episode):
    u, words = np.full(12, np.nan), np.zeros(12, dtype=np.uint32)
    lib.pd_draw(C.byref(cfg), C.c_uint32(inst), C.c_uint32(episode), _p(u), _p(words))
    return u, words


def _compose(lib, cfg, u, q_spawn=Q_SPAWN, ground_z=GROUND_Z):
    a, rel, kn, row = np.full(2, np.nan), np.full(2 * KMAX, np.nan), np.full(2 * KMAX, np.nan), np.full(abi.HB_PD_N, np.nan)
    pro, gmap = np.full(lib.pd_profile_stored(), np.nan), np.full(lib.pd_ground_size(), np.nan)
    nk = lib.pd_compose(C.byref(cfg), _p(u), _p(np.array(q_spawn, dtype=float)), C.c_double(ground_z), _p(a), _p(rel), _p(kn), _p(row), _p(pro), _p(gmap))
    return dict(nk=nk, a=a, rel=rel.reshape(KMAX, 2), knots=kn.reshape(KMAX, 2), row=row, pro=pro, map=gmap)


def _profile_record(lib, nk, direction, knots, mu, cfg_mu=CFG_MU):
    rec, why = np.full(lib.pd_profile_stored(), np.nan), C.create_string_buffer(128)
    rc = lib.pd_profile_record(int(nk), _p(np.array(direction, dtype=float)), _p(np.ascontiguousarray(knots, dtype=float)),
                               None if mu is None else _p(np.array(mu, dtype=float)), C.c_double(cfg_mu), _p(rec), why)
    return (rec, None) if rc == 0 else (None, why.value.decode())


def _ground_record(lib, nk, direction, knots):
    rec, why = np.full(lib.pd_ground_size(), np.nan), C.create_string_buffer(128)
    rc = lib.pd_ground_record(int(nk), _p(np.array(direction, dtype=float)), _p(np.ascontiguousarray(knots, dtype=float)), _p(rec), why)
    return (rec, None) if rc == 0 else (None, why.value.decode())


def _same_bytes(a, b):
    return np.asarray(a, dtype=float).tobytes() == np.asarray(b, dtype=float).tobytes()


def _kind_variants():
    return [("host_all", {})] + [("host_all", dict(kinds=k)) for k in (abi.HB_PD_FLAT, abi.HB_PD_CURB, abi.HB_PD_STAIRS)]


# ---- exact parity ----------------------------------------------------------------------------------------------------------------------------
def test_struct_and_constants_are_the_headers(lib):
    assert lib.pd_n() == abi.HB_PD_N == 9 and lib.pd_log_w() == abi.HB_PD_LOG_W == 14 and lib.pd_log_max() == abi.HB_PD_LOG_MAX
    assert lib.pd_stream() == abi.HB_PD_STREAM and len({abi.HB_PD_STREAM, abi.HB_SC_STREAM, abi.HB_RS_STREAM}) == 3
    assert lib.pd_blocks() == pd.NBLOCKS and lib.pd_config_size() == C.sizeof(abi.HbProfileDrawConfig)
    off = np.zeros(18, dtype=np.int32)
    lib.pd_config_offsets(_p(off))
    names = ["seed", "kinds", "mu_per_point", "dir", "height_lo", "height_hi", "at_lo", "at_hi", "riser_slope", "steps_lo", "steps_hi", "run_lo",
             "run_hi", "mu_lo", "mu_hi", "follow_map", "log_capacity", "reserved"]
    assert [f[0] for f in abi.HbProfileDrawConfig._fields_] == names
    assert off.tolist() == [getattr(abi.HbProfileDrawConfig, n).offset for n in names]


def test_words_uniforms_kind_knots_and_row_are_the_twins(lib):
    seen = set()
    for name, over in _kind_variants():
        cfg = _cfg(name, **over)
        for inst, episode in CASES:
            u, words = _draw(lib, cfg, inst, episode)
            for b in range(pd.NBLOCKS):
                want = pd.block_words(cfg, inst, episode, b)
                assert words[4 * b:4 * b + 4].tolist() == want, (inst, episode, b)
                assert u[4 * b:4 * b + 4].tolist() == [pd.uniform(w) for w in want]
            assert (0.0 < u).all() and (u < 1.0).all()
            got = _compose(lib, cfg, u)
            tw = pd.draw(cfg, inst, episode, Q_SPAWN, GROUND_Z)
            nk = len(tw["rel"])
            assert got["nk"] == nk and got["row"][0] == tw["kind"] and tw["kind"] in pd.kinds_of(cfg)
            assert _same_bytes(got["a"], tw["a"])
            assert _same_bytes(got["rel"], pd.padded(tw["rel"])), (name, over, inst, episode)
            assert _same_bytes(got["knots"], pd.padded(tw["knots"]))
            assert _same_bytes(got["row"], tw["row"]), (got["row"], tw["row"])
            seen.add(tw["kind"])
            r = abi.split_profile_draw(got["row"])
            assert (cfg.mu_lo <= r["MUS"]).all() and (r["MUS"] <= cfg.mu_hi).all() and len(set(r["MUS"].tolist())) == 4
            if tw["kind"] == abi.HB_PD_FLAT:
                assert not got["row"][1:5].any() and nk == 2
            else:
                assert cfg.height_lo <= r["HEIGHT"] <= cfg.height_hi and cfg.at_lo <= r["AT"] <= cfg.at_hi
            if tw["kind"] == abi.HB_PD_CURB:
                # the knots of rollout.curb_profile(h, s_r, riser_slope), bit for bit
                assert not got["row"][3:5].any() and nk == 4
                assert _same_bytes(tw["rel"], rollout.curb_profile(float(r["HEIGHT"]), tw["s0"] + float(r["AT"]), cfg.riser_slope))
            if tw["kind"] == abi.HB_PD_STAIRS:
                assert cfg.steps_lo <= r["STEPS"] <= cfg.steps_hi and cfg.run_lo <= r["RUN"] <= cfg.run_hi and nk == 2 + 2 * int(r["STEPS"])
    assert seen == {abi.HB_PD_FLAT, abi.HB_PD_CURB, abi.HB_PD_STAIRS}
    # another episode: another draw;  the scenario's and the spawn state's streams keep their bits
    cfg = _cfg()
    assert _draw(lib, cfg, 3, 1)[1].tolist() != _draw(lib, cfg, 3, 2)[1].tolist()
    import _respawnemu as rs
    import _scenarioemu as sc
    assert pd.block_words(cfg, 3, 1, 0) != rs.block_words(abi.make_respawn_config(seed=cfg.seed), 3, 1, 0)
    assert pd.block_words(cfg, 3, 1, 0) != sc.block_words(abi.make_scenario_config(seed=cfg.seed), 3, 1, 0)


def test_log_row_is_the_twins(lib):
    cfg = _cfg()
    a = np.array(pd.direction(cfg))
    irec, drec = np.zeros((1, abi.HB_EP_NI), dtype=np.int32), np.zeros((1, abi.HB_EP_ND))
    rng = np.random.default_rng(5)
    drec[0] = rng.normal(size=abi.HB_EP_ND)
    irec[0] = rng.integers(0, 50, size=abi.HB_EP_NI)
    rec = {k: v[0] for k, v in abi.split_episode_record(irec, drec).items()}
    itot = np.zeros(abi.HB_RS_NI, dtype=np.int32)
    itot[abi.RESPAWN_INT_FIELDS.index("EPISODE_INDEX")] = 6
    row = pd.draw(cfg, 3, 6, Q_SPAWN, GROUND_Z)["row"]
    count, log = np.zeros(1, dtype=np.int32), np.zeros((cfg.log_capacity, abi.HB_PD_LOG_W))
    for n in range(cfg.log_capacity + 2):                                      # (full: later episodes are not logged)
        lib.pd_log_append(cfg.log_capacity, abi.HB_RS_TIMEOUT, _p(a), _p(irec), _p(drec), _p(itot), _p(row), _p(count), _p(log))
        assert count[0] == min(n + 1, cfg.log_capacity)
    want = pd.log_row(6, abi.HB_RS_TIMEOUT, rec, row, a)
    assert all(_same_bytes(log[k], want) for k in range(cfg.log_capacity))
    assert abi.PROFILE_DRAW_LOG_HEAD == ("EPISODE", "CAUSE", "TICKS", "PROGRESS", "TILT_MAX")


# ---- record parity -----------------------------------------------------------------------------------------------------------------------------
def test_records_are_the_host_setters_byte_for_byte(lib):
    """The profile record the draw composes == what hb_plant_set_terrain_profile's routine stores for the twin's K, the direction as given,
    the twin's knots and the twin's mu; the map record == what hb_ground_set_profile's routine stores for the relative knots.  Both sides
    end in profile_compose / ground_compose (one routine, as terrain_plane_record is for the scenario), so what this proves is that the
    draw hands the composers the twin's inputs — K, the direction normalised once, every knot, every coefficient — and that validation
    accepts them; the record arithmetic itself is pinned by tests/test_profile_plant_host.py and tests/test_groundmap_host.py against their
    numpy definitions and by the second context of tests/test_gpu_profile_draw.py on the device."""
    for name, over in _kind_variants() + [("gpu_steps", {}), ("host_edge", {})]:
        cfg = _cfg(name, **over)
        for inst, episode in CASES:
            got = _compose(lib, cfg, _draw(lib, cfg, inst, episode)[0])
            tw = pd.draw(cfg, inst, episode, Q_SPAWN, GROUND_Z)
            rec, why = _profile_record(lib, len(tw["knots"]), cfg.dir, pd.padded(tw["knots"]), tw["mu"])
            assert why is None and _same_bytes(got["pro"], rec), (name, over, inst, episode, why)
            grec, why = _ground_record(lib, len(tw["rel"]), cfg.dir, pd.padded(tw["rel"]))
            assert why is None and _same_bytes(got["map"], grec), (name, over, inst, episode, why)


def test_flat_is_the_level_profile(lib):
    """FLAT with mu_lo = mu_hi = cfg.mu: the record of the level two-knot profile at ground_z with the contact model's mu, and so is the
    ground the set call starts every instance on."""
    cfg = _cfg(kinds=abi.HB_PD_FLAT, mu_lo=CFG_MU, mu_hi=CFG_MU)
    a = pd.direction(cfg)
    s0 = a[0] * Q_SPAWN[0] + a[1] * Q_SPAWN[1]
    level, why = _profile_record(lib, 2, cfg.dir, pd.padded([(s0 - 1.0, GROUND_Z), (s0 + 1.0, GROUND_Z)]), None)
    assert why is None
    for inst, episode in CASES:
        got = _compose(lib, cfg, _draw(lib, cfg, inst, episode)[0])
        assert got["nk"] == 2 and _same_bytes(got["pro"], level)
        assert not got["map"][lib.pd_ground_size() - (KMAX - 1):].any()                 # the zero map: no slope anywhere
    rel, kn, pro = np.zeros(2 * KMAX), np.zeros(2 * KMAX), np.zeros(lib.pd_profile_stored())
    assert lib.pd_flat(_p(np.array(cfg.dir[:])), _p(Q_SPAWN), C.c_double(GROUND_Z), C.c_double(CFG_MU), _p(rel), _p(kn), _p(pro)) == 2
    assert _same_bytes(pro, level)
    trel, tkn = pd.flat(cfg, Q_SPAWN, GROUND_Z)
    assert _same_bytes(rel.reshape(KMAX, 2), pd.padded(trel)) and _same_bytes(kn.reshape(KMAX, 2), pd.padded(tkn))
    # T = I and d = ground_z in both segments' place: the step without a terrain, value for value
    seg0 = level[14 + 2 + 1 + KMAX:][:10]
    assert np.array_equal(seg0[:9], np.eye(3).reshape(9)) and seg0[9] == GROUND_Z


def test_channels_are_independent(lib):
    """Disabling a kind or mu_per_point leaves every other block's values bit for bit."""
    full = _cfg()
    for inst, episode in CASES:
        u = _draw(lib, full, inst, episode)[0]
        ref = _compose(lib, full, u)
        kind = int(ref["row"][0])
        alone = _cfg(kinds=kind)
        assert _same_bytes(_draw(lib, alone, inst, episode)[0], u)
        got = _compose(lib, alone, u)
        assert _same_bytes(got["row"], ref["row"]) and _same_bytes(got["knots"], ref["knots"]) and _same_bytes(got["pro"], ref["pro"])
        one = _compose(lib, _cfg(mu_per_point=0), u)
        assert _same_bytes(one["row"][:5], ref["row"][:5]) and (one["row"][5:9] == ref["row"][5]).all() and _same_bytes(one["knots"], ref["knots"])
        # a kind taken out: height, first riser, steps and run are drawn as before, only the pick changes
        others = _compose(lib, _cfg(kinds=abi.HB_PD_CURB | abi.HB_PD_STAIRS), u)
        if others["row"][0] == kind:
            assert _same_bytes(others["row"], ref["row"])
        assert _same_bytes(others["row"][5:9], ref["row"][5:9])


# ---- validity ------------------------------------------------------------------------------------------------------------------------------------
def _sweep(lib, cfg, pairs, spawns):
    """-> (profiles drawn, refusals as (instance, episode, s0, why)) over pairs x spawns, the profile record's own check on every draw."""
    bad, n = [], 0
    a = pd.direction(cfg)
    for sx in spawns:
        q_spawn = np.array([sx * a[0], sx * a[1]])                             # s0 = sx to rounding
        for inst, episode in pairs:
            got = _compose(lib, cfg, _draw(lib, cfg, inst, episode)[0], q_spawn, GROUND_Z)
            rec, why = _profile_record(lib, got["nk"], cfg.dir, got["knots"], got["row"][5:9])
            n += 1
            if why is not None or got["nk"] > KMAX:
                bad.append((inst, episode, sx, why))
    return n, bad


def test_every_admitted_draw_is_a_valid_profile(lib):
    """A condition, not a measurement: over 21 000 (instance, episode) pairs — the configurations of this file and of
    tests/test_gpu_profile_draw.py and the edges of the admitted set, spawn points with s0 in {0, +-100, +-1000} — every drawn profile
    passes profile_record with K <= 16.  One step outside the admitted set (riser_slope 1.74 > sqrt(3)) the set call refuses the
    configuration and the same sweep, run on it regardless, finds profiles the record refuses."""
    spawns = (0.0, 100.0, -100.0, 1000.0, -1000.0)
    pairs = [(i, e) for i in (0, 1, 2, 77, 4103, 0xFFFFFFFF, 65536) for e in range(1, 101)]
    total = 0
    for name in pd.CONFIGS:
        cfg = _cfg(name)
        assert lib.pd_config_refusal(C.byref(cfg)) is None, name
        n, bad = _sweep(lib, cfg, pairs, spawns)
        assert not bad, (name, bad[:3])
        total += n
    assert total >= 20000
    steep = _cfg("host_all", riser_slope=1.74)
    assert b"riser_slope" in lib.pd_config_refusal(C.byref(steep))
    n, bad = _sweep(lib, steep, pairs[:100], spawns[:1])
    assert bad and all("steeper" in why for _, _, _, why in bad)


def test_every_refusal_names_its_field(lib):
    base = pd.CONFIGS["host_all"]
    assert lib.pd_config_refusal(C.byref(_cfg())) is None
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(kinds=0), "kinds"), (dict(kinds=8), "kinds"), (dict(kinds=-1), "kinds"), (dict(mu_per_point=2), "mu_per_point"),
        (dict(dir=(0.0, 0.0)), "dir"), (dict(dir=(nan, 1.0)), "dir"), (dict(dir=(1.0, inf)), "dir"),
        (dict(height_lo=nan), "height_lo"), (dict(height_hi=inf), "height_hi"), (dict(height_lo=0.1, height_hi=0.05), "height_hi"),
        (dict(at_lo=-1000.5), "at_lo"), (dict(at_lo=nan), "at_lo"), (dict(at_hi=1000.5), "at_hi"), (dict(at_lo=0.5, at_hi=0.4), "at_hi"),
        (dict(riser_slope=0.0), "riser_slope"), (dict(riser_slope=-1.0), "riser_slope"), (dict(riser_slope=1.7000001), "riser_slope"),
        (dict(riser_slope=nan), "riser_slope"), (dict(steps_lo=0), "steps_lo"), (dict(steps_hi=8), "steps_hi"), (dict(steps_lo=3, steps_hi=2), "steps_hi"),
        (dict(run_lo=nan), "run_lo"), (dict(run_hi=inf), "run_hi"), (dict(run_hi=1000.5), "run_hi"), (dict(run_lo=0.3, run_hi=0.29), "run_hi"),
        # the widest riser of [-0.06, 0.08] at slope 1.7 is 0.08 / 1.7 = 0.04706: a tread of 0.0479 leaves less than 1e-3 behind it
        (dict(run_lo=0.0479, run_hi=0.3), "run_lo"), (dict(height_lo=-0.5, height_hi=0.0), "run_lo"), (dict(run_lo=0.0019, run_hi=0.3, height_lo=0.0, height_hi=0.0), "run_lo"),
        (dict(mu_lo=-0.1), "mu_lo"), (dict(mu_lo=nan), "mu_lo"), (dict(mu_hi=inf), "mu_hi"), (dict(mu_lo=0.5, mu_hi=0.4), "mu_hi"),
        (dict(follow_map=2), "follow_map"), (dict(log_capacity=-1), "log_capacity"), (dict(log_capacity=abi.HB_PD_LOG_MAX + 1), "log_capacity"),
    ]
    for over, field in cases:
        why = lib.pd_config_refusal(C.byref(abi.make_profile_draw_config(**{**base, **over})))
        assert why is not None and why.decode().startswith(field), (over, why)
    for k in (0, 1):
        cfg = _cfg()
        cfg.reserved[k] = 1
        assert lib.pd_config_refusal(C.byref(cfg)).decode().startswith("`reserved`")
    # the edges themselves are admitted
    for over in (dict(riser_slope=1.7), dict(at_lo=-1000.0, at_hi=1000.0), dict(run_hi=1000.0), dict(steps_lo=1, steps_hi=7), dict(kinds=7),
                 dict(log_capacity=abi.HB_PD_LOG_MAX), dict(run_lo=0.0481, run_hi=0.3)):
        assert lib.pd_config_refusal(C.byref(abi.make_profile_draw_config(**{**base, **over}))) is None, over


# ---- placement ---------------------------------------------------------------------------------------------------------------------------------
def _standing(params):
    x0 = np.array(params["config"]["initial_state"], dtype=float)
    q = np.zeros(16)
    q[0:3], q[3:6], q[6:] = x0[6:9], x0[9:12], x0[12:]
    return q


def _foot_fn(lib, mdl):
    def foot_fn(q):
        q = np.ascontiguousarray(np.atleast_2d(q), dtype=float)
        out = np.zeros((q.shape[0], 12))
        for i in range(q.shape[0]):
            lib.pd_feet(C.byref(mdl), _p(q[i]), _p(out[i]))
        return out
    return foot_fn


def _place(lib, mdl, rcfg, pro, q):
    q, feet, seg, base = np.array(q, dtype=float), np.zeros(12), np.zeros(5, dtype=np.int32), np.zeros(14)
    lib.pd_place(C.byref(mdl), C.byref(rcfg), _p(pro), _p(q), _p(feet), _p(seg), _p(base))
    return q, feet.reshape(4, 3), seg, base


def _segment_records(lib, pro):
    return pro[14 + 2 + 1 + KMAX:].reshape(KMAX - 1, 10)


def _placed_gaps(lib, pro, feet, seg):
    """gap_c of the placed points over the facets of the STORED record, with the rounding bound of the comparison: a gap is a sum of four
    terms of magnitude at most M = |n_x x| + |n_y y| + |n_z z| + |d| (four roundings of at most M eps / 2 each, here and once more in the
    routine), the shift adds a quotient and a sum (two more), and re-evaluating the kinematics at q + D e_z moves a point's z by D up to
    the rounding of a chain that sums under ten terms of at most M: 32 eps max(M, 1) covers them."""
    recs = _segment_records(lib, pro)
    gaps, M = np.zeros(4), 1.0
    for c in range(4):
        r = recs[seg[c]]
        n, d = r[[2, 5, 8]], r[9]
        gaps[c] = n @ feet[c] - d
        M = max(M, float(np.abs(n * feet[c]).sum() + abs(d)))
    return gaps, 32.0 * EPS * M


def _ok(gaps, bound, clearance):
    return abs(gaps.min() - clearance) <= bound and (gaps >= clearance - bound).all()


def test_placement_on_a_level_profile_is_the_planes(lib, mdl, params):
    rcfg = abi.make_respawn_config(place=1, clearance=0.002)
    q = _standing(params)
    q[2] += 0.05
    q[3:6] = 0.2, 0.03, -0.04
    rel, kn, pro = np.zeros(2 * KMAX), np.zeros(2 * KMAX), np.zeros(lib.pd_profile_stored())
    lib.pd_flat(_p(np.array([3.0, 4.0])), _p(q[0:2].copy()), C.c_double(GROUND_Z), C.c_double(CFG_MU), _p(rel), _p(kn), _p(pro))
    qp, feet, seg, base = _place(lib, mdl, rcfg, pro, q)
    qq, ff = q.copy(), np.zeros(12)
    lib.pd_place_plane(C.byref(mdl), C.byref(rcfg), _p(np.array([0.0, 0.0, 1.0, GROUND_Z])), _p(qq), _p(ff))
    assert _same_bytes(qp, qq) and _same_bytes(feet, ff) and qp[2] != q[2]
    assert seg.tolist() == [0] * 5 and np.array_equal(base[:9], np.eye(3).reshape(9)) and base[9] == GROUND_Z and (base[10:] == CFG_MU).all()
    # place = 0: no shift, the locate alone
    q0, _, seg0, _ = _place(lib, mdl, abi.make_respawn_config(place=0, clearance=0.002), pro, q)
    assert _same_bytes(q0, q) and seg0.tolist() == [0] * 5


def test_placement_on_an_incline_and_on_a_straddled_curb(lib, mdl, params):
    """min_c gap_c == clearance to the bound of _placed_gaps and no point below it, on a one-segment incline and on a curb one foot
    straddles (the twin asserts the straddle first); the placed state == the twin's at the tolerance the respawn tests hold a placed state
    to (1e-10).  A mutant that measures all four points against the facet under the base origin fails the same check on the curb."""
    rcfg = abi.make_respawn_config(place=1, clearance=0.002)
    foot_fn = _foot_fn(lib, mdl)
    q = _standing(params)
    q[2] += 0.03
    q[3:6] = 0.1, 0.02, -0.03
    direction = np.array([0.8, 0.6])
    a = direction / np.sqrt(direction @ direction)
    s = foot_fn(q)[0].reshape(4, 3)[:, :2] @ a
    # the incline: one segment of slope 0.3 through ground_z under the base
    s_b = float(a @ q[0:2])
    incline = np.array([(s_b - 5.0, GROUND_Z - 1.5), (s_b + 5.0, GROUND_Z + 1.5)])
    # the curb: its riser between the two foremost contact points, so the foremost stands on top and its leg straddles
    order = np.argsort(s)
    h = 0.02
    w = h / np.sqrt(3.0)
    assert s[order[3]] - s[order[2]] > 2.0 * w, "the two foremost points are too close for a riser between them"
    curb = rollout.curb_profile(h, 0.5 * (s[order[3]] + s[order[2]]) - 0.5 * w)
    curb[:, 1] += GROUND_Z
    for name, knots in (("incline", incline), ("curb", curb)):
        pro, why = _profile_record(lib, len(knots), direction, pd.padded(knots), None)
        assert why is None
        if name == "curb":
            assert pd.straddles(a, knots, q, foot_fn) == [int(order[3]) % 2]
        qp, feet, seg, base = _place(lib, mdl, rcfg, pro, q)
        assert _same_bytes(qp[[0, 1, 3, 4, 5]], q[[0, 1, 3, 4, 5]]) and _same_bytes(qp[6:], q[6:]) and qp[2] != q[2]
        assert _same_bytes(feet, foot_fn(qp)[0].reshape(4, 3))                # re-evaluated at the placed state
        assert seg.tolist() == pd.locate(a, knots, qp, foot_fn).tolist() and seg.tolist() == pd.locate(a, knots, q, foot_fn).tolist()
        assert _same_bytes(base[:10], _segment_records(lib, pro)[seg[4]]) and (base[10:] == CFG_MU).all()
        assert _same_bytes(base, pd.base_record(a, knots, qp, _segment_records(lib, pro), [CFG_MU] * 4))
        gaps, bound = _placed_gaps(lib, pro, feet, seg)
        print(name, "gaps - clearance", gaps - rcfg.clearance, "bound", bound, "segments", seg.tolist())
        assert _ok(gaps, bound, rcfg.clearance), (name, gaps - rcfg.clearance, bound)
        qt = pd.place(rcfg, q, foot_fn, a, knots)
        assert np.abs(qp - qt).max() <= 1e-10
        if name == "curb":
            assert len(set(seg[:4].tolist())) > 1
            qm = pd.place(rcfg, q, foot_fn, a, knots, against_base=True)
            fm = foot_fn(qm)[0].reshape(4, 3)
            gm, bm = _placed_gaps(lib, pro, fm, pd.locate(a, knots, qm, foot_fn))
            assert not _ok(gm, bm, rcfg.clearance), "the mutant passes: the check does not see which facet a point is measured against"
