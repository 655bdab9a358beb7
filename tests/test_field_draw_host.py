"""CPU: the field-draw routines (csrc/hb_fielddraw.hpp, compiled for the host: what k_plant_field_draw runs per instance and what
k_plant_respawn_field runs on a height field) against the independent twin of the definition in include/hunter_hip.h
(tests/_fielddrawemu.py) and against the host setters' own records (field_record, ground_field_record).  The draw uses no transcendental
function, so everything up to the records is exact: the Philox words, the uniforms, the kind, the row, the header, every height, the log
row, and the records byte for byte.  The placement goes through the leg kinematics; its bound is derived where it is used."""
import ctypes as C

import numpy as np
import pytest

import _fielddrawemu as fd
from hunter_bipedal_control_amd import abi

_p = fd._p
EPS = 2.0 ** -52
CASES = ((0, 1), (3, 1), (3, 2), (0xFFFFFFFF, 77), (4103, 1000), (12, 5), (13, 5))   # the pairs of tests/test_profile_draw_host.py
Q_SPAWN = np.array([0.31, -0.17])
GROUND_Z, CFG_MU = 0.123, 0.31
NMAX = abi.HB_FIELD_MAX_NODES
NZ = NMAX * NMAX


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(str(fd.build()))
    lib.fd_config_refusal.restype = C.c_char_p
    lib.fd_stream.restype = C.c_uint
    return lib


@pytest.fixture(scope="module")
def mdl(params):
    return abi.make_model(params)


def _cfg(name="host_all", **over):
    return abi.make_field_draw_config(**{**fd.CONFIGS[name], **over})


def _grid(nu, nw, spacing=(0.11, 0.09)):
    """host_all on the grid (nu, nw), the spawn point at an uneven place inside it."""
    return dict(n_nodes=(nu, nw), centre=(0.37 * (nu - 1) * spacing[0], 0.61 * (nw - 1) * spacing[1]))


def _block(lib, cfg, inst, episode, block):
    u, words = np.full(4, np.nan), np.zeros(4, dtype=np.uint32)
    lib.fd_block(C.byref(cfg), C.c_uint32(inst), C.c_uint32(episode), block, _p(u), _p(words))
    return u, words


def _compose(lib, cfg, inst, episode, q_spawn=Q_SPAWN, ground_z=GROUND_Z):
    a, row = np.full(2, np.nan), np.full(abi.HB_FD_N, np.nan)
    z, gz = np.full(NZ, np.nan), np.full(NZ, np.nan)
    hdr, ghdr = np.full(lib.fd_field_stored(), np.nan), np.full(lib.fd_ground_size(), np.nan)
    lib.fd_compose(C.byref(cfg), C.c_uint32(inst), C.c_uint32(episode), _p(np.array(q_spawn, dtype=float)), C.c_double(ground_z), _p(a), _p(row),
                   _p(z), _p(gz), _p(hdr), _p(ghdr))
    return dict(a=a, row=row, z=z.reshape(NMAX, NMAX), gz=gz.reshape(NMAX, NMAX), hdr=hdr, ghdr=ghdr)


def _field_record(lib, n, direction, org, step, z, mu, cfg_mu=CFG_MU):
    rec, why = np.full(lib.fd_field_stored(), np.nan), C.create_string_buffer(128)
    rc = lib.fd_field_record(_p(np.array(n, dtype=np.int32)), _p(np.array(direction, dtype=float)), _p(np.array(org, dtype=float)),
                             _p(np.array(step, dtype=float)), _p(np.ascontiguousarray(z, dtype=float)),
                             None if mu is None else _p(np.array(mu, dtype=float)), C.c_double(cfg_mu), _p(rec), why)
    return (rec, None) if rc == 0 else (None, why.value.decode())


def _ground_field_record(lib, n, direction, org, step, z):
    rec, why = np.full(lib.fd_ground_size(), np.nan), C.create_string_buffer(128)
    rc = lib.fd_ground_field_record(_p(np.array(n, dtype=np.int32)), _p(np.array(direction, dtype=float)), _p(np.array(org, dtype=float)),
                                    _p(np.array(step, dtype=float)), _p(np.ascontiguousarray(z, dtype=float)), _p(rec), why)
    return (rec, None) if rc == 0 else (None, why.value.decode())


def _same_bytes(a, b):
    return np.asarray(a, dtype=float).tobytes() == np.asarray(b, dtype=float).tobytes()


def _kind_variants():
    return [{}] + [dict(kinds=k) for k in fd.KINDS]


# ---- exact parity ----------------------------------------------------------------------------------------------------------------------------
def test_struct_and_constants_are_the_headers(lib):
    assert lib.fd_n() == abi.HB_FD_N == 8 and lib.fd_log_w() == abi.HB_FD_LOG_W == 13 and lib.fd_log_max() == abi.HB_FD_LOG_MAX == 1024
    assert lib.fd_stream() == abi.HB_FD_STREAM and len({abi.HB_FD_STREAM, abi.HB_PD_STREAM, abi.HB_SC_STREAM, abi.HB_RS_STREAM}) == 4
    assert (abi.HB_FD_FLAT, abi.HB_FD_ROUGH, abi.HB_FD_TILT, abi.HB_FD_TILT_ROUGH) == (1, 2, 4, 8)
    assert lib.fd_head_blocks() == fd.HEAD_BLOCKS and lib.fd_node_blocks() == fd.NODE_BLOCKS == 256 and lib.fd_nz() == NZ
    assert lib.fd_config_size() == C.sizeof(abi.HbFieldDrawConfig)
    off = np.zeros(19, dtype=np.int32)
    lib.fd_config_offsets(_p(off))
    names = ["seed", "kinds", "mu_per_point", "dir", "n_nodes", "spacing", "centre", "calm", "amp_lo", "amp_hi", "slope_u_lo", "slope_u_hi",
             "slope_w_lo", "slope_w_hi", "mu_lo", "mu_hi", "follow_map", "log_capacity", "reserved"]
    assert [f[0] for f in abi.HbFieldDrawConfig._fields_] == names
    assert off.tolist() == [getattr(abi.HbFieldDrawConfig, n).offset for n in names]
    header = (fd.CSRC.parents[1] / "include" / "hunter_hip.h").read_text()
    assert f"#define HB_FD_STREAM 0x{abi.HB_FD_STREAM:X}u" in header
    assert "HB_FD_FLAT = 1, HB_FD_ROUGH = 2, HB_FD_TILT = 4, HB_FD_TILT_ROUGH = 8" in header
    assert [n for n, _, _ in abi.FIELD_DRAW_FIELDS] == ["KIND", "AMPLITUDE", "SLOPE_U", "SLOPE_W", "MUS"]
    assert abi.FIELD_DRAW_LOG_HEAD == ("EPISODE", "CAUSE", "TICKS", "PROGRESS", "TILT_MAX")


def test_words_uniforms_kind_row_header_and_heights_are_the_twins(lib):
    """Under all kinds and each alone, on every grid of the issue (the non-square ones show a pitch / count mix-up), for the
    (instance, episode) pairs of the profile test."""
    seen = set()
    for nu, nw in fd.GRIDS:
        for over in _kind_variants():
            cfg = _cfg(**_grid(nu, nw), **over)
            assert lib.fd_config_refusal(C.byref(cfg)) is None
            for inst, episode in CASES:
                if (nu, nw) == (5, 7) and not over:                           # every block's words and uniforms, once per pair
                    for b in range(fd.HEAD_BLOCKS + fd.NODE_BLOCKS):
                        u, words = _block(lib, cfg, inst, episode, b)
                        want = fd.block_words(cfg, inst, episode, b)
                        assert words.tolist() == want, (inst, episode, b)
                        assert u.tolist() == [fd.uniform(w) for w in want] and (0.0 < u).all() and (u < 1.0).all()
                got = _compose(lib, cfg, inst, episode)
                tw = fd.draw(cfg, inst, episode, Q_SPAWN, GROUND_Z)
                assert got["row"][0] == tw["kind"] and tw["kind"] in fd.kinds_of(cfg)
                assert _same_bytes(got["a"], tw["a"]) and _same_bytes(got["row"], tw["row"]), (got["row"], tw["row"])
                assert _same_bytes(got["hdr"][lib.fd_field_dir():lib.fd_field_dir() + 8], tw["header"]), (nu, nw, inst, episode)
                assert _same_bytes(got["ghdr"], tw["header"])
                assert _same_bytes(got["z"], tw["heights"]), (nu, nw, over, inst, episode)
                assert _same_bytes(got["gz"], tw["map"])
                assert not got["z"][nu:].any() and not got["z"][:, nw:].any() and not got["gz"][nu:].any() and not got["gz"][:, nw:].any()
                assert not np.signbit(got["z"][got["z"] == 0.0]).any() and not np.signbit(got["gz"][got["gz"] == 0.0]).any()   # no negative zero
                seen.add(tw["kind"])
                r = abi.split_field_draw(got["row"])
                assert (cfg.mu_lo <= r["MUS"]).all() and (r["MUS"] <= cfg.mu_hi).all() and len(set(r["MUS"].tolist())) == 4
                rough, tilt = tw["kind"] in (abi.HB_FD_ROUGH, abi.HB_FD_TILT_ROUGH), tw["kind"] in (abi.HB_FD_TILT, abi.HB_FD_TILT_ROUGH)
                assert (cfg.amp_lo <= r["AMPLITUDE"] <= cfg.amp_hi) if rough else r["AMPLITUDE"] == 0.0
                assert (cfg.slope_u_lo <= r["SLOPE_U"] <= cfg.slope_u_hi and r["SLOPE_U"] != 0.0) if tilt else r["SLOPE_U"] == 0.0
                assert (cfg.slope_w_lo <= r["SLOPE_W"] <= cfg.slope_w_hi and r["SLOPE_W"] != 0.0) if tilt else r["SLOPE_W"] == 0.0
    assert seen == set(fd.KINDS)
    # another episode: another draw;  the other streams keep their bits
    cfg = _cfg()
    assert _block(lib, cfg, 3, 1, 0)[1].tolist() != _block(lib, cfg, 3, 2, 0)[1].tolist()
    import _profiledrawemu as pd
    import _respawnemu as rs
    import _scenarioemu as sc
    assert fd.block_words(cfg, 3, 1, 0) != rs.block_words(abi.make_respawn_config(seed=cfg.seed), 3, 1, 0)
    assert fd.block_words(cfg, 3, 1, 0) != sc.block_words(abi.make_scenario_config(seed=cfg.seed), 3, 1, 0)
    assert fd.block_words(cfg, 3, 1, 0) != pd.block_words(abi.make_profile_draw_config(seed=cfg.seed), 3, 1, 0)


def test_log_row_is_the_twins(lib):
    cfg = _cfg()
    a = np.array(fd.direction(cfg))
    irec, drec = np.zeros((1, abi.HB_EP_NI), dtype=np.int32), np.zeros((1, abi.HB_EP_ND))
    rng = np.random.default_rng(5)
    drec[0] = rng.normal(size=abi.HB_EP_ND)
    irec[0] = rng.integers(0, 50, size=abi.HB_EP_NI)
    rec = {k: v[0] for k, v in abi.split_episode_record(irec, drec).items()}
    itot = np.zeros(abi.HB_RS_NI, dtype=np.int32)
    itot[abi.RESPAWN_INT_FIELDS.index("EPISODE_INDEX")] = 6
    row = fd.draw(cfg, 3, 6, Q_SPAWN, GROUND_Z)["row"]
    count, log = np.zeros(1, dtype=np.int32), np.zeros((cfg.log_capacity, abi.HB_FD_LOG_W))
    for n in range(cfg.log_capacity + 2):                                      # (full: later episodes are not logged)
        lib.fd_log_append(cfg.log_capacity, abi.HB_RS_TIMEOUT, _p(a), _p(irec), _p(drec), _p(itot), _p(row), _p(count), _p(log))
        assert count[0] == min(n + 1, cfg.log_capacity)
    want = fd.log_row(6, abi.HB_RS_TIMEOUT, rec, row, a)
    assert all(_same_bytes(log[k], want) for k in range(cfg.log_capacity))


# ---- record parity -----------------------------------------------------------------------------------------------------------------------------
def test_records_are_the_host_setters_byte_for_byte(lib):
    """The stored record the draw composes == what hb_plant_set_terrain_field's routine stores for the twin's counts, the direction as
    given, the twin's origin, spacing, heights and mu — header, the head facet under the world origin, friction — and the map header ==
    what hb_ground_set_field's routine stores for the relative heights.  Both sides end in field_compose / ground_field_compose (one
    routine), so what this proves is that the draw hands the composers the twin's inputs and that validation accepts them; the facet
    arithmetic itself is pinned by tests/test_field_plant_host.py against its numpy definition."""
    variants = [("host_all", {**_grid(nu, nw), **over}) for nu, nw in ((5, 7), (3, 32)) for over in _kind_variants()]
    for name, over in variants + [("gpu_small", {}), ("gpu_full", {}), ("host_steep", {}), ("host_coarse", {})]:
        cfg = _cfg(name, **over)
        for inst, episode in CASES:
            got = _compose(lib, cfg, inst, episode)
            tw = fd.draw(cfg, inst, episode, Q_SPAWN, GROUND_Z)
            rec, why = _field_record(lib, tw["n"], cfg.dir, tw["origin"], cfg.spacing, tw["heights"], tw["mu"])
            assert why is None and _same_bytes(got["hdr"], rec), (name, over, inst, episode, why)
            grec, why = _ground_field_record(lib, tw["n"], cfg.dir, tw["origin"], cfg.spacing, tw["map"])
            assert why is None and _same_bytes(got["ghdr"], grec), (name, over, inst, episode, why)


def test_flat_is_the_level_record(lib):
    """FLAT with mu_lo = mu_hi = cfg.mu: the record of the level field at ground_z with the contact model's mu, and so is the ground the
    set call starts every instance on; the map is the zero map."""
    cfg = _cfg(kinds=abi.HB_FD_FLAT, mu_lo=CFG_MU, mu_hi=CFG_MU)
    hts, header = fd.flat(cfg, Q_SPAWN, GROUND_Z)
    nu, nw = int(cfg.n_nodes[0]), int(cfg.n_nodes[1])
    assert (hts[:nu, :nw] == GROUND_Z).all() and not hts[nu:].any() and not hts[:, nw:].any()
    level, why = _field_record(lib, (nu, nw), cfg.dir, header[2:4], cfg.spacing, hts, None)
    assert why is None
    for inst, episode in CASES:
        got = _compose(lib, cfg, inst, episode)
        assert _same_bytes(got["hdr"], level) and _same_bytes(got["z"], hts) and not got["gz"].any()
        assert not got["row"][1:4].any() and (got["row"][4:] == CFG_MU).all()
    z, gz = np.full(NZ, np.nan), np.full(NZ, np.nan)
    hdr, ghdr = np.full(lib.fd_field_stored(), np.nan), np.full(lib.fd_ground_size(), np.nan)
    lib.fd_flat(C.byref(cfg), _p(Q_SPAWN), C.c_double(GROUND_Z), C.c_double(CFG_MU), _p(z), _p(gz), _p(hdr), _p(ghdr))
    assert _same_bytes(hdr, level) and _same_bytes(z.reshape(NMAX, NMAX), hts) and not gz.any() and _same_bytes(ghdr, header)
    # T = I and d = ground_z in the head: the step without a terrain, value for value
    assert np.array_equal(level[:9], np.eye(3).reshape(9)) and level[9] == GROUND_Z and (level[10:14] == CFG_MU).all()


def test_a_nodes_bump_is_independent_of_the_grid_and_of_the_other_channels(lib):
    """The uniform of node (iu, iw) comes from the pitch numbering: the same on every grid that holds the node.  With calm = 0 and no
    tilt the height of a ROUGH node is A (2 u - 1), whatever (nu, nw), the slopes' ranges, the friction or the kinds beside it."""
    base = dict(kinds=abi.HB_FD_ROUGH, calm=0.0, amp_lo=0.0125, amp_hi=0.0125)
    for inst, episode in CASES:
        ref = _compose(lib, _cfg(**_grid(32, 32), **base), inst, episode)
        un = fd.node_uniforms(_cfg(), inst, episode)
        assert _same_bytes(ref["gz"], 0.0 + 0.0125 * (2.0 * un - 1.0))
        for nu, nw in fd.GRIDS:
            got = _compose(lib, _cfg(**_grid(nu, nw), **base), inst, episode)
            assert _same_bytes(got["gz"][:nu, :nw], ref["gz"][:nu, :nw]), (nu, nw)
            other = _compose(lib, _cfg(**_grid(nu, nw), **{**base, "slope_u_lo": -0.3, "slope_u_hi": -0.1, "mu_per_point": 0, "mu_hi": 1.5}), inst, episode)
            assert _same_bytes(other["gz"], got["gz"]) and _same_bytes(other["row"][:4], got["row"][:4])
        # a kind taken out or added: amplitude, slopes and friction are drawn as before, only the pick changes
        full = _compose(lib, _cfg(), inst, episode)
        alone = _compose(lib, _cfg(kinds=int(full["row"][0])), inst, episode)
        assert _same_bytes(alone["row"], full["row"]) and _same_bytes(alone["z"], full["z"]) and _same_bytes(alone["hdr"], full["hdr"])
        one = _compose(lib, _cfg(mu_per_point=0), inst, episode)
        assert _same_bytes(one["row"][:4], full["row"][:4]) and (one["row"][4:] == full["row"][4]).all() and _same_bytes(one["z"], full["z"])


def test_calm_zeroes_exactly_the_nodes_the_rule_names(lib):
    """ROUGH on the 7 x 5 grid: the nodes with |un - cu| <= calm and |wn - cw| <= calm have g = 0, every other node its bump (nonzero:
    2 u - 1 = 0 needs a word no block of these cases holds).  calm = the exact distance of a node is inclusive."""
    spacing = (0.11, 0.09)
    for calm in (0.0, 0.05, 0.12, 0.25, 10.0):
        cfg = _cfg(kinds=abi.HB_FD_ROUGH, **_grid(7, 5), calm=calm)
        named = np.zeros((7, 5), dtype=bool)
        for iu in range(7):
            for iw in range(5):
                named[iu, iw] = abs(float(iu) * spacing[0] - cfg.centre[0]) <= calm and abs(float(iw) * spacing[1] - cfg.centre[1]) <= calm
        for inst, episode in CASES:
            g = _compose(lib, cfg, inst, episode)["gz"][:7, :5]
            assert ((g == 0.0) == named).all(), (calm, inst, episode)
        assert named.sum() == {0.0: 0, 10.0: 35}.get(calm, named.sum()) and (calm in (0.0, 10.0) or 0 < named.sum() < 35)
    on_node = float(3) * spacing[0] - cfg.centre[0]                            # the exact distance of node row 3 from the centre
    cfg = _cfg(kinds=abi.HB_FD_ROUGH, **_grid(7, 5), calm=abs(on_node))
    g = _compose(lib, cfg, 3, 1)["gz"][:7, :5]
    assert (g[3] == 0.0).any()


# ---- validity ------------------------------------------------------------------------------------------------------------------------------------
def _sweep(lib, cfg, pairs, spawns):
    """-> (fields drawn, refusals as (instance, episode, spawn, why)) over pairs x spawns, the field record's own check on every draw."""
    bad, n = [], 0
    a = np.array(fd.direction(cfg))
    b = np.array([-a[1], a[0]])
    for su, sw in spawns:
        q_spawn = su * a + sw * b                                              # (a . q_s, b . q_s) = (su, sw) to rounding
        for inst, episode in pairs:
            got = _compose(lib, cfg, inst, episode, q_spawn, GROUND_Z_SWEEP)
            d = lib.fd_field_dir()
            rec, why = _field_record(lib, cfg.n_nodes[:], cfg.dir, got["hdr"][d + 2:d + 4], cfg.spacing, got["z"], got["row"][4:8])
            n += 1
            if why is None:
                why = _ground_field_record(lib, cfg.n_nodes[:], cfg.dir, got["hdr"][d + 2:d + 4], cfg.spacing, got["gz"])[1]
            if why is not None:
                bad.append((inst, episode, (su, sw), why))
    return n, bad


GROUND_Z_SWEEP = -1000.0                                                       # the far end of the admitted |ground_z|


def test_every_admitted_draw_is_a_valid_field(lib):
    """A condition, not a measurement: over 21 000 draws — the configurations of this file and of tests/test_gpu_field_draw.py and the
    edges of the admitted set (finest and coarsest spacing with slope and amplitude at the bound, |ground_z| = 1e3), spawn points with
    (a . q_s, b . q_s) in {0, (+-1000, -+1000)} — every drawn field passes field_record and its map ground_field_record.  One step outside the
    admitted set (the bound's left side at 3.3 > 3) the set call refuses the configuration and the same sweep, run on it regardless,
    finds fields the record refuses."""
    spawns = ((0.0, 0.0), (1000.0, -1000.0), (-1000.0, 1000.0))
    pairs = [(i, e) for i in (0, 1, 2, 77, 4103, 0xFFFFFFFF, 65536) for e in range(1, 144)]
    total = 0
    for name in fd.CONFIGS:
        cfg = _cfg(name)
        assert lib.fd_config_refusal(C.byref(cfg)) is None, name
        n, bad = _sweep(lib, cfg, pairs, spawns)
        assert not bad, (name, bad[:3])
        total += n
    assert total >= 20000
    # (1.0 + 2 * 1.4e-4 / 1e-3)^2 * 2 = 3.28: past the bound, and past the field's limit in the triangles whose shared node is bumped up
    # and whose other two down (the tilt climbs along u and falls along w, so one node can steepen both edges of a lower triangle)
    steep = _cfg("host_fine", amp_hi=1.4e-4, amp_lo=1.4e-4, slope_u_lo=1.0, slope_w_hi=-1.0, kinds=abi.HB_FD_TILT_ROUGH)
    assert b"slope and amplitude" in lib.fd_config_refusal(C.byref(steep))
    n, bad = _sweep(lib, steep, pairs[:20], spawns[:1])
    assert bad and all("steeper" in why for _, _, _, why in bad)


def test_the_bound_is_tight_where_it_says(lib):
    """At the bound itself the configuration is admitted; a hair past it, refused — for slope alone, amplitude alone and both."""
    ok = [dict(slope_u_lo=-1.2, slope_u_hi=1.2, slope_w_lo=-1.2, slope_w_hi=1.2, amp_lo=0.0, amp_hi=0.0),           # 2.88
          dict(slope_u_lo=0.0, slope_u_hi=0.0, slope_w_lo=0.0, slope_w_hi=0.0, amp_lo=0.0, amp_hi=0.6e-3),          # 1.2^2 * 2
          dict(slope_u_lo=-1.7, slope_u_hi=0.0, slope_w_lo=0.0, slope_w_hi=0.0, amp_lo=0.0, amp_hi=0.0)]            # 2.89
    bad = [dict(slope_u_lo=-1.21, slope_u_hi=1.2, slope_w_lo=-1.2, slope_w_hi=1.2, amp_lo=0.0, amp_hi=0.0),
           dict(slope_u_lo=0.0, slope_u_hi=0.0, slope_w_lo=0.0, slope_w_hi=0.0, amp_lo=0.0, amp_hi=0.61e-3),
           dict(slope_u_lo=-1.71, slope_u_hi=0.0, slope_w_lo=0.0, slope_w_hi=0.0, amp_lo=0.0, amp_hi=0.0)]
    for over in ok:
        assert lib.fd_config_refusal(C.byref(_cfg("host_fine", **over))) is None, over
    for over in bad:
        assert lib.fd_config_refusal(C.byref(_cfg("host_fine", **over))).decode().startswith("slope and amplitude"), over


def test_every_refusal_names_its_field(lib):
    base = fd.CONFIGS["host_all"]
    assert lib.fd_config_refusal(C.byref(_cfg())) is None
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(kinds=0), "kinds"), (dict(kinds=16), "kinds"), (dict(kinds=-1), "kinds"), (dict(mu_per_point=2), "mu_per_point"),
        (dict(mu_per_point=-1), "mu_per_point"), (dict(dir=(0.0, 0.0)), "dir"), (dict(dir=(nan, 1.0)), "dir"), (dict(dir=(1.0, inf)), "dir"),
        (dict(n_nodes=(1, 7)), "n_nodes"), (dict(n_nodes=(5, 33)), "n_nodes"), (dict(n_nodes=(0, 0)), "n_nodes"),
        (dict(spacing=(0.9e-3, 0.09)), "spacing"), (dict(spacing=(0.11, 10.5)), "spacing"), (dict(spacing=(nan, 0.09)), "spacing"),
        (dict(spacing=(0.11, -0.09)), "spacing"), (dict(spacing=(inf, 0.09)), "spacing"),
        (dict(centre=(-0.01, 0.25)), "centre"), (dict(centre=(0.2, 0.55)), "centre"), (dict(centre=(nan, 0.25)), "centre"), (dict(centre=(0.45, 0.25)), "centre"),
        (dict(calm=-0.1), "calm"), (dict(calm=nan), "calm"), (dict(calm=inf), "calm"),
        (dict(amp_lo=-0.001), "amp_lo"), (dict(amp_lo=nan), "amp_lo"), (dict(amp_hi=inf), "amp_hi"), (dict(amp_lo=0.02, amp_hi=0.01), "amp_hi"),
        (dict(slope_u_lo=nan), "slope_u_lo"), (dict(slope_u_hi=inf), "slope_u_hi"), (dict(slope_u_lo=0.3, slope_u_hi=0.2), "slope_u_hi"),
        (dict(slope_w_lo=-inf), "slope_w_lo"), (dict(slope_w_hi=nan), "slope_w_hi"), (dict(slope_w_lo=0.2, slope_w_hi=0.1), "slope_w_hi"),
        (dict(slope_u_lo=-1.8), "slope and amplitude"), (dict(amp_hi=0.1), "slope and amplitude"), (dict(slope_w_hi=1.7), "slope and amplitude"),
        (dict(mu_lo=-0.1), "mu_lo"), (dict(mu_lo=nan), "mu_lo"), (dict(mu_hi=inf), "mu_hi"), (dict(mu_lo=0.5, mu_hi=0.4), "mu_hi"),
        (dict(follow_map=2), "follow_map"), (dict(follow_map=-1), "follow_map"), (dict(log_capacity=-1), "log_capacity"),
        (dict(log_capacity=abi.HB_FD_LOG_MAX + 1), "log_capacity"),
    ]
    for over, field in cases:
        why = lib.fd_config_refusal(C.byref(abi.make_field_draw_config(**{**base, **over})))
        assert why is not None and why.decode().startswith(field), (over, why)
    for k in (0, 1):
        cfg = _cfg()
        cfg.reserved[k] = 1
        assert lib.fd_config_refusal(C.byref(cfg)).decode().startswith("`reserved`")
    # the edges themselves are admitted
    for over in (dict(spacing=(1e-3, 10.0), centre=(0.0, 0.0), amp_lo=0.0, amp_hi=0.0), dict(n_nodes=(2, 32), centre=(0.11, 0.25)), dict(kinds=15),
                 dict(centre=(0.0, 0.0)), dict(centre=(4 * 0.11, 6 * 0.09)), dict(calm=0.0), dict(log_capacity=abi.HB_FD_LOG_MAX), dict(amp_lo=0.0)):
        assert lib.fd_config_refusal(C.byref(abi.make_field_draw_config(**{**base, **over}))) is None, over


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
            lib.fd_feet(C.byref(mdl), _p(q[i]), _p(out[i]))
        return out
    return foot_fn


def _place(lib, mdl, rcfg, hdr, z, q):
    q, feet, sel, base = np.array(q, dtype=float), np.zeros(12), np.zeros(5, dtype=np.int32), np.zeros(14)
    lib.fd_place(C.byref(mdl), C.byref(rcfg), _p(hdr), _p(np.ascontiguousarray(z)), _p(q), _p(feet), _p(sel), _p(base))
    return q, feet.reshape(4, 3), sel, base


def _facet_record(lib, hdr, z, x):
    rec = np.zeros(10)
    return lib.fd_facet(_p(hdr), _p(np.ascontiguousarray(z)), _p(np.array(x, dtype=float)), _p(rec)), rec


def _placed_gaps(lib, hdr, z, feet):
    """gap_c of the placed points over the facets of the STORED field (the routine's own facet records), with the rounding bound of the
    comparison, derived as tests/test_profile_draw_host.py derives its own: a gap is a sum of four terms of magnitude at most
    M = |n_x x| + |n_y y| + |n_z z| + |d| (four roundings of at most M eps / 2 each, here and once more in the routine), the shift adds a
    quotient and a sum (two more), and re-evaluating the kinematics at q + D e_z moves a point's z by D up to the rounding of a chain that
    sums under ten terms of at most M: 32 eps max(M, 1) covers them."""
    gaps, M, ids = np.zeros(4), 1.0, []
    for c in range(4):
        fid, r = _facet_record(lib, hdr, z, feet[c])
        n, d = r[[2, 5, 8]], r[9]
        gaps[c] = n @ feet[c] - d
        M = max(M, float(np.abs(n * feet[c]).sum() + abs(d)))
        ids.append(fid)
    return gaps, 32.0 * EPS * M, ids


def _ok(gaps, bound, clearance):
    return abs(gaps.min() - clearance) <= bound and (gaps >= clearance - bound).all()


def test_placement_on_a_level_field_is_the_planes(lib, mdl, params):
    rcfg = abi.make_respawn_config(place=1, clearance=0.002)
    q = _standing(params)
    q[2] += 0.05
    q[3:6] = 0.2, 0.03, -0.04
    cfg = _cfg("gpu_small")
    z, gz = np.zeros(NZ), np.zeros(NZ)
    hdr, ghdr = np.zeros(lib.fd_field_stored()), np.zeros(lib.fd_ground_size())
    lib.fd_flat(C.byref(cfg), _p(q[0:2].copy()), C.c_double(GROUND_Z), C.c_double(CFG_MU), _p(z), _p(gz), _p(hdr), _p(ghdr))
    qp, feet, sel, base = _place(lib, mdl, rcfg, hdr, z, q)
    qq, ff = q.copy(), np.zeros(12)
    lib.fd_place_plane(C.byref(mdl), C.byref(rcfg), _p(np.array([0.0, 0.0, 1.0, GROUND_Z])), _p(qq), _p(ff))
    assert _same_bytes(qp, qq) and _same_bytes(feet, ff) and qp[2] != q[2]
    assert np.array_equal(base[:9], np.eye(3).reshape(9)) and base[9] == GROUND_Z and (base[10:] == CFG_MU).all()
    hts, _ = fd.flat(cfg, q[0:2], GROUND_Z)
    fld = dict(dir=fd.direction(cfg), origin=fd.origin(cfg, q[0:2]), spacing=cfg.spacing[:], heights=hts[:5, :7])
    foot_fn = _foot_fn(lib, mdl)
    assert fd.margin(fld, qp, foot_fn) >= fd.MARGIN
    assert sel.tolist() == fd.locate(fld, qp, foot_fn).tolist()
    # place = 0: no shift, the locate alone
    q0, _, sel0, _ = _place(lib, mdl, abi.make_respawn_config(place=0, clearance=0.002), hdr, z, q)
    assert _same_bytes(q0, q) and sel0.tolist() == sel.tolist()


PLACE_CASES = (("tilt", "gpu_small", dict(kinds=abi.HB_FD_TILT, slope_u_lo=0.25, slope_u_hi=0.3, slope_w_lo=-0.2, slope_w_hi=-0.15), 5, 2),
               ("rough", "gpu_full", dict(kinds=abi.HB_FD_ROUGH, calm=0.0, amp_lo=0.02, amp_hi=0.02), 3, 1))


def test_placement_on_a_tilt_and_on_a_rough_field(lib, mdl, params):
    """min_c gap_c == clearance to the bound of _placed_gaps and no point below it, on a drawn tilt and on a drawn rough field whose
    bumps reach under the feet (calm = 0; the twin asserts first that every point keeps MARGIN from node lines and diagonals and, on the
    rough field, that the four points stand on more than one facet plane); the placed state == the twin's at the tolerance the respawn
    tests hold a placed state to (1e-10), facet ids and the base record's plane included.  A mutant that measures all four points against
    the facet under the base origin fails the same check on the rough field."""
    rcfg = abi.make_respawn_config(place=1, clearance=0.002)
    foot_fn = _foot_fn(lib, mdl)
    q = _standing(params)
    q[0:2] = 0.31, -0.17
    q[2] += 0.03
    q[3:6] = 0.1, 0.02, -0.03
    for name, conf, over, inst, episode in PLACE_CASES:
        cfg = _cfg(conf, **over)
        assert lib.fd_config_refusal(C.byref(cfg)) is None
        got = _compose(lib, cfg, inst, episode, q[0:2], GROUND_Z)
        tw = fd.draw(cfg, inst, episode, q[0:2], GROUND_Z)
        assert _same_bytes(got["z"], tw["heights"]) and _same_bytes(got["hdr"][lib.fd_field_dir():lib.fd_field_dir() + 8], tw["header"])
        fld = fd.field_of(tw)
        qt = fd.place(rcfg, q, foot_fn, fld)
        assert fd.margin(fld, q, foot_fn) >= fd.MARGIN and fd.margin(fld, qt, foot_fn) >= fd.MARGIN, name    # on the twin alone, first
        qp, feet, sel, base = _place(lib, mdl, rcfg, got["hdr"], got["z"], q)
        assert _same_bytes(qp[[0, 1, 3, 4, 5]], q[[0, 1, 3, 4, 5]]) and _same_bytes(qp[6:], q[6:]) and qp[2] != q[2]
        assert _same_bytes(feet, foot_fn(qp)[0].reshape(4, 3))                # re-evaluated at the placed state
        assert sel.tolist() == fd.locate(fld, qp, foot_fn).tolist() and sel.tolist() == fd.locate(fld, q, foot_fn).tolist()
        fid, rec = _facet_record(lib, got["hdr"], got["z"], qp[0:3])
        assert fid == sel[4] and _same_bytes(base[:10], rec) and _same_bytes(base[10:], tw["mu"])
        pl = fd.base_plane(fld, qp)
        assert np.abs(base[[2, 5, 8]] - pl[:3]).max() <= 1e-12 and abs(base[9] - pl[3]) <= 1e-12
        gaps, bound, ids = _placed_gaps(lib, got["hdr"], got["z"], feet)
        print(name, "gaps - clearance", gaps - rcfg.clearance, "bound", bound, "facets", sel.tolist())
        assert ids == sel[:4].tolist()
        assert _ok(gaps, bound, rcfg.clearance), (name, gaps - rcfg.clearance, bound)
        assert np.abs(qp - qt).max() <= 1e-10
        if name == "rough":
            assert len(set(sel.tolist())) > 1
            qm = fd.place(rcfg, q, foot_fn, fld, against_base=True)
            gm, bm, _ = _placed_gaps(lib, got["hdr"], got["z"], foot_fn(qm)[0].reshape(4, 3))
            assert not _ok(gm, bm, rcfg.clearance), "the mutant passes: the check does not see which facet a point is measured against"
