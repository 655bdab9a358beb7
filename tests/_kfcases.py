"""Sensor streams that take the state estimator to its edges, and the runs of each implementation over them, for
tests/test_estimator_twin_host.py and tests/test_gpu_estimator_twin.py.  One instance per row, seeded generators, the smallest that still reach
each edge:

  contacts      B 21 x 96: instances 0..15 hold each of the 16 contact patterns (0: all swing, P grows), 16..20 change pattern every 1, 2, 3, 5, 8
                ticks; wide sensors, roll to 1.2, pitch to 1.3, yaw falling 0.35 a tick
  yaw           B 8 x 64: descent through -pi, ascent through +pi, four revolutions each way, single-tick steps of +-(pi - 1e-3), starts at
                +-2.9 after a reset (yaw_last starts at 0)
  pitch         B 4 x 48: sweeps to 1.568 (the clamp is active above asin(0.99999) = 1.56632, 1 / cos ~ 224) and to -1.5
  dt_0001, dt_0005, dt_alternating   the contacts stream at other tick lengths (alternating: 0.001 / 0.004 from tick to tick)
  cond_*        the contacts stream under three noise settings that make S = C Pm C' + R ill-conditioned
  long          B 4 x 2000: the kind of stream tests/test_gpu_estimator.py runs, for drift
  reset         the yaw stream with estimator_reset issued again at tick 20 with a non-zero x_hat0

Every stream keeps -2 (x z - w y) >= -0.9999: the reference has no lower clamp, and NaN behaviour is not the subject."""
import ctypes as C

import numpy as np

import _kftwin as kt
from hunter_bipedal_control_amd import abi

EPS = kt.EPS
FACTOR = 8.0             # device bound = FACTOR x the oracle's worst distance from the twin on the same stream and quantity ...
FLOOR = 64.0 * EPS       # ... and no less than this, all relative to max(1, |value|)
DET_THRESHOLD = 1e-6
DET_BAND = 1e-6          # relative distance the twin's det(P[0:2, 0:2]) keeps from the threshold at every tick
QUANTITIES = ("zyx", "omega", "pos", "vel", "xhat", "P", "yaw")


def quat_from_zyx(zyx):
    """[..., 3] yaw, pitch, roll -> [..., 4] x y z w of Rz Ry Rx, from the half angles (no division, good at any angle)."""
    h = 0.5 * np.asarray(zyx, dtype=np.float64)
    cy, sy, cp, sp, cr, sr = np.cos(h[..., 0]), np.sin(h[..., 0]), np.cos(h[..., 1]), np.sin(h[..., 1]), np.cos(h[..., 2]), np.sin(h[..., 2])
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], axis=-1)


def _stream(name, dt, zyx, w, a, qj, qdj, contact, overrides=None, x_hat0=None, resets=None):
    T, B = zyx.shape[:2]
    quat = quat_from_zyx(zyx)
    assert (-2 * (quat[..., 0] * quat[..., 2] - quat[..., 3] * quat[..., 1])).min() >= -0.9999
    return dict(name=name, T=T, B=B, dt=np.broadcast_to(np.asarray(dt, dtype=np.float64), (T,)).copy(), quat=quat, zyx_in=zyx, w=w, a=a, qj=qj,
                qdj=qdj, contact=contact.astype(np.int32), overrides=dict(overrides or {}), x_hat0=x_hat0, resets=dict(resets or {}))


def _easy_sensors(rng, params, T, B):
    qj0 = np.array(params["config"]["default_joint_state"])
    return dict(w=0.5 * rng.standard_normal((T, B, 3)), a=np.array([0, 0, 9.81]) + 0.5 * rng.standard_normal((T, B, 3)),
                qj=qj0 + 0.1 * rng.standard_normal((T, B, 10)), qdj=rng.standard_normal((T, B, 10)),
                contact=(rng.uniform(size=(T, B, 4)) < 0.7))


def _contacts(params, name="contacts", dt=0.002, overrides=None, seed=101):
    rng = np.random.default_rng(seed)
    T, B = 96, 21
    k = np.arange(T)[:, None]
    ph = rng.uniform(0, 2 * np.pi, (2, B))
    zyx = np.stack([0.3 * np.arange(B)[None, :] - 0.35 * k, 1.3 * np.sin(0.07 * k + ph[0]), 1.2 * np.sin(0.05 * k + ph[1])], axis=-1)
    qj0 = np.array(params["config"]["default_joint_state"])
    pattern = np.zeros((T, B), dtype=np.int64)
    pattern[:, :16] = np.arange(16)
    for j, every in enumerate((1, 2, 3, 5, 8)):
        seq = rng.integers(0, 16, T)
        pattern[:, 16 + j] = seq[np.arange(T) // every]
    contact = (pattern[..., None] >> np.arange(4)) & 1
    return _stream(name, dt, zyx, 5.0 * rng.standard_normal((T, B, 3)), np.array([0, 0, 9.81]) + 10.0 * rng.standard_normal((T, B, 3)),
                   qj0 + rng.uniform(-0.5, 0.5, (T, B, 10)), 10.0 * rng.standard_normal((T, B, 10)), contact, overrides=overrides)


def _yaw(params, name="yaw", resets=None, seed=202):
    rng = np.random.default_rng(seed)
    T, B = 64, 8
    k = np.arange(T, dtype=np.float64)
    big = np.pi - 1e-3
    yaw = np.stack([-2.6 - 0.03 * k, 2.6 + 0.03 * k, 0.2 + 0.41 * k, -0.2 - 0.41 * k, 0.3 - 0.0002 * k + big * ((k + 3) // 8),
                    -0.3 + 0.0002 * k - big * ((k + 5) // 8), 2.9 + 0.001 * k, -2.9 - 0.002 * k], axis=1)
    # every step of the unwrap (from yaw_last = 0 at the start and after a reset) stays 1e-6 away from +-pi: no branch decided by rounding
    for t0 in [0] + sorted(resets or {}):
        steps = np.diff(np.concatenate([np.zeros((1, B)), yaw[t0:]]), axis=0)
        steps[0] = np.arctan2(np.sin(yaw[t0]), np.cos(yaw[t0]))     # the first tick sees the wrapped angle against yaw_last = 0
        d = np.mod(steps + np.pi, 2 * np.pi) - np.pi
        assert (np.pi - np.abs(d)).min() > 1e-6
    zyx = np.stack([yaw, 0.1 * rng.standard_normal((T, B)), 0.1 * rng.standard_normal((T, B))], axis=-1)
    s = _easy_sensors(rng, params, T, B)
    return _stream(name, 0.002, zyx, s["w"], s["a"], s["qj"], s["qdj"], s["contact"], resets=resets)


def _pitch(params, seed=303):
    rng = np.random.default_rng(seed)
    T, B = 48, 4
    k = np.arange(T, dtype=np.float64) / (T - 1)
    pitch = np.stack([1.2 + (1.568 - 1.2) * k, 1.568 * np.sin(np.pi * k), -1.5 * k, 1.55 + 0.018 * np.sin(7 * np.pi * k)], axis=1)
    zyx = np.stack([0.5 + 0.05 * rng.standard_normal((T, B)), pitch, 0.4 * rng.standard_normal((T, B))], axis=-1)
    s = _easy_sensors(rng, params, T, B)
    return _stream("pitch", 0.002, zyx, 2.0 * s["w"], s["a"], s["qj"], s["qdj"], s["contact"])


def _long(params, seed=404):
    rng = np.random.default_rng(seed)
    T, B = 2000, 4
    k = np.arange(T, dtype=np.float64)[:, None]
    zyx = np.stack([2.7 + 0.04 * k + 0.01 * np.arange(B), 0.1 * rng.standard_normal((T, B)), 0.1 * rng.standard_normal((T, B))], axis=-1)
    s = _easy_sensors(rng, params, T, B)
    return _stream("long", 0.002, zyx, s["w"], s["a"], s["qj"], s["qdj"], s["contact"])


def _reset_x0(seed=505):
    x0 = 0.3 * np.random.default_rng(seed).standard_normal((8, 18))
    x0[:, 2] += 0.6
    return x0


BUILDERS = {
    "contacts": lambda p: _contacts(p),
    "yaw": lambda p: _yaw(p),
    "pitch": lambda p: _pitch(p),
    "dt_0001": lambda p: _contacts(p, "dt_0001", dt=0.001),
    "dt_0005": lambda p: _contacts(p, "dt_0005", dt=0.005),
    "dt_alternating": lambda p: _contacts(p, "dt_alternating", dt=np.where(np.arange(96) % 2 == 0, 0.001, 0.004)),
    "cond_foot_noise": lambda p: _contacts(p, "cond_foot_noise", overrides=dict(foot_sensor_noise_position=1e-6, foot_sensor_noise_velocity=1e-6)),
    "cond_height_noise": lambda p: _contacts(p, "cond_height_noise", overrides=dict(foot_height_sensor_noise=1e-8)),
    "cond_process_noise": lambda p: _contacts(p, "cond_process_noise", overrides=dict(imu_process_noise_position=50.0, imu_process_noise_velocity=50.0,
                                                                                      foot_process_noise_position=1e-6)),
    "long": lambda p: _long(p),
    "reset": lambda p: _yaw(p, "reset", resets={20: _reset_x0()}),
}
NAMES = tuple(BUILDERS)
_STREAMS, _RUNS = {}, {}


def stream(params, name):
    if name not in _STREAMS:
        _STREAMS[name] = BUILDERS[name](params)
    return _STREAMS[name]


def config_of(params, s):
    return abi.make_estimator_config(params, **s["overrides"])


def sensors_at(s, k):
    return s["quat"][k], s["w"][k], s["a"][k], s["qj"][k], s["qdj"][k], s["contact"][k]


def collect(rows):
    return {key: np.stack([r[key] for r in rows]) for key in rows[0]}


def run_twin(params, oracle, s, height=None, x_hat0=None, **mutant):
    """The twin over a stream -> dict of [T][B][...] arrays: the keys of _kftwin.tick, pos = xhat[0:3], vel = xhat[3:6]."""
    cfg = config_of(params, s)
    st = kt.init(s["B"], s["x_hat0"] if x_hat0 is None else x_hat0)
    rows = []
    for k in range(s["T"]):
        if k in s["resets"]:
            st = kt.init(s["B"], s["resets"][k])
        rows.append(kt.tick(oracle, cfg, st, s["dt"][k], *sensors_at(s, k), height=height, **mutant))
    out = collect(rows)
    out["pos"], out["vel"] = out["xhat"][..., 0:3], out["xhat"][..., 3:6]
    return out


def pack_tick(rbd, x, xhat, P):
    """What an implementation in double returns per tick, under the twin's names (+ x, rbd: the whole outputs)."""
    return dict(zyx=rbd[:, 0:3].copy(), omega=rbd[:, 16:19].copy(), pos=rbd[:, 3:6].copy(), vel=rbd[:, 19:22].copy(), xhat=xhat.copy(), P=P.copy(),
                yaw=x[:, 9].copy(), x=x.copy(), rbd=rbd.copy(), shrink=np.all(P[:, 0, 2:] == 0.0, axis=1))


def run_oracle(params, oracle, s):
    cfg = config_of(params, s)
    rows = []

    def fresh(x0):
        st = oracle.kf_init(s["B"])
        if x0 is not None:
            st["xhat"][:] = x0
        return st
    st = fresh(s["x_hat0"])
    for k in range(s["T"]):
        if k in s["resets"]:
            st = fresh(s["resets"][k])
        rbd, x = oracle.kf_update(cfg, st, float(s["dt"][k]), *sensors_at(s, k))
        rows.append(pack_tick(rbd, x, st["xhat"], st["P"]))
    return collect(rows)


_EMU = {}


def _emu_lib():
    if "lib" not in _EMU:
        import _hostemu
        _EMU["lib"] = C.CDLL(str(_hostemu.build()))
    return _EMU["lib"]


def run_emu(params, s):
    """The device algorithm on the host emulator (hb_estimator.hpp, one emulated lane), instance by instance."""
    lib, mdl, cfg = _emu_lib(), abi.make_model(params), config_of(params, s)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    B = s["B"]

    def fresh(x0):
        return (np.zeros((B, 18)) if x0 is None else np.array(x0, dtype=np.float64).reshape(B, 18)), np.tile(100.0 * np.eye(18), (B, 1, 1)), np.zeros(B)
    xhat, P, yaw = fresh(s["x_hat0"])
    rows = []
    for k in range(s["T"]):
        if k in s["resets"]:
            xhat, P, yaw = fresh(s["resets"][k])
        sens = [np.ascontiguousarray(a) for a in sensors_at(s, k)]
        rbd, x = np.zeros((B, 32)), np.zeros((B, 22))
        for i in range(B):
            lib.emu_kf_update(C.byref(mdl), C.byref(cfg), C.c_double(float(s["dt"][k])), p(xhat[i]), p(P[i]), p(yaw[i:i + 1]),
                              *[p(a[i]) for a in sens], p(rbd[i]), p(x[i]))
        rows.append(pack_tick(rbd, x, xhat, P))
    return collect(rows)


def rel_err(got, want):
    """Worst over ticks and instances of max |got - want| / max(1, max |want|), the scale taken per instance and tick."""
    want = np.asarray(want)
    d = np.abs(np.asarray(got).astype(kt.LD) - want)
    ax = tuple(range(2, d.ndim))
    if ax:
        d, sc = d.max(axis=ax), np.abs(want).max(axis=ax)
    else:
        sc = np.abs(want)
    return float((d / np.maximum(1, sc)).max())


def errors(run, twin):
    return {q: rel_err(run[q], twin[q]) for q in QUANTITIES}


def bounds(levels):
    """The bound of every compared quantity from the oracle's levels on the same stream."""
    return {q: max(FACTOR * levels[q], FLOOR) for q in levels}


def momentum_ratio(oracle, run):
    """Worst of |x[0:6] - h| / (64 eps max(1, |h|)) over a run, h the oracle's normalised momentum at the run's own rbd."""
    T, B = run["rbd"].shape[:2]
    h = oracle.centroidal_state_from_rbd(np.ascontiguousarray(run["rbd"]).reshape(T * B, 32))[:, 0:6].reshape(T, B, 6)
    d = np.abs(run["x"][..., 0:6] - h).max(axis=2)
    return float((d / (FLOOR * np.maximum(1.0, np.abs(h).max(axis=2)))).max())


def runs(params, oracle, name):
    """(stream, twin run, oracle run, the oracle's levels) — computed once per process."""
    if name not in _RUNS:
        s = stream(params, name)
        twin = run_twin(params, oracle, s)
        orc = run_oracle(params, oracle, s)
        _RUNS[name] = (s, twin, orc, errors(orc, twin))
    return _RUNS[name]


def assert_matches_twin(run, twin, levels, label, quantities=QUANTITIES):
    """Every compared quantity of a run in double (pack_tick rows) within the bound, P exactly symmetric, the shrink decision of every instance
    and tick (read from whether P[0, 2:] is exactly zero after the tick) equal to the twin's.  Prints and returns the ratios to the levels."""
    err, bound = {q: rel_err(run[q], twin[q]) for q in quantities}, bounds(levels)
    print("\n%-19s" % label + "  ".join("%s %.1e (%.2f x level)" % (q, err[q], err[q] / max(levels[q], 1e-300)) for q in quantities))
    for q in quantities:
        assert err[q] <= bound[q], (label, q, err[q], bound[q])
    assert rel_err(run["x"][..., 6:9], twin["pos"]) <= bound["pos"], label
    if "zyx" in quantities:
        assert rel_err(run["x"][..., 10:12], twin["zyx"][..., 1:3]) <= bound["zyx"], label
    assert np.array_equal(run["P"], np.swapaxes(run["P"], -1, -2)), label
    assert np.array_equal(run["shrink"], twin["shrink"]), label
    return {q: err[q] / max(levels[q], 1e-300) for q in quantities}


# ---- the map forms: the cases of tests/_groundtwin.py (profile) and tests/_groundfieldtwin.py (field), ten ticks per map ---------------------
_MAPS = {}


def map_case(params, oracle, kind):
    """-> (stream, the maps of the cases, fresh twin maps the twin's run has evaluated, twin run on the maps, levels).  The oracle has no map
    form: the levels are its distance from the twin on the same sensors over level ground — the map changes four measured values of a tick,
    not one operation of it."""
    if kind not in _MAPS:
        import _groundtwin as gt
        if kind == "profile":
            inputs, maps, _, _ = gt.cases(params)
            fresh = [gt.GroundMap(m.dir_given, m.knots) for m in maps]
        else:
            import _groundfieldtwin as gft
            inputs, maps, _, _ = gft.cases(params)
            fresh = [gft.FieldMap(m.dir_given, m.origin, m.spacing, m.g) for m in maps]
        from oracle import refgen
        B, T = len(maps), 10
        x0 = np.stack([case["calls"][0][1] for case in inputs])
        xh0 = np.zeros((B, 18))
        xh0[:, 0:3] = x0[:, 6:9]
        xh0[:, 6:18] = np.stack([refgen.foot_positions(params["model"], xi) for xi in x0]).reshape(B, 12)
        xh0[:, 3] = 0.3
        rng = np.random.default_rng(41)
        e = _easy_sensors(rng, params, T, B)
        s = _stream("map_" + kind, 0.002, 0.2 * rng.standard_normal((T, B, 3)), e["w"], e["a"], e["qj"], e["qdj"], e["contact"], x_hat0=xh0)
        level = errors(run_oracle(params, oracle, s), run_twin(params, oracle, s))
        twin = run_twin(params, oracle, s, height=[m.G for m in fresh])
        _MAPS[kind] = (s, maps, fresh, twin, level)
    return _MAPS[kind]


def det_band(twin):
    """Smallest relative distance of the twin's det(P[0:2, 0:2]) from the shrink threshold over a run."""
    return float(np.abs(twin["det"] / kt.LD(DET_THRESHOLD) - 1).min())
