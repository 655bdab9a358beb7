"""Extended-precision twin of one estimator tick (oracle/estimator.hpp kf_update) for tests/test_estimator_twin_host.py and
tests/test_gpu_estimator_twin.py: the filter in np.longdouble, dense, batched over instances, nothing exploited.

  * quatToZyx with its one-sided clamp, the local-rates / world-omega / rates chain, R a - g;
  * the dense A, B, C, Q, R of KalmanFilterEstimate::update, A P A' + Q, S = C Pm C' + R solved by Gaussian elimination with row pivoting
    (written here: np.linalg does not take longdouble), (I - K C) Pm, the symmetrisation, the shrink branch;
  * the yaw unwrap with the fmod formula.

The float literals are np.float32(20) and np.float32(9.81) widened, as in the reference.  The foot positions and velocities come from the oracle
in double (oracle.rbd_full: exact Jacobian velocities, no finite difference); the leg kinematics have their own tests and their 1e-16 is below
what is measured against this module.  The foot-height measurement is a callable height(x, y) at the predicted foot x, y rounded to double
(default 0), so the two map forms reuse the module.

MUTANTS: the keyword flags of tick(), one wrong thing each; tests/test_estimator_twin_host.py requires every one of them to be seen."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
PI = LD(3.14159265358979323846)          # the double literal of the reference, widened
F20 = LD(np.float32(20))
F981 = LD(np.float32(9.81))

MUTANTS = ("g981_double", "q_pos_with_velocity_literal", "no_suspicion_velocity", "no_suspicion_height", "no_suspicion_q", "no_pitch_clamp",
           "no_wrap", "shrink_threshold_1e5", "keep_cross_block", "b_dt2", "radius_on_x")


def _c_matrix():
    c = np.zeros((28, 18), dtype=LD)
    for f in range(4):
        for k in range(3):
            c[3 * f + k, k] = 1
            c[3 * f + k, 6 + 3 * f + k] = -1
            c[12 + 3 * f + k, 3 + k] = 1
        c[24 + f, 8 + 3 * f] = 1
    return c


C = _c_matrix()


def init(n, x_hat0=None):
    """-> dict(xhat[n][18], P[n][18][18] = 100 I, yaw_last[n]) in longdouble (kf_init; estimator_reset with x_hat0)."""
    xh = np.zeros((n, 18), dtype=LD) if x_hat0 is None else np.asarray(x_hat0, dtype=np.float64).astype(LD).reshape(n, 18).copy()
    return dict(xhat=xh, P=np.tile(LD(100) * np.eye(18, dtype=LD), (n, 1, 1)), yaw_last=np.zeros(n, dtype=LD))


def quat_to_zyx(quat, clamp=True):
    x, y, z, w = (quat[:, i] for i in range(4))
    s = -2 * (x * z - w * y)
    if clamp:
        s = np.minimum(s, LD(0.99999))
    return np.stack([np.arctan2(2 * (x * y + w * z), w * w + x * x - y * y - z * z), np.arcsin(s),
                     np.arctan2(2 * (y * z + w * x), w * w - x * x - y * y + z * z)], axis=1)


def rates_from_local_omega(zyx, w):
    sy, cy, sx, cx = np.sin(zyx[:, 1]), np.cos(zyx[:, 1]), np.sin(zyx[:, 2]), np.cos(zyx[:, 2])
    tmp = sx * w[:, 1] / cy + cx * w[:, 2] / cy
    return np.stack([tmp, cx * w[:, 1] - sx * w[:, 2], w[:, 0] + sy * tmp], axis=1)


def global_omega_from_rates(zyx, d):
    sz, cz, sy, cy = np.sin(zyx[:, 0]), np.cos(zyx[:, 0]), np.sin(zyx[:, 1]), np.cos(zyx[:, 1])
    return np.stack([-sz * d[:, 1] + cy * cz * d[:, 2], cz * d[:, 1] + cy * sz * d[:, 2], d[:, 0] - sy * d[:, 2]], axis=1)


def rates_from_global_omega(zyx, w):
    sz, cz, sy, cy = np.sin(zyx[:, 0]), np.cos(zyx[:, 0]), np.sin(zyx[:, 1]), np.cos(zyx[:, 1])
    return np.stack([(cz * sy * w[:, 0] + sy * sz * w[:, 1]) / cy + w[:, 2], -sz * w[:, 0] + cz * w[:, 1], (cz * w[:, 0] + sz * w[:, 1]) / cy], axis=1)


def rotation(zyx):
    """Rz(yaw) Ry(pitch) Rx(roll), [n][3][3]."""
    sz, cz, sy, cy, sx, cx = (f(zyx[:, i]) for i in range(3) for f in (np.sin, np.cos))
    return np.stack([np.stack([cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx], axis=1),
                     np.stack([sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx], axis=1),
                     np.stack([-sy, cy * sx, cy * cx], axis=1)], axis=1)


def solve_row_pivoting(S, B):
    """S X = B for [n][m][m], [n][m][k] by Gaussian elimination with partial (row) pivoting, every instance with its own pivots."""
    n, m = S.shape[0], S.shape[1]
    W = np.concatenate([S, B], axis=2)                           # the rows of [S | B] are exchanged and eliminated together
    rows = np.arange(n)
    for k in range(m):
        piv = k + np.argmax(np.abs(W[:, k:, k]), axis=1)
        if np.any(piv != k):
            wk, wp = W[rows, k].copy(), W[rows, piv].copy()
            W[rows, k], W[rows, piv] = wp, wk
        f = W[:, k + 1:, k] / W[:, k, k][:, None]
        W[:, k + 1:, k:] -= f[:, :, None] * W[:, k, k:][:, None, :]
    X = np.zeros_like(B)
    for i in range(m - 1, -1, -1):
        X[:, i] = (W[:, i, m:] - (W[:, i, None, i + 1:m] @ X[:, i + 1:])[:, 0]) / W[:, i, i][:, None]
    return X


_ORACLE = {}


def exact_foot_velocities(params, zyx, w_glob, qj, qdj):
    """World-frame contact-point velocities [4][3] (base at the origin, zero base linear velocity) from the oracle's Jacobians, in double:
    what the numpy twins of tests/test_oracle_estimator.py and tests/_groundtwin.py use in place of a central difference of the FK."""
    if "o" not in _ORACLE:
        from oracle.pyoracle import Oracle
        _ORACLE["o"] = Oracle(params)
    sz, cz, sy, cy = np.sin(zyx[0]), np.cos(zyx[0]), np.sin(zyx[1]), np.cos(zyx[1])
    rates = [(cz * sy * w_glob[0] + sy * sz * w_glob[1]) / cy + w_glob[2], -sz * w_glob[0] + cz * w_glob[1], (cz * w_glob[0] + sz * w_glob[1]) / cy]
    return _ORACLE["o"].rbd_full(np.concatenate([np.zeros(3), zyx, qj]), np.concatenate([np.zeros(3), rates, qdj]))["ee_vel"]


def tick(oracle, cfg, st, dt, quat, w_local, a_local, qj, qdj, contact, height=None, **mutant):
    """One tick for n instances; st (from init) is updated in place.  -> dict(zyx[n][3], omega[n][3] (world), xhat[n][18], P[n][18][18],
    yaw[n] (unwrapped), det[n] (of P[0:2, 0:2] before the branch), shrink[n] (bool), cond[n] (of S, in double)), longdouble where it is a
    filter quantity."""
    unknown = set(mutant) - set(MUTANTS)
    assert not unknown, unknown
    mu = lambda k: bool(mutant.get(k, False))
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    quat, w_local, a_local, qj, qdj = (f64(np.atleast_2d(a)).astype(LD) for a in (quat, w_local, a_local, qj, qdj))
    contact = np.atleast_2d(contact) != 0
    n = quat.shape[0]
    dt = LD(float(dt))

    # updateImu
    zyx = quat_to_zyx(quat, clamp=not mu("no_pitch_clamp"))
    w_glob = global_omega_from_rates(zyx, rates_from_local_omega(zyx, w_local))
    rates_g = rates_from_global_omega(zyx, w_glob)

    # leg kinematics with the base at the origin and zero linear velocity: the oracle's, in double
    pos, vel = np.zeros((n, 4, 3)), np.zeros((n, 4, 3))
    for i in range(n):
        o = oracle.rbd_full(np.concatenate([np.zeros(3), f64(zyx[i]), f64(qj[i])]), np.concatenate([np.zeros(3), f64(rates_g[i]), f64(qdj[i])]))
        pos[i], vel[i] = o["ee_pos"], o["ee_vel"]
    pos, vel = pos.astype(LD), vel.astype(LD)

    A = np.eye(18, dtype=LD)
    Bm = np.zeros((18, 3), dtype=LD)
    for i in range(3):
        A[i, 3 + i] = dt
        Bm[i, i] = dt * dt if mu("b_dt2") else LD(0.5) * dt * dt
        Bm[3 + i, i] = dt
    g981 = LD(9.81) if mu("g981_double") else F981
    q = np.zeros((n, 18), dtype=LD)
    q[:, 0:3] = (dt * g981 / F20 if mu("q_pos_with_velocity_literal") else dt / F20) * LD(cfg.imu_process_noise_position)
    q[:, 3:6] = (dt * g981 / F20) * LD(cfg.imu_process_noise_velocity)
    q[:, 6:18] = dt * LD(cfg.foot_process_noise_position)
    r = np.zeros((n, 28), dtype=LD)
    r[:, 0:12] = LD(cfg.foot_sensor_noise_position)
    r[:, 12:24] = LD(cfg.foot_sensor_noise_velocity)
    r[:, 24:28] = LD(cfg.foot_height_sensor_noise)
    sus = np.where(contact, LD(1), LD(100))                     # high_suspect_number, [n][4]
    sus3 = np.repeat(sus, 3, axis=1)
    if not mu("no_suspicion_q"):
        q[:, 6:18] *= sus3
    r[:, 0:12] *= sus3
    if not mu("no_suspicion_velocity"):
        r[:, 12:24] *= sus3
    if not mu("no_suspicion_height"):
        r[:, 24:28] *= sus
    y = np.zeros((n, 28), dtype=LD)
    y[:, 0:12] = -pos.reshape(n, 12)
    y[:, 12:24] = -vel.reshape(n, 12)
    y[:, (0 if mu("radius_on_x") else 2):12:3] += LD(cfg.foot_radius)

    acc = np.einsum("nij,nj->ni", rotation(zyx), a_local)
    acc[:, 2] -= LD(9.81)

    xh = st["xhat"] @ A.T + acc @ Bm.T
    if height is not None:
        for i in range(n):
            for f in range(4):
                y[i, 24 + f] = LD(float(height[i](float(xh[i, 6 + 3 * f]), float(xh[i, 7 + 3 * f]))))
    Pm = A @ st["P"] @ A.T
    Pm[:, np.arange(18), np.arange(18)] += q
    ey = y - xh @ C.T
    PmCt = Pm @ C.T                                              # [n][18][28]
    S = C @ PmCt
    S[:, np.arange(28), np.arange(28)] += r
    rhs = np.concatenate([ey[:, :, None], np.tile(C, (n, 1, 1))], axis=2)
    sol = solve_row_pivoting(S, rhs)                             # column 0: S^-1 ey, columns 1..18: S^-1 C
    xhat = xh + np.einsum("nij,nj->ni", PmCt, sol[:, :, 0])
    Pn = (np.eye(18, dtype=LD) - PmCt @ sol[:, :, 1:]) @ Pm
    P = (Pn + Pn.transpose(0, 2, 1)) / LD(2)
    det = P[:, 0, 0] * P[:, 1, 1] - P[:, 0, 1] * P[:, 1, 0]
    shrink = det > LD(0.00001 if mu("shrink_threshold_1e5") else 0.000001)
    blk = P[:, 0:2, 0:2].copy()
    if not mu("keep_cross_block"):
        P[shrink, 0:2, :] = 0
        P[shrink, :, 0:2] = 0
    P[shrink, 0:2, 0:2] = blk[shrink] / LD(10)
    st["xhat"], st["P"] = xhat, P

    # yaw continuity: yawLast + shortest_angular_distance(yawLast, yaw)
    d = np.fmod(np.fmod(zyx[:, 0] - st["yaw_last"], 2 * PI) + 2 * PI, 2 * PI)
    wrap = (d >= -PI) if mu("no_wrap") else (d > PI)
    d = np.where(wrap, d - 2 * PI, d)
    st["yaw_last"] = st["yaw_last"] + d
    return dict(zyx=zyx, omega=w_glob, xhat=xhat.copy(), P=P.copy(), yaw=st["yaw_last"].copy(), det=det, shrink=shrink,
                cond=np.linalg.cond(S.astype(np.float64)))
