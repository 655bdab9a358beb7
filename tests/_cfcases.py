"""Inputs of the contact-force observer tests (tests/test_ref_kf.py on the host emulator, tests/test_gpu_contact_force.py on the device)."""
import numpy as np

COND_LIMIT = 1e6         # a leg whose 5 x 6 block is worse conditioned than this is left out of the comparison with the oracle


def singular_leg_cases(n=40, seed=7):
    """-> rbd[n][32], tau[n][10]: joint configurations around zero knee / ankle angles, the places where the hunter's hip-pitch, knee and ankle
    axes (all parallel) can come into line and the per-leg 5 x 5 system A A' loses rank."""
    rng = np.random.default_rng(seed)
    rbd, tau = np.zeros((n, 32)), np.zeros((n, 10))
    for trial in range(n):
        rbd[trial, 5] = 0.9
        qj = 0.3 * rng.standard_normal(10)
        if trial % 2 == 0:
            qj[[3, 4, 8, 9]] = 0.0 if trial % 4 == 0 else 1e-9 * rng.standard_normal(4)   # straight knees and ankles
        if trial % 8 == 0:
            qj[[2, 7]] = 0.0
        rbd[trial, 6:16] = qj
        rbd[trial, 16:] = 0.2 * rng.standard_normal(16)
        tau[trial] = 5.0 * rng.standard_normal(10)
    return rbd, tau


def leg_blocks(oracle, rbd):
    """The 5 x 6 block A of each leg (rows: the leg's joints, columns: the wrench) from oracle.contact_force_rbd -> A[2][5][6], cond[2]."""
    J6 = oracle.contact_force_rbd(np.concatenate([rbd[3:6], rbd[0:3], rbd[6:16]]), np.zeros(16))["J6"]
    A = np.stack([J6[leg][:, 6 + 5 * leg:11 + 5 * leg].T for leg in range(2)])
    return A, np.array([np.linalg.cond(A[leg]) for leg in range(2)])


def wide_states(params, n=67, ticks=6, seed=67):
    """-> rbd[ticks][n][32], tau[ticks][n][10]: yaw and roll over +-3.1, pitch +-1.4, base omega ~ 5 rad/s, v ~ 3 m/s, joints +-0.6 about the
    default, joint rates ~ 10 rad/s, tau ~ 50 N m; a new state every tick (the observer state is what carries over)."""
    rng = np.random.default_rng(seed)
    qj0 = np.array(params["config"]["default_joint_state"])
    rbd = np.zeros((ticks, n, 32))
    rbd[..., 0] = rng.uniform(-3.1, 3.1, (ticks, n))
    rbd[..., 1] = rng.uniform(-1.4, 1.4, (ticks, n))
    rbd[..., 2] = rng.uniform(-3.1, 3.1, (ticks, n))
    rbd[..., 3:6] = rng.standard_normal((ticks, n, 3)) + [0, 0, 0.7]
    rbd[..., 6:16] = qj0 + rng.uniform(-0.6, 0.6, (ticks, n, 10))
    rbd[..., 16:19] = 5.0 * rng.standard_normal((ticks, n, 3))
    rbd[..., 19:22] = 3.0 * rng.standard_normal((ticks, n, 3))
    rbd[..., 22:32] = 10.0 * rng.standard_normal((ticks, n, 10))
    return rbd, 50.0 * rng.standard_normal((ticks, n, 10))
