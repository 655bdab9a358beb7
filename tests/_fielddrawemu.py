"""Helpers of the field-draw tests (tests/test_field_draw_host.py, tests/test_gpu_field_draw.py):

  * build() of tests/host_emu/libfielddrawemu.so — csrc/hb_fielddraw.hpp compiled for the host behind a tiny C API (fielddrawemu.cpp),
    under the file lock of tests/_hostemu.py, installed atomically, rebuilt when a source it includes is newer;
  * an independent twin of the procedure as include/hunter_hip.h defines it above hb_plant_set_field_draw: the draw (Philox4x32-10 of
    tests/_respawnemu.py's import, the counter layout of the header), the parameters by kind, the grid origin, the height of every node,
    the parameter row, the log row, the vertical placement on a field and the locate of the placed state.  Written from the header text
    in Python floats (IEEE doubles), one operation per rounding in the order written, so heights, header, row and log row are EXACT; it
    shares no route with the C++.  Placement and locate go through the leg kinematics, which the caller passes in (foot_fn(q[1][16]) ->
    [1][4][3] or [1][12]: the device's own); the facets (cell, triangle, plane, distance from the nearest node line or diagonal) are
    tests/_fieldemu.py facet(), the numpy definition of the height field.
"""
import fcntl
import math
import os
import subprocess

import numpy as np

import _contactemu as ce
import _fieldemu as fe
import _respawnemu as rs
from hunter_bipedal_control_amd import abi

HERE, CSRC = ce.HERE, ce.CSRC
_p = ce._p
NMAX = abi.HB_FIELD_MAX_NODES
HEAD_BLOCKS, NODE_BLOCKS = 2, NMAX * NMAX // 4
MARGIN = 1e-6                      # [m] in (u, w): what a compared point keeps from every node line and cell diagonal
KINDS = (abi.HB_FD_FLAT, abi.HB_FD_ROUGH, abi.HB_FD_TILT, abi.HB_FD_TILT_ROUGH)


def build():
    so = HERE / "libfielddrawemu.so"
    deps = [HERE / "fielddrawemu.cpp", CSRC.parents[1] / "include" / "hunter_hip.h", *CSRC.glob("*.hpp")]
    with open(HERE / ".hostemu.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            tmp = HERE / f"libfielddrawemu.{os.getpid()}.so"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", str(tmp), str(HERE / "fielddrawemu.cpp")])
            os.replace(tmp, so)
    return so


# ---- the twin -----------------------------------------------------------------------------------------------------------------------------
def block_words(cfg, inst, episode, block):
    seed = int(cfg.seed)
    return rs.se.philox4x32_10([inst & 0xFFFFFFFF, episode, abi.HB_FD_STREAM, block], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])


def uniform(word) -> float:
    return (float(word) + 0.5) * 2.0 ** -32


def direction(cfg):
    dx, dy = float(cfg.dir[0]), float(cfg.dir[1])
    ln = math.sqrt(dx * dx + dy * dy)
    return dx / ln, dy / ln


def kinds_of(cfg):
    return [k for k in KINDS if int(cfg.kinds) & k]


def kind_of(cfg, inst, episode) -> int:
    """The kind of episode `episode` of global instance `inst` alone (word 0 of block 0)."""
    ks = kinds_of(cfg)
    return ks[int(uniform(block_words(cfg, inst, episode, 0)[0]) * float(len(ks)))]


def origin(cfg, q_spawn):
    ax, ay = direction(cfg)
    x, y = float(q_spawn[0]), float(q_spawn[1])
    return (ax * x + ay * y) - cfg.centre[0], ((-ay) * x + ax * y) - cfg.centre[1]


def node_uniforms(cfg, inst, episode):
    """u[NMAX][NMAX]: the uniform of every node of the pitch numbering n = iu NMAX + iw, word n % 4 of block 2 + n // 4."""
    out = np.zeros(NMAX * NMAX)
    for k in range(NODE_BLOCKS):
        out[4 * k:4 * k + 4] = [uniform(w) for w in block_words(cfg, inst, episode, HEAD_BLOCKS + k)]
    return out.reshape(NMAX, NMAX)


def node_height(cfg, A, p, r, iu, iw, u) -> float:
    """g of node (iu, iw) of the grid from its uniform."""
    un, wn = float(iu) * cfg.spacing[0], float(iw) * cfg.spacing[1]
    eu, ew = un - cfg.centre[0], wn - cfg.centre[1]
    c = 0.0 if (abs(eu) <= cfg.calm and abs(ew) <= cfg.calm) else 1.0
    return (p * eu + r * ew) + (A * (2.0 * u - 1.0)) * c


def draw(cfg, inst, episode, q_spawn, ground_z):
    """The draw of episode `episode` of global instance `inst` -> dict(kind, a, origin, row[HB_FD_N], mu[4], un[NMAX][NMAX] the node
    uniforms, g / heights / map [NMAX][NMAX] = the relative heights, the plant's 0 + (ground_z + g) and the map's 0 + g, all zero beyond
    (nu, nw), header[8] = a | origin | spacing | nu, nw)."""
    u0 = [uniform(w) for w in block_words(cfg, inst, episode, 0)]
    u1 = [uniform(w) for w in block_words(cfg, inst, episode, 1)]
    ks = kinds_of(cfg)
    kind = ks[int(u0[0] * float(len(ks)))]
    A = cfg.amp_lo + (cfg.amp_hi - cfg.amp_lo) * u0[1]
    p = cfg.slope_u_lo + (cfg.slope_u_hi - cfg.slope_u_lo) * u0[2]
    r = cfg.slope_w_lo + (cfg.slope_w_hi - cfg.slope_w_lo) * u0[3]
    if kind in (abi.HB_FD_FLAT, abi.HB_FD_TILT):
        A = 0.0
    if kind in (abi.HB_FD_FLAT, abi.HB_FD_ROUGH):
        p = r = 0.0
    mu = [cfg.mu_lo + (cfg.mu_hi - cfg.mu_lo) * u1[c if cfg.mu_per_point else 0] for c in range(4)]
    row = np.array([float(kind), A, p, r, *mu])
    un = node_uniforms(cfg, inst, episode)
    nu, nw = int(cfg.n_nodes[0]), int(cfg.n_nodes[1])
    g, hts, gmap = np.zeros((NMAX, NMAX)), np.zeros((NMAX, NMAX)), np.zeros((NMAX, NMAX))
    for iu in range(nu):
        for iw in range(nw):
            g[iu, iw] = node_height(cfg, A, p, r, iu, iw, float(un[iu, iw]))
            hts[iu, iw] = 0.0 + (float(ground_z) + g[iu, iw])
            gmap[iu, iw] = 0.0 + g[iu, iw]
    ax, ay = direction(cfg)
    org = origin(cfg, q_spawn)
    header = np.array([ax, ay, org[0], org[1], cfg.spacing[0], cfg.spacing[1], float(nu), float(nw)])
    return dict(kind=kind, a=np.array([ax, ay]), origin=np.array(org), row=row, mu=np.array(mu), un=un, g=g, heights=hts, map=gmap, header=header,
                n=(nu, nw))


def flat(cfg, q_spawn, ground_z):
    """The level ground the set call puts an instance on -> (heights[NMAX][NMAX], header[8])."""
    nu, nw = int(cfg.n_nodes[0]), int(cfg.n_nodes[1])
    hts = np.zeros((NMAX, NMAX))
    hts[:nu, :nw] = 0.0 + (float(ground_z) + 0.0)
    ax, ay = direction(cfg)
    org = origin(cfg, q_spawn)
    return hts, np.array([ax, ay, org[0], org[1], cfg.spacing[0], cfg.spacing[1], float(nu), float(nw)])


def log_row(episode_index, cause, rec, row, a):
    """The row of a finished episode from its record (a dict of abi.split_episode_record of ONE instance), the row it ran under and the
    stored direction."""
    progress = a[0] * (rec["LAST_BASE"][0] - rec["START_POS"][0]) + a[1] * (rec["LAST_BASE"][1] - rec["START_POS"][1])
    return np.concatenate([[float(episode_index), float(cause), float(rec["TICKS"]), progress, rec["TILT_MAX"]], row])


# ---- a state on a field ----------------------------------------------------------------------------------------------------------------------
def field_of(tw, relative=False):
    """The field dict of tests/_fieldemu.py facet() from a draw of the twin (relative: the map's heights)."""
    nu, nw = tw["n"]
    return dict(dir=tw["a"], origin=tw["origin"], spacing=tw["header"][4:6], heights=(tw["map"] if relative else tw["heights"])[:nu, :nw], mu=tw["mu"])


def _feet(foot_fn, q):
    return np.asarray(foot_fn(np.asarray(q, dtype=float)[None]))[0].reshape(4, 3)


def points(q, foot_fn):
    """[5][3]: the four contact points and the base origin at q."""
    return np.vstack([_feet(foot_fn, q), np.asarray(q, dtype=float)[None, 0:3]])


def margin(fld, q, foot_fn) -> float:
    """The smallest distance [m in (u, w)] of a contact point or the base origin at q from a node line or the diagonal of its cell."""
    return float(fe.facet(fld, points(q, foot_fn))[2].min())


def gaps(fld, q, foot_fn, against_base=False):
    """gap_c of the four contact points at q, each over the facet under it (against_base: the MUTANT, all four over the facet under the
    base origin) -> (gap[4], n_z[4])."""
    pts = points(q, foot_fn)
    planes = fe.facet(fld, pts)[1]
    out, nz = np.zeros(4), np.zeros(4)
    for c in range(4):
        pl = planes[4] if against_base else planes[c]
        out[c], nz[c] = pl[:3] @ pts[c] - pl[3], pl[2]
    return out, nz


def place(cfg, q, foot_fn, fld, against_base=False):
    """The vertical placement: q[2] += max_c (clearance - gap_c) / n_cz."""
    q = np.array(q, dtype=float)
    if cfg.place:
        g, nz = gaps(fld, q, foot_fn, against_base)
        q[2] += ((cfg.clearance - g) / nz).max()
    return q


def locate(fld, q, foot_fn):
    """sel[5]: the facet under the four contact points and the base origin at q."""
    return fe.facet(fld, points(q, foot_fn))[0].astype(np.int32)


def base_plane(fld, q):
    """(n[3], d) of the facet under the base origin at q."""
    return fe.facet(fld, np.asarray(q, dtype=float)[None, 0:3])[1][0]


# ---- the configurations of the tests (the validity sweep of tests/test_field_draw_host.py runs over all of them) -----------------------------
GRIDS = ((2, 2), (5, 7), (7, 5), (3, 32), (32, 32))
CONFIGS = dict(
    # tests/test_field_draw_host.py: every kind, a direction that is not of unit length, friction per point, a calm square of two cells
    host_all=dict(kinds=abi.HB_FD_ALL, mu_per_point=1, dir=(3.0, 4.0), n_nodes=(5, 7), spacing=(0.11, 0.09), centre=(0.2, 0.25), calm=0.1,
                  amp_lo=0.005, amp_hi=0.02, slope_u_lo=-0.2, slope_u_hi=0.3, slope_w_lo=-0.15, slope_w_hi=0.1, mu_lo=0.3, mu_hi=0.9,
                  seed=0x1234567890ABCDEF, log_capacity=3),
    # the edges of the admitted set: the finest spacing with the amplitude that just fits the bound beside the steepest tilt that does,
    # the coarsest spacing, the spawn point on the corner of the grid
    host_fine=dict(kinds=abi.HB_FD_ALL, dir=(-1.0, 1e-3), n_nodes=(32, 32), spacing=(1e-3, 1e-3), centre=(0.0, 0.03), calm=0.0, amp_lo=0.0,
                   amp_hi=1e-4, slope_u_lo=-1.0, slope_u_hi=1.0, slope_w_lo=-1.0, slope_w_hi=1.0, mu_lo=0.0, mu_hi=2.0, seed=7),
    host_coarse=dict(kinds=abi.HB_FD_ROUGH | abi.HB_FD_TILT_ROUGH, dir=(0.0, 2.0), n_nodes=(32, 3), spacing=(10.0, 10.0), centre=(310.0, 0.0),
                     calm=5.0, amp_lo=2.0, amp_hi=2.0, slope_u_lo=-0.8, slope_u_hi=0.8, slope_w_lo=-0.8, slope_w_hi=0.8, mu_lo=0.5, mu_hi=0.5, seed=11),
    host_steep=dict(kinds=abi.HB_FD_TILT | abi.HB_FD_TILT_ROUGH, dir=(1.0, 1.0), n_nodes=(7, 5), spacing=(0.05, 0.2), centre=(0.15, 0.4), calm=0.0,
                    amp_lo=0.0, amp_hi=0.005, slope_u_lo=-1.2, slope_u_hi=1.2, slope_w_lo=-0.9, slope_w_hi=0.9, mu_lo=0.2, mu_hi=0.4, seed=13),
    # tests/test_gpu_field_draw.py
    gpu_small=dict(kinds=abi.HB_FD_ALL, mu_per_point=1, dir=(3.0, 4.0), n_nodes=(5, 7), spacing=(0.3, 0.25), centre=(0.47, 0.66), calm=0.1,
                   amp_lo=0.004, amp_hi=0.012, slope_u_lo=-0.1, slope_u_hi=0.15, slope_w_lo=-0.08, slope_w_hi=0.08, mu_lo=0.4, mu_hi=0.9,
                   seed=0xC0FFEE1234, log_capacity=4),
    gpu_full=dict(kinds=abi.HB_FD_ALL, mu_per_point=0, dir=(1.0, 0.0), n_nodes=(32, 32), spacing=(0.06, 0.05), centre=(0.91, 0.79), calm=0.05,
                  amp_lo=0.002, amp_hi=0.01, slope_u_lo=-0.12, slope_u_hi=0.12, slope_w_lo=-0.1, slope_w_hi=0.1, mu_lo=0.5, mu_hi=0.8, seed=99,
                  log_capacity=2),
    gpu_loop=dict(kinds=abi.HB_FD_ALL, mu_per_point=0, dir=(1.0, 0.0), n_nodes=(32, 32), spacing=(0.1, 0.1), centre=(0.63, 1.56), calm=0.15,
                  amp_lo=0.002, amp_hi=0.008, slope_u_lo=-0.05, slope_u_hi=0.05, slope_w_lo=-0.03, slope_w_hi=0.03, mu_lo=0.6, mu_hi=0.9,
                  seed=0x5EED, follow_map=1, log_capacity=4),
)
