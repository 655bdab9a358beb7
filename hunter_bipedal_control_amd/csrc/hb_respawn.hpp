// Respawn of ended instances (hb_plant_respawn in include/hunter_hip.h, where the procedure is defined): configuration check, decision,
// fold of a finished episode record into the totals, draw and placement of the spawn state, and the writes that put one instance of every
// subsystem back.  One instance per call, over pointers to that instance's rows; k_plant_respawn (one wavefront per instance) and the host
// emulator (tests/host_emu/respawnemu.cpp, one emulated lane) run the same routines.
//
// Every sum, difference and product below is rounded on its own (no fused multiply-add), as in hb_episode.hpp.
#pragma once
#include <stdint.h>
#include "../../include/hunter_hip.h"
#include "hb_math.hpp"
#include "hb_episode.hpp"
#include "hb_sensors.hpp"
#include "hb_plant.hpp"
#include "hb_estimator.hpp"

namespace hb {

// null: valid; else the text that names what a configuration is refused for
inline const char* respawn_config_refusal(const hb_respawn_config& K) {
  const auto bad = [](double x) { return !(x >= 0.0) || !(x <= EP_DBL_MAX); };
  if (bad(K.clearance)) return "clearance must be finite and >= 0";
  if (bad(K.yaw_range)) return "yaw_range must be finite and >= 0";
  if (bad(K.joint_pos_sigma)) return "joint_pos_sigma must be finite and >= 0";
  if (bad(K.base_vel_sigma)) return "base_vel_sigma must be finite and >= 0";
  if (K.hold_ticks < 0) return "hold_ticks must be >= 0";
  if (K.max_ticks < 0) return "max_ticks must be >= 0";
  if (K.place < 0 || K.place > 1) return "place must be 0 or 1";
  if (K.reserved[0] != 0 || K.reserved[1] != 0) return "`reserved` must be 0";
  return nullptr;
}

// 0: the instance stays; else the cause its episode is folded under (HB_EP_FALLEN, HB_EP_NONFINITE, HB_RS_TIMEOUT)
HB_HD int respawn_decide(const hb_respawn_config& K, const int* irec) {
  const int end = irec[HB_EP_I_END_TICK];
  if (end >= 0) return irec[HB_EP_I_STEPS] - (end + 1) >= K.hold_ticks ? irec[HB_EP_I_END_CAUSE] : 0;
  if (K.max_ticks > 0 && irec[HB_EP_I_TICKS] >= K.max_ticks) return HB_RS_TIMEOUT;
  return 0;
}

HB_HD void respawn_totals_init(int* itot, double* dtot) {
  for (int a = 0; a < HB_RS_NI; ++a) itot[a] = 0;
  for (int a = 0; a < HB_RS_ND; ++a) dtot[a] = 0.0;
}

// step 1 (EPISODE_INDEX is step 5's)
HB_HD void respawn_fold(int cause, const int* irec, const double* drec, int* itot, double* dtot) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int ticks = irec[HB_EP_I_TICKS];
  if (cause == HB_EP_FALLEN) itot[HB_RS_I_N_FALLEN] += 1;
  else if (cause == HB_EP_NONFINITE) itot[HB_RS_I_N_NONFINITE] += 1;
  else itot[HB_RS_I_N_TIMEOUT] += 1;
  itot[HB_RS_I_TICKS_SUM] += ticks;
  if (itot[HB_RS_I_EPISODES] == 0 || ticks < itot[HB_RS_I_TICKS_MIN]) itot[HB_RS_I_TICKS_MIN] = ticks;
  if (ticks > itot[HB_RS_I_TICKS_MAX]) itot[HB_RS_I_TICKS_MAX] = ticks;
  itot[HB_RS_I_SLIP_TICKS_SUM] += irec[HB_EP_I_SLIP_TICKS];
  itot[HB_RS_I_WBC_FAIL_TICKS_SUM] += irec[HB_EP_I_WBC_FAIL_TICKS];
  itot[HB_RS_I_STEPS_SUM] += irec[HB_EP_I_STEPS];
  itot[HB_RS_I_LAST_CAUSE] = cause;
  itot[HB_RS_I_LAST_TICKS] = ticks;
  itot[HB_RS_I_EPISODES] += 1;
  const double dx = drec[HB_EP_D_LAST_BASE] - drec[HB_EP_D_START_POS], dy = drec[HB_EP_D_LAST_BASE + 1] - drec[HB_EP_D_START_POS + 1];
  dtot[HB_RS_D_DIST_X_SUM] += dx;
  dtot[HB_RS_D_DIST_Y_SUM] += dy;
  dtot[HB_RS_D_WORK_ABS_SUM] += drec[HB_EP_D_WORK_ABS];
  if (drec[HB_EP_D_TILT_MAX] > dtot[HB_RS_D_TILT_MAX]) dtot[HB_RS_D_TILT_MAX] = drec[HB_EP_D_TILT_MAX];
  for (int j = 0; j < HB_NJ; ++j)
    if (drec[HB_EP_D_TAU_MAX + j] > dtot[HB_RS_D_TAU_MAX]) dtot[HB_RS_D_TAU_MAX] = drec[HB_EP_D_TAU_MAX + j];
}

// ---- draw (step 2) ----------------------------------------------------------------------------------------------------------------
constexpr int RS_BLOCKS = 5;                            // block 0: the yaw uniform; 1-3: joint normals 0-9; 4: base velocity normals 12-14
constexpr int RS_N_JOINT = 0, RS_N_BASE_VEL = 12;       // first normal of the two Gaussian channels
constexpr int RS_DRAW = 4 * RS_BLOCKS;                  // doubles of a drawn set: [0] = u, [4 + n] = normal n

HB_HD bool respawn_block_needed(const hb_respawn_config& K, int block) {
  return block == 0 ? K.yaw_range > 0.0 : (block <= 3 ? K.joint_pos_sigma > 0.0 : (block == 4 && K.base_vel_sigma > 0.0));
}
// Block `block` of (instance, episode) into its four slots of draw[RS_DRAW]; words[4] (or null) receives the raw Philox words.  Blocks are
// independent: the kernel draws one per lane.
HB_HD void respawn_draw_block(const hb_respawn_config& K, uint32_t instance, uint32_t episode, int block, double* draw, uint32_t* words) {
  const Philox4 p = philox4x32_10(instance, episode, HB_RS_STREAM, uint32_t(block), uint32_t(K.seed), uint32_t(K.seed >> 32));
  if (words)
    for (int a = 0; a < 4; ++a) words[a] = p.w[a];
  double* z = draw + 4 * block;
  if (block == 0) {
    z[0] = (double(p.w[0]) + 0.5) * 2.3283064365386963e-10;  // 2^-32
    z[1] = z[2] = z[3] = 0.0;
  } else {
    box_muller(p.w[0], p.w[1], z[0], z[1]);
    box_muller(p.w[2], p.w[3], z[2], z[3]);
  }
}
// (q, v) [16] each from the given spawn state and a drawn set (slots of blocks nobody needed are not read); v_spawn null: zero
HB_HD void respawn_perturb(const hb_respawn_config& K, const double* q_spawn, const double* v_spawn, const double* draw, double* q, double* v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int a = 0; a < 16; ++a) { q[a] = q_spawn[a]; v[a] = v_spawn ? v_spawn[a] : 0.0; }
  if (K.yaw_range > 0.0) {
    const double s = 2.0 * draw[0] - 1.0;
    q[3] = q_spawn[3] + K.yaw_range * s;
  }
  if (K.joint_pos_sigma > 0.0)
    for (int j = 0; j < HB_NJ; ++j) {
      const double d = K.joint_pos_sigma * draw[4 + RS_N_JOINT + j];
      q[6 + j] = q_spawn[6 + j] + d;
    }
  if (K.base_vel_sigma > 0.0)
    for (int a = 0; a < 3; ++a) {
      const double d = K.base_vel_sigma * draw[4 + RS_N_BASE_VEL + a];
      v[a] = v[a] + d;
    }
}

// ---- placement (step 3) -------------------------------------------------------------------------------------------------------------
// plane[4] = unit normal and d.  feet[12] = the contact points at q on entry and on return (re-evaluated at the placed q, so that they are
// bit for bit what hb_plant_reset computes from the stored state).
HB_HD void respawn_place(const DevModel& Mdl, const hb_respawn_config& K, const double* plane, double* q, double* feet) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!K.place) return;
  double g = EP_INF;
  for (int c = 0; c < HB_NC; ++c) {
    const double* x = feet + 3 * c;
    const double gc = ((plane[0] * x[0] + plane[1] * x[1]) + plane[2] * x[2]) - plane[3];
    if (gc < g) g = gc;
  }
  const double s = K.clearance - g;
  for (int a = 0; a < 3; ++a) {
    const double d = s * plane[a];
    q[a] = q[a] + d;
  }
  plant_feet(Mdl, q, feet);
}

// ---- the instance's rows of every subsystem (a null group: its arrays do not exist) ---------------------------------------------------
struct RespawnRows {
  // plant
  double *q, *v, *anchor, *lambda, *vdot, *tau_last, *rbd;   // [16] [16] [12] [12] [16] [10] [HB_NRBD]
  int *pinned, *contact_last;                                // [4] [4]
  double *q_last, *v_last;                                   // [16] [16] last spawned state
  // contact model (c_imp null: none)
  double *c_imp, *c_gap, *c_pvel, *c_res;                    // [12] [4] [12] [1]
  int *c_touching, *c_status;                                // [4] [1]
  // joint model (j_imp null: none)
  double *j_imp, *j_tau_applied, *j_friction, *j_limit, *j_res;   // [20] [10] [10] [10] [1]
  int* j_status;
  // actuator record (a_tau_first null: none)
  double *a_tau_first, *a_tau_mean, *a_rcmd[5];              // [10] each
  uint64_t* a_last_ts;
  int* estop;                                                // [1] or null
  // episode
  int* irec;
  double *drec, *trace;                                      // trace: [trace_cap][HB_EP_TRACE_W] or null
  int trace_cap;
  // estimator (xhat null: none)
  double *xhat, *P, *yaw_last, *cf_z;                        // [18] [324] [1] [HB_NV]
  // resident observation
  double *res_rbd, *res_x0;                                  // [HB_NRBD] [HB_NX]
  // pending flags of the MPC side
  int* rg_pending;
  unsigned char* mpc_pending;
};

// Steps 4 - 8 for one instance, lanes cx.lane, cx.lane + cx.nlanes, ... of every row (consecutive lanes on consecutive words).  q, v [16],
// feet [12]: the spawn state and its contact points; rbd [HB_NRBD], x0 [HB_NX]: its repacked forms; plane[4].  The episode record (a
// sequential routine) and the scalars are lane 0's.
template <class Ctx>
HB_HD void respawn_write(const Ctx& cx, const RespawnRows& r, const double* q, const double* v, const double* feet, const double* rbd,
                         const double* x0, const double* plane) {
  const int l = cx.lane, nl = cx.nlanes;
  const auto zero = [l, nl](double* p, int n) { for (int a = l; a < n; a += nl) p[a] = 0.0; };
  for (int a = l; a < 16; a += nl) { r.q[a] = q[a]; r.v[a] = v[a]; r.q_last[a] = q[a]; r.v_last[a] = v[a]; r.vdot[a] = 0.0; }
  for (int a = l; a < 12; a += nl) { r.anchor[a] = feet[a]; r.lambda[a] = 0.0; }
  for (int a = l; a < HB_NC; a += nl) { r.pinned[a] = 0; r.contact_last[a] = 1; }
  zero(r.tau_last, HB_NJ);
  for (int a = l; a < HB_NRBD; a += nl) { r.rbd[a] = rbd[a]; r.res_rbd[a] = rbd[a]; }
  for (int a = l; a < HB_NX; a += nl) r.res_x0[a] = x0[a];
  if (r.c_imp) {
    zero(r.c_imp, 12); zero(r.c_gap, 4); zero(r.c_pvel, 12);
    for (int a = l; a < HB_NC; a += nl) r.c_touching[a] = 0;
    if (l == 0) { r.c_res[0] = 0.0; r.c_status[0] = 0; }
  }
  if (r.j_imp) {
    zero(r.j_imp, 20); zero(r.j_tau_applied, HB_NJ); zero(r.j_friction, HB_NJ); zero(r.j_limit, HB_NJ);
    if (l == 0) { r.j_res[0] = 0.0; r.j_status[0] = 0; }
  }
  if (r.a_tau_first) {
    zero(r.a_tau_first, HB_NJ); zero(r.a_tau_mean, HB_NJ);
    for (int k = 0; k < 5; ++k) zero(r.a_rcmd[k], HB_NJ);
    if (l == 0) r.a_last_ts[0] = 0;
  }
  if (r.trace) zero(r.trace, r.trace_cap * HB_EP_TRACE_W);
  if (r.xhat) {
    for (int a = l; a < 18; a += nl) r.xhat[a] = a < 3 ? q[a] : (a < 6 ? 0.0 : feet[a - 6]);
    for (int a = l; a < 324; a += nl) r.P[a] = (a / 18 == a % 18) ? 100.0 : 0.0;
    zero(r.cf_z, HB_NV);
    if (l == 0) r.yaw_last[0] = 0.0;
  }
  if (l == 0) {
    if (r.estop) r.estop[0] = 0;
    EpisodeIn in{};
    in.q = q;
    in.n[0] = plane[0]; in.n[1] = plane[1]; in.n[2] = plane[2];
    in.d = plane[3];
    episode_init(in, r.irec, r.drec);
    r.rg_pending[0] = 1;
    r.mpc_pending[0] = 1;
  }
}

}  // namespace hb
