// Per-instance episode record of the plant (hb_plant_set_episode in include/hunter_hip.h, where the procedure is defined): what a rollout
// produced, reduced on the device after every plant step, so that a batch of scenarios runs without a read-back per tick.  One instance
// per call, over pointers to that instance's rows of the plant's, the contact model's and the joint model's arrays; k_plant_episode /
// k_plant_episode_init (one thread per instance) and the host emulator (tests/host_emu/episodeemu.cpp) run the same routines.
//
// Every sum and product below is rounded on its own (no fused multiply-add): the record of a run then equals, value for value, the
// reduction of the per-tick outputs the getters return, whichever compiler built the routine.
#pragma once
#include <stdint.h>
#include "../../include/hunter_hip.h"
#include "hb_math.hpp"

namespace hb {

constexpr double EP_DBL_MAX = 1.7976931348623157e308;
constexpr double EP_INF = __builtin_huge_val();

inline bool episode_config_valid(const hb_episode_config& K) {
  if (K.reserved[0] != 0 || K.reserved[1] != 0 || K.reserved[2] != 0) return false;
  return K.slip_speed >= 0.0 && K.slip_speed <= EP_DBL_MAX && K.tilt_limit >= 0.0 && K.tilt_limit <= EP_DBL_MAX && K.stop_on_fall >= 0 &&
         K.stop_on_fall <= 1 && K.trace_every >= 0 && K.trace_capacity >= 0 && K.trace_capacity <= HB_EP_TRACE_MAX;
}

// What a step left behind for one instance.  The groups are null where their source is absent: wbc_status before the first WBC call, the
// contact group outside contact model 1, the joint group without a joint model.
struct EpisodeIn {
  const double *q, *v, *tau_last;   // [16] [16] [10]
  double n[3], d;                   // the instance's plane n . x = d
  const int* wbc_status;
  const double *gap, *lambda, *pvel, *res;   // [4] [12] [12] [1]
  const int *touching, *cstatus;             // [4] [1]
  const double* jres;
  const int* jstatus;
};

HB_HD bool episode_finite(const EpisodeIn& in) {
  bool finite = true;
  for (int a = 0; a < 16; ++a) finite = finite && fabs(in.q[a]) <= EP_DBL_MAX && fabs(in.v[a]) <= EP_DBL_MAX;
  return finite;
}
// n . x - d, summed over x, y, z in that order
HB_HD double episode_height(const EpisodeIn& in, const double* x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return ((in.n[0] * x[0] + in.n[1] * x[1]) + in.n[2] * x[2]) - in.d;
}

// The record of an episode that starts at the plant's present state.
HB_HD void episode_init(const EpisodeIn& in, int* irec, double* drec) {
  for (int a = 0; a < HB_EP_NI; ++a) irec[a] = 0;
  for (int a = 0; a < HB_EP_ND; ++a) drec[a] = 0.0;
  irec[HB_EP_I_END_TICK] = irec[HB_EP_I_FIRST_NONFINITE] = irec[HB_EP_I_FIRST_WBC_FAIL] = irec[HB_EP_I_FIRST_SLIP] = -1;
  for (int a = 0; a < 3; ++a) drec[HB_EP_D_START_POS + a] = in.q[a];
  for (int a = 0; a < 6; ++a) drec[HB_EP_D_LAST_BASE + a] = in.q[a];
  drec[HB_EP_D_HEIGHT_LAST] = episode_height(in, in.q);
  drec[HB_EP_D_HEIGHT_MIN] = EP_INF;
  drec[HB_EP_D_HEIGHT_MAX] = -EP_INF;
  drec[HB_EP_D_GAP_MIN] = EP_INF;
}

// The update after one plant step of length dt (steps 1 - 7 of the definition).  trace: the instance's [trace_capacity][HB_EP_TRACE_W];
// estop: the instance's emergency-stop latch, or null without stop_on_fall.
HB_HD void episode_update(const hb_episode_config& K, const EpisodeIn& in, double dt, int* irec, double* drec, double* trace, int* estop) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int k = irec[HB_EP_I_STEPS];
  irec[HB_EP_I_STEPS] = k + 1;
  const bool finite = episode_finite(in);
  if (!finite && irec[HB_EP_I_FIRST_NONFINITE] < 0) irec[HB_EP_I_FIRST_NONFINITE] = k;
  if (irec[HB_EP_I_END_TICK] >= 0) return;   // frozen
  if (!finite) {
    irec[HB_EP_I_END_TICK] = k;
    irec[HB_EP_I_END_CAUSE] = HB_EP_NONFINITE;
    return;
  }
  const double* q = in.q;
  const double* v = in.v;
  const double height = episode_height(in, q);
  const double tilt = fabs(q[4]) > fabs(q[5]) ? fabs(q[4]) : fabs(q[5]);
  const bool fallen = (in.cstatus && (in.cstatus[0] & HB_CONTACT_FALLEN)) || (K.tilt_limit > 0.0 && tilt > K.tilt_limit);
  if (fallen) {
    irec[HB_EP_I_END_TICK] = k;
    irec[HB_EP_I_END_CAUSE] = HB_EP_FALLEN;
    if (K.stop_on_fall && estop) estop[0] = 1;
    return;
  }
  irec[HB_EP_I_TICKS] += 1;
  for (int a = 0; a < 6; ++a) drec[HB_EP_D_LAST_BASE + a] = q[a];
  drec[HB_EP_D_HEIGHT_LAST] = height;
  if (height < drec[HB_EP_D_HEIGHT_MIN]) drec[HB_EP_D_HEIGHT_MIN] = height;
  if (height > drec[HB_EP_D_HEIGHT_MAX]) drec[HB_EP_D_HEIGHT_MAX] = height;
  if (tilt > drec[HB_EP_D_TILT_MAX]) drec[HB_EP_D_TILT_MAX] = tilt;
  double work_abs = 0.0, work_net = 0.0;
  for (int j = 0; j < HB_NJ; ++j) {
    const double t = in.tau_last[j], pw = t * v[6 + j];
    if (fabs(t) > drec[HB_EP_D_TAU_MAX + j]) drec[HB_EP_D_TAU_MAX + j] = fabs(t);
    work_abs += fabs(pw);
    work_net += pw;
  }
  drec[HB_EP_D_WORK_ABS] += dt * work_abs;
  drec[HB_EP_D_WORK_NET] += dt * work_net;
  if (in.wbc_status) {
    const int st = in.wbc_status[0];
    irec[HB_EP_I_WBC_STATUS_OR] |= st;
    if (st != 0) {
      irec[HB_EP_I_WBC_FAIL_TICKS] += 1;
      if (irec[HB_EP_I_FIRST_WBC_FAIL] < 0) irec[HB_EP_I_FIRST_WBC_FAIL] = k;
    }
  }
  int n_touching = 0;
  if (in.cstatus) {
    bool slip = false;
    for (int c = 0; c < HB_NC; ++c) {
      const double* lam = in.lambda + 3 * c;
      const double* pv = in.pvel + 3 * c;
      if (in.gap[c] < drec[HB_EP_D_GAP_MIN]) drec[HB_EP_D_GAP_MIN] = in.gap[c];
      const double fn = (in.n[0] * lam[0] + in.n[1] * lam[1]) + in.n[2] * lam[2];
      if (fn > drec[HB_EP_D_FN_MAX + c]) drec[HB_EP_D_FN_MAX + c] = fn;
      const int touch = in.touching[c] != 0 ? 1 : 0;
      irec[HB_EP_I_CONTACT_TICKS + c] += touch;
      if (touch && !irec[HB_EP_I_PREV_TOUCHING + c]) irec[HB_EP_I_TOUCHDOWNS + c] += 1;
      irec[HB_EP_I_PREV_TOUCHING + c] = touch;
      n_touching += touch;
      if (touch) {
        const double vn = (in.n[0] * pv[0] + in.n[1] * pv[1]) + in.n[2] * pv[2];
        const double t0 = pv[0] - vn * in.n[0], t1 = pv[1] - vn * in.n[1], t2 = pv[2] - vn * in.n[2];
        const double speed = sqrt((t0 * t0 + t1 * t1) + t2 * t2);
        if (speed > drec[HB_EP_D_SLIP_SPEED_MAX]) drec[HB_EP_D_SLIP_SPEED_MAX] = speed;
        slip = slip || speed > K.slip_speed;
      }
    }
    if (slip) {
      irec[HB_EP_I_SLIP_TICKS] += 1;
      if (irec[HB_EP_I_FIRST_SLIP] < 0) irec[HB_EP_I_FIRST_SLIP] = k;
    }
    if (in.res[0] > drec[HB_EP_D_RES_MAX]) drec[HB_EP_D_RES_MAX] = in.res[0];
    if (in.cstatus[0] & HB_CONTACT_UNCONVERGED) irec[HB_EP_I_UNCONVERGED_TICKS] += 1;
    irec[HB_EP_I_CONTACT_STATUS_OR] |= in.cstatus[0];
  }
  if (in.jstatus) {
    const int st = in.jstatus[0];
    if (in.jres[0] > drec[HB_EP_D_JRES_MAX]) drec[HB_EP_D_JRES_MAX] = in.jres[0];
    irec[HB_EP_I_JOINT_STATUS_OR] |= st;
    if (st & HB_EP_JOINT_CLAMP_BITS) irec[HB_EP_I_CLAMP_TICKS] += 1;
    if (st & HB_EP_JOINT_STOP_BITS) irec[HB_EP_I_STOP_TICKS] += 1;
  }
  if (K.trace_every > 0 && k % K.trace_every == 0 && irec[HB_EP_I_N_TRACE] < K.trace_capacity) {
    double* s = trace + size_t(irec[HB_EP_I_N_TRACE]) * HB_EP_TRACE_W;
    s[0] = double(k); s[1] = q[0]; s[2] = q[1]; s[3] = height; s[4] = q[3]; s[5] = q[4]; s[6] = q[5]; s[7] = double(n_touching);
    irec[HB_EP_I_N_TRACE] += 1;
  }
}

}  // namespace hb
