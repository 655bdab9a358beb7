// Gait manager on the device: the per-instance gait scheduler and the command-driven gait selection of the reference manager,
// one thread per robot instance, ahead of the reference generation of the same pass (include/hunter_hip.h, hb_gait_reset):
//   * GaitSchedule::{insertModeSequenceTemplate, getModeSchedule, tileModeSequenceTemplate}   legged_interface/src/gait/GaitSchedule.cpp:57-161
//   * calculateVelAbs, walkGait, findInsertModeSequenceTemplateTimer      legged_interface/src/SwitchedModelReferenceManager.cpp:173-249
//   * the cmd_vel rate limiter                                 legged_controllers/include/legged_controllers/TargetTrajectoriesPublisher.h:97-129
// The work of an instance is a short serial edit of a list of at most HB_MAX_EVENTS event times, so the mapping is one lane per
// instance and the per-instance lists are laid out slot-major, instance-minor: element k of instance i lives at [k * stride + i],
// neighbouring lanes touch neighbouring addresses.  Nothing is kept in thread-private arrays (they would be indexed dynamically and
// end up in scratch): the lists are edited in place in HBM.  Event times are accumulated as last + (sw[k + 1] - sw[k]) — no product,
// nothing to contract or reassociate — and come out bit-identical to the host classes (gait.py, hunter_hip.hpp).
// A list edit that would not fit is detected by a dry run of the tiling BEFORE anything is written: an instance that overflows keeps its
// state and its window exactly as they were (status 1, frozen until the next reset).
#pragma once
#include "../../include/hunter_hip.h"
#include "hb_math.hpp"

namespace hb {

constexpr int GAIT_HIST = 50;   // velAbsHistory_ (SwitchedModelReferenceManager.cpp:243-247)
constexpr int GAIT_STANCE = 3;

struct GaitBatch {
  int B;              // instances of this view
  int stride;         // instances of the whole batch: the pitch of the slot-major arrays
  int* n_ev;          // [B] events of the persistent schedule (it has n_ev + 1 modes)
  double* ev;         // [HB_MAX_EVENTS][stride]
  int* modes;         // [HB_MAX_EVENTS + 1][stride]
  int* tpl_n;         // [B] phases of the current mode-sequence template
  double* tpl_sw;     // [HB_GAIT_MAX_PHASES + 1][stride]
  int* tpl_modes;     // [HB_GAIT_MAX_PHASES][stride]
  double* last_vel;   // [4][stride] lastVel_ of the rate limiter
  double* cmd;        // [B][4] the filtered command, instance-major: the reference-generation kernels read it as RefgenBatch::cmd
  double* hist;       // [GAIT_HIST][stride] velAbsHistory_ as a ring
  int* hist_n;        // [B]
  int* hist_head;     // [B] slot of the newest sample
  int* level;         // [B] gaitLevel_
  double* vel_abs;    // [B]
  double* vel_avg;    // [B]
  int* status;        // [B] sticky: 1 after an overflow
};

// index of the first event >= t of instance i's persistent schedule (std::lower_bound)
HB_HD int gait_bisect_left(const GaitBatch& g, int i, int n, double t) {
  const size_t S = g.stride;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (g.ev[mid * S + i] < t) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Number of events tileModeSequenceTemplate(start, final) would append (the start and whole templates until the last event reaches
// final), by the same additions; room + 1 as soon as it exceeds room (this also ends the loop for a template that does not advance).
HB_HD int gait_tile_count(const GaitBatch& g, int i, double start, double final_time, int room) {
  const size_t S = g.stride;
  const int np = g.tpl_n[i];
  int cnt = 1;
  double last = start;
  if (cnt > room) return room + 1;
  while (last < final_time) {
    if (cnt + np > room) return room + 1;
    for (int k = 0; k < np; ++k) last = last + (g.tpl_sw[(k + 1) * S + i] - g.tpl_sw[k * S + i]);
    cnt += np;
  }
  return cnt;
}

// tileModeSequenceTemplate (GaitSchedule.cpp:126-161) on a list of n events and n modes (the last mode was popped or is about to be
// written); the caller has checked the room with gait_tile_count.
HB_HD void gait_tile(const GaitBatch& g, int i, int& n, double start, double final_time) {
  const size_t S = g.stride;
  const int np = g.tpl_n[i];
  g.ev[n * S + i] = start;
  ++n;
  double last = start;
  while (last < final_time)
    for (int k = 0; k < np; ++k) {
      g.modes[n * S + i] = g.tpl_modes[k * S + i];
      last = last + (g.tpl_sw[(k + 1) * S + i] - g.tpl_sw[k * S + i]);
      g.ev[n * S + i] = last;
      ++n;
    }
  g.modes[n * S + i] = GAIT_STANCE;
}

// The hard-coded templates next to the reference manager (SwitchedModelReferenceManager.cpp:55-61) as instance i's template.
HB_HD void gait_store_selected_template(const GaitBatch& g, int i, bool trot) {
  const size_t S = g.stride;
  g.tpl_sw[0 * S + i] = 0.0;
  if (trot) {
    g.tpl_n[i] = 2;
    g.tpl_sw[1 * S + i] = 0.3; g.tpl_sw[2 * S + i] = 0.6;
    g.tpl_modes[0 * S + i] = 2; g.tpl_modes[1 * S + i] = 1;
  } else {
    g.tpl_n[i] = 1;
    g.tpl_sw[1 * S + i] = 0.5;
    g.tpl_modes[0 * S + i] = GAIT_STANCE;
  }
}

// insertModeSequenceTemplate(the instance's current template, start, final) (GaitSchedule.cpp:57-89); the template must already be
// stored.  false (nothing written): the list would overflow.
HB_HD bool gait_insert(const GaitBatch& g, int i, double pts_cfg, double start, double final_time) {
  const size_t S = g.stride;
  const int n0 = g.n_ev[i];
  const int idx = gait_bisect_left(g, i, n0, start);   // events from idx on and the modes behind them go
  double pts = pts_cfg;
  if (g.modes[idx * S + i] == GAIT_STANCE) pts = 0.0;
  int n = idx + (pts > 0.0 ? 1 : 0);
  const int cnt = gait_tile_count(g, i, start + pts, final_time, HB_MAX_EVENTS - n);
  if (n + cnt > HB_MAX_EVENTS) return false;
  if (pts > 0.0) {
    g.ev[idx * S + i] = start;
    g.modes[(idx + 1) * S + i] = GAIT_STANCE;
  }
  gait_tile(g, i, n, start + pts, final_time);
  g.n_ev[i] = n;
  return true;
}

// getModeSchedule(lower, upper) (GaitSchedule.cpp:94-121), with its quirks: everything before the event in front of `lower` is dropped
// and the first mode becomes STANCE, the last event and mode are popped and the template is tiled again from that event on.  The
// window it returns is the whole persistent list.  false (nothing written): the list would overflow.
HB_HD bool gait_get_mode_schedule(const GaitBatch& g, int i, double lower, double upper) {
  const size_t S = g.stride;
  const int n0 = g.n_ev[i];
  const int idx = gait_bisect_left(g, i, n0, lower);
  const int sh = idx > 0 ? idx - 1 : 0;
  const int nt = n0 - sh;                                  // events after the trim (>= 1: hb_gait_reset wants an initial event)
  const double start = nt > 0 ? g.ev[(n0 - 1) * S + i] : lower;
  int n = nt > 0 ? nt - 1 : 0;
  const int cnt = gait_tile_count(g, i, start, upper, HB_MAX_EVENTS - n);
  if (n + cnt > HB_MAX_EVENTS) return false;
  if (sh > 0) {
    for (int k = 0; k < n; ++k) g.ev[k * S + i] = g.ev[(k + sh) * S + i];
    for (int k = 0; k <= n; ++k) g.modes[k * S + i] = g.modes[(k + sh) * S + i];
  }
  if (idx > 0) g.modes[i] = GAIT_STANCE;
  gait_tile(g, i, n, start, upper);
  g.n_ev[i] = n;
  return true;
}

// lastVel_ moved towards the request by at most lim (TargetTrajectoriesPublisher.h:104-117)
HB_HD double gait_rate_limit(double req, double last, double lim) {
  double d = req - last;
  d = d > 0.0 ? (d < lim ? d : lim) : (d > -lim ? d : -lim);
  return last + d;
}

// A fresh reference object for instance i.
HB_HD void gait_reset_instance(const GaitBatch& g, int i, const hb_gait_config& K) {
  const size_t S = g.stride;
  g.n_ev[i] = K.n_init_events;
  for (int k = 0; k < K.n_init_events; ++k) g.ev[k * S + i] = K.init_event_times[k];
  for (int k = 0; k <= K.n_init_events; ++k) g.modes[k * S + i] = K.init_modes[k];
  g.tpl_n[i] = K.n_template_phases;
  for (int k = 0; k <= K.n_template_phases; ++k) g.tpl_sw[k * S + i] = K.template_switching_times[k];
  for (int k = 0; k < K.n_template_phases; ++k) g.tpl_modes[k * S + i] = K.template_modes[k];
  for (int k = 0; k < 4; ++k) {
    g.last_vel[k * S + i] = 0.0;
    g.cmd[size_t(i) * 4 + k] = 0.0;
  }
  g.hist_n[i] = 0;
  g.hist_head[i] = 0;
  g.level[i] = 0;
  g.vel_abs[i] = 0.0;
  g.vel_avg[i] = 0.0;
  g.status[i] = 0;
}

// One pass of instance i at time t0 with horizon T (SwitchedModelReferenceManager.cpp:145-158, gaitType_ == 0): rate limiter, window,
// velocity average, gait level, template insertion for the next pass.  The window goes to (w_n, w_ev [HB_MAX_EVENTS], w_modes
// [HB_MAX_EVENTS + 1]), the instance's rows of the planner's schedule.  x_now [22] is the observation, req [4] the incoming command.
HB_HD void gait_pass(const GaitBatch& g, int i, const hb_gait_config& K, double t0, double T, const double* x_now, const double* req, int* w_n,
                     double* w_ev, int* w_modes) {
  if (g.status[i] != 0) return;   // frozen after an overflow: window, command and state stay as they are
  const size_t S = g.stride;
  // 1. cmd_vel callback: every pass moves the filtered command by at most changeLimit_ towards the request
  double c0, c1, c2, c3;
  if (K.filter_cmd) {
    c0 = gait_rate_limit(req[0], g.last_vel[0 * S + i], 0.1);
    c1 = gait_rate_limit(req[1], g.last_vel[1 * S + i], 0.05);
    c2 = 0.0;
    c3 = gait_rate_limit(req[3], g.last_vel[3 * S + i], 0.3);
    g.last_vel[0 * S + i] = c0; g.last_vel[1 * S + i] = c1; g.last_vel[2 * S + i] = c2; g.last_vel[3 * S + i] = c3;
  } else {
    c0 = req[0]; c1 = req[1]; c2 = req[2]; c3 = req[3];
  }
  double* cf = g.cmd + size_t(i) * 4;
  cf[0] = c0; cf[1] = c1; cf[2] = c2; cf[3] = c3;
  // 2. the window the planner of this pass reads
  if (!gait_get_mode_schedule(g, i, t0 - T, t0 + 2.0 * T)) {
    g.status[i] = 1;
    return;
  }
  const int n = g.n_ev[i];
  *w_n = n;
  for (int k = 0; k < n; ++k) w_ev[k] = g.ev[k * S + i];
  for (int k = 0; k <= n; ++k) w_modes[k] = g.modes[k * S + i];
  // 3. calculateVelAbs on stateTrajectory[0] of cmdVelToTargetTrajectories: the command in the world frame by the observed ZYX angles
  //    with the 0.06 dead band (x, else y) is the "estimate", the command turned by the yaw alone the "command"
  double sz, cz, sy, cy, sx, cx;
  sincos_t(x_now[9], sz, cz);
  sincos_t(x_now[10], sy, cy);
  sincos_t(x_now[11], sx, cx);
  double e0 = (cz * cy) * c0 + (cz * sy * sx - sz * cx) * c1 + (cz * sy * cx + sz * sx) * c2;
  double e1 = (sz * cy) * c0 + (sz * sy * sx + cz * cx) * c1 + (sz * sy * cx - cz * sx) * c2;
  if (fabs(e0) < 0.06) e0 = 0.0;
  else if (fabs(e1) < 0.06) e1 = 0.0;
  const double v0 = cz * c0 - sz * c1, v1 = sz * c0 + cz * c1, v3 = c3 / 3.0;
  const double a0 = 0.5 * v0 + 0.5 * e0, a1 = 0.5 * v1 + 0.5 * e1, a3 = 0.5 * v3;
  const double vel_abs = sqrt(a0 * a0 + a1 * a1 + a3 * a3);
  int hn = g.hist_n[i], head = g.hist_head[i];
  head = head + 1 == GAIT_HIST ? 0 : head + 1;
  g.hist[head * S + i] = vel_abs;
  if (hn < GAIT_HIST) ++hn;
  double sum = 0.0;   // newest to oldest, as std::accumulate over the deque
  for (int k = 0, slot = head; k < hn; ++k) {
    sum += g.hist[slot * S + i];
    slot = slot == 0 ? GAIT_HIST - 1 : slot - 1;
  }
  const double vel_avg = sum / double(hn);
  g.hist_n[i] = hn;
  g.hist_head[i] = head;
  g.vel_abs[i] = vel_abs;
  g.vel_avg[i] = vel_avg;
  // 4. walkGait
  const int level = g.level[i];
  int want = level;
  if (vel_avg <= 0.02) want = 0;
  else if (vel_avg > 0.03 && vel_avg < 0.4) want = 1;
  else if (vel_avg >= 0.4) want = 3;
  if (want == level) return;
  g.level[i] = want;
  if (want == 3) return;   // "flying trot": the reference only reports it
  // 5. findInsertModeSequenceTemplateTimer: the first event of the window >= t0; the template takes effect from the next pass
  const int at = gait_bisect_left(g, i, n, t0);
  if (at >= n) return;
  gait_store_selected_template(g, i, want == 1);
  if (!gait_insert(g, i, K.phase_transition_stance_time, g.ev[at * S + i], t0 + T)) g.status[i] = 1;
}

// hb_gait_insert_template for instance i: the given template (n_switch times at sw, n_switch - 1 modes) becomes the instance's template
// and is inserted over [start, final].
HB_HD void gait_insert_template(const GaitBatch& g, int i, double pts, int n_switch, const double* sw, const int* modes, double start,
                                double final_time) {
  if (g.status[i] != 0) return;
  const size_t S = g.stride;
  g.tpl_n[i] = n_switch - 1;
  for (int k = 0; k < n_switch; ++k) g.tpl_sw[k * S + i] = sw[k];
  for (int k = 0; k < n_switch - 1; ++k) g.tpl_modes[k * S + i] = modes[k];
  if (!gait_insert(g, i, pts, start, final_time)) g.status[i] = 1;
}

}  // namespace hb
