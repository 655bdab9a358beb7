// Scenario draw at respawn (hb_plant_set_scenario in include/hunter_hip.h, where the procedure is defined): configuration check, the Philox
// blocks, the composition of one instance's terrain record, DevModel record, push record and parameter row from them, the log row of the
// finished episode and the per-tick push.  One instance per call, over pointers to that instance's rows; k_plant_scenario (one wavefront
// per instance), k_plant_push (one thread per instance) and the host emulator (tests/host_emu/scenarioemu.cpp, one emulated lane) run the
// same routines.
//
// Every sum, difference, product, quotient and square root below is rounded on its own (no fused multiply-add), as in hb_respawn.hpp; the
// terrain record and the model record come from the routines the host setters call (terrain_plane_record, modelvar_compose).
#pragma once
#include <stdint.h>
#include "../../include/hunter_hip.h"
#include "hb_math.hpp"
#include "hb_episode.hpp"
#include "hb_sensors.hpp"
#include "hb_contact.hpp"
#include "hb_modelvar.hpp"

namespace hb {

constexpr int SC_BLOCKS = 7;              // 0 slope, 1 friction, 2 payload, 3 - 5 mass scales, 6 push
constexpr int SC_DRAW = 4 * SC_BLOCKS;    // uniforms of a drawn set: u[4 block + word]
constexpr int SC_PUSH = 3;                // push record: first pushed step (-1: none), F_x, F_y
constexpr int SC_WORK = MODELVAR_PAYLOAD + HB_NBODY;
constexpr int SC_MODEL_WORDS = int(sizeof(DevModel) / sizeof(double));
static_assert(sizeof(DevModel) % sizeof(double) == 0, "DevModel is an array of doubles");

// null: valid; else the text that names what a configuration is refused for
inline const char* scenario_config_refusal(const hb_scenario_config& K) {
  const auto bad = [](double x) { return !(x >= 0.0) || !(x <= EP_DBL_MAX); };
  if (K.channels < 0 || K.channels > (HB_SC_SLOPE | HB_SC_MU | HB_SC_PAYLOAD | HB_SC_MASS | HB_SC_PUSH)) return "channels must be an OR of HB_SC_*";
  if (K.mu_per_point < 0 || K.mu_per_point > 1) return "mu_per_point must be 0 or 1";
  if (bad(K.grade_max) || K.grade_max > 1.0) return "grade_max must be in [0, 1]";
  if (bad(K.mu_lo)) return "mu_lo must be finite and >= 0";
  if (bad(K.mu_hi) || K.mu_hi < K.mu_lo) return "mu_hi must be finite and >= mu_lo";
  if (bad(K.payload_mass_max)) return "payload_mass_max must be finite and >= 0";
  for (int a = 0; a < 3; ++a) {
    if (!(K.payload_center[a] >= -EP_DBL_MAX && K.payload_center[a] <= EP_DBL_MAX)) return "payload_center must be finite";
    if (bad(K.payload_half_extent[a])) return "payload_half_extent must be finite and >= 0";
  }
  if (bad(K.mass_scale_range) || !(K.mass_scale_range < 1.0)) return "mass_scale_range must be in [0, 1)";
  if (bad(K.push_force_max)) return "push_force_max must be finite and >= 0";
  if (K.push_start_lo < 0) return "push_start_lo must be >= 0";
  if (K.push_start_hi < K.push_start_lo || K.push_start_hi > (1 << 20)) return "push_start_hi must be in [push_start_lo, 1 << 20]";
  if (K.push_ticks < ((K.channels & HB_SC_PUSH) ? 1 : 0)) return "push_ticks must be >= 1 with HB_SC_PUSH (>= 0 without)";
  if (K.log_capacity < 0 || K.log_capacity > HB_SC_LOG_MAX) return "log_capacity must be in 0 .. HB_SC_LOG_MAX";
  if (K.reserved[0] != 0 || K.reserved[1] != 0) return "`reserved` must be 0";
  return nullptr;
}

HB_HD int scenario_block_channel(int block) {
  return block == 0 ? HB_SC_SLOPE : (block == 1 ? HB_SC_MU : (block == 2 ? HB_SC_PAYLOAD : (block <= 5 ? HB_SC_MASS : HB_SC_PUSH)));
}
HB_HD bool scenario_block_needed(const hb_scenario_config& K, int block) { return (K.channels & scenario_block_channel(block)) != 0; }

// Block `block` of (instance, episode) into its four slots of u[SC_DRAW]; words[4] (or null) receives the raw Philox words.  Blocks are
// independent: the kernel draws one per lane.
HB_HD void scenario_draw_block(const hb_scenario_config& K, uint32_t instance, uint32_t episode, int block, double* u, uint32_t* words) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const Philox4 p = philox4x32_10(instance, episode, HB_SC_STREAM, uint32_t(block), uint32_t(K.seed), uint32_t(K.seed >> 32));
  for (int a = 0; a < 4; ++a) {
    if (words) words[a] = p.w[a];
    u[4 * block + a] = (double(p.w[a]) + 0.5) * 2.3283064365386963e-10;  // 2^-32
  }
}

// scen before the first draw: zero, no push
HB_HD void scenario_row_init(double* scen, double* push) {
  for (int a = 0; a < HB_SC_N; ++a) scen[a] = 0.0;
  scen[HB_SC_PUSH_START] = -1.0;
  push[0] = -1.0; push[1] = 0.0; push[2] = 0.0;
}

// The composition for one instance from a drawn set (slots of blocks nobody needed are not read).  ter[Terrain::size] and *mdl hold the
// instance's records on entry and the new ones on return; the part of a channel that is off is not touched.  N: the nominal model;
// spawn_xy: q_spawn[0:2]; scen[HB_SC_N], push[SC_PUSH]: written whole; work[SC_WORK]: the caller's (LDS on the device), for the payload and the
// scales handed to modelvar_compose.
HB_HD void scenario_compose(const hb_scenario_config& K, const double* u, const double* spawn_xy, double ground_z, const DevModel& N, double* ter,
                            DevModel* mdl, double* scen, double* push, double* work) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int a = 0; a < HB_SC_N; ++a) scen[a] = 0.0;
  if (K.channels & HB_SC_SLOPE) {
    const double gx = K.grade_max * (2.0 * u[0] - 1.0), gy = K.grade_max * (2.0 * u[1] - 1.0);
    const double l = sqrt((gx * gx + gy * gy) + 1.0);
    double pl[4] = {-gx / l, -gy / l, 1.0 / l, 0.0};
    pl[3] = (pl[0] * spawn_xy[0] + pl[1] * spawn_xy[1]) + pl[2] * ground_z;
    terrain_plane_record(pl, terrain_normal_length(pl), ter);
    scen[HB_SC_GRADE] = gx;
    scen[HB_SC_GRADE + 1] = gy;
  }
  if (K.channels & HB_SC_MU)
    for (int c = 0; c < HB_NC; ++c) {
      const double m = K.mu_lo + (K.mu_hi - K.mu_lo) * u[4 + (K.mu_per_point ? c : 0)];
      ter[Terrain::mu + c] = m;
      scen[HB_SC_MUS + c] = m;
    }
  if (K.channels & (HB_SC_PAYLOAD | HB_SC_MASS)) {
    double *payload = work, *scale = work + MODELVAR_PAYLOAD;
    for (int k = 0; k < MODELVAR_PAYLOAD; ++k) payload[k] = 0.0;
    if (K.channels & HB_SC_PAYLOAD) {
      payload[Payload::m] = K.payload_mass_max * u[8];
      for (int a = 0; a < 3; ++a) payload[Payload::r + a] = K.payload_center[a] + K.payload_half_extent[a] * (2.0 * u[9 + a] - 1.0);
      for (int k = 0; k < 4; ++k) scen[HB_SC_PAYLOAD_M + k] = payload[k];
    }
    if (K.channels & HB_SC_MASS)
      for (int b = 0; b < HB_NBODY; ++b) {
        scale[b] = 1.0 + K.mass_scale_range * (2.0 * u[12 + b] - 1.0);
        scen[HB_SC_SCALE + b] = scale[b];
      }
    modelvar_compose(N, (K.channels & HB_SC_MASS) ? scale : nullptr, (K.channels & HB_SC_PAYLOAD) ? payload : nullptr, mdl);
  }
  push[0] = -1.0; push[1] = 0.0; push[2] = 0.0;
  if (K.channels & HB_SC_PUSH) {
    const int start = K.push_start_lo + int(u[24] * double(K.push_start_hi - K.push_start_lo + 1));
    push[0] = double(start);
    push[1] = K.push_force_max * (2.0 * u[25] - 1.0);
    push[2] = K.push_force_max * (2.0 * u[26] - 1.0);
    for (int a = 0; a < SC_PUSH; ++a) scen[HB_SC_PUSH_START + a] = push[a];
  }
}

// The wrench of one instance for the step that follows: (F_x, F_y, 0, 0, 0, 0) on the steps start .. start + push_ticks - 1 of the
// instance's current record (steps = its STEPS), else zero; a record with start < 0 ("none") never pushes.
HB_HD void scenario_push_wrench(const hb_scenario_config& K, const double* push, int steps, double* wrench) {
  const double s = double(steps);
  const bool on = push[0] >= 0.0 && push[0] <= s && s < push[0] + double(K.push_ticks);
  wrench[0] = on ? push[1] : 0.0;
  wrench[1] = on ? push[2] : 0.0;
  for (int a = 2; a < 6; ++a) wrench[a] = 0.0;
}

// The log row of the episode that `cause` finishes, from its record, the totals before the fold (EPISODE_INDEX = its index) and the scen
// still in place: lanes cx.lane, cx.lane + cx.nlanes, ... of the row; nothing once *count == capacity.  *count is lane 0's, after the row.
template <class Ctx>
HB_HD void scenario_log_append(const Ctx& cx, int capacity, int cause, const int* irec, const double* drec, const int* itot, const double* scen,
                               int* count, double* log) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int n = *count;
  if (n >= capacity) return;
  double* row = log + size_t(n) * HB_SC_LOG_W;
  for (int a = cx.lane; a < HB_SC_LOG_W; a += cx.nlanes) {
    double x;
    if (a == 0) x = double(itot[HB_RS_I_EPISODE_INDEX]);
    else if (a == 1) x = double(cause);
    else if (a == 2) x = double(irec[HB_EP_I_TICKS]);
    else if (a == 3) x = drec[HB_EP_D_LAST_BASE] - drec[HB_EP_D_START_POS];
    else if (a == 4) x = drec[HB_EP_D_LAST_BASE + 1] - drec[HB_EP_D_START_POS + 1];
    else if (a == 5) x = drec[HB_EP_D_TILT_MAX];
    else x = scen[a - 6];
    row[a] = x;
  }
  cx.sync();
  if (cx.lane == 0) *count = n + 1;
}

// The instance's rows (ter / mdl null: the channel pair is off and the array may not exist)
struct ScenarioRows {
  double* ter;      // [Terrain::size]
  double* mdl;      // [SC_MODEL_WORDS], the DevModel record as words
  double *push, *scen;   // [SC_PUSH] [HB_SC_N]
};
// The composed records out to the rows, consecutive lanes on consecutive words.
template <class Ctx>
HB_HD void scenario_store(const Ctx& cx, const ScenarioRows& r, const double* ter, const double* mdl, const double* push, const double* scen) {
  const int l = cx.lane, nl = cx.nlanes;
  if (r.ter)
    for (int a = l; a < Terrain::size; a += nl) r.ter[a] = ter[a];
  if (r.mdl)
    for (int a = l; a < SC_MODEL_WORDS; a += nl) r.mdl[a] = mdl[a];
  for (int a = l; a < SC_PUSH; a += nl) r.push[a] = push[a];
  for (int a = l; a < HB_SC_N; a += nl) r.scen[a] = scen[a];
}

}  // namespace hb
