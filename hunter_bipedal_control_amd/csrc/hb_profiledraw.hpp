// Profile draw at respawn (hb_plant_set_profile_draw in include/hunter_hip.h, where the procedure is defined): configuration check, the
// Philox blocks, the knots of one instance's ground and its parameter row from them, the log row of the finished episode, and the placement
// and the locate of a spawn state on a profile.  One instance per call, over pointers to that instance's rows; k_plant_profile_draw and
// k_plant_respawn (one wavefront per instance) and the host emulator (tests/host_emu/profiledrawemu.cpp, one emulated lane) run the same
// routines.  Plain C++ apart from HB_HD.
//
// Every sum, difference, product and quotient below is rounded on its own (no fused multiply-add), as in hb_scenario.hpp; the profile
// record and the map record come from the routines the host setters call (profile_compose, ground_compose).
#pragma once
#include <stdint.h>
#include "../../include/hunter_hip.h"
#include "hb_math.hpp"
#include "hb_episode.hpp"
#include "hb_sensors.hpp"
#include "hb_plant.hpp"
#include "hb_contact.hpp"
#include "hb_ground.hpp"

namespace hb {

constexpr int PD_BLOCKS = 3;                       // 0: kind, height, first riser, steps; 1: run; 2: friction
constexpr int PD_DRAW = 4 * PD_BLOCKS;             // uniforms of a drawn set: u[4 block + word]
constexpr int PD_KNOTS = 2 * HB_PROFILE_MAX_KNOTS; // a knot row: (s, z) pairs, zero behind the last knot
constexpr double PD_REACH = 1e3;                   // bound on |s0|, |at|, run_hi and |ground_z| (the validity argument of the header)
constexpr double PD_RISER_MIN = 1e-3;              // narrowest riser and shortest tread [m]
static_assert(2 + 2 * 7 <= HB_PROFILE_MAX_KNOTS, "a flight of seven stairs fits a profile");

// null: valid; else the text that names what a configuration is refused for
inline const char* profile_draw_config_refusal(const hb_profile_draw_config& K) {
  const auto finite = [](double x) { return x >= -EP_DBL_MAX && x <= EP_DBL_MAX; };
  if (K.kinds < 1 || K.kinds > (HB_PD_FLAT | HB_PD_CURB | HB_PD_STAIRS)) return "kinds must be an OR of HB_PD_*, at least one";
  if (K.mu_per_point < 0 || K.mu_per_point > 1) return "mu_per_point must be 0 or 1";
  if (!finite(K.dir[0]) || !finite(K.dir[1])) return "dir must be finite";
  {
    const double len = sqrt(K.dir[0] * K.dir[0] + K.dir[1] * K.dir[1]);
    if (!(len > 0.0) || !finite(len)) return "dir must have a length above zero";
  }
  if (!finite(K.height_lo)) return "height_lo must be finite";
  if (!finite(K.height_hi) || K.height_hi < K.height_lo) return "height_hi must be finite and >= height_lo";
  if (!finite(K.at_lo) || fabs(K.at_lo) > PD_REACH) return "at_lo must be within [-1e3, 1e3]";
  if (!finite(K.at_hi) || fabs(K.at_hi) > PD_REACH || K.at_hi < K.at_lo) return "at_hi must be within [at_lo, 1e3]";
  if (!(K.riser_slope > 0.0) || !(K.riser_slope <= 1.7)) return "riser_slope must be in (0, 1.7]";
  if (K.steps_lo < 1) return "steps_lo must be >= 1";
  if (K.steps_hi < K.steps_lo || K.steps_hi > 7) return "steps_hi must be in [steps_lo, 7]";
  if (!finite(K.run_lo)) return "run_lo must be finite";
  if (!finite(K.run_hi) || K.run_hi < K.run_lo || K.run_hi > PD_REACH) return "run_hi must be within [run_lo, 1e3]";
  {
    const double hmax = fabs(K.height_lo) > fabs(K.height_hi) ? fabs(K.height_lo) : fabs(K.height_hi);
    const double wq = hmax / K.riser_slope, w = wq > PD_RISER_MIN ? wq : PD_RISER_MIN;
    if (!(K.run_lo - w >= PD_RISER_MIN)) return "run_lo must leave a tread of 1e-3 behind the widest riser (run_lo - max(max|height| / riser_slope, 1e-3) >= 1e-3)";
  }
  if (!(K.mu_lo >= 0.0) || !finite(K.mu_lo)) return "mu_lo must be finite and >= 0";
  if (!finite(K.mu_hi) || K.mu_hi < K.mu_lo) return "mu_hi must be finite and >= mu_lo";
  if (K.follow_map < 0 || K.follow_map > 1) return "follow_map must be 0 or 1";
  if (K.log_capacity < 0 || K.log_capacity > HB_PD_LOG_MAX) return "log_capacity must be in 0 .. HB_PD_LOG_MAX";
  if (K.reserved[0] != 0 || K.reserved[1] != 0) return "`reserved` must be 0";
  return nullptr;
}

// Block `block` of (instance, episode) into its four slots of u[PD_DRAW]; words[4] (or null) receives the raw Philox words.  Blocks are
// independent: the kernel draws one per lane.
HB_HD void profile_draw_block(const hb_profile_draw_config& K, uint32_t instance, uint32_t episode, int block, double* u, uint32_t* words) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const Philox4 p = philox4x32_10(instance, episode, HB_PD_STREAM, uint32_t(block), uint32_t(K.seed), uint32_t(K.seed >> 32));
  for (int a = 0; a < 4; ++a) {
    if (words) words[a] = p.w[a];
    u[4 * block + a] = (double(p.w[a]) + 0.5) * 2.3283064365386963e-10;  // 2^-32
  }
}

// s0 of an instance: its spawn point along the stored unit direction a
HB_HD double profile_draw_s0(const double* a, const double* q_spawn) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a[0] * q_spawn[0] + a[1] * q_spawn[1];
}

// The level ground around s0: the FLAT knots, relative (rel) and the plant's (pk), and K = 2.  What the set call puts every instance on.
HB_HD int profile_draw_flat(double s0, double ground_z, double* rel, double* pk) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int k = 0; k < PD_KNOTS; ++k) { rel[k] = 0.0; pk[k] = 0.0; }
  rel[0] = s0 - 1.0;
  rel[2] = s0 + 1.0;
  for (int k = 0; k < 2; ++k) {
    pk[2 * k] = rel[2 * k];
    pk[2 * k + 1] = 0.0 + (ground_z + rel[2 * k + 1]);
  }
  return 2;
}

// The composition for one instance from a drawn set: the relative knots rel[PD_KNOTS] = (s, g), the plant's knots pk[PD_KNOTS] =
// (s, 0 + (ground_z + g)), both zero behind the last knot, and the parameter row row[HB_PD_N], written whole.  K.dir: the stored unit
// direction.  -> the number of knots.  A sequential routine (lane 0 on the device, over LDS).
HB_HD int profile_draw_knots(const hb_profile_draw_config& K, const double* u, double s0, double ground_z, double* rel, double* pk, double* row) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  int n = 0;
  for (int bit = 1; bit <= HB_PD_STAIRS; bit <<= 1) n += (K.kinds & bit) ? 1 : 0;
  const int pick = int(u[0] * double(n));
  int kind = 0, seen = 0;
  for (int bit = 1; bit <= HB_PD_STAIRS; bit <<= 1)
    if (K.kinds & bit) {
      if (seen == pick) kind = bit;
      ++seen;
    }
  const double h = K.height_lo + (K.height_hi - K.height_lo) * u[1];
  const double at = K.at_lo + (K.at_hi - K.at_lo) * u[2];
  const double sr = s0 + at;
  const int steps = K.steps_lo + int(u[3] * double(K.steps_hi - K.steps_lo + 1));
  const double r = K.run_lo + (K.run_hi - K.run_lo) * u[4];
  const double wq = fabs(h) / K.riser_slope, w = wq > PD_RISER_MIN ? wq : PD_RISER_MIN;
  for (int k = 0; k < PD_KNOTS; ++k) rel[k] = 0.0;
  for (int k = 0; k < HB_PD_N; ++k) row[k] = 0.0;
  int nk;
  if (kind == HB_PD_FLAT) {
    rel[0] = s0 - 1.0;
    rel[2] = s0 + 1.0;
    nk = 2;
  } else if (kind == HB_PD_CURB) {
    rel[0] = sr - 1.0;
    rel[2] = sr;
    rel[4] = sr + w;  rel[5] = h;
    rel[6] = (sr + w) + 1.0;  rel[7] = h;
    nk = 4;
  } else {
    rel[0] = sr - 1.0;
    for (int i = 0; i < steps; ++i) {
      const double sa = sr + double(i) * r;
      rel[2 + 4 * i] = sa;          rel[3 + 4 * i] = double(i) * h;
      rel[4 + 4 * i] = sa + w;      rel[5 + 4 * i] = double(i + 1) * h;
    }
    rel[2 + 4 * steps] = (sr + double(steps) * r) + 1.0;
    rel[3 + 4 * steps] = double(steps) * h;
    nk = 2 + 2 * steps;
  }
  for (int k = 0; k < PD_KNOTS; ++k) pk[k] = 0.0;
  for (int k = 0; k < nk; ++k) {
    pk[2 * k] = rel[2 * k];
    pk[2 * k + 1] = 0.0 + (ground_z + rel[2 * k + 1]);
  }
  row[HB_PD_KIND] = double(kind);
  if (kind != HB_PD_FLAT) {
    row[HB_PD_HEIGHT] = h;
    row[HB_PD_AT] = at;
  }
  if (kind == HB_PD_STAIRS) {
    row[HB_PD_STEPS] = double(steps);
    row[HB_PD_RUN] = r;
  }
  for (int c = 0; c < HB_NC; ++c) row[HB_PD_MUS + c] = K.mu_lo + (K.mu_hi - K.mu_lo) * u[8 + (K.mu_per_point ? c : 0)];
  return nk;
}

// The log row of the episode that `cause` finishes, from its record, the totals before the fold (EPISODE_INDEX = its index) and the
// parameter row still in place: lanes cx.lane, cx.lane + cx.nlanes, ... of the row; nothing once *count == capacity.  *count is lane
// 0's, after the row.  a: the stored unit direction.
template <class Ctx>
HB_HD void profile_draw_log_append(const Ctx& cx, int capacity, int cause, const double* a, const int* irec, const double* drec, const int* itot,
                                   const double* row, int* count, double* log) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int n = *count;
  if (n >= capacity) return;
  double* out = log + size_t(n) * HB_PD_LOG_W;
  for (int k = cx.lane; k < HB_PD_LOG_W; k += cx.nlanes) {
    double x;
    if (k == 0) x = double(itot[HB_RS_I_EPISODE_INDEX]);
    else if (k == 1) x = double(cause);
    else if (k == 2) x = double(irec[HB_EP_I_TICKS]);
    else if (k == 3) x = a[0] * (drec[HB_EP_D_LAST_BASE] - drec[HB_EP_D_START_POS]) + a[1] * (drec[HB_EP_D_LAST_BASE + 1] - drec[HB_EP_D_START_POS + 1]);
    else if (k == 4) x = drec[HB_EP_D_TILT_MAX];
    else x = row[k - 5];
    out[k] = x;
  }
  cx.sync();
  if (cx.lane == 0) *count = n + 1;
}

// The instance's rows (map null: the controller's map does not follow)
struct ProfileDrawRows {
  double *prof, *knots, *row, *map;   // [Profile::stored] [PD_KNOTS] [HB_PD_N] [Ground::size]
};
// The composed records out to the rows, consecutive lanes on consecutive words.
template <class Ctx>
HB_HD void profile_draw_store(const Ctx& cx, const ProfileDrawRows& r, const double* prof, const double* knots, const double* row, const double* map) {
  const int l = cx.lane, nl = cx.nlanes;
  for (int k = l; k < Profile::stored; k += nl) r.prof[k] = prof[k];
  for (int k = l; k < PD_KNOTS; k += nl) r.knots[k] = knots[k];
  for (int k = l; k < HB_PD_N; k += nl) r.row[k] = row[k];
  if (r.map)
    for (int k = l; k < Ground::size; k += nl) r.map[k] = map[k];
}

// ---- a spawn state on a profile (k_plant_respawn with a profile in force) ---------------------------------------------------------------
// Vertical placement.  pro: the instance's stored record; feet[12] = the contact points at q on entry and on return (re-evaluated at the
// placed q).  Point c is measured against the facet under it; the shift is the largest any point asks for, so no point ends below
// `clearance` and the one that asked for it ends at it.
HB_HD void profile_place(const DevModel& Mdl, const hb_respawn_config& K, const double* pro, double* q, double* feet) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!K.place) return;
  double shift = -EP_INF;
  for (int c = 0; c < HB_NC; ++c) {
    const double* x = feet + 3 * c;
    const double* r = pro + Profile::seg + Profile::rec * profile_segment(pro, x);
    const double gap = ((r[Terrain::T + 2] * x[0] + r[Terrain::T + 5] * x[1]) + r[Terrain::T + 8] * x[2]) - r[Terrain::d];
    const double s = (K.clearance - gap) / r[Terrain::T + 8];
    if (s > shift) shift = s;
  }
  q[2] = q[2] + shift;
  plant_feet(Mdl, q, feet);
}
// What a profile step leaves behind besides its outputs, for a state nobody stepped to: seg[5] = the segment under the four contact
// points and the base origin, base[Terrain::size] = the Terrain record of the facet under the base origin with the instance's friction.
HB_HD void profile_locate_state(const double* pro, const double* q, const double* feet, int* seg, double* base) {
  for (int c = 0; c < HB_NC + 1; ++c) seg[c] = profile_segment(pro, c < HB_NC ? feet + 3 * c : q);
  const double* r = pro + Profile::seg + Profile::rec * seg[HB_NC];
  for (int k = 0; k < Terrain::size; ++k) base[k] = k < Profile::rec ? r[k] : pro[Profile::head + k];
}

}  // namespace hb
