// Ground map of the controller (hb_ground_set_profile): per instance a piecewise-linear height over one horizontal direction, what the
// swing planner, the command target and the filter's foot-height rows take for the ground in place of the level plane.  The map has the
// shape of the plant's terrain profile (hb_contact.hpp Profile: direction, knots, open-ended end segments) without its friction, and its
// heights are RELATIVE to the level ground the controller has always assumed: g = 0 everywhere is the world of the base forms.
// Plain C++ apart from HB_HD: tests/host_emu/groundemu.cpp compiles this header with g++.
#pragma once
#include "hb_contact.hpp"

namespace hb {

// The record of an instance (doubles): dir: a (unit); nseg: K - 1 as a double; brk[k] = s_k (k = 1 .. nseg - 1 are scanned);
// hgt[k] = g_k; slope[j] = (g_{j+1} - g_j) / (s_{j+1} - s_j), computed once on the host.
struct Ground {
  static constexpr int dir = 0, nseg = dir + 2, brk = nseg + 1, hgt = brk + HB_PROFILE_MAX_KNOTS, slope = hgt + HB_PROFILE_MAX_KNOTS,
                       size = slope + HB_PROFILE_MAX_KNOTS - 1;
};

// The record r[Ground::size] of VALID knots (K of them, (s, g), along the unit direction a): what ground_record composes once it has
// accepted them, and what k_plant_profile_draw composes for the map that follows a drawn profile, one knot per lane.  r is written whole.
template <class Ctx>
HB_HD void ground_compose(const Ctx& cx, int K, const double* a, const double* knots, double* r) {
  for (int k = cx.lane; k < Ground::size; k += cx.nlanes) r[k] = 0.0;
  cx.sync();
  if (cx.lane == 0) {
    r[Ground::dir] = a[0];
    r[Ground::dir + 1] = a[1];
    r[Ground::nseg] = double(K - 1);
  }
  for (int k = cx.lane; k < K; k += cx.nlanes) {
    r[Ground::brk + k] = knots[2 * k];
    r[Ground::hgt + k] = 0.0 + knots[2 * k + 1];   // (0 + : no negative zero, so that a level segment returns its height bit for bit)
  }
  for (int j = cx.lane; j + 1 < K; j += cx.nlanes) r[Ground::slope + j] = (knots[2 * j + 3] - knots[2 * j + 1]) / (knots[2 * j + 2] - knots[2 * j]);
  cx.sync();
}
// Host: the record r[Ground::size] of one instance from its map (K knots (s, g), direction), or the reason it is refused.  The checks
// are profile_record's (the routine is run on the map, so a plant profile is always a valid map and the two never drift apart); the
// direction is normalised by the same division.
inline const char* ground_record(int K, const double* dir, const double* knots, double* r) {
  double pro[Profile::stored];
  if (const char* why = profile_record(K, dir, knots, nullptr, 0.0, pro)) return why;
  ground_compose(OneLane{}, K, pro + Profile::dir, knots, r);
  return nullptr;
}

// G(x, y) of the map g: s = a . (x, y); the segment is the last j with s_j <= s, the end segments open-ended (the scan of
// profile_segment); G = g_j + m_j (s - s_j).  No contraction: a level segment returns g_j bit for bit, and the host twin of the tests
// rounds where this routine rounds.  A NaN argument selects segment 0 and returns NaN.  *seg (or null): the segment.
HB_HD double ground_height(const double* g, double x, double y, int* seg = nullptr) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double s = g[Ground::dir] * x + g[Ground::dir + 1] * y;
  const int nseg = int(g[Ground::nseg]);
  int j = 0;
  for (int k = 1; k < nseg; ++k) j = s >= g[Ground::brk + k] ? k : j;
  if (seg) *seg = j;
  return g[Ground::hgt + j] + g[Ground::slope + j] * (s - g[Ground::brk + j]);
}

}  // namespace hb
