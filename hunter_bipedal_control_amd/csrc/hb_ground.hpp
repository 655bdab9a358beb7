// Ground map of the controller (hb_ground_set_profile; its two-dimensional form, hb_ground_set_field, is the second half of this file): per instance a piecewise-linear height over one horizontal direction, what the
// swing planner, the command target and the filter's foot-height rows take for the ground in place of the level plane.  The map has the
// shape of the plant's terrain profile (hb_contact.hpp Profile: direction, knots, open-ended end segments) without its friction, and its
// heights are RELATIVE to the level ground the controller has always assumed: g = 0 everywhere is the world of the base forms.
// Plain C++ apart from HB_HD: tests/host_emu/groundemu.cpp compiles this header with g++.
#pragma once
#include "hb_contact.hpp"
#include "hb_forms.hpp"  // MAP_NONE, MAP_PROFILE, MAP_FIELD

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

// ---- the field map (hb_ground_set_field): the grid of a plant height field (hb_contact.hpp Field) without its friction ----------------
// The header of an instance (doubles): direction a (unit) | origin (u0, w0) | spacing (du, dw) | nu, nw as doubles — the eight doubles
// field_cell reads; the heights g[iu * pitch + iw] stay in global memory, relative to the level ground like a profile map's.
struct GroundField {
  static constexpr int dir = 0, org = 2, step = 4, nu = 6, nw = 7, size = 8, pitch = Field::pitch, nz = Field::nz;
};
// The header h[GroundField::size] of a VALID map (node counts, the unit direction a, origin, spacing): what ground_field_record stores
// once it has accepted them, and what k_plant_field_draw stores for the map that follows a drawn field.
HB_HD void ground_field_compose(const int* n, const double* a, const double* org, const double* step, double* h) {
  h[GroundField::dir] = a[0]; h[GroundField::dir + 1] = a[1];
  h[GroundField::org] = org[0]; h[GroundField::org + 1] = org[1];
  h[GroundField::step] = step[0]; h[GroundField::step + 1] = step[1];
  h[GroundField::nu] = double(n[0]); h[GroundField::nw] = double(n[1]);
}
// Host: the header h[GroundField::size] of one instance from its map, or the reason it is refused (h is then not written).  The checks
// are field_record's, the triangle bound included (the routine is run on the map, so a plant field is always a valid map); the direction
// is normalised by the same division.
inline const char* ground_field_record(const int* n, const double* dir, const double* org, const double* step, const double* z, double* h) {
  double fld[Field::stored];
  if (const char* why = field_record(n, dir, org, step, z, nullptr, 0.0, fld)) return why;
  ground_field_compose(n, fld + Field::dir, org, step, h);
  return nullptr;
}
// G(x, y) of the field map (h: its header, z: its heights): the cell (i, j), the fractions and the triangle are field_cell's, the ones
// the plant's field_facet cuts its cells by; over the lower triangle (t = 0) G = g00 + (g10 - g00) fu + (g11 - g10) fw, over the upper
// G = g00 + (g01 - g00) fw + (g11 - g01) fu, left to right, every operation rounded on its own: a level cell returns g00 bit for bit.
// The four loads are issued together.  A NaN coordinate selects facet 0 and returns NaN.  *facet (or null): 2 (i (nw - 1) + j) + t.
HB_HD double ground_field_height(const double* h, const double* __restrict__ z, double x, double y, int* facet = nullptr) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double xy[2] = {x, y};
  const FieldCell fc = field_cell(h, z, xy);
  const double* c = fc.cell;
  const double g00 = c[0], g01 = c[1], g10 = c[GroundField::pitch], g11 = c[GroundField::pitch + 1];
  if (facet) *facet = 2 * (fc.i * (fc.nw - 1) + fc.j) + fc.t;
  const double e1 = fc.t ? g01 - g00 : g10 - g00, e2 = fc.t ? g11 - g01 : g11 - g10;
  const double f1 = fc.t ? fc.fw : fc.fu, f2 = fc.t ? fc.fu : fc.fw;
  return g00 + e1 * f1 + e2 * f2;
}

// What the planner, the command target and the filter put their points to.  MAP (hb_forms.hpp): MAP_NONE no map, MAP_PROFILE the profile
// map (gnd: its Ground record), MAP_FIELD the field map (gnd: its header, gz: its heights).  *id (or null): the segment or the facet.
template <int MAP>
HB_HD double map_height(const double* gnd, const double* gz, double x, double y, int* id = nullptr) {
  if constexpr (MAP == MAP_FIELD) return ground_field_height(gnd, gz, x, y, id);
  else return ground_height(gnd, x, y, id);
}

}  // namespace hb
