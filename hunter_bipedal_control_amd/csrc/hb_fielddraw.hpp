// Field draw at respawn (hb_plant_set_field_draw in include/hunter_hip.h, where the procedure is defined): configuration check, the Philox
// blocks, the parameters of one instance's ground and its row from them, the relative height of a node, the log row of the finished
// episode, and the placement and the locate of a spawn state on a height field.  One instance per call, over pointers to that instance's
// rows; k_plant_field_draw and k_plant_respawn_field (one wavefront per instance) and the host emulator (tests/host_emu/fielddrawemu.cpp,
// one emulated lane) run the same routines.  Plain C++ apart from HB_HD.
//
// Every sum, difference, product and quotient below is rounded on its own (no fused multiply-add), as in hb_profiledraw.hpp; the field
// record and the map header come from the routines the host setters call (field_compose, ground_field_compose).
#pragma once
#include <stdint.h>
#include "../../include/hunter_hip.h"
#include "hb_math.hpp"
#include "hb_episode.hpp"
#include "hb_sensors.hpp"
#include "hb_plant.hpp"
#include "hb_contact.hpp"
#include "hb_ground.hpp"
#include "hb_profiledraw.hpp"

namespace hb {

constexpr int FD_HEAD_BLOCKS = 2;                   // 0: kind, amplitude, the two slopes; 1: friction
constexpr int FD_NODE_BLOCKS = Field::nz / 4;       // block 2 + k: the uniforms of nodes 4 k .. 4 k + 3 in the pitch numbering
constexpr int FD_HEAD = 4 * FD_HEAD_BLOCKS;         // uniforms of the head blocks: u[4 block + word]
constexpr double FD_REACH = PD_REACH;               // bound on |ground_z|, |a . q_s| and |b . q_s| (the validity argument of the header)
constexpr double FD_STEP_MIN = 1e-3, FD_STEP_MAX = 10.0;
constexpr double FD_SLOPE2_MAX = 2.9;               // bound on (P + 2 amp_hi / du)^2 + (R + 2 amp_hi / dw)^2: 0.1 under field_record's 3
constexpr int FD_KINDS = HB_FD_FLAT | HB_FD_ROUGH | HB_FD_TILT | HB_FD_TILT_ROUGH;
static_assert(Field::nz % 4 == 0 && Field::pitch % 4 == 0, "a Philox block covers four nodes of one row");

// null: valid; else the text that names what a configuration is refused for
inline const char* field_draw_config_refusal(const hb_field_draw_config& K) {
  const auto finite = [](double x) { return x >= -EP_DBL_MAX && x <= EP_DBL_MAX; };
  if (K.kinds < 1 || K.kinds > FD_KINDS) return "kinds must be an OR of HB_FD_*, at least one";
  if (K.mu_per_point < 0 || K.mu_per_point > 1) return "mu_per_point must be 0 or 1";
  if (!finite(K.dir[0]) || !finite(K.dir[1])) return "dir must be finite";
  {
    const double len = sqrt(K.dir[0] * K.dir[0] + K.dir[1] * K.dir[1]);
    if (!(len > 0.0) || !finite(len)) return "dir must have a length above zero";
  }
  for (int k = 0; k < 2; ++k)
    if (K.n_nodes[k] < 2 || K.n_nodes[k] > HB_FIELD_MAX_NODES) return "n_nodes must be in 2 .. HB_FIELD_MAX_NODES";
  for (int k = 0; k < 2; ++k)
    if (!(K.spacing[k] >= FD_STEP_MIN && K.spacing[k] <= FD_STEP_MAX)) return "spacing must be within [1e-3, 10]";
  for (int k = 0; k < 2; ++k)
    if (!(K.centre[k] >= 0.0 && K.centre[k] <= double(K.n_nodes[k] - 1) * K.spacing[k])) return "centre must lie inside the grid (0 .. (n_nodes - 1) spacing)";
  if (!(K.calm >= 0.0) || !finite(K.calm)) return "calm must be finite and >= 0";
  if (!(K.amp_lo >= 0.0) || !finite(K.amp_lo)) return "amp_lo must be finite and >= 0";
  if (!finite(K.amp_hi) || K.amp_hi < K.amp_lo) return "amp_hi must be finite and >= amp_lo";
  if (!finite(K.slope_u_lo)) return "slope_u_lo must be finite";
  if (!finite(K.slope_u_hi) || K.slope_u_hi < K.slope_u_lo) return "slope_u_hi must be finite and >= slope_u_lo";
  if (!finite(K.slope_w_lo)) return "slope_w_lo must be finite";
  if (!finite(K.slope_w_hi) || K.slope_w_hi < K.slope_w_lo) return "slope_w_hi must be finite and >= slope_w_lo";
  {
    const double P = fabs(K.slope_u_lo) > fabs(K.slope_u_hi) ? fabs(K.slope_u_lo) : fabs(K.slope_u_hi);
    const double R = fabs(K.slope_w_lo) > fabs(K.slope_w_hi) ? fabs(K.slope_w_lo) : fabs(K.slope_w_hi);
    const double su = P + 2.0 * K.amp_hi / K.spacing[0], sw = R + 2.0 * K.amp_hi / K.spacing[1];
    if (!(su * su + sw * sw <= FD_SLOPE2_MAX)) return "slope and amplitude must keep every triangle under the field's limit ((P + 2 amp_hi / du)^2 + (R + 2 amp_hi / dw)^2 <= 2.9)";
  }
  if (!(K.mu_lo >= 0.0) || !finite(K.mu_lo)) return "mu_lo must be finite and >= 0";
  if (!finite(K.mu_hi) || K.mu_hi < K.mu_lo) return "mu_hi must be finite and >= mu_lo";
  if (K.follow_map < 0 || K.follow_map > 1) return "follow_map must be 0 or 1";
  if (K.log_capacity < 0 || K.log_capacity > HB_FD_LOG_MAX) return "log_capacity must be in 0 .. HB_FD_LOG_MAX";
  if (K.reserved[0] != 0 || K.reserved[1] != 0) return "`reserved` must be 0";
  return nullptr;
}

// Block `block` of (instance, episode): its four uniforms into u[0 .. 3]; words[4] (or null) receives the raw Philox words.  Blocks are
// independent: the kernel draws the head blocks one per lane and the node blocks four per lane.
HB_HD void field_draw_block(const hb_field_draw_config& K, uint32_t instance, uint32_t episode, int block, double* u, uint32_t* words) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const Philox4 p = philox4x32_10(instance, episode, HB_FD_STREAM, uint32_t(block), uint32_t(K.seed), uint32_t(K.seed >> 32));
  if (words) { words[0] = p.w[0]; words[1] = p.w[1]; words[2] = p.w[2]; words[3] = p.w[3]; }
  u[0] = (double(p.w[0]) + 0.5) * 2.3283064365386963e-10;  // 2^-32
  u[1] = (double(p.w[1]) + 0.5) * 2.3283064365386963e-10;
  u[2] = (double(p.w[2]) + 0.5) * 2.3283064365386963e-10;
  u[3] = (double(p.w[3]) + 0.5) * 2.3283064365386963e-10;
}

// The grid origin (u0, w0) of an instance: its spawn point, along the stored unit direction a and across it, stands at `centre`.  sq[2]
// (or null) receives (a . q_s, b . q_s), what the set call bounds by FD_REACH.
HB_HD void field_draw_origin(const hb_field_draw_config& K, const double* a, const double* q_spawn, double* org, double* sq = nullptr) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double su = a[0] * q_spawn[0] + a[1] * q_spawn[1];
  const double sw = (-a[1]) * q_spawn[0] + a[0] * q_spawn[1];
  org[0] = su - K.centre[0];
  org[1] = sw - K.centre[1];
  if (sq) { sq[0] = su; sq[1] = sw; }
}

// What the node routine needs of a drawn set, as the kind left it: A (0 for FLAT and TILT), p and r (0 for FLAT and ROUGH)
struct FieldDrawPar {
  double A, p, r;
};
// The parameters of one instance from its head blocks u[FD_HEAD]: the row row[HB_FD_N], written whole, and the node parameters.  A
// sequential routine (one lane on the device, over LDS).
HB_HD FieldDrawPar field_draw_head(const hb_field_draw_config& K, const double* u, double* row) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  int n = 0;
  for (int bit = 1; bit <= HB_FD_TILT_ROUGH; bit <<= 1) n += (K.kinds & bit) ? 1 : 0;
  const int pick = int(u[0] * double(n));
  int kind = 0, seen = 0;
  for (int bit = 1; bit <= HB_FD_TILT_ROUGH; bit <<= 1)
    if (K.kinds & bit) {
      if (seen == pick) kind = bit;
      ++seen;
    }
  const double A = K.amp_lo + (K.amp_hi - K.amp_lo) * u[1];
  const double p = K.slope_u_lo + (K.slope_u_hi - K.slope_u_lo) * u[2];
  const double r = K.slope_w_lo + (K.slope_w_hi - K.slope_w_lo) * u[3];
  const bool rough = kind == HB_FD_ROUGH || kind == HB_FD_TILT_ROUGH, tilt = kind == HB_FD_TILT || kind == HB_FD_TILT_ROUGH;
  FieldDrawPar par;
  par.A = rough ? A : 0.0;
  par.p = tilt ? p : 0.0;
  par.r = tilt ? r : 0.0;
  row[HB_FD_KIND] = double(kind);
  row[HB_FD_AMPLITUDE] = par.A;
  row[HB_FD_SLOPE_U] = par.p;
  row[HB_FD_SLOPE_W] = par.r;
  for (int c = 0; c < HB_NC; ++c) row[HB_FD_MUS + c] = K.mu_lo + (K.mu_hi - K.mu_lo) * u[4 + (K.mu_per_point ? c : 0)];
  return par;
}

// The relative height g of node (iu, iw) from its uniform un_: 0 beyond (nu, nw) (*inside: whether the node belongs to the grid).
HB_HD double field_draw_node(const hb_field_draw_config& K, const FieldDrawPar& par, int iu, int iw, double un_, bool* inside) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  *inside = iu < K.n_nodes[0] && iw < K.n_nodes[1];
  if (!*inside) return 0.0;
  const double un = double(iu) * K.spacing[0], wn = double(iw) * K.spacing[1];
  const double eu = un - K.centre[0], ew = wn - K.centre[1];
  const double c = (fabs(eu) <= K.calm && fabs(ew) <= K.calm) ? 0.0 : 1.0;
  const double plane = par.p * eu + par.r * ew;
  const double bump = (par.A * (2.0 * un_ - 1.0)) * c;
  return plane + bump;
}
// what the plant stores for a node of relative height g, and what the map does
HB_HD double field_draw_plant_height(double ground_z, double g) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return 0.0 + (ground_z + g);
}
HB_HD double field_draw_map_height(double g) { return 0.0 + g; }

// The four nodes of block 2 + k of (instance, episode) out to z[4 k .. 4 k + 3] (the plant's heights) and, with gz, the map's: 32
// contiguous bytes each.  No array is indexed by a variable.
HB_HD void field_draw_nodes(const hb_field_draw_config& K, const FieldDrawPar& par, uint32_t instance, uint32_t episode, int k, double ground_z,
                            double* __restrict__ z, double* __restrict__ gz) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const Philox4 p = philox4x32_10(instance, episode, HB_FD_STREAM, uint32_t(FD_HEAD_BLOCKS + k), uint32_t(K.seed), uint32_t(K.seed >> 32));
  const int iu = (4 * k) / Field::pitch, iw = (4 * k) % Field::pitch;
  bool in0, in1, in2, in3;
  const double g0 = field_draw_node(K, par, iu, iw + 0, (double(p.w[0]) + 0.5) * 2.3283064365386963e-10, &in0);
  const double g1 = field_draw_node(K, par, iu, iw + 1, (double(p.w[1]) + 0.5) * 2.3283064365386963e-10, &in1);
  const double g2 = field_draw_node(K, par, iu, iw + 2, (double(p.w[2]) + 0.5) * 2.3283064365386963e-10, &in2);
  const double g3 = field_draw_node(K, par, iu, iw + 3, (double(p.w[3]) + 0.5) * 2.3283064365386963e-10, &in3);
  double* o = z + 4 * k;
  o[0] = in0 ? field_draw_plant_height(ground_z, g0) : 0.0;
  o[1] = in1 ? field_draw_plant_height(ground_z, g1) : 0.0;
  o[2] = in2 ? field_draw_plant_height(ground_z, g2) : 0.0;
  o[3] = in3 ? field_draw_plant_height(ground_z, g3) : 0.0;
  if (gz) {
    double* m = gz + 4 * k;
    m[0] = in0 ? field_draw_map_height(g0) : 0.0;
    m[1] = in1 ? field_draw_map_height(g1) : 0.0;
    m[2] = in2 ? field_draw_map_height(g2) : 0.0;
    m[3] = in3 ? field_draw_map_height(g3) : 0.0;
  }
}

// The level ground of the configured grid: what the set call puts every instance on.  z[Field::nz] the plant's heights, gz (or null) the
// map's.
inline void field_draw_flat(const hb_field_draw_config& K, double ground_z, double* z, double* gz) {
  for (int iu = 0; iu < Field::pitch; ++iu)
    for (int iw = 0; iw < Field::pitch; ++iw) {
      const bool inside = iu < K.n_nodes[0] && iw < K.n_nodes[1];
      z[iu * Field::pitch + iw] = inside ? field_draw_plant_height(ground_z, 0.0) : 0.0;
      if (gz) gz[iu * Field::pitch + iw] = 0.0;
    }
}

// The log row of the episode that `cause` finishes: the profile draw's five leading entries (progress along a), then the parameter row
// still in place.  Lanes cx.lane, cx.lane + cx.nlanes, ... of the row; nothing once *count == capacity.  *count is lane 0's, after the row.
template <class Ctx>
HB_HD void field_draw_log_append(const Ctx& cx, int capacity, int cause, const double* a, const int* irec, const double* drec, const int* itot,
                                 const double* row, int* count, double* log) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int n = *count;
  if (n >= capacity) return;
  double* out = log + size_t(n) * HB_FD_LOG_W;
  for (int k = cx.lane; k < HB_FD_LOG_W; k += cx.nlanes) {
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

// ---- a spawn state on a height field (k_plant_respawn_field) --------------------------------------------------------------------------------
// Vertical placement.  fld: the instance's stored record, z: its heights; feet[12] = the contact points at q on entry and on return
// (re-evaluated at the placed q).  Point c is measured against the facet under it; the shift is the largest any point asks for, so no
// point ends below `clearance` and the one that asked for it ends at it.  A vertical shift changes no (u, w), hence no facet.
HB_HD void field_place(const DevModel& Mdl, const hb_respawn_config& K, const double* fld, const double* __restrict__ z, double* q, double* feet) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!K.place) return;
  double shift = -EP_INF;
  for (int c = 0; c < HB_NC; ++c) {
    const double* x = feet + 3 * c;
    double r[Profile::rec];
    field_facet(fld, z, x, r);
    const double gap = ((r[Terrain::T + 2] * x[0] + r[Terrain::T + 5] * x[1]) + r[Terrain::T + 8] * x[2]) - r[Terrain::d];
    const double s = (K.clearance - gap) / r[Terrain::T + 8];
    if (s > shift) shift = s;
  }
  q[2] = q[2] + shift;
  plant_feet(Mdl, q, feet);
}
// What a field step leaves behind besides its outputs, for a state nobody stepped to: sel[5] = the facet under the four contact points and
// the base origin, base[Terrain::size] = the Terrain record of the facet under the base origin with the instance's friction (what the
// host's field_locate writes).
HB_HD void field_locate_state(const double* fld, const double* __restrict__ z, const double* q, const double* feet, int* sel, double* base) {
  for (int k = 0; k < Terrain::size; ++k) base[k] = fld[Field::head + k];
  for (int c = 0; c < HB_NC; ++c) {
    double r[Profile::rec];
    sel[c] = field_facet(fld, z, feet + 3 * c, r);
  }
  sel[HB_NC] = field_facet(fld, z, q, base);
}

}  // namespace hb
