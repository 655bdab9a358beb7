// Height scan (hb_plant_set_height_scan / hb_plant_scan in include/hunter_hip.h, where the procedure is defined): the controller's field
// map perceived from the plant's ground — a robot-centred grid of limited range, with noise and lost returns, registered with the true
// or the estimated base position, that keeps what it saw once the ground has left the sensor's reach.  Configuration check, the origin of
// the grid, the height of a plane and of a field over a point, one node (sample point, truth, return rule, noise) and the lane-cooperative scan of one
// instance.  k_plant_scan (one wavefront per instance) and the host emulator (tests/host_emu/scanemu.cpp, one emulated lane) run the same
// routines.  Plain C++ apart from HB_HD.
//
// Every sum, difference, product and quotient below is rounded on its own (no fused multiply-add), as in hb_fielddraw.hpp.  The scan does
// not run the steepness check of field_record: ground_field_height needs no normal, so a noisy map of any steepness is a valid map.
#pragma once
#include <stdint.h>
#include "../../include/hunter_hip.h"
#include "hb_math.hpp"
#include "hb_episode.hpp"
#include "hb_sensors.hpp"
#include "hb_contact.hpp"
#include "hb_ground.hpp"

namespace hb {

// The plant's ground a scan samples (picked on the host: hb_forms.hpp scan_ground), the template argument GROUND of the routines below.
constexpr int SCAN_NONE = 0, SCAN_PLANE = 1, SCAN_PROFILE = 2, SCAN_FIELD = 3;
constexpr int HS_BLOCKS = GroundField::nz / 4;            // blocks per channel: block k = the normals, HS_BLOCKS + k = the uniforms of nodes 4 k .. 4 k + 3
constexpr double HS_INDEX_MAX = 1073741824.0;             // 2^30: bound on |a . e / du| and |b . e / dw| ahead of the conversion to int
static_assert(GroundField::nz % 4 == 0 && GroundField::pitch % 4 == 0, "a Philox block covers four nodes of one row");

HB_HD bool scan_finite(double x) { return x >= -EP_DBL_MAX && x <= EP_DBL_MAX; }

// null: valid; else the text that names what a configuration is refused for
inline const char* height_scan_config_refusal(const hb_height_scan_config& K) {
  for (int k = 0; k < 2; ++k)
    if (K.n_nodes[k] < 2 || K.n_nodes[k] > HB_FIELD_MAX_NODES) return "n_nodes must be in 2 .. HB_FIELD_MAX_NODES";
  for (int k = 0; k < 2; ++k)
    if (K.back[k] < 0 || K.back[k] > K.n_nodes[k] - 2) return "back must be in 0 .. n_nodes - 2";
  if (!scan_finite(K.dir[0]) || !scan_finite(K.dir[1])) return "dir must be finite";
  {
    const double len = sqrt(K.dir[0] * K.dir[0] + K.dir[1] * K.dir[1]);
    if (!(len > 0.0) || !scan_finite(len)) return "dir must have a length above zero";
  }
  for (int k = 0; k < 2; ++k)
    if (!(K.spacing[k] > 0.0) || !scan_finite(K.spacing[k])) return "spacing must be finite and > 0";
  if (!(K.range >= 0.0) || !scan_finite(K.range)) return "range must be finite and >= 0";
  if (!(K.noise >= 0.0) || !scan_finite(K.noise)) return "noise must be finite and >= 0";
  if (!(K.dropout >= 0.0 && K.dropout < 1.0)) return "dropout must be in [0, 1)";
  if (K.register_mode < 0 || K.register_mode > 1) return "register_mode must be 0 or 1";
  if (K.reserved != 0 || K.pad != 0) return "`reserved` and `pad` must be 0";
  return nullptr;
}
inline bool height_scan_config_valid(const hb_height_scan_config& K) { return height_scan_config_refusal(K) == nullptr; }

// Steps 1 and 2: the lattice index k[2] of grid node (0, 0) and the origin org[2] of the grid registered at e[3], for the true base
// position p[3]; a is the stored unit direction.  false: the scan of this instance is skipped (a non-finite position, or an index the
// conversion to int must not see), nothing is written.
HB_HD bool scan_origin(const hb_height_scan_config& K, const double* p, const double* e, int* k, double* org) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int c = 0; c < 3; ++c)
    if (!scan_finite(p[c]) || !scan_finite(e[c])) return false;
  const double ax = K.dir[0], ay = K.dir[1], bx = -ay, by = ax;
  const double su = (ax * e[0] + ay * e[1]) / K.spacing[0];
  const double sw = (bx * e[0] + by * e[1]) / K.spacing[1];
  if (!(fabs(su) < HS_INDEX_MAX) || !(fabs(sw) < HS_INDEX_MAX)) return false;
  k[0] = int(floor(su)) - K.back[0];
  k[1] = int(floor(sw)) - K.back[1];
  org[0] = double(k[0]) * K.spacing[0];
  org[1] = double(k[1]) * K.spacing[1];
  return true;
}

// The height of the plane n . x = d over the horizontal point s[2].
HB_HD double scan_plane_z(const double* n, double d, const double* s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return ((d - n[0] * s[0]) - n[1] * s[1]) / n[2];
}

// Step 4 without a field: the plane (n[3], *d) the plant would put a contact point at s[2] on.  gnd: nothing (SCAN_NONE), the instance's
// Terrain record (SCAN_PLANE) or its stored Profile record (SCAN_PROFILE).
template <int GROUND>
HB_HD void scan_truth(const double* gnd, double ground_z, const double* s, double* n, double* d) {
  static_assert(GROUND != SCAN_FIELD, "a field is read from its heights: scan_field_z");
  if constexpr (GROUND == SCAN_NONE) {
    n[0] = 0.0; n[1] = 0.0; n[2] = 1.0;
    *d = ground_z;
  } else {
    const double x[3] = {s[0], s[1], 0.0};
    const double* r = gnd;
    if constexpr (GROUND == SCAN_PROFILE) r = gnd + Profile::seg + Profile::rec * profile_segment(gnd, x);
    n[0] = r[Terrain::T + 2]; n[1] = r[Terrain::T + 5]; n[2] = r[Terrain::T + 8];
    *d = r[Terrain::d];
  }
}
// Step 4 over a field (fld: the stored Field record, fz: its heights): the height over s[2] of the facet the plant would put a contact point
// at s on.  field_cell cuts the cell for field_facet and for this, and the facet's plane is read from the heights of its cell as
// ground_field_height reads a map's: no unit normal lies between the stored heights and the scanned one, so a sample point on a node of the
// field returns that node's height bit for bit.  (The record of field_facet holds the same plane to the rounding of its unit normal and its
// offset; its steepness never enters.)
static_assert(Field::pitch == GroundField::pitch, "the plant's field and the field map store their heights with one pitch");
HB_HD double scan_field_z(const double* fld, const double* __restrict__ fz, const double* s) {
  return ground_field_height(fld + Field::dir, fz, s[0], s[1]);
}

// The pose a scan runs under (wave-uniform): the true base position p, the registration point e, the grid origin.
struct ScanPose {
  double p[3], e[3], org[2];
};

// Steps 3 to 6 of node (iu, iw) inside the grid: *ret = whether it has a return, and then the height the map stores.  zn: the node's
// normal (read only with noise > 0), un: its uniform (read only with dropout > 0).
template <int GROUND>
HB_HD double scan_node(const hb_height_scan_config& K, const ScanPose& P, const double* gnd, const double* __restrict__ fz, double ground_z, int iu,
                       int iw, double zn, double un, bool* ret) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double ax = K.dir[0], ay = K.dir[1], bx = -ay, by = ax;
  const double um = P.org[0] + double(iu) * K.spacing[0], wm = P.org[1] + double(iw) * K.spacing[1];
  const double m[2] = {ax * um + bx * wm, ay * um + by * wm};
  double s[2] = {m[0], m[1]};
  if (K.register_mode == 1) {
    s[0] = (m[0] - P.e[0]) + P.p[0];
    s[1] = (m[1] - P.e[1]) + P.p[1];
  }
  double zs;
  if constexpr (GROUND == SCAN_FIELD) {
    zs = scan_field_z(gnd, fz, s);
  } else {
    double n[3], d;
    scan_truth<GROUND>(gnd, ground_z, s, n, &d);
    zs = scan_plane_z(n, d, s);
  }
  const double h = K.register_mode == 1 ? ((zs - P.p[2]) + P.e[2]) - ground_z : zs - ground_z;
  const double dx = s[0] - P.p[0], dy = s[1] - P.p[1];
  const bool in_range = K.range == 0.0 || dx * dx + dy * dy <= K.range * K.range;
  const bool kept = K.dropout == 0.0 || un >= K.dropout;
  *ret = in_range && kept;
  return K.noise == 0.0 ? 0.0 + h : 0.0 + (h + K.noise * zn);
}

// The arrays of one instance.  itot: its respawn totals, or null without a respawn configuration in force.
struct ScanIo {
  const double* q;     // plant state [16]
  const double* rbd;   // resident observation [HB_NRBD]
  const int* itot;
  const double* gnd;   // the plant's ground record (by GROUND), fz: the heights of its field
  const double* fz;
  double* hdr;         // the map: header [GroundField::size], heights [GroundField::nz]
  double* z;
  int* k;              // ScanBatch: [2]
  int* episode_seen;
  int* n_returns;
  unsigned char* returned;   // [GroundField::nz]
};

// One scan of one instance (steps 1 to 9).  Blocks cx.lane, cx.lane + cx.nlanes, ... of each channel, four consecutive nodes each, so a
// pass of a wavefront stores one contiguous run of heights.  old[GroundField::nz] and cnt[cx.nlanes] are staging shared by the lanes
// (LDS on the device): every old height of the instance is staged before any is written.  episode_seen < 0: the map is cleared.
template <int GROUND, class Ctx>
HB_HD void scan_instance(const Ctx& cx, const hb_height_scan_config& K, uint32_t instance, uint32_t count, double ground_z, const ScanIo& io,
                         double* old, int* cnt) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  ScanPose P;
  for (int c = 0; c < 3; ++c) {
    P.p[c] = io.q[c];
    P.e[c] = K.register_mode == 1 ? io.rbd[3 + c] : io.q[c];
  }
  int k[2];
  if (!scan_origin(K, P.p, P.e, k, P.org)) {   // (wave-uniform: every lane leaves)
    if (cx.lane == 0) *io.n_returns = -1;
    return;
  }
  const int seen = *io.episode_seen, episode = io.itot ? io.itot[HB_RS_I_EPISODE_INDEX] : 0;
  const bool clear = seen < 0 || (io.itot && episode != seen);
  const long long su = (long long)k[0] - (long long)io.k[0], sw = (long long)k[1] - (long long)io.k[1];
  const int nu = K.n_nodes[0], nw = K.n_nodes[1];
  for (int n = cx.lane; n < GroundField::nz; n += cx.nlanes) old[n] = clear ? 0.0 : io.z[n];
  cx.sync();
  const uint32_t k0 = uint32_t(K.seed), k1 = uint32_t(K.seed >> 32);
  int returns = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int blk = cx.lane; blk < HS_BLOCKS; blk += cx.nlanes) {
    double z0 = 0.0, z1 = 0.0, z2 = 0.0, z3 = 0.0, u0 = 1.0, u1 = 1.0, u2 = 1.0, u3 = 1.0;
    if (K.noise > 0.0) {
      const Philox4 w = philox4x32_10(instance, count, HB_HS_STREAM, uint32_t(blk), k0, k1);
      box_muller(w.w[0], w.w[1], z0, z1);
      box_muller(w.w[2], w.w[3], z2, z3);
    }
    if (K.dropout > 0.0) {
      const Philox4 w = philox4x32_10(instance, count, HB_HS_STREAM, uint32_t(HS_BLOCKS + blk), k0, k1);
      u0 = (double(w.w[0]) + 0.5) * 2.3283064365386963e-10;  // 2^-32
      u1 = (double(w.w[1]) + 0.5) * 2.3283064365386963e-10;
      u2 = (double(w.w[2]) + 0.5) * 2.3283064365386963e-10;
      u3 = (double(w.w[3]) + 0.5) * 2.3283064365386963e-10;
    }
    const int iu = (4 * blk) / GroundField::pitch, iw = (4 * blk) % GroundField::pitch;
    // one node: outside the grid 0; with a return the scanned height; else what the map held at that lattice node
    const auto node = [&](int jw, double zn, double un, unsigned char* flag) -> double {
      *flag = 0;
      if (!(iu < nu && jw < nw)) return 0.0;
      bool ret;
      const double h = scan_node<GROUND>(K, P, io.gnd, io.fz, ground_z, iu, jw, zn, un, &ret);
      if (ret) {
        *flag = 1;
        ++returns;
        return h;
      }
      const long long ou = (long long)iu + su, ow = (long long)jw + sw;
      if (ou < 0 || ou >= nu || ow < 0 || ow >= nw) return 0.0;
      return old[int(ou) * GroundField::pitch + int(ow)];
    };
    unsigned char f0, f1, f2, f3;
    const double h0 = node(iw + 0, z0, u0, &f0);
    const double h1 = node(iw + 1, z1, u1, &f1);
    const double h2 = node(iw + 2, z2, u2, &f2);
    const double h3 = node(iw + 3, z3, u3, &f3);
    double* o = io.z + 4 * blk;
    o[0] = h0; o[1] = h1; o[2] = h2; o[3] = h3;
    unsigned char* r = io.returned + 4 * blk;
    r[0] = f0; r[1] = f1; r[2] = f2; r[3] = f3;
  }
  cnt[cx.lane] = returns;
  cx.sync();
  if (cx.lane == 0) {
    int total = 0;
    for (int l = 0; l < cx.nlanes; ++l) total += cnt[l];
    *io.n_returns = total;
    io.k[0] = k[0];
    io.k[1] = k[1];
    *io.episode_seen = episode;
    ground_field_compose(K.n_nodes, K.dir, P.org, K.spacing, io.hdr);
  }
}

}  // namespace hb
