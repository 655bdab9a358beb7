// Plant with unilateral frictional ground contact (contact model 1 of include/hunter_hip.h, "ground"), one 64-lane workgroup per robot.
// A velocity-level time stepper: per substep the rigid-body terms, the Cholesky factor of M, M^-1 [rhs | J'] and J M^-1 J' are the front
// half of the pinned stub's substep with every contact point switched on (hb_plant.hpp plant_substep<1>); the contact impulses then come
// from projected Gauss-Seidel sweeps over the four points (normal first, then the tangential pair projected onto the friction disc),
// warm-started from the previous substep.  Contact is decided by geometry (the gap to the plane z = ground_z), never by the schedule.
//
// The sweep is lane-cooperative on the device: lane r < 12 keeps row r of W, g_r and p_r in registers; a point's three (g, p) pairs
// reach every lane by cross-lane reads, every lane computes the point's update redundantly and applies its own three
// g_r += W[r][j] dp_j.  No LDS traffic and no barrier inside a sweep.  The host build (one emulated lane) runs the same update
// routines (pgs_normal / pgs_tangent) over arrays.
#pragma once
#include <cmath>
#include <cstring>
#include "../../include/hunter_hip.h"
#include "hb_plant.hpp"

namespace hb {

struct ContactLds {
  static constexpr int q = PlantLds::total;   // 16
  static constexpr int v = q + 16;            // 16
  static constexpr int wgen = v + 16;         // 16 : generalised force of the external base wrench
  static constexpr int imp = wgen + 16;       // 12 : impulses (warm start, then the substep's result)
  static constexpr int res = imp + 12;        // 1  : residual of the last sweep
  static constexpr int total = res + 2;
};
constexpr int CONTACT_LDS_TOTAL = ContactLds::total;
constexpr int HB_CONTACT_SWEEPS_MAX = 10000;   // (a runtime loop count that comes from the caller is range-checked)

inline bool contact_config_valid(const hb_contact_config& K) {
  if (K.reserved[0] != 0 || K.reserved[1] != 0 || K.mode < 0 || K.mode > 1) return false;
  if (K.mode == 0) return true;
  const double big = 1.7976931348623157e308;
  return K.sweeps >= 1 && K.sweeps <= HB_CONTACT_SWEEPS_MAX && K.mu >= 0.0 && K.mu <= big && K.ground_z >= -big && K.ground_z <= big && K.erp >= 0.0 &&
         K.erp <= 1.0 && K.tol >= 0.0 && K.tol <= big && K.fall_height >= 0.0 && K.fall_height <= big;
}

// Normal update of a point: p_n <- max(0, p_n - g_n / W_nn).
HB_HD double pgs_normal(double gn, double pn, double Wnn) { return fmax(0.0, pn - gn / Wnn); }
// Tangential update of a point: both entries from the g of before either changes, then projected onto the disc of radius mu p_n.
HB_HD void pgs_tangent(double ga, double gb, double pa, double pb, double Waa, double Wbb, double mu, double pn, double& ta, double& tb) {
  ta = pa - ga / Waa;
  tb = pb - gb / Wbb;
  const double lim = mu * pn, nrm = sqrt(ta * ta + tb * tb);
  if (nrm > lim) {
    const double sc = pn > 0.0 ? lim / nrm : 0.0;
    ta *= sc;
    tb *= sc;
  }
}

// ---- per-instance terrain (hb_plant_set_terrain): an inclined plane n . x = d and a friction coefficient per contact point ---------------
// The record of an instance, staged in LDS behind the form's own arrays by the terrain kernels: T = [t1 t2 n] row-major (T[3 a + k] =
// world component a of frame axis k), d, mu of the four points.  Uniform over the wavefront.
struct Terrain {
  static constexpr int T = 0, d = 9, mu = 10, size = 14;
};
constexpr int TER_LDS = Terrain::size;
// The frame of a unit normal n: t1 = (e_x - n_x n) / |e_x - n_x n|, t2 = n x t1, T = [t1 t2 n] row-major; the identity exactly for n = e_z.
// Every product, sum and quotient is rounded on its own, so the host setter and the device (k_plant_scenario) store the same bits.
HB_HD void terrain_frame(const double n[3], double* T) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double t1[3] = {1.0 - n[0] * n[0], -n[0] * n[1], -n[0] * n[2]};
  const double l = sqrt(t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2]);
  for (int a = 0; a < 3; ++a) t1[a] /= l;
  const double t2[3] = {n[1] * t1[2] - n[2] * t1[1], n[2] * t1[0] - n[0] * t1[2], n[0] * t1[1] - n[1] * t1[0]};
  for (int a = 0; a < 3; ++a) { T[3 * a] = t1[a]; T[3 * a + 1] = t2[a]; T[3 * a + 2] = n[a]; }
}
// |pl[0:3]| of a plane (n, d), summed x, y, z
HB_HD double terrain_normal_length(const double* pl) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return sqrt(pl[0] * pl[0] + pl[1] * pl[1] + pl[2] * pl[2]);
}
// T and d of the record r[Terrain::size] of the plane pl[4] = (n, d), len = terrain_normal_length(pl): n is normalised before it is stored.
// The four friction coefficients are the caller's.
HB_HD void terrain_plane_record(const double* pl, double len, double* r) {
  double n[3];
  for (int a = 0; a < 3; ++a) n[a] = pl[a] / len;
  terrain_frame(n, r + Terrain::T);
  r[Terrain::d] = pl[3];
}
// (x, y, z) <- T' (x, y, z): world components to (t1, t2, n) components, every sum over the world axes in the order x, y, z.  T = I returns
// the operand.
HB_HD void terrain_to_frame(const double* T, double& x, double& y, double& z) {
  const double a = T[0] * x + T[3] * y + T[6] * z, b = T[1] * x + T[4] * y + T[7] * z, c = T[2] * x + T[5] * y + T[8] * z;
  x = a;
  y = b;
  z = c;
}
// world component a of T p, p[3] in (t1, t2, n)
HB_HD double terrain_to_world(const double* T, int a, const double* p) { return T[3 * a] * p[0] + T[3 * a + 1] * p[1] + T[3 * a + 2] * p[2]; }
// After the front half of a substep: Jc <- blockdiag(T') Jc, the contact columns of X <- X blockdiag(T), A <- blockdiag(T') A blockdiag(T)
// (block rows, then block columns) and feet_c <- T' feet_c, in place in LDS, every triple by one lane.  Behind it feet[3 c + 2] = n . x_c,
// so that the gap of point c is feet[3 c + 2] - d.  XS: columns of X.
template <int XS, class Ctx>
HB_HD void terrain_rotate(const Ctx& cx, const double* T, double* Jc, double* X, double* A, double* feet) {
  for (int e = cx.lane; e < 64; e += cx.nlanes) {
    const int c = e >> 4, k = e & 15;
    double* r = Jc + 48 * c + k;
    terrain_to_frame(T, r[0], r[16], r[32]);
    double* x = X + k * XS + 1 + 3 * c;
    terrain_to_frame(T, x[0], x[1], x[2]);
  }
  for (int e = cx.lane; e < 48; e += cx.nlanes) {
    const int c = e / 12, j = e - 12 * c;
    double* a = A + 36 * c + j;
    terrain_to_frame(T, a[0], a[12], a[24]);
  }
  for (int c = cx.lane; c < HB_NC; c += cx.nlanes) terrain_to_frame(T, feet[3 * c], feet[3 * c + 1], feet[3 * c + 2]);
  cx.sync();
  for (int e = cx.lane; e < 48; e += cx.nlanes) {
    double* a = A + 3 * e;   // row e / 4, block column e % 4
    terrain_to_frame(T, a[0], a[1], a[2]);
  }
  cx.sync();
}
// n . x - d of a world point x[3]
HB_HD double terrain_height(const double* ter, const double* x) {
  const double* T = ter + Terrain::T;
  return (T[2] * x[0] + T[5] * x[1] + T[8] * x[2]) - ter[Terrain::d];
}
// Outputs of row i = 3 c + a of a step on a terrain: the world force (T p_c)_a / h and the world velocity (T (J~ v)_c)_a of point c; Jc holds
// J~ of the last substep, imp[12] its impulses in (t1, t2, n).
HB_HD void contact_outputs_terrain(const double* ter, int i, const double* Jc, const double* v, const double* imp, double h, double* lambda_out,
                                   double* pvel) {
  const int c = i / 3, a = i - 3 * c;
  double s[3];
  for (int m = 0; m < 3; ++m) {
    s[m] = 0.0;
    for (int k = 0; k < 16; ++k) s[m] += Jc[(3 * c + m) * 16 + k] * v[k];
  }
  lambda_out[i] = terrain_to_world(ter + Terrain::T, a, imp + 3 * c) / h;
  pvel[i] = terrain_to_world(ter + Terrain::T, a, s);
}
// The friction coefficient of each point for the sweep: the context's, or with a terrain the point's own (device: out of lane 0 into
// scalar registers; nothing is loaded inside a sweep).
template <bool TERRAIN>
HB_HD void point_mu(const double* ter, double mu, double* mup) {
  for (int c = 0; c < HB_NC; ++c) {
    if constexpr (TERRAIN) {
#if defined(__HIP_DEVICE_COMPILE__)
      mup[c] = wave_bcast_f64(ter[Terrain::mu + c], 0);
#else
      mup[c] = ter[Terrain::mu + c];
#endif
    } else {
      mup[c] = mu;
    }
  }
}

// ---- per-instance terrain profile (hb_plant_set_terrain_profile): piecewise-planar ground, a facet per contact point and substep ---------
// The record of an instance.  [0, stored) is what the host stores per instance and the profile kernels stage once per step in LDS behind the
// form's own arrays; the rest is working storage of the step.  head: a Terrain record — T, d of the facet under the base origin at q+
// (written by the outputs) and mu of the four points; dir: a; nseg: K - 1 as a double; brk[k] = s_k (k = 1 .. nseg - 1 are scanned);
// seg[j] = (T_j row-major, d_j), the first ten entries of the Terrain record of the plane; act[c]: the record of the segment under point c
// in this substep; sel: the segment under the four points and the base origin at q+ (as doubles).
struct Profile {
  static constexpr int rec = 10;
  static constexpr int head = 0, dir = Terrain::size, nseg = dir + 2, brk = nseg + 1, seg = brk + HB_PROFILE_MAX_KNOTS,
                       stored = seg + rec * (HB_PROFILE_MAX_KNOTS - 1), act = stored, sel = act + rec * HB_NC, size = sel + HB_NC + 1;
};
constexpr int PRO_LDS = Profile::size;
// What a profile step leaves behind per instance besides ContactOut: seg[5] and the Terrain record of the facet under the base (base[14]:
// what k_plant_episode measures height and tilt against); pro: the staged record (LDS).
struct ProfileIo {
  double* pro;
  int* seg;
  double* base;
};
// One lane that owns every element: what the host runs the lane-cooperative composers below with.
struct OneLane {
  int lane = 0, nlanes = 1;
  HB_HD void sync() const {}
};
// a[2] = dir / |dir|: the division every stored direction goes through once (profile_record, ground_record, hb_plant_set_profile_draw).
HB_HD void profile_direction(const double* dir, double* a) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double len = sqrt(dir[0] * dir[0] + dir[1] * dir[1]);
  a[0] = dir[0] / len;
  a[1] = dir[1] / len;
}
// The record rec[Profile::rec] = (T_j, d_j) of segment j of valid knots along the unit direction a.  It comes from terrain_plane_record,
// the routine behind hb_plant_set_terrain: the plane handed to it is the unit normal and d of the segment.  Every operation is rounded on
// its own, so the host setter and the device (k_plant_profile_draw) store the same bits.
HB_HD void profile_segment_record(const double* a, const double* knots, int j, double* rec) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double ds = knots[2 * j + 2] - knots[2 * j];
  const double m = (knots[2 * j + 3] - knots[2 * j + 1]) / ds;
  const double w = sqrt(1.0 + m * m);
  double pl[4] = {0.0 - m * a[0] / w, 0.0 - m * a[1] / w, 1.0 / w, 0.0};   // (0 - : no negative zero on level ground)
  // (normalised until its length rounds to 1, so that hb_plant_set_terrain, which divides by the length once more, stores the same bits)
  for (int it = 0; it < 4 && terrain_normal_length(pl) != 1.0; ++it) {
    const double l = terrain_normal_length(pl);
    for (int x = 0; x < 3; ++x) pl[x] /= l;
  }
  pl[3] = pl[0] * (a[0] * knots[2 * j]) + pl[1] * (a[1] * knots[2 * j]) + pl[2] * knots[2 * j + 1];
  terrain_plane_record(pl, terrain_normal_length(pl), rec);   // (writes T and d: the Profile::rec leading entries of a Terrain record)
}
static_assert(Terrain::d + 1 == Profile::rec, "a segment record is T and d of a Terrain record");
// The stored record r[Profile::stored] of VALID knots (K of them, (s, z), along the unit direction a) and the friction coefficients mu[4]:
// what profile_record composes once it has accepted them, and what k_plant_profile_draw composes for a drawn profile, one segment per lane.
// knots, a, mu and r may be LDS or plain memory; r is written whole.
template <class Ctx>
HB_HD void profile_compose(const Ctx& cx, int K, const double* a, const double* knots, const double* mu, double* r) {
  for (int k = cx.lane; k < Profile::stored; k += cx.nlanes) r[k] = 0.0;
  cx.sync();
  for (int k = cx.lane; k < K; k += cx.nlanes) r[Profile::brk + k] = knots[2 * k];
  for (int j = cx.lane; j + 1 < K; j += cx.nlanes) profile_segment_record(a, knots, j, r + Profile::seg + Profile::rec * j);
  for (int c = cx.lane; c < HB_NC; c += cx.nlanes) r[Profile::head + Terrain::mu + c] = mu[c];
  if (cx.lane == 0) {
    r[Profile::dir] = a[0];
    r[Profile::dir + 1] = a[1];
    r[Profile::nseg] = double(K - 1);
  }
  cx.sync();
  for (int k = cx.lane; k < Profile::rec; k += cx.nlanes) r[Profile::head + k] = r[Profile::seg + k];   // (until a state is located: segment 0)
  cx.sync();
}
// Host: the stored record r[Profile::stored] of one instance from its profile (K knots (s, z), direction, mu[4] or null for cfg_mu), or the
// reason it is refused (r is then not written).  The validation; the record of what it accepts is profile_compose's.
inline const char* profile_record(int K, const double* dir, const double* knots, const double* mu, double cfg_mu, double* r) {
  if (K < 2 || K > HB_PROFILE_MAX_KNOTS) return "a number of knots outside 2 .. HB_PROFILE_MAX_KNOTS";
  if (!(std::isfinite(dir[0]) && std::isfinite(dir[1]))) return "a non-finite direction";
  const double len = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1]);
  if (!(len > 0.0) || !std::isfinite(len)) return "a direction of length zero";
  for (int k = 0; k < 2 * K; ++k)
    if (!std::isfinite(knots[k])) return "a non-finite knot";
  for (int j = 0; j + 1 < K; ++j) {
    const double ds = knots[2 * j + 2] - knots[2 * j];
    if (!(ds > 0.0)) return "knots whose s is not strictly increasing";
    const double m = (knots[2 * j + 3] - knots[2 * j + 1]) / ds;
    // (sqrt(3) to rounding: a riser given by its height and width)
    if (!(std::isfinite(m) && m * m <= 3.0 * (1.0 + 1e-12))) return "a segment steeper than sqrt(3) (n_z < 0.5)";
  }
  double mu4[HB_NC];
  for (int c = 0; c < HB_NC; ++c) {
    mu4[c] = mu ? mu[c] : cfg_mu;
    if (!(std::isfinite(mu4[c]) && mu4[c] >= 0.0)) return "a friction coefficient that is negative or not finite";
  }
  double a[2];
  profile_direction(dir, a);
  profile_compose(OneLane{}, K, a, knots, mu4, r);
  return nullptr;
}

// The segment under the world point x[3]: the last j with s_j <= a . x, the end segments open-ended.  A scan over the breakpoints.
HB_HD int profile_segment(const double* pro, const double* x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double s = pro[Profile::dir] * x[0] + pro[Profile::dir + 1] * x[1];
  const int nseg = int(pro[Profile::nseg]);
  int j = 0;
  for (int k = 1; k < nseg; ++k) j = s >= pro[Profile::brk + k] ? k : j;
  return j;
}
// Point c copies the record of the segment under feet[3 c ..] into its slot of act, one lane per point.
template <class Ctx>
HB_HD void profile_select(const Ctx& cx, double* pro, const double* feet) {
  for (int c = cx.lane; c < HB_NC; c += cx.nlanes) {
    const double* src = pro + Profile::seg + Profile::rec * profile_segment(pro, feet + 3 * c);
    double* dst = pro + Profile::act + Profile::rec * c;
    for (int k = 0; k < Profile::rec; ++k) dst[k] = src[k];
  }
  cx.sync();
}
// terrain_rotate with the frame of each point: Jc <- blockdiag(T_c') Jc, the contact columns of X take their point's frame, block (c, c') of
// A <- T_c' A_cc' T_c' (block rows, then block columns), feet_c <- T_c' feet_c.  act: the four active records.
template <int XS, class Ctx>
HB_HD void profile_rotate(const Ctx& cx, const double* act, double* Jc, double* X, double* A, double* feet) {
  for (int e = cx.lane; e < 64; e += cx.nlanes) {
    const int c = e >> 4, k = e & 15;
    const double* T = act + Profile::rec * c;
    double* r = Jc + 48 * c + k;
    terrain_to_frame(T, r[0], r[16], r[32]);
    double* x = X + k * XS + 1 + 3 * c;
    terrain_to_frame(T, x[0], x[1], x[2]);
  }
  for (int e = cx.lane; e < 48; e += cx.nlanes) {
    const int c = e / 12, j = e - 12 * c;
    double* a = A + 36 * c + j;
    terrain_to_frame(act + Profile::rec * c, a[0], a[12], a[24]);
  }
  for (int c = cx.lane; c < HB_NC; c += cx.nlanes) terrain_to_frame(act + Profile::rec * c, feet[3 * c], feet[3 * c + 1], feet[3 * c + 2]);
  cx.sync();
  for (int e = cx.lane; e < 48; e += cx.nlanes) {
    double* a = A + 3 * e;   // row e / 4, block column e % 4
    terrain_to_frame(act + Profile::rec * (e & 3), a[0], a[1], a[2]);
  }
  cx.sync();
}
// d of the facet the normal row r = 3 c + 2 measures its gap from (TERRAIN 2 and 3), else the caller's
template <int TERRAIN>
HB_HD double row_ground(const double* ter, int r, double ground_z) {
  if constexpr (TERRAIN >= 2) return ter[Profile::act + Profile::rec * (r / 3) + Terrain::d];
  else return ground_z;
}
// The outputs of a profile step at q+ (feet[12] world, q[16]): the segment under the four points and the base origin is selected again, the
// points' records go to act (gap_c), the base's to head (the fall test, ProfileIo::base).  One lane per point and one for the base.
template <class Ctx>
HB_HD void profile_outputs_select(const Ctx& cx, double* pro, const double* feet, const double* q) {
  for (int c = cx.lane; c < HB_NC + 1; c += cx.nlanes) {
    const int j = profile_segment(pro, c < HB_NC ? feet + 3 * c : q);
    const double* src = pro + Profile::seg + Profile::rec * j;
    double* dst = c < HB_NC ? pro + Profile::act + Profile::rec * c : pro + Profile::head;
    for (int k = 0; k < Profile::rec; ++k) dst[k] = src[k];
    pro[Profile::sel + c] = double(j);
  }
  cx.sync();
}
template <class Ctx>
HB_HD void profile_publish(const Ctx& cx, const ProfileIo& io) {
  for (int c = cx.lane; c < HB_NC + 1; c += cx.nlanes) io.seg[c] = int(io.pro[Profile::sel + c]);
  for (int k = cx.lane; k < Terrain::size; k += cx.nlanes) io.base[k] = io.pro[Profile::head + k];
}

// ---- per-instance height field (hb_plant_set_terrain_field): triangulated ground over a grid, a facet per contact point and substep --------
// The record of an instance where the field kernels stage it (TERRAIN 3).  head, act and sel lie where the profile's do, so that
// profile_rotate, row_ground, profile_publish and the outputs serve both grounds; [0, stored) is what the host stores per instance: head (a
// Terrain record: T, d of the facet under the base origin at q+, mu of the four points), dir: a, org: (u0, w0), step: (du, dw), nu / nw as
// doubles.  The heights z[iu * HB_FIELD_MAX_NODES + iw] stay in global memory (FieldBatch::z); a facet's record is computed from the four
// heights of its cell where it is needed.
struct Field {
  static constexpr int head = Profile::head, dir = Profile::dir, org = dir + 2, step = org + 2, nu = step + 2, nw = nu + 1, stored = nw + 1,
                       act = Profile::act, sel = Profile::sel, size = Profile::size, pitch = HB_FIELD_MAX_NODES,
                       nz = HB_FIELD_MAX_NODES * HB_FIELD_MAX_NODES;
};
static_assert(Field::stored <= Field::act, "the stored part of a field record ends ahead of the working part");
// The cell and triangle under the world point x[0], x[1] of a grid whose header is h[8] = direction a | origin (u0, w0) | spacing (du, dw) | nu,
// nw as doubles (the eight doubles at Field::dir of a field record; the controller's field map, hb_ground.hpp, stores the same eight):
// u, w along a and b = (-a_y, a_x) from the origin, the cell (i, j) = clamp(floor(u / du), 0, nu - 2), the same for w, the fractions fu, fw
// within it (beyond the grid: below 0 or above 1, the border cell's planes continue) and t = 0 (fu >= fw: the lower triangle) or 1.
// ONE routine for the plant's facet and the map's height: they cannot cut a cell differently.
struct FieldCell {
  double ax, ay, bx, by, u0, w0, du, dw, u, w, fu, fw;
  int nw, i, j, t;
  const double* cell;   // heights of the cell: cell[0], cell[1], cell[pitch], cell[pitch + 1] = z00, z01, z10, z11
};
HB_HD FieldCell field_cell(const double* h, const double* __restrict__ z, const double* x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  FieldCell c;
  c.ax = h[0]; c.ay = h[1]; c.bx = -c.ay; c.by = c.ax;
  c.u0 = h[2]; c.w0 = h[3]; c.du = h[4]; c.dw = h[5];
  const int nu = int(h[6]);
  c.nw = int(h[7]);
  c.u = (c.ax * x[0] + c.ay * x[1]) - c.u0;
  c.w = (c.bx * x[0] + c.by * x[1]) - c.w0;
  const double su = c.u / c.du, sw = c.w / c.dw;
  // clamp(floor(s), 0, n - 2); a NaN fails every comparison and lands in cell 0
  c.i = su >= 1.0 ? (su < double(nu - 2) ? int(su) : nu - 2) : 0;
  c.j = sw >= 1.0 ? (sw < double(c.nw - 2) ? int(sw) : c.nw - 2) : 0;
  c.fu = su - double(c.i);
  c.fw = sw - double(c.j);
  c.t = c.fu < c.fw ? 1 : 0;   // (fu >= fw: the lower triangle)
  c.cell = z + c.i * HB_FIELD_MAX_NODES + c.j;
  return c;
}
static_assert(Field::org == Field::dir + 2 && Field::step == Field::dir + 4 && Field::nu == Field::dir + 6 && Field::nw == Field::dir + 7,
              "field_cell reads the header of a field record as eight consecutive doubles");
// The facet under the world point x[3] of the field (hdr: its record, z: its heights): the id 2 (i (nw - 1) + j) + t, and in
// rec[Profile::rec] the record (T, d) of its plane, which comes from terrain_plane_record as a profile segment's does.  Every operation is
// rounded on its own: host, host emulation and device return the same bits.  A NaN coordinate gives facet 0 and a NaN record.
HB_HD int field_facet(const double* hdr, const double* __restrict__ z, const double* x, double* rec) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const FieldCell fc = field_cell(hdr + Field::dir, z, x);
  const double ax = fc.ax, ay = fc.ay, bx = fc.bx, by = fc.by, u0 = fc.u0, w0 = fc.w0, du = fc.du, dw = fc.dw, u = fc.u, w = fc.w;
  const int nw = fc.nw, i = fc.i, j = fc.j, t = fc.t;
  const double* c = fc.cell;
  const double z00 = c[0], z01 = c[1], z10 = c[Field::pitch], z11 = c[Field::pitch + 1];
  const double p = (t ? z11 - z01 : z10 - z00) / du;
  const double r = (t ? z01 - z00 : z11 - z10) / dw;
  const double len = sqrt(1.0 + p * p + r * r);
  double pl[4] = {0.0 - (p * ax + r * bx) / len, 0.0 - (p * ay + r * by) / len, 1.0 / len, 0.0};   // (0 - : no negative zero on level ground)
  for (int it = 0; it < 4 && terrain_normal_length(pl) != 1.0; ++it) {   // (as profile_segment_record)
    const double l = terrain_normal_length(pl);
    for (int k = 0; k < 3; ++k) pl[k] /= l;
  }
  const double un = u0 + double(i) * du, wn = w0 + double(j) * dw;
  pl[3] = pl[0] * (ax * un + bx * wn) + pl[1] * (ay * un + by * wn) + pl[2] * z00;
  terrain_plane_record(pl, terrain_normal_length(pl), rec);
  if (u != u || w != w)
    for (int k = 0; k < Profile::rec; ++k) rec[k] = u + w;
  return 2 * (i * (nw - 1) + j) + t;
}
// The stored record r[Field::stored] of a VALID field (n[2] node counts, the unit direction a, origin, spacing, the stored heights z with
// the pitch HB_FIELD_MAX_NODES, mu[4]): what field_record composes once it has accepted them, and what k_plant_field_draw composes for a
// drawn field (one lane: the record is 22 stores and one facet).  r is written whole; its head is the facet under the world origin until
// a state is located.
HB_HD void field_compose(const int* n, const double* a, const double* org, const double* step, const double* __restrict__ z, const double* mu,
                         double* r) {
  for (int k = 0; k < Field::stored; ++k) r[k] = 0.0;
  r[Field::dir] = a[0]; r[Field::dir + 1] = a[1];
  r[Field::org] = org[0]; r[Field::org + 1] = org[1];
  r[Field::step] = step[0]; r[Field::step + 1] = step[1];
  r[Field::nu] = double(n[0]); r[Field::nw] = double(n[1]);
  for (int c = 0; c < HB_NC; ++c) r[Field::head + Terrain::mu + c] = mu[c];
  const double x0[3] = {0.0, 0.0, 0.0};
  field_facet(r, z, x0, r + Field::head);   // (until a state is located: the facet under the world origin)
}
// Host: the stored record r[Field::stored] of one instance from its field (n[2] node counts, direction, origin, spacing, heights with the
// pitch HB_FIELD_MAX_NODES, mu[4] or null for cfg_mu), or the reason it is refused (r is then not written).
inline const char* field_record(const int* n, const double* dir, const double* org, const double* step, const double* z, const double* mu,
                                double cfg_mu, double* r) {
  if (n[0] < 2 || n[0] > HB_FIELD_MAX_NODES || n[1] < 2 || n[1] > HB_FIELD_MAX_NODES) return "a number of nodes outside 2 .. HB_FIELD_MAX_NODES";
  if (!(std::isfinite(dir[0]) && std::isfinite(dir[1]))) return "a non-finite direction";
  const double len = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1]);
  if (!(len > 0.0) || !std::isfinite(len)) return "a direction of length zero";
  if (!(std::isfinite(org[0]) && std::isfinite(org[1]))) return "a non-finite origin";
  if (!(std::isfinite(step[0]) && std::isfinite(step[1]))) return "a non-finite spacing";
  if (!(step[0] > 0.0 && step[1] > 0.0)) return "a spacing that is not positive";
  for (int i = 0; i < n[0]; ++i)
    for (int j = 0; j < n[1]; ++j)
      if (!std::isfinite(z[i * Field::pitch + j])) return "a non-finite height";
  for (int i = 0; i + 1 < n[0]; ++i)
    for (int j = 0; j + 1 < n[1]; ++j) {
      const double* c = z + i * Field::pitch + j;
      const double pr[2][2] = {{(c[Field::pitch] - c[0]) / step[0], (c[Field::pitch + 1] - c[Field::pitch]) / step[1]},
                               {(c[Field::pitch + 1] - c[1]) / step[0], (c[1] - c[0]) / step[1]}};
      for (const auto& t : pr) {
        const double s2 = t[0] * t[0] + t[1] * t[1];
        if (!(std::isfinite(s2) && s2 <= 3.0 * (1.0 + 1e-12))) return "a triangle steeper than sqrt(3) (n_z < 0.5)";
      }
    }
  double mu4[HB_NC];
  for (int c = 0; c < HB_NC; ++c) {
    mu4[c] = mu ? mu[c] : cfg_mu;
    if (!(std::isfinite(mu4[c]) && mu4[c] >= 0.0)) return "a friction coefficient that is negative or not finite";
  }
  double a[2];
  profile_direction(dir, a);
  field_compose(n, a, org, step, z, mu4, r);
  return nullptr;
}
// profile_select for a field: point c takes the record of the facet under feet[3 c ..] into its slot of act, one lane per point.
template <class Ctx>
HB_HD void field_select(const Ctx& cx, double* fld, const double* __restrict__ z, const double* feet) {
  for (int c = cx.lane; c < HB_NC; c += cx.nlanes) field_facet(fld, z, feet + 3 * c, fld + Field::act + Profile::rec * c);
  cx.sync();
}
// profile_outputs_select for a field: the facets under the four points and the base origin at q+; the points' records go to act, the
// base's to head, the ids to sel.
template <class Ctx>
HB_HD void field_outputs_select(const Ctx& cx, double* fld, const double* __restrict__ z, const double* feet, const double* q) {
  for (int c = cx.lane; c < HB_NC + 1; c += cx.nlanes) {
    double rec[Profile::rec];
    const int id = field_facet(fld, z, c < HB_NC ? feet + 3 * c : q, rec);
    double* dst = c < HB_NC ? fld + Field::act + Profile::rec * c : fld + Field::head;
    for (int k = 0; k < Profile::rec; ++k) dst[k] = rec[k];
    fld[Field::sel + c] = double(id);
  }
  cx.sync();
}

// What a step leaves behind per instance (global memory; hb_plant_get_contact).
struct ContactOut {
  double *gap, *pvel, *res;
  int *touching, *status;
};

// One substep of length h.  q[16], v[16] in / out (LDS); imp[12] (LDS behind `lds`) in / out; wrench[6] = world force and world moment at
// the base origin, or null; all_on[4] = {1, 1, 1, 1} in memory every lane can read.  TERRAIN: ter = the instance's Terrain record (LDS); W, c,
// the impulses and the gap are those of the plane's frame, and K.mu / K.ground_z are not read.  TERRAIN 2: ter = the instance's staged
// Profile record (LDS, writable: ProfileIo::pro); frame and offset are those of each point's facet, selected here from the substep's start.
// TERRAIN 3: the same with ter = the instance's staged Field record and hts = its heights (global memory): the facet comes from field_facet.
template <int TERRAIN = 0, class Ctx>
HB_HD void contact_substep(const Ctx& cx, const DevModel& Mdl, double* q, double* v, const double* tau, const double* wrench, const int* all_on,
                           const hb_contact_config& K, double eps, double h, double* lds, double* vdot_out, const double* ter = nullptr,
                           const double* hts = nullptr) {
  double* Jc = lds + PlantLds::Jc;
  double* X = lds + PlantLds::X;
  double* A = lds + PlantLds::A;
  double* feet = lds + PlantLds::feet;
  double* wgen = lds + ContactLds::wgen;
  double* imp = lds + ContactLds::imp;
  if (cx.lane == 0 && wrench) {   // w = [F, E(zyx)' m, 0]: the power of the moment is m . E rates
    double sz, cz, sy, cy;
    sincos_t(q[3], sz, cz);
    sincos_t(q[4], sy, cy);
    for (int a = 0; a < 3; ++a) wgen[a] = wrench[a];
    wgen[3] = wrench[5];
    wgen[4] = -sz * wrench[3] + cz * wrench[4];
    wgen[5] = cy * cz * wrench[3] + cy * sz * wrench[4] - sy * wrench[5];
    for (int a = 6; a < 16; ++a) wgen[a] = 0.0;
  }
  // the front half of the pinned stub's substep with every point on (its first barrier publishes wgen)
  plant_substep<1>(cx, Mdl, q, v, tau, all_on, nullptr, 0.0, 0.0, h, lds, nullptr, nullptr, wrench ? wgen : nullptr);
  double ground_z;
  if constexpr (TERRAIN >= 2) {
    if constexpr (TERRAIN == 3) field_select(cx, const_cast<double*>(ter), hts, feet);
    else profile_select(cx, const_cast<double*>(ter), feet);
    profile_rotate<PlantLds::xs>(cx, ter + Profile::act, Jc, X, A, feet);
    ground_z = row_ground<TERRAIN>(ter, cx.lane < 12 ? cx.lane : 0, 0.0);   // (the lane's own row)
  } else if constexpr (TERRAIN) {
    terrain_rotate<PlantLds::xs>(cx, ter + Terrain::T, Jc, X, A, feet);
    ground_z = ter[Terrain::d];
  } else {
    ground_z = K.ground_z;
  }
  double tr = 0.0;
  for (int i = 0; i < 12; ++i) tr += A[i * 13];
  const double reg = eps * tr, mu = K.mu;
  double mup[HB_NC];
  point_mu<(TERRAIN != 0)>(ter, mu, mup);
#if defined(__HIP_DEVICE_COMPILE__)
  {
    const int r = cx.lane < 12 ? cx.lane : 0;   // (lanes 12.. shadow lane 0: nothing reads them)
    double W[12], D[12];
    for (int j = 0; j < 12; ++j) {
      W[j] = A[r * 12 + j] + (j == r ? reg : 0.0);
      D[j] = A[j * 13] + reg;
    }
    double g = 0.0;
    for (int k = 0; k < 16; ++k) g += Jc[r * 16 + k] * (v[k] + h * X[k * 13]);
    if (r % 3 == 2) {
      const double phi = feet[r] - ground_z;
      g += (fmax(phi, 0.0) + K.erp * fmin(phi, 0.0)) / h;
    }
    for (int j = 0; j < 12; ++j) g += W[j] * imp[j];
    double p = imp[r], res = 0.0;
    for (int s = 0; s < K.sweeps; ++s) {
      res = 0.0;
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) {
        const int a = 3 * pt, b = a + 1, n = a + 2;
        const double pn0 = wave_bcast_f64(p, n), pn = pgs_normal(wave_bcast_f64(g, n), pn0, D[n]), dn = pn - pn0;
        g += W[n] * dn;
        p = cx.lane == n ? pn : p;
        res = fmax(res, fabs(D[n] * dn));
        const double pa0 = wave_bcast_f64(p, a), pb0 = wave_bcast_f64(p, b);
        double ta, tb;
        pgs_tangent(wave_bcast_f64(g, a), wave_bcast_f64(g, b), pa0, pb0, D[a], D[b], mup[pt], pn, ta, tb);
        const double da = ta - pa0, db = tb - pb0;
        g += W[a] * da;
        g += W[b] * db;
        p = cx.lane == a ? ta : (cx.lane == b ? tb : p);
        res = fmax(res, fmax(fabs(D[a] * da), fabs(D[b] * db)));
      }
    }
    cx.sync();   // (every lane has read the warm start)
    if (cx.lane < 12) imp[cx.lane] = p;
    if (cx.lane == 0) lds[ContactLds::res] = res;
  }
#else
  {
    double W[144], g[12], p[12], res = 0.0;
    for (int r = 0; r < 12; ++r) {
      for (int j = 0; j < 12; ++j) W[r * 12 + j] = A[r * 12 + j] + (j == r ? reg : 0.0);
      double s = 0.0;
      for (int k = 0; k < 16; ++k) s += Jc[r * 16 + k] * (v[k] + h * X[k * 13]);
      if (r % 3 == 2) {
        const double phi = feet[r] - row_ground<TERRAIN>(ter, r, ground_z);
        s += (fmax(phi, 0.0) + K.erp * fmin(phi, 0.0)) / h;
      }
      for (int j = 0; j < 12; ++j) s += W[r * 12 + j] * imp[j];
      g[r] = s;
      p[r] = imp[r];
    }
    for (int s = 0; s < K.sweeps; ++s) {
      res = 0.0;
      for (int pt = 0; pt < 4; ++pt) {
        const int a = 3 * pt, b = a + 1, n = a + 2;
        const double pn = pgs_normal(g[n], p[n], W[n * 13]), dn = pn - p[n];
        for (int r = 0; r < 12; ++r) g[r] += W[r * 12 + n] * dn;
        p[n] = pn;
        res = fmax(res, fabs(W[n * 13] * dn));
        double ta, tb;
        pgs_tangent(g[a], g[b], p[a], p[b], W[a * 13], W[b * 13], mup[pt], pn, ta, tb);
        const double da = ta - p[a], db = tb - p[b];
        for (int r = 0; r < 12; ++r) { g[r] += W[r * 12 + a] * da; g[r] += W[r * 12 + b] * db; }
        p[a] = ta;
        p[b] = tb;
        res = fmax(res, fmax(fabs(W[a * 13] * da), fabs(W[b * 13] * db)));
      }
    }
    for (int r = 0; r < 12; ++r) imp[r] = p[r];
    lds[ContactLds::res] = res;
  }
#endif
  cx.sync();
  // ---- v+ = v_f + M^-1 J' p,  q+ = q + h v+
  for (int i = cx.lane; i < 16; i += cx.nlanes) {
    double vn = v[i] + h * X[i * 13];
    for (int j = 0; j < 12; ++j) vn += X[i * 13 + 1 + j] * imp[j];
    if (vdot_out) vdot_out[i] = (vn - v[i]) / h;
    v[i] = vn;
    q[i] = q[i] + h * vn;
  }
  cx.sync();
}

// One plant tick of one instance in contact model 1: `substeps` substeps of dt / substeps, then the outputs of the step.  State (q, v,
// impulses, status) lives in global memory and is staged in LDS behind `lds` (CONTACT_LDS_TOTAL doubles).
// TERRAIN: ter = the instance's Terrain record (LDS); lambda is T p / h, the point velocities are brought back to the world, gaps and the
// fall test are measured along n.  TERRAIN 2: pio = the instance's profile record and outputs, ter = pio->pro; lambda and the point
// velocities come back through the frames of the last substep, gaps and the fall test are measured over the facets selected at q+.
template <bool HYBRID = false, int TERRAIN = 0, class Ctx>
HB_HD void contact_step(const Ctx& cx, const DevModel& Mdl, double* q_g, double* v_g, double* imp_g, const double* tau, const double* wrench,
                        const int* all_on, const hb_contact_config& K, double eps, double dt, int substeps, double* lds, double* lambda_out,
                        double* vdot_out, const ContactOut& out, const HybridActuator* actuator = nullptr, const double* ter = nullptr,
                        const ProfileIo* pio = nullptr, const double* hts = nullptr) {
  double* q = lds + ContactLds::q;
  double* v = lds + ContactLds::v;
  double* imp = lds + ContactLds::imp;
  for (int i = cx.lane; i < 16; i += cx.nlanes) { q[i] = q_g[i]; v[i] = v_g[i]; }
  for (int i = cx.lane; i < 12; i += cx.nlanes) imp[i] = imp_g[i];
  cx.sync();
  const double h = dt / substeps;
  if constexpr (HYBRID) {   // (hb_plant.hpp: the law before every substep; `tau` is not read)
    const HybridActuator& act = *actuator;
    ActuatorAcc acc;
    for (int s = 0; s < substeps; ++s) {
      actuator_eval(cx, act, q, v, s, act.tau, acc, [](int, double ts) { return ts; });
      contact_substep<TERRAIN>(cx, Mdl, q, v, act.tau, wrench, all_on, K, eps, h, lds, vdot_out, ter, hts);
    }
    actuator_finish(cx, act, substeps, acc, false);
  } else {
    for (int s = 0; s < substeps; ++s) contact_substep<TERRAIN>(cx, Mdl, q, v, tau, wrench, all_on, K, eps, h, lds, vdot_out, ter, hts);
  }
  // ---- outputs: world forces, touching flags and point velocities J v+ of the last substep; gaps at q+
  const double* Jc = lds + PlantLds::Jc;
  double* feet = lds + PlantLds::feet;
  if (cx.lane == 0) plant_feet(Mdl, q, feet);
  for (int i = cx.lane; i < 16; i += cx.nlanes) { q_g[i] = q[i]; v_g[i] = v[i]; }
  for (int i = cx.lane; i < 12; i += cx.nlanes) {
    imp_g[i] = imp[i];
    if constexpr (TERRAIN >= 2) {
      contact_outputs_terrain(ter + Profile::act + Profile::rec * (i / 3), i, Jc, v, imp, h, lambda_out, out.pvel);
    } else if constexpr (TERRAIN) {
      contact_outputs_terrain(ter, i, Jc, v, imp, h, lambda_out, out.pvel);
    } else {
      lambda_out[i] = imp[i] / h;
      double s = 0.0;
      for (int k = 0; k < 16; ++k) s += Jc[i * 16 + k] * v[k];
      out.pvel[i] = s;
    }
  }
  cx.sync();
  if constexpr (TERRAIN == 3) field_outputs_select(cx, pio->pro, hts, feet, q);
  else if constexpr (TERRAIN == 2) profile_outputs_select(cx, pio->pro, feet, q);
  for (int c = cx.lane; c < HB_NC; c += cx.nlanes) {
    if constexpr (TERRAIN >= 2) out.gap[c] = terrain_height(ter + Profile::act + Profile::rec * c, feet + 3 * c);
    else if constexpr (TERRAIN) out.gap[c] = terrain_height(ter, feet + 3 * c);
    else out.gap[c] = feet[3 * c + 2] - K.ground_z;
    out.touching[c] = imp[3 * c + 2] > 0.0 ? 1 : 0;
  }
  if constexpr (TERRAIN >= 2) profile_publish(cx, *pio);
  if (cx.lane == 0) {
    const double res = lds[ContactLds::res];
    bool finite = true;
    for (int i = 0; i < 16; ++i) finite = finite && fabs(q[i]) <= 1.7976931348623157e308 && fabs(v[i]) <= 1.7976931348623157e308;
    int st = out.status[0] & HB_CONTACT_FALLEN;   // (latched until hb_plant_reset)
    if (!finite) st |= HB_CONTACT_NONFINITE;
    double height;
    if constexpr (TERRAIN) height = terrain_height(ter, q);   // (TERRAIN 2: the head of the record is the facet under the base)
    else height = q[2] - K.ground_z;
    if (K.fall_height > 0.0 && height < K.fall_height) st |= HB_CONTACT_FALLEN;
    if (!(res <= K.tol)) st |= HB_CONTACT_UNCONVERGED;
    out.res[0] = res;
    out.status[0] = st;
  }
  cx.sync();
}

}  // namespace hb
