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

// What a step leaves behind per instance (global memory; hb_plant_get_contact).
struct ContactOut {
  double *gap, *pvel, *res;
  int *touching, *status;
};

// One substep of length h.  q[16], v[16] in / out (LDS); imp[12] (LDS behind `lds`) in / out; wrench[6] = world force and world moment at
// the base origin, or null; all_on[4] = {1, 1, 1, 1} in memory every lane can read.  TERRAIN: ter = the instance's Terrain record (LDS); W, c,
// the impulses and the gap are those of the plane's frame, and K.mu / K.ground_z are not read.
template <bool TERRAIN = false, class Ctx>
HB_HD void contact_substep(const Ctx& cx, const DevModel& Mdl, double* q, double* v, const double* tau, const double* wrench, const int* all_on,
                           const hb_contact_config& K, double eps, double h, double* lds, double* vdot_out, const double* ter = nullptr) {
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
  if constexpr (TERRAIN) {
    terrain_rotate<PlantLds::xs>(cx, ter + Terrain::T, Jc, X, A, feet);
    ground_z = ter[Terrain::d];
  } else {
    ground_z = K.ground_z;
  }
  double tr = 0.0;
  for (int i = 0; i < 12; ++i) tr += A[i * 13];
  const double reg = eps * tr, mu = K.mu;
  double mup[HB_NC];
  point_mu<TERRAIN>(ter, mu, mup);
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
        const double phi = feet[r] - ground_z;
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
// fall test are measured along n.
template <bool HYBRID = false, bool TERRAIN = false, class Ctx>
HB_HD void contact_step(const Ctx& cx, const DevModel& Mdl, double* q_g, double* v_g, double* imp_g, const double* tau, const double* wrench,
                        const int* all_on, const hb_contact_config& K, double eps, double dt, int substeps, double* lds, double* lambda_out,
                        double* vdot_out, const ContactOut& out, const HybridActuator* actuator = nullptr, const double* ter = nullptr) {
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
      contact_substep<TERRAIN>(cx, Mdl, q, v, act.tau, wrench, all_on, K, eps, h, lds, vdot_out, ter);
    }
    actuator_finish(cx, act, substeps, acc, false);
  } else {
    for (int s = 0; s < substeps; ++s) contact_substep<TERRAIN>(cx, Mdl, q, v, tau, wrench, all_on, K, eps, h, lds, vdot_out, ter);
  }
  // ---- outputs: world forces, touching flags and point velocities J v+ of the last substep; gaps at q+
  const double* Jc = lds + PlantLds::Jc;
  double* feet = lds + PlantLds::feet;
  if (cx.lane == 0) plant_feet(Mdl, q, feet);
  for (int i = cx.lane; i < 16; i += cx.nlanes) { q_g[i] = q[i]; v_g[i] = v[i]; }
  for (int i = cx.lane; i < 12; i += cx.nlanes) {
    imp_g[i] = imp[i];
    if constexpr (TERRAIN) {
      contact_outputs_terrain(ter, i, Jc, v, imp, h, lambda_out, out.pvel);
    } else {
      lambda_out[i] = imp[i] / h;
      double s = 0.0;
      for (int k = 0; k < 16; ++k) s += Jc[i * 16 + k] * v[k];
      out.pvel[i] = s;
    }
  }
  cx.sync();
  for (int c = cx.lane; c < HB_NC; c += cx.nlanes) {
    if constexpr (TERRAIN) out.gap[c] = terrain_height(ter, feet + 3 * c);
    else out.gap[c] = feet[3 * c + 2] - K.ground_z;
    out.touching[c] = imp[3 * c + 2] > 0.0 ? 1 : 0;
  }
  if (cx.lane == 0) {
    const double res = lds[ContactLds::res];
    bool finite = true;
    for (int i = 0; i < 16; ++i) finite = finite && fabs(q[i]) <= 1.7976931348623157e308 && fabs(v[i]) <= 1.7976931348623157e308;
    int st = out.status[0] & HB_CONTACT_FALLEN;   // (latched until hb_plant_reset)
    if (!finite) st |= HB_CONTACT_NONFINITE;
    double height;
    if constexpr (TERRAIN) height = terrain_height(ter, q);
    else height = q[2] - K.ground_z;
    if (K.fall_height > 0.0 && height < K.fall_height) st |= HB_CONTACT_FALLEN;
    if (!(res <= K.tol)) st |= HB_CONTACT_UNCONVERGED;
    out.res[0] = res;
    out.status[0] = st;
  }
  cx.sync();
}

}  // namespace hb
