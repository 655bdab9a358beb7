// Joint model of contact model 1 of the plant (include/hunter_hip.h, hb_joint_model): rotor inertia and implicit viscous damping on the
// joint diagonal of M, actuator saturation, dry friction and joint stops, one 64-lane workgroup per robot.  The substep is
// contact_substep (hb_contact.hpp) with 32 rows in the projected Gauss-Seidel problem instead of 12: rows 0-11 the contact points, row
// 12 + j the friction of joint j (Jacobian row e_{6+j}, box +-frictionloss_j h), row 22 + j its stop (Jacobian row s_j e_{6+j}, p >= 0).
// The front half is plant_substep<2> (hb_plant.hpp): X = Mh^-1 [rhs | Jc' | e_6 .. e_15], so that every entry of W = Jh Mh^-1 Jh' is an
// entry of Jc Mh^-1 Jc' (A) or of X; the stop rows are s_j times the friction rows and are never formed: a lane keeps the 22 entries of
// its row against the contact and friction columns, and a stop update dp enters g as W[r][12 + j] (s_j dp).
//
// Lane r < 32 keeps row r, g_r and p_r in registers; a row's (g, p) reaches every lane by cross-lane reads, every lane computes the
// update redundantly and applies its own g_r += W[r][k] dp_k.  No LDS traffic, no barrier and no memory instruction inside a sweep.
// The host build (one emulated lane) runs the same row set-up (joint_row) and the same update routines over arrays.
#pragma once
#include "hb_contact.hpp"

namespace hb {

struct JointLds {
  static constexpr int q = PlantJointLds::total;   // 16
  static constexpr int v = q + 16;                 // 16
  static constexpr int wgen = v + 16;              // 16 : generalised force of the base wrench and of the viscous damping
  static constexpr int imp = wgen + 16;            // 32 : impulses (contact 12 | friction 10 | stops 10, the stops as u = s p)
  static constexpr int res = imp + 32;             // 2  : contact residual, joint residual of the last sweep
  static constexpr int taua = res + 2;             // 10 : the saturated torque
  static constexpr int mdiag = taua + 10;          // 10 : armature + h damping
  static constexpr int sgn = mdiag + 10;           // 10 : side of the stop row, +-1
  static constexpr int bstop = sgn + 10;           // 10 : right-hand side of the stop row
  static constexpr int vf = bstop + 10;             // 16 : free velocity
  static constexpr int total = vf + 16;
};
constexpr int JOINT_LDS_TOTAL = JointLds::total;
constexpr int XJ = PlantJointLds::xs;   // 23

inline bool joint_model_valid(const hb_joint_model& J) {
  const double big = 1.7976931348623157e308;
  if (J.reserved != 0 || J.limits < 0 || J.limits > 1) return false;
  for (int j = 0; j < HB_NJ; ++j) {
    const bool ok = J.armature[j] >= 0.0 && J.armature[j] <= big && J.damping[j] >= 0.0 && J.damping[j] <= big && J.frictionloss[j] >= 0.0 &&
                    J.frictionloss[j] <= big && J.lower[j] >= -big && J.upper[j] <= big && J.lower[j] < J.upper[j] && J.torque_limit[j] > 0.0;
    if (!ok) return false;
  }
  return J.limit_erp >= 0.0 && J.limit_erp <= 1.0 && J.tol >= 0.0 && J.tol <= big;
}

// Friction update of a joint: p <- clamp(p - g / W_rr, -lim, +lim).   Stop update: pgs_normal.
HB_HD double pgs_box(double g, double p, double Wrr, double lim) { return fmax(-lim, fmin(lim, p - g / Wrr)); }
// tau_a = clamp(tau, -limit, +limit) (numpy's clip: minimum(maximum(tau, -limit), limit))
HB_HD double joint_saturate(double tau, double limit) { return fmin(fmax(tau, -limit), limit); }

// What a step leaves behind per instance (global memory; hb_plant_get_joints).
struct JointOut {
  double *tau_applied, *friction_torque, *limit_torque, *res;
  int* status;
};

// Row r < 32 of the problem at the start of a substep: W[22] = its entries against the contact columns 0-11 and the friction columns
// 12-21 (the stop column 22 + j is sgn[j] times column 12 + j), its diagonal, g_r = c_r + (W p)_r at the warm start, and p_r.
// A = Jc Mh^-1 Jc' (12 x 12), X (16 x 23), vf = free velocity, wp[32] = warm start (stops as p, not u), reg = eps tr(A); feet, ground_z,
// erp: the gap term of the contact normals.
HB_HD void joint_row(int r, const double* A, const double* X, const double* Jc, const double* vf, const double* feet, double ground_z,
                     double erp, double h, const double* sgn, const double* bstop, const double* wp, double reg, double* W, double& g,
                     double& p) {
  const int j = r < 12 ? 0 : (r < 22 ? r - 12 : r - 22);
  const double sr = r >= 22 ? sgn[j] : 1.0;
  const double* Xj = X + (6 + j) * XJ;
  double c;
  if (r < 12) {
    for (int k = 0; k < 12; ++k) W[k] = A[r * 12 + k] + (k == r ? reg : 0.0);
    for (int k = 0; k < 10; ++k) W[12 + k] = X[(6 + k) * XJ + 1 + r];
    c = 0.0;
    for (int k = 0; k < 16; ++k) c += Jc[r * 16 + k] * vf[k];
    if (r % 3 == 2) {
      const double phi = feet[r] - ground_z;
      c += (fmax(phi, 0.0) + erp * fmin(phi, 0.0)) / h;
    }
  } else {
    for (int k = 0; k < 12; ++k) W[k] = sr * Xj[1 + k];
    for (int k = 0; k < 10; ++k) W[12 + k] = sr * Xj[13 + k];
    c = sr * vf[6 + j] + (r >= 22 ? bstop[j] : 0.0);
  }
  g = c;
  for (int k = 0; k < 12; ++k) g += W[k] * wp[k];
  for (int k = 0; k < 10; ++k) g += W[12 + k] * (wp[12 + k] + sgn[k] * wp[22 + k]);
  p = wp[r];
}

// One substep of length h.  q[16], v[16] in / out (LDS); imp[32] (LDS behind `lds`) in / out; taua[10] (LDS) the saturated torque.
// TERRAIN (hb_contact.hpp): rows 0-11 are those of the plane's frame, through A, the contact columns of X and Jc; the joint rows are unchanged.
// TERRAIN 2 (the profile) and 3 (the height field, hts = its heights): the same with the frame and offset of each point's facet.
template <int TERRAIN = 0, class Ctx>
HB_HD void joints_substep(const Ctx& cx, const DevModel& Mdl, double* q, double* v, const double* wrench, const int* all_on,
                          const hb_contact_config& K, const hb_joint_model& Jm, double eps, double h, double* lds, double* vdot_out,
                          const double* ter = nullptr, const double* hts = nullptr) {
  double* Jc = lds + PlantJointLds::Jc;
  double* X = lds + PlantJointLds::X;
  double* A = lds + PlantJointLds::A;
  double* feet = lds + PlantJointLds::feet;
  double* vf = lds + JointLds::vf;
  double* wgen = lds + JointLds::wgen;
  double* imp = lds + JointLds::imp;
  double* taua = lds + JointLds::taua;
  double* mdiag = lds + JointLds::mdiag;
  double* sgn = lds + JointLds::sgn;
  double* bstop = lds + JointLds::bstop;
  if (cx.lane == 0) {
    for (int a = 0; a < 6; ++a) wgen[a] = 0.0;
    if (wrench) {   // w = [F, E(zyx)' m, 0]: the power of the moment is m . E rates
      double sz, cz, sy, cy;
      sincos_t(q[3], sz, cz);
      sincos_t(q[4], sy, cy);
      for (int a = 0; a < 3; ++a) wgen[a] = wrench[a];
      wgen[3] = wrench[5];
      wgen[4] = -sz * wrench[3] + cz * wrench[4];
      wgen[5] = cy * cz * wrench[3] + cy * sz * wrench[4] - sy * wrench[5];
    }
#pragma unroll
    for (int j = 0; j < HB_NJ; ++j) {
      wgen[6 + j] = -Jm.damping[j] * v[6 + j];
      mdiag[j] = Jm.armature[j] + h * Jm.damping[j];
      const double lo = q[6 + j] - Jm.lower[j], up = Jm.upper[j] - q[6 + j];
      const bool low = lo <= up;
      const double phi = low ? lo : up;
      sgn[j] = low ? 1.0 : -1.0;
      bstop[j] = (fmax(phi, 0.0) + Jm.limit_erp * fmin(phi, 0.0)) / h;
      const double u = imp[22 + j];   // stored signed in joint coordinates: a change of side starts from zero
      imp[22 + j] = Jm.limits ? fmax(0.0, sgn[j] * u) : 0.0;
    }
  }
  // the front half of the pinned stub's substep with every point on (its first barrier publishes what lane 0 wrote above)
  plant_substep<2>(cx, Mdl, q, v, taua, all_on, nullptr, 0.0, 0.0, h, lds, nullptr, nullptr, wgen, mdiag);
  for (int i = cx.lane; i < 16; i += cx.nlanes) vf[i] = v[i] + h * X[i * XJ];
  double ground_z;
  if constexpr (TERRAIN >= 2) {
    if constexpr (TERRAIN == 3) field_select(cx, const_cast<double*>(ter), hts, feet);   // (its barrier publishes vf)
    else profile_select(cx, const_cast<double*>(ter), feet);   // (its barrier publishes vf)
    profile_rotate<XJ>(cx, ter + Profile::act, Jc, X, A, feet);
    ground_z = row_ground<TERRAIN>(ter, cx.lane < 12 ? cx.lane : 0, 0.0);   // (the lane's own row)
  } else if constexpr (TERRAIN) {
    terrain_rotate<XJ>(cx, ter + Terrain::T, Jc, X, A, feet);   // (its barriers publish vf)
    ground_z = ter[Terrain::d];
  } else {
    cx.sync();
    ground_z = K.ground_z;
  }
  double tr = 0.0;
  for (int i = 0; i < 12; ++i) tr += A[i * 13];
  const double reg = eps * tr, mu = K.mu;
  double mup[HB_NC];
  point_mu<(TERRAIN != 0)>(ter, mu, mup);
  const bool stops = Jm.limits != 0;
  double D[12], Dj[HB_NJ], lim[HB_NJ], sj[HB_NJ];
  for (int k = 0; k < 12; ++k) D[k] = A[k * 13] + reg;
  for (int j = 0; j < HB_NJ; ++j) {
    Dj[j] = X[(6 + j) * XJ + 13 + j];
    lim[j] = Jm.frictionloss[j] * h;
    sj[j] = sgn[j];
  }
#if defined(__HIP_DEVICE_COMPILE__)
  {
    const int r = cx.lane < 32 ? cx.lane : 0;   // (lanes 32.. shadow lane 0: nothing reads them)
    double W[22], g, p, res = 0.0, jres = 0.0;
    joint_row(r, A, X, Jc, vf, feet, ground_z, K.erp, h, sgn, bstop, imp, reg, W, g, p);
    for (int s = 0; s < K.sweeps; ++s) {
      res = 0.0;
      jres = 0.0;
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
#pragma unroll
      for (int j = 0; j < HB_NJ; ++j) {
        const double p0 = wave_bcast_f64(p, 12 + j), pf = pgs_box(wave_bcast_f64(g, 12 + j), p0, Dj[j], lim[j]), dp = pf - p0;
        g += W[12 + j] * dp;
        p = cx.lane == 12 + j ? pf : p;
        jres = fmax(jres, fabs(Dj[j] * dp));
      }
      if (stops) {
#pragma unroll
        for (int j = 0; j < HB_NJ; ++j) {
          const double p0 = wave_bcast_f64(p, 22 + j), ps = pgs_normal(wave_bcast_f64(g, 22 + j), p0, Dj[j]), dp = ps - p0;
          g += W[12 + j] * (sj[j] * dp);
          p = cx.lane == 22 + j ? ps : p;
          jres = fmax(jres, fabs(Dj[j] * dp));
        }
      }
    }
    cx.sync();   // (every lane has read the warm start)
    if (cx.lane < 22) imp[cx.lane] = p;
    else if (cx.lane < 32) imp[cx.lane] = sgn[cx.lane - 22] * p;
    if (cx.lane == 0) { lds[JointLds::res] = res; lds[JointLds::res + 1] = jres; }
  }
#else
  {
    double W[32 * 22], g[32], p[32], res = 0.0, jres = 0.0;
    for (int r = 0; r < 32; ++r)
      joint_row(r, A, X, Jc, vf, feet, row_ground<TERRAIN>(ter, r < 12 ? r : 0, ground_z), K.erp, h, sgn, bstop, imp, reg, W + 22 * r, g[r], p[r]);
    auto col = [&](int k, double d) { for (int r = 0; r < 32; ++r) g[r] += W[22 * r + k] * d; };
    for (int s = 0; s < K.sweeps; ++s) {
      res = 0.0;
      jres = 0.0;
      for (int pt = 0; pt < 4; ++pt) {
        const int a = 3 * pt, b = a + 1, n = a + 2;
        const double pn = pgs_normal(g[n], p[n], D[n]), dn = pn - p[n];
        col(n, dn);
        p[n] = pn;
        res = fmax(res, fabs(D[n] * dn));
        double ta, tb;
        pgs_tangent(g[a], g[b], p[a], p[b], D[a], D[b], mup[pt], pn, ta, tb);
        const double da = ta - p[a], db = tb - p[b];
        for (int r = 0; r < 32; ++r) { g[r] += W[22 * r + a] * da; g[r] += W[22 * r + b] * db; }
        p[a] = ta;
        p[b] = tb;
        res = fmax(res, fmax(fabs(D[a] * da), fabs(D[b] * db)));
      }
      for (int j = 0; j < HB_NJ; ++j) {
        const double pf = pgs_box(g[12 + j], p[12 + j], Dj[j], lim[j]), dp = pf - p[12 + j];
        col(12 + j, dp);
        p[12 + j] = pf;
        jres = fmax(jres, fabs(Dj[j] * dp));
      }
      if (stops)
        for (int j = 0; j < HB_NJ; ++j) {
          const double ps = pgs_normal(g[22 + j], p[22 + j], Dj[j]), dp = ps - p[22 + j];
          col(12 + j, sj[j] * dp);
          p[22 + j] = ps;
          jres = fmax(jres, fabs(Dj[j] * dp));
        }
    }
    for (int r = 0; r < 22; ++r) imp[r] = p[r];
    for (int j = 0; j < HB_NJ; ++j) imp[22 + j] = sj[j] * p[22 + j];
    lds[JointLds::res] = res;
    lds[JointLds::res + 1] = jres;
  }
#endif
  cx.sync();
  // ---- v+ = v_f + Mh^-1 Jh' p (s_j p_j = u_j),  q+ = q + h v+
  for (int i = cx.lane; i < 16; i += cx.nlanes) {
    double vn = vf[i];
    for (int j = 0; j < 12; ++j) vn += X[i * XJ + 1 + j] * imp[j];
    for (int j = 0; j < HB_NJ; ++j) vn += X[i * XJ + 13 + j] * (imp[12 + j] + imp[22 + j]);
    if (vdot_out) vdot_out[i] = (vn - v[i]) / h;
    v[i] = vn;
    q[i] = q[i] + h * vn;
  }
  cx.sync();
}

// One plant tick of one instance in contact model 1 with the joint model: `substeps` substeps of dt / substeps, then the outputs of the
// step.  imp_g[12] the contact impulses, jimp_g[20] the friction impulses and the signed stop impulses; tau_last_g[10] takes the
// saturated torque (what hb_plant_sense reports as the joint torque).  HYBRID (hb_plant.hpp): `tau` is not read; the law is
// evaluated and saturated into taua before every substep, tau_last / tau_applied are the last substep's and saturation bit 10 + j is set
// if joint j was saturated in any substep.
template <bool HYBRID = false, int TERRAIN = 0, class Ctx>
HB_HD void joints_step(const Ctx& cx, const DevModel& Mdl, double* q_g, double* v_g, double* imp_g, double* jimp_g, const double* tau,
                       const double* wrench, const int* all_on, const hb_contact_config& K, const hb_joint_model& Jm, double eps, double dt,
                       int substeps, double* lds, double* lambda_out, double* vdot_out, double* tau_last_g, const ContactOut& out,
                       const JointOut& jout, const HybridActuator* actuator = nullptr, const double* ter = nullptr,
                       const ProfileIo* pio = nullptr, const double* hts = nullptr) {
  double* q = lds + JointLds::q;
  double* v = lds + JointLds::v;
  double* imp = lds + JointLds::imp;
  double* taua = lds + JointLds::taua;
  for (int i = cx.lane; i < 16; i += cx.nlanes) { q[i] = q_g[i]; v[i] = v_g[i]; }
  for (int i = cx.lane; i < 12; i += cx.nlanes) imp[i] = imp_g[i];
  for (int i = cx.lane; i < 20; i += cx.nlanes) imp[12 + i] = jimp_g[i];
  if constexpr (!HYBRID) {
    if (cx.lane == 0) {
#pragma unroll
      for (int j = 0; j < HB_NJ; ++j) taua[j] = joint_saturate(tau[j], Jm.torque_limit[j]);
    }
  }
  cx.sync();
  const double h = dt / substeps;
  if constexpr (HYBRID) {
    const HybridActuator& act = *actuator;
    ActuatorAcc acc;
    for (int s = 0; s < substeps; ++s) {
      actuator_eval(cx, act, q, v, s, taua, acc, [&](int j, double ts) { return joint_saturate(ts, actuator_pick(Jm.torque_limit, j)); });
      joints_substep<TERRAIN>(cx, Mdl, q, v, wrench, all_on, K, Jm, eps, h, lds, vdot_out, ter, hts);
    }
    actuator_finish(cx, act, substeps, acc, true);
  } else {
    for (int s = 0; s < substeps; ++s) joints_substep<TERRAIN>(cx, Mdl, q, v, wrench, all_on, K, Jm, eps, h, lds, vdot_out, ter, hts);
  }
  // ---- outputs: as contact_step, then the joint arrays
  const double* Jc = lds + PlantJointLds::Jc;
  double* feet = lds + PlantJointLds::feet;
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
  for (int i = cx.lane; i < 20; i += cx.nlanes) jimp_g[i] = imp[12 + i];
  for (int j = cx.lane; j < HB_NJ; j += cx.nlanes) {
    tau_last_g[j] = taua[j];
    jout.tau_applied[j] = taua[j];
    jout.friction_torque[j] = imp[12 + j] / h;
    jout.limit_torque[j] = imp[22 + j] / h;
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
    const double res = lds[JointLds::res], jres = lds[JointLds::res + 1];
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
    int js = 0;
    for (int j = 0; j < HB_NJ; ++j) {
      if (imp[22 + j] != 0.0) js |= 1 << j;              // (u = s p with p >= 0: nonzero exactly where the stop impulse is > 0)
      if constexpr (HYBRID) { if (actuator->sat[j] != 0.0) js |= 1 << (10 + j); }
      else { if (taua[j] != tau[j]) js |= 1 << (10 + j); }
    }
    if (!(jres <= Jm.tol)) js |= HB_JOINT_UNCONVERGED;
    jout.res[0] = jres;
    jout.status[0] = js;
  }
  cx.sync();
}

}  // namespace hb
