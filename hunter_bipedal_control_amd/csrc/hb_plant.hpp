// Contact-consistent rigid-body plant stub on the device, one 64-lane workgroup per robot —
// the device counterpart of hunter_bipedal_control_amd/plant.py (same equations, same constants):
//     M(q) vdot + nle(q, v) = S' tau + Jc' lambda,      Jc vdot = -dJc v - 2 a Jc v - a^2 (p_c - p_anchor)
// with lambda from the damped normal equations (Jc M^-1 Jc' + eps tr(.) I) lambda = rhs (a foot's two contact points
// give a rank-5 Jacobian), semi-implicit Euler.  The reference closes its loop through Gazebo / MuJoCo
// (legged_gazebo/src/LeggedHWSim.cpp:166-192, mujoco/src/main.cc:247); this stub replaces them for regression rollouts
// and does NOT enforce unilateral contact or friction limits (contact model 1, hb_contact.hpp, does).
// Coordinates: q = [pos, zyx, joints], v = [v_lin (world), ZYX rates, joint rates] (pinocchio's, WbcBase.cpp:72-79).
#pragma once
#include "hb_wbc.hpp"

namespace hb {

struct PlantLds {
  static constexpr int M = 0;            // 16 x 16 mass matrix, then its Cholesky factor (lower)
  static constexpr int Jc = M + 256;     // 12 x 16 masked contact Jacobian
  static constexpr int X = Jc + 192;     // 16 x 13 : M^-1 [rhs | Jc']
  static constexpr int A = X + 208;      // 12 x 12 : Jc M^-1 Jc' + regularisation (then its Cholesky factor)
  static constexpr int b = A + 144;      // 12 : constraint right-hand side, then lambda
  static constexpr int nle = b + 12;     // 16
  static constexpr int dJv = nle + 16;   // 12
  static constexpr int feet = dJv + 12;  // 12
  static constexpr int total = feet + 12;
  static constexpr int xs = 13;          // columns of X
};
// The same with X = M^-1 [rhs | Jc' | e_6 .. e_15] (16 x 23) for the joint model of contact model 1 (hb_joints.hpp)
struct PlantJointLds {
  static constexpr int M = 0;
  static constexpr int Jc = M + 256;
  static constexpr int X = Jc + 192;     // 16 x 23
  static constexpr int A = X + 368;
  static constexpr int b = A + 144;
  static constexpr int nle = b + 12;
  static constexpr int dJv = nle + 16;
  static constexpr int feet = dJv + 12;
  static constexpr int total = feet + 12;
  static constexpr int xs = 23;
};
template <int FRONT> struct PlantLdsOf { using type = PlantLds; };
template <> struct PlantLdsOf<2> { using type = PlantJointLds; };

// ---- the actuator of a step: a compile-time switch of plant_step / contact_step (hb_contact.hpp) / joints_step (hb_joints.hpp) ---------
// HYBRID = false: the caller's torque, held over every substep (hb_plant_step).  HYBRID = true: `actuator` is the instance's hybrid command; the law
//     tau_s[j] = ff[j] + kp[j] (pos[j] - q_s[6 + j]) + kd[j] (vel[j] - v_s[6 + j])        (operand order of k_joint_command)
// is evaluated before every substep from the staged (q, v) by the lanes j < 10 into tau[10] (LDS), which the substep routine takes as
// its torque (hb_plant_step_hybrid; the reference's simulator does the same per simulator step, mujoco/src/main.cc:243-249).  The five
// command values are re-read from global memory per substep, not kept live across the sweeps.
struct HybridActuator {
  const double *pos, *vel, *kp, *kd, *ff;   // [10] each, of the instance (global)
  double *tau_first, *tau_mean;             // [10] each, of the instance (global): tau_0 before saturation | mean of the torque integrated
  double* tau;                              // [10] LDS: tau_s
  double* sat;                              // [10] LDS (joint model only): != 0 where the joint was saturated in any substep
};
constexpr int ACT_LDS = 20;                 // tau | sat, behind a form's own LDS
// A lane's record of a hybrid step: lane j < 10 owns joint j; the one emulated lane of the host build owns all ten.
#if defined(__HIP_DEVICE_COMPILE__)
constexpr int ACT_SLOTS = 1;
#else
constexpr int ACT_SLOTS = HB_NJ;
#endif
struct ActuatorAcc {
  double sum[ACT_SLOTS];
  bool sat[ACT_SLOTS];
};
// f(joint, slot) for the joints the lane owns
template <class Ctx, class F>
HB_HD void actuator_joints(const Ctx& cx, F&& f) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (cx.lane < HB_NJ) f(cx.lane, 0);
#else
  (void)cx;
  for (int j = 0; j < HB_NJ; ++j) f(j, j);
#endif
}
// a[j] of a ten-entry array that lives in registers (a kernel argument): selected, never indexed by the lane
HB_HD double actuator_pick(const double (&a)[HB_NJ], int j) {
#if defined(__HIP_DEVICE_COMPILE__)
  double x = a[0];
#pragma unroll
  for (int k = 1; k < HB_NJ; ++k) x = j == k ? a[k] : x;
  return x;
#else
  return a[j];
#endif
}
// Before substep s: the law into out[10] (LDS; a.tau, or the joint model's saturated torque) through saturate(joint, tau_s) -> the torque
// the substep integrates.  The substep's first barrier publishes it.
template <class Ctx, class Sat>
HB_HD void actuator_eval(const Ctx& cx, const HybridActuator& a, const double* q, const double* v, int s, double* out, ActuatorAcc& acc,
                         Sat&& saturate) {
  actuator_joints(cx, [&](int j, int k) {
    const double ts = a.ff[j] + a.kp[j] * (a.pos[j] - q[6 + j]) + a.kd[j] * (a.vel[j] - v[6 + j]);
    const double ti = saturate(j, ts);
    if (s == 0) a.tau_first[j] = ts;
    acc.sum[k] = s == 0 ? ti : acc.sum[k] + ti;
    acc.sat[k] = (s != 0 && acc.sat[k]) || ti != ts;
    out[j] = ti;
  });
}
// After the last substep: the mean, and the saturation record where the form keeps one (a barrier of the caller publishes it).
template <class Ctx>
HB_HD void actuator_finish(const Ctx& cx, const HybridActuator& a, int substeps, const ActuatorAcc& acc, bool record_sat) {
  actuator_joints(cx, [&](int j, int k) {
    a.tau_mean[j] = acc.sum[k] / substeps;
    if (record_sat) a.sat[j] = acc.sat[k] ? 1.0 : 0.0;
  });
}

// One substep of length h.  q[16], v[16], anchor[12] in/out (global or LDS); rows[12] = 1 for pinned contact rows.
// FRONT = 1: the front half alone, for the ground-contact model (hb_contact.hpp) — the rigid-body terms at (q, v), the Cholesky factor
// of M, X = M^-1 [rhs | Jc'] with rhs = S' tau - nle (+ wext[16], a generalised force, when one is given) and Jc M^-1 Jc' are left in LDS
// (PlantLds: M, Jc, X, A, nle, dJv, feet); nothing behind `contact` in the argument list is used except lds and wext.
// FRONT = 2: the same for the joint model of that contact model (hb_joints.hpp), on the layout PlantJointLds: mdiag[10] is added to the
// joint diagonal of M before it is factored, and X carries the ten more columns M^-1 [e_6 .. e_15].
template <int FRONT = 0, class Ctx>
HB_HD void plant_substep(const Ctx& cx, const DevModel& Mdl, double* q, double* v, const double* tau, const int* contact, const double* anchor,
                         double baum, double eps, double h, double* lds, double* lambda_out, double* vdot_out, const double* wext = nullptr,
                         const double* mdiag = nullptr) {
  using L = typename PlantLdsOf<FRONT>::type;
  constexpr int XS = L::xs;
  double* Mm = lds + L::M;
  double* Jc = lds + L::Jc;
  double* X = lds + L::X;
  double* A = lds + L::A;
  double* b = lds + L::b;
  double* nle = lds + L::nle;
  double* dJv = lds + L::dJv;
  double* feet = lds + L::feet;
  // ---- rigid-body terms (lane 0)
  if (cx.lane == 0) {
    // results and work arrays in LDS (the X / A buffers are not live yet): thread-private they would sit in scratch
    static_assert((sizeof(BodyPass) + sizeof(BodyWork) + 7) / 8 <= L::b + 12 - L::X, "rigid-body workspace must fit X | A | b");
    BodyPass& P = *reinterpret_cast<BodyPass*>(X);
    body_pass(Mdl, q, v, P, *reinterpret_cast<BodyWork*>(X + (sizeof(BodyPass) + 7) / 8));
    mass_matrix(P, Mm);
    if constexpr (FRONT == 2) { for (int j = 0; j < 10; ++j) Mm[(6 + j) * 17] += mdiag[j]; }
    for (int a = 0; a < 16; ++a) nle[a] = P.nle[a];
    for (int ci = 0; ci < HB_NC; ++ci) {
      const double on = contact[ci] ? 1.0 : 0.0;
      for (int col = 0; col < 16; ++col) {
        const Vec3<double> jc = contact_jac(P, ci, col);
        Jc[(3 * ci + 0) * 16 + col] = on * jc.x; Jc[(3 * ci + 1) * 16 + col] = on * jc.y; Jc[(3 * ci + 2) * 16 + col] = on * jc.z;
      }
      dJv[3 * ci] = P.foot_acc[ci].x; dJv[3 * ci + 1] = P.foot_acc[ci].y; dJv[3 * ci + 2] = P.foot_acc[ci].z;
      feet[3 * ci] = q[0] + P.foot[ci].x; feet[3 * ci + 1] = q[1] + P.foot[ci].y; feet[3 * ci + 2] = q[2] + P.foot[ci].z;
    }
  }
  cx.sync();
  // ---- Cholesky of M in place (lower), column by column
  for (int k = 0; k < 16; ++k) {
    const double d = sqrt(Mm[k * 17]);
    cx.sync();
    for (int i = k + cx.lane; i < 16; i += cx.nlanes) Mm[i * 16 + k] = (i == k) ? d : Mm[i * 16 + k] / d;
    cx.sync();
    for (int e = cx.lane; e < (15 - k) * (15 - k); e += cx.nlanes) {
      const int a = e / (15 - k), c = e - a * (15 - k);
      if (c <= a) Mm[(k + 1 + a) * 16 + k + 1 + c] -= Mm[(k + 1 + a) * 16 + k] * Mm[(k + 1 + c) * 16 + k];
    }
    cx.sync();
  }
  // ---- X = M^-1 [rhs | Jc'],  rhs = S' tau - nle   (one right-hand side per lane)
  for (int c = cx.lane; c < XS; c += cx.nlanes) {
    double y[16];
    for (int i = 0; i < 16; ++i) {
      double s;
      if constexpr (FRONT == 2) {   // (the unit columns load nothing: Jc has twelve rows)
        if (c == 0) s = (i >= 6 ? tau[i - 6] : 0.0) - nle[i];
        else if (c < 13) s = Jc[(c - 1) * 16 + i];
        else s = (i == c - 7) ? 1.0 : 0.0;
      } else {
        s = (c == 0) ? ((i >= 6 ? tau[i - 6] : 0.0) - nle[i]) : Jc[(c - 1) * 16 + i];
      }
      if constexpr (FRONT != 0) { if (c == 0 && wext) s += wext[i]; }
      for (int k = 0; k < i; ++k) s -= Mm[i * 16 + k] * y[k];
      y[i] = s / Mm[i * 17];
    }
    for (int i = 15; i >= 0; --i) {
      double s = y[i];
      for (int k = i + 1; k < 16; ++k) s -= Mm[k * 16 + i] * y[k];
      y[i] = s / Mm[i * 17];
    }
    for (int i = 0; i < 16; ++i) X[i * XS + c] = y[i];
  }
  cx.sync();
  // ---- A = Jc M^-1 Jc' (+ damping, + identity on the free rows), b
  for (int idx = cx.lane; idx < 144; idx += cx.nlanes) {
    const int i = idx / 12, j = idx - 12 * i;
    double s = 0.0;
    for (int k = 0; k < 16; ++k) s += Jc[i * 16 + k] * X[k * XS + 1 + j];
    A[idx] = s;
  }
  cx.sync();
  if constexpr (FRONT != 0) return;
  double tr = 0.0;
  for (int i = 0; i < 12; ++i) tr += A[i * 13];
  tr = fmax(tr, 1e-12);
  cx.sync();
  for (int i = cx.lane; i < 12; i += cx.nlanes) {
    const bool on = contact[i / 3] != 0;
    A[i * 13] += eps * tr + (on ? 0.0 : 1.0);
    double vel = 0.0, jr = 0.0;
    for (int k = 0; k < 16; ++k) { vel += Jc[i * 16 + k] * v[k]; jr += Jc[i * 16 + k] * X[k * 13]; }
    const double err = on ? feet[i] - anchor[i] : 0.0;
    b[i] = (on ? (-dJv[i] - 2.0 * baum * vel - baum * baum * err) : 0.0) - jr;
  }
  cx.sync();
  // ---- Cholesky of A (12 x 12, SPD) and lambda, by lane 0 (tiny)
  if (cx.lane == 0) {
    for (int k = 0; k < 12; ++k) {
      double d = A[k * 13];
      for (int t = 0; t < k; ++t) d -= A[k * 12 + t] * A[k * 12 + t];
      d = sqrt(d);
      A[k * 13] = d;
      for (int i = k + 1; i < 12; ++i) {
        double s = A[i * 12 + k];
        for (int t = 0; t < k; ++t) s -= A[i * 12 + t] * A[k * 12 + t];
        A[i * 12 + k] = s / d;
      }
    }
    for (int i = 0; i < 12; ++i) {
      double s = b[i];
      for (int k = 0; k < i; ++k) s -= A[i * 12 + k] * b[k];
      b[i] = s / A[i * 13];
    }
    for (int i = 11; i >= 0; --i) {
      double s = b[i];
      for (int k = i + 1; k < 12; ++k) s -= A[k * 12 + i] * b[k];
      b[i] = s / A[i * 13];
    }
    for (int i = 0; i < 12; ++i) b[i] = contact[i / 3] ? b[i] : 0.0;
  }
  cx.sync();
  // ---- vdot, semi-implicit Euler
  for (int i = cx.lane; i < 16; i += cx.nlanes) {
    double a = X[i * 13];
    for (int j = 0; j < 12; ++j) a += X[i * 13 + 1 + j] * b[j];
    const double vn = v[i] + h * a;
    if (vdot_out) vdot_out[i] = a;
    v[i] = vn;
    q[i] = q[i] + h * vn;
  }
  for (int i = cx.lane; i < 12; i += cx.nlanes)
    if (lambda_out) lambda_out[i] = b[i];
  cx.sync();
}

// Contact point positions at q (for the anchors).
HB_HD void plant_feet(const DevModel& Mdl, const double* q, double* feet12) {
  const Mat3<double> R0 = [&] {
    double sz, cz, sy, cy, sx, cx;
    sincos_t(q[3], sz, cz); sincos_t(q[4], sy, cy); sincos_t(q[5], sx, cx);
    Mat3<double> R;
    R.m[0] = cz * cy; R.m[1] = cz * sy * sx - sz * cx; R.m[2] = cz * sy * cx + sz * sx;
    R.m[3] = sz * cy; R.m[4] = sz * sy * sx + cz * cx; R.m[5] = sz * sy * cx - cz * sx;
    R.m[6] = -sy;     R.m[7] = cy * sx;                R.m[8] = cy * cx;
    return R;
  }();
  const Vec3<double> p0(q[0], q[1], q[2]);
  const double* qj = q + 6;
  for (int leg = 0; leg < 2; ++leg) {
    LegOut<double> L;
    leg_eval<double>(Mdl, leg, [qj](int j) { return qj[j]; }, [](int) { return 0.0; }, L);
    st3(feet12 + 3 * leg, p0 + R0 * L.foot[0]);
    st3(feet12 + 3 * (leg + 2), p0 + R0 * L.foot[1]);
  }
}

// The plant's state (q, v) repacked as the rbd state a plant step publishes: euler zyx | position | joints | omega_world = E(zyx) rates |
// linear velocity | joint rates.
HB_HD void plant_rbd_from_state(const double* q, const double* v, double* rbd) {
  double sz, cz, sy, cy;
  sincos_t(q[3], sz, cz);
  sincos_t(q[4], sy, cy);
  for (int a = 0; a < 3; ++a) { rbd[a] = q[3 + a]; rbd[3 + a] = q[a]; rbd[HB_NV + 3 + a] = v[a]; }
  for (int j = 0; j < HB_NJ; ++j) { rbd[6 + j] = q[6 + j]; rbd[6 + HB_NV + j] = v[6 + j]; }
  rbd[HB_NV + 0] = -sz * v[4] + cy * cz * v[5];
  rbd[HB_NV + 1] = cz * v[4] + cy * sz * v[5];
  rbd[HB_NV + 2] = v[3] - sy * v[5];
}

// One plant tick of one instance: re-anchor the feet whose contact phase starts, `substeps` substeps of dt / substeps.
// State (q, v, anchor, pinned) lives in global memory; q / v are staged in LDS behind `lds`.
// HYBRID: `tau` is not read; the law's torque of every substep is (see above).
template <bool HYBRID = false, class Ctx>
HB_HD void plant_step(const Ctx& cx, const DevModel& Mdl, double* q_g, double* v_g, double* anchor_g, int* pinned_g, const double* tau,
                      const int* contact, double baum, double eps, double dt, int substeps, double* lds, double* lambda_out,
                      double* vdot_out, const HybridActuator* actuator = nullptr) {
  double* q = lds + PlantLds::total;
  double* v = q + 16;
  double* anchor = v + 16;
  for (int i = cx.lane; i < 16; i += cx.nlanes) { q[i] = q_g[i]; v[i] = v_g[i]; }
  for (int i = cx.lane; i < 12; i += cx.nlanes) anchor[i] = anchor_g[i];
  cx.sync();
  if (cx.lane == 0) {
    double feet[12];
    plant_feet(Mdl, q, feet);
    for (int ci = 0; ci < HB_NC; ++ci) {
      if (contact[ci] && !pinned_g[ci])
        for (int a = 0; a < 3; ++a) anchor[3 * ci + a] = feet[3 * ci + a];
      pinned_g[ci] = contact[ci] ? 1 : 0;
    }
  }
  cx.sync();
  const double h = dt / substeps;
  if constexpr (HYBRID) {
    const HybridActuator& act = *actuator;
    ActuatorAcc acc;
    for (int s = 0; s < substeps; ++s) {
      actuator_eval(cx, act, q, v, s, act.tau, acc, [](int, double ts) { return ts; });
      plant_substep(cx, Mdl, q, v, act.tau, contact, anchor, baum, eps, h, lds, lambda_out, vdot_out);
    }
    actuator_finish(cx, act, substeps, acc, false);
  } else {
    for (int s = 0; s < substeps; ++s) plant_substep(cx, Mdl, q, v, tau, contact, anchor, baum, eps, h, lds, lambda_out, vdot_out);
  }
  for (int i = cx.lane; i < 16; i += cx.nlanes) { q_g[i] = q[i]; v_g[i] = v[i]; }
  for (int i = cx.lane; i < 12; i += cx.nlanes) anchor_g[i] = anchor[i];
  cx.sync();
}
constexpr int PLANT_LDS_TOTAL = PlantLds::total + 16 + 16 + 12;

}  // namespace hb
