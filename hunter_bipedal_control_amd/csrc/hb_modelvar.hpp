// Per-instance variation of the plant's inertial parameters (hb_plant_set_model_variation; the definition stands in include/hunter_hip.h
// above that declaration): the composition of one instance's DevModel from the nominal one, a mass scale per body and a payload on the
// base, and the refusals.  Plain C++ without a device dependency: the host composes the image it uploads, and
// tests/host_emu/modelvaremu.cpp compiles this header with g++.
#pragma once
#include <cmath>

#include "hb_model.hpp"

namespace hb {

constexpr int MODELVAR_PAYLOAD = HB_PAYLOAD_SIZE;   // m_p | r[3] | I_p[6] = xx xy xz yy yz zz (HB_PAYLOAD_SIZE)
struct Payload {
  enum : int { m = 0, r = 1, I = 4 };
};
// slack of the 2 x 2 and of the 3 x 3 principal minors of I_p, in units of a^2 and a^3 with a the largest |entry|: the roundings of the
// expressions below on entries up to a (two products and a difference; six triple products and five sums)
constexpr double MODELVAR_PSD2 = 4.0 * 2.220446049250313e-16, MODELVAR_PSD3 = 64.0 * 2.220446049250313e-16;

// P(m, d) = m (|d|^2 1 - d d') as xx xy xz yy yz zz: |d|^2 = (dx dx + dy dy) + dz dz; diagonal m (|d|^2 - da da); off-diagonal m (0 - da db)
HB_HD void modelvar_shift(double m, const double* d, double* P) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  P[0] = m * (dd - d[0] * d[0]);
  P[1] = m * (0.0 - d[0] * d[1]);
  P[2] = m * (0.0 - d[0] * d[2]);
  P[3] = m * (dd - d[1] * d[1]);
  P[4] = m * (0.0 - d[1] * d[2]);
  P[5] = m * (dd - d[2] * d[2]);
}

// Why the variation (scale[HB_NBODY] or null, payload[MODELVAR_PAYLOAD] or null) of one instance is refused, or null.
HB_HD const char* modelvar_refusal(const double* scale, const double* payload) {
  for (int b = 0; scale && b < HB_NBODY; ++b)
    if (!std::isfinite(scale[b])) return "a non-finite mass scale";
  for (int k = 0; payload && k < MODELVAR_PAYLOAD; ++k)
    if (!std::isfinite(payload[k])) return "a non-finite payload entry";
  for (int b = 0; scale && b < HB_NBODY; ++b)
    if (!(scale[b] > 0.0)) return "a mass scale <= 0";
  if (!payload) return nullptr;
  if (payload[Payload::m] < 0.0) return "a negative payload mass";
  const double* I = payload + Payload::I;
  double a = 0.0;
  for (int k = 0; k < 6; ++k) a = std::fmax(a, std::fabs(I[k]));
  if (payload[Payload::m] == 0.0 && a != 0.0) return "a payload inertia without a payload mass";
  const double xx = I[0], xy = I[1], xz = I[2], yy = I[3], yz = I[4], zz = I[5];
  const double s2 = MODELVAR_PSD2 * a * a, s3 = MODELVAR_PSD3 * a * a * a;
  const double det = ((xx * yy * zz + xy * yz * xz) + xz * xy * yz) - ((xz * yy * xz + xy * xy * zz) + xx * yz * yz);
  if (xx < 0.0 || yy < 0.0 || zz < 0.0 || xx * yy - xy * xy < -s2 || xx * zz - xz * xz < -s2 || yy * zz - yz * yz < -s2 || det < -s3)
    return "a payload inertia that is not positive semidefinite";
  return nullptr;
}

// The instance's model.  Unvaried (no payload mass, every scale == 1.0): a copy of the nominal record, total_mass included.  Nothing is
// fused (here and in modelvar_shift): the device (k_plant_scenario) composes the bits the host composes.
HB_HD void modelvar_compose(const DevModel& N, const double* scale, const double* payload, DevModel* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  *out = N;
  const double mp = payload ? payload[Payload::m] : 0.0;
  bool varied = mp != 0.0;
  for (int b = 0; scale && b < HB_NBODY; ++b) varied = varied || scale[b] != 1.0;
  if (!varied) return;
  for (int b = 1; b < HB_NBODY; ++b) {
    const double s = scale ? scale[b] : 1.0;
    out->mass[b] = s * N.mass[b];
    for (int k = 0; k < 6; ++k) out->inertia[b][k] = s * N.inertia[b][k];
  }
  const double s0 = scale ? scale[0] : 1.0, ms = s0 * N.mass[0], m0 = ms + mp;
  const double zero[3] = {0.0, 0.0, 0.0};
  const double* r = payload ? payload + Payload::r : zero;
  double d1[3], d2[3], P1[6], P2[6];
  for (int a = 0; a < 3; ++a) {
    out->com[0][a] = (ms * N.com[0][a] + mp * r[a]) / m0;
    d1[a] = N.com[0][a] - out->com[0][a];
    d2[a] = r[a] - out->com[0][a];
  }
  modelvar_shift(ms, d1, P1);
  modelvar_shift(mp, d2, P2);
  out->mass[0] = m0;
  for (int k = 0; k < 6; ++k) out->inertia[0][k] = ((s0 * N.inertia[0][k] + P1[k]) + (payload ? payload[Payload::I + k] : 0.0)) + P2[k];
  double total = 0.0;
  for (int b = 0; b < HB_NBODY; ++b) total += out->mass[b];
  out->total_mass = total;
}

// The batch: out[B] records from scale[B][HB_NBODY] or null and payload[B][MODELVAR_PAYLOAD] or null.  Returns null, or the reason the
// first offending instance *bad is refused for (out is then partly written and to be dropped).
inline const char* modelvar_compose_batch(const DevModel& N, int B, const double* scale, const double* payload, DevModel* out, int* bad) {
  for (int i = 0; i < B; ++i) {
    const double* sc = scale ? scale + HB_NBODY * i : nullptr;
    const double* pl = payload ? payload + MODELVAR_PAYLOAD * i : nullptr;
    if (const char* why = modelvar_refusal(sc, pl)) {
      *bad = i;
      return why;
    }
    modelvar_compose(N, sc, pl, out + i);
  }
  return nullptr;
}

}  // namespace hb
