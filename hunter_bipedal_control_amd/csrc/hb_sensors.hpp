// Sensor model of the plant stub (hb_plant_sense): what LeggedController::updateStateEstimation reads from the hardware interfaces
// (LeggedController.cpp:318-345: IMU quaternion, gyroscope, accelerometer, joint encoders, joint efforts, commanded contact flags),
// computed from the plant's state, with optional constant biases and seeded, reproducible noise.  One instance per call; the kernel
// (k_plant_sense) and the host emulator (tests/host_emu/sensemu.cpp) run the same routine.
//
// Noise is counter based (Philox4x32-10, Salmon et al., SC'11) and has no state on the device:
//     key     = (seed low 32, seed high 32)
//     counter = (global instance index, sense_count low 32, sense_count high 32, block)
// A block of four words gives four standard normals by Box-Muller, u = (word + 0.5) 2^-32:
//     (w0, w1) -> r cos(2 pi u1), r sin(2 pi u1),  r = sqrt(-2 ln u0);   (w2, w3) likewise.
// Normal number n is lane n % 4 of block n / 4; the channels own fixed normals (SENSE_N_*), so a channel's noise does not depend on
// which other channels are on, and a channel with sigma = 0 is the ideal value bit for bit.  Blocks nobody needs are not generated.
#pragma once
#include <stdint.h>
#include "../../include/hunter_hip.h"
#include "hb_math.hpp"

namespace hb {

struct Philox4 { uint32_t w[4]; };

HB_HD void philox_mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
  const uint64_t p = uint64_t(a) * uint64_t(b);
  hi = uint32_t(p >> 32);
  lo = uint32_t(p);
}

// Philox4x32 with 10 rounds: counter c[4], key (k0, k1).
HB_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0, lo0, hi1, lo1;
    philox_mulhilo(0xD2511F53u, c0, hi0, lo0);
    philox_mulhilo(0xCD9E8D57u, c2, hi1, lo1);
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  Philox4 o;
  o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}

HB_HD void box_muller(uint32_t w0, uint32_t w1, double& z0, double& z1) {
  const double u0 = (double(w0) + 0.5) * 2.3283064365386963e-10;  // 2^-32
  const double u1 = (double(w1) + 0.5) * 2.3283064365386963e-10;
  const double r = sqrt(-2.0 * log(u0));
  double s, c;
  sincos_t(6.283185307179586477 * u1, s, c);
  z0 = r * c;
  z1 = r * s;
}

// first normal of every channel
constexpr int SENSE_N_ORIENTATION = 0, SENSE_N_GYRO = 3, SENSE_N_ACCEL = 6, SENSE_N_JOINT_POS = 9, SENSE_N_JOINT_VEL = 19, SENSE_N_JOINT_TORQUE = 29;

// The normals of one (instance, sense call), generated block by block on demand: asking for normals in increasing order generates
// every needed block once.
struct SenseNormals {
  uint32_t k0, k1, c0, c1, c2;
  int cur;
  double z[4];
  HB_HD SenseNormals(uint64_t seed, uint32_t instance, uint64_t count)
      : k0(uint32_t(seed)), k1(uint32_t(seed >> 32)), c0(instance), c1(uint32_t(count)), c2(uint32_t(count >> 32)), cur(-1) {
    z[0] = z[1] = z[2] = z[3] = 0.0;
  }
  HB_HD double get(int n) {
    const int blk = n >> 2, l = n & 3;
    if (blk != cur) {
      const Philox4 p = philox4x32_10(c0, c1, c2, uint32_t(blk), k0, k1);
      box_muller(p.w[0], p.w[1], z[0], z[1]);
      box_muller(p.w[2], p.w[3], z[2], z[3]);
      cur = blk;
    }
    return l == 0 ? z[0] : (l == 1 ? z[1] : (l == 2 ? z[2] : z[3]));
  }
};

// Outputs of one instance (anywhere: global memory, LDS, host).
struct SenseOut {
  double *quat, *gyro, *accel, *joint_pos, *joint_vel, *joint_torque;  // [4] (x y z w), [3], [3], [10], [10], [10]
  int* contact;                                                         // [4]
};

// q[16], v[16] of the plant (hb_plant.hpp coordinates), vdot_lin[3] = the base's last linear acceleration (world), tau[10] / contact[4] =
// what the last plant step applied.  noisy = false: ideal sensors, K is not read (a reference and a flag rather than a nullable pointer:
// the kernel's by-value argument then never needs an address).  gyro_bias / accel_bias [3] of this instance or null.  `instance` is the
// GLOBAL instance index (hb_sensor_config::instance_offset already added), `count` the number of the sense call.
HB_HD void plant_sense(double gravity, const double* q, const double* v, const double* vdot_lin, const double* tau, const int* contact,
                       const hb_sensor_config& K, bool noisy, const double* gyro_bias, const double* accel_bias, uint32_t instance,
                       uint64_t count, const SenseOut& o) {
  SenseNormals N(K.seed, instance, count);
  // ---- orientation: ZYX half-angle closed form, w >= 0
  double sz, cz, sy, cy, sx, cx;
  sincos_t(0.5 * q[3], sz, cz);
  sincos_t(0.5 * q[4], sy, cy);
  sincos_t(0.5 * q[5], sx, cx);
  double qx = cz * cy * sx - sz * sy * cx;
  double qy = cz * sy * cx + sz * cy * sx;
  double qz = sz * cy * cx - cz * sy * sx;
  double qw = cz * cy * cx + sz * sy * sx;
  if (noisy && K.orientation_noise > 0.0) {  // quat <- quat (x) [axis sin(|delta| / 2), cos(|delta| / 2)],  delta = sigma * (3 normals)
    const double dx = K.orientation_noise * N.get(SENSE_N_ORIENTATION), dy = K.orientation_noise * N.get(SENSE_N_ORIENTATION + 1),
                 dz = K.orientation_noise * N.get(SENSE_N_ORIENTATION + 2);
    const double ang = sqrt(dx * dx + dy * dy + dz * dz);
    if (ang > 0.0) {
      double sh, ch;
      sincos_t(0.5 * ang, sh, ch);
      const double f = sh / ang, bx = f * dx, by = f * dy, bz = f * dz, bw = ch;
      const double rx = qw * bx + bw * qx + (qy * bz - qz * by);
      const double ry = qw * by + bw * qy + (qz * bx - qx * bz);
      const double rz = qw * bz + bw * qz + (qx * by - qy * bx);
      const double rw = qw * bw - (qx * bx + qy * by + qz * bz);
      qx = rx; qy = ry; qz = rz; qw = rw;
    }
  }
  if (qw < 0.0) { qx = -qx; qy = -qy; qz = -qz; qw = -qw; }
  o.quat[0] = qx; o.quat[1] = qy; o.quat[2] = qz; o.quat[3] = qw;
  // ---- rotation matrix (world <- body) of the TRUE attitude, row-major
  sincos_t(q[3], sz, cz);
  sincos_t(q[4], sy, cy);
  sincos_t(q[5], sx, cx);
  const double r00 = cz * cy, r01 = cz * sy * sx - sz * cx, r02 = cz * sy * cx + sz * sx;
  const double r10 = sz * cy, r11 = sz * sy * sx + cz * cx, r12 = sz * sy * cx - cz * sx;
  const double r20 = -sy, r21 = cy * sx, r22 = cy * cx;
  // gyroscope: R' E(zyx) rates;  accelerometer: specific force R' (a + g e_z)   (scalars, not arrays: everything stays in registers)
  const double wx = -sz * v[4] + cy * cz * v[5], wy = cz * v[4] + cy * sz * v[5], wz = v[3] - sy * v[5];
  const double ax = vdot_lin[0], ay = vdot_lin[1], az = vdot_lin[2] + gravity;
  o.gyro[0] = r00 * wx + r10 * wy + r20 * wz;
  o.gyro[1] = r01 * wx + r11 * wy + r21 * wz;
  o.gyro[2] = r02 * wx + r12 * wy + r22 * wz;
  o.accel[0] = r00 * ax + r10 * ay + r20 * az;
  o.accel[1] = r01 * ax + r11 * ay + r21 * az;
  o.accel[2] = r02 * ax + r12 * ay + r22 * az;
  if (gyro_bias)
    for (int a = 0; a < 3; ++a) o.gyro[a] += gyro_bias[a];
  if (accel_bias)
    for (int a = 0; a < 3; ++a) o.accel[a] += accel_bias[a];
  if (noisy && K.gyro_noise > 0.0)
    for (int a = 0; a < 3; ++a) o.gyro[a] += K.gyro_noise * N.get(SENSE_N_GYRO + a);
  if (noisy && K.accel_noise > 0.0)
    for (int a = 0; a < 3; ++a) o.accel[a] += K.accel_noise * N.get(SENSE_N_ACCEL + a);
  // ---- joint encoders and efforts
  for (int j = 0; j < HB_NJ; ++j) { o.joint_pos[j] = q[6 + j]; o.joint_vel[j] = v[6 + j]; o.joint_torque[j] = tau[j]; }
  if (noisy && K.joint_pos_noise > 0.0)
    for (int j = 0; j < HB_NJ; ++j) o.joint_pos[j] += K.joint_pos_noise * N.get(SENSE_N_JOINT_POS + j);
  if (noisy && K.joint_vel_noise > 0.0)
    for (int j = 0; j < HB_NJ; ++j) o.joint_vel[j] += K.joint_vel_noise * N.get(SENSE_N_JOINT_VEL + j);
  if (noisy && K.joint_torque_noise > 0.0)
    for (int j = 0; j < HB_NJ; ++j) o.joint_torque[j] += K.joint_torque_noise * N.get(SENSE_N_JOINT_TORQUE + j);
  // ---- contact flags: never corrupted
  for (int c = 0; c < HB_NC; ++c) o.contact[c] = contact[c];
}

// Range check of a sensor model (hb_plant_set_sensor_model): every sigma finite and >= 0, reserved == 0.
inline bool sensor_config_valid(const hb_sensor_config& K) {
  const double s[6] = {K.orientation_noise, K.gyro_noise, K.accel_noise, K.joint_pos_noise, K.joint_vel_noise, K.joint_torque_noise};
  for (int k = 0; k < 6; ++k)
    if (!(s[k] >= 0.0) || !(s[k] <= 1.7976931348623157e308)) return false;
  return K.reserved == 0;
}

}  // namespace hb
