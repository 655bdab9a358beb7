// LCM wire format of the reference's low-level messages (include/hunter_lcm.h): member tables, lcm-gen's structure
// hash, the host codec and the device-side packers.  Reference: lcm_msg/include/*.lcm, lcm_msg/include/lcm_msg/*.hpp
// (generated encoders), legged_examples/legged_mujoco/src/LeggedMujocoSim.cpp:28-62 (field mapping).
#pragma once
#include <cstdint>
#include <cstring>
#include "../../include/hunter_lcm.h"
#include "hb_sensors.hpp"

namespace hb {

struct LcmMember {
  const char* name;
  const char* type;
  int dim;  // 0 = scalar
};
struct LcmType {
  const LcmMember* m;
  int n_members, n_fields;  // fields = doubles after the timestamp
};
inline const LcmType& lcm_type(int type) {
  static const LcmMember low_cmd[] = {{"timestamp", "int64_t", 0}, {"joint_pos", "double", 10}, {"joint_vel", "double", 10},
                                      {"joint_torque", "double", 10}, {"ff_tau", "double", 10}, {"kp", "double", 10}, {"kd", "double", 10}};
  static const LcmMember low_state[] = {{"timestamp", "int64_t", 0}, {"quaternion", "double", 4}, {"gyroscope", "double", 3},
                                        {"accelerometer", "double", 3}, {"joint_pos", "double", 10}, {"joint_vel", "double", 10},
                                        {"joint_torque", "double", 10}};
  static const LcmMember full_state[] = {{"timestamp", "int64_t", 0}, {"quaternion", "double", 4}, {"gyroscope", "double", 3},
                                         {"accelerometer", "double", 3}, {"position", "double", 3}, {"velocity", "double", 3},
                                         {"joint_pos", "double", 12}, {"joint_vel", "double", 12}, {"joint_torque", "double", 12},
                                         {"foot_force", "double", 4}};
  static const LcmType types[3] = {{low_cmd, 7, 60}, {low_state, 7, 40}, {full_state, 10, 56}};
  return types[type];
}
// lcm-gen's structure hash (lcmgen.c lcm_struct_hash: seed 0x12345678; per member the name, the primitive type name, the
// number of dimensions and per dimension its mode (0 = constant) and its size as a string; the struct name is not hashed)
inline int64_t lcm_hash_update(int64_t v, char c) {
  v = int64_t((uint64_t(v) << 8) ^ uint64_t(v >> 55)) + c;  // v >> 55 is the arithmetic shift of the original
  return v;
}
inline int64_t lcm_hash_string(int64_t v, const char* s) {
  v = lcm_hash_update(v, char(strlen(s)));
  for (; *s; ++s) v = lcm_hash_update(v, *s);
  return v;
}
inline uint64_t lcm_fingerprint(int type) {
  const LcmType& t = lcm_type(type);
  int64_t v = 0x12345678;
  for (int i = 0; i < t.n_members; ++i) {
    v = lcm_hash_string(v, t.m[i].name);
    v = lcm_hash_string(v, t.m[i].type);
    const int ndim = t.m[i].dim ? 1 : 0;
    v = lcm_hash_update(v, char(ndim));
    if (ndim) {
      char buf[16];
      snprintf(buf, sizeof buf, "%d", t.m[i].dim);
      v = lcm_hash_update(v, 0);
      v = lcm_hash_string(v, buf);
    }
  }
  const uint64_t h = uint64_t(v);
  return (h << 1) + ((h >> 63) & 1);  // _computeHash of a struct without compound members (low_cmd_t.hpp:188-192)
}
inline void lcm_put64(uint8_t* p, uint64_t v) {
  for (int b = 0; b < 8; ++b) p[b] = uint8_t(v >> (56 - 8 * b));
}
inline uint64_t lcm_get64(const uint8_t* p) {
  uint64_t v = 0;
  for (int b = 0; b < 8; ++b) v = (v << 8) | p[b];
  return v;
}

// ---- the simulator end of the link, per item: what the three kernels below and the host emulation (tests/host_emu/actemu.cpp) run ----
HB_HD uint64_t lcm_bits(double x) { uint64_t b; __builtin_memcpy(&b, &x, 8); return b; }
HB_HD double lcm_double(uint64_t b) { double x; __builtin_memcpy(&x, &b, 8); return x; }
// MujocoLcm::HandleLowCmd (mujoco/src/lcm_interface/LcmInterface.cpp:23-33) for one instance: in[62] = a low_cmd_t wire image (big-endian
// words: 0 fingerprint, 1 timestamp, 2 + 10 f + j field f joint j; fields joint_pos joint_vel joint_torque ff_tau kp kd).  The message
// replaces the command iff (uint64) timestamp > *last_ts; joint_torque is not read.  -> 1 if accepted.
HB_HD int lcm_accept_cmd(const uint64_t* in, double* pos, double* vel, double* kp, double* kd, double* ff, uint64_t* last_ts) {
  const uint64_t ts = __builtin_bswap64(in[1]);
  if (!(ts > *last_ts)) return 0;
  *last_ts = ts;
  for (int j = 0; j < 10; ++j) {
    pos[j] = lcm_double(__builtin_bswap64(in[2 + j]));
    vel[j] = lcm_double(__builtin_bswap64(in[12 + j]));
    ff[j] = lcm_double(__builtin_bswap64(in[32 + j]));
    kp[j] = lcm_double(__builtin_bswap64(in[42 + j]));
    kd[j] = lcm_double(__builtin_bswap64(in[52 + j]));
  }
  return 1;
}
// Word w < 42 of the low_state_t of MujocoLcm::SetSend (LcmInterface.cpp:52-71) in host byte order, from one instance's sensed arrays:
// 0 fingerprint, 1 timestamp, 2..5 quaternion (w x y z) from quat (x y z w), 6..8 gyroscope, 9..11 accelerometer, 12..21 joint_pos,
// 22..31 joint_vel, 32..41 joint_torque (the sensed torque; the reference sends qfrc_applied, zero in its runs and never read).
HB_HD uint64_t lcm_low_state_word(int w, uint64_t fingerprint, int64_t timestamp, const double* quat, const double* gyro, const double* accel,
                                  const double* jp, const double* jv, const double* jt) {
  if (w == 0) return fingerprint;
  if (w == 1) return uint64_t(timestamp);
  if (w < 6) return lcm_bits(quat[w == 2 ? 3 : w - 3]);
  if (w < 9) return lcm_bits(gyro[w - 6]);
  if (w < 12) return lcm_bits(accel[w - 9]);
  if (w < 22) return lcm_bits(jp[w - 12]);
  if (w < 32) return lcm_bits(jv[w - 22]);
  return lcm_bits(jt[w - 32]);
}
// The full_state_t of SetSend (:78-100) of one instance, out[58] big-endian words, ground truth: the ideal reading of plant_sense (no
// noise, no bias) for quaternion and gyroscope; 2..5 quaternion (w x y z), 6..8 gyroscope, 9..11 accelerometer = 0, 12..14 position,
// 15..17 velocity, 18..29 joint_pos, 30..41 joint_vel, 42..53 joint_torque (entries 10, 11 zero), 54..57 foot_force = 0.
HB_HD void lcm_full_state(double gravity, const double* q, const double* v, const double* tau, uint64_t fingerprint, int64_t timestamp,
                          uint64_t* out) {
  double quat[4], gyro[3], accel[3], jp[10], jv[10], jt[10];
  const double zero3[3] = {0.0, 0.0, 0.0};
  const int on[4] = {1, 1, 1, 1};
  int flags[4];
  plant_sense(gravity, q, v, zero3, tau, on, hb_sensor_config{}, false, nullptr, nullptr, 0u, 0u, SenseOut{quat, gyro, accel, jp, jv, jt, flags});
  out[0] = __builtin_bswap64(fingerprint);
  out[1] = __builtin_bswap64(uint64_t(timestamp));
  out[2] = __builtin_bswap64(lcm_bits(quat[3]));
  for (int a = 0; a < 3; ++a) {
    out[3 + a] = __builtin_bswap64(lcm_bits(quat[a]));
    out[6 + a] = __builtin_bswap64(lcm_bits(gyro[a]));
    out[9 + a] = 0;
    out[12 + a] = __builtin_bswap64(lcm_bits(q[a]));
    out[15 + a] = __builtin_bswap64(lcm_bits(v[a]));
  }
  for (int j = 0; j < 12; ++j) {
    out[18 + j] = j < 10 ? __builtin_bswap64(lcm_bits(jp[j])) : 0;
    out[30 + j] = j < 10 ? __builtin_bswap64(lcm_bits(jv[j])) : 0;
    out[42 + j] = j < 10 ? __builtin_bswap64(lcm_bits(jt[j])) : 0;
  }
  for (int c = 0; c < 4; ++c) out[54 + c] = 0;
}

#if defined(__HIPCC__)
// ---- device-side packers --------------------------------------------------------------------------------------------
// One thread per 8-byte word of the wire image.  low_cmd_t: word 0 fingerprint, 1 timestamp, 2 + 10 f + j field f joint j.
// jc = joint-command outputs [6][B][10]: posDes velDes kp kd ff torque (k_joint_command).
__global__ void k_lcm_pack_cmd(int B, const double* __restrict__ jc, uint64_t fingerprint, int64_t timestamp, uint64_t* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * 62) return;
  const int i = idx / 62, w = idx - 62 * i;
  uint64_t v;
  if (w == 0) v = fingerprint;
  else if (w == 1) v = uint64_t(timestamp);
  else {
    const int f = (w - 2) / 10, j = (w - 2) - 10 * f;
    // wire field f: joint_pos joint_vel joint_torque ff_tau kp kd  <-  jc block: posDes(0) velDes(1) -(zero) ff(4) kp(2) kd(3)
    const int src = f == 0 ? 0 : f == 1 ? 1 : f == 3 ? 4 : f == 4 ? 2 : 3;
    const double x = f == 2 ? 0.0 : jc[(size_t(src) * B + i) * 10 + j];
    v = uint64_t(__double_as_longlong(x));
  }
  out[idx] = __builtin_bswap64(v);
}
// low_state_t: word 0 fingerprint, 1 timestamp, 2..5 quaternion (w x y z), 6..8 gyroscope, 9..11 accelerometer,
// 12..21 joint_pos, 22..31 joint_vel, 32..41 joint_torque.  bad[0] is set when a fingerprint does not match.
__global__ void k_lcm_unpack_state(int B, const uint64_t* __restrict__ in, uint64_t fingerprint, double* __restrict__ quat,
                                   double* __restrict__ w_local, double* __restrict__ a_local, double* __restrict__ qj,
                                   double* __restrict__ qdj, long long* __restrict__ ts, int* __restrict__ bad) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * 42) return;
  const int i = idx / 42, w = idx - 42 * i;
  const uint64_t v = __builtin_bswap64(in[idx]);
  const double x = __longlong_as_double((long long)v);
  if (w == 0) { if (v != fingerprint) atomicOr(bad, 1); }
  else if (w == 1) { if (ts) ts[i] = (long long)v; }
  else if (w < 6) quat[4 * i + (w == 2 ? 3 : w - 3)] = x;  // (w x y z) on the wire -> (x y z w)
  else if (w < 9) w_local[3 * i + w - 6] = x;
  else if (w < 12) a_local[3 * i + w - 9] = x;
  else if (w < 22) qj[10 * i + w - 12] = x;
  else if (w < 32) qdj[10 * i + w - 22] = x;
}
// ---- the simulator end (hb_plant_step_lcm, hb_plant_sense_lcm) -------------------------------------------------------------------
// low_cmd_t in: one thread per instance — the acceptance reads and writes the instance's last_ts, so an instance is one thread's.
__global__ void k_lcm_unpack_cmd(int B, const uint64_t* __restrict__ in, double* pos, double* vel, double* kp, double* kd, double* ff,
                                 uint64_t* last_ts, int* accepted) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  accepted[i] = lcm_accept_cmd(in + size_t(i) * 62, pos + 10 * i, vel + 10 * i, kp + 10 * i, kd + 10 * i, ff + 10 * i, last_ts + i);
}
// low_state_t out: one thread per 8-byte word, from the sensor arrays hb_plant_sense left on the device
__global__ void k_lcm_pack_state(int B, const double* __restrict__ quat, const double* __restrict__ gyro, const double* __restrict__ accel,
                                 const double* __restrict__ jp, const double* __restrict__ jv, const double* __restrict__ jt, uint64_t fingerprint,
                                 int64_t timestamp, uint64_t* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * 42) return;
  const int i = idx / 42, w = idx - 42 * i;
  out[idx] = __builtin_bswap64(lcm_low_state_word(w, fingerprint, timestamp, quat + 4 * i, gyro + 3 * i, accel + 3 * i, jp + 10 * i, jv + 10 * i, jt + 10 * i));
}
// full_state_t out: one thread per instance, from the plant's state
__global__ void k_lcm_pack_full(int B, double gravity, const double* __restrict__ q, const double* __restrict__ v, const double* __restrict__ tau,
                                uint64_t fingerprint, int64_t timestamp, uint64_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  lcm_full_state(gravity, q + 16 * i, v + 16 * i, tau + 10 * i, fingerprint, timestamp, out + size_t(i) * 58);
}
#endif

}  // namespace hb
