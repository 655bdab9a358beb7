// TEST HARNESS: the plant's sensor model (hb_sensors.hpp: the routine k_plant_sense runs per instance, and its Philox4x32-10 generator)
// compiled for the host, one loop iteration per instance, for tests/test_sensors_host.py.
// Not part of the product; the product path always runs the kernel.
#include <cstddef>
#include <cstdint>
#include "../../hunter_bipedal_control_amd/csrc/hb_sensors.hpp"

using namespace hb;

extern "C" {
void se_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
  const Philox4 p = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
  for (int k = 0; k < 4; ++k) out[k] = p.w[k];
}
// four normals of one block, as the routine draws them
void se_normals(uint64_t seed, uint32_t instance, uint64_t count, int block, double* z) {
  SenseNormals N(seed, instance, count);
  for (int l = 0; l < 4; ++l) z[l] = N.get(4 * block + l);
}
int se_config_valid(const hb_sensor_config* K) { return sensor_config_valid(*K) ? 1 : 0; }
// q, v, vdot [B][16], tau [B][10], contact [B][4]; K / gyro_bias / accel_bias may be null; outputs as hb_plant_sense
void se_sense(int B, double gravity, const double* q, const double* v, const double* vdot, const double* tau, const int* contact,
              const hb_sensor_config* K, const double* gyro_bias, const double* accel_bias, uint64_t count, double* quat, double* gyro,
              double* accel, double* jp, double* jv, double* jt, int* cf) {
  const hb_sensor_config ideal{};
  for (int i = 0; i < B; ++i) {
    const size_t s = size_t(i);
    const SenseOut o{quat + 4 * s, gyro + 3 * s, accel + 3 * s, jp + 10 * s, jv + 10 * s, jt + 10 * s, cf + 4 * s};
    plant_sense(gravity, q + 16 * s, v + 16 * s, vdot + 16 * s, tau + 10 * s, contact + 4 * s, K ? *K : ideal, K != nullptr, gyro_bias ? gyro_bias + 3 * s : nullptr,
                accel_bias ? accel_bias + 3 * s : nullptr, (K ? K->instance_offset : 0u) + uint32_t(i), count, o);
  }
}
}
