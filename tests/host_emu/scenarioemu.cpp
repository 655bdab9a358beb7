// TEST HARNESS: the scenario routines (hb_scenario.hpp: what k_plant_scenario and k_plant_push run per instance) compiled for the host with
// one emulated lane, for tests/test_scenario_host.py.  Not part of the product; the product path always runs the kernels.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "../../hunter_bipedal_control_amd/csrc/hb_host.hpp"
#include "../../hunter_bipedal_control_amd/csrc/hb_scenario.hpp"

using namespace hb;
namespace {
struct HostCtx {
  int lane = 0, nlanes = 1;
  void sync() const {}
};
}  // namespace

extern "C" {
int sc_n() { return HB_SC_N; }
int sc_log_w() { return HB_SC_LOG_W; }
int sc_log_max() { return HB_SC_LOG_MAX; }
int sc_blocks() { return SC_BLOCKS; }
int sc_record_bytes() { return int(sizeof(DevModel)); }
int sc_config_size() { return int(sizeof(hb_scenario_config)); }
unsigned sc_stream() { return HB_SC_STREAM; }
// offsets of the fields, in the order of the struct
void sc_config_offsets(int* out) {
  out[0] = offsetof(hb_scenario_config, seed); out[1] = offsetof(hb_scenario_config, channels);
  out[2] = offsetof(hb_scenario_config, mu_per_point); out[3] = offsetof(hb_scenario_config, grade_max);
  out[4] = offsetof(hb_scenario_config, mu_lo); out[5] = offsetof(hb_scenario_config, mu_hi);
  out[6] = offsetof(hb_scenario_config, payload_mass_max); out[7] = offsetof(hb_scenario_config, payload_center);
  out[8] = offsetof(hb_scenario_config, payload_half_extent); out[9] = offsetof(hb_scenario_config, mass_scale_range);
  out[10] = offsetof(hb_scenario_config, push_force_max); out[11] = offsetof(hb_scenario_config, push_start_lo);
  out[12] = offsetof(hb_scenario_config, push_start_hi); out[13] = offsetof(hb_scenario_config, push_ticks);
  out[14] = offsetof(hb_scenario_config, log_capacity); out[15] = offsetof(hb_scenario_config, reserved);
}
const char* sc_config_refusal(const hb_scenario_config* K) { return scenario_config_refusal(*K); }
// the blocks the configuration needs into u[SC_DRAW] / words[SC_DRAW] (the others untouched); generated[SC_BLOCKS] tells which
void sc_draw(const hb_scenario_config* K, uint32_t instance, uint32_t episode, double* u, uint32_t* words, int* generated) {
  for (int b = 0; b < SC_BLOCKS; ++b) {
    generated[b] = scenario_block_needed(*K, b) ? 1 : 0;
    if (generated[b]) scenario_draw_block(*K, instance, episode, b, u, words + 4 * b);
  }
}
// the nominal DevModel record
void sc_nominal(const hb_model* m, void* rec) {
  const DevModel d = make_dev_model(*m);
  std::memcpy(rec, &d, sizeof d);
}
// the composition from a drawn set: ter[Terrain::size] and rec[sizeof(DevModel)] in and out, scen[HB_SC_N] and push[3] out
void sc_compose(const hb_model* m, const hb_scenario_config* K, const double* u, const double* spawn_xy, double ground_z, double* ter, void* rec,
                double* scen, double* push) {
  const DevModel nom = make_dev_model(*m);
  DevModel d;
  std::memcpy(&d, rec, sizeof d);
  double work[SC_WORK];
  scenario_compose(*K, u, spawn_xy, ground_z, nom, ter, &d, scen, push, work);
  std::memcpy(rec, &d, sizeof d);
}
// what hb_plant_set_terrain stores for plane[4] (T and d of r[Terrain::size]); returns | |n| - 1 |'s operand, the length
double sc_terrain_record(const double* plane, double* r) {
  const double len = terrain_normal_length(plane);
  terrain_plane_record(plane, len, r);
  return len;
}
// mass[11], com[11][3], inertia[11][6], total_mass of a record
void sc_model_arrays(const void* rec, double* mass, double* com, double* inertia, double* total_mass) {
  DevModel d;
  std::memcpy(&d, rec, sizeof d);
  std::memcpy(mass, d.mass, sizeof d.mass);
  std::memcpy(com, d.com, sizeof d.com);
  std::memcpy(inertia, d.inertia, sizeof d.inertia);
  *total_mass = d.total_mass;
}
void sc_row_init(double* scen, double* push) { scenario_row_init(scen, push); }
void sc_log_append(int capacity, int cause, const int* irec, const double* drec, const int* itot, const double* scen, int* count, double* log) {
  scenario_log_append(HostCtx{}, capacity, cause, irec, drec, itot, scen, count, log);
}
void sc_push_wrench(const hb_scenario_config* K, const double* push, int steps, double* wrench) { scenario_push_wrench(*K, push, steps, wrench); }
}
