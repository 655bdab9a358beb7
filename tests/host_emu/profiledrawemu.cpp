// TEST HARNESS: the profile-draw routines (hb_profiledraw.hpp: what k_plant_profile_draw runs per instance, and the placement and locate
// k_plant_respawn runs on a profile) compiled for the host with one emulated lane, for tests/test_profile_draw_host.py.  Not part of the
// product; the product path always runs the kernels.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "../../hunter_bipedal_control_amd/csrc/hb_host.hpp"
#include "../../hunter_bipedal_control_amd/csrc/hb_respawn.hpp"
#include "../../hunter_bipedal_control_amd/csrc/hb_profiledraw.hpp"

using namespace hb;

extern "C" {
int pd_n() { return HB_PD_N; }
int pd_log_w() { return HB_PD_LOG_W; }
int pd_log_max() { return HB_PD_LOG_MAX; }
int pd_blocks() { return PD_BLOCKS; }
int pd_config_size() { return int(sizeof(hb_profile_draw_config)); }
int pd_profile_stored() { return Profile::stored; }
int pd_ground_size() { return Ground::size; }
unsigned pd_stream() { return HB_PD_STREAM; }
// offsets of the fields, in the order of the struct
void pd_config_offsets(int* out) {
  out[0] = offsetof(hb_profile_draw_config, seed); out[1] = offsetof(hb_profile_draw_config, kinds);
  out[2] = offsetof(hb_profile_draw_config, mu_per_point); out[3] = offsetof(hb_profile_draw_config, dir);
  out[4] = offsetof(hb_profile_draw_config, height_lo); out[5] = offsetof(hb_profile_draw_config, height_hi);
  out[6] = offsetof(hb_profile_draw_config, at_lo); out[7] = offsetof(hb_profile_draw_config, at_hi);
  out[8] = offsetof(hb_profile_draw_config, riser_slope); out[9] = offsetof(hb_profile_draw_config, steps_lo);
  out[10] = offsetof(hb_profile_draw_config, steps_hi); out[11] = offsetof(hb_profile_draw_config, run_lo);
  out[12] = offsetof(hb_profile_draw_config, run_hi); out[13] = offsetof(hb_profile_draw_config, mu_lo);
  out[14] = offsetof(hb_profile_draw_config, mu_hi); out[15] = offsetof(hb_profile_draw_config, follow_map);
  out[16] = offsetof(hb_profile_draw_config, log_capacity); out[17] = offsetof(hb_profile_draw_config, reserved);
}
const char* pd_config_refusal(const hb_profile_draw_config* K) { return profile_draw_config_refusal(*K); }
// the three blocks into u[PD_DRAW] / words[PD_DRAW]
void pd_draw(const hb_profile_draw_config* K, uint32_t instance, uint32_t episode, double* u, uint32_t* words) {
  for (int b = 0; b < PD_BLOCKS; ++b) profile_draw_block(*K, instance, episode, b, u, words + 4 * b);
}
// What the kernel does with a drawn set, the set call's normalisation of the direction included: a[2] = the stored direction, rel /
// pk[32] = the relative and the plant's knots, row[HB_PD_N], pro[Profile::stored] = the profile record, map[Ground::size] = the record of
// the map that follows.  -> the number of knots.
int pd_compose(const hb_profile_draw_config* K0, const double* u, const double* q_spawn, double ground_z, double* a, double* rel, double* pk,
               double* row, double* pro, double* map) {
  hb_profile_draw_config K = *K0;
  profile_direction(K0->dir, K.dir);
  a[0] = K.dir[0];
  a[1] = K.dir[1];
  const int nk = profile_draw_knots(K, u, profile_draw_s0(K.dir, q_spawn), ground_z, rel, pk, row);
  profile_compose(OneLane{}, nk, K.dir, pk, row + HB_PD_MUS, pro);
  ground_compose(OneLane{}, nk, K.dir, rel, map);
  return nk;
}
// the level ground the set call puts an instance on: its knots and its record with mu = cfg_mu
int pd_flat(const double* dir, const double* q_spawn, double ground_z, double cfg_mu, double* rel, double* pk, double* pro) {
  double a[2];
  profile_direction(dir, a);
  const int nk = profile_draw_flat(profile_draw_s0(a, q_spawn), ground_z, rel, pk);
  const double mu4[HB_NC] = {cfg_mu, cfg_mu, cfg_mu, cfg_mu};
  profile_compose(OneLane{}, nk, a, pk, mu4, pro);
  return nk;
}
// the host setters' records: 0, or -1 with the refusal in why[128]
static int refusal(const char* w, char* why) {
  if (!w) return 0;
  int k = 0;
  for (; k < 127 && w[k]; ++k) why[k] = w[k];
  why[k] = 0;
  return -1;
}
int pd_profile_record(int K, const double* dir, const double* knots, const double* mu, double cfg_mu, double* rec, char* why) {
  return refusal(profile_record(K, dir, knots, mu, cfg_mu, rec), why);
}
int pd_ground_record(int K, const double* dir, const double* knots, double* rec, char* why) { return refusal(ground_record(K, dir, knots, rec), why); }
void pd_log_append(int capacity, int cause, const double* a, const int* irec, const double* drec, const int* itot, const double* row, int* count,
                   double* log) {
  profile_draw_log_append(OneLane{}, capacity, cause, a, irec, drec, itot, row, count, log);
}
// contact points at q, the placement on the profile and the locate of the placed state: q, feet[12], seg[5], base[14] as k_plant_respawn
// leaves them
void pd_place(const hb_model* m, const hb_respawn_config* K, const double* pro, double* q, double* feet, int* seg, double* base) {
  const DevModel d = make_dev_model(*m);
  plant_feet(d, q, feet);
  profile_place(d, *K, pro, q, feet);
  profile_locate_state(pro, q, feet, seg, base);
}
// the placement on a plane (hb_respawn.hpp), for the level anchor
void pd_place_plane(const hb_model* m, const hb_respawn_config* K, const double* plane, double* q, double* feet) {
  const DevModel d = make_dev_model(*m);
  plant_feet(d, q, feet);
  respawn_place(d, *K, plane, q, feet);
}
void pd_feet(const hb_model* m, const double* q, double* feet) { plant_feet(make_dev_model(*m), q, feet); }
}
