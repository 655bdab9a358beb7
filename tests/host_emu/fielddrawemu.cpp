// TEST HARNESS: the field-draw routines (hb_fielddraw.hpp: what k_plant_field_draw runs per instance, and the placement and locate
// k_plant_respawn_field runs on a height field) compiled for the host with one emulated lane, for tests/test_field_draw_host.py.  Not part
// of the product; the product path always runs the kernels.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "../../hunter_bipedal_control_amd/csrc/hb_host.hpp"
#include "../../hunter_bipedal_control_amd/csrc/hb_respawn.hpp"
#include "../../hunter_bipedal_control_amd/csrc/hb_fielddraw.hpp"

using namespace hb;

extern "C" {
int fd_n() { return HB_FD_N; }
int fd_log_w() { return HB_FD_LOG_W; }
int fd_log_max() { return HB_FD_LOG_MAX; }
int fd_head_blocks() { return FD_HEAD_BLOCKS; }
int fd_node_blocks() { return FD_NODE_BLOCKS; }
int fd_config_size() { return int(sizeof(hb_field_draw_config)); }
int fd_field_stored() { return Field::stored; }
int fd_field_dir() { return Field::dir; }
int fd_ground_size() { return GroundField::size; }
int fd_nz() { return Field::nz; }
unsigned fd_stream() { return HB_FD_STREAM; }
// offsets of the fields, in the order of the struct
void fd_config_offsets(int* out) {
  out[0] = offsetof(hb_field_draw_config, seed); out[1] = offsetof(hb_field_draw_config, kinds);
  out[2] = offsetof(hb_field_draw_config, mu_per_point); out[3] = offsetof(hb_field_draw_config, dir);
  out[4] = offsetof(hb_field_draw_config, n_nodes); out[5] = offsetof(hb_field_draw_config, spacing);
  out[6] = offsetof(hb_field_draw_config, centre); out[7] = offsetof(hb_field_draw_config, calm);
  out[8] = offsetof(hb_field_draw_config, amp_lo); out[9] = offsetof(hb_field_draw_config, amp_hi);
  out[10] = offsetof(hb_field_draw_config, slope_u_lo); out[11] = offsetof(hb_field_draw_config, slope_u_hi);
  out[12] = offsetof(hb_field_draw_config, slope_w_lo); out[13] = offsetof(hb_field_draw_config, slope_w_hi);
  out[14] = offsetof(hb_field_draw_config, mu_lo); out[15] = offsetof(hb_field_draw_config, mu_hi);
  out[16] = offsetof(hb_field_draw_config, follow_map); out[17] = offsetof(hb_field_draw_config, log_capacity);
  out[18] = offsetof(hb_field_draw_config, reserved);
}
const char* fd_config_refusal(const hb_field_draw_config* K) { return field_draw_config_refusal(*K); }
// block `block` into u[4] / words[4]
void fd_block(const hb_field_draw_config* K, uint32_t instance, uint32_t episode, int block, double* u, uint32_t* words) {
  field_draw_block(*K, instance, episode, block, u, words);
}
// What the kernel does for a respawning instance, the set call's normalisation of the direction included, in the kernel's order: the head
// blocks, the row, the 256 node blocks out to z / gz [Field::nz], then the stored header hdr[Field::stored] and the map's
// ghdr[GroundField::size].  a[2] = the stored direction.
void fd_compose(const hb_field_draw_config* K0, uint32_t instance, uint32_t episode, const double* q_spawn, double ground_z, double* a, double* row,
                double* z, double* gz, double* hdr, double* ghdr) {
  hb_field_draw_config K = *K0;
  profile_direction(K0->dir, K.dir);
  a[0] = K.dir[0];
  a[1] = K.dir[1];
  double u[FD_HEAD];
  for (int b = 0; b < FD_HEAD_BLOCKS; ++b) field_draw_block(K, instance, episode, b, u + 4 * b, nullptr);
  const FieldDrawPar par = field_draw_head(K, u, row);
  for (int m = 0; m < FD_NODE_BLOCKS / 64; ++m)
    for (int lane = 0; lane < 64; ++lane) field_draw_nodes(K, par, instance, episode, lane + 64 * m, ground_z, z, gz);
  double org[2];
  field_draw_origin(K, K.dir, q_spawn, org);
  field_compose(K.n_nodes, K.dir, org, K.spacing, z, row + HB_FD_MUS, hdr);
  ground_field_compose(K.n_nodes, K.dir, org, K.spacing, ghdr);
}
// the level ground the set call puts an instance on: its heights, its header with mu = cfg_mu, and the zero map's
void fd_flat(const hb_field_draw_config* K0, const double* q_spawn, double ground_z, double cfg_mu, double* z, double* gz, double* hdr, double* ghdr) {
  hb_field_draw_config K = *K0;
  profile_direction(K0->dir, K.dir);
  double org[2];
  field_draw_origin(K, K.dir, q_spawn, org);
  field_draw_flat(K, ground_z, z, gz);
  const double mu4[HB_NC] = {cfg_mu, cfg_mu, cfg_mu, cfg_mu};
  field_compose(K.n_nodes, K.dir, org, K.spacing, z, mu4, hdr);
  ground_field_compose(K.n_nodes, K.dir, org, K.spacing, ghdr);
}
// the host setters' records: 0, or -1 with the refusal in why[128]
static int refusal(const char* w, char* why) {
  if (!w) return 0;
  int k = 0;
  for (; k < 127 && w[k]; ++k) why[k] = w[k];
  why[k] = 0;
  return -1;
}
int fd_field_record(const int* n, const double* dir, const double* org, const double* step, const double* z, const double* mu, double cfg_mu,
                    double* rec, char* why) {
  return refusal(field_record(n, dir, org, step, z, mu, cfg_mu, rec), why);
}
int fd_ground_field_record(const int* n, const double* dir, const double* org, const double* step, const double* z, double* h, char* why) {
  return refusal(ground_field_record(n, dir, org, step, z, h), why);
}
void fd_log_append(int capacity, int cause, const double* a, const int* irec, const double* drec, const int* itot, const double* row, int* count,
                   double* log) {
  field_draw_log_append(OneLane{}, capacity, cause, a, irec, drec, itot, row, count, log);
}
// the facet under a world point: its id and its record (T, d)
int fd_facet(const double* hdr, const double* z, const double* x, double* rec) { return field_facet(hdr, z, x, rec); }
// contact points at q, the placement on the field and the locate of the placed state: q, feet[12], sel[5], base[14] as
// k_plant_respawn_field leaves them
void fd_place(const hb_model* m, const hb_respawn_config* K, const double* hdr, const double* z, double* q, double* feet, int* sel, double* base) {
  const DevModel d = make_dev_model(*m);
  plant_feet(d, q, feet);
  field_place(d, *K, hdr, z, q, feet);
  field_locate_state(hdr, z, q, feet, sel, base);
}
// the placement on a plane (hb_respawn.hpp), for the level anchor
void fd_place_plane(const hb_model* m, const hb_respawn_config* K, const double* plane, double* q, double* feet) {
  const DevModel d = make_dev_model(*m);
  plant_feet(d, q, feet);
  respawn_place(d, *K, plane, q, feet);
}
void fd_feet(const hb_model* m, const double* q, double* feet) { plant_feet(make_dev_model(*m), q, feet); }
}
