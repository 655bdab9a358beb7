// TEST HARNESS: the height-scan routines (hb_scan.hpp: what k_plant_scan runs per instance) compiled for the host with one emulated lane,
// for tests/test_height_scan_host.py and tests/test_gpu_height_scan.py.  Not part of the product; the product path always runs the kernel.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "../../hunter_bipedal_control_amd/csrc/hb_host.hpp"
#include "../../hunter_bipedal_control_amd/csrc/hb_scan.hpp"

using namespace hb;

extern "C" {
int hs_config_size() { return int(sizeof(hb_height_scan_config)); }
unsigned hs_stream() { return HB_HS_STREAM; }
int hs_nz() { return GroundField::nz; }
int hs_ground_size() { return GroundField::size; }
int hs_terrain_size() { return Terrain::size; }
int hs_profile_stored() { return Profile::stored; }
int hs_field_stored() { return Field::stored; }
int hs_profile_brk() { return Profile::brk; }
int hs_profile_seg() { return Profile::seg; }
int hs_profile_rec() { return Profile::rec; }
int hs_field_dir() { return Field::dir; }
int hs_nrbd() { return HB_NRBD; }
int hs_episode_index() { return HB_RS_I_EPISODE_INDEX; }
int hs_rs_ni() { return HB_RS_NI; }
// offsets of the fields, in the order of the struct
void hs_config_offsets(int* out) {
  out[0] = offsetof(hb_height_scan_config, n_nodes); out[1] = offsetof(hb_height_scan_config, back);
  out[2] = offsetof(hb_height_scan_config, dir); out[3] = offsetof(hb_height_scan_config, spacing);
  out[4] = offsetof(hb_height_scan_config, range); out[5] = offsetof(hb_height_scan_config, noise);
  out[6] = offsetof(hb_height_scan_config, dropout); out[7] = offsetof(hb_height_scan_config, register_mode);
  out[8] = offsetof(hb_height_scan_config, reserved); out[9] = offsetof(hb_height_scan_config, seed);
  out[10] = offsetof(hb_height_scan_config, instance_offset); out[11] = offsetof(hb_height_scan_config, pad);
}
int hs_config_valid(const hb_height_scan_config* K) { return height_scan_config_valid(*K) ? 1 : 0; }
// What the set call does with a configuration: refused (0) and *stored untouched, or accepted (1) and *stored = the configuration with the
// direction normalised.
int hs_config_store(const hb_height_scan_config* K, hb_height_scan_config* stored) {
  if (!height_scan_config_valid(*K)) return 0;
  *stored = *K;
  profile_direction(K->dir, stored->dir);
  return 1;
}
int hs_origin(const hb_height_scan_config* K, const double* p, const double* e, int* k, double* org) { return scan_origin(*K, p, e, k, org) ? 1 : 0; }
double hs_plane_z(const double* n, double d, const double* s) { return scan_plane_z(n, d, s); }
// the normals / uniforms of block `blk` of a channel as scan_instance generates them
void hs_normals(const hb_height_scan_config* K, uint32_t instance, uint32_t count, int blk, double* z) {
  const Philox4 w = philox4x32_10(instance, count, HB_HS_STREAM, uint32_t(blk), uint32_t(K->seed), uint32_t(K->seed >> 32));
  box_muller(w.w[0], w.w[1], z[0], z[1]);
  box_muller(w.w[2], w.w[3], z[2], z[3]);
}
// the records of the host setters the scan samples: 0, or -1 when the setter refuses
int hs_plane_record(const double* plane, double* rec) {
  for (int k = 0; k < Terrain::size; ++k) rec[k] = 0.0;
  terrain_plane_record(plane, terrain_normal_length(plane), rec);
  return 0;
}
int hs_profile_record(int K, const double* dir, const double* knots, double* rec) { return profile_record(K, dir, knots, nullptr, 0.5, rec) ? -1 : 0; }
int hs_field_record(const int* n, const double* dir, const double* org, const double* step, const double* z, double* rec) {
  return field_record(n, dir, org, step, z, nullptr, 0.5, rec) ? -1 : 0;
}
double hs_map_height(const double* hdr, const double* z, double x, double y, int* facet) { return ground_field_height(hdr, z, x, y, facet); }
int hs_facet(const double* hdr, const double* z, const double* x, double* rec) { return field_facet(hdr, z, x, rec); }

// One scan of B instances, as hb_plant_scan enqueues it: K the STORED configuration, `count` the scan count, ground = SCAN_* with gnd
// [B][gstride] and fz [B][nz]; q [B][16], rbd [B][HB_NRBD], itot [B][HB_RS_NI] or null; the map hdr [B][8] / z [B][nz] and the ScanBatch
// arrays k [B][2], episode_seen [B], n_returns [B], returned [B][nz] are updated in place.
void hs_scan(const hb_height_scan_config* K, uint32_t count, int B, int ground, const double* gnd, int gstride, const double* fz, const double* q,
             const double* rbd, const int* itot, double ground_z, double* hdr, double* z, int* k, int* episode_seen, int* n_returns,
             unsigned char* returned) {
  static double old[GroundField::nz];
  int cnt[1];
  for (int i = 0; i < B; ++i) {
    ScanIo io;
    io.q = q + 16 * size_t(i);
    io.rbd = rbd + HB_NRBD * size_t(i);
    io.itot = itot ? itot + HB_RS_NI * size_t(i) : nullptr;
    io.gnd = gnd ? gnd + size_t(gstride) * i : nullptr;
    io.fz = fz ? fz + size_t(Field::nz) * i : nullptr;
    io.hdr = hdr + size_t(GroundField::size) * i;
    io.z = z + size_t(GroundField::nz) * i;
    io.k = k + 2 * size_t(i);
    io.episode_seen = episode_seen + i;
    io.n_returns = n_returns + i;
    io.returned = returned + size_t(GroundField::nz) * i;
    const uint32_t inst = K->instance_offset + uint32_t(i);
    const OneLane cx{};
    if (ground == SCAN_FIELD) scan_instance<SCAN_FIELD>(cx, *K, inst, count, ground_z, io, old, cnt);
    else if (ground == SCAN_PROFILE) scan_instance<SCAN_PROFILE>(cx, *K, inst, count, ground_z, io, old, cnt);
    else if (ground == SCAN_PLANE) scan_instance<SCAN_PLANE>(cx, *K, inst, count, ground_z, io, old, cnt);
    else scan_instance<SCAN_NONE>(cx, *K, inst, count, ground_z, io, old, cnt);
  }
}
}
