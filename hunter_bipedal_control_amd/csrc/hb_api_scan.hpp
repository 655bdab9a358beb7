// Host side, part 6b: the height scan (hb_plant_set_height_scan, hb_plant_scan, hb_plant_get_height_scan; include/hunter_hip.h above
// hb_plant_set_height_scan).  The procedure is hb_scan.hpp scan_instance, the kernel k_plant_scan; the static helpers shared with the plant
// and ground entries (scan_refresh_host, scan_off, scan_mark_cleared) stand at the head of hb_api_plant.hpp.
#pragma once

extern "C" {

int32_t hb_plant_set_height_scan(hb_ctx* ctx, const hb_height_scan_config* cfg) {
  HB_ENTER_ARGS(false);
  if (!cfg && !ctx->scan_on) return HB_OK;
  HB_TRY(contact_ready(ctx, "hb_plant_set_height_scan"));
  HB_TRY(refuse_config(ctx, "hb_plant_set_height_scan", cfg ? height_scan_config_refusal(*cfg) : nullptr));
  HB_FAIL_IF(cfg && !ctx->gfield_on, HB_ERR_STATE, ctx->ground_on ? "hb_plant_set_height_scan: a profile map is in force (hb_ground_set_profile): the scan writes field maps, set the zero field map first (hb_ground_set_field)"
                                                                  : "hb_plant_set_height_scan: no field map in force (hb_ground_set_field): set the zero field map first");
  HB_FAIL_IF(cfg && ctx->field_draw_on && ctx->field_draw_cfg.follow_map, HB_ERR_STATE, "hb_plant_set_height_scan: the field draw in force writes the field map (hb_plant_set_field_draw, follow_map): turn it off first");
  HB_FAIL_IF(cfg && ctx->profile_draw_on && ctx->profile_draw_cfg.follow_map, HB_ERR_STATE, "hb_plant_set_height_scan: the profile draw in force writes the controller's map (hb_plant_set_profile_draw, follow_map): turn it off first");
  HB_FAIL_IF(cfg && ctx->n_chunks > 1, HB_ERR_STATE, "hb_plant_set_height_scan: instance ranges are in force (hb_set_chunks > 1): the scan runs on the whole batch only");
  HB_ENTER_DEVICE();
  HB_TRY(hb_sync(ctx));   // (a scan or a pass in flight still runs under the configuration and on the map it was launched with)
  if (!cfg) return scan_off(ctx);
  ScanBatch& c = ctx->scan;
  HB_TRY(ensure_fields(ctx, c));
  hb_height_scan_config K = *cfg;
  profile_direction(cfg->dir, K.dir);
  // the map is cleared: no height, no return, and the first scan holds nothing
  HB_TRY(zero_field(ctx, ctx->gfield, ctx->gfield.z));
  std::fill(ctx->gfield_z_host.begin(), ctx->gfield_z_host.end(), 0.0);
  HB_TRY(zero_field(ctx, c, c.k));
  HB_TRY(zero_field(ctx, c, c.n_returns));
  HB_TRY(zero_field(ctx, c, c.returned));
  HB_TRY(scan_mark_cleared(ctx, ctx->s_wbc));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  ctx->scan_cfg = K;
  ctx->scan_count = 0;
  ctx->scan_on = true;
  return HB_OK;
}

int32_t hb_plant_scan(hb_ctx* ctx) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->scan_on, HB_ERR_STATE, "hb_plant_scan: no height scan in force (hb_plant_set_height_scan)");
  HB_ENTER_DEVICE();
  hipStream_t s = ctx->s_wbc;   // behind the plant step and a respawn: the stream k_plant_field_draw writes the map on
  const int* itot = ctx->respawn_on ? ctx->respawn.itot : nullptr;
  const double gz = ctx->contact_cfg.ground_z;
  const uint32_t count = ctx->scan_count;
  // a reader of the resident observation and a writer of the map the MPC stream's planner and filter read: between the two ordering points
  HB_TRY(resident_write(ctx, s, true, [&] {
    auto go = [&](auto kernel, const double* gnd, int gstride, const double* fz) {
      hipLaunchKernelGGL(kernel, dim3(ctx->B), dim3(64), 0, s, ctx->scan, ctx->scan_cfg, count, ctx->plant.q, ctx->w.rbd, itot, gnd, gstride, fz,
                         ctx->gfield, gz);
    };
    switch (scan_ground(ctx->terrain_on, ctx->profile_on, ctx->field_on)) {
      case ScanGround::Field: go(k_plant_scan<SCAN_FIELD>, ctx->field.hdr, Field::stored, ctx->field.z); break;
      case ScanGround::Profile: go(k_plant_scan<SCAN_PROFILE>, ctx->profile.prof, Profile::stored, nullptr); break;
      case ScanGround::Plane: go(k_plant_scan<SCAN_PLANE>, ctx->terrain.ter, Terrain::size, nullptr); break;
      case ScanGround::None: go(k_plant_scan<SCAN_NONE>, nullptr, 0, nullptr); break;
    }
  }));
  ++ctx->scan_count;
  return HB_OK;
}

int32_t hb_plant_get_height_scan(hb_ctx* ctx, hb_height_scan_config* cfg, int32_t* origin_index, int32_t* n_returns, uint8_t* returned) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->scan_on, HB_ERR_STATE, "hb_plant_get_height_scan: no height scan in force (hb_plant_set_height_scan)");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  if (cfg) *cfg = ctx->scan_cfg;
  ScanBatch& c = ctx->scan;
  HB_TRY(pull(ctx, origin_index, c, c.k, whole(ctx)));
  HB_TRY(pull(ctx, n_returns, c, c.n_returns, whole(ctx)));
  return pull(ctx, returned, c, c.returned, whole(ctx));
}

}  // extern "C"
