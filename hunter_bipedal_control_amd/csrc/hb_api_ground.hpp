// Host side, part 10: the ground map of the controller (hb_ground_*; include/hunter_hip.h above hb_ground_set_profile and
// hb_ground_set_field).  The stored record of an instance, validation included, is hb_ground.hpp ground_record (profile map) or
// ground_field_record (field map); the kernels that read it are the ground and field forms of the planner and the filter
// (launch_refgen, launch_estimator).
#pragma once

// One map at a time: the profile map, the field map or none.  Every change of what a range enqueues (on, off, profile <-> field) bumps
// graph_epoch, as hb_gait_reset does.
static void ground_map_select(hb_ctx* ctx, bool profile, bool field) {
  if (ctx->ground_on != profile || ctx->gfield_on != field) ++ctx->graph_epoch;
  ctx->ground_on = profile;
  ctx->gfield_on = field;
}

extern "C" {

int32_t hb_ground_set_profile(hb_ctx* ctx, const int32_t* n_knots, const double* dir, const double* knots) {
  HB_ENTER_ARGS(false);
  const bool on = n_knots || dir || knots;
  HB_FAIL_IF(on && !(n_knots && dir && knots), HB_ERR_ARG, "hb_ground_set_profile: give n_knots, dir and knots, or none of them to switch the map off (the map in force is kept)");
  HB_FAIL_IF(on && ctx->field_draw_on && ctx->field_draw_cfg.follow_map, HB_ERR_STATE, "hb_ground_set_profile: the field draw in force writes the field map (hb_plant_set_field_draw, follow_map): turn it off first");
  HB_FAIL_IF(ctx->scan_on, HB_ERR_STATE, "hb_ground_set_profile: the height scan in force writes the field map (hb_plant_set_height_scan): turn it off first");
  const size_t B = ctx->B;
  std::vector<double> rec(on ? B * Ground::size : 0), kn(on ? B * HB_PROFILE_MAX_KNOTS * 2 : 0);
  for (size_t i = 0; i < B && on; ++i) {
    const double* k = knots + i * HB_PROFILE_MAX_KNOTS * 2;
    if (const char* why = ground_record(n_knots[i], dir + 2 * i, k, rec.data() + i * Ground::size))
      return refuse_instance(ctx, HB_ERR_ARG, "hb_ground_set_profile", i, why, "map");
    std::memcpy(kn.data() + i * HB_PROFILE_MAX_KNOTS * 2, k, size_t(n_knots[i]) * 2 * sizeof(double));
  }
  HB_ENTER_DEVICE();
  HB_TRY(hb_sync(ctx));   // (a pass in flight still runs on the map it was launched with)
  if (on) {
    GroundBatch& g = ctx->ground;
    HB_TRY(ensure_fields(ctx, g));
    HB_TRY(push(ctx, rec.data(), g, g.map, whole(ctx)));
    ctx->ground_host = std::move(rec);
    ctx->ground_knots = std::move(kn);
  }
  ground_map_select(ctx, on, false);
  return HB_OK;
}

int32_t hb_ground_get_profile(hb_ctx* ctx, int32_t* n_knots, double* dir, double* knots, double* slopes) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(ctx->gfield_on, HB_ERR_STATE, "hb_ground_get_profile: the map in force is a field map (hb_ground_get_field)");
  HB_FAIL_IF(!ctx->ground_on, HB_ERR_STATE, "hb_ground_get_profile: no ground map in force (hb_ground_set_profile)");
  if (ctx->profile_draw_on && ctx->profile_draw_cfg.follow_map) {   // the device draws the records: the host image is stale
    HB_ENTER_DEVICE();
    HB_HIP(hipStreamSynchronize(ctx->s_wbc));
    HB_TRY(profile_draw_refresh_host(ctx));
  }
  for (size_t i = 0; i < size_t(ctx->B); ++i) {
    const double* r = ctx->ground_host.data() + i * Ground::size;
    if (n_knots) n_knots[i] = int32_t(r[Ground::nseg]) + 1;
    if (dir) std::memcpy(dir + 2 * i, r + Ground::dir, 2 * sizeof(double));
    if (knots) std::memcpy(knots + i * HB_PROFILE_MAX_KNOTS * 2, ctx->ground_knots.data() + i * HB_PROFILE_MAX_KNOTS * 2, HB_PROFILE_MAX_KNOTS * 2 * sizeof(double));
    if (slopes) std::memcpy(slopes + i * (HB_PROFILE_MAX_KNOTS - 1), r + Ground::slope, (HB_PROFILE_MAX_KNOTS - 1) * sizeof(double));
  }
  return HB_OK;
}

// The field map (include/hunter_hip.h above hb_ground_set_field): the stored header of an instance, validation included, is hb_ground.hpp
// ground_field_record; the kernels that read it are the field forms of the planner and the filter.
int32_t hb_ground_set_field(hb_ctx* ctx, const int32_t* n_nodes, const double* dir, const double* origin, const double* spacing, const double* heights) {
  HB_ENTER_ARGS(false);
  const bool on = n_nodes || dir || origin || spacing || heights;
  HB_FAIL_IF(on && !(n_nodes && dir && origin && spacing && heights), HB_ERR_ARG, "hb_ground_set_field: give n_nodes, dir, origin, spacing and heights, or none of them to switch the map off (the map in force is kept)");
  HB_FAIL_IF(on && ctx->profile_draw_on && ctx->profile_draw_cfg.follow_map, HB_ERR_STATE, "hb_ground_set_field: the profile draw in force writes the profile map (hb_plant_set_profile_draw, follow_map): turn it off first");
  HB_FAIL_IF(ctx->scan_on, HB_ERR_STATE, "hb_ground_set_field: the height scan in force writes the field map (hb_plant_set_height_scan): turn it off first");
  const size_t B = ctx->B;
  std::vector<double> hdr(on ? B * GroundField::size : 0), z(on ? B * GroundField::nz : 0);
  for (size_t i = 0; i < B && on; ++i) {
    const int n[2] = {n_nodes[2 * i], n_nodes[2 * i + 1]};
    const double* zi = heights + i * GroundField::nz;
    double* zo = z.data() + i * GroundField::nz;
    if (n[0] >= 2 && n[0] <= HB_FIELD_MAX_NODES && n[1] >= 2 && n[1] <= HB_FIELD_MAX_NODES)   // (the stored heights: zero beyond (nu, nw))
      for (int iu = 0; iu < n[0]; ++iu)
        for (int iw = 0; iw < n[1]; ++iw) zo[iu * GroundField::pitch + iw] = 0.0 + zi[iu * GroundField::pitch + iw];   // (0 + : no negative zero, as ground_compose)
    if (const char* why = ground_field_record(n, dir + 2 * i, origin + 2 * i, spacing + 2 * i, zo, hdr.data() + i * GroundField::size))
      return refuse_instance(ctx, HB_ERR_ARG, "hb_ground_set_field", i, why, "map");
  }
  HB_ENTER_DEVICE();
  HB_TRY(hb_sync(ctx));   // (a pass in flight still runs on the map it was launched with)
  if (on) {
    GroundFieldBatch& g = ctx->gfield;
    HB_TRY(ensure_fields(ctx, g));
    HB_TRY(push(ctx, hdr.data(), g, g.hdr, whole(ctx)));
    HB_TRY(push(ctx, z.data(), g, g.z, whole(ctx)));
    ctx->gfield_hdr_host = std::move(hdr);
    ctx->gfield_z_host = std::move(z);
  }
  ground_map_select(ctx, false, on);
  return HB_OK;
}

int32_t hb_ground_get_field(hb_ctx* ctx, int32_t* n_nodes, double* dir, double* origin, double* spacing, double* heights) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->gfield_on, HB_ERR_STATE, ctx->ground_on ? "hb_ground_get_field: the map in force is a profile map (hb_ground_get_profile)"
                                                            : "hb_ground_get_field: no field map in force (hb_ground_set_field)");
  if (field_draw_follows(ctx)) {   // the device draws the records: the host image is stale
    HB_ENTER_DEVICE();
    HB_HIP(hipStreamSynchronize(ctx->s_wbc));
    HB_TRY(field_draw_refresh_host(ctx));
  }
  if (ctx->scan_on) {   // likewise the map the device scans
    HB_ENTER_DEVICE();
    HB_HIP(hipStreamSynchronize(ctx->s_wbc));
    HB_TRY(scan_refresh_host(ctx));
  }
  for (size_t i = 0; i < size_t(ctx->B); ++i) {
    const double* h = ctx->gfield_hdr_host.data() + i * GroundField::size;
    if (n_nodes) { n_nodes[2 * i] = int32_t(h[GroundField::nu]); n_nodes[2 * i + 1] = int32_t(h[GroundField::nw]); }
    if (dir) std::memcpy(dir + 2 * i, h + GroundField::dir, 2 * sizeof(double));
    if (origin) std::memcpy(origin + 2 * i, h + GroundField::org, 2 * sizeof(double));
    if (spacing) std::memcpy(spacing + 2 * i, h + GroundField::step, 2 * sizeof(double));
  }
  if (heights) std::memcpy(heights, ctx->gfield_z_host.data(), ctx->gfield_z_host.size() * sizeof(double));
  return HB_OK;
}

// The foothold configuration (include/hunter_hip.h above hb_ground_set_foothold): which forms of the planner launch_refgen takes while a
// map is in force (hb_forms.hpp use_sole_forms).  On / off changes what a range enqueues: graph_epoch, as ground_map_select.
int32_t hb_ground_set_foothold(hb_ctx* ctx, const hb_foothold_config* cfg) {
  HB_ENTER_ARGS(false);
  hb_foothold_config c{};
  if (cfg && cfg->mode != 0) {
    if (const char* why = foothold_refusal(*cfg)) {
      ctx->err = std::string("hb_ground_set_foothold: ") + why + " (the configuration in force is kept)";
      return HB_ERR_ARG;
    }
    c = *cfg;
  }
  HB_ENTER_DEVICE();
  HB_TRY(hb_sync(ctx));   // (a pass in flight still runs on the configuration it was launched with)
  if (c.mode == 1 && ctx->foothold_cfg.mode != 1) {
    SoleBatch& sb = ctx->sole;
    HB_TRY(ensure_fields(ctx, sb));
    std::vector<int32_t> none(size_t(ctx->B) * 2, RG_NO_FOOTHOLD);
    HB_TRY(push(ctx, none.data(), sb, sb.shift, whole(ctx)));
    HB_TRY(zero_field(ctx, sb, sb.defect));
    HB_TRY(zero_field(ctx, sb, sb.level));
  }
  if (c.mode != ctx->foothold_cfg.mode) ++ctx->graph_epoch;
  ctx->foothold_cfg = c;
  return HB_OK;
}

int32_t hb_ground_get_foothold(hb_ctx* ctx, hb_foothold_config* out) {
  HB_ENTER_ARGS(!out);
  *out = ctx->foothold_cfg;
  return HB_OK;
}

int32_t hb_ground_get_foothold_choice(hb_ctx* ctx, int32_t i0, int32_t cnt, int32_t* shift, double* defect, int32_t* level) {
  HB_ENTER_ARGS(!range_ok(ctx, i0, cnt, 1));
  HB_FAIL_IF(ctx->foothold_cfg.mode != 1, HB_ERR_STATE, "hb_ground_get_foothold_choice: the sole mode is off (hb_ground_set_foothold)");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  SoleBatch& sb = ctx->sole;
  const Range r{i0, cnt};
  HB_TRY(pull(ctx, shift, sb, sb.shift, r));
  HB_TRY(pull(ctx, defect, sb, sb.defect, r));
  HB_TRY(pull(ctx, level, sb, sb.level, r));
  return HB_OK;
}

}  // extern "C"
