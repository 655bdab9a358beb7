// Host side, part 10: the ground map of the controller (hb_ground_*; include/hunter_hip.h above hb_ground_set_profile).  The stored
// record of an instance, validation included, is hb_ground.hpp ground_record; the kernels that read it are the ground forms of the
// planner and the filter (launch_refgen, launch_estimator).
#pragma once

extern "C" {

int32_t hb_ground_set_profile(hb_ctx* ctx, const int32_t* n_knots, const double* dir, const double* knots) {
  HB_ENTER_ARGS(false);
  const bool on = n_knots || dir || knots;
  HB_FAIL_IF(on && !(n_knots && dir && knots), HB_ERR_ARG, "hb_ground_set_profile: give n_knots, dir and knots, or none of them to switch the map off (the map in force is kept)");
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
  if (ctx->ground_on != on) {
    ctx->ground_on = on;
    ++ctx->graph_epoch;   // (as hb_gait_reset: what a range enqueues has changed)
  }
  return HB_OK;
}

int32_t hb_ground_get_profile(hb_ctx* ctx, int32_t* n_knots, double* dir, double* knots, double* slopes) {
  HB_ENTER_ARGS(false);
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

}  // extern "C"
