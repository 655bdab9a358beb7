// Host side, part 5: the plant (hb_plant_*; pinned stub and ground-contact model).  First the static helpers the plant entries and the
// episode layer on top of them (hb_api_episode.hpp) both need, each below what it calls: joint-command state, episode record, clear
// functions, the refusals of the step and ground-model entries, level terrain, scenario and profile-draw bookkeeping, the locate of a height
// field, profile installation.  Then the entries: reset, plant_launch and the step calls, state and actuator getters, contact model and
// wrench, joint model, terrain, terrain profile, height field, model variation, sensor model and hb_plant_sense.
#pragma once

// joint command outputs and the per-instance controller flags (allocated on first use; loaded = 1, no emergency stop): the entries of
// hb_api_est.hpp own them, an episode with stop_on_fall latches the emergency stop
static int32_t joint_state_alloc(hb_ctx* ctx) {
  if (ctx->jc_out) return HB_OK;
  const size_t n = size_t(ctx->B) * HB_NJ;
  HB_HIP(dalloc(ctx, &ctx->jc_out, 6 * n));
  HB_HIP(dalloc(ctx, &ctx->jc_estop, size_t(ctx->B)));
  HB_HIP(dalloc(ctx, &ctx->jc_loaded, size_t(ctx->B)));
  std::vector<int> ones(size_t(ctx->B), 1);
  HB_HIP(hipMemcpy(ctx->jc_loaded, ones.data(), ones.size() * sizeof(int), hipMemcpyHostToDevice));
  return HB_OK;
}

// ---- per-instance episode record (include/hunter_hip.h above hb_plant_set_episode) -------------------------------------------------
// The plane the record measures heights from: the terrain records if a terrain is in force, the records of the facet under each base origin
// if a profile or a height field is (ProfileBatch::base / FieldBatch::base, the Terrain layout), else e_z . x = *d0 (ground_z in model 1, 0 in model 0).
static const double* episode_plane(const hb_ctx* ctx, double* d0) {
  *d0 = ctx->contact_cfg.mode == 1 ? ctx->contact_cfg.ground_z : 0.0;
  if (ctx->contact_cfg.mode == 1 && ctx->field_on) return ctx->field.base;
  if (ctx->contact_cfg.mode == 1 && ctx->profile_on) return ctx->profile.base;
  return ctx->contact_cfg.mode == 1 && ctx->terrain_on ? ctx->terrain.ter : nullptr;
}

// the record of every instance from the plant's present state, on s
static int32_t episode_start(hb_ctx* ctx, hipStream_t s) {
  EpisodeBatch& e = ctx->episode;
  double d0;
  const double* ter = episode_plane(ctx, &d0);
  HB_TRY(log_zero(ctx, e.trace, e.trace_cap, HB_EP_TRACE_W, &s));
  hipLaunchKernelGGL(k_plant_episode_init, dim3((ctx->B + 63) / 64), dim3(64), 0, s, e, ctx->plant, ter, d0);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

// Enqueues a plant step of length dt on s (launch(): a writer of the resident observation, resident_write) and, with an episode in force,
// the update of the record behind it: the one place every step entry point and every plant form goes through.
template <class F>
static int32_t plant_write(hb_ctx* ctx, hipStream_t s, bool fence, double dt, F&& launch) {
  if (ctx->scenario_on && (ctx->scenario_cfg.channels & HB_SC_PUSH)) {   // the scenario's push: the wrench of this step, ahead of the plant kernel
    HB_TRY(resident_write(ctx, s, fence, [&] {
      hipLaunchKernelGGL(k_plant_push, dim3((ctx->B + 63) / 64), dim3(64), 0, s, ctx->scenario, ctx->scenario_cfg, ctx->episode, ctx->contact.wrench);
      launch();
    }));
  } else {
    HB_TRY(resident_write(ctx, s, fence, launch));
  }
  if (!ctx->episode_on) return HB_OK;
  double d0;
  const double* ter = episode_plane(ctx, &d0);
  const int ground = ctx->contact_cfg.mode == 1 ? 1 : 0;
  hipLaunchKernelGGL(k_plant_episode, dim3((ctx->B + 63) / 64), dim3(64), 0, s, ctx->episode, ctx->episode_cfg, ctx->plant, ctx->contact, ctx->joints, ter,
                     d0, ground, ground && ctx->joints_on ? 1 : 0, ctx->stats.n_wbc_solves > 0 ? ctx->w.status : nullptr,
                     ctx->episode_cfg.stop_on_fall ? ctx->jc_estop : nullptr, dt);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

// ---- clear functions --------------------------------------------------------------------------------------------------------------------
// impulses, outputs and status of the ground-contact model back to zero (the wrench stays)
static int32_t contact_clear(hb_ctx* ctx, hipStream_t s) {
  ContactBatch& c = ctx->contact;
  HB_TRY(zero_field(ctx, c, c.imp, &s));
  HB_TRY(zero_field(ctx, c, c.gap, &s));
  HB_TRY(zero_field(ctx, c, c.pvel, &s));
  HB_TRY(zero_field(ctx, c, c.res, &s));
  HB_TRY(zero_field(ctx, c, c.touching, &s));
  return zero_field(ctx, c, c.status, &s);
}

// The warm start of the ground-contact model is expressed in the frame(s) of the ground of before: forgotten when the ground changes.
// On ctx->s_wbc, which is drained behind it.
static int32_t contact_forget_warm_start(hb_ctx* ctx) {
  HB_TRY(zero_field(ctx, ctx->contact, ctx->contact.imp, &ctx->s_wbc));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  return HB_OK;
}

// friction and stop impulses, outputs and status of the joint model back to zero
static int32_t joints_clear(hb_ctx* ctx, hipStream_t s) {
  JointBatch& j = ctx->joints;
  HB_TRY(zero_field(ctx, j, j.imp, &s));
  HB_TRY(zero_field(ctx, j, j.tau_applied, &s));
  HB_TRY(zero_field(ctx, j, j.friction_torque, &s));
  HB_TRY(zero_field(ctx, j, j.limit_torque, &s));
  HB_TRY(zero_field(ctx, j, j.res, &s));
  return zero_field(ctx, j, j.status, &s);
}

// Record of the last hybrid step, received command and timestamps back to zero (hb_plant_reset).  (The arrays of the actuator loop and of
// the simulator end of the LCM link are zero-filled on first use: no hybrid step, zero command, zero timestamps.)
static int32_t actuator_clear(hb_ctx* ctx, hipStream_t s) {
  ActuatorBatch& a = ctx->act;
  HB_TRY(zero_field(ctx, a, a.tau_first, &s));
  HB_TRY(zero_field(ctx, a, a.tau_mean, &s));
  for (int k = 0; k < 5; ++k) HB_TRY(zero_field(ctx, a, a.rcmd[k], &s));
  return zero_field(ctx, a, a.last_ts, &s);
}

// the totals of the respawn back to their initial values (all zero), no flag pending, "last spawned state" = the given spawn state; on s
static int32_t respawn_totals_start(hb_ctx* ctx, hipStream_t s) {
  RespawnBatch& r = ctx->respawn;
  HB_TRY(zero_field(ctx, r, r.itot, &s));
  HB_TRY(zero_field(ctx, r, r.dtot, &s));
  HB_TRY(zero_field(ctx, r, r.rg_pending, &s));
  HB_TRY(zero_field(ctx, r, r.mpc_pending, &s));
  HB_TRY(copy_field(ctx, hipMemcpyDeviceToDevice, r.q_spawn, r, r.q_last, whole(ctx), &s));
  HB_TRY(copy_field(ctx, hipMemcpyDeviceToDevice, r.v_spawn, r, r.v_last, whole(ctx), &s));
  std::lock_guard<std::mutex> lk(ctx->mtx);
  ctx->rs_rg_due = ctx->rs_mpc_due = false;
  return HB_OK;
}

// ---- what an entry checks before anything changes; `who` names it -----------------------------------------------------------------------
// the step calls
static int32_t plant_step_ready(hb_ctx* ctx, const char* who, bool need_jc, bool need_mode) {
  return refuse_state(ctx, who, !ctx->plant_ready ? "call hb_plant_reset first"
                                : need_jc && !ctx->jc_computed ? "no device-resident joint command yet (hb_joint_command after a WBC call)"
                                : need_mode && ctx->stats.n_wbc_solves == 0 ? "no device-resident contact flags yet (a WBC call)"
                                                                            : nullptr);
}
// the entry points that only exist in the ground model
static int32_t contact_ready(hb_ctx* ctx, const char* who) {
  return refuse_state(ctx, who, !ctx->plant_ready ? "call hb_plant_reset first"
                                : ctx->contact_cfg.mode != 1 ? "the ground-contact model is not in force (hb_plant_set_contact_model, mode 1)"
                                                             : nullptr);
}

// ---- level terrain ----------------------------------------------------------------------------------------------------------------------
// the level record of the contact configuration in force: T = I, d = ground_z, cfg.mu at the four points
static void terrain_level_record(const hb_ctx* ctx, double* r) {
  const hb_contact_config& K = ctx->contact_cfg;
  const double level[Terrain::size] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, K.ground_z, K.mu, K.mu, K.mu, K.mu};
  std::memcpy(r, level, sizeof level);
}

// The level record into the terrain array of every instance (allocated on first use): the step without a terrain, value for value.  With
// in_force as the terrain in force, host image included (the caller has drained ctx->s_wbc); else for the varied kernels alone, behind the
// earlier work of ctx->s_wbc (modelvar_level).
static int32_t terrain_level_install(hb_ctx* ctx, bool in_force) {
  TerrainBatch& t = ctx->terrain;
  HB_TRY(ensure_fields(ctx, t));
  std::vector<double> rec(size_t(ctx->B) * Terrain::size);
  for (size_t i = 0; i < size_t(ctx->B); ++i) terrain_level_record(ctx, rec.data() + i * Terrain::size);
  if (!in_force) HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  HB_TRY(push(ctx, rec.data(), t, t.ter, whole(ctx)));
  if (!in_force) return HB_OK;
  ctx->terrain_host = std::move(rec);
  ctx->terrain_on = true;
  return HB_OK;
}

// While a model variation is in force without a terrain, the varied kernels (the terrain forms) read the level record of the contact
// configuration in force out of the terrain array.  Called wherever the variation, the terrain or the configuration changes.
static int32_t modelvar_level(hb_ctx* ctx) {
  if (!ctx->modelvar_on || ctx->terrain_on) return HB_OK;
  return terrain_level_install(ctx, false);
}

// ---- scenario draw at respawn: what the plant entries share with hb_plant_set_scenario -----------------------------------------------------
// No finished episode logged and no push in every instance; with `rows`, scen back to "before the first draw" too.  Synchronous; the
// caller has drained ctx->s_wbc.
static int32_t scenario_start(hb_ctx* ctx, bool rows) {
  ScenarioBatch& c = ctx->scenario;
  const size_t B = ctx->B;
  std::vector<double> scen(B * HB_SC_N), psh(B * SC_PUSH);
  for (size_t i = 0; i < B; ++i) scenario_row_init(scen.data() + HB_SC_N * i, psh.data() + SC_PUSH * i);
  if (rows) HB_TRY(push(ctx, scen.data(), c, c.scen, whole(ctx)));
  HB_TRY(push(ctx, psh.data(), c, c.push, whole(ctx)));
  HB_TRY(zero_field(ctx, c, c.count));
  return log_zero(ctx, c.log, c.log_cap, HB_SC_LOG_W);
}

// The host images of the records the device has been drawing, from the device.  The caller has drained ctx->s_wbc.
static int32_t scenario_refresh_host(hb_ctx* ctx) {
  if (!ctx->scenario_on) return HB_OK;
  const int ch = ctx->scenario_cfg.channels;
  if ((ch & (HB_SC_SLOPE | HB_SC_MU)) && ctx->terrain_on) HB_TRY(pull(ctx, ctx->terrain_host.data(), ctx->terrain, ctx->terrain.ter, whole(ctx)));
  if ((ch & (HB_SC_PAYLOAD | HB_SC_MASS)) && ctx->modelvar_on) HB_TRY(pull(ctx, ctx->modelvar_host.data(), ctx->modelvar, ctx->modelvar.mdl, whole(ctx)));
  return HB_OK;
}

// Scenario off: terrain and variation stay in force as last drawn (the host images follow the device), the wrench the scenario owned is
// cleared.  The caller has drained ctx->s_wbc.
static int32_t scenario_off(hb_ctx* ctx) {
  if (!ctx->scenario_on) return HB_OK;
  HB_TRY(scenario_refresh_host(ctx));
  ctx->scenario_on = false;
  if (ctx->scenario_cfg.channels & HB_SC_PUSH) {
    HB_TRY(zero_field(ctx, ctx->contact, ctx->contact.wrench));
    ctx->contact.use_wrench = 0;
  }
  return HB_OK;
}

// ---- terrain profile and its draw at respawn: what the plant entries share with hb_plant_set_profile_draw ----------------------------------
// seg and base of every instance from the host state q[B][16]: the segment under the four contact points and the base origin, and the Terrain
// record of the facet under the base.  On s, behind its earlier work; the caller synchronises.
static int32_t profile_locate(hb_ctx* ctx, const double* q, hipStream_t s) {
  const size_t B = ctx->B;
  std::vector<int> seg(B * (HB_NC + 1));
  std::vector<double> base(B * Terrain::size);
  for (size_t i = 0; i < B; ++i) {
    const double* r = ctx->profile_host.data() + i * Profile::stored;
    double feet[12];
    plant_feet(ctx->hmodel, q + 16 * i, feet);
    for (int c = 0; c < HB_NC + 1; ++c) seg[(HB_NC + 1) * i + c] = profile_segment(r, c < HB_NC ? feet + 3 * c : q + 16 * i);
    double* b = base.data() + Terrain::size * i;
    std::memcpy(b, r + Profile::head, Terrain::size * sizeof(double));
    std::memcpy(b, r + Profile::seg + Profile::rec * seg[(HB_NC + 1) * i + HB_NC], Profile::rec * sizeof(double));
  }
  HB_HIP(hipStreamSynchronize(s));
  ProfileBatch& t = ctx->profile;
  HB_TRY(push(ctx, seg.data(), t, t.seg, whole(ctx)));
  return push(ctx, base.data(), t, t.base, whole(ctx));
}

// ---- height field: what the plant entries share ---------------------------------------------------------------------------------------------
// sel and base of every instance from the host state q[B][16]: the facet under the four contact points and the base origin, and the Terrain
// record of the facet under the base.  On s, behind its earlier work; the caller synchronises.
static int32_t field_locate(hb_ctx* ctx, const double* q, hipStream_t s) {
  const size_t B = ctx->B;
  std::vector<int> sel(B * (HB_NC + 1));
  std::vector<double> base(B * Terrain::size);
  for (size_t i = 0; i < B; ++i) {
    const double* r = ctx->field_hdr_host.data() + i * Field::stored;
    const double* z = ctx->field_z_host.data() + i * Field::nz;
    double feet[12], rec[Profile::rec];
    plant_feet(ctx->hmodel, q + 16 * i, feet);
    double* b = base.data() + Terrain::size * i;
    std::memcpy(b, r + Field::head, Terrain::size * sizeof(double));
    for (int c = 0; c < HB_NC + 1; ++c) sel[(HB_NC + 1) * i + c] = field_facet(r, z, c < HB_NC ? feet + 3 * c : q + 16 * i, c < HB_NC ? rec : b);
  }
  HB_HIP(hipStreamSynchronize(s));
  FieldBatch& t = ctx->field;
  HB_TRY(push(ctx, sel.data(), t, t.sel, whole(ctx)));
  return push(ctx, base.data(), t, t.base, whole(ctx));
}

// No finished episode logged in every instance; with `rows`, the parameter rows back to "before the first draw" (zero) too.  Synchronous;
// the caller has drained ctx->s_wbc.
static int32_t profile_draw_start(hb_ctx* ctx, bool rows) {
  ProfileDrawBatch& d = ctx->profile_draw;
  if (rows) HB_TRY(zero_field(ctx, d, d.row));
  HB_TRY(zero_field(ctx, d, d.count));
  return log_zero(ctx, d.log, d.log_cap, HB_PD_LOG_W);
}

// The host images of the records the device has been drawing, from the device: the profile's records and knots and, where the map
// follows, the map's (its knots as given are its breakpoints and heights).  The caller has drained ctx->s_wbc.
static int32_t profile_draw_refresh_host(hb_ctx* ctx) {
  if (!ctx->profile_draw_on) return HB_OK;
  HB_TRY(pull(ctx, ctx->profile_host.data(), ctx->profile, ctx->profile.prof, whole(ctx)));
  HB_TRY(pull(ctx, ctx->profile_knots.data(), ctx->profile_draw, ctx->profile_draw.knots, whole(ctx)));
  if (!(ctx->profile_draw_cfg.follow_map && ctx->ground_on)) return HB_OK;
  HB_TRY(pull(ctx, ctx->ground_host.data(), ctx->ground, ctx->ground.map, whole(ctx)));
  for (size_t i = 0; i < size_t(ctx->B); ++i) {
    const double* r = ctx->ground_host.data() + i * Ground::size;
    double* k = ctx->ground_knots.data() + i * PD_KNOTS;
    const int K = int(r[Ground::nseg]) + 1;
    for (int j = 0; j < HB_PROFILE_MAX_KNOTS; ++j) {
      k[2 * j] = j < K ? r[Ground::brk + j] : 0.0;
      k[2 * j + 1] = j < K ? r[Ground::hgt + j] : 0.0;
    }
  }
  return HB_OK;
}

// Draw off: profile and map stay in force as last drawn (the host images follow the device).  The caller has drained ctx->s_wbc.
static int32_t profile_draw_off(hb_ctx* ctx) {
  if (!ctx->profile_draw_on) return HB_OK;
  HB_TRY(profile_draw_refresh_host(ctx));
  ctx->profile_draw_on = false;
  return HB_OK;
}

// Installs the profile records rec[B][Profile::stored] and their knots as given, kn, as the ground in force: records to the device, host
// images, the facets under the plant's present state, one ground at a time (the profile replaces a terrain), no warm start from the ground
// of before.  With `drawn` the knots go to the draw's device copy too; with a map (grec: its records, grel: its knots as given) the ground
// map of the controller follows.  The caller has drained ctx->s_wbc; rec, kn, *grec and *grel are moved from.
static int32_t profile_install(hb_ctx* ctx, std::vector<double>& rec, std::vector<double>& kn, bool drawn, std::vector<double>* grec = nullptr,
                               std::vector<double>* grel = nullptr) {
  ProfileBatch& t = ctx->profile;
  HB_TRY(ensure_fields(ctx, t));
  HB_TRY(push(ctx, rec.data(), t, t.prof, whole(ctx)));
  if (drawn) HB_TRY(push(ctx, kn.data(), ctx->profile_draw, ctx->profile_draw.knots, whole(ctx)));
  ctx->profile_host = std::move(rec);
  ctx->profile_knots = std::move(kn);
  if (grec) {
    HB_TRY(hb_sync(ctx));   // (a pass in flight on the MPC stream still runs on the map it was launched with)
    HB_TRY(push(ctx, grec->data(), ctx->ground, ctx->ground.map, whole(ctx)));
    ctx->ground_host = std::move(*grec);
    ctx->ground_knots = std::move(*grel);
  }
  std::vector<double> q(size_t(ctx->B) * 16);
  HB_TRY(pull(ctx, q.data(), ctx->plant, ctx->plant.q, whole(ctx)));
  HB_TRY(profile_locate(ctx, q.data(), ctx->s_wbc));
  ctx->terrain_on = false;
  ctx->field_on = false;
  ctx->profile_on = true;
  HB_TRY(modelvar_level(ctx));
  return contact_forget_warm_start(ctx);
}

// ---- field draw at respawn: what the plant entries share with hb_plant_set_field_draw ------------------------------------------------------
// No finished episode logged in every instance; with `rows`, the parameter rows back to "before the first draw" (zero) too.  Synchronous;
// the caller has drained ctx->s_wbc.
static int32_t field_draw_start(hb_ctx* ctx, bool rows) {
  FieldDrawBatch& d = ctx->field_draw;
  if (rows) HB_TRY(zero_field(ctx, d, d.row));
  HB_TRY(zero_field(ctx, d, d.count));
  return log_zero(ctx, d.log, d.log_cap, HB_FD_LOG_W);
}

// whether the controller's field map follows the draw in force
static bool field_draw_follows(const hb_ctx* ctx) { return ctx->field_draw_on && ctx->field_draw_cfg.follow_map && ctx->gfield_on; }

// The host images of the records the device has been drawing, from the device: the field's headers and heights and, where the map
// follows, the map's.  The caller has drained ctx->s_wbc.
static int32_t field_draw_refresh_host(hb_ctx* ctx) {
  if (!ctx->field_draw_on) return HB_OK;
  HB_TRY(pull(ctx, ctx->field_hdr_host.data(), ctx->field, ctx->field.hdr, whole(ctx)));
  HB_TRY(pull(ctx, ctx->field_z_host.data(), ctx->field, ctx->field.z, whole(ctx)));
  if (!field_draw_follows(ctx)) return HB_OK;
  HB_TRY(pull(ctx, ctx->gfield_hdr_host.data(), ctx->gfield, ctx->gfield.hdr, whole(ctx)));
  return pull(ctx, ctx->gfield_z_host.data(), ctx->gfield, ctx->gfield.z, whole(ctx));
}

// Draw off: field and map stay in force as last drawn (the host images follow the device).  The caller has drained ctx->s_wbc.
static int32_t field_draw_off(hb_ctx* ctx) {
  if (!ctx->field_draw_on) return HB_OK;
  HB_TRY(field_draw_refresh_host(ctx));
  ctx->field_draw_on = false;
  return HB_OK;
}

// ---- height scan: what the plant and ground entries share with hb_plant_set_height_scan ---------------------------------------------------
// The host images of the field map the device has been scanning, from the device.  The caller has drained ctx->s_wbc.
static int32_t scan_refresh_host(hb_ctx* ctx) {
  if (!(ctx->scan_on && ctx->gfield_on)) return HB_OK;
  HB_TRY(pull(ctx, ctx->gfield_hdr_host.data(), ctx->gfield, ctx->gfield.hdr, whole(ctx)));
  return pull(ctx, ctx->gfield_z_host.data(), ctx->gfield, ctx->gfield.z, whole(ctx));
}
// Scan off: the map stays in force as last written (the host images follow the device).  The caller has drained ctx->s_wbc.
static int32_t scan_off(hb_ctx* ctx) {
  if (!ctx->scan_on) return HB_OK;
  HB_TRY(scan_refresh_host(ctx));
  ctx->scan_on = false;
  return HB_OK;
}
// every instance's map counts as cleared from here on (ScanBatch::episode_seen below zero), on s
static int32_t scan_mark_cleared(hb_ctx* ctx, hipStream_t s) {
  HB_HIP(hipMemsetAsync(ctx->scan.episode_seen, 0xFF, size_t(ctx->B) * sizeof(int), s));
  return HB_OK;
}

// Installs the field records hdr[B][Field::stored] and heights z[B][Field::nz] as the ground in force: records to the device, host images,
// the facets under the plant's present state, one ground at a time (the field replaces a terrain and a profile), no warm start from the
// ground of before.  With a map (ghdr, gz) the field map of the controller follows.  The caller has drained ctx->s_wbc; the vectors are
// moved from.
static int32_t field_install(hb_ctx* ctx, std::vector<double>& hdr, std::vector<double>& z, std::vector<double>* ghdr = nullptr,
                             std::vector<double>* gz = nullptr) {
  FieldBatch& t = ctx->field;
  HB_TRY(ensure_fields(ctx, t));
  HB_TRY(push(ctx, hdr.data(), t, t.hdr, whole(ctx)));
  HB_TRY(push(ctx, z.data(), t, t.z, whole(ctx)));
  ctx->field_hdr_host = std::move(hdr);
  ctx->field_z_host = std::move(z);
  if (ghdr) {
    HB_TRY(hb_sync(ctx));   // (a pass in flight on the MPC stream still runs on the map it was launched with)
    HB_TRY(push(ctx, ghdr->data(), ctx->gfield, ctx->gfield.hdr, whole(ctx)));
    HB_TRY(push(ctx, gz->data(), ctx->gfield, ctx->gfield.z, whole(ctx)));
    ctx->gfield_hdr_host = std::move(*ghdr);
    ctx->gfield_z_host = std::move(*gz);
  }
  std::vector<double> q(size_t(ctx->B) * 16);
  HB_TRY(pull(ctx, q.data(), ctx->plant, ctx->plant.q, whole(ctx)));
  HB_TRY(field_locate(ctx, q.data(), ctx->s_wbc));
  ctx->terrain_on = false;   // one ground at a time: the field replaces a terrain and a profile
  ctx->profile_on = false;
  ctx->field_on = true;
  HB_TRY(modelvar_level(ctx));
  return contact_forget_warm_start(ctx);
}

extern "C" {

int32_t hb_plant_reset(hb_ctx* ctx, const double* q0, const double* v0, double baumgarte, double eps) {
  HB_ENTER(!q0 || !(baumgarte >= 0.0) || !(eps >= 0.0));
  PlantBatch& p = ctx->plant;
  HB_TRY(ensure_fields(ctx, p));
  ctx->sensed = false;
  p.baum = baumgarte;
  p.eps = eps;
  HB_TRY(push(ctx, q0, p, p.q, whole(ctx)));
  if (v0) HB_TRY(push(ctx, v0, p, p.v, whole(ctx)));
  else HB_TRY(zero_field(ctx, p, p.v));
  hipLaunchKernelGGL(k_plant_reset, dim3((ctx->B + 63) / 64), dim3(64), 0, ctx->s_wbc, p, ctx->dmodel);
  HB_HIP(hipGetLastError());
  if (has_fields(ctx, ctx->contact)) HB_TRY(contact_clear(ctx, ctx->s_wbc));
  if (has_fields(ctx, ctx->joints)) HB_TRY(joints_clear(ctx, ctx->s_wbc));
  if (has_fields(ctx, ctx->act)) HB_TRY(actuator_clear(ctx, ctx->s_wbc));
  if (ctx->profile_draw_on) {   // the device draws the records: the host image the locate reads is stale
    HB_HIP(hipStreamSynchronize(ctx->s_wbc));
    HB_TRY(profile_draw_refresh_host(ctx));
  }
  if (ctx->field_draw_on) {   // likewise the field the device draws
    HB_HIP(hipStreamSynchronize(ctx->s_wbc));
    HB_TRY(field_draw_refresh_host(ctx));
  }
  if (ctx->profile_on) HB_TRY(profile_locate(ctx, q0, ctx->s_wbc));   // the facets under the reset state
  if (ctx->field_on) HB_TRY(field_locate(ctx, q0, ctx->s_wbc));
  if (ctx->episode_on) HB_TRY(episode_start(ctx, ctx->s_wbc));   // the record restarts from the reset state
  if (ctx->respawn_on) HB_TRY(respawn_totals_start(ctx, ctx->s_wbc));   // ... and so do the totals of the respawn
  if (ctx->scan_on) HB_TRY(scan_mark_cleared(ctx, ctx->s_wbc));         // the first scan of the reset plant starts from an empty map
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  if (ctx->scenario_on) HB_TRY(scenario_start(ctx, false));   // the log is empty, nobody has a push; terrain, models and scen stay as last drawn
  if (ctx->profile_draw_on) HB_TRY(profile_draw_start(ctx, false));   // the log is empty; profile, map and rows stay as last drawn
  if (ctx->field_draw_on) HB_TRY(field_draw_start(ctx, false));       // ... and so do field, map and rows of a field draw
  ctx->plant_ready = true;
  return HB_OK;
}

// A step of the plant form in force (hb_forms.hpp plant_form), behind plant_write.  The drive is the held device torque dtau, or with cmd
// the five device arrays of the hybrid actuator (pos_des vel_des kp kd ff, [B][10] each); contact: host flags or null.  Each form's launch
// names its kernel and the arguments ahead of the tail every step kernel ends with.
static int32_t plant_launch(hb_ctx* ctx, const double* dtau, const double* const* cmd, const int32_t* contact, double dt, int32_t substeps,
                            int32_t to_resident) {
  PlantBatch& p = ctx->plant;
  hipStream_t s = ctx->s_wbc;  // the plant follows the control thread
  HB_TRY(push(ctx, contact, p, p.contact, whole(ctx), &s));
  const ActuatorCmd c = cmd ? ActuatorCmd{{cmd[0], cmd[1], cmd[2], cmd[3], cmd[4]}} : ActuatorCmd{};
  const int* dcontact = contact ? p.contact : nullptr;
  // the resident observation feeds the next hb_mpc_solve(NULL) / hb_refgen_update(NULL) on the MPC stream
  double* rr = to_resident ? ctx->w.rbd : nullptr;
  double* rx = to_resident ? ctx->b.x0 : nullptr;
  double* rt = to_resident ? ctx->w.t_now : nullptr;
  const DevModel* mvar = ctx->modelvar_on ? ctx->modelvar.mdl : nullptr;   // (the profile forms take the variation by pointer)
  auto go = [&](auto kernel, const auto&... lead) {
    return plant_write(ctx, s, to_resident, dt, [&] {
      hipLaunchKernelGGL(kernel, dim3(ctx->B), dim3(64), 0, s, lead..., dcontact, ctx->w.mode, dt, substeps, rr, rx, rt);
    });
  };
  const ContactBatch& cb = ctx->contact;
  const JointBatch& jb = ctx->joints;
  const ActuatorBatch& a = ctx->act;
  const double* ter = ctx->terrain.ter;
  const hb_contact_config& K = ctx->contact_cfg;
  const hb_joint_model& J = ctx->joint_model;
  const DevModel* M = ctx->dmodel;
  const PlantForm f = plant_form(K.mode, ctx->joints_on, ctx->terrain_on, ctx->modelvar_on, ctx->profile_on, cmd != nullptr, ctx->field_on);
  switch (f.ground) {
    case PlantForm::Ground::Pinned:
      return f.hybrid ? go(k_plant_hybrid, p, a, c, M) : go(k_plant, p, M, dtau);
    case PlantForm::Ground::Level:
      if (f.hybrid) return f.joints ? go(k_plant_joints_hybrid, p, cb, jb, a, c, K, J, M) : go(k_plant_contact_hybrid, p, cb, a, c, K, M);
      return f.joints ? go(k_plant_joints, p, cb, jb, K, J, M, dtau) : go(k_plant_contact, p, cb, K, M, dtau);
    case PlantForm::Ground::Terrain:
      if (f.hybrid) return f.joints ? go(k_plant_terrain_joints_hybrid, p, cb, jb, ter, a, c, K, J, M) : go(k_plant_terrain_hybrid, p, cb, ter, a, c, K, M);
      return f.joints ? go(k_plant_terrain_joints, p, cb, jb, ter, K, J, M, dtau) : go(k_plant_terrain, p, cb, ter, K, M, dtau);
    case PlantForm::Ground::Varied:
      if (f.hybrid) return f.joints ? go(k_plant_varied_joints_hybrid, p, cb, jb, ter, a, c, K, J, M, mvar) : go(k_plant_varied_hybrid, p, cb, ter, a, c, K, M, mvar);
      return f.joints ? go(k_plant_varied_joints, p, cb, jb, ter, K, J, M, mvar, dtau) : go(k_plant_varied, p, cb, ter, K, M, mvar, dtau);
    case PlantForm::Ground::Profile:
      if (f.hybrid) return f.joints ? go(k_plant_profile_joints_hybrid, p, cb, jb, ctx->profile, a, c, K, J, M, mvar) : go(k_plant_profile_hybrid, p, cb, ctx->profile, a, c, K, M, mvar);
      return f.joints ? go(k_plant_profile_joints, p, cb, jb, ctx->profile, K, J, M, mvar, dtau) : go(k_plant_profile, p, cb, ctx->profile, K, M, mvar, dtau);
    case PlantForm::Ground::Field:
      if (f.hybrid) return f.joints ? go(k_plant_field_joints_hybrid, p, cb, jb, ctx->field, a, c, K, J, M, mvar) : go(k_plant_field_hybrid, p, cb, ctx->field, a, c, K, M, mvar);
      return f.joints ? go(k_plant_field_joints, p, cb, jb, ctx->field, K, J, M, mvar, dtau) : go(k_plant_field, p, cb, ctx->field, K, M, mvar, dtau);
  }
  return HB_ERR_STATE;   // (not reached: the switch covers PlantForm::Ground)
}

int32_t hb_plant_step(hb_ctx* ctx, const double* tau, const int32_t* contact, double dt, int32_t substeps, int32_t to_resident) {
  HB_ENTER_ARGS(!(dt > 0.0) || substeps < 1);
  HB_FAIL_IF(!ctx->plant_ready, HB_ERR_STATE, "hb_plant_step: call hb_plant_reset first");
  HB_FAIL_IF((!tau && !ctx->jc_computed) || (!contact && ctx->stats.n_wbc_solves == 0), HB_ERR_STATE, "hb_plant_step: no device-resident torque / contact flags yet (hb_joint_command after a WBC call)");
  HB_ENTER_DEVICE();
  PlantBatch& p = ctx->plant;
  HB_TRY(push(ctx, tau, p, p.tau, whole(ctx), &ctx->s_wbc));
  return plant_launch(ctx, tau ? p.tau : ctx->jc_out + 5 * size_t(ctx->B) * HB_NJ, nullptr, contact, dt, substeps, to_resident);
}

int32_t hb_plant_step_hybrid(hb_ctx* ctx, const double* pos_des, const double* vel_des, const double* kp, const double* kd, const double* tau_ff,
                             const int32_t* contact, double dt, int32_t substeps, int32_t to_resident) {
  const double* const host[5] = {pos_des, vel_des, kp, kd, tau_ff};
  int given = 0;
  for (const double* h : host) given += h ? 1 : 0;
  HB_ENTER_ARGS(!(dt > 0.0) || substeps < 1);
  HB_FAIL_IF(given != 0 && given != 5, HB_ERR_ARG, "hb_plant_step_hybrid: give all five command arrays, or none for the device-resident command of hb_joint_command");
  HB_TRY(plant_step_ready(ctx, "hb_plant_step_hybrid", given == 0, !contact));
  HB_ENTER_DEVICE();
  ActuatorBatch& a = ctx->act;
  HB_TRY(ensure_fields(ctx, a));
  const size_t n = size_t(ctx->B) * HB_NJ;
  const double* cmd[5];
  for (int k = 0; k < 5; ++k) {
    HB_TRY(push(ctx, host[k], a, a.cmd[k], whole(ctx), &ctx->s_wbc));
    cmd[k] = given ? a.cmd[k] : ctx->jc_out + k * n;   // planes 0-4 of the joint command: posDes velDes kp kd ff
  }
  return plant_launch(ctx, nullptr, cmd, contact, dt, substeps, to_resident);
}

int32_t hb_plant_get_actuator(hb_ctx* ctx, double* tau_first, double* tau_mean, int64_t* last_timestamp) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->plant_ready, HB_ERR_STATE, "hb_plant_get_actuator: call hb_plant_reset first");
  HB_ENTER_DEVICE();
  ActuatorBatch& a = ctx->act;
  HB_TRY(ensure_fields(ctx, a));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  HB_TRY(pull(ctx, tau_first, a, a.tau_first, whole(ctx)));
  HB_TRY(pull(ctx, tau_mean, a, a.tau_mean, whole(ctx)));
  HB_TRY(pull(ctx, last_timestamp, a, a.last_ts, whole(ctx)));
  return HB_OK;
}

int32_t hb_plant_get_state(hb_ctx* ctx, double* q, double* v, double* rbd, double* lambda, double* vdot) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->plant_ready, HB_ERR_STATE, "hb_plant_get_state: call hb_plant_reset first");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  PlantBatch& p = ctx->plant;
  HB_TRY(pull(ctx, q, p, p.q, whole(ctx)));
  HB_TRY(pull(ctx, v, p, p.v, whole(ctx)));
  HB_TRY(pull(ctx, rbd, p, p.rbd, whole(ctx)));
  HB_TRY(pull(ctx, lambda, p, p.lambda, whole(ctx)));
  HB_TRY(pull(ctx, vdot, p, p.vdot, whole(ctx)));
  return HB_OK;
}

// ---- ground-contact model, external wrench, joint model ------------------------------------------------------------------------------------
int32_t hb_plant_set_contact_model(hb_ctx* ctx, const hb_contact_config* cfg) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->plant_ready, HB_ERR_STATE, "hb_plant_set_contact_model: call hb_plant_reset first");
  HB_FAIL_IF(cfg && !contact_config_valid(*cfg), HB_ERR_ARG, "hb_plant_set_contact_model: mode 0 / 1, sweeps 1 .. 10000, mu >= 0, erp in [0, 1], tol >= 0, fall_height >= 0, every field finite and `reserved` 0");
  HB_FAIL_IF(cfg && cfg->mode == 1 && ctx->profile_draw_on && !(std::fabs(cfg->ground_z) <= PD_REACH), HB_ERR_ARG, "hb_plant_set_contact_model: |ground_z| above 1e3 while a profile draw is in force (hb_plant_set_profile_draw): its knots are drawn around ground_z");
  HB_FAIL_IF(cfg && cfg->mode == 1 && ctx->field_draw_on && !(std::fabs(cfg->ground_z) <= FD_REACH), HB_ERR_ARG, "hb_plant_set_contact_model: |ground_z| above 1e3 while a field draw is in force (hb_plant_set_field_draw): its heights are drawn around ground_z");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));  // (a step in flight still runs under the model it was launched with)
  const bool ground = cfg && cfg->mode == 1;
  bool fresh = false;
  if (ground) HB_TRY(ensure_fields(ctx, ctx->contact, &fresh));
  if (ground && !fresh && ctx->contact_cfg.mode != 1) HB_TRY(contact_clear(ctx, ctx->s_wbc));  // back from the pinned stub: no warm start from before it
  if (!ground && ctx->contact_cfg.mode == 1) {
    // the ground model moved the feet without touching the stub's anchors: no point counts as pinned, so the next step of the stub
    // anchors every commanded contact where the foot is now
    HB_TRY(zero_field(ctx, ctx->plant, ctx->plant.pinned, &ctx->s_wbc));
  }
  if (!ground) HB_TRY(scenario_off(ctx));   // the scenario belongs to contact model 1 (and gives the wrench back)
  if (!ground) HB_TRY(profile_draw_off(ctx));   // ... and so does the profile draw
  if (!ground) HB_TRY(field_draw_off(ctx));     // ... and the field draw
  if (!ground) HB_TRY(scan_off(ctx));           // ... and the height scan
  ctx->contact_cfg = ground ? *cfg : hb_contact_config{};
  if (!ground) ctx->terrain_on = false;   // the terrain belongs to contact model 1
  if (!ground) ctx->profile_on = false;   // ... and so does the terrain profile
  if (!ground) ctx->field_on = false;     // ... and the height field
  if (!ground) ctx->modelvar_on = false;  // ... and so does the model variation
  HB_TRY(modelvar_level(ctx));            // (the level record follows the configuration)
  if (!ground && ctx->joints_on) {   // the joint model belongs to contact model 1
    ctx->joints_on = false;
    HB_TRY(joints_clear(ctx, ctx->s_wbc));
  }
  return HB_OK;
}

int32_t hb_plant_set_external_wrench(hb_ctx* ctx, const double* wrench) {
  HB_ENTER_ARGS(false);
  HB_TRY(contact_ready(ctx, "hb_plant_set_external_wrench"));
  HB_FAIL_IF(ctx->scenario_on && (ctx->scenario_cfg.channels & HB_SC_PUSH), HB_ERR_STATE, "hb_plant_set_external_wrench: the scenario in force owns the wrench (hb_plant_set_scenario with HB_SC_PUSH)");
  HB_ENTER_DEVICE();
  ContactBatch& c = ctx->contact;
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));  // (an earlier step may still be reading the wrench)
  HB_TRY(push(ctx, wrench, c, c.wrench, whole(ctx)));
  c.use_wrench = wrench ? 1 : 0;
  return HB_OK;
}

int32_t hb_plant_get_contact(hb_ctx* ctx, double* gap, double* point_vel, double* residual, int32_t* touching, int32_t* status) {
  HB_ENTER_ARGS(false);
  HB_TRY(contact_ready(ctx, "hb_plant_get_contact"));
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  ContactBatch& c = ctx->contact;
  HB_TRY(pull(ctx, gap, c, c.gap, whole(ctx)));
  HB_TRY(pull(ctx, point_vel, c, c.pvel, whole(ctx)));
  HB_TRY(pull(ctx, residual, c, c.res, whole(ctx)));
  HB_TRY(pull(ctx, touching, c, c.touching, whole(ctx)));
  HB_TRY(pull(ctx, status, c, c.status, whole(ctx)));
  return HB_OK;
}

int32_t hb_plant_set_joint_model(hb_ctx* ctx, const hb_joint_model* model) {
  HB_ENTER_ARGS(false);
  HB_TRY(contact_ready(ctx, "hb_plant_set_joint_model"));
  HB_FAIL_IF(model && !joint_model_valid(*model), HB_ERR_ARG, "hb_plant_set_joint_model: armature, damping, frictionloss >= 0, lower < upper, torque_limit > 0 (+inf allowed), limit_erp in [0, 1], tol >= 0, limits 0 / 1, every other field finite and `reserved` 0");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));  // (a step in flight still runs under the model it was launched with)
  bool fresh = false;
  if (model) HB_TRY(ensure_fields(ctx, ctx->joints, &fresh));
  if (model && !fresh && !ctx->joints_on) HB_TRY(joints_clear(ctx, ctx->s_wbc));  // back from ideal joints: no warm start from before them
  if (!model && ctx->joints_on) HB_TRY(joints_clear(ctx, ctx->s_wbc));  // ideal joints again: the outputs read zero
  if (model) ctx->joint_model = *model;
  ctx->joints_on = model != nullptr;
  return HB_OK;
}

int32_t hb_plant_get_joints(hb_ctx* ctx, double* tau_applied, double* friction_torque, double* limit_torque, double* residual, int32_t* status) {
  HB_ENTER_ARGS(false);
  HB_TRY(contact_ready(ctx, "hb_plant_get_joints"));
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  JointBatch& j = ctx->joints;
  if (!has_fields(ctx, j)) {  // no joint model was ever set: the outputs are zero
    const size_t B = ctx->B;
    double* const outs[3] = {tau_applied, friction_torque, limit_torque};
    for (double* o : outs)
      if (o) std::memset(o, 0, B * HB_NJ * 8);
    if (residual) std::memset(residual, 0, B * 8);
    if (status) std::memset(status, 0, B * sizeof(int32_t));
    return HB_OK;
  }
  HB_TRY(pull(ctx, tau_applied, j, j.tau_applied, whole(ctx)));
  HB_TRY(pull(ctx, friction_torque, j, j.friction_torque, whole(ctx)));
  HB_TRY(pull(ctx, limit_torque, j, j.limit_torque, whole(ctx)));
  HB_TRY(pull(ctx, residual, j, j.res, whole(ctx)));
  HB_TRY(pull(ctx, status, j, j.status, whole(ctx)));
  return HB_OK;
}

// ---- per-instance terrain of contact model 1 (include/hunter_hip.h above hb_plant_set_terrain) ----------------------------------------
// (the stored record of a plane — normalisation and the frame T — is hb_contact.hpp terrain_plane_record, shared with k_plant_scenario)
int32_t hb_plant_set_terrain(hb_ctx* ctx, const double* plane, const double* mu) {
  HB_ENTER_ARGS(false);
  HB_TRY(contact_ready(ctx, "hb_plant_set_terrain"));
  HB_FAIL_IF(!plane && !mu && ctx->scenario_on && (ctx->scenario_cfg.channels & (HB_SC_SLOPE | HB_SC_MU)), HB_ERR_STATE, "hb_plant_set_terrain: the scenario in force draws the terrain (hb_plant_set_scenario): turn it off first");
  HB_FAIL_IF(ctx->profile_draw_on, HB_ERR_STATE, "hb_plant_set_terrain: the profile draw in force draws the ground (hb_plant_set_profile_draw): turn it off first");
  HB_FAIL_IF(ctx->field_draw_on, HB_ERR_STATE, "hb_plant_set_terrain: the field draw in force draws the ground (hb_plant_set_field_draw): turn it off first");
  const size_t B = ctx->B;
  std::vector<double> rec(B * Terrain::size);
  for (size_t i = 0; i < B && (plane || mu); ++i) {
    double* r = rec.data() + i * Terrain::size;
    const char* why = nullptr;
    if (plane) {
      const double* pl = plane + 4 * i;
      const double len = terrain_normal_length(pl);
      if (!(std::isfinite(pl[0]) && std::isfinite(pl[1]) && std::isfinite(pl[2]) && std::isfinite(pl[3]))) why = "a non-finite plane entry";
      else if (!(std::fabs(len - 1.0) <= 1e-9)) why = "a normal that is not of unit length (| |n| - 1 | > 1e-9)";
      else if (!(pl[2] / len >= 0.5)) why = "n_z < 0.5";
      if (!why) terrain_plane_record(pl, len, r);
    } else {   // (the frame of e_z as terrain_frame stores it: signed zeros where terrain_level_record has plain ones, kept bit for bit)
      const double n[3] = {0.0, 0.0, 1.0};
      terrain_frame(n, r + Terrain::T);
      r[Terrain::d] = ctx->contact_cfg.ground_z;
    }
    for (int c = 0; c < HB_NC && !why; ++c) {
      const double m = mu ? mu[4 * i + c] : ctx->contact_cfg.mu;
      if (!(std::isfinite(m) && m >= 0.0)) why = "a friction coefficient that is negative or not finite";
      r[Terrain::mu + c] = m;
    }
    if (why) return refuse_instance(ctx, HB_ERR_ARG, "hb_plant_set_terrain", i, why, "terrain");
  }
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));  // (a step in flight still runs on the terrain it was launched with)
  if (plane || mu) {
    TerrainBatch& t = ctx->terrain;
    HB_TRY(ensure_fields(ctx, t));
    HB_TRY(push(ctx, rec.data(), t, t.ter, whole(ctx)));
    ctx->terrain_host = std::move(rec);
  }
  ctx->terrain_on = plane || mu;
  ctx->profile_on = false;   // one ground at a time: the call replaces a terrain profile
  ctx->field_on = false;     // ... and a height field
  HB_TRY(modelvar_level(ctx));
  return contact_forget_warm_start(ctx);
}

int32_t hb_plant_get_terrain(hb_ctx* ctx, double* plane, double* mu, double* frame) {
  HB_ENTER_ARGS(false);
  HB_TRY(contact_ready(ctx, "hb_plant_get_terrain"));
  if (ctx->scenario_on) {   // the device draws the records: the host image is stale
    HB_ENTER_DEVICE();
    HB_HIP(hipStreamSynchronize(ctx->s_wbc));
    HB_TRY(scenario_refresh_host(ctx));
  }
  for (size_t i = 0; i < size_t(ctx->B); ++i) {
    double r[Terrain::size];
    terrain_level_record(ctx, r);
    if (ctx->terrain_on) std::memcpy(r, ctx->terrain_host.data() + i * Terrain::size, sizeof r);
    if (plane) { for (int a = 0; a < 3; ++a) plane[4 * i + a] = r[Terrain::T + 3 * a + 2]; plane[4 * i + 3] = r[Terrain::d]; }
    if (mu) std::memcpy(mu + 4 * i, r + Terrain::mu, 4 * sizeof(double));
    if (frame) std::memcpy(frame + 9 * i, r + Terrain::T, 9 * sizeof(double));
  }
  return HB_OK;
}

// ---- per-instance terrain profile of contact model 1 (include/hunter_hip.h above hb_plant_set_terrain_profile) ------------------------
// (the stored record of an instance, validation included, is hb_contact.hpp profile_record)
int32_t hb_plant_set_terrain_profile(hb_ctx* ctx, const int32_t* n_knots, const double* dir, const double* knots, const double* mu) {
  HB_ENTER_ARGS(false);
  HB_TRY(contact_ready(ctx, "hb_plant_set_terrain_profile"));
  const bool on = n_knots || dir || knots;
  HB_FAIL_IF(on && !(n_knots && dir && knots), HB_ERR_ARG, "hb_plant_set_terrain_profile: give n_knots, dir and knots, or none of them to switch the profile off (the profile in force is kept)");
  HB_FAIL_IF(!on && mu, HB_ERR_ARG, "hb_plant_set_terrain_profile: friction coefficients without a profile (the profile in force is kept)");
  HB_FAIL_IF(ctx->profile_draw_on, HB_ERR_STATE, "hb_plant_set_terrain_profile: the profile draw in force draws the ground (hb_plant_set_profile_draw): turn it off first");
  HB_FAIL_IF(ctx->field_draw_on, HB_ERR_STATE, "hb_plant_set_terrain_profile: the field draw in force draws the ground (hb_plant_set_field_draw): turn it off first");
  HB_FAIL_IF(on && ctx->respawn_on, HB_ERR_STATE, "hb_plant_set_terrain_profile: a respawn configuration is in force (hb_plant_set_respawn): no respawn on a profile, turn it off first");
  HB_FAIL_IF(on && ctx->scenario_on && (ctx->scenario_cfg.channels & (HB_SC_SLOPE | HB_SC_MU)), HB_ERR_STATE, "hb_plant_set_terrain_profile: the scenario in force draws the terrain (hb_plant_set_scenario): turn it off first");
  const size_t B = ctx->B;
  std::vector<double> rec(on ? B * Profile::stored : 0), kn(on ? B * HB_PROFILE_MAX_KNOTS * 2 : 0);
  for (size_t i = 0; i < B && on; ++i) {
    const double* k = knots + i * HB_PROFILE_MAX_KNOTS * 2;
    if (const char* why = profile_record(n_knots[i], dir + 2 * i, k, mu ? mu + 4 * i : nullptr, ctx->contact_cfg.mu, rec.data() + i * Profile::stored))
      return refuse_instance(ctx, HB_ERR_ARG, "hb_plant_set_terrain_profile", i, why, "profile");
    std::memcpy(kn.data() + i * HB_PROFILE_MAX_KNOTS * 2, k, size_t(n_knots[i]) * 2 * sizeof(double));
  }
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));  // (a step in flight still runs on the ground it was launched with)
  if (on) return profile_install(ctx, rec, kn, false);
  ctx->profile_on = false;
  HB_TRY(modelvar_level(ctx));
  return contact_forget_warm_start(ctx);
}

int32_t hb_plant_get_terrain_profile(hb_ctx* ctx, int32_t* n_knots, double* dir, double* knots, double* mu, double* records, int32_t* segment) {
  HB_ENTER_ARGS(false);
  HB_TRY(contact_ready(ctx, "hb_plant_get_terrain_profile"));
  HB_FAIL_IF(!ctx->profile_on, HB_ERR_STATE, "hb_plant_get_terrain_profile: no terrain profile in force (hb_plant_set_terrain_profile)");
  if (segment || ctx->profile_draw_on) {
    HB_ENTER_DEVICE();
    HB_HIP(hipStreamSynchronize(ctx->s_wbc));
    HB_TRY(profile_draw_refresh_host(ctx));   // (the device draws the records: the host image is stale)
    HB_TRY(pull(ctx, segment, ctx->profile, ctx->profile.seg, whole(ctx)));
  }
  constexpr size_t nrec = size_t(Profile::rec) * (HB_PROFILE_MAX_KNOTS - 1);
  for (size_t i = 0; i < size_t(ctx->B); ++i) {
    const double* r = ctx->profile_host.data() + i * Profile::stored;
    if (n_knots) n_knots[i] = int32_t(r[Profile::nseg]) + 1;
    if (dir) std::memcpy(dir + 2 * i, r + Profile::dir, 2 * sizeof(double));
    if (knots) std::memcpy(knots + i * HB_PROFILE_MAX_KNOTS * 2, ctx->profile_knots.data() + i * HB_PROFILE_MAX_KNOTS * 2, HB_PROFILE_MAX_KNOTS * 2 * sizeof(double));
    if (mu) std::memcpy(mu + 4 * i, r + Profile::head + Terrain::mu, 4 * sizeof(double));
    if (records) std::memcpy(records + i * nrec, r + Profile::seg, nrec * sizeof(double));
  }
  return HB_OK;
}

// ---- per-instance height field of contact model 1 (include/hunter_hip.h above hb_plant_set_terrain_field) ------------------------------
// (the stored record of an instance, validation included, is hb_contact.hpp field_record)
int32_t hb_plant_set_terrain_field(hb_ctx* ctx, const int32_t* n_nodes, const double* dir, const double* origin, const double* spacing,
                                   const double* heights, const double* mu) {
  HB_ENTER_ARGS(false);
  HB_TRY(contact_ready(ctx, "hb_plant_set_terrain_field"));
  const bool on = n_nodes || dir || origin || spacing || heights;
  HB_FAIL_IF(on && !(n_nodes && dir && origin && spacing && heights), HB_ERR_ARG, "hb_plant_set_terrain_field: give n_nodes, dir, origin, spacing and heights, or none of them to switch the field off (the ground in force is kept)");
  HB_FAIL_IF(!on && mu, HB_ERR_ARG, "hb_plant_set_terrain_field: friction coefficients without a field (the ground in force is kept)");
  HB_FAIL_IF(ctx->profile_draw_on, HB_ERR_STATE, "hb_plant_set_terrain_field: the profile draw in force draws the ground (hb_plant_set_profile_draw): turn it off first");
  HB_FAIL_IF(ctx->field_draw_on, HB_ERR_STATE, "hb_plant_set_terrain_field: the field draw in force draws the ground (hb_plant_set_field_draw): turn it off first");
  HB_FAIL_IF(on && ctx->respawn_on, HB_ERR_STATE, "hb_plant_set_terrain_field: a respawn configuration is in force (hb_plant_set_respawn): no respawn on a field, turn it off first");
  HB_FAIL_IF(on && ctx->scenario_on && (ctx->scenario_cfg.channels & (HB_SC_SLOPE | HB_SC_MU)), HB_ERR_STATE, "hb_plant_set_terrain_field: the scenario in force draws the terrain (hb_plant_set_scenario): turn it off first");
  const size_t B = ctx->B;
  std::vector<double> hdr(on ? B * Field::stored : 0), z(on ? B * Field::nz : 0);
  for (size_t i = 0; i < B && on; ++i) {
    const int n[2] = {n_nodes[2 * i], n_nodes[2 * i + 1]};
    const double* zi = heights + i * Field::nz;
    if (n[0] >= 2 && n[0] <= HB_FIELD_MAX_NODES && n[1] >= 2 && n[1] <= HB_FIELD_MAX_NODES)   // (the stored heights: zero beyond (nu, nw))
      for (int iu = 0; iu < n[0]; ++iu) std::memcpy(z.data() + i * Field::nz + iu * Field::pitch, zi + iu * Field::pitch, size_t(n[1]) * sizeof(double));
    if (const char* why = field_record(n, dir + 2 * i, origin + 2 * i, spacing + 2 * i, z.data() + i * Field::nz, mu ? mu + 4 * i : nullptr, ctx->contact_cfg.mu,
                                       hdr.data() + i * Field::stored))
      return refuse_instance(ctx, HB_ERR_ARG, "hb_plant_set_terrain_field", i, why, "ground");
  }
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));  // (a step in flight still runs on the ground it was launched with)
  if (on) return field_install(ctx, hdr, z);
  ctx->field_on = false;
  HB_TRY(modelvar_level(ctx));
  return contact_forget_warm_start(ctx);
}

int32_t hb_plant_get_terrain_field(hb_ctx* ctx, int32_t* n_nodes, double* dir, double* origin, double* spacing, double* heights, double* mu,
                                   int32_t* facet) {
  HB_ENTER_ARGS(false);
  HB_TRY(contact_ready(ctx, "hb_plant_get_terrain_field"));
  HB_FAIL_IF(!ctx->field_on, HB_ERR_STATE, "hb_plant_get_terrain_field: no height field in force (hb_plant_set_terrain_field)");
  if (facet || ctx->field_draw_on) {
    HB_ENTER_DEVICE();
    HB_HIP(hipStreamSynchronize(ctx->s_wbc));
    HB_TRY(field_draw_refresh_host(ctx));   // (the device draws the records: the host image is stale)
    HB_TRY(pull(ctx, facet, ctx->field, ctx->field.sel, whole(ctx)));
  }
  for (size_t i = 0; i < size_t(ctx->B); ++i) {
    const double* r = ctx->field_hdr_host.data() + i * Field::stored;
    if (n_nodes) { n_nodes[2 * i] = int32_t(r[Field::nu]); n_nodes[2 * i + 1] = int32_t(r[Field::nw]); }
    if (dir) std::memcpy(dir + 2 * i, r + Field::dir, 2 * sizeof(double));
    if (origin) std::memcpy(origin + 2 * i, r + Field::org, 2 * sizeof(double));
    if (spacing) std::memcpy(spacing + 2 * i, r + Field::step, 2 * sizeof(double));
    if (mu) std::memcpy(mu + 4 * i, r + Field::head + Terrain::mu, 4 * sizeof(double));
  }
  if (heights) std::memcpy(heights, ctx->field_z_host.data(), ctx->field_z_host.size() * sizeof(double));
  return HB_OK;
}

int32_t hb_plant_field_eval(hb_ctx* ctx, int32_t n_points, const double* xyz, int32_t* facet_id, double* records, double* height) {
  HB_ENTER_ARGS(n_points <= 0 || !xyz || !(facet_id || records || height));
  HB_TRY(contact_ready(ctx, "hb_plant_field_eval"));
  HB_FAIL_IF(!ctx->field_on, HB_ERR_STATE, "hb_plant_field_eval: no height field in force (hb_plant_set_terrain_field)");
  HB_ENTER_DEVICE();
  const size_t m = size_t(ctx->B) * size_t(n_points);
  DevBuf<double> dx, dr, dh;
  DevBuf<int> df;
  HB_HIP(dx.alloc(m * 3, xyz));
  HB_HIP(dr.alloc(m * Profile::rec));
  HB_HIP(dh.alloc(m));
  HB_HIP(df.alloc(m));
  hipStream_t s = ctx->s_wbc;
  hipLaunchKernelGGL(k_field_eval, dim3(unsigned((m + 63) / 64)), dim3(64), 0, s, ctx->field, n_points, dx.p, df.p, dr.p, dh.p);
  HB_HIP(hipGetLastError());
  HB_HIP(hipStreamSynchronize(s));
  if (facet_id) HB_HIP(hipMemcpy(facet_id, df.p, m * 4, hipMemcpyDeviceToHost));
  if (records) HB_HIP(hipMemcpy(records, dr.p, m * Profile::rec * 8, hipMemcpyDeviceToHost));
  if (height) HB_HIP(hipMemcpy(height, dh.p, m * 8, hipMemcpyDeviceToHost));
  return HB_OK;
}

// ---- per-instance model variation of contact model 1 (include/hunter_hip.h above hb_plant_set_model_variation) --------------------------
int32_t hb_plant_set_model_variation(hb_ctx* ctx, const double* mass_scale, const double* payload) {
  HB_ENTER_ARGS(false);
  HB_TRY(contact_ready(ctx, "hb_plant_set_model_variation"));
  HB_FAIL_IF(!mass_scale && !payload && ctx->scenario_on && (ctx->scenario_cfg.channels & (HB_SC_PAYLOAD | HB_SC_MASS)), HB_ERR_STATE, "hb_plant_set_model_variation: the scenario in force draws the variation (hb_plant_set_scenario): turn it off first");
  const size_t B = ctx->B;
  const bool on = mass_scale || payload;
  std::vector<DevModel> img(on ? B : 0);
  int bad = 0;
  if (const char* why = on ? modelvar_compose_batch(ctx->hmodel, int(B), mass_scale, payload, img.data(), &bad) : nullptr)
    return refuse_instance(ctx, HB_ERR_ARG, "hb_plant_set_model_variation", size_t(bad), why, "variation");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));  // (a step in flight still runs on the models it was launched with)
  if (on) {
    ModelVarBatch& m = ctx->modelvar;
    HB_TRY(ensure_fields(ctx, m));
    HB_TRY(push(ctx, img.data(), m, m.mdl, whole(ctx)));
    ctx->modelvar_host = std::move(img);
  }
  ctx->modelvar_on = on;
  return modelvar_level(ctx);
}

int32_t hb_plant_get_model_variation(hb_ctx* ctx, double* mass, double* com, double* inertia, double* total_mass) {
  HB_ENTER_ARGS(false);
  HB_TRY(contact_ready(ctx, "hb_plant_get_model_variation"));
  if (ctx->scenario_on) {   // the device draws the records: the host image is stale
    HB_ENTER_DEVICE();
    HB_HIP(hipStreamSynchronize(ctx->s_wbc));
    HB_TRY(scenario_refresh_host(ctx));
  }
  for (size_t i = 0; i < size_t(ctx->B); ++i) {
    const DevModel& d = ctx->modelvar_on ? ctx->modelvar_host[i] : ctx->hmodel;
    if (mass) std::memcpy(mass + HB_NBODY * i, d.mass, sizeof d.mass);
    if (com) std::memcpy(com + 3 * HB_NBODY * i, d.com, sizeof d.com);
    if (inertia) std::memcpy(inertia + 6 * HB_NBODY * i, d.inertia, sizeof d.inertia);
    if (total_mass) total_mass[i] = d.total_mass;
  }
  return HB_OK;
}

// ---- sensor model ------------------------------------------------------------------------------------------------------------------------
int32_t hb_plant_set_sensor_model(hb_ctx* ctx, const hb_sensor_config* cfg, const double* gyro_bias, const double* accel_bias) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->plant_ready, HB_ERR_STATE, "hb_plant_set_sensor_model: call hb_plant_reset first (the sensor arrays belong to the plant)");
  HB_FAIL_IF(cfg && !sensor_config_valid(*cfg), HB_ERR_ARG, "hb_plant_set_sensor_model: every noise standard deviation must be finite and >= 0, and `reserved` 0");
  HB_ENTER_DEVICE();
  const size_t B = ctx->B;
  PlantBatch& p = ctx->plant;
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));  // (an earlier reading may still be using the biases)
  // the bias arrays are kept once allocated; a null pointer in the batch means "no bias"
  const double* src[2] = {gyro_bias, accel_bias};
  double** dst[2] = {&p.gyro_bias, &p.accel_bias};
  double** store[2] = {&ctx->sens_gyro_bias_buf, &ctx->sens_accel_bias_buf};
  for (int k = 0; k < 2; ++k) {
    if (src[k]) {
      if (!*store[k]) HB_HIP(dalloc(ctx, store[k], B * 3));
      HB_HIP(hipMemcpy(*store[k], src[k], B * 3 * 8, hipMemcpyHostToDevice));
    }
    *dst[k] = src[k] ? *store[k] : nullptr;
  }
  ctx->sens_cfg = cfg ? *cfg : hb_sensor_config{};
  ctx->sens_noisy = cfg && (cfg->orientation_noise > 0.0 || cfg->gyro_noise > 0.0 || cfg->accel_noise > 0.0 || cfg->joint_pos_noise > 0.0 ||
                            cfg->joint_vel_noise > 0.0 || cfg->joint_torque_noise > 0.0);
  ctx->sense_count = 0;
  return HB_OK;
}

int32_t hb_plant_sense(hb_ctx* ctx, double* quat, double* ang_vel_local, double* lin_acc_local, double* joint_pos, double* joint_vel,
                       double* joint_torque, int32_t* contact_flag) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->plant_ready, HB_ERR_STATE, "hb_plant_sense: call hb_plant_reset first");
  HB_ENTER_DEVICE();
  PlantBatch& p = ctx->plant;
  hipStream_t s = ctx->s_wbc;  // behind the plant step, in front of the estimator
  hipLaunchKernelGGL(k_plant_sense, dim3((ctx->B + kSenseThreads - 1) / kSenseThreads), dim3(kSenseThreads), 0, s, p, ctx->dmodel, ctx->sens_cfg,
                     ctx->sens_noisy ? 1 : 0, static_cast<unsigned long long>(ctx->sense_count));
  HB_HIP(hipGetLastError());
  ++ctx->sense_count;
  ctx->sensed = true;
  double* const outs[6] = {quat, ang_vel_local, lin_acc_local, joint_pos, joint_vel, joint_torque};
  double* const* dev[6] = {&p.s_quat, &p.s_gyro, &p.s_accel, &p.s_jp, &p.s_jv, &p.s_jt};
  bool any = contact_flag != nullptr;
  for (int k = 0; k < 6; ++k) {
    HB_TRY(pull(ctx, outs[k], p, *dev[k], whole(ctx), &s));
    any = any || outs[k];
  }
  HB_TRY(pull(ctx, contact_flag, p, p.s_contact, whole(ctx), &s));
  if (any) HB_HIP(hipStreamSynchronize(s));  // without host outputs the call is enqueue-only
  return HB_OK;
}

}  // extern "C"
