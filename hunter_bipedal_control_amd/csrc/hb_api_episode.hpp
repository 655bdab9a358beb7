// Host side, part 6: the episode layer on top of the plant, each entry below the ones it depends on: the per-instance episode record
// (hb_plant_set / get_episode), the respawn of ended instances (hb_plant_set_respawn, hb_plant_respawn, hb_plant_get_respawn) and what is
// drawn at respawn: the scenario (hb_plant_set / get_scenario, hb_plant_get_scenario_log), the profile (hb_plant_set / get_profile_draw,
// hb_plant_get_profile_draw_log) and the height field (hb_plant_set / get_field_draw, hb_plant_get_field_draw_log).  The static helpers they share with the plant entries stand at the head of hb_api_plant.hpp.
#pragma once

extern "C" {

// ---- per-instance episode record (include/hunter_hip.h above hb_plant_set_episode) -------------------------------------------------
int32_t hb_plant_set_episode(hb_ctx* ctx, const hb_episode_config* cfg) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->plant_ready, HB_ERR_STATE, "hb_plant_set_episode: call hb_plant_reset first");
  HB_FAIL_IF(cfg && !episode_config_valid(*cfg), HB_ERR_ARG, "hb_plant_set_episode: slip_speed, tilt_limit >= 0 and finite, stop_on_fall 0 / 1, trace_every >= 0, trace_capacity 0 .. 4096 and `reserved` 0 (the episode in force is kept)");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));  // (a step in flight still updates the record it was launched with)
  if (!cfg) {
    ctx->episode_on = false;
    ctx->respawn_on = false;   // the respawn reads its decision from the record
    HB_TRY(profile_draw_off(ctx));   // ... and the scenario, the profile and the field are drawn at respawn
    HB_TRY(field_draw_off(ctx));
    return scenario_off(ctx);
  }
  EpisodeBatch& e = ctx->episode;
  HB_TRY(ensure_fields(ctx, e));
  HB_TRY(log_grow(ctx, e.trace, e.trace_cap, cfg->trace_capacity, HB_EP_TRACE_W));
  if (cfg->stop_on_fall) HB_TRY(joint_state_alloc(ctx));
  ctx->episode_cfg = *cfg;
  ctx->episode_on = true;
  HB_TRY(episode_start(ctx, ctx->s_wbc));
  if (ctx->respawn_on) HB_TRY(respawn_totals_start(ctx, ctx->s_wbc));   // (the totals account for the steps of the records they folded)
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  return HB_OK;
}

int32_t hb_plant_get_episode(hb_ctx* ctx, int32_t* irec, double* drec, double* trace) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->plant_ready, HB_ERR_STATE, "hb_plant_get_episode: call hb_plant_reset first");
  HB_FAIL_IF(!ctx->episode_on, HB_ERR_STATE, "hb_plant_get_episode: no episode in force (hb_plant_set_episode)");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  EpisodeBatch& e = ctx->episode;
  HB_TRY(pull(ctx, irec, e, e.irec, whole(ctx)));
  HB_TRY(pull(ctx, drec, e, e.drec, whole(ctx)));
  return log_read(ctx, trace, e.trace, e.trace_cap, ctx->episode_cfg.trace_capacity, HB_EP_TRACE_W);
}

// ---- respawn of ended instances (include/hunter_hip.h above hb_plant_set_respawn) ------------------------------------------------------
int32_t hb_plant_set_respawn(hb_ctx* ctx, const hb_respawn_config* cfg, const double* q_spawn, const double* v_spawn) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->plant_ready, HB_ERR_STATE, "hb_plant_set_respawn: call hb_plant_reset first");
  HB_FAIL_IF(!ctx->episode_on, HB_ERR_STATE, "hb_plant_set_respawn: no episode in force (hb_plant_set_episode): the decision is read from the episode record");
  HB_TRY(refuse_config(ctx, "hb_plant_set_respawn", cfg ? respawn_config_refusal(*cfg) : nullptr));
  HB_FAIL_IF(cfg && ctx->field_on, HB_ERR_STATE, "hb_plant_set_respawn: a height field is in force (hb_plant_set_terrain_field): no respawn on a field, turn it off first");
  HB_FAIL_IF(cfg && ctx->profile_on, HB_ERR_STATE, "hb_plant_set_respawn: a terrain profile is in force (hb_plant_set_terrain_profile): no respawn on a profile, turn it off first");
  HB_FAIL_IF(cfg && !q_spawn, HB_ERR_ARG, "hb_plant_set_respawn: q_spawn is required with a configuration (the configuration in force is kept)");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));  // (a respawn in flight still runs under the configuration it was launched with)
  if (!cfg) {
    {
      std::lock_guard<std::mutex> lk(ctx->mtx);
      ctx->respawn_on = false;
      ctx->rs_rg_due = ctx->rs_mpc_due = false;   // (flags still pending are dropped: the next configuration starts with none)
    }
    HB_TRY(profile_draw_off(ctx));   // the scenario, the profile and the field are drawn at respawn
    HB_TRY(field_draw_off(ctx));
    return scenario_off(ctx);
  }
  RespawnBatch& r = ctx->respawn;
  HB_TRY(ensure_fields(ctx, r));
  HB_TRY(push(ctx, q_spawn, r, r.q_spawn, whole(ctx)));
  if (v_spawn) HB_TRY(push(ctx, v_spawn, r, r.v_spawn, whole(ctx)));
  else HB_TRY(zero_field(ctx, r, r.v_spawn));
  ctx->respawn_cfg = *cfg;
  ctx->respawn_on = true;
  HB_TRY(respawn_totals_start(ctx, ctx->s_wbc));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  return HB_OK;
}

int32_t hb_plant_respawn(hb_ctx* ctx) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->respawn_on, HB_ERR_STATE, "hb_plant_respawn: no respawn configuration in force (hb_plant_set_respawn)");
  HB_ENTER_DEVICE();
  double d0;
  const double* ter = episode_plane(ctx, &d0);
  hipStream_t s = ctx->s_wbc;  // behind the plant step and the update of the record
  const ContactBatch cb = has_fields(ctx, ctx->contact) ? ctx->contact : ContactBatch{};
  const JointBatch jb = has_fields(ctx, ctx->joints) ? ctx->joints : JointBatch{};
  const ActuatorBatch ab = has_fields(ctx, ctx->act) ? ctx->act : ActuatorBatch{};
  const EstBatch est = ctx->est_ready ? ctx->est : EstBatch{};
  // (on a profile the kernel takes its plane from the facet it locates and writes ProfileBatch::base: `ter`, which would be that array, is not passed)
  const bool on_profile = ctx->contact_cfg.mode == 1 && ctx->profile_on;
  // (likewise on a height field: the kernel's field form writes FieldBatch::base)
  const bool on_field = ctx->contact_cfg.mode == 1 && ctx->field_on;
  // a writer of the resident observation, and of the pending flags and the gait state the MPC stream reads: always between the two
  // ordering points
  HB_TRY(resident_write(ctx, s, true, [&] {
    if (ctx->scenario_on) {   // the scenario of the episode that starts, drawn ahead of the respawn from the same decision
      const int ch = ctx->scenario_cfg.channels;
      hipLaunchKernelGGL(k_plant_scenario, dim3(ctx->B), dim3(64), 0, s, ctx->scenario, ctx->scenario_cfg, ctx->respawn_cfg, ctx->respawn, ctx->episode,
                         (ch & (HB_SC_SLOPE | HB_SC_MU)) ? ctx->terrain.ter : nullptr, (ch & (HB_SC_PAYLOAD | HB_SC_MASS)) ? ctx->modelvar.mdl : nullptr,
                         ctx->dmodel, ctx->contact_cfg.ground_z);
    }
    if (ctx->profile_draw_on)   // the ground of the episode that starts, from the same decision (the map follows where asked and in force)
      hipLaunchKernelGGL(k_plant_profile_draw, dim3(ctx->B), dim3(64), 0, s, ctx->profile_draw, ctx->profile_draw_cfg, ctx->respawn_cfg, ctx->respawn,
                         ctx->episode, ctx->profile, ctx->profile_draw_cfg.follow_map && ctx->ground_on ? ctx->ground.map : nullptr,
                         ctx->contact_cfg.ground_z);
    if (ctx->field_draw_on)   // the height field of the episode that starts, from the same decision (the field map follows where asked and in force)
      hipLaunchKernelGGL(k_plant_field_draw, dim3(ctx->B), dim3(64), 0, s, ctx->field_draw, ctx->field_draw_cfg, ctx->respawn_cfg, ctx->respawn,
                         ctx->episode, ctx->field, field_draw_follows(ctx) ? ctx->gfield : GroundFieldBatch{}, ctx->contact_cfg.ground_z);
    if (on_field)
      hipLaunchKernelGGL(k_plant_respawn_field, dim3(ctx->B), dim3(64), 0, s, ctx->respawn, ctx->respawn_cfg, ctx->episode, ctx->plant, cb, jb, ab,
                         est, ctx->gait, ctx->gait_cfg, ctx->gait_on ? 1 : 0, d0, ctx->dmodel, ctx->jc_estop, ctx->w.rbd, ctx->b.x0, ctx->field);
    else
      hipLaunchKernelGGL(k_plant_respawn, dim3(ctx->B), dim3(64), 0, s, ctx->respawn, ctx->respawn_cfg, ctx->episode, ctx->plant, cb, jb, ab, est,
                         ctx->gait, ctx->gait_cfg, ctx->gait_on ? 1 : 0, on_profile ? nullptr : ter, d0, ctx->dmodel, ctx->jc_estop, ctx->w.rbd,
                         ctx->b.x0, on_profile ? ctx->profile : ProfileBatch{});
  }));
  std::lock_guard<std::mutex> lk(ctx->mtx);
  ctx->rs_rg_due = ctx->rs_mpc_due = true;
  return HB_OK;
}

int32_t hb_plant_get_respawn(hb_ctx* ctx, int32_t* itot, double* dtot, double* q_last, double* v_last) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->respawn_on, HB_ERR_STATE, "hb_plant_get_respawn: no respawn configuration in force (hb_plant_set_respawn)");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  RespawnBatch& r = ctx->respawn;
  HB_TRY(pull(ctx, itot, r, r.itot, whole(ctx)));
  HB_TRY(pull(ctx, dtot, r, r.dtot, whole(ctx)));
  HB_TRY(pull(ctx, q_last, r, r.q_last, whole(ctx)));
  HB_TRY(pull(ctx, v_last, r, r.v_last, whole(ctx)));
  return HB_OK;
}

// ---- scenario draw at respawn (include/hunter_hip.h above hb_plant_set_scenario) --------------------------------------------------------
int32_t hb_plant_set_scenario(hb_ctx* ctx, const hb_scenario_config* cfg) {
  HB_ENTER_ARGS(false);
  if (!cfg && !ctx->scenario_on) return HB_OK;
  HB_TRY(contact_ready(ctx, "hb_plant_set_scenario"));
  HB_FAIL_IF(cfg && !ctx->respawn_on, HB_ERR_STATE, "hb_plant_set_scenario: no respawn configuration in force (hb_plant_set_respawn): the scenario is drawn at respawn");
  HB_FAIL_IF(cfg && ctx->field_on && (cfg->channels & (HB_SC_SLOPE | HB_SC_MU)), HB_ERR_STATE, "hb_plant_set_scenario: a height field is in force (hb_plant_set_terrain_field): no slope or friction draw on a field, turn it off first");
  HB_FAIL_IF(cfg && ctx->profile_on && (cfg->channels & (HB_SC_SLOPE | HB_SC_MU)), HB_ERR_STATE, "hb_plant_set_scenario: a terrain profile is in force (hb_plant_set_terrain_profile): no slope or friction draw on a profile, turn it off first");
  HB_TRY(refuse_config(ctx, "hb_plant_set_scenario", cfg ? scenario_config_refusal(*cfg) : nullptr));
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));  // (a respawn or a step in flight still runs under the configuration it was launched with)
  HB_TRY(scenario_off(ctx));   // (a configuration in force hands its records and its wrench back first; a failure below leaves it off)
  if (!cfg) return HB_OK;
  ScenarioBatch& c = ctx->scenario;
  HB_TRY(ensure_fields(ctx, c));
  HB_TRY(log_grow(ctx, c.log, c.log_cap, cfg->log_capacity, HB_SC_LOG_W));
  if ((cfg->channels & (HB_SC_SLOPE | HB_SC_MU)) && !ctx->terrain_on) HB_TRY(terrain_level_install(ctx, true));
  if ((cfg->channels & (HB_SC_PAYLOAD | HB_SC_MASS)) && !ctx->modelvar_on) {   // nominal copies
    ModelVarBatch& m = ctx->modelvar;
    HB_TRY(ensure_fields(ctx, m));
    std::vector<DevModel> img(size_t(ctx->B), ctx->hmodel);
    HB_TRY(push(ctx, img.data(), m, m.mdl, whole(ctx)));
    ctx->modelvar_host = std::move(img);
    ctx->modelvar_on = true;
    HB_TRY(modelvar_level(ctx));
  }
  if (cfg->channels & HB_SC_PUSH) {   // the scenario owns the wrench
    HB_TRY(zero_field(ctx, ctx->contact, ctx->contact.wrench));
    ctx->contact.use_wrench = 1;
  }
  ctx->scenario_cfg = *cfg;
  ctx->scenario_on = true;
  return scenario_start(ctx, true);
}

int32_t hb_plant_get_scenario(hb_ctx* ctx, double* scen) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->scenario_on, HB_ERR_STATE, "hb_plant_get_scenario: no scenario in force (hb_plant_set_scenario)");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  return pull(ctx, scen, ctx->scenario, ctx->scenario.scen, whole(ctx));
}

int32_t hb_plant_get_scenario_log(hb_ctx* ctx, int32_t* count, double* log) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->scenario_on, HB_ERR_STATE, "hb_plant_get_scenario_log: no scenario in force (hb_plant_set_scenario)");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  ScenarioBatch& c = ctx->scenario;
  HB_TRY(pull(ctx, count, c, c.count, whole(ctx)));
  return log_read(ctx, log, c.log, c.log_cap, ctx->scenario_cfg.log_capacity, HB_SC_LOG_W);
}

// ---- profile draw at respawn (include/hunter_hip.h above hb_plant_set_profile_draw) -----------------------------------------------------
int32_t hb_plant_set_profile_draw(hb_ctx* ctx, const hb_profile_draw_config* cfg) {
  HB_ENTER_ARGS(false);
  if (!cfg && !ctx->profile_draw_on) return HB_OK;
  HB_TRY(contact_ready(ctx, "hb_plant_set_profile_draw"));
  HB_FAIL_IF(cfg && ctx->field_draw_on, HB_ERR_STATE, "hb_plant_set_profile_draw: a field draw is in force (hb_plant_set_field_draw): turn it off first");
  HB_FAIL_IF(cfg && ctx->field_on, HB_ERR_STATE, "hb_plant_set_profile_draw: a height field is in force (hb_plant_set_terrain_field): turn it off first");
  HB_FAIL_IF(cfg && !ctx->respawn_on, HB_ERR_STATE, "hb_plant_set_profile_draw: no respawn configuration in force (hb_plant_set_respawn): the profile is drawn at respawn");
  HB_FAIL_IF(cfg && ctx->scenario_on && (ctx->scenario_cfg.channels & (HB_SC_SLOPE | HB_SC_MU)), HB_ERR_STATE, "hb_plant_set_profile_draw: the scenario in force draws the terrain (hb_plant_set_scenario with HB_SC_SLOPE or HB_SC_MU): turn it off first");
  HB_TRY(refuse_config(ctx, "hb_plant_set_profile_draw", cfg ? profile_draw_config_refusal(*cfg) : nullptr));
  HB_FAIL_IF(cfg && cfg->follow_map && ctx->gfield_on, HB_ERR_STATE, "hb_plant_set_profile_draw: follow_map while a field map is in force (hb_ground_set_field): the draw writes profile records, turn the field map off first");
  HB_FAIL_IF(cfg && cfg->follow_map && !ctx->ground_on, HB_ERR_STATE, "hb_plant_set_profile_draw: follow_map without a ground map in force (hb_ground_set_profile): set the zero map first");
  HB_FAIL_IF(cfg && !(std::fabs(ctx->contact_cfg.ground_z) <= PD_REACH), HB_ERR_STATE, "hb_plant_set_profile_draw: |ground_z| of the contact model above 1e3: the knots are drawn around ground_z");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));  // (a respawn or a step in flight still runs under the configuration it was launched with)
  if (!cfg) return profile_draw_off(ctx);
  const size_t B = ctx->B;
  hb_profile_draw_config K = *cfg;
  profile_direction(cfg->dir, K.dir);
  // the level ground every instance starts on: the FLAT knots around its spawn point
  std::vector<double> qs(B * 16), rec(B * Profile::stored), kn(B * PD_KNOTS), grel(cfg->follow_map ? B * PD_KNOTS : 0),
      grec(cfg->follow_map ? B * Ground::size : 0);
  HB_TRY(pull(ctx, qs.data(), ctx->respawn, ctx->respawn.q_spawn, whole(ctx)));
  const double mu4[HB_NC] = {ctx->contact_cfg.mu, ctx->contact_cfg.mu, ctx->contact_cfg.mu, ctx->contact_cfg.mu};
  for (size_t i = 0; i < B; ++i) {
    const double s0 = profile_draw_s0(K.dir, qs.data() + 16 * i);
    if (!(std::fabs(s0) <= PD_REACH))
      return refuse_instance(ctx, HB_ERR_STATE, "hb_plant_set_profile_draw", i, "a spawn point further than 1e3 along dir", "configuration");
    double rel[PD_KNOTS];
    const int nk = profile_draw_flat(s0, ctx->contact_cfg.ground_z, rel, kn.data() + i * PD_KNOTS);
    profile_compose(OneLane{}, nk, K.dir, kn.data() + i * PD_KNOTS, mu4, rec.data() + i * Profile::stored);
    if (cfg->follow_map) {   // the map follows from the start: the zero map over the same knots
      std::memcpy(grel.data() + i * PD_KNOTS, rel, sizeof rel);
      ground_compose(OneLane{}, nk, K.dir, rel, grec.data() + i * Ground::size);
    }
  }
  HB_TRY(profile_draw_off(ctx));   // (a configuration in force hands its records back first; a failure below leaves it off)
  ProfileDrawBatch& d = ctx->profile_draw;
  HB_TRY(ensure_fields(ctx, d));
  HB_TRY(log_grow(ctx, d.log, d.log_cap, cfg->log_capacity, HB_PD_LOG_W));
  HB_TRY(profile_install(ctx, rec, kn, true, cfg->follow_map ? &grec : nullptr, &grel));   // the level profile replaces a terrain
  ctx->profile_draw_cfg = K;
  ctx->profile_draw_on = true;
  return profile_draw_start(ctx, true);
}

int32_t hb_plant_get_profile_draw(hb_ctx* ctx, double* row) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->profile_draw_on, HB_ERR_STATE, "hb_plant_get_profile_draw: no profile draw in force (hb_plant_set_profile_draw)");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  return pull(ctx, row, ctx->profile_draw, ctx->profile_draw.row, whole(ctx));
}

int32_t hb_plant_get_profile_draw_log(hb_ctx* ctx, int32_t* count, double* log) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->profile_draw_on, HB_ERR_STATE, "hb_plant_get_profile_draw_log: no profile draw in force (hb_plant_set_profile_draw)");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  ProfileDrawBatch& d = ctx->profile_draw;
  HB_TRY(pull(ctx, count, d, d.count, whole(ctx)));
  return log_read(ctx, log, d.log, d.log_cap, ctx->profile_draw_cfg.log_capacity, HB_PD_LOG_W);
}

// ---- field draw at respawn (include/hunter_hip.h above hb_plant_set_field_draw) -----------------------------------------------------------
int32_t hb_plant_set_field_draw(hb_ctx* ctx, const hb_field_draw_config* cfg) {
  HB_ENTER_ARGS(false);
  if (!cfg && !ctx->field_draw_on) return HB_OK;
  HB_TRY(contact_ready(ctx, "hb_plant_set_field_draw"));
  HB_FAIL_IF(cfg && !ctx->respawn_on, HB_ERR_STATE, "hb_plant_set_field_draw: no respawn configuration in force (hb_plant_set_respawn): the field is drawn at respawn");
  HB_FAIL_IF(cfg && ctx->profile_draw_on, HB_ERR_STATE, "hb_plant_set_field_draw: a profile draw is in force (hb_plant_set_profile_draw): turn it off first");
  HB_FAIL_IF(cfg && ctx->scenario_on && (ctx->scenario_cfg.channels & (HB_SC_SLOPE | HB_SC_MU)), HB_ERR_STATE, "hb_plant_set_field_draw: the scenario in force draws the terrain (hb_plant_set_scenario with HB_SC_SLOPE or HB_SC_MU): turn it off first");
  HB_TRY(refuse_config(ctx, "hb_plant_set_field_draw", cfg ? field_draw_config_refusal(*cfg) : nullptr));
  HB_FAIL_IF(cfg && cfg->follow_map && ctx->ground_on, HB_ERR_STATE, "hb_plant_set_field_draw: follow_map while a profile map is in force (hb_ground_set_profile): the draw writes field maps, set the zero field map first (hb_ground_set_field)");
  HB_FAIL_IF(cfg && cfg->follow_map && ctx->scan_on, HB_ERR_STATE, "hb_plant_set_field_draw: follow_map while a height scan is in force (hb_plant_set_height_scan): the scan writes the field map, turn it off first");
  HB_FAIL_IF(cfg && cfg->follow_map && !ctx->gfield_on, HB_ERR_STATE, "hb_plant_set_field_draw: follow_map without a field map in force (hb_ground_set_field): set the zero field map first");
  HB_FAIL_IF(cfg && !(std::fabs(ctx->contact_cfg.ground_z) <= FD_REACH), HB_ERR_STATE, "hb_plant_set_field_draw: |ground_z| of the contact model above 1e3: the heights are drawn around ground_z");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));  // (a respawn or a step in flight still runs under the configuration it was launched with)
  if (!cfg) return field_draw_off(ctx);
  const size_t B = ctx->B;
  hb_field_draw_config K = *cfg;
  profile_direction(cfg->dir, K.dir);
  // the level ground every instance starts on: the configured grid around its spawn point, at ground_z
  std::vector<double> qs(B * 16), hdr(B * Field::stored), z(B * Field::nz), ghdr(cfg->follow_map ? B * GroundField::size : 0),
      gz(cfg->follow_map ? B * GroundField::nz : 0);
  HB_TRY(pull(ctx, qs.data(), ctx->respawn, ctx->respawn.q_spawn, whole(ctx)));
  const double mu4[HB_NC] = {ctx->contact_cfg.mu, ctx->contact_cfg.mu, ctx->contact_cfg.mu, ctx->contact_cfg.mu};
  for (size_t i = 0; i < B; ++i) {
    double org[2], sq[2];
    field_draw_origin(K, K.dir, qs.data() + 16 * i, org, sq);
    if (!(std::fabs(sq[0]) <= FD_REACH && std::fabs(sq[1]) <= FD_REACH))
      return refuse_instance(ctx, HB_ERR_STATE, "hb_plant_set_field_draw", i, "a spawn point further than 1e3 along or across dir", "configuration");
    field_draw_flat(K, ctx->contact_cfg.ground_z, z.data() + i * Field::nz, cfg->follow_map ? gz.data() + i * GroundField::nz : nullptr);
    field_compose(K.n_nodes, K.dir, org, K.spacing, z.data() + i * Field::nz, mu4, hdr.data() + i * Field::stored);
    if (cfg->follow_map) ground_field_compose(K.n_nodes, K.dir, org, K.spacing, ghdr.data() + i * GroundField::size);
  }
  HB_TRY(field_draw_off(ctx));   // (a configuration in force hands its records back first; a failure below leaves it off)
  FieldDrawBatch& d = ctx->field_draw;
  HB_TRY(ensure_fields(ctx, d));
  HB_TRY(log_grow(ctx, d.log, d.log_cap, cfg->log_capacity, HB_FD_LOG_W));
  HB_TRY(field_install(ctx, hdr, z, cfg->follow_map ? &ghdr : nullptr, &gz));   // the level field replaces a terrain or a profile
  ctx->field_draw_cfg = K;
  ctx->field_draw_on = true;
  return field_draw_start(ctx, true);
}

int32_t hb_plant_get_field_draw(hb_ctx* ctx, double* row) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->field_draw_on, HB_ERR_STATE, "hb_plant_get_field_draw: no field draw in force (hb_plant_set_field_draw)");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  return pull(ctx, row, ctx->field_draw, ctx->field_draw.row, whole(ctx));
}

int32_t hb_plant_get_field_draw_log(hb_ctx* ctx, int32_t* count, double* log) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->field_draw_on, HB_ERR_STATE, "hb_plant_get_field_draw_log: no field draw in force (hb_plant_set_field_draw)");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  FieldDrawBatch& d = ctx->field_draw;
  HB_TRY(pull(ctx, count, d, d.count, whole(ctx)));
  return log_read(ctx, log, d.log, d.log_cap, ctx->field_draw_cfg.log_capacity, HB_FD_LOG_W);
}

}  // extern "C"
