// Host side, part 4: reference generation (hb_refgen_*) and the device gait manager (hb_gait_*).
#pragma once

// message of the refusal of a horizon that needs more joint-reference knots than the knot arrays hold (hb_refgen.hpp
// rg_horizon_over_knot_bound): RG_MAX_KNOTS - 2 = 22 knots, 0.15 s apart
static_assert(RG_MAX_KNOTS - 2 == 22, "the bound named in RG_KNOT_BOUND_TEXT and in include/hunter_hip.h");
#define RG_KNOT_BOUND_TEXT(fn) \
  fn ": with joint_ik the horizon must stay below 3.3 s (22 joint-reference knots, one every 0.15 s); a longer one is refused, not resampled onto fewer knots"

extern "C" {

int32_t hb_refgen_reset(hb_ctx* ctx, const hb_refgen_config* cfg, const double* latest_stance) {
  HB_ENTER(!cfg || !(cfg->dt > 0.0));
  RefgenBatch& r = ctx->rg;
  bool fresh = false;
  HB_TRY(ensure_fields(ctx, r, &fresh));
  if (fresh) ctx->rg_have_schedule.assign(size_t(ctx->B), 0);
  ctx->rg_cfg = *cfg;
  r.init_stance = latest_stance ? 0 : 1;
  HB_TRY(push(ctx, latest_stance, r, r.stance, whole(ctx)));
  ctx->rg_ready = true;
  return HB_OK;
}

int32_t hb_refgen_set_schedule(hb_ctx* ctx, int32_t i0, int32_t cnt, const int32_t* n_events, const double* event_times,
                               const int32_t* modes) {
  HB_ENTER_ARGS(!n_events || !event_times || !modes || !range_ok(ctx, i0, cnt, 1));
  HB_FAIL_IF(!ctx->rg_ready, HB_ERR_STATE, "hb_refgen_set_schedule: call hb_refgen_reset first");
  HB_FAIL_IF(ctx->gait_on, HB_ERR_STATE, "hb_refgen_set_schedule: the device gait manager writes the schedules (hb_gait_reset); call hb_gait_disable to supply them from the host");
  for (int i = 0; i < cnt; ++i) {
    HB_FAIL_IF(n_events[i] < 0 || n_events[i] > HB_MAX_EVENTS, HB_ERR_ARG, "hb_refgen_set_schedule: n_events out of range");
    for (int e = 0; e <= n_events[i]; ++e) {
      const int m = modes[size_t(i) * (HB_MAX_EVENTS + 1) + e];
      HB_FAIL_IF(m < 0 || m > 3, HB_ERR_ARG, "hb_refgen_set_schedule: mode out of range");
    }
  }
  HB_ENTER_DEVICE();
  RefgenBatch& r = ctx->rg;
  HB_TRY(push(ctx, n_events, r, r.n_ev, Range{i0, cnt}));
  HB_TRY(push(ctx, event_times, r, r.ev, Range{i0, cnt}));
  HB_TRY(push(ctx, modes, r, r.modes, Range{i0, cnt}));
  for (int i = 0; i < cnt; ++i) ctx->rg_have_schedule[i0 + i] = 1;
  return HB_OK;
}

// Reference generation of the instances of b / r (instances [i0, i0 + b.B) of the context): planner, joint IK (when configured), node
// tables.  With the gait manager on, k_gait first: it writes the schedule window the planner reads, and the three kernels take the
// filtered command of the gait state instead of the uploaded one.
// init_flag: the respawn's pending flags of these instances, or null (hb_refgen_update alone consumes them).
static void launch_refgen(const hb_ctx* ctx, const Batch& b, RefgenBatch r, int i0, double horizon, hipStream_t s, const int* init_flag = nullptr) {
  if (ctx->gait_on) {
    const GaitBatch g = view(ctx->gait, ctx->Nmax, i0, b.B);
    hipLaunchKernelGGL(k_gait, dim3((b.B + 63) / 64), dim3(64), 0, s, b, r, g, ctx->gait_cfg, horizon);
    r.cmd = g.cmd;
  }
  const GroundForm gf = use_ground_forms(ctx->ground_on, ctx->gfield_on);
  if (use_sole_forms(gf, ctx->foothold_cfg.mode)) {   // the two points of a foot planned as one sole (hb_ground_set_foothold)
    const SoleBatch sb = view(ctx->sole, ctx->Nmax, i0, b.B);
    if (gf == GroundForm::Field)
      hipLaunchKernelGGL(k_refgen_gfield_sole, dim3((4 * b.B + 63) / 64), dim3(64), 0, s, b, r, view(ctx->gfield, ctx->Nmax, i0, b.B), ctx->dmodel,
                         ctx->rg_cfg, horizon, init_flag, ctx->foothold_cfg, sb);
    else
      hipLaunchKernelGGL(k_refgen_ground_sole, dim3((4 * b.B + 63) / 64), dim3(64), 0, s, b, r, view(ctx->ground, ctx->Nmax, i0, b.B), ctx->dmodel,
                         ctx->rg_cfg, horizon, init_flag, ctx->foothold_cfg, sb);
  } else if (gf == GroundForm::Field)   // the planner on the field map of these instances (hb_ground_set_field)
    hipLaunchKernelGGL(k_refgen_gfield, dim3((4 * b.B + 63) / 64), dim3(64), 0, s, b, r, view(ctx->gfield, ctx->Nmax, i0, b.B), ctx->dmodel, ctx->rg_cfg,
                       horizon, init_flag);
  else if (gf == GroundForm::Profile)   // the planner on the ground map of these instances (hb_ground_set_profile)
    hipLaunchKernelGGL(k_refgen_ground, dim3((4 * b.B + 63) / 64), dim3(64), 0, s, b, r, view(ctx->ground, ctx->Nmax, i0, b.B), ctx->dmodel, ctx->rg_cfg,
                       horizon, init_flag);
  else
    hipLaunchKernelGGL(k_refgen, dim3((4 * b.B + 63) / 64), dim3(64), 0, s, b, r, ctx->dmodel, ctx->rg_cfg, horizon, init_flag);
  if (ctx->rg_cfg.joint_ik)
    hipLaunchKernelGGL(k_refgen_ik, dim3((2 * b.B + 7) / 8), dim3(64), 0, s, b, r, ctx->dmodel, ctx->rg_cfg, horizon);
  hipLaunchKernelGGL(k_refgen_nodes, dim3((b.B * ctx->Nmax + 63) / 64), dim3(64), 0, s, b, r, ctx->rg_cfg);
}

int32_t hb_refgen_update(hb_ctx* ctx, const double* t0, double horizon, const double* x_now, const double* cmd_vel, int32_t* status) {
  HB_ENTER_ARGS(!t0 || !cmd_vel || !(horizon > 0.0));
  HB_FAIL_IF(!ctx->rg_ready, HB_ERR_STATE, "hb_refgen_update: call hb_refgen_reset first");
  HB_FAIL_IF(rg_horizon_over_knot_bound(ctx->rg_cfg, horizon), HB_ERR_ARG, RG_KNOT_BOUND_TEXT("hb_refgen_update"));
  for (int v : ctx->rg_have_schedule)
    HB_FAIL_IF(!v && !ctx->gait_on, HB_ERR_STATE, "hb_refgen_update: an instance has no mode schedule (hb_refgen_set_schedule)");
  HB_ENTER_DEVICE();
  RefgenBatch& r = ctx->rg;
  hipStream_t s = ctx->s_mpc;  // the tables belong to the MPC side
  HB_TRY(save_grid_before_table_update(ctx, 0, ctx->B));
  if (status) {
    HB_TRY(push(ctx, t0, r, r.t0, whole(ctx), &s));
    HB_TRY(push(ctx, cmd_vel, r, r.cmd, whole(ctx), &s));
    HB_TRY(push(ctx, x_now, ctx->b, ctx->b.x0, whole(ctx), &s));
  } else {  // enqueue-only form (status through hb_refgen_get_status)
    HB_TRY(stage_upload(ctx, ST_T0, r, r.t0, t0, s));
    HB_TRY(stage_upload(ctx, ST_CMD, r, r.cmd, cmd_vel, s));
    if (x_now) HB_TRY(stage_upload(ctx, ST_X0, ctx->b, ctx->b.x0, x_now, s));
  }
  // a respawn enqueued since the last update: its instances take their latest stance positions from this call's observation, once
  bool respawned = false;
  {
    std::lock_guard<std::mutex> lk(ctx->mtx);
    respawned = ctx->respawn_on && ctx->rs_rg_due;
    ctx->rs_rg_due = false;
  }
  launch_refgen(ctx, ctx->b, r, 0, horizon, s, respawned ? ctx->respawn.rg_pending : nullptr);
  HB_HIP(hipGetLastError());
  if (respawned) HB_TRY(zero_field(ctx, ctx->respawn, ctx->respawn.rg_pending, &s));
  r.init_stance = 0;
  ++ctx->mpc_tables_epoch;
  if (status) {
    HB_TRY(pull(ctx, status, r, r.status, whole(ctx), &s));
    HB_HIP(hipStreamSynchronize(s));
  }
  ctx->refs_set = true;
  return HB_OK;
}

int32_t hb_refgen_get_status(hb_ctx* ctx, int32_t* status) {
  HB_ENTER_ARGS(!status);
  HB_FAIL_IF(!ctx->rg_ready, HB_ERR_STATE, "hb_refgen_get_status: call hb_refgen_reset first");
  HB_ENTER_DEVICE();
  HB_TRY(pull(ctx, status, ctx->rg, ctx->rg.status, whole(ctx), &ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  return HB_OK;
}

int32_t hb_refgen_get_schedule(hb_ctx* ctx, int32_t i0, int32_t cnt, int32_t* n_events, double* event_times, int32_t* modes) {
  HB_ENTER_ARGS(!range_ok(ctx, i0, cnt, 1));
  HB_FAIL_IF(!ctx->rg_ready, HB_ERR_STATE, "hb_refgen_get_schedule: call hb_refgen_reset first");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  RefgenBatch& r = ctx->rg;
  HB_TRY(pull(ctx, n_events, r, r.n_ev, Range{i0, cnt}));
  HB_TRY(pull(ctx, event_times, r, r.ev, Range{i0, cnt}));
  HB_TRY(pull(ctx, modes, r, r.modes, Range{i0, cnt}));
  return HB_OK;
}

// ---- device gait manager ------------------------------------------------------------------------------------------------------
int32_t hb_gait_reset(hb_ctx* ctx, const hb_gait_config* cfg, const uint8_t* mask) {
  HB_ENTER_ARGS(!cfg);
  bool ok = cfg->n_init_events >= 1 && cfg->n_init_events <= HB_GAIT_MAX_INIT_EVENTS && cfg->n_template_phases >= 1 &&
            cfg->n_template_phases <= HB_GAIT_MAX_PHASES && cfg->phase_transition_stance_time >= 0.0 && (cfg->filter_cmd == 0 || cfg->filter_cmd == 1) &&
            cfg->reserved == 0;
  for (int k = 0; ok && k <= cfg->n_init_events; ++k) ok = cfg->init_modes[k] >= 0 && cfg->init_modes[k] <= 3;
  for (int k = 0; ok && k + 1 < cfg->n_init_events; ++k) ok = cfg->init_event_times[k] < cfg->init_event_times[k + 1];
  for (int k = 0; ok && k < cfg->n_template_phases; ++k)
    ok = cfg->template_modes[k] >= 0 && cfg->template_modes[k] <= 3 && cfg->template_switching_times[k] < cfg->template_switching_times[k + 1];
  if (!ok) {
    ctx->err = "hb_gait_reset: hb_gait_config wants 1..8 strictly increasing initial events, a template of 1..8 phases with strictly increasing "
               "switching times, modes in 0..3, phase_transition_stance_time >= 0, filter_cmd 0 / 1 and reserved = 0";
    return HB_ERR_ARG;
  }
  HB_FAIL_IF(!ctx->rg_ready, HB_ERR_STATE, "hb_gait_reset: call hb_refgen_reset first");
  HB_ENTER_DEVICE();
  HB_TRY(hb_sync(ctx));
  GaitBatch& g = ctx->gait;
  bool fresh = false;
  HB_TRY(ensure_fields(ctx, g, &fresh));
  if (fresh) {
    g.stride = ctx->B;
    mask = nullptr;   // first use: every instance starts as a fresh object
  }
  DevBuf<unsigned char> dmask;
  if (mask) HB_HIP(dmask.alloc(size_t(ctx->B), mask));
  hipLaunchKernelGGL(k_gait_reset, dim3((ctx->B + 63) / 64), dim3(64), 0, ctx->s_mpc, g, *cfg, dmask.p);
  HB_HIP(hipGetLastError());
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  ctx->gait_cfg = *cfg;
  if (!ctx->gait_on) {
    ctx->gait_on = true;
    ++ctx->graph_epoch;  // (as hb_wbc_set_certificate: what a range enqueues has changed)
  }
  return HB_OK;
}

int32_t hb_gait_disable(hb_ctx* ctx) {
  HB_ENTER_ARGS(false);
  if (!ctx->gait_on) return HB_OK;
  HB_ENTER_DEVICE();
  HB_TRY(hb_sync(ctx));
  ctx->gait_on = false;
  ++ctx->graph_epoch;
  return HB_OK;
}

int32_t hb_gait_insert_template(hb_ctx* ctx, int32_t i0, int32_t cnt, int32_t n_switch, const double* switching_times, const int32_t* modes,
                                const double* start, const double* final_time) {
  HB_ENTER_ARGS(!switching_times || !modes || !start || !final_time || !range_ok(ctx, i0, cnt, 1));
  bool ok = n_switch >= 2 && n_switch <= HB_GAIT_MAX_PHASES + 1;
  for (int k = 0; ok && k + 1 < n_switch; ++k) ok = modes[k] >= 0 && modes[k] <= 3 && switching_times[k] < switching_times[k + 1];
  HB_FAIL_IF(!ok, HB_ERR_ARG, "hb_gait_insert_template: 2..9 strictly increasing switching times and modes in 0..3");
  HB_FAIL_IF(!ctx->gait_on, HB_ERR_STATE, "hb_gait_insert_template: the device gait manager is not enabled (hb_gait_reset)");
  HB_ENTER_DEVICE();
  HB_TRY(hb_sync(ctx));
  DevBuf<double> dsw, dstart, dfinal;
  DevBuf<int> dmodes;
  HB_HIP(dsw.alloc(n_switch, switching_times));
  HB_HIP(dmodes.alloc(n_switch - 1, modes));
  HB_HIP(dstart.alloc(cnt, start));
  HB_HIP(dfinal.alloc(cnt, final_time));
  hipLaunchKernelGGL(k_gait_insert, dim3((cnt + 63) / 64), dim3(64), 0, ctx->s_mpc, view(ctx->gait, ctx->Nmax, i0, cnt), ctx->gait_cfg.phase_transition_stance_time,
                     n_switch, dsw.p, dmodes.p, dstart.p, dfinal.p);
  HB_HIP(hipGetLastError());
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  return HB_OK;
}

int32_t hb_gait_get_state(hb_ctx* ctx, int32_t i0, int32_t cnt, int32_t* level, double* vel_abs, double* vel_avg, double* cmd, int32_t* n_events,
                          double* event_times, int32_t* modes, int32_t* status) {
  HB_ENTER_ARGS(!range_ok(ctx, i0, cnt, 1));
  HB_FAIL_IF(!has_fields(ctx, ctx->gait), HB_ERR_STATE, "hb_gait_get_state: call hb_gait_reset first");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  GaitBatch& g = ctx->gait;
  const Range r{i0, cnt};
  HB_TRY(pull(ctx, level, g, g.level, r));
  HB_TRY(pull(ctx, vel_abs, g, g.vel_abs, r));
  HB_TRY(pull(ctx, vel_avg, g, g.vel_avg, r));
  HB_TRY(pull(ctx, cmd, g, g.cmd, r));
  HB_TRY(pull(ctx, n_events, g, g.n_ev, r));
  HB_TRY(pull(ctx, status, g, g.status, r));
  HB_TRY(pull_slot_major(ctx, event_times, g, g.ev, r));
  HB_TRY(pull_slot_major(ctx, modes, g, g.modes, r));
  return HB_OK;
}

}  // extern "C"
