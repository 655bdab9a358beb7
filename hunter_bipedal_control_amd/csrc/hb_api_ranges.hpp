// Host side, part 9: instance ranges (hb_set_chunks), hb_step_resident, hb_tick_resident and the range graphs.
#pragma once

extern "C" {

int32_t hb_set_resident_x0_sequence(hb_ctx* ctx, int32_t n_seq, const double* x0_seq) {
  HB_ENTER(n_seq < 0 || (n_seq > 0 && !x0_seq));
  ctx->n_seq = 0;
  ctx->seq_idx = 0;
  ++ctx->graph_epoch;
  if (n_seq == 0) return HB_OK;
  const size_t bytes = size_t(n_seq) * field_count(ctx, ctx->b, ctx->b.x0) * 8;
  HB_FAIL_IF(hipMalloc(reinterpret_cast<void**>(&ctx->x0_seq), bytes) != hipSuccess, HB_ERR_DEVICE, "hb_set_resident_x0_sequence: hipMalloc failed");
  ctx->allocs.push_back(ctx->x0_seq);
  HB_HIP(hipMemcpy(ctx->x0_seq, x0_seq, bytes, hipMemcpyHostToDevice));
  ctx->n_seq = n_seq;
  return HB_OK;
}

// ---- instance ranges (hb_set_chunks > 1) --------------------------------------------------------------------------------------
// A chunked hb_step_resident / hb_tick_resident runs every range of instances on a stream of its own, which goes from one call straight
// into the next (instances are independent) without a per-call join (lazy_join).

// SQP iterations, publish, policy evaluation and WBC of the instance range [i0, i0 + cnt) on s: the tail of a range's step and tick.
static int32_t enqueue_range_update(hb_ctx* ctx, int i0, int cnt, hipStream_t s) {
  const Batch b = view(ctx->b, ctx->Nmax, i0, cnt);
  const WbcBatch w = view(ctx->w, ctx->Nmax, i0, cnt);
  HB_TRY(enqueue_sqp(ctx, b, i0, s, false));
  launch_publish(b, w, s);
  return launch_policy_wbc(ctx, w, i0, true, nullptr, s);
}

// Fork, only when another entry point ran since the last chunked call, the tables changed or the range count did (`fork` tells): the
// range streams start after everything queued so far on the MPC stream (table updates, warm start, resident-input writers ordered
// into it) and on the WBC stream (resident rbd / time writers, the last reader of the policy buffers).
static int32_t fork_ranges(hb_ctx* ctx, bool& fork) {
  fork = ctx->fork_needed || ctx->grid_saved || ctx->chunks_pending != ctx->n_chunks;
  if (!fork) return HB_OK;
  ++ctx->dbg_forks;
  lazy_join(ctx);
  HB_TRY(warm_start_onto_new_tables(ctx));
  HB_HIP(hipEventRecord(ctx->ev_sync[SYNC_FORK_MPC], ctx->s_mpc));
  HB_HIP(hipEventRecord(ctx->ev_sync[SYNC_FORK_WBC], ctx->s_wbc));
  return HB_OK;
}

extern "C++" {
// body(c, i0, cnt, s) enqueues range c, instances [i0, i0 + cnt), on its stream s: behind the fork points when `fork`, ahead of the
// range's join point.
template <class F>
static int32_t for_each_range(hb_ctx* ctx, bool fork, F&& body) {
  const int per = (ctx->B + ctx->n_chunks - 1) / ctx->n_chunks;
  int used = 0;
  for (int c = 0; c < ctx->n_chunks; ++c) {
    const int i0 = c * per, cnt = std::min(per, ctx->B - i0);
    if (cnt <= 0) break;
    hipStream_t s = ctx->s_chunk[c];
    if (fork) {
      HB_HIP(hipStreamWaitEvent(s, ctx->ev_sync[SYNC_FORK_MPC], 0));
      HB_HIP(hipStreamWaitEvent(s, ctx->ev_sync[SYNC_FORK_WBC], 0));
    }
    HB_TRY(body(c, i0, cnt, s));
    HB_HIP(hipGetLastError());
    HB_HIP(hipEventRecord(ctx->ev_sync[SYNC_JOIN + c], s));
    used = c + 1;
  }
  ctx->chunks_pending = used;
  return HB_OK;
}

// The step of range c, enqueue() on s: with `graphable`, one launch of a hipGraph of it (captured on first use in the graph epoch, kept
// in `slot`), else direct launches.
template <class F>
static int32_t enqueue_range_step(hb_ctx* ctx, int c, int slot, bool graphable, hipStream_t s, F&& enqueue) {
  if (graphable) {
    hipGraphExec_t& ge = ctx->chunk_graph[c][slot];
    if (ge && ctx->chunk_graph_epoch[c][slot] != ctx->graph_epoch) { (void)hipGraphExecDestroy(ge); ge = nullptr; }
    if (!ge && !ctx->graph_disabled) {
      hipGraph_t g = nullptr;
      bool ok = false;
      if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        const int32_t rc = enqueue();
        const hipError_t ce = hipStreamEndCapture(s, &g);
        ++ctx->dbg_captures;
        ok = rc == HB_OK && ce == hipSuccess && g && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess;
        if (g) (void)hipGraphDestroy(g);
      }
      if (ok) {
        ctx->chunk_graph_epoch[c][slot] = ctx->graph_epoch;
      } else {
        // a capture / instantiation that fails once is not retried on every step (it would double the host cost for good):
        // this context steps its ranges with direct launches from now on; hb_debug_chunk_counters reports the failure
        ge = nullptr;
        ctx->graph_disabled = true;
        ++ctx->dbg_capture_failures;
      }
      (void)hipGetLastError();
    }
    if (ge && hipGraphLaunch(ge, s) == hipSuccess) {
      ++ctx->dbg_graph_launches;
      return HB_OK;
    }
  }
  ++ctx->dbg_direct;
  return enqueue();
}
}  // extern "C++"

// End of a chunked step / tick: every range has solved, published and read its policy.  `steady`: the call did not fork.
static void finish_ranges(hb_ctx* ctx, bool steady) {
  ctx->fork_needed = false;
  ctx->steady_chunked_steps = steady ? ctx->steady_chunked_steps + 1 : 0;
  std::lock_guard<std::mutex> lk(ctx->mtx);
  ctx->w.policy_valid = true;
  ctx->policy_read_pending = false;  // the lazy join orders the next policy write (by another entry point) after these readers
  ctx->stats.n_mpc_solves += ctx->B;
  ctx->stats.n_wbc_solves += ctx->B;
  ctx->cert_last = ctx->wbc_cert;
  ctx->mpc_solved_epoch = ctx->mpc_tables_epoch;
  ctx->ls_per = (ctx->B + ctx->n_chunks - 1) / ctx->n_chunks;   // (for_each_range)
}

int32_t hb_step_resident(hb_ctx* ctx, double dt) {
  if (!ctx) return HB_ERR_ARG;
  HB_FAIL_IF(ctx->respawn_on, HB_ERR_STATE, "hb_step_resident: a respawn configuration is in force (hb_plant_set_respawn): the instance-range / graph paths do not consume its pending flags; clear it first");
  HB_FAIL_IF(!ctx->refs_set || !ctx->traj_set, HB_ERR_STATE, "hb_step_resident: references / trajectory not initialised");
  HB_ENTER_DEVICE();
  const double* x0_next = nullptr;
  const int seq_slot = ctx->seq_idx;
  if (ctx->n_seq > 0) {
    x0_next = ctx->x0_seq + size_t(ctx->seq_idx) * field_count(ctx, ctx->b, ctx->b.x0);
    ctx->seq_idx = (ctx->seq_idx + 1) % ctx->n_seq;
  }
  if (ctx->n_chunks <= 1) {
    lazy_join(ctx);
    if (x0_next) HB_TRY(copy_field(ctx, hipMemcpyDeviceToDevice, x0_next, ctx->b, ctx->b.x0, whole(ctx), &ctx->s_mpc));
    HB_TRY(mpc_solve_batch(ctx));
    HB_TRY(hb_mpc_publish(ctx));
    HB_TRY(wbc_launch(ctx, true));
    // hb_mpc_publish already orders the next policy write after this step's policy evaluation.  The next step's SQP
    // kernels are additionally held back until this WBC has finished: letting them time-slice the CUs with the WBC
    // cost throughput (re-measured in round 2 with the lighter WBC: 367 k -> 357 k updates/s; the LQ kernel fills every
    // CU's LDS) and blurred the per-kernel timings.
    HB_HIP(hipStreamWaitEvent(ctx->s_mpc, ctx->ev[EV_WBC_END], 0));
    return HB_OK;
  }
  // pipelined: every range of instances is a linear sequence x0 -> MPC -> publish -> policy evaluation -> WBC on its own stream, and
  // consecutive steps of one range follow each other on that stream without waiting for the other ranges: the per-instance sweeps of
  // one range (k_ric_bwd: a serial chain over the horizon that leaves most SIMDs idle at small batch sizes) overlap the LQ kernel of
  // the others, across step boundaries.
  bool fork;
  HB_TRY(fork_ranges(ctx, fork));
  // steady state (no fork for a few steps, the x0 slot fits): the step of a range is replayed as one graph launch
  const int slot = ctx->n_seq > 0 ? seq_slot : 0;
  const bool graphable = !fork && ctx->steady_chunked_steps >= 2 && slot < hb_ctx::GRAPH_SLOTS && ctx->n_seq <= hb_ctx::GRAPH_SLOTS;
  HB_TRY(for_each_range(ctx, fork, [&](int c, int i0, int cnt, hipStream_t s) {
    return enqueue_range_step(ctx, c, slot, graphable, s, [&]() -> int32_t {
      if (x0_next) HB_TRY(copy_field(ctx, hipMemcpyDeviceToDevice, x0_next, ctx->b, ctx->b.x0, Range{i0, cnt}, &s));
      return enqueue_range_update(ctx, i0, cnt, s);
    });
  }));
  finish_ranges(ctx, !fork);
  return HB_OK;
}

// One whole tick on the resident state — controller time, estimator, reference generation at that time, one MPC iteration, publish,
// policy evaluation, WBC — enqueue-only.  With instance ranges (hb_set_chunks > 1) every range runs ITS slice of all of that on its
// own stream and goes from one tick straight into the next: the small per-instance kernels of the estimator and the reference
// generation (thread- or wave-per-instance, a fraction of the chip each) and the serial sweeps of one range run under the LQ
// kernel of the others instead of in a whole-batch prologue between two steps.  The host inputs of a tick are uploaded once, on
// their own stream, into buffers that every range reads EARLY in its tick (estimator, reference generation, a private copy of the
// time): the next tick's upload waits only for that point, so ranges may be up to one tick apart.
int32_t hb_tick_resident(hb_ctx* ctx, double dt_est, const double* quat, const double* ang_vel_local, const double* lin_acc_local,
                         const double* joint_pos, const double* joint_vel, const int32_t* contact_flag, const double* t_now, double horizon,
                         const double* cmd_vel, double dt_wbc) {
  if (!ctx || !quat || !ang_vel_local || !lin_acc_local || !joint_pos || !joint_vel || !contact_flag || !t_now || !cmd_vel || !(dt_est > 0.0) ||
      !(horizon > 0.0))
    return HB_ERR_ARG;
  HB_FAIL_IF(ctx->rg_ready && rg_horizon_over_knot_bound(ctx->rg_cfg, horizon), HB_ERR_ARG, RG_KNOT_BOUND_TEXT("hb_tick_resident"));
  HB_FAIL_IF(ctx->respawn_on, HB_ERR_STATE, "hb_tick_resident: a respawn configuration is in force (hb_plant_set_respawn): the instance-range / graph paths do not consume its pending flags; clear it first");
  if (ctx->n_chunks <= 1) {  // one stream: the four calls themselves (enqueue-only forms)
    HB_TRY(hb_set_resident_time(ctx, t_now));
    HB_TRY(hb_estimator_update(ctx, dt_est, quat, ang_vel_local, lin_acc_local, joint_pos, joint_vel, contact_flag, 1, nullptr, nullptr));
    HB_TRY(hb_refgen_update(ctx, t_now, horizon, nullptr, cmd_vel, nullptr));
    return hb_step_resident(ctx, dt_wbc);
  }
  HB_FAIL_IF(!ctx->est_ready || !ctx->rg_ready || !ctx->refs_set || !ctx->traj_set, HB_ERR_STATE, "hb_tick_resident: estimator / reference generation / references / trajectory not initialised");
  for (int v : ctx->rg_have_schedule)
    HB_FAIL_IF(!v && !ctx->gait_on, HB_ERR_STATE, "hb_tick_resident: an instance has no mode schedule (hb_refgen_set_schedule)");
  HB_ENTER_DEVICE();
  TickUpload& up = ctx->up;
  if (!ctx->s_up) {
    HB_HIP(hipStreamCreateWithFlags(&ctx->s_up, hipStreamNonBlocking));
    HB_HIP(hipEventCreateWithFlags(&ctx->ev_up, hipEventDisableTiming));
    for (auto& ev : ctx->ev_consumed) HB_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HB_HIP(alloc_fields(ctx, up));
  }
  bool fork;
  HB_TRY(fork_ranges(ctx, fork));
  // this tick's host inputs: one upload, after every range has read the previous tick's
  hipStream_t su = ctx->s_up;
  for (int c = 0; c < ctx->consumed_pending; ++c) HB_HIP(hipStreamWaitEvent(su, ctx->ev_consumed[c], 0));
  const void* const src[6] = {quat, ang_vel_local, lin_acc_local, joint_pos, joint_vel, contact_flag};
  double* const* const dst[5] = {&up.quat, &up.w, &up.a, &up.qj, &up.qdj};
  HB_TRY(upload_sensors(ctx, up, dst, up.contact, src, true, su));
  HB_TRY(stage_upload(ctx, ST_TNOW, up, up.tnow, t_now, su));
  HB_TRY(stage_upload(ctx, ST_T0, up, up.t0, t_now, su));
  HB_TRY(stage_upload(ctx, ST_CMD, up, up.cmd, cmd_vel, su));
  HB_HIP(hipEventRecord(ctx->ev_up, su));
  // the tables change for every instance: the previous iterate becomes the source of the warm start (as warm_start_onto_new_tables)
  swap_iterate(ctx);
  // the estimator and the reference generation read this tick's uploads
  EstBatch est = ctx->est;
  est.quat = up.quat; est.w_local = up.w; est.a_local = up.a; est.qj = up.qj; est.qdj = up.qdj; est.contact = up.contact;
  RefgenBatch rg = ctx->rg;
  rg.t0 = up.t0;
  rg.cmd = up.cmd;
  HB_TRY(for_each_range(ctx, fork, [&](int c, int i0, int cnt, hipStream_t s) -> int32_t {
    HB_HIP(hipStreamWaitEvent(s, ctx->ev_up, 0));
    const Batch b = view(ctx->b, ctx->Nmax, i0, cnt);
    const WbcBatch w = view(ctx->w, ctx->Nmax, i0, cnt);
    // controller time + estimator -> resident rbd state and observation of the range
    HB_TRY(copy_field(ctx, hipMemcpyDeviceToDevice, up.tnow, ctx->w, ctx->w.t_now, Range{i0, cnt}, &s));
    EstBatch e = view(est, ctx->Nmax, i0, cnt);
    e.res_rbd = w.rbd;
    e.res_x0 = b.x0;
    launch_estimator(ctx, e, dt_est, s, i0);
    // reference generation at the new time (the grid that is about to be replaced is kept for the warm start)
    HB_TRY(launch_grid_save(ctx, b, true, 0, cnt, s));
    launch_refgen(ctx, b, view(rg, ctx->Nmax, i0, cnt), i0, horizon, s);
    HB_HIP(hipEventRecord(ctx->ev_consumed[c], s));  // the upload buffers are free for the next tick
    // warm start onto the new tables, MPC iteration, publish, policy evaluation, WBC
    launch_warm_start(ctx, b, s);
    return enqueue_range_update(ctx, i0, cnt, s);
  }));
  ctx->rg.init_stance = 0;
  ctx->consumed_pending = ctx->chunks_pending;
  finish_ranges(ctx, false);
  return HB_OK;
}

int32_t hb_debug_chunk_counters(hb_ctx* ctx, int64_t* out4) {
  if (!ctx || !out4) return HB_ERR_ARG;
  out4[0] = ctx->dbg_graph_launches; out4[1] = ctx->dbg_direct; out4[2] = ctx->dbg_forks; out4[3] = ctx->dbg_captures;
  return HB_OK;
}

int32_t hb_debug_graph_state(hb_ctx* ctx, int64_t* out2) {
  if (!ctx || !out2) return HB_ERR_ARG;
  out2[0] = ctx->dbg_capture_failures; out2[1] = ctx->graph_disabled ? 1 : 0;
  return HB_OK;
}

int32_t hb_set_chunks(hb_ctx* ctx, int32_t n_chunks) {
  HB_ENTER_ARGS(n_chunks < 1 || n_chunks > kMaxRanges);
  HB_FAIL_IF(n_chunks > 1 && ctx->scan_on, HB_ERR_STATE, "hb_set_chunks: a height scan is in force (hb_plant_set_height_scan): the scan runs on the whole batch only, turn it off first");
  HB_TRY(hb_sync(ctx));
  ctx->n_chunks = n_chunks;
  ctx->graph_disabled = false;  // a new set of ranges gets a new chance to capture
  ++ctx->graph_epoch;
  return HB_OK;
}

}  // extern "C"
