// Host side, part 2: the MPC — node tables, cold and warm start, the SQP iteration and its launchers, read-back of the iterate,
// KKT certificate, stage-QP export and the export of the records' recovery data.
#pragma once

extern "C" {

// Before the node tables of b are overwritten while an iterate exists: keeps the grid that iterate lives on (`copy`; tp / modep /
// np_nodes) and marks instances [i0, i0 + cnt) of b dirty, so that the next solve brings them onto the new tables (k_warm_shift).
static int32_t launch_grid_save(hb_ctx* ctx, Batch b, bool copy, int i0, int cnt, hipStream_t s) {
  if (copy) {
    const Range all{0, b.B};
    HB_TRY(copy_field(ctx, hipMemcpyDeviceToDevice, b.t, b, b.tp, all, &s));
    HB_TRY(copy_field(ctx, hipMemcpyDeviceToDevice, b.mode, b, b.modep, all, &s));
    HB_TRY(copy_field(ctx, hipMemcpyDeviceToDevice, b.n_nodes, b, b.np_nodes, all, &s));
  }
  HB_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b.grid_dirty + i0), 1, size_t(cnt), s));
  return HB_OK;
}

// The iterate of b brought onto the current node tables (the previous iterate xp / up is the source).
static void launch_warm_start(const hb_ctx* ctx, const Batch& b, hipStream_t s) {
  hipLaunchKernelGGL(k_warm_shift, dim3(((ctx->Nmax + 1) * HB_NX + kWarmShiftThreads - 1) / kWarmShiftThreads, b.B), dim3(kWarmShiftThreads), 0, s, b,
                     ctx->dmodel);
  hipLaunchKernelGGL(k_grid_clean, dim3((b.B + 255) / 256), dim3(256), 0, s, b);
}

// Called (on the MPC stream) before the whole batch's node tables are written: see launch_grid_save.
static int32_t save_grid_before_table_update(hb_ctx* ctx, int i0, int cnt) {
  if (!ctx->traj_set) return HB_OK;
  HB_TRY(launch_grid_save(ctx, ctx->b, !ctx->grid_saved, i0, cnt, ctx->s_mpc));
  ctx->grid_saved = true;
  return HB_OK;
}

int32_t hb_mpc_set_references(hb_ctx* ctx, int32_t i0, int32_t cnt, const int32_t* n_nodes, const double* t,
                              const int32_t* mode, const double* x_ref, const double* swing_ref) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!n_nodes || !t || !mode || !x_ref || !swing_ref || !range_ok(ctx, i0, cnt, 1), HB_ERR_ARG, "hb_mpc_set_references: bad argument");
  for (int i = 0; i < cnt; ++i)
    HB_FAIL_IF(n_nodes[i] < 1 || n_nodes[i] > ctx->Nmax, HB_ERR_ARG, "hb_mpc_set_references: n_nodes out of range");
  Batch& b = ctx->b;
  const Range r{i0, cnt};
  HB_ENTER_DEVICE();
  HB_TRY(save_grid_before_table_update(ctx, i0, cnt));
  HB_TRY(push(ctx, n_nodes, b, b.n_nodes, r, &ctx->s_mpc));
  HB_TRY(push(ctx, t, b, b.t, r, &ctx->s_mpc));
  HB_TRY(push(ctx, mode, b, b.mode, r, &ctx->s_mpc));
  HB_TRY(push(ctx, x_ref, b, b.xref, r, &ctx->s_mpc));
  HB_TRY(push(ctx, swing_ref, b, b.swing, r, &ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));  // host buffers are caller-owned: safe to reuse on return
  ctx->refs_set = true;
  ++ctx->mpc_tables_epoch;
  return HB_OK;
}

static int32_t mpc_cold_start(hb_ctx* ctx, const double* x0, const uint8_t* mask) {
  HB_FAIL_IF(!ctx->refs_set, HB_ERR_STATE, "hb_mpc_reset: references not set");
  HB_ENTER_DEVICE();
  const size_t B = ctx->B;
  unsigned char* dmask = nullptr;
  if (mask) {
    HB_FAIL_IF(!ctx->traj_set, HB_ERR_STATE, "hb_mpc_reset_masked: no iterate yet (hb_mpc_reset first)");
    if (!ctx->reset_mask) HB_HIP(dalloc(ctx, &ctx->reset_mask, B));
    dmask = ctx->reset_mask;
    HB_HIP(hipMemcpyAsync(dmask, mask, B, hipMemcpyHostToDevice, ctx->s_mpc));
  }
  if (x0) {
    if (!mask) {
      HB_TRY(push(ctx, x0, ctx->b, ctx->b.x0, whole(ctx), &ctx->s_mpc));
    } else {  // only the masked rows of the observation are replaced
      const size_t nx = extent_of(ctx->b, ctx->Nmax, ctx->b.x0).n;
      for (size_t i = 0; i < B; ++i)
        if (mask[i]) HB_TRY(push(ctx, x0 + i * nx, ctx->b, ctx->b.x0, Range{int(i), 1}, &ctx->s_mpc));
    }
  }
  ++ctx->mpc_tables_epoch;
  hipLaunchKernelGGL(k_cold_start, dim3(ctx->Nmax + 1, ctx->B), dim3(64), 0, ctx->s_mpc, ctx->b, ctx->dmodel, dmask);
  HB_HIP(hipGetLastError());
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  if (!mask) ctx->grid_saved = false;  // every instance sits on the current tables
  ctx->traj_set = true;
  return HB_OK;
}

int32_t hb_mpc_reset(hb_ctx* ctx, const double* x0) {
  HB_ENTER_ARGS(false);
  return mpc_cold_start(ctx, x0, nullptr);
}

int32_t hb_mpc_reset_masked(hb_ctx* ctx, const uint8_t* mask, const double* x0) {
  HB_ENTER_ARGS(!mask);
  return mpc_cold_start(ctx, x0, mask);
}

int32_t hb_mpc_get_status(hb_ctx* ctx, int32_t* status) {
  HB_ENTER(!status);
  HB_TRY(pull(ctx, status, ctx->b, ctx->b.mpc_status, whole(ctx), &ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  return HB_OK;
}

int32_t hb_mpc_set_trajectory(hb_ctx* ctx, const double* x, const double* u) {
  HB_ENTER_ARGS(!x || !u);
  HB_ENTER_DEVICE();
  ++ctx->mpc_tables_epoch;
  HB_TRY(push(ctx, x, ctx->b, ctx->b.x, whole(ctx), &ctx->s_mpc));
  HB_TRY(push(ctx, u, ctx->b, ctx->b.u, whole(ctx), &ctx->s_mpc));
  hipLaunchKernelGGL(k_grid_clean, dim3((ctx->B + 255) / 256), dim3(256), 0, ctx->s_mpc, ctx->b);  // given on the current tables
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  ctx->grid_saved = false;
  ctx->traj_set = true;
  return HB_OK;
}

// The tables changed: the iterate becomes the previous iterate, the source of the warm start.
static void swap_iterate(hb_ctx* ctx) {
  std::swap(ctx->b.x, ctx->b.xp);
  std::swap(ctx->b.u, ctx->b.up);
  ++ctx->graph_epoch;  // captured range graphs hold the old pointers
}

// Brings the iterate onto the current node tables if they changed since it was computed (see k_warm_shift); MPC stream.
static int32_t warm_start_onto_new_tables(hb_ctx* ctx) {
  if (!ctx->grid_saved) return HB_OK;
  swap_iterate(ctx);
  launch_warm_start(ctx, ctx->b, ctx->s_mpc);
  HB_HIP(hipGetLastError());
  ctx->grid_saved = false;
  return HB_OK;
}

// The three launchers pick the kernel form by ctx->forms and `concurrent` = the instances whose kernels may be in flight at the same time (hb_forms.hpp:
// use_ric_bwd4, lq_trip_len, use_ric_fwd_wave); the forms agree bit for bit.  `dbg`: the sweeps take hb_config.reserved as an argument (profiling stops).
static void launch_ric_bwd(hb_ctx* ctx, const Batch& b, int B, int concurrent, hipStream_t s) {
  const int dbg = ctx->hconfig.debug_stop;
  if (use_ric_bwd4(ctx->forms, concurrent)) hipLaunchKernelGGL(k_ric_bwd4, dim3(B), dim3(256), 0, s, b, dbg);
  else hipLaunchKernelGGL(k_ric_bwd, dim3(B), dim3(64), 0, s, b, dbg);
}

static void launch_lq(hb_ctx* ctx, const Batch& b, int B, int concurrent, hipStream_t s) {
  if (ctx->forms.lq == KernelForms::Lq::OneNode) { hipLaunchKernelGGL(k_lq, dim3(ctx->Nmax, B), dim3(64), 0, s, b, ctx->dmodel, ctx->dconfig); return; }
  const int len = lq_trip_len(ctx->forms, concurrent, ctx->Nmax, ctx->n_cu);
  const int ntrip = (ctx->Nmax + len - 1) / len;
  hipLaunchKernelGGL(k_lq_trip, dim3(unsigned(ntrip) * B), dim3(64), 0, s, b, ctx->dmodel, ctx->dconfig, len);
}

static void launch_ric_fwd(hb_ctx* ctx, const Batch& b, int B, int concurrent, hipStream_t s) {
  if (use_ric_fwd_wave(ctx->forms, concurrent)) hipLaunchKernelGGL(k_ric_fwd_w, dim3(B), dim3(64), 0, s, b);
  else hipLaunchKernelGGL(k_ric_fwd, dim3(B), dim3(64), 0, s, b);
}

// The SQP iterations of the instances of b (the view of the batch from instance i0 on) on s; `timed`: iteration 0 records the phase
// events ev[EV_LQ_BEGIN .. EV_LS_END].
static int32_t enqueue_sqp(hb_ctx* ctx, const Batch& b, int i0, hipStream_t s, bool timed) {
  const int B = b.B, N = ctx->Nmax;
  const LsList ls = from_instance(ctx->lslist, N, i0);
  const bool ls_node = ctx->forms.ls == KernelForms::Ls::Node;
  // k_ls_tail_eval walks its work list on a bounded grid: eight workgroups per CU are resident (two wavefronts per SIMD)
  const unsigned tail_grid = unsigned(std::min<long>(8L * ctx->n_cu, long(B) * ((N + 31) / 32) * LS_TAIL_MAX));
  for (int it = 0; it < ctx->config.sqp_iterations; ++it) {
    const bool mark = timed && it == 0;
    hipLaunchKernelGGL(k_set_x0, dim3((B * HB_NX + 255) / 256), dim3(256), 0, s, b);
    if (mark) HB_HIP(hipEventRecord(ctx->ev[EV_LQ_BEGIN], s));
    launch_lq(ctx, b, B, ctx->B, s);
    if (mark) HB_HIP(hipEventRecord(ctx->ev[EV_LQ_END], s));
    launch_ric_bwd(ctx, b, B, ctx->B, s);
    if (mark) HB_HIP(hipEventRecord(ctx->ev[EV_RIC_BWD_END], s));
    launch_ric_fwd(ctx, b, B, ctx->B, s);
    if (mark) HB_HIP(hipEventRecord(ctx->ev[EV_RIC_FWD_END], s));
    // filter line search: the full step for every instance, node-parallel; then the backtracking tail in one launch
    // (the refused instances go to the list ls, which the tail walks; the thread-per-node form of the tail does not read it)
    if (ls_node) hipLaunchKernelGGL(k_ls_eval_node, dim3((B * N + 63) / 64), dim3(64), 0, s, b, ls, ctx->dmodel, ctx->dconfig, 1.0);
    else hipLaunchKernelGGL(k_ls_eval, dim3((B * N + 31) / 32), dim3(64), 0, s, b, ls, ctx->dmodel, ctx->dconfig, 1.0);
    hipLaunchKernelGGL(k_ls_decide, dim3(B), dim3(64), 0, s, b, ls, ctx->dconfig, 1.0);
    if (ctx->config.alpha_decay > 0.0 && ctx->config.alpha_decay < 1.0 && ctx->config.alpha_decay >= ctx->config.alpha_min) {
      // step sizes alpha_decay^1, ^2, ... >= alpha_min, in windows of LS_TAIL_MAX = 16 evaluated side by side (the shipped 0.5 / 1e-4
      // makes 13: one window).  A slower decay (0.9 / 1e-4: 88 step sizes) walks on window after window down to alpha_min as OCS2's
      // FilterLinesearch does; an instance that has accepted or given up makes the later windows return at once.  The window's first
      // step size is the running product the sequential search would hold there (same rounding as the kernels' own products).
      double a_win = ctx->config.alpha_decay;
      while (a_win >= ctx->config.alpha_min) {
        int n_alpha = 0;
        double a = a_win;
        for (; a >= ctx->config.alpha_min && n_alpha < LS_TAIL_MAX; a *= ctx->config.alpha_decay) ++n_alpha;
        if (ls_node)
          hipLaunchKernelGGL(k_ls_tail_eval_node, dim3((B * N + 63) / 64, n_alpha), dim3(64), 0, s, b, ctx->dmodel, ctx->dconfig, a_win,
                             ctx->config.alpha_decay, ctx->config.alpha_min);
        else
          hipLaunchKernelGGL(k_ls_tail_eval, dim3(tail_grid), dim3(64), 0, s, b, ls, ctx->dmodel, ctx->dconfig, a_win, ctx->config.alpha_decay,
                             ctx->config.alpha_min, n_alpha);
        hipLaunchKernelGGL(k_ls_tail_decide, dim3(B), dim3(64), 0, s, b, ctx->dconfig, a_win, ctx->config.alpha_decay,
                           ctx->config.alpha_min, n_alpha);
        a_win = a;
      }
    }
    if (mark) HB_HIP(hipEventRecord(ctx->ev[EV_LS_END], s));
    // evaluated per iteration: ric_fail / accepted are overwritten by the next one
    hipLaunchKernelGGL(k_mpc_status, dim3((B + 255) / 256), dim3(256), 0, s, b, it == 0 ? 1 : 0);
  }
  HB_HIP(hipGetLastError());
  return HB_OK;
}

// MPC solve of the whole batch on the MPC stream: warm start onto new tables, the timed SQP iterations, the solve counted.
static int32_t mpc_solve_batch(hb_ctx* ctx) {
  HB_TRY(warm_start_onto_new_tables(ctx));
  // a respawn enqueued since the last solve: its instances start cold from this call's observation, once (hb_mpc_reset_masked semantics)
  bool respawned = false;
  {
    std::lock_guard<std::mutex> lk(ctx->mtx);
    respawned = ctx->respawn_on && ctx->rs_mpc_due;
    ctx->rs_mpc_due = false;
  }
  if (respawned) {
    hipLaunchKernelGGL(k_cold_start, dim3(ctx->Nmax + 1, ctx->B), dim3(64), 0, ctx->s_mpc, ctx->b, ctx->dmodel, ctx->respawn.mpc_pending);
    HB_HIP(hipGetLastError());
    HB_TRY(zero_field(ctx, ctx->respawn, ctx->respawn.mpc_pending, &ctx->s_mpc));
  }
  HB_TRY(enqueue_sqp(ctx, ctx->b, 0, ctx->s_mpc, true));
  std::lock_guard<std::mutex> lk(ctx->mtx);
  ctx->timed = true;
  ctx->stats.n_mpc_solves += ctx->B;
  ctx->mpc_solved_epoch = ctx->mpc_tables_epoch;
  ctx->ls_per = ctx->B;
  return HB_OK;
}

int32_t hb_mpc_solve(hb_ctx* ctx, const double* x0) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->refs_set || !ctx->traj_set, HB_ERR_STATE, "hb_mpc_solve: call hb_mpc_set_references and hb_mpc_reset/hb_mpc_set_trajectory first");
  HB_ENTER_DEVICE();
  if (x0) {
    HB_TRY(push(ctx, x0, ctx->b, ctx->b.x0, whole(ctx), &ctx->s_mpc));
    HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  }
  return mpc_solve_batch(ctx);
}

int32_t hb_mpc_get_solution(hb_ctx* ctx, int32_t i0, int32_t cnt, double* x, double* u) {
  HB_ENTER(!range_ok(ctx, i0, cnt, 1));
  HB_TRY(pull(ctx, x, ctx->b, ctx->b.x, Range{i0, cnt}, &ctx->s_mpc));
  HB_TRY(pull(ctx, u, ctx->b, ctx->b.u, Range{i0, cnt}, &ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  return HB_OK;
}

int32_t hb_mpc_get_step(hb_ctx* ctx, double* dx, double* du) {
  HB_ENTER(false);
  HB_TRY(pull(ctx, dx, ctx->b, ctx->b.dx, whole(ctx), &ctx->s_mpc));
  HB_TRY(pull(ctx, du, ctx->b, ctx->b.du, whole(ctx), &ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  return HB_OK;
}

int32_t hb_mpc_get_performance(hb_ctx* ctx, double* perf) {
  HB_ENTER(!perf);
  HB_TRY(pull(ctx, perf, ctx->b, ctx->b.perf, whole(ctx), &ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  return HB_OK;
}

int32_t hb_mpc_get_references(hb_ctx* ctx, int32_t i0, int32_t cnt, int32_t* n_nodes, double* t, int32_t* mode, double* x_ref,
                              double* swing_ref) {
  HB_ENTER_ARGS(!range_ok(ctx, i0, cnt, 1));
  HB_FAIL_IF(!ctx->refs_set, HB_ERR_STATE, "hb_mpc_get_references: references not set");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  Batch& b = ctx->b;
  const Range r{i0, cnt};
  HB_TRY(pull(ctx, n_nodes, b, b.n_nodes, r));
  HB_TRY(pull(ctx, t, b, b.t, r));
  HB_TRY(pull(ctx, mode, b, b.mode, r));
  HB_TRY(pull(ctx, x_ref, b, b.xref, r));
  HB_TRY(pull(ctx, swing_ref, b, b.swing, r));
  return HB_OK;
}

// The records, gains and step on the device are those of the last MPC call, on the tables and the iterate it ran on
static int32_t mpc_records_current(hb_ctx* ctx, const char* who) {
  if (ctx->mpc_solved_epoch == 0) {
    ctx->err = std::string(who) + ": no MPC call has completed on this context (hb_mpc_solve, hb_step_resident, hb_tick_resident)";
    return HB_ERR_STATE;
  }
  if (ctx->mpc_solved_epoch != ctx->mpc_tables_epoch) {
    ctx->err = std::string(who) + ": the node tables or the iterate were replaced since the last MPC call (hb_mpc_set_references, "
               "hb_refgen_update, hb_mpc_reset, hb_mpc_reset_masked, hb_mpc_set_trajectory): solve again first";
    return HB_ERR_STATE;
  }
  return HB_OK;
}

int32_t hb_mpc_get_certificate(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, double* cert, double* costate, double* u_til) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!range_ok(ctx, inst_begin, inst_count, 1), HB_ERR_ARG, "hb_mpc_get_certificate: instance range outside the batch");
  HB_TRY(mpc_records_current(ctx, "hb_mpc_get_certificate"));
  HB_ENTER_DEVICE();
  MpcCertBuf& m = ctx->mcert;
  HB_TRY(ensure_fields(ctx, m));
  const Range r{inst_begin, inst_count};
  const Batch b = view(ctx->b, ctx->Nmax, inst_begin, inst_count);
  const MpcCertBuf v = from_instance(m, ctx->Nmax, inst_begin);
  hipStream_t s = ctx->s_mpc;
  hipLaunchKernelGGL(k_mpc_cert_nodes, dim3(ctx->Nmax, inst_count), dim3(64), 0, s, b, v);
  hipLaunchKernelGGL(k_mpc_cert_sweep, dim3(inst_count), dim3(64), 0, s, b, v);
  HB_HIP(hipGetLastError());
  HB_TRY(pull(ctx, cert, m, m.cert, r, &s));
  HB_TRY(pull(ctx, costate, m, m.costate, r, &s));
  HB_TRY(pull(ctx, u_til, m, m.util, r, &s));
  HB_HIP(hipStreamSynchronize(s));
  return HB_OK;
}

// What hb_mpc_get_lq and hb_mpc_get_recovery share: the checks, the node count n of instance `inst` (clamped to [0, max_nodes]) and its
// records, pulled on the MPC stream and synchronised.
static int32_t pull_instance_records(hb_ctx* ctx, const char* who, int32_t inst, std::vector<double>& recs, int& n) {
  if (inst < 0 || inst >= ctx->B) {
    ctx->err = std::string(who) + ": instance outside the batch";
    return HB_ERR_ARG;
  }
  HB_TRY(mpc_records_current(ctx, who));
  HB_ENTER_DEVICE();
  recs.resize(extent_of(ctx->b, ctx->Nmax, ctx->b.recs).n);
  n = 0;
  HB_TRY(pull(ctx, &n, ctx->b, ctx->b.n_nodes, Range{inst, 1}, &ctx->s_mpc));
  HB_TRY(pull(ctx, recs.data(), ctx->b, ctx->b.recs, Range{inst, 1}, &ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  n = std::max(0, std::min(n, ctx->Nmax));
  return HB_OK;
}

int32_t hb_mpc_get_lq(hb_ctx* ctx, int32_t inst, double* A, double* B, double* b, double* Q, double* P, double* R, double* q, double* r,
                      int32_t* n_til) {
  HB_ENTER_ARGS(false);
  std::vector<double> recs;
  int n = 0;
  HB_TRY(pull_instance_records(ctx, "hb_mpc_get_lq", inst, recs, n));
  const size_t N = ctx->Nmax;
  const auto zero = [N](double* p, size_t per) { if (p) std::memset(p, 0, N * per * 8); };   // rows k >= n stay zero
  zero(A, 22 * 22); zero(B, 22 * NU_T); zero(b, 22); zero(Q, 22 * 22); zero(P, NU_T * 22); zero(R, NU_T * NU_T); zero(q, 22); zero(r, NU_T);
  if (n_til) std::memset(n_til, 0, N * sizeof(int32_t));
  for (size_t k = 0; k < size_t(n); ++k) {
    int nt = 0;
    rec_unpack(recs.data() + k * REC_SIZE, A ? A + k * 484 : nullptr, B ? B + k * 264 : nullptr, b ? b + k * 22 : nullptr,
               Q ? Q + k * 484 : nullptr, P ? P + k * 264 : nullptr, R ? R + k * 144 : nullptr, q ? q + k * 22 : nullptr,
               r ? r + k * 12 : nullptr, &nt);
    if (n_til) n_til[k] = nt;
  }
  return HB_OK;
}

int32_t hb_mpc_get_recovery(hb_ctx* ctx, int32_t inst, double* Kx, double* ke, double* Z, double* dF, double* qf, double* rf, double* meta,
                            double* dt, double* dq) {
  HB_ENTER_ARGS(false);
  std::vector<double> recs;
  int n = 0;
  HB_TRY(pull_instance_records(ctx, "hb_mpc_get_recovery", inst, recs, n));
  const size_t N = ctx->Nmax;
  const auto zero = [N](double* p, size_t per) { if (p) std::memset(p, 0, N * per * 8); };   // rows k >= n stay zero
  zero(Kx, 220); zero(ke, 10); zero(Z, 60); zero(dF, 12); zero(qf, 22); zero(rf, 22); zero(meta, 6); zero(dt, 1); zero(dq, 10);
  const auto at = [](double* p, size_t k, size_t per) { return p ? p + k * per : nullptr; };
  for (size_t k = 0; k < size_t(n); ++k)
    rec_unpack_recovery(recs.data() + k * REC_SIZE, at(Kx, k, 220), at(ke, k, 10), at(Z, k, 60), at(dF, k, 12), at(qf, k, 22), at(rf, k, 22),
                        at(meta, k, 6), at(dt, k, 1), at(dq, k, 10));
  return HB_OK;
}

// The line-search state of the last SQP iteration of the last MPC call, as the kernels left it (Batch fields of the same names): copies only.
int32_t hb_mpc_get_linesearch(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, double* acc, double* partial, double* ls_tail, double* ls_norm,
                              int32_t* accepted, int32_t* ric_fail) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!range_ok(ctx, inst_begin, inst_count, 1), HB_ERR_ARG, "hb_mpc_get_linesearch: instance range outside the batch");
  HB_TRY(mpc_records_current(ctx, "hb_mpc_get_linesearch"));
  HB_ENTER_DEVICE();
  const Range r{inst_begin, inst_count};
  Batch& b = ctx->b;
  hipStream_t s = ctx->s_mpc;
  HB_TRY(pull(ctx, acc, b, b.acc, r, &s));
  HB_TRY(pull(ctx, partial, b, b.partial, r, &s));
  HB_TRY(pull(ctx, ls_tail, b, b.ls_tail, r, &s));
  HB_TRY(pull(ctx, ls_norm, b, b.ls_norm, r, &s));
  HB_TRY(pull(ctx, accepted, b, b.accepted, r, &s));
  HB_TRY(pull(ctx, ric_fail, b, b.ric_fail, r, &s));
  HB_HIP(hipStreamSynchronize(s));
  return HB_OK;
}

// How many instances the last SQP iteration of the last MPC call put on the list of the backtracking tail: the counters of the instance
// ranges of that call, summed.
int32_t hb_mpc_get_linesearch_refused(hb_ctx* ctx, int32_t* count) {
  HB_ENTER_ARGS(!count);
  HB_TRY(mpc_records_current(ctx, "hb_mpc_get_linesearch_refused"));
  HB_ENTER_DEVICE();
  std::vector<int> slots(size_t(ctx->B));
  HB_TRY(pull(ctx, slots.data(), ctx->lslist, ctx->lslist.count, whole(ctx), &ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  *count = 0;
  for (int i0 = 0; i0 < ctx->B; i0 += ctx->ls_per) *count += slots[size_t(i0)];
  return HB_OK;
}

}  // extern "C"
