// Host side, part 3: policy hand-over (publish), policy evaluation and WBC, resident inputs, both WBC certificates.
#pragma once

extern "C" {

// MPC_MRT_Interface::updatePolicy as ONE launch: the iterate (x, u), its time grid, mode sequence and node counts of `cnt` instances become
// the policy the controller evaluates (five device-to-device copies before: five launches with their gaps in every step of every range).
__global__ __launch_bounds__(256) void k_publish(const double* __restrict__ x, const double* __restrict__ u, const double* __restrict__ t,
                                                 const int* __restrict__ mode, const int* __restrict__ n_nodes, double* __restrict__ px,
                                                 double* __restrict__ pu, double* __restrict__ pt, int* __restrict__ pmode, int* __restrict__ pn,
                                                 size_t nx, size_t nu, size_t nt, size_t nm, size_t nn) {
  const size_t total = nx + nu + nt + nm + nn, stride = size_t(gridDim.x) * blockDim.x;
  for (size_t e = size_t(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += stride) {
    if (e < nx) px[e] = x[e];
    else if (e < nx + nu) pu[e - nx] = u[e - nx];
    else if (e < nx + nu + nt) pt[e - nx - nu] = t[e - nx - nu];
    else if (e < nx + nu + nt + nm) pmode[e - nx - nu - nt] = mode[e - nx - nu - nt];
    else pn[e - nx - nu - nt - nm] = n_nodes[e - nx - nu - nt - nm];
  }
}
static void launch_publish(Batch b, const WbcBatch& w, hipStream_t s) {
  const size_t cnt = b.B, N = b.Nmax;
  const auto count = [&](auto* const& field) { return cnt * extent_of(b, N, field).n; };
  const size_t nx = count(b.x), nu = count(b.u), nt = count(b.t), nm = count(b.mode), nn = count(b.n_nodes);
  const size_t total = nx + nu + nt + nm + nn;
  const unsigned blocks = unsigned(std::min<size_t>((total + 256 * 4 - 1) / (256 * 4), 8192));   // four elements per thread, grid-stride beyond
  hipLaunchKernelGGL(k_publish, dim3(blocks), dim3(256), 0, s, b.x, b.u, b.t, b.mode, b.n_nodes, w.px, w.pu, w.pt, w.pmode, w.pn, nx, nu, nt, nm, nn);
}

int32_t hb_mpc_publish(hb_ctx* ctx) {
  HB_ENTER(false);
  // device-to-device copy of the solution into the policy buffers read by the WBC stream
  hipStream_t s = ctx->s_mpc;
  std::lock_guard<std::mutex> lk(ctx->mtx);  // enqueue only: the control thread may be inside hb_wbc_update right now
  // only the copies below touch the policy buffers: they wait for the last policy evaluation on the WBC stream, the SQP
  // kernels of the next solve do not (so a WBC solve overlaps the next LQ approximation)
  if (ctx->policy_read_pending) {
    HB_HIP(hipStreamWaitEvent(s, ctx->ev[EV_POLICY_READ], 0));
    ctx->policy_read_pending = false;
  }
  launch_publish(ctx->b, ctx->w, s);
  HB_HIP(hipEventRecord(ctx->ev[EV_PUBLISHED], s));
  HB_HIP(hipStreamWaitEvent(ctx->s_wbc, ctx->ev[EV_PUBLISHED], 0));
  ctx->w.policy_valid = true;
  return HB_OK;
}

// Policy evaluation (`from_policy`; then policy_read records when the policy buffers are free again) and WBC of the instances of w,
// instances [i0, i0 + w.B) of the batch, on s: the WBC kernel of the configuration and of the certificate switch.
static int32_t launch_policy_wbc(hb_ctx* ctx, const WbcBatch& w, int i0, bool from_policy, hipEvent_t policy_read, hipStream_t s) {
  if (from_policy) {
    hipLaunchKernelGGL(k_policy_eval, dim3((w.B + 63) / 64), dim3(64), 0, s, w, ctx->Nmax, ctx->dconfig);
    if (policy_read) HB_HIP(hipEventRecord(policy_read, s));
  }
  if (ctx->config.wbc_type == 1 && ctx->wbc_cert) {  // (in a range graph: chosen at capture, hb_hwbc_set_certificate re-captures)
    const HwbcCertBuf c = from_instance(ctx->hcert, ctx->Nmax, i0);
    hipLaunchKernelGGL(k_hwbc_cert, dim3(w.B), dim3(64), (HoLdsDev::total + HoCertLds::total) * sizeof(double), s, w, ctx->dmodel, ctx->dconfig, c.cert,
                       c.xlev, c.slack, c.dual);
  } else if (ctx->config.wbc_type == 1)
    hipLaunchKernelGGL(k_hwbc, dim3(w.B), dim3(64), HoLdsDev::total * sizeof(double), s, w, ctx->dmodel, ctx->dconfig);
  else if (ctx->wbc_cert) {  // (in a range graph: chosen at capture, hb_wbc_set_certificate re-captures)
    const WbcCertBuf c = from_instance(ctx->wcert, ctx->Nmax, i0);
    hipLaunchKernelGGL(k_wbc_cert, dim3(w.B), dim3(64), 0, s, w, ctx->dmodel, ctx->dconfig, c.cert, c.dual);
  } else
    hipLaunchKernelGGL(k_wbc, dim3(w.B), dim3(64), 0, s, w, ctx->dmodel, ctx->dconfig);
  return HB_OK;
}

// WBC of the whole batch on the WBC stream, timed (ev[EV_WBC_BEGIN .. EV_WBC_END]) and counted
static int32_t wbc_launch(hb_ctx* ctx, bool from_policy) {
  hipStream_t s = ctx->s_wbc;
  std::lock_guard<std::mutex> lk(ctx->mtx);  // enqueue only (pairs with hb_mpc_publish on the MPC thread)
  HB_HIP(hipEventRecord(ctx->ev[EV_WBC_BEGIN], s));
  HB_TRY(launch_policy_wbc(ctx, ctx->w, 0, from_policy, ctx->ev[EV_POLICY_READ], s));
  if (from_policy) ctx->policy_read_pending = true;
  HB_HIP(hipEventRecord(ctx->ev[EV_WBC_END], s));
  HB_HIP(hipGetLastError());
  ctx->stats.n_wbc_solves += ctx->B;
  ctx->cert_last = ctx->wbc_cert;
  return HB_OK;
}

int32_t hb_wbc_update(hb_ctx* ctx, const double* t_now, const double* rbd, const int32_t* walk_flag, double dt,
                      double* sol, double* x_des, double* u_des, int32_t* planned_mode, int32_t* status) {
  HB_ENTER_ARGS(((t_now == nullptr) != (rbd == nullptr)));
  HB_FAIL_IF(!ctx->w.policy_valid, HB_ERR_STATE, "hb_wbc_update: no published policy (hb_mpc_publish)");
  WbcBatch& w = ctx->w;
  hipStream_t s = ctx->s_wbc;
  const Range all = whole(ctx);
  HB_ENTER_DEVICE();
  // a null time / rbd: the device-resident ones (hb_set_resident_inputs, hb_estimator_update, hb_plant_step)
  HB_TRY(push(ctx, t_now, w, w.t_now, all, &s));
  HB_TRY(push(ctx, rbd, w, w.rbd, all, &s));
  HB_TRY(push(ctx, walk_flag, w, w.walk, all, &s));
  HB_TRY(wbc_launch(ctx, true));
  HB_TRY(pull(ctx, sol, w, w.sol, all, &s));
  HB_TRY(pull(ctx, x_des, w, w.xdes, all, &s));
  HB_TRY(pull(ctx, u_des, w, w.udes, all, &s));
  HB_TRY(pull(ctx, planned_mode, w, w.mode, all, &s));
  HB_TRY(pull(ctx, status, w, w.status, all, &s));
  HB_HIP(hipStreamSynchronize(s));
  return HB_OK;
}

int32_t hb_wbc_update_direct(hb_ctx* ctx, const double* x_des, const double* u_des, const double* rbd, const int32_t* mode,
                             const int32_t* stance_flag, double dt, double* sol, int32_t* status) {
  HB_ENTER_ARGS(!x_des || !u_des || !rbd || !mode);
  WbcBatch& w = ctx->w;
  hipStream_t s = ctx->s_wbc;
  const Range all = whole(ctx);
  HB_ENTER_DEVICE();
  HB_TRY(push(ctx, x_des, w, w.xdes, all, &s));
  HB_TRY(push(ctx, u_des, w, w.udes, all, &s));
  HB_TRY(push(ctx, rbd, w, w.rbd, all, &s));
  HB_TRY(push(ctx, mode, w, w.mode, all, &s));
  if (stance_flag) HB_TRY(push(ctx, stance_flag, w, w.stance, all, &s));
  else HB_TRY(zero_field(ctx, w, w.stance, &s));
  HB_TRY(wbc_launch(ctx, false));
  HB_TRY(pull(ctx, sol, w, w.sol, all, &s));
  HB_TRY(pull(ctx, status, w, w.status, all, &s));
  HB_HIP(hipStreamSynchronize(s));
  return HB_OK;
}

int32_t hb_set_resident_inputs(hb_ctx* ctx, const double* x0, const double* t_now, const double* rbd, const int32_t* walk_flag) {
  HB_ENTER_ARGS(!x0 || !t_now || !rbd);
  HB_ENTER_DEVICE();
  HB_TRY(push(ctx, x0, ctx->b, ctx->b.x0, whole(ctx)));
  HB_TRY(push(ctx, t_now, ctx->w, ctx->w.t_now, whole(ctx)));
  HB_TRY(push(ctx, rbd, ctx->w, ctx->w.rbd, whole(ctx)));
  HB_TRY(push(ctx, walk_flag, ctx->w, ctx->w.walk, whole(ctx)));
  return HB_OK;
}

int32_t hb_set_resident_time(hb_ctx* ctx, const double* t_now) {
  HB_ENTER(!t_now);
  return stage_upload(ctx, ST_TNOW, ctx->w, ctx->w.t_now, t_now, ctx->s_wbc);  // no device synchronisation
}

int32_t hb_get_wbc_solution(hb_ctx* ctx, double* sol, int32_t* status) {
  HB_ENTER_ARGS(false);
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  HB_TRY(pull(ctx, sol, ctx->w, ctx->w.sol, whole(ctx)));
  HB_TRY(pull(ctx, status, ctx->w, ctx->w.status, whole(ctx)));
  return HB_OK;
}

int32_t hb_wbc_set_certificate(hb_ctx* ctx, int32_t enable) {
  HB_ENTER_ARGS(enable < 0 || enable > 1);
  HB_FAIL_IF(enable && ctx->config.wbc_type != 0, HB_ERR_ARG, "hb_wbc_set_certificate: the KKT certificate is defined for WeightedWbc only, not for HierarchicalWbc (wbc_type = 1)");
  if (bool(enable) == ctx->wbc_cert) return HB_OK;
  HB_ENTER_DEVICE();
  HB_TRY(hb_sync(ctx));
  if (enable) HB_TRY(ensure_fields(ctx, ctx->wcert));
  ctx->wbc_cert = enable != 0;
  ++ctx->graph_epoch;  // captured range graphs hold the other WBC kernel
  return HB_OK;
}

int32_t hb_wbc_get_certificate(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, double* cert, double* dual) {
  HB_ENTER_ARGS(!range_ok(ctx, inst_begin, inst_count, 0));
  if (!ctx->cert_last || ctx->config.wbc_type != 0) {  // (a HierarchicalWbc context keeps its certificates elsewhere: hb_hwbc_get_certificate)
    ctx->err = "hb_wbc_get_certificate: certificates were off at the last WBC call (hb_wbc_set_certificate)";
    return HB_ERR_STATE;
  }
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  if (inst_count == 0) return HB_OK;
  HB_TRY(pull(ctx, cert, ctx->wcert, ctx->wcert.cert, Range{inst_begin, inst_count}));
  HB_TRY(pull(ctx, dual, ctx->wcert, ctx->wcert.dual, Range{inst_begin, inst_count}));
  return HB_OK;
}

int32_t hb_hwbc_set_certificate(hb_ctx* ctx, int32_t enable) {
  HB_ENTER_ARGS(enable < 0 || enable > 1);
  HB_FAIL_IF(ctx->config.wbc_type != 1, HB_ERR_ARG, "hb_hwbc_set_certificate: the per-level certificate is defined for HierarchicalWbc (wbc_type = 1) only; WeightedWbc has hb_wbc_set_certificate");
  if (bool(enable) == ctx->wbc_cert) return HB_OK;
  HB_ENTER_DEVICE();
  HB_TRY(hb_sync(ctx));
  if (enable) HB_TRY(ensure_fields(ctx, ctx->hcert));
  ctx->wbc_cert = enable != 0;
  ++ctx->graph_epoch;  // captured range graphs hold the other WBC kernel
  return HB_OK;
}

int32_t hb_hwbc_get_certificate(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, double* cert, double* x_levels, double* slack0,
                                double* dual) {
  HB_ENTER_ARGS(!range_ok(ctx, inst_begin, inst_count, 0));
  HB_FAIL_IF(ctx->config.wbc_type != 1 || !ctx->cert_last, HB_ERR_STATE, "hb_hwbc_get_certificate: certificates were off at the last WBC call (hb_hwbc_set_certificate)");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  if (inst_count == 0) return HB_OK;
  HwbcCertBuf& c = ctx->hcert;
  const Range r{inst_begin, inst_count};
  HB_TRY(pull(ctx, cert, c, c.cert, r));
  HB_TRY(pull(ctx, x_levels, c, c.xlev, r));
  HB_TRY(pull(ctx, slack0, c, c.slack, r));
  HB_TRY(pull(ctx, dual, c, c.dual, r));
  return HB_OK;
}

int32_t hb_get_wbc_iterations(hb_ctx* ctx, int32_t* iters) {
  HB_ENTER(!iters);
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  HB_TRY(pull(ctx, iters, ctx->w, ctx->w.iters, whole(ctx)));
  return HB_OK;
}

}  // extern "C"
