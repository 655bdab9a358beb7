// Host side, part 7: the joint command and the per-instance controller flags (hb_joint_*; their arrays: joint_state_alloc, hb_api_plant.hpp),
// launch_estimator, the state estimator (hb_estimator_*) and the contact-force observer, on host sensor arrays or on the ones hb_plant_sense
// left on the device.
#pragma once

extern "C" {

int32_t hb_joint_set_flags(hb_ctx* ctx, const int32_t* controller_loaded, const int32_t* emergency_stop) {
  HB_ENTER(false);
  HB_TRY(joint_state_alloc(ctx));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  if (controller_loaded) HB_HIP(hipMemcpy(ctx->jc_loaded, controller_loaded, size_t(ctx->B) * sizeof(int), hipMemcpyHostToDevice));
  if (emergency_stop) HB_HIP(hipMemcpy(ctx->jc_estop, emergency_stop, size_t(ctx->B) * sizeof(int), hipMemcpyHostToDevice));
  return HB_OK;
}

int32_t hb_joint_get_emergency_stop(hb_ctx* ctx, int32_t* emergency_stop) {
  HB_ENTER(!emergency_stop);
  HB_TRY(joint_state_alloc(ctx));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  HB_HIP(hipMemcpy(emergency_stop, ctx->jc_estop, size_t(ctx->B) * sizeof(int), hipMemcpyDeviceToHost));
  return HB_OK;
}

int32_t hb_joint_command(hb_ctx* ctx, const hb_joint_gains* gains, double dt, double* pos_des, double* vel_des, double* kp, double* kd,
                         double* tau_ff, double* torque) {
  HB_ENTER_ARGS(!gains);
  HB_FAIL_IF(ctx->stats.n_wbc_solves == 0, HB_ERR_STATE, "hb_joint_command: no WBC solution yet");
  HB_ENTER_DEVICE();
  const size_t n = size_t(ctx->B) * HB_NJ;
  HB_TRY(joint_state_alloc(ctx));
  hipStream_t s = ctx->s_wbc;
  hipLaunchKernelGGL(k_joint_command, dim3((ctx->B + 63) / 64), dim3(64), 0, s, ctx->w, ctx->dmodel, *gains, dt, ctx->jc_estop, ctx->jc_loaded,
                     ctx->jc_out);
  HB_HIP(hipGetLastError());
  ctx->jc_computed = true;
  double* outs[6] = {pos_des, vel_des, kp, kd, tau_ff, torque};
  for (int a = 0; a < 6; ++a)
    if (outs[a]) HB_HIP(hipMemcpyAsync(outs[a], ctx->jc_out + a * n, n * 8, hipMemcpyDeviceToHost, s));
  HB_HIP(hipStreamSynchronize(s));
  return HB_OK;
}

// Filter step of the instances of e (instances [i0, i0 + e.B) of the context); in its ground or field form while a map is in force.
static void launch_estimator(const hb_ctx* ctx, const EstBatch& e, double dt, hipStream_t s, int i0 = 0) {
  const GroundForm gf = use_ground_forms(ctx->ground_on, ctx->gfield_on);
  if (gf == GroundForm::Field)
    hipLaunchKernelGGL(k_estimator_gfield, dim3(e.B), dim3(64), 0, s, e, view(ctx->gfield, ctx->Nmax, i0, e.B), ctx->dmodel, ctx->est_cfg, dt);
  else if (gf == GroundForm::Profile)
    hipLaunchKernelGGL(k_estimator_ground, dim3(e.B), dim3(64), 0, s, e, view(ctx->ground, ctx->Nmax, i0, e.B), ctx->dmodel, ctx->est_cfg, dt);
  else
    hipLaunchKernelGGL(k_estimator, dim3(e.B), dim3(64), 0, s, e, ctx->dmodel, ctx->est_cfg, dt);
}

int32_t hb_estimator_reset(hb_ctx* ctx, const hb_estimator_config* cfg, const double* x_hat0) {
  HB_ENTER(!cfg);
  EstBatch& e = ctx->est;
  HB_TRY(ensure_fields(ctx, e));
  ctx->est_cfg = *cfg;
  double* x0_dev = nullptr;
  if (x_hat0) {  // staged through the (not yet used) output buffer: 22 >= 18 doubles per instance
    x0_dev = e.x;
    HB_HIP(hipMemcpy(x0_dev, x_hat0, field_count(ctx, e, e.xhat) * 8, hipMemcpyHostToDevice));
  }
  HB_TRY(zero_field(ctx, e, e.cf_z, &ctx->s_wbc));   // pSCgZinvlast_ = 0 (StateEstimateBase.cpp:58-59)
  const int n = int(field_count(ctx, e, e.P));
  hipLaunchKernelGGL(k_estimator_reset, dim3((n + 255) / 256), dim3(256), 0, ctx->s_wbc, ctx->B, e.xhat, e.P, e.yaw_last, x0_dev);
  HB_HIP(hipGetLastError());
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  ctx->est_ready = true;
  return HB_OK;
}

// observer step of length dt on the device arrays rbd_dev and tau_dev, on s
static void launch_contact_force(const hb_ctx* ctx, double dt, const double* rbd_dev, const double* tau_dev, hipStream_t s) {
  const EstBatch& e = ctx->est;
  if (dt > 1.0) dt = 0.002;     // (StateEstimateBase.cpp:133-134)
  const double gama = std::exp(-ctx->est_cfg.contact_force_cutoff_frequency * dt), beta = (1.0 - gama) / (gama * dt);
  hipLaunchKernelGGL(k_contact_force, dim3((ctx->B + kCfThreads - 1) / kCfThreads), dim3(kCfThreads), 0, s, ctx->B, ctx->dmodel, gama, beta, rbd_dev,
                     tau_dev, e.cf_z, e.cf_dist, e.cf_out);
}

int32_t hb_estimator_contact_force(hb_ctx* ctx, double dt, const double* rbd, const double* joint_torque, double* est_disturbance_torque,
                                   double* est_contact_force) {
  HB_ENTER_ARGS(!joint_torque || !(dt > 0.0));
  HB_FAIL_IF(!ctx->est_ready, HB_ERR_STATE, "hb_estimator_contact_force: call hb_estimator_reset first (it carries the cut-off frequency and zeroes the observer state)");
  HB_ENTER_DEVICE();
  EstBatch& e = ctx->est;
  hipStream_t s = ctx->s_wbc;   // control-thread side, behind the estimator update it follows (LeggedController.cpp:327-345)
  HB_TRY(push(ctx, joint_torque, e, e.cf_tau, whole(ctx), &s));
  const double* rbd_dev = e.rbd;   // NULL: the rbd state the last hb_estimator_update left on the device
  if (rbd) {
    HB_TRY(push(ctx, rbd, e, e.cf_rbd, whole(ctx), &s));
    rbd_dev = e.cf_rbd;
  }
  launch_contact_force(ctx, dt, rbd_dev, e.cf_tau, s);
  HB_HIP(hipGetLastError());
  HB_TRY(pull(ctx, est_disturbance_torque, e, e.cf_dist, whole(ctx), &s));
  HB_TRY(pull(ctx, est_contact_force, e, e.cf_out, whole(ctx), &s));
  HB_HIP(hipStreamSynchronize(s));   // (the joint efforts were read from the caller's array)
  return HB_OK;
}

// filter step on the inputs e points to (device; ctx->est: its own upload buffers), outputs as in hb_estimator_update
static int32_t estimator_run(hb_ctx* ctx, EstBatch e, double dt, int32_t to_resident, double* rbd, double* x_state) {
  hipStream_t s = ctx->s_wbc;
  e.res_rbd = to_resident ? ctx->w.rbd : nullptr;
  e.res_x0 = to_resident ? ctx->b.x0 : nullptr;
  HB_TRY(resident_write(ctx, s, to_resident, [&] { launch_estimator(ctx, e, dt, s); }));
  HB_TRY(pull(ctx, rbd, e, e.rbd, whole(ctx), &s));
  HB_TRY(pull(ctx, x_state, e, e.x, whole(ctx), &s));
  if (rbd || x_state) HB_HIP(hipStreamSynchronize(s));  // without host outputs the call is enqueue-only
  return HB_OK;
}

int32_t hb_estimator_update(hb_ctx* ctx, double dt, const double* quat, const double* ang_vel_local, const double* lin_acc_local,
                            const double* joint_pos, const double* joint_vel, const int32_t* contact_flag, int32_t to_resident,
                            double* rbd, double* x_state) {
  HB_ENTER_ARGS(!quat || !ang_vel_local || !lin_acc_local || !joint_pos || !joint_vel || !contact_flag || !(dt > 0.0));
  HB_FAIL_IF(!ctx->est_ready, HB_ERR_STATE, "hb_estimator_update: call hb_estimator_reset first");
  HB_ENTER_DEVICE();
  EstBatch& e = ctx->est;
  const void* const src[6] = {quat, ang_vel_local, lin_acc_local, joint_pos, joint_vel, contact_flag};
  // (enqueue-only form: the sensor arrays go through pinned staging and are the caller's again on return)
  const double* const* const dst[5] = {&e.quat, &e.w_local, &e.a_local, &e.qj, &e.qdj};
  HB_TRY(upload_sensors(ctx, e, dst, e.contact, src, !(rbd || x_state), ctx->s_wbc));  // the estimator belongs to the control-thread side (LeggedController::update)
  return estimator_run(ctx, ctx->est, dt, to_resident, rbd, x_state);
}

// The two estimator calls on the sensor arrays hb_plant_sense left on the device.
static int32_t sensed_ready(hb_ctx* ctx, const char* who) {
  return refuse_state(ctx, who, !ctx->plant_ready ? "call hb_plant_reset first"
                                : !ctx->est_ready ? "call hb_estimator_reset first"
                                : !ctx->sensed    ? "no sensor reading on the device yet (hb_plant_sense after hb_plant_reset)"
                                                  : nullptr);
}

int32_t hb_estimator_update_resident(hb_ctx* ctx, double dt, int32_t to_resident, double* rbd, double* x_state) {
  HB_ENTER_ARGS(!(dt > 0.0));
  HB_TRY(sensed_ready(ctx, "hb_estimator_update_resident"));
  HB_ENTER_DEVICE();
  const PlantBatch& p = ctx->plant;
  EstBatch e = ctx->est;  // the same kernel with its input pointers aimed at the plant's sensor arrays: nothing is copied
  e.quat = p.s_quat; e.w_local = p.s_gyro; e.a_local = p.s_accel; e.qj = p.s_jp; e.qdj = p.s_jv; e.contact = p.s_contact;
  return estimator_run(ctx, e, dt, to_resident, rbd, x_state);
}

int32_t hb_estimator_contact_force_resident(hb_ctx* ctx, double dt, double* est_disturbance_torque, double* est_contact_force) {
  HB_ENTER_ARGS(!(dt > 0.0));
  HB_TRY(sensed_ready(ctx, "hb_estimator_contact_force_resident"));
  HB_ENTER_DEVICE();
  EstBatch& e = ctx->est;
  hipStream_t s = ctx->s_wbc;
  launch_contact_force(ctx, dt, e.rbd, ctx->plant.s_jt, s);
  HB_HIP(hipGetLastError());
  HB_TRY(pull(ctx, est_disturbance_torque, e, e.cf_dist, whole(ctx), &s));
  HB_TRY(pull(ctx, est_contact_force, e, e.cf_out, whole(ctx), &s));
  if (est_disturbance_torque || est_contact_force) HB_HIP(hipStreamSynchronize(s));  // without host outputs the call is enqueue-only
  return HB_OK;
}

int32_t hb_estimator_get_filter(hb_ctx* ctx, double* x_hat, double* P) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!ctx->est_ready, HB_ERR_STATE, "hb_estimator_get_filter: call hb_estimator_reset first");
  HB_ENTER_DEVICE();
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  HB_TRY(pull(ctx, x_hat, ctx->est, ctx->est.xhat, whole(ctx)));
  HB_TRY(pull(ctx, P, ctx->est, ctx->est.P, whole(ctx)));
  return HB_OK;
}

}  // extern "C"