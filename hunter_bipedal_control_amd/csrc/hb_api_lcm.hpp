// Host side, part 8: the LCM wire format (include/hunter_lcm.h) and the entry points that speak it: the controller end and the simulator end.
#pragma once

extern "C" {

// ---- LCM wire format (include/hunter_lcm.h) -----------------------------------------------------------------------
uint64_t hb_lcm_fingerprint(int32_t type) { return (type < 0 || type > 2) ? 0 : lcm_fingerprint(type); }
int32_t hb_lcm_field_count(int32_t type) { return (type < 0 || type > 2) ? HB_ERR_ARG : lcm_type(type).n_fields; }
int32_t hb_lcm_encoded_size(int32_t type) { return (type < 0 || type > 2) ? HB_ERR_ARG : 16 + 8 * lcm_type(type).n_fields; }

int32_t hb_lcm_encode(int32_t type, int32_t n, const int64_t* timestamp, const double* fields, uint8_t* out) {
  if (type < 0 || type > 2 || n < 0 || !timestamp || !fields || !out) return HB_ERR_ARG;
  const int nf = lcm_type(type).n_fields, sz = 16 + 8 * nf;
  const uint64_t fp = lcm_fingerprint(type);
  for (int i = 0; i < n; ++i) {
    uint8_t* p = out + size_t(i) * sz;
    lcm_put64(p, fp);
    lcm_put64(p + 8, uint64_t(timestamp[i]));
    for (int k = 0; k < nf; ++k) {
      uint64_t bits;
      std::memcpy(&bits, fields + size_t(i) * nf + k, 8);
      lcm_put64(p + 16 + 8 * k, bits);
    }
  }
  return HB_OK;
}

int32_t hb_lcm_decode(int32_t type, int32_t n, const uint8_t* in, int64_t* timestamp, double* fields) {
  if (type < 0 || type > 2 || n < 0 || !in || !timestamp || !fields) return HB_ERR_ARG;
  const int nf = lcm_type(type).n_fields, sz = 16 + 8 * nf;
  const uint64_t fp = lcm_fingerprint(type);
  for (int i = 0; i < n; ++i)
    if (lcm_get64(in + size_t(i) * sz) != fp) return HB_ERR_ARG;
  for (int i = 0; i < n; ++i) {
    const uint8_t* p = in + size_t(i) * sz;
    timestamp[i] = int64_t(lcm_get64(p + 8));
    for (int k = 0; k < nf; ++k) {
      const uint64_t bits = lcm_get64(p + 16 + 8 * k);
      std::memcpy(fields + size_t(i) * nf + k, &bits, 8);
    }
  }
  return HB_OK;
}

int32_t hb_lcm_frame(const char* channel, uint32_t seq, const uint8_t* payload, int32_t payload_len, uint8_t* out, int32_t maxlen) {
  if (!channel || !payload || !out || payload_len < 0) return HB_ERR_ARG;
  const size_t cl = std::strlen(channel) + 1;
  const size_t total = 8 + cl + size_t(payload_len);
  if (cl > 64 || total > size_t(maxlen) || total > 65499) return HB_ERR_ARG;  // LCM_MAX_CHANNEL_NAME_LENGTH 63, short-message limit
  const uint32_t magic = 0x4c433032u;
  for (int b = 0; b < 4; ++b) { out[b] = uint8_t(magic >> (24 - 8 * b)); out[4 + b] = uint8_t(seq >> (24 - 8 * b)); }
  std::memcpy(out + 8, channel, cl);
  std::memcpy(out + 8 + cl, payload, size_t(payload_len));
  return int32_t(total);
}

int32_t hb_lcm_unframe(const uint8_t* frame, int32_t frame_len, char* channel, int32_t channel_cap, uint32_t* seq, int32_t* payload_offset) {
  if (!frame || frame_len < 10 || !channel || channel_cap < 2 || !payload_offset) return HB_ERR_ARG;
  uint32_t magic = 0, sq = 0;
  for (int b = 0; b < 4; ++b) { magic = (magic << 8) | frame[b]; sq = (sq << 8) | frame[4 + b]; }
  if (magic != 0x4c433032u) return HB_ERR_ARG;   // not a short LCM message ("LC03" fragments are not produced by this path)
  int32_t i = 8;
  while (i < frame_len && frame[i] != 0) ++i;
  if (i >= frame_len || i - 8 >= channel_cap || i - 8 > 63) return HB_ERR_ARG;
  std::memcpy(channel, frame + 8, size_t(i - 8) + 1);
  if (seq) *seq = sq;
  *payload_offset = i + 1;
  return frame_len - (i + 1);
}

int32_t hb_joint_command_lcm(hb_ctx* ctx, const hb_joint_gains* gains, double dt, int64_t timestamp_ns, uint8_t* low_cmd) {
  HB_ENTER_ARGS(!gains || !low_cmd);
  HB_TRY(hb_joint_command(ctx, gains, dt, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  const size_t B = ctx->B, words = B * 62;
  if (!ctx->lcm_cmd) HB_HIP(dalloc(ctx, &ctx->lcm_cmd, words));
  hipStream_t s = ctx->s_wbc;
  hipLaunchKernelGGL(k_lcm_pack_cmd, dim3((unsigned(words) + 255) / 256), dim3(256), 0, s, ctx->B, ctx->jc_out,
                     lcm_fingerprint(HB_LCM_LOW_CMD), timestamp_ns, ctx->lcm_cmd);
  HB_HIP(hipGetLastError());
  HB_HIP(hipMemcpyAsync(low_cmd, ctx->lcm_cmd, words * 8, hipMemcpyDeviceToHost, s));
  HB_HIP(hipStreamSynchronize(s));
  return HB_OK;
}

int32_t hb_estimator_update_lcm(hb_ctx* ctx, double dt, const uint8_t* low_state, const int32_t* contact_flag, int32_t to_resident,
                                double* rbd, double* x_state, int64_t* timestamp) {
  HB_ENTER_ARGS(!low_state || !contact_flag || !(dt > 0.0));
  HB_FAIL_IF(!ctx->est_ready, HB_ERR_STATE, "hb_estimator_update_lcm: call hb_estimator_reset first");
  HB_ENTER_DEVICE();
  const size_t B = ctx->B, words = B * 42;
  if (!ctx->lcm_state) {
    HB_HIP(dalloc(ctx, &ctx->lcm_state, words));
    HB_HIP(dalloc(ctx, &ctx->lcm_ts, B));
    HB_HIP(dalloc(ctx, &ctx->lcm_bad, size_t(1)));
  }
  EstBatch e = ctx->est;
  hipStream_t s = ctx->s_wbc;
  HB_HIP(hipMemcpyAsync(ctx->lcm_state, low_state, words * 8, hipMemcpyHostToDevice, s));
  HB_HIP(hipMemsetAsync(ctx->lcm_bad, 0, sizeof(int), s));
  HB_TRY(push(ctx, contact_flag, e, e.contact, whole(ctx), &s));
  hipLaunchKernelGGL(k_lcm_unpack_state, dim3((unsigned(words) + 255) / 256), dim3(256), 0, s, ctx->B, ctx->lcm_state,
                     lcm_fingerprint(HB_LCM_LOW_STATE), const_cast<double*>(e.quat), const_cast<double*>(e.w_local),
                     const_cast<double*>(e.a_local), const_cast<double*>(e.qj), const_cast<double*>(e.qdj), ctx->lcm_ts, ctx->lcm_bad);
  HB_HIP(hipGetLastError());
  int bad = 0;
  HB_HIP(hipMemcpyAsync(&bad, ctx->lcm_bad, sizeof(int), hipMemcpyDeviceToHost, s));
  HB_HIP(hipStreamSynchronize(s));
  HB_FAIL_IF(bad, HB_ERR_ARG, "hb_estimator_update_lcm: a message does not carry the low_state_t fingerprint");
  if (timestamp) HB_HIP(hipMemcpy(timestamp, ctx->lcm_ts, B * 8, hipMemcpyDeviceToHost));
  return estimator_run(ctx, ctx->est, dt, to_resident, rbd, x_state);
}

// ---- the simulator end of the link ---------------------------------------------------------------------------------------------------
int32_t hb_plant_step_lcm(hb_ctx* ctx, const uint8_t* low_cmd, const int32_t* contact, double dt, int32_t substeps, int32_t to_resident,
                          int32_t* accepted) {
  HB_ENTER_ARGS(!low_cmd || !(dt > 0.0) || substeps < 1);
  HB_TRY(plant_step_ready(ctx, "hb_plant_step_lcm", false, !contact));
  // the fingerprints are looked at here, where the bytes still are: nothing has changed when one is foreign
  const uint64_t fp = lcm_fingerprint(HB_LCM_LOW_CMD);
  for (int i = 0; i < ctx->B; ++i)
    HB_FAIL_IF(lcm_get64(low_cmd + size_t(i) * HB_LCM_LOW_CMD_BYTES) != fp, HB_ERR_ARG, "hb_plant_step_lcm: a message does not carry the low_cmd_t fingerprint");
  HB_ENTER_DEVICE();
  HB_TRY(ensure_fields(ctx, ctx->act));
  ActuatorBatch& a = ctx->act;
  hipStream_t s = ctx->s_wbc;
  HB_HIP(hipMemcpyAsync(a.wire_cmd, low_cmd, field_count(ctx, a, a.wire_cmd) * 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_lcm_unpack_cmd, dim3((ctx->B + 63) / 64), dim3(64), 0, s, ctx->B, a.wire_cmd, a.rcmd[0], a.rcmd[1], a.rcmd[2], a.rcmd[3], a.rcmd[4],
                     a.last_ts, a.accepted);
  HB_HIP(hipGetLastError());
  HB_TRY(pull(ctx, accepted, a, a.accepted, whole(ctx), &s));
  HB_TRY(plant_launch(ctx, nullptr, a.rcmd, contact, dt, substeps, to_resident));
  if (accepted) HB_HIP(hipStreamSynchronize(s));
  return HB_OK;
}

int32_t hb_plant_sense_lcm(hb_ctx* ctx, int64_t timestamp_ns, uint8_t* low_state, uint8_t* full_state) {
  HB_ENTER_ARGS(false);
  HB_FAIL_IF(!low_state && !full_state, HB_ERR_ARG, "hb_plant_sense_lcm: give low_state, full_state or both");
  HB_FAIL_IF(!ctx->plant_ready, HB_ERR_STATE, "hb_plant_sense_lcm: call hb_plant_reset first");
  HB_ENTER_DEVICE();
  HB_TRY(ensure_fields(ctx, ctx->act));
  HB_TRY(hb_plant_sense(ctx, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));   // (enqueue-only: the arrays stay on the device)
  ActuatorBatch& a = ctx->act;
  const PlantBatch& p = ctx->plant;
  hipStream_t s = ctx->s_wbc;
  const unsigned B = unsigned(ctx->B);
  if (low_state) {
    hipLaunchKernelGGL(k_lcm_pack_state, dim3((B * 42 + 255) / 256), dim3(256), 0, s, ctx->B, p.s_quat, p.s_gyro, p.s_accel, p.s_jp, p.s_jv, p.s_jt,
                       lcm_fingerprint(HB_LCM_LOW_STATE), timestamp_ns, a.wire_low);
    HB_HIP(hipGetLastError());
    HB_TRY(pull(ctx, low_state, a, a.wire_low, whole(ctx), &s));
  }
  if (full_state) {
    hipLaunchKernelGGL(k_lcm_pack_full, dim3((B + 63) / 64), dim3(64), 0, s, ctx->B, ctx->hmodel.gravity, p.q, p.v, p.tau_last,
                       lcm_fingerprint(HB_LCM_FULL_STATE), timestamp_ns, a.wire_full);
    HB_HIP(hipGetLastError());
    HB_TRY(pull(ctx, full_state, a, a.wire_full, whole(ctx), &s));
  }
  HB_HIP(hipStreamSynchronize(s));
  return HB_OK;
}

}  // extern "C"
