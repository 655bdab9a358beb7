// Host side, part 11: unit-level entry points (one kernel or one routine on caller-given data, device scratch per call).
#pragma once

extern "C" {

// ---- unit-level entry points ---------------------------------------------------------------------------
int32_t hb_eval_flow_map(hb_ctx* ctx, int32_t n, const double* x, const double* u, double* f, double* dfdx, double* dfdu) {
  HB_ENTER(n <= 0 || !x || !u || !f);
  const size_t m = n;
  DevBuf<double> dx_, du_, df_, dA, dB;
  HB_HIP(dx_.alloc(m * HB_NX, x));
  HB_HIP(du_.alloc(m * HB_NU, u));
  HB_HIP(df_.alloc(m * HB_NX));
  hipLaunchKernelGGL(k_flow_map, dim3((n + 63) / 64), dim3(64), 0, ctx->s_mpc, n, ctx->dmodel, dx_.p, du_.p, df_.p, (double*)nullptr, (double*)nullptr);
  if (dfdx || dfdu) {
    HB_HIP(dA.alloc(m * 484));
    HB_HIP(dB.alloc(m * 484));
    hipLaunchKernelGGL(k_flow_jac, dim3(n), dim3(64), 0, ctx->s_mpc, ctx->dmodel, dx_.p, du_.p, dA.p, dB.p);
  }
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  HB_HIP(hipMemcpy(f, df_.p, m * HB_NX * 8, hipMemcpyDeviceToHost));
  if (dfdx) HB_HIP(hipMemcpy(dfdx, dA.p, m * 484 * 8, hipMemcpyDeviceToHost));
  if (dfdu) HB_HIP(hipMemcpy(dfdu, dB.p, m * 484 * 8, hipMemcpyDeviceToHost));
  return HB_OK;
}

int32_t hb_eval_foot_kinematics(hb_ctx* ctx, int32_t n, const double* x, const double* u, double* pos, double* vel) {
  HB_ENTER(n <= 0 || !x || !u || !pos || !vel);
  const size_t m = n;
  DevBuf<double> dx_, du_, dp, dv;
  HB_HIP(dx_.alloc(m * HB_NX, x));
  HB_HIP(du_.alloc(m * HB_NU, u));
  HB_HIP(dp.alloc(m * 12));
  HB_HIP(dv.alloc(m * 12));
  hipLaunchKernelGGL(k_flow_map, dim3((n + 63) / 64), dim3(64), 0, ctx->s_mpc, n, ctx->dmodel, dx_.p, du_.p, (double*)nullptr, dp.p, dv.p);
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  HB_HIP(hipMemcpy(pos, dp.p, m * 12 * 8, hipMemcpyDeviceToHost));
  HB_HIP(hipMemcpy(vel, dv.p, m * 12 * 8, hipMemcpyDeviceToHost));
  return HB_OK;
}

int32_t hb_eval_rbd(hb_ctx* ctx, int32_t n, const double* rbd, double* Mo, double* nle, double* J, double* dJv) {
  HB_ENTER(n <= 0 || !rbd);
  const size_t m = n;
  DevBuf<double> dr, dM, dn, dJ, dd;
  HB_HIP(dr.alloc(m * HB_NRBD, rbd));
  HB_HIP(dM.alloc(m * 256));
  HB_HIP(dn.alloc(m * 16));
  HB_HIP(dJ.alloc(m * 192));
  HB_HIP(dd.alloc(m * 12));
  hipLaunchKernelGGL(k_rbd, dim3((n + 63) / 64), dim3(64), 0, ctx->s_wbc, n, ctx->dmodel, dr.p, dM.p, dn.p, dJ.p, dd.p);
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  if (Mo) HB_HIP(hipMemcpy(Mo, dM.p, m * 256 * 8, hipMemcpyDeviceToHost));
  if (nle) HB_HIP(hipMemcpy(nle, dn.p, m * 16 * 8, hipMemcpyDeviceToHost));
  if (J) HB_HIP(hipMemcpy(J, dJ.p, m * 192 * 8, hipMemcpyDeviceToHost));
  if (dJv) HB_HIP(hipMemcpy(dJv, dd.p, m * 12 * 8, hipMemcpyDeviceToHost));
  return HB_OK;
}

int32_t hb_ik_solve(hb_ctx* ctx, int32_t n, const double* q16, const int32_t* leg, const double* des_pos, const double* R_des, double* out5) {
  HB_ENTER(n <= 0 || !q16 || !leg || !des_pos || !R_des || !out5);
  const size_t m = n;
  DevBuf<double> dq, dd, dR, dout;
  DevBuf<int> dl;
  HB_HIP(dq.alloc(m * HB_NV, q16));
  HB_HIP(dd.alloc(m * 3, des_pos));
  HB_HIP(dR.alloc(m * 9, R_des));
  HB_HIP(dout.alloc(m * 5));
  HB_HIP(dl.alloc(m, leg));
  hipLaunchKernelGGL(k_ik_solve, dim3((n + 7) / 8), dim3(64), 0, ctx->s_mpc, n, ctx->dmodel, dq.p, dl.p, dd.p, dR.p, dout.p);
  HB_HIP(hipGetLastError());
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  HB_HIP(hipMemcpy(out5, dout.p, m * 5 * 8, hipMemcpyDeviceToHost));
  return HB_OK;
}

int32_t hb_ground_eval(hb_ctx* ctx, int32_t n, const int32_t* inst, const double* xy, double* height, int32_t* segment) {
  HB_ENTER_ARGS(n <= 0 || !inst || !xy || !(height || segment));
  HB_FAIL_IF(!ctx->ground_on && !ctx->gfield_on, HB_ERR_STATE, "hb_ground_eval: no ground map in force (hb_ground_set_profile)");
  for (int p = 0; p < n; ++p) HB_FAIL_IF(inst[p] < 0 || inst[p] >= ctx->B, HB_ERR_ARG, "hb_ground_eval: instance index outside the batch");
  HB_ENTER_DEVICE();
  const size_t m = n;
  DevBuf<double> dxy, dh;
  DevBuf<int> di, ds;
  HB_HIP(dxy.alloc(m * 2, xy));
  HB_HIP(di.alloc(m, inst));
  HB_HIP(dh.alloc(m));
  HB_HIP(ds.alloc(m));
  if (use_ground_forms(ctx->ground_on, ctx->gfield_on) == GroundForm::Field)   // (segment: the facet id)
    hipLaunchKernelGGL(k_ground_field_eval, dim3((n + 63) / 64), dim3(64), 0, ctx->s_mpc, n, ctx->gfield, di.p, dxy.p, dh.p, ds.p);
  else
    hipLaunchKernelGGL(k_ground_eval, dim3((n + 63) / 64), dim3(64), 0, ctx->s_mpc, n, ctx->ground, di.p, dxy.p, dh.p, ds.p);
  HB_HIP(hipGetLastError());
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  if (height) HB_HIP(hipMemcpy(height, dh.p, m * 8, hipMemcpyDeviceToHost));
  if (segment) HB_HIP(hipMemcpy(segment, ds.p, m * 4, hipMemcpyDeviceToHost));
  return HB_OK;
}

int32_t hb_hoqp_solve(hb_ctx* ctx, int32_t n_problems, int32_t n_vars, int32_t n_levels, const int32_t* m_eq, const int32_t* m_in,
                      const double* A, const double* b, const double* D, const double* f, double* x, double* slack, int32_t* status) {
  HB_ENTER_ARGS(n_problems <= 0 || n_vars <= 0 || n_vars > HQ_N || n_levels <= 0 || n_levels > HQ_L || !m_eq || !m_in || !A || !b || !D || !f ||
                !x || !slack || !status);
  for (int l = 0; l < n_levels; ++l)
    HB_FAIL_IF(m_eq[l] < 0 || m_eq[l] > HQ_M || m_in[l] < 0 || m_in[l] > HQ_M, HB_ERR_ARG, "hb_hoqp_solve: at most 8 equality-type and 8 inequality rows per level");
  HB_ENTER_DEVICE();
  const size_t P = size_t(n_problems), nm = P * HQ_L * HQ_M * HQ_N, nv = P * HQ_L * HQ_M, nx = P * HQ_L * HQ_N;
  DevBuf<double> dA, dD, db, df, dx, ds;
  DevBuf<int> dma, dmd, dst;
  HB_HIP(dA.alloc(nm, A));
  HB_HIP(dD.alloc(nm, D));
  HB_HIP(db.alloc(nv, b));
  HB_HIP(df.alloc(nv, f));
  HB_HIP(dx.alloc(nx));
  HB_HIP(ds.alloc(nv));
  HB_HIP(dma.alloc(HQ_L));
  HB_HIP(dmd.alloc(HQ_L));
  HB_HIP(dst.alloc(P));
  HB_HIP(hipMemcpy(dma.p, m_eq, size_t(n_levels) * sizeof(int), hipMemcpyHostToDevice));
  HB_HIP(hipMemcpy(dmd.p, m_in, size_t(n_levels) * sizeof(int), hipMemcpyHostToDevice));
  HB_HIP(hipMemset(dx.p, 0, nx * 8));
  HB_HIP(hipMemset(ds.p, 0, nv * 8));
  hipLaunchKernelGGL(k_hoqp_generic, dim3(n_problems), dim3(64), 0, ctx->s_wbc, n_vars, n_levels, dma.p, dmd.p, dA.p, db.p, dD.p, df.p,
                     ctx->hconfig.wbc_eps, 4 * ctx->hconfig.wbc_max_iter, dx.p, ds.p, dst.p, ctx->hconfig.wbc_reg_steps);
  HB_HIP(hipGetLastError());
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  HB_HIP(hipMemcpy(x, dx.p, nx * 8, hipMemcpyDeviceToHost));
  HB_HIP(hipMemcpy(slack, ds.p, nv * 8, hipMemcpyDeviceToHost));
  HB_HIP(hipMemcpy(status, dst.p, P * sizeof(int), hipMemcpyDeviceToHost));
  return HB_OK;
}

int32_t hb_centroidal_state_from_rbd(hb_ctx* ctx, int32_t n, const double* rbd, double* x) {
  HB_ENTER(!rbd || !x || n <= 0);
  DevBuf<double> drbd, dx;
  HB_HIP(drbd.alloc(size_t(n) * HB_NRBD, rbd));
  HB_HIP(dx.alloc(size_t(n) * HB_NX));
  hipLaunchKernelGGL(k_centroidal_state, dim3((n + 63) / 64), dim3(64), 0, ctx->s_wbc, n, ctx->dmodel, drbd.p, dx.p);
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  HB_HIP(hipMemcpy(x, dx.p, size_t(n) * HB_NX * 8, hipMemcpyDeviceToHost));
  return HB_OK;
}

int32_t hb_riccati_solve(hb_ctx* ctx, int32_t n, int32_t N, int32_t nu, const double* A, const double* Bm, const double* bv,
                         const double* Q, const double* R, const double* P, const double* q, const double* r,
                         const double* dx0, double* dx, double* du) {
  HB_ENTER_ARGS(n <= 0 || N <= 0 || nu <= 0 || nu > NU_T || n > ctx->B || N > ctx->Nmax);
  // pack stage data into node records on the host, run the same kernels the MPC uses
  const size_t Nm = ctx->Nmax;
  const size_t rec_inst = extent_of(ctx->b, Nm, ctx->b.recs).n, gain_inst = extent_of(ctx->b, Nm, ctx->b.gains).n;   // doubles per instance
  std::vector<double> recs(size_t(n) * rec_inst, 0.0);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < N; ++k) {
      const size_t sk = size_t(i) * N + k;
      rec_pack(recs.data() + size_t(i) * rec_inst + size_t(k) * REC_SIZE, nu, 0, nu, A + sk * 484, Bm + sk * 22 * nu, bv + sk * 22, Q + sk * 484,
               R + sk * nu * nu, P + sk * nu * 22, q + sk * 22, r + sk * nu);
    }
  // The forward kernel reconstructs du through the projection data; for this unit entry point the reduced input
  // is returned directly, so run backward on the device and the (cheap) forward recursion on the host.
  HB_ENTER_DEVICE();
  std::vector<int> nn(ctx->B, 1);
  for (int i = 0; i < n; ++i) nn[i] = N;
  HB_TRY(push(ctx, nn.data(), ctx->b, ctx->b.n_nodes, whole(ctx)));
  HB_TRY(push(ctx, recs.data(), ctx->b, ctx->b.recs, Range{0, n}));
  launch_ric_bwd(ctx, ctx->b, n, n, ctx->s_mpc);
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  std::vector<double> gains(size_t(n) * gain_inst);
  HB_TRY(pull(ctx, gains.data(), ctx->b, ctx->b.gains, Range{0, n}));
  ctx->refs_set = false;  // the batch buffers were clobbered
  for (int i = 0; i < n; ++i) {
    double xk[22];
    std::memcpy(xk, dx0 + size_t(i) * 22, 22 * 8);
    for (int k = 0; k < N; ++k) {
      const double* g = gains.data() + size_t(i) * gain_inst + size_t(k) * GAIN_SIZE;
      const size_t sk = size_t(i) * N + k;
      std::memcpy(dx + (size_t(i) * (N + 1) + k) * 22, xk, 22 * 8);
      double ut[NU_T];
      for (int a = 0; a < nu; ++a) {
        double s = g[264 + a];
        for (int c = 0; c < 22; ++c) s += g[a * 22 + c] * xk[c];
        ut[a] = s;
        du[sk * nu + a] = s;
      }
      double xn[22];
      for (int row = 0; row < 22; ++row) {
        double s = bv[sk * 22 + row];
        for (int c = 0; c < 22; ++c) s += A[(sk * 22 + row) * 22 + c] * xk[c];
        for (int a = 0; a < nu; ++a) s += Bm[(sk * 22 + row) * nu + a] * ut[a];
        xn[row] = s;
      }
      std::memcpy(xk, xn, 22 * 8);
    }
    std::memcpy(dx + (size_t(i) * (N + 1) + N) * 22, xk, 22 * 8);
  }
  return HB_OK;
}

int32_t hb_riccati_gains(hb_ctx* ctx, int32_t n, const int32_t* N, const int32_t* n_f, const int32_t* n_z, const double* A, const double* Bm,
                         const double* bv, const double* Q, const double* R, const double* P, const double* q, const double* r,
                         double* K, double* kv, int32_t* ric_fail) {
  HB_ENTER_ARGS(n <= 0 || n > ctx->B || !N || !n_f || !n_z || !A || !Bm || !bv || !Q || !R || !P || !q || !r || !K || !kv || !ric_fail);
  const size_t Nm = ctx->Nmax;
  for (int i = 0; i < n; ++i) {
    HB_FAIL_IF(N[i] < 1 || N[i] > ctx->Nmax, HB_ERR_ARG, "hb_riccati_gains: 1 <= N[i] <= max_nodes");
    for (int k = 0; k < N[i]; ++k) {
      const int f = n_f[i * Nm + k], z = n_z[i * Nm + k];
      HB_FAIL_IF(f < 0 || z < 0 || (f + z != 6 && f + z != 9 && f + z != 12), HB_ERR_ARG, "hb_riccati_gains: n_f + n_z of a stage must be 6, 9 or 12");
    }
  }
  // Records of the real stages exactly as hb_riccati_solve packs them; whatever the sweep has no business reading — the stages behind
  // an instance's horizon, the instances behind the call's — is a quiet NaN, and the gains start as HB_RIC_GAINS_SENTINEL_BITS everywhere.
  const size_t rec_inst = extent_of(ctx->b, Nm, ctx->b.recs).n, gain_inst = extent_of(ctx->b, Nm, ctx->b.gains).n;   // doubles per instance
  std::vector<double> recs(size_t(ctx->B) * rec_inst, __builtin_nan(""));
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < N[i]; ++k) {
      const size_t sk = size_t(i) * Nm + k;
      rec_pack(recs.data() + size_t(i) * rec_inst + size_t(k) * REC_SIZE, n_f[sk], n_z[sk], NU_T, A + sk * 484, Bm + sk * 22 * NU_T, bv + sk * 22,
               Q + sk * 484, R + sk * NU_T * NU_T, P + sk * NU_T * 22, q + sk * 22, r + sk * NU_T);
    }
  const uint64_t sentinel_bits = HB_RIC_GAINS_SENTINEL_BITS;
  double sentinel;
  std::memcpy(&sentinel, &sentinel_bits, 8);
  std::vector<double> gains(size_t(ctx->B) * gain_inst, sentinel);
  HB_ENTER_DEVICE();
  std::vector<int> nn(ctx->B, 1), fail(ctx->B, -1);
  for (int i = 0; i < n; ++i) nn[i] = N[i];
  HB_TRY(push(ctx, nn.data(), ctx->b, ctx->b.n_nodes, whole(ctx)));
  HB_TRY(push(ctx, recs.data(), ctx->b, ctx->b.recs, whole(ctx)));
  HB_TRY(push(ctx, gains.data(), ctx->b, ctx->b.gains, whole(ctx)));
  HB_TRY(push(ctx, fail.data(), ctx->b, ctx->b.ric_fail, whole(ctx)));
  launch_ric_bwd(ctx, ctx->b, n, n, ctx->s_mpc);
  HB_HIP(hipGetLastError());
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  HB_TRY(pull(ctx, gains.data(), ctx->b, ctx->b.gains, Range{0, n}));
  HB_TRY(pull(ctx, ric_fail, ctx->b, ctx->b.ric_fail, Range{0, n}));
  ctx->refs_set = false;  // the batch buffers were clobbered
  for (int i = 0; i < n; ++i)
    for (size_t k = 0; k < Nm; ++k) {
      const double* g = gains.data() + size_t(i) * gain_inst + k * GAIN_SIZE;
      std::memcpy(K + (size_t(i) * Nm + k) * NU_T * 22, g, NU_T * 22 * 8);
      std::memcpy(kv + (size_t(i) * Nm + k) * NU_T, g + NU_T * 22, NU_T * 8);
    }
  return HB_OK;
}

}  // extern "C"
