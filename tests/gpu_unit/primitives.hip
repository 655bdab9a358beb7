// TEST HARNESS: one tiny kernel per device-only primitive of the product headers (hb_math.hpp, hb_tile.hpp, hb_qpfactor.hpp, ric_rcp of
// hb_riccati.hpp), so that tests/test_gpu_primitives_*.py can compare each of them with an exact reference on its own.  Built with
// the flags of csrc/hipcc_flags.sh into tests/gpu_unit/libhb_primitives.so; needs no hb_ctx and is not part of libhunter_hip.so.
// Every kernel runs 64-lane workgroups (one wavefront, blockIdx.x = case index) under the product's WaveCtx; every host entry
// allocates, copies, launches on the default stream, checks hipGetLastError and the synchronise status, copies back and returns an
// int32_t status (0 = ok, otherwise the hipError_t, or -1 for arguments the entry does not accept).  What a case does is written
// in prim_cases.hpp, shared with the host twin (tests/host_emu/hostemu.cpp: emu_prim_*, same arguments).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../hunter_bipedal_control_amd/csrc/hb_riccati.hpp"
#include "../../hunter_bipedal_control_amd/csrc/hb_qpfactor.hpp"
#include "../../hunter_bipedal_control_amd/csrc/hb_wavectx.hpp"
#include "prim_cases.hpp"

using namespace hb;
using namespace hbp;

namespace {

// ---------------------------------------------------------------------------------------------------------------- host plumbing
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  hipError_t err = hipSuccess;
  DevBuf(const void* src, size_t n) : bytes(n) {
    err = hipMalloc(&p, n ? n : 8);
    if (err == hipSuccess && src && n) err = hipMemcpy(p, src, n, hipMemcpyHostToDevice);
  }
  DevBuf(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t back(void* dst) const { return bytes ? hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
  template <class T> T* as() const { return static_cast<T*>(p); }
};
int32_t first_error(std::initializer_list<hipError_t> es) {
  for (hipError_t e : es)
    if (e != hipSuccess) return int32_t(e);
  return 0;
}
// after a launch: launch status, then the synchronise status
int32_t finish_launch() {
  const hipError_t e1 = hipGetLastError();
  const hipError_t e2 = hipDeviceSynchronize();
  return first_error({e1, e2});
}

// ---------------------------------------------------------------------------------------------------------------- scalar math
// point = blockIdx.x * 64 + lane
template <int OP>
__global__ __launch_bounds__(64) void k_math(const double* in, int n, double* out) {
  const int i = blockIdx.x * 64 + WaveCtx().lane;
  if (i < n) math_point<OP>(in, n, i, out);
}

// ---------------------------------------------------------------------------------------------------------------- lane primitives
// in / out: [ncases][words] doubles, idx: [ncases][64] ints; lane l of case c reads in[c * words + round * 64 + l]
enum LaneOp { L_WAVE_MAX = 0, L_WAVE_MAX_NONNEG, L_WAVE_SUM, L_QUAD_SUM, L_SEG8_ALLSUM, L_SEG8_ALLMAX, L_WAVE_BCAST, L_WAVE_GATHER,
              L_SEG8_GET, L_SEG8_SUFFIX3, L_SEG8_PREFIX3, L_SEG8_PREFIX_PRODUCT, L_WAVE_MAX_POS };
template <int OP>
__global__ __launch_bounds__(64) void k_lanes(const double* in_all, const int* idx_all, double* out_all, int words) {
#if defined(__HIP_DEVICE_COMPILE__)   // (the lane primitives only exist in the device pass)
  const WaveCtx cx;
  const int l = cx.lane;
  const double* in = in_all + size_t(blockIdx.x) * words;
  double* out = out_all + size_t(blockIdx.x) * words;
  const int ix = idx_all[blockIdx.x * 64 + l];
  if constexpr (OP == L_WAVE_MAX) out[l] = wave_max_f64(in[l]);
  if constexpr (OP == L_WAVE_MAX_NONNEG) out[l] = wave_max_nonneg_f64(in[l]);
  if constexpr (OP == L_WAVE_MAX_POS) out[l] = wave_max_pos_f64(in[l]);
  if constexpr (OP == L_WAVE_SUM) out[l] = wave_sum_f64(in[l]);
  if constexpr (OP == L_QUAD_SUM) out[l] = quad_sum_f64(in[l]);
  if constexpr (OP == L_SEG8_ALLSUM) out[l] = seg8_allsum(in[l]);
  if constexpr (OP == L_SEG8_ALLMAX) out[l] = seg8_allmax(in[l]);
  if constexpr (OP == L_WAVE_BCAST) out[l] = wave_bcast_f64(in[l], __builtin_amdgcn_readfirstlane(ix));   // src is wave-uniform
  if constexpr (OP == L_WAVE_GATHER) out[l] = wave_gather_f64(in[l], ix);
  if constexpr (OP == L_SEG8_GET) out[l] = seg8_get(in[l], ix);
  if constexpr (OP == L_SEG8_SUFFIX3 || OP == L_SEG8_PREFIX3) {
    // three calls on ONE carrier object, new data each time: [round][component][64]
    Seg8Carry sc;
#pragma unroll 1
    for (int r = 0; r < 3; ++r) {
      const double* p = in + r * 192;
      const Vec3<double> v(p[l], p[64 + l], p[128 + l]);
      const Vec3<double> o = OP == L_SEG8_SUFFIX3 ? seg8_suffix_sum(v, sc) : seg8_prefix_sum(v, sc);
      out[r * 192 + l] = o.x; out[r * 192 + 64 + l] = o.y; out[r * 192 + 128 + l] = o.z;
    }
  }
  if constexpr (OP == L_SEG8_PREFIX_PRODUCT) {
    Mat3<double> P;
#pragma unroll
    for (int e = 0; e < 9; ++e) P.m[e] = in[e * 64 + l];
    seg8_prefix_product(P);
#pragma unroll
    for (int e = 0; e < 9; ++e) out[e * 64 + l] = P.m[e];
  }
#endif
}

// ---------------------------------------------------------------------------------------------------------------- tile GEMMs
template <class S>
__global__ __launch_bounds__(64) void k_tile_mma(const double* img_all, const int* par_all, double sw, double* dst_all) {
  __shared__ double lds[TILE_LDS];
  const WaveCtx cx;
  const double* img = img_all + size_t(blockIdx.x) * TILE_LDS;
  for (int i = cx.lane; i < TILE_LDS; i += 64) lds[i] = img[i];
  cx.sync();
  tile_mma_case<S>(cx, lds, par_all + blockIdx.x * 8, sw, dst_all + size_t(blockIdx.x) * TILE_DST);
}
__global__ __launch_bounds__(64) void k_tile_roundtrip(const double* a_all, const double* b_all, const int* par_all, double scale, double* dst_all,
                                                        int* flag_all) {
  tile_roundtrip_case(WaveCtx(), a_all + size_t(blockIdx.x) * RT_WORDS, b_all + size_t(blockIdx.x) * RT_WORDS, par_all + blockIdx.x * 8, scale,
                      dst_all + size_t(blockIdx.x) * RT_WORDS, flag_all + blockIdx.x);
}

// ---------------------------------------------------------------------------------------------------------------- QP factorisation
// diag: [ncases][64], what householder_factor returns to each lane (regularised_factor drops it, so the wrapper calls
// householder_factor once more on the same columns, into a scratch factor).
template <int MA, bool kGrad, bool kHeadTail>
__global__ __launch_bounds__(64) void k_regularised_factor(const double* A_all, const double* b_all, const int* par_all, const double* dpar_all,
                                                            double* R_all, double* J_all, double* g_all, double* diag_all) {
  __shared__ double A[QF_A], R[QF_R], J[QF_R], R2[QF_R], b[32], g[16], np[64];
  const WaveCtx cx;
  const int* par = par_all + blockIdx.x * 8;
  const double* dp = dpar_all + blockIdx.x * 2;
  for (int i = cx.lane; i < QF_A; i += 64) A[i] = A_all[size_t(blockIdx.x) * QF_A + i];
  for (int i = cx.lane; i < QF_R; i += 64) { R[i] = R_all[size_t(blockIdx.x) * QF_R + i]; J[i] = J_all[size_t(blockIdx.x) * QF_R + i]; }
  if (cx.lane < 32) b[cx.lane] = b_all[blockIdx.x * 32 + cx.lane];
  if (cx.lane < 16) g[cx.lane] = g_all[blockIdx.x * 16 + cx.lane];
  cx.sync();
  regularised_factor_case<MA, kGrad, kHeadTail>(cx, par, dp, A, b, R, J, g, np);
#if defined(__HIP_DEVICE_COMPILE__)
  {
    const int n = par[0], mA = par[1], lda = par[2], ld = par[3], wstore = par[4], n_head = par[5];
    double acol[MA];
#pragma unroll
    for (int r = 0; r < MA; ++r) acol[r] = (cx.lane < n && r < mA) ? A[r * lda + cx.lane] : 0.0;
    double dg;
    if constexpr (kHeadTail) dg = householder_factor<MA>(acol, cx.lane, n, wstore, HeadTailDiag{dp[0], dp[1], n_head}, R2, ld);
    else dg = householder_factor<MA>(acol, cx.lane, n, wstore, UniformDiag(dp[0]), R2, ld);
    diag_all[blockIdx.x * 64 + cx.lane] = dg;
  }
#endif
  cx.sync();
  for (int i = cx.lane; i < QF_R; i += 64) { R_all[size_t(blockIdx.x) * QF_R + i] = R[i]; J_all[size_t(blockIdx.x) * QF_R + i] = J[i]; }
  if (cx.lane < 16) g_all[blockIdx.x * 16 + cx.lane] = g[cx.lane];
}
__global__ __launch_bounds__(64) void k_givens(int* par_all, double* R_all, double* J_all, double* np_all, int* act_all, int* isact_all,
                                               double* lam_all) {
  __shared__ double R[QF_R], J[QF_R], np[64], lam[64];
  __shared__ int act[64], is_active[64];
  const WaveCtx cx;
  for (int i = cx.lane; i < QF_R; i += 64) { R[i] = R_all[size_t(blockIdx.x) * QF_R + i]; J[i] = J_all[size_t(blockIdx.x) * QF_R + i]; }
  np[cx.lane] = np_all[blockIdx.x * 64 + cx.lane];
  lam[cx.lane] = lam_all[blockIdx.x * 64 + cx.lane];
  act[cx.lane] = act_all[blockIdx.x * 64 + cx.lane];
  is_active[cx.lane] = isact_all[blockIdx.x * 64 + cx.lane];
  cx.sync();
  givens_case(cx, par_all + blockIdx.x * 8, R, J, np, act, is_active, lam);
  cx.sync();
  for (int i = cx.lane; i < QF_R; i += 64) { R_all[size_t(blockIdx.x) * QF_R + i] = R[i]; J_all[size_t(blockIdx.x) * QF_R + i] = J[i]; }
  np_all[blockIdx.x * 64 + cx.lane] = np[cx.lane];
  lam_all[blockIdx.x * 64 + cx.lane] = lam[cx.lane];
  act_all[blockIdx.x * 64 + cx.lane] = act[cx.lane];
  isact_all[blockIdx.x * 64 + cx.lane] = is_active[cx.lane];
}

}  // namespace

extern "C" {

// y[4][n] <- op(x[4][n])
int32_t hbp_math(int32_t op, const double* x, int32_t n, double* y) {
  if (n <= 0) return -1;
  DevBuf in(x, size_t(4) * n * 8), out(nullptr, size_t(4) * n * 8);
  if (int32_t e = first_error({in.err, out.err})) return e;
  const dim3 grid((n + 63) / 64), block(64);
#define HBP_MATH_CASE(OP) case OP: hipLaunchKernelGGL(k_math<OP>, grid, block, 0, 0, in.as<double>(), n, out.as<double>()); break;
  switch (op) {
    HBP_MATH_OPS(HBP_MATH_CASE)
    default: return -1;
  }
#undef HBP_MATH_CASE
  if (int32_t e = finish_launch()) return e;
  return first_error({out.back(y)});
}

// out[ncases][words] <- op(in[ncases][words], idx[ncases][64])
int32_t hbp_lanes(int32_t op, int32_t ncases, int32_t words, const double* in, const int32_t* idx, double* out) {
  const int need = (op == L_SEG8_SUFFIX3 || op == L_SEG8_PREFIX3 || op == L_SEG8_PREFIX_PRODUCT) ? 576 : 64;
  if (ncases <= 0 || words != need) return -1;
  for (int i = 0; i < ncases * 64; ++i)   // lane indices the primitives take: inside the wavefront (the group for seg8_get)
    if (idx[i] < 0 || idx[i] > (op == L_SEG8_GET ? 7 : 63)) return -1;
  DevBuf din(in, size_t(ncases) * words * 8), didx(idx, size_t(ncases) * 64 * 4), dout(nullptr, size_t(ncases) * words * 8);
  if (int32_t e = first_error({din.err, didx.err, dout.err})) return e;
  const dim3 grid(ncases), block(64);
#define HBP_LANE_CASE(OP) case OP: hipLaunchKernelGGL(k_lanes<OP>, grid, block, 0, 0, din.as<double>(), didx.as<int>(), dout.as<double>(), words); break;
  switch (op) {
    HBP_LANE_CASE(L_WAVE_MAX) HBP_LANE_CASE(L_WAVE_MAX_NONNEG) HBP_LANE_CASE(L_WAVE_SUM) HBP_LANE_CASE(L_QUAD_SUM) HBP_LANE_CASE(L_SEG8_ALLSUM)
    HBP_LANE_CASE(L_SEG8_ALLMAX) HBP_LANE_CASE(L_WAVE_BCAST) HBP_LANE_CASE(L_WAVE_GATHER) HBP_LANE_CASE(L_SEG8_GET) HBP_LANE_CASE(L_SEG8_SUFFIX3)
    HBP_LANE_CASE(L_SEG8_PREFIX3) HBP_LANE_CASE(L_SEG8_PREFIX_PRODUCT) HBP_LANE_CASE(L_WAVE_MAX_POS)
    default: return -1;
  }
#undef HBP_LANE_CASE
  if (int32_t e = finish_launch()) return e;
  return first_error({dout.back(out)});
}

int32_t hbp_tile_desc(int32_t id, int32_t* d) { return tile_desc(id, d); }
int32_t hbp_sizes(int32_t* s) {
  const int32_t v[8] = {N_TILE_SPECS, TILE_LDS, TILE_DST, RT_LD, RT_LDD, RT_WORDS, QF_A, QF_R};
  std::memcpy(s, v, sizeof(v));
  return 0;
}
// dst[ncases][TILE_DST] (in / out) <- C0 + A B of instantiation `id` on img[ncases][TILE_LDS], par[ncases][8]
int32_t hbp_tile_mma(int32_t id, int32_t ncases, const double* img, const int32_t* par, double sw, double* dst) {
  if (ncases <= 0) return -1;
  for (int c = 0; c < ncases; ++c)
    if (!tile_par_ok(par + 8 * c)) return -1;
  DevBuf dimg(img, size_t(ncases) * TILE_LDS * 8), dpar(par, size_t(ncases) * 8 * 4), ddst(dst, size_t(ncases) * TILE_DST * 8);
  if (int32_t e = first_error({dimg.err, dpar.err, ddst.err})) return e;
  const dim3 grid(ncases), block(64);
#define HBP_TILE_CASE(ID, ...) \
  case ID: { typedef __VA_ARGS__ S; hipLaunchKernelGGL(k_tile_mma<S>, grid, block, 0, 0, dimg.as<double>(), dpar.as<int>(), sw, ddst.as<double>()); break; }
  switch (id) {
    HBP_TILE_SPECS(HBP_TILE_CASE)
    default: return -1;
  }
#undef HBP_TILE_CASE
  if (int32_t e = finish_launch()) return e;
  return first_error({ddst.back(dst)});
}
// a, b: [ncases][RT_WORDS]; dst: [ncases][RT_WORDS] in / out; flag: [ncases] out
int32_t hbp_tile_roundtrip(int32_t ncases, const double* a, const double* b, const int32_t* par, double scale, double* dst, int32_t* flag) {
  if (ncases <= 0) return -1;
  for (int c = 0; c < ncases; ++c)
    if (!roundtrip_par_ok(par + 8 * c)) return -1;
  std::vector<int32_t> zero(ncases, 0);
  DevBuf da(a, size_t(ncases) * RT_WORDS * 8), db(b, size_t(ncases) * RT_WORDS * 8), dpar(par, size_t(ncases) * 8 * 4),
      ddst(dst, size_t(ncases) * RT_WORDS * 8), dflag(zero.data(), size_t(ncases) * 4);
  if (int32_t e = first_error({da.err, db.err, dpar.err, ddst.err, dflag.err})) return e;
  hipLaunchKernelGGL(k_tile_roundtrip, dim3(ncases), dim3(64), 0, 0, da.as<double>(), db.as<double>(), dpar.as<int>(), scale, ddst.as<double>(),
                     dflag.as<int>());
  if (int32_t e = finish_launch()) return e;
  return first_error({ddst.back(dst), dflag.back(flag)});
}

// which: 0 = regularised_factor<18, false> with UniformDiag (hb_wbc.hpp), 1 = regularised_factor<24, true> with HeadTailDiag (hb_hoqp.hpp)
int32_t hbp_regularised_factor(int32_t which, int32_t ncases, const double* A, const double* b, const int32_t* par, const double* dpar, double* R,
                               double* J, double* g, double* diag) {
  if (ncases <= 0 || which < 0 || which > 1) return -1;
  for (int c = 0; c < ncases; ++c)
    if (!regfac_par_ok(par + 8 * c, which == 0 ? 18 : 24)) return -1;
  DevBuf dA(A, size_t(ncases) * QF_A * 8), db(b, size_t(ncases) * 32 * 8), dpar_(par, size_t(ncases) * 8 * 4), ddp(dpar, size_t(ncases) * 2 * 8),
      dR(R, size_t(ncases) * QF_R * 8), dJ(J, size_t(ncases) * QF_R * 8), dg(g, size_t(ncases) * 16 * 8), ddiag(nullptr, size_t(ncases) * 64 * 8);
  if (int32_t e = first_error({dA.err, db.err, dpar_.err, ddp.err, dR.err, dJ.err, dg.err, ddiag.err})) return e;
  const dim3 grid(ncases), block(64);
  if (which == 0)
    hipLaunchKernelGGL((k_regularised_factor<18, false, false>), grid, block, 0, 0, dA.as<double>(), db.as<double>(), dpar_.as<int>(), ddp.as<double>(),
                       dR.as<double>(), dJ.as<double>(), dg.as<double>(), ddiag.as<double>());
  else
    hipLaunchKernelGGL((k_regularised_factor<24, true, true>), grid, block, 0, 0, dA.as<double>(), db.as<double>(), dpar_.as<int>(), ddp.as<double>(),
                       dR.as<double>(), dJ.as<double>(), dg.as<double>(), ddiag.as<double>());
  if (int32_t e = finish_launch()) return e;
  return first_error({dR.back(R), dJ.back(J), dg.back(g), ddiag.back(diag)});
}
// everything in / out
int32_t hbp_givens(int32_t ncases, int32_t* par, double* R, double* J, double* np, int32_t* act, int32_t* is_active, double* lam) {
  if (ncases <= 0) return -1;
  for (int c = 0; c < ncases; ++c)
    if (!givens_par_ok(par + 8 * c, act + 64 * c)) return -1;
  DevBuf dpar(par, size_t(ncases) * 8 * 4), dR(R, size_t(ncases) * QF_R * 8), dJ(J, size_t(ncases) * QF_R * 8), dnp(np, size_t(ncases) * 64 * 8),
      dact(act, size_t(ncases) * 64 * 4), dis(is_active, size_t(ncases) * 64 * 4), dlam(lam, size_t(ncases) * 64 * 8);
  if (int32_t e = first_error({dpar.err, dR.err, dJ.err, dnp.err, dact.err, dis.err, dlam.err})) return e;
  hipLaunchKernelGGL(k_givens, dim3(ncases), dim3(64), 0, 0, dpar.as<int>(), dR.as<double>(), dJ.as<double>(), dnp.as<double>(), dact.as<int>(),
                     dis.as<int>(), dlam.as<double>());
  if (int32_t e = finish_launch()) return e;
  return first_error({dpar.back(par), dR.back(R), dJ.back(J), dnp.back(np), dact.back(act), dis.back(is_active), dlam.back(lam)});
}
}
