// TEST HARNESS: what one case of each primitive wrapper does, written once for both builds of the product headers — the device
// kernels of primitives.hip (WaveCtx, operands in LDS) and the host twin of tests/host_emu/hostemu.cpp (one emulated lane, operands
// on the heap).  The caller includes hb_riccati.hpp and hb_qpfactor.hpp first.  The lane primitives have no host form and live in
// primitives.hip alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace hbp {
using namespace hb;

// ---------------------------------------------------------------------------------------------------------------- scalar math
// in: [4][n] (as many rows as the operation has operands), out: [4][n]
enum MathOp { M_RCP = 0, M_RIC_RCP, M_SINCOS_REDUCED, M_SINCOS_T, M_SINCOS_BOUNDED, M_LOG_FD, M_RSQRT, M_SQRT,
              M_D_SINCOS = 10, M_D_DIV, M_D_RCP, M_D_SQRT };
template <int OP>
HB_HD void math_point(const double* in, int n, int i, double* out) {
  const double a0 = in[i], a1 = in[n + i], a2 = in[2 * n + i], a3 = in[3 * n + i];
  double o0 = 0.0, o1 = 0.0, o2 = 0.0, o3 = 0.0;
  if constexpr (OP == M_RCP) o0 = rcp_t(a0);
  if constexpr (OP == M_RIC_RCP) o0 = ric_rcp(a0);
  if constexpr (OP == M_SINCOS_REDUCED) sincos_reduced(a0, o0, o1);
  if constexpr (OP == M_SINCOS_T) sincos_t(a0, o0, o1);
  if constexpr (OP == M_SINCOS_BOUNDED) sincos_bounded(a0, o0, o1);
  if constexpr (OP == M_LOG_FD) o0 = log_fd(a0);
  if constexpr (OP == M_RSQRT) o0 = rsqrt_t(a0);
  if constexpr (OP == M_SQRT) o0 = sqrt_t(a0);
  if constexpr (OP == M_D_SINCOS) {
    Dual1 s, c;
    sincos_t(Dual1(a0, a1), s, c);
    o0 = s.v; o1 = s.d; o2 = c.v; o3 = c.d;
  }
  if constexpr (OP == M_D_DIV) {
    const Dual1 q = Dual1(a0, a1) / Dual1(a2, a3);
    o0 = q.v; o1 = q.d;
  }
  if constexpr (OP == M_D_RCP) {
    const Dual1 q = rcp_t(Dual1(a0, a1));
    o0 = q.v; o1 = q.d;
  }
  if constexpr (OP == M_D_SQRT) {
    const Dual1 q = sqrt_t(Dual1(a0, a1));
    o0 = q.v; o1 = q.d;
  }
  out[i] = o0; out[n + i] = o1; out[2 * n + i] = o2; out[3 * n + i] = o3;
}
#define HBP_MATH_OPS(X) \
  X(M_RCP) X(M_RIC_RCP) X(M_SINCOS_REDUCED) X(M_SINCOS_T) X(M_SINCOS_BOUNDED) X(M_LOG_FD) X(M_RSQRT) X(M_SQRT) X(M_D_SINCOS) X(M_D_DIV) \
  X(M_D_RCP) X(M_D_SQRT)

// ---------------------------------------------------------------------------------------------------------------- tile GEMMs
// One case: an image of TILE_LDS doubles (the test lays the operands out in it; LDS on the device), the start values C0 as a dense
// [16 MT][16 NT] block of it (through tile_init), the product, and tile_store_rm<16 NT + 3> into a destination the test has
// pre-filled with a sentinel.  par: 8 ints {offA, offB, offC, Mr, Nr, cfm, tnb0, -}; sw: soft weight.
constexpr int TILE_LDS = 4096, TILE_DST = 4096;
enum WeightKind { W_NONE = 0, W_EQ = 1, W_SOFT = 2 };
template <int K_, int LDA_, bool TA_, int LDB_, bool TB_, int KR_, bool PRE_, int MT_, int NT_, int WK_, int MTB_ = 0, int NTB_ = 0>
struct TileSpec {
  static constexpr int K = K_, LDA = LDA_, LDB = LDB_, KR = KR_, MT = MT_, NT = NT_, WK = WK_, MTB = MTB_, NTB = NTB_;
  static constexpr bool TA = TA_, TB = TB_, PRE = PRE_;
};
template <class S, class Ctx>
HB_HD void tile_mma_case(const Ctx& cx, const double* lds, const int* par, double sw, double* dst) {
  const double* A = lds + par[0];
  const double* B = lds + par[1];
  const double* C0 = lds + par[2];
  int Mr = par[3], Nr = par[4];
  const int cfm = par[5], tnb0 = par[6];
#if !defined(__HIP_DEVICE_COMPILE__)
  // k_ric_bwd4 hands a one-tile product the width of everything to its right (Nr up to 36 on 16 columns): the device forms select on
  // row < Mr && col < Nr, the host loops run to Mr x Nr and would leave the tile
  Mr = Mr < 16 * S::MT ? Mr : 16 * S::MT;
  Nr = Nr < 16 * S::NT ? Nr : 16 * S::NT;
#endif
  WaveTile<S::MT, S::NT> t;
  tile_init(cx, t, Mr, Nr, [C0](int r, int c) { return C0[r * (16 * S::NT) + c]; });
  if constexpr (S::MTB > 0) {
    // the right operand out of the accumulators of an earlier tile: Bt(k, j) = B[k * 16 NTB + j], every element of it live
    WaveTile<S::MTB, S::NTB> bt;
    tile_init(cx, bt, 16 * S::MTB, 16 * S::NTB, [B](int r, int c) { return B[r * (16 * S::NTB) + c]; });
    tile_mma_bacc<S::K, S::LDA, S::TA>(cx, t, A, bt, tnb0, Mr, Nr);
  } else if constexpr (S::WK == W_EQ) {
    tile_mma<S::K, S::LDA, S::TA, S::LDB, S::TB, S::KR, S::PRE>(cx, t, A, B, Mr, Nr, [cfm](int slot) { return slot_is_eq(slot, cfm) ? 1.0 : 0.0; },
                                                                EqStepLive{cfm});
  } else if constexpr (S::WK == W_SOFT) {
    tile_mma<S::K, S::LDA, S::TA, S::LDB, S::TB, S::KR, S::PRE>(cx, t, A, B, Mr, Nr, [cfm, sw](int slot) { return slot_is_soft(slot, cfm) ? sw : 0.0; },
                                                                SoftStepLive{cfm});
  } else {
    tile_mma<S::K, S::LDA, S::TA, S::LDB, S::TB, S::KR, S::PRE>(cx, t, A, B, Mr, Nr);
  }
  tile_store_rm<16 * S::NT + 3>(cx, t, Mr, Nr, dst);
}
// The template argument lists of the product's call sites (id -> site), LDK = LqLds::LDK, LDN / LDW of RicLds:
constexpr int LDK = LqLds::LDK, LDN = RicLds::LDN, LDW = RicLds::LDW;
#define HBP_TILE_SPECS(X)                                                                                       \
  X(0, TileSpec<24, LDN, true, LDW, false, 24, false, 2, 2, W_NONE>)           /* hb_riccati.hpp ric_phase1, NTW 2 */ \
  X(1, TileSpec<24, LDN, true, LDW, false, 24, false, 2, 3, W_NONE>)           /* hb_riccati.hpp ric_phase1, NTW 3 */ \
  X(2, TileSpec<24, LDW, true, 0, false, 24, false, 1, 2, W_NONE, 2, 2>)       /* ric_phase2_gemm (bacc), NTW 2; ric_phase3_mma t0 */ \
  X(3, TileSpec<24, LDW, true, 0, false, 24, false, 1, 3, W_NONE, 2, 3>)       /* ric_phase2_gemm (bacc), NTW 3 */ \
  X(4, TileSpec<24, LDW, true, 0, false, 24, false, 1, 1, W_NONE, 2, 2>)       /* ric_phase3_mma t1 (bacc, tnb0 1) */ \
  X(5, TileSpec<NU_T, LDW, true, LDN, false, NU_T, true, 1, 2, W_NONE>)        /* ric_phase3_mma t0: Hux' K */ \
  X(6, TileSpec<NU_T, LDW, true, LDN, false, NU_T, true, 1, 1, W_NONE>)        /* ric_phase3_mma t1; hb_kernels.hip GEMM 3 rest */ \
  X(7, TileSpec<24, LDN, true, LDW, false, 24, true, 1, 1, W_NONE>)            /* hb_kernels.hip k_ric_bwd4 GEMM 1 */ \
  X(8, TileSpec<24, LDN, true, LDW, false, 24, true, 1, 2, W_NONE>)            /* hb_kernels.hip k_ric_bwd4 GEMM 1, wide */ \
  X(9, TileSpec<24, LDW, true, LDW, false, 24, true, 1, 1, W_NONE>)            /* hb_kernels.hip k_ric_bwd4 GEMM 2 / GEMM 3 first part */ \
  X(10, TileSpec<8, 9, false, 9, false, 6, false, 2, 1, W_NONE>)               /* hb_lq.hpp momentum Jacobian product */ \
  X(11, TileSpec<12, 12, false, 12, true, 12, false, 1, 2, W_EQ>)              /* hb_lq.hpp masked Gram product, equality rows */ \
  X(12, TileSpec<12, 12, true, LDK, false, 10, false, 1, 2, W_NONE>)           /* hb_lq.hpp ABt' [Kx | ke | Z] */ \
  X(13, TileSpec<12, 12, false, 12, true, 12, false, 1, 2, W_SOFT>)            /* hb_lq.hpp soft-row Gram products (1, 2 tiles wide) */ \
  X(14, TileSpec<12, 10, false, LDK, false, 10, false, 1, 2, W_NONE>)          /* hb_lq.hpp R_jj [Kx | ke | Z] */ \
  X(15, TileSpec<12, 12, false, 12, true, 12, false, 1, 1, W_SOFT>)            /* hb_lq.hpp soft rows, tile (1, 1) */ \
  X(16, TileSpec<12, LDK, true, LDK, false, 10, false, 1, 2, W_NONE>)          /* hb_lq.hpp Kx' M, Z' M */ \
  X(17, TileSpec<12, LDK, true, LDK, false, 10, false, 1, 1, W_NONE>)          /* hb_lq.hpp Kx' M, tile (1, 1) */ \
  X(18, TileSpec<12, 22, true, LDK, false, 10, false, 1, 2, W_NONE>)           /* hb_lq.hpp P_j' Kx */ \
  X(19, TileSpec<12, 22, true, LDK, false, 10, false, 1, 1, W_NONE>)           /* hb_lq.hpp P_j' Kx, tile (1, 1) */
constexpr int N_TILE_SPECS = 20;
// {K, LDA, TA, LDB, TB, KR, PRE, MT, NT, weight kind, MTB, NTB} of instantiation `id`; 0 when it exists
inline int32_t tile_desc(int32_t id, int32_t* d) {
#define HBP_DESC(ID, ...) \
  if (id == ID) { typedef __VA_ARGS__ S; const int32_t v[12] = {S::K, S::LDA, S::TA, S::LDB, S::TB, S::KR, S::PRE, S::MT, S::NT, S::WK, S::MTB, S::NTB}; \
    for (int i = 0; i < 12; ++i) d[i] = v[i]; return 0; }
  HBP_TILE_SPECS(HBP_DESC)
#undef HBP_DESC
  return -1;
}
// operand bases inside the image; Mr / Nr positive (beyond the tile block they are selected away)
inline bool tile_par_ok(const int32_t* p) {
  return p[0] >= 0 && p[1] >= 0 && p[2] >= 0 && p[0] < TILE_LDS && p[1] < TILE_LDS && p[2] < TILE_LDS && p[3] >= 1 && p[4] >= 1 && p[6] >= 0 && p[6] <= 1;
}

// Round trips of the initialisers and stores on a WaveTile<2, 3> (32 x 48 accumulators).  Sources a, b are dense [32][RT_LD] blocks,
// the destination is [.][RT_LDD], pre-filled by the test; RT_WORDS doubles each.  par: 8 ints {op, Mr, Nr, p0, p1, -, -, -}.
// *flag counts initialiser / pre / set_col calls with an index outside the live range (the clamped-index rule of hb_tile.hpp).
constexpr int RT_LD = 50, RT_LDD = 53, RT_WORDS = 2048;
enum RtOp { RT_INIT = 0, RT_INIT_RM, RT_INIT_COL, RT_SET_COL, RT_ADD, RT_STORE_PRE, RT_STORE_RM_COLS };
HB_HD void flag_hit(int* flag) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(flag, 1);
#else
  *flag += 1;
#endif
}
template <class Ctx>
HB_HD void tile_roundtrip_case(const Ctx& cx, const double* a, const double* b, const int* par, double scale, double* dst, int* flag) {
  const int op = par[0], Mr = par[1], Nr = par[2], p0 = par[3], p1 = par[4];
  WaveTile<2, 3> t, o;
  auto in_range = [Mr, Nr, flag](int r, int c) {
    if (r < 0 || r >= Mr || c < 0 || c >= Nr) flag_hit(flag);
  };
  if (op == RT_INIT) {
    tile_init(cx, t, Mr, Nr, [a, in_range](int r, int c) { in_range(r, c); return a[r * RT_LD + c]; });
    tile_store(cx, t, Mr, Nr, [dst](int r, int c, double v) { dst[r * RT_LDD + c] = v; });
    return;
  }
  if (op == RT_INIT_COL) tile_init_col(cx, t, Mr, p0, b);
  else tile_init_rm<RT_LD>(cx, t, Mr, Nr, a);
  if (op == RT_SET_COL) tile_set_col(cx, t, p0, Mr, [b, in_range](int r) { in_range(r, 0); return b[r]; });
  if (op == RT_ADD) {
    tile_init_rm<RT_LD>(cx, o, Mr, Nr, b);
    tile_add(t, o);
  }
  if (op == RT_STORE_PRE) {
    tile_store_pre(cx, t, Mr, Nr, [b, in_range](int r, int c) { in_range(r, c); return b[r * RT_LD + c]; },
                   [dst](int r, int c, double acc, double p) { dst[r * RT_LDD + c] = acc + 2.0 * p; });
  } else if (op == RT_STORE_RM_COLS) {
    tile_store_rm_cols<RT_LDD>(cx, t, Mr, p0, p1, dst, scale);
  } else {
    tile_store_rm<RT_LDD>(cx, t, Mr, Nr, dst, scale);
  }
}
inline bool roundtrip_par_ok(const int32_t* p) {
  return p[0] >= 0 && p[0] <= RT_STORE_RM_COLS && p[1] >= 1 && p[1] <= 32 && p[2] >= 1 && p[2] <= 48 && p[3] >= 0 && p[3] <= 48 && p[4] >= 0 && p[4] <= 48;
}

// ---------------------------------------------------------------------------------------------------------------- QP factorisation
// par: 8 ints {n, mA, lda, ld, wstore, n_head, -, -}; dp: 2 doubles {se | head, tail}.  A: QF_A doubles (row-major, lda), b: 32;
// R, J: QF_R doubles pre-filled by the test; g: 16; np: 64 (workspace of the host form).
constexpr int QF_A = 512, QF_R = 1536;
template <int MA, bool kGrad, bool kHeadTail, class Ctx>
HB_HD void regularised_factor_case(const Ctx& cx, const int* par, const double* dp, const double* A, const double* b, double* R, double* J, double* g,
                                   double* np) {
  const int n = par[0], mA = par[1], lda = par[2], ld = par[3], wstore = par[4], n_head = par[5];
  if constexpr (kHeadTail) regularised_factor<MA, kGrad>(cx, n, mA, A, lda, b, g, HeadTailDiag{dp[0], dp[1], n_head}, R, ld, wstore, np);
  else regularised_factor<MA, kGrad>(cx, n, mA, A, lda, kGrad ? b : nullptr, kGrad ? g : nullptr, UniformDiag(dp[0]), R, ld, wstore, np);
  invert_upper(cx, R, ld, n, J);
}
inline bool regfac_par_ok(const int32_t* p, int MA) {
  const int n = p[0], mA = p[1], lda = p[2], ld = p[3], wstore = p[4];
  return n >= 1 && n <= 16 && mA >= 0 && mA <= MA && lda >= n && MA * lda <= QF_A && ld >= n && wstore <= ld && wstore >= n && n * ld <= QF_R;
}
// givens_insert_row (op 0: R n x n, np) and drop_constraint (op 1: R q x q, J n x n, working-set records).
// par: 8 ints {op, n, ld, l, q (in / out), -, -, -}; R, J: QF_R; np, lam: 64 doubles; act, is_active: 64 ints.
template <class Ctx>
HB_HD void givens_case(const Ctx& cx, int* par, double* R, double* J, double* np, int* act, int* is_active, double* lam) {
  const int op = par[0], n = par[1], ld = par[2], l = par[3];
  int q = par[4];
  if (op == 0) givens_insert_row(cx, R, ld, n, np);
  else drop_constraint(cx, n, ld, R, J, act, lam, is_active, l, q);
  cx.sync();
  if (cx.lane == 0) par[4] = q;
}
inline bool givens_par_ok(const int32_t* p, const int32_t* act) {
  const int op = p[0], n = p[1], ld = p[2], l = p[3], q = p[4];
  if (op < 0 || op > 1 || n < 1 || n > 38 || ld < n || n * ld > QF_R) return false;
  if (op == 1) {
    if (q < 1 || q > n || l < 0 || l >= q) return false;
    for (int i = 0; i < q; ++i)
      if (act[i] < 0 || act[i] >= 64) return false;
  }
  return true;
}

}  // namespace hbp
