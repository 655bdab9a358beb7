// HIP kernels (gfx950) + C-ABI implementation of include/hunter_hip.h.
// One process per GPU; two HIP streams mirror the reference's two threads (MPC thread / control thread,
// legged_controllers/src/LeggedController.cpp:396-421).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <algorithm>
#include <mutex>
#include <vector>

#include "hb_host.hpp"
#include "hb_riccati.hpp"
#include "hb_mpccert.hpp"
#include "hb_lcm.hpp"
#include "hb_wbc.hpp"
#include "hb_hoqp.hpp"
#include "hb_estimator.hpp"
#include "hb_refgen.hpp"
#include "hb_gait.hpp"
#include "hb_plant.hpp"
#include "hb_sensors.hpp"

using namespace hb;

namespace {

struct DeviceCtx {
  int lane, nlanes;
  __device__ DeviceCtx() : lane(threadIdx.x), nlanes(blockDim.x) {}
  __device__ void sync() const { __syncthreads(); }
};
// Context of the kernels whose workgroup is exactly one wavefront and whose lanes exchange data through LDS only.  The
// LDS unit executes the DS instructions of one wave in order, so "every lane's earlier LDS writes are visible to every
// lane's later LDS reads" needs no hardware barrier and, unlike __syncthreads() (a workgroup-scope fence: s_waitcnt
// vmcnt(0)), does not drain the global loads / stores in flight — software-pipelined prefetches stay in flight across
// the phases of a stage.  What remains is a compiler-level ordering point.
struct WaveCtx {
  int lane;
  static constexpr int nlanes = 64;
  __device__ WaveCtx() : lane(threadIdx.x) {}
  __device__ explicit WaveCtx(int l) : lane(l) {}
  __device__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
};

// ---------------------------------------------------------------------------------------------------------
// device-resident problem data of a batch
constexpr int LS_TAIL_MAX = 16;   // step sizes the backtracking tail evaluates side by side (decay 0.5, alpha_min 1e-4: 13 of them)
struct Batch {
  int B, Nmax;
  int* n_nodes;     // [B]
  double* t;        // [B][Nmax+1]
  int* mode;        // [B][Nmax]
  double* xref;     // [B][Nmax][22]
  double* swing;    // [B][Nmax][24]
  double* x;        // [B][Nmax+1][22]
  double* u;        // [B][Nmax][22]
  double* x0;       // [B][22]
  double* recs;     // [B][Nmax][REC_SIZE]
  double* gains;    // [B][Nmax][GAIN_SIZE]
  double* dx;       // [B][Nmax+1][22]
  double* du;       // [B][Nmax][22]
  double* acc;      // [B][4] armijo, base merit, base dyn, base eq
  double* partial;  // [B][Nmax][3]
  double* ls_norm;  // [B][2]: |dx|, |du| (l2, whole trajectory) of the instances whose full step was refused (k_ls_decide)
  double* ls_tail;  // [B][LS_TAIL_MAX][Nmax][3]: per-node line-search partials of the backtracking step sizes, evaluated side by side
  int* accepted;    // [B]
  double* perf;     // [B][4] merit dyn eq step
  int* ric_fail;    // [B]
  int* mpc_status;  // [B] hb_inst_status of the last MPC call
  // iterate of the previous MPC call on ITS time grid (warm start across calls, k_warm_shift); x / u and xp / up swap roles
  double* xp;       // [B][Nmax+1][22]
  double* up;       // [B][Nmax][22]
  double* tp;       // [B][Nmax+1]
  int* modep;       // [B][Nmax]
  int* np_nodes;    // [B]
  int* grid_dirty;  // [B] the node tables changed since the iterate was last brought onto them
  double* lqpark;   // [B][Nmax + LqPark::trip_max][LqPark::size]: phase-1 images of the nodes, parked by the value phase of k_lq_trip
};

__global__ void k_set_x0(Batch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.B * HB_NX) return;
  const int inst = i / HB_NX, c = i % HB_NX;
  b.x[size_t(inst) * (b.Nmax + 1) * HB_NX + c] = b.x0[i];
}

// cold start: x_k = x0, u_k = weight compensation of mode_k (LeggedRobotInitializer.cpp:67-77)
__global__ void k_cold_start(Batch b, const DevModel* __restrict__ M, const unsigned char* mask) {
  const int k = blockIdx.x, inst = blockIdx.y;
  const int lane = threadIdx.x;
  if (mask && !mask[inst]) return;
  if (k == 0 && lane == 0) { b.grid_dirty[inst] = 0; b.mpc_status[inst] = HB_INST_OK; }
  if (k > b.n_nodes[inst]) return;
  double* xk = b.x + (size_t(inst) * (b.Nmax + 1) + k) * HB_NX;
  if (lane < HB_NX) xk[lane] = b.x0[inst * HB_NX + lane];
  if (k < b.n_nodes[inst] && lane < HB_NU) {
    bool cf[HB_NC];
    mode_flags(b.mode[size_t(inst) * b.Nmax + k], cf);
    int nc = 0;
    for (int i = 0; i < HB_NC; ++i) nc += cf[i];
    double v = 0.0;
    if (lane < 12 && lane % 3 == 2 && cf[lane / 3]) v = M->total_mass * M->gravity / nc;
    b.u[(size_t(inst) * b.Nmax + k) * HB_NU + lane] = v;
  }
}

// Warm start across MPC calls: the previous call's iterate (xp, up on the grid tp / modep / np_nodes) is brought onto the new node
// tables — OCS2 SqpSolver::initializeStateInputTrajectories [OCS2-knowledge]: inside the previous horizon the state at every
// new node time and the input at the start of every new interval are interpolated linearly from the previous solution; beyond
// it the initializer takes over (LeggedRobotInitializer.cpp:67-77: the state is carried on, the input is the weight
// compensation of the interval's mode).  Defined here: an input is HELD instead of interpolated across a mode
// switch of the previous solution (the neighbouring node belongs to another contact configuration), and the last previous
// interval holds its input.  One thread per (instance, node); instances whose tables did not change are left alone.
constexpr int kWarmShiftThreads = 256;
__global__ __launch_bounds__(kWarmShiftThreads) void k_warm_shift(Batch b, const DevModel* __restrict__ M) {
  // one thread per (node, entry index) of an instance: it moves state entry e AND input entry e of its node (the interval lookup is the
  // same for both), consecutive threads = consecutive entries, every lane of a wavefront has work (one block per node used 44 of 64
  // lanes; the kernel is a chain of three dependent round trips per thread, so what it costs is wavefronts / resident wavefronts).
  // Instances whose tables did
  // not change keep their iterate (plain copy from the previous buffers: the host swapped them); the others are interpolated
  // from the previous solution on ITS time grid.  The old interval that contains the node time is found by bisection (a
  // linear scan was a chain of up to N dependent loads per block: 0.51 ms per 4096 x 100 launch, 0.06 ms of it memory traffic).
  const int flat = blockIdx.x * kWarmShiftThreads + threadIdx.x, inst = blockIdx.y;
  static_assert(HB_NX == HB_NU, "one thread moves entry e of the state and of the input");
  const int k = flat / HB_NX, e = flat - k * HB_NX;
  const size_t N = b.Nmax;
  if (k > int(N)) return;
  constexpr bool is_x = true, is_u = true;
  const double* xp = b.xp + size_t(inst) * (N + 1) * HB_NX;
  const double* up = b.up + size_t(inst) * N * HB_NU;
  double* xk = b.x + (size_t(inst) * (N + 1) + k) * HB_NX;
  double* uk = b.u + (size_t(inst) * N + k) * HB_NU;
  if (!b.grid_dirty[inst]) {
    if (is_x) xk[e] = xp[size_t(k) * HB_NX + e];
    if (is_u && k < int(N)) uk[e] = up[size_t(k) * HB_NU + e];
    return;
  }
  const int n = b.n_nodes[inst], np = b.np_nodes[inst];
  if (k > n) return;
  const double* tp = b.tp + size_t(inst) * (N + 1);
  const int* mp = b.modep + size_t(inst) * N;
  const double t = b.t[size_t(inst) * (N + 1) + k];
  // old interval that contains t: the largest i in [0, np - 1] with tp[i] <= t (0 if there is none)
  // Between two MPC calls the grid moves by a fraction of an interval, so the answer is k, k + 1 or k - 1 almost always: those three
  // candidates are tested first with loads that do not depend on one another (one round trip); the bisection (up to seven dependent
  // loads per block) is the fallback.  tp is non-decreasing: i is the answer iff tp[i] <= t and (i is the last or tp[i + 1] > t).
  int lo = 0, hi = np > 0 ? np - 1 : 0;
  {
    const int last = hi;
    const int c0 = min(max(k - 1, 0), last);
    const double t0 = tp[c0], t1 = tp[min(c0 + 1, last)], t2 = tp[min(c0 + 2, last)], t3 = tp[min(c0 + 3, last)];
    const double tc[4] = {t0, t1, t2, t3};
    for (int d = 0; d < 3; ++d) {
      const int c = c0 + d;
      if (c <= last && tc[d] <= t && (c == last || tc[d + 1] > t)) { lo = hi = c; break; }
    }
  }
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tp[mid] <= t) lo = mid; else hi = mid - 1;
  }
  const int i = lo;
  const bool beyond = np <= 0 || t >= tp[np], before = !beyond && t <= tp[0];
  const double a = (beyond || before) ? 0.0 : (t - tp[i]) / (tp[i + 1] - tp[i]);
  if (is_x) {
    double v;
    if (beyond) v = xp[size_t(np > 0 ? np : 0) * HB_NX + e];
    else if (before) v = xp[e];
    else v = (1.0 - a) * xp[size_t(i) * HB_NX + e] + a * xp[size_t(i + 1) * HB_NX + e];
    xk[e] = v;
  }
  if (is_u && k < n) {
    double v;
    if (beyond) {  // beyond the previous horizon: weight compensation of this interval's mode
      bool cf[HB_NC];
      mode_flags(b.mode[size_t(inst) * N + k], cf);
      int nc = 0;
      for (int c = 0; c < HB_NC; ++c) nc += cf[c];
      v = (e < 12 && e % 3 == 2 && cf[e / 3]) ? M->total_mass * M->gravity / nc : 0.0;
    } else if (before) {
      v = up[e];
    } else if (i + 1 >= np || mp[i + 1] != mp[i]) {
      v = up[size_t(i) * HB_NU + e];
    } else {
      v = (1.0 - a) * up[size_t(i) * HB_NU + e] + a * up[size_t(i + 1) * HB_NU + e];
    }
    uk[e] = v;
  }
}
__global__ void k_grid_clean(Batch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < b.B) b.grid_dirty[i] = 0;
}
// per-instance status word of an MPC call: a failed Riccati pivot or a non-finite performance index is HB_INST_NAN (the
// step was not taken), a line search that rejected every step size is HB_INST_MAXITER (iterate unchanged)
__global__ void k_mpc_status(Batch b, int first_iteration) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.B) return;
  const double* p = b.perf + size_t(i) * 4;
  // (every forward sweep resets perf to the baseline of THIS iteration with step size 0 — what a no-step exit of the line search
  // reports, like the oracle's res.step = 0 —; an accepted step overwrites it.  acc is the same baseline, kept for the filter.)
  const bool finite = isfinite(b.acc[i * 4 + 0]) && isfinite(b.acc[i * 4 + 1]) && isfinite(b.acc[i * 4 + 2]) && isfinite(b.acc[i * 4 + 3]) &&
                      (!b.accepted[i] || (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])));
  int st = HB_INST_OK;
  if (b.ric_fail[i] || !finite) st = HB_INST_NAN;
  else if (!b.accepted[i]) st = HB_INST_MAXITER;   // (accepted = 2: the search stopped on deltaTol — converged, no step — is OK)
  // sticky over the SQP iterations of one call: the worst word any iteration produced (NAN > INFEASIBLE > MAXITER > OK)
  b.mpc_status[i] = first_iteration ? st : max(b.mpc_status[i], st);
}

// HB_LQ_LDS_PAD: occupancy experiments only (tools/occupancy_variants.sh) — extra (or, negative, missing) doubles of LDS per node
#ifndef HB_LQ_LDS_PAD
#define HB_LQ_LDS_PAD 0
#endif
__global__ __launch_bounds__(64, 3) void k_lq(Batch b, const DevModel* __restrict__ M, const DevConfig* __restrict__ C) {
  const int k = blockIdx.x, inst = blockIdx.y;
  __shared__ double lds[LqLds::total + HB_LQ_LDS_PAD];
  const size_t nd = size_t(inst) * b.Nmax + k;
  const double* tt = b.t + size_t(inst) * (b.Nmax + 1);
  NodeIn in;
  in.x = b.x + (size_t(inst) * (b.Nmax + 1) + k) * HB_NX;
  in.xnext = in.x + HB_NX;
  in.u = b.u + nd * HB_NU;
  in.xref = b.xref + nd * HB_NX;
  in.swing = b.swing + nd * 24;
  // Everything the node's entry reads from global memory is requested BEFORE the node-count test (every node slot of the arrays
  // exists): node count, interval, mode, this lane's entry of x and u, the lane's leg-pass constants — one round trip, not four in a row
  const int n_nodes = b.n_nodes[inst];
  LegJointConst jc;
  lq_leg_const_of_lane(*M, threadIdx.x, jc);
  if (threadIdx.x < HB_NX) { in.x_lane = in.x[threadIdx.x]; in.u_lane = in.u[threadIdx.x]; }
  in.jc = &jc;
  in.preloaded = true;
  const double t_a = tt[k], t_b = tt[k + 1];
  const int mode_v = b.mode[nd];
  if (k >= n_nodes) return;
  {
    const double dtv = t_b - t_a;  // (uniform: kept in a scalar register pair for the whole node)
    const long long bits = __builtin_bit_cast(long long, dtv);
    const unsigned lo = __builtin_amdgcn_readfirstlane(unsigned(bits)), hi = __builtin_amdgcn_readfirstlane(unsigned(bits >> 32));
    in.dt = __builtin_bit_cast(double, (long long)(((unsigned long long)hi << 32) | lo));
  }
  in.mode = __builtin_amdgcn_readfirstlane(mode_v);  // (uniform by construction; tells the compiler so: mode tests become scalar)
  lq_node(WaveCtx(), *M, *C, in, lds, b.recs + nd * REC_SIZE);
}

// The LQ approximation of a TRIP of up to tlen <= 16 consecutive nodes of an instance per wavefront (hb_lq.hpp lq_trip_values): the
// lane-sparse value phases of all the trip's nodes at once, one (node, leg evaluation) pair per lane, their phase-1 images parked in
// global memory; then node after node: image -> LDS, direction pass, tail.  The arithmetic of a node does not depend on the trip
// length (a lane's work is the same whatever its neighbours do), so launches that cut the batch differently agree bit for bit.
__global__ __launch_bounds__(64, 3) void k_lq_trip(Batch b, const DevModel* __restrict__ M, const DevConfig* __restrict__ C, int tlen) {
#if defined(__HIP_DEVICE_COMPILE__)   // (the value phase exists for the device only)
  // Workgroups are handed out in the order of their index: every instance's FULL trips first, the short last trip of each horizon
  // (N = 100, 16 nodes a trip: six full trips and one of four nodes) at the end of the grid, where it fills the gaps the full trips leave
  // on the chip — 4096 x 6 full trips are exactly eight rounds of the 3072 wavefront slots.  (longest job first)
  int trip, inst;
  {
    const int ntrip = (b.Nmax + tlen - 1) / tlen, g = blockIdx.x, nfull = (ntrip - 1) * b.B;
    if (g < nfull) { inst = g / (ntrip - 1); trip = g - inst * (ntrip - 1); }
    else { inst = g - nfull; trip = ntrip - 1; }
    if (ntrip == 1) { inst = g; trip = 0; }
  }
  __shared__ double lds[LqLds::total + HB_LQ_LDS_PAD];
  const int n_nodes = b.n_nodes[inst];
  const int k0 = trip * tlen;
  if (k0 >= n_nodes) return;
  const int nt = min(tlen, n_nodes - k0);
  const double* tt = b.t + size_t(inst) * (b.Nmax + 1);
  double* park = b.lqpark + (size_t(inst) * (b.Nmax + LqPark::trip_max) + k0) * LqPark::size;   // the trip's parked data (LqPark)
  lq_trip_stage_constants(*M, lds, threadIdx.x);
  WaveCtx().sync();
  // (profiling build, 125: the value phase runs once per trip, later launches re-use what it parked — the dense part alone on valid data)
  if (!(HB_ABLATE_ON && C->debug_stop == 125 && park[size_t(LqPark::n_feet / 4 * tlen) * 16] != 0.0)) {
    // (every lane runs the phase: lanes beyond the trip's last node repeat it and park nothing.  Raising the wavefront's priority for
    // this one long dependent chain was tried — s_setprio 3: 515 k against 525 k updates/s — and dropped)
    lq_trip_values(LqTrip{lds, park, tlen, nt, int(threadIdx.x), HB_ABLATE_ON ? C->debug_stop : 0}, *M, *C, b.x + size_t(inst) * (b.Nmax + 1) * HB_NX, b.u + size_t(inst) * b.Nmax * HB_NU,
                   b.swing + size_t(inst) * b.Nmax * 24, tt, b.mode + size_t(inst) * b.Nmax, k0);
  }
  // the images are read back by other lanes of this wavefront: stores complete before the first load is issued
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#if defined(HB_ABLATE) && defined(HB_LQV_TRACE)
  if (C->debug_stop == 118 && blockIdx.x == 1000 && threadIdx.x == 0) {
    const long long* m = reinterpret_cast<const long long*>(lds + LqLds::total - 24);
    const long long t12 = __builtin_readcyclecounter();
    printf("lq value-phase trace (cycles): loads %lld | fwd sweep %lld | feet %lld | bwd joints %lld %lld %lld %lld %lld | stash %lld | wait %lld | value pass 0 %lld | 1 %lld | drain %lld\n",
           m[1] - m[0], m[2] - m[1], 0LL, m[3] - m[2], m[4] - m[3], m[5] - m[4], m[6] - m[5], m[7] - m[6], m[8] - m[7], m[9] - m[8], m[10] - m[9], m[11] - m[10], t12 - m[11]);
    printf("   value pass 1: stash reads %lld | point values %lld | contact point, sums %lld | hand-out %lld | park %lld\n", m[12] - m[10], m[13] - m[12], m[14] - m[13], m[15] - m[14], m[11] - m[15]);
  }
  if (C->debug_stop == 118) return;
#endif
  if (HB_ABLATE_ON && C->debug_stop >= 126 && C->debug_stop <= 128) return;   // profiling build: the value phase alone (127 / 128: parts of it)
  // the lane's entry of the table the cost phase reads per lane, for all the trip's nodes (NodeIn::consts)
  const double c_tab = lq_lane_constants(*M, *C, threadIdx.x);
  for (int t = 0; t < nt; ++t) {
    // (the lane id is rebuilt from an opaque copy every node: as loop invariants the compiler hoists the per-lane offsets of the whole
    // node out of the loop and spills them — as in k_ric_bwd)
    int l = threadIdx.x;
    asm volatile("" : "+v"(l));
    l &= 63;   // (the range is what lets the compiler turn the lane-strided loops of the node into single passes)
    const WaveCtx cx(l);
    const int k = k0 + t;
    const size_t nd = size_t(inst) * b.Nmax + k;
    NodeIn in;
    in.x = b.x + (size_t(inst) * (b.Nmax + 1) + k) * HB_NX;
    in.xnext = in.x + HB_NX;
    in.u = b.u + nd * HB_NU;
    in.xref = b.xref + nd * HB_NX;
    in.swing = b.swing + nd * 24;
    double x_lane = 0.0, u_lane = 0.0;
    if (l < HB_NX) { x_lane = in.x[l]; u_lane = in.u[l]; }
    {
      const double dtv = tt[k + 1] - tt[k];  // (uniform: kept in a scalar register pair for the whole node)
      const long long bits = __builtin_bit_cast(long long, dtv);
      const unsigned lo = __builtin_amdgcn_readfirstlane(unsigned(bits)), hi = __builtin_amdgcn_readfirstlane(unsigned(bits >> 32));
      in.dt = __builtin_bit_cast(double, (long long)(((unsigned long long)hi << 32) | lo));
    }
    in.mode = __builtin_amdgcn_readfirstlane(b.mode[nd]);
    in.consts = true;
    in.c_tab = c_tab;
    lq_image_to_lds(park, t, tlen, lds, l);
    if (l < HB_NX) { lds[LqLds::xs + l] = x_lane; lds[LqLds::us + l] = u_lane; }
    cx.sync();
    const double* park_lds = lds + LqLds::park;
    const double* xnext_lds = lds + LqLds::xnext_park;
    // (profiling build, 117: every node of a workgroup writes ONE record slot — the stores are issued, their lines stay in the L2)
    double* recp = b.recs + ((HB_ABLATE_ON && C->debug_stop == 117) ? size_t(blockIdx.x & 4095) : nd) * REC_SIZE;
    lq_node_dense(cx, *M, *C, in, lds, recp, [park_lds](int i) { return park_lds[i]; }, [xnext_lds](int i) { return xnext_lds[i]; });
    cx.sync();
  }
#endif
}

constexpr int kRicBwd4MaxBatch = 512;    // instances per launch up to which the four-wavefront backward sweep is taken (measured)
__global__ __launch_bounds__(64, 2) void k_ric_bwd(Batch b, int dbg) {
  // per-instance serial chain: when this kernel shares SIMDs with the node-parallel LQ kernel of another chunk stream (chunked
  // hb_step_resident), it is the latency-critical one — ask the arbiter to issue it first
  __builtin_amdgcn_s_setprio(3);
  const int inst = blockIdx.x;
  __shared__ double lds[RicLds::total];
  const WaveCtx cx;
  for (int i = cx.lane; i < RicLds::total; i += cx.nlanes) lds[i] = 0.0;  // S = 0, s = 0 and every padding zero
  cx.sync();
  const int n = b.n_nodes[inst];
  // Staging of a stage record through registers, 16-byte loads, every load of a lane issued before the first is
  // consumed.  The Riccati part of the record is the LDS image (hb_lq.hpp REC_* layout), so staging is two straight copies:
  //   buf[r]    pair l + 64 r of doubles [0, REC_QT): rows of [A~ b~ B~ .] -> RicLds::ABb, rows of [P~ r~ R~ .] -> RicLds::PRr
  //   bufq[r]   pair l + 64 r of [Q~ (upper triangle, packed) | q~] (138 pairs), dropped over the dead A~ block at the end of the stage (RicLds::Qs)
  // Slots beyond a block read a few doubles further inside the same record and are never stored.
  // Software pipeline (WaveCtx::sync does not drain global loads): [Q~ q~] of stage k and the staged part of stage k-1
  // are requested between the factorisation and the last GEMM of stage k — requested earlier they would be live across
  // the register-resident Cholesky, the register peak of the kernel.
  constexpr int NL = 10, NPQ = (REC_QT_PACKED + 22) / 2, NQ = (NPQ + 63) / 64, NP_AB = REC_PR / 2, NP = REC_QT / 2;  // 396 pairs of [A~ b~ B~ .], 612 pairs staged; 138 of [Q~ | q~]
  static_assert(NP <= 64 * NL && 64 * NL * 2 + 2 * 64 * NQ <= REC_SIZE && REC_QT % 2 == 0 && REC_PR % 2 == 0, "record layout");
  typedef double d2 __attribute__((ext_vector_type(2)));  // (HIP's double2 struct kept the buffers in scratch memory)
  d2 buf[NL], bufq[NQ];
#define HB_RIC_FETCH(kk, l)                                                                                        \
  {                                                                                                                \
    const d2* rec2_ = reinterpret_cast<const d2*>(b.recs + (size_t(inst) * b.Nmax + (kk)) * REC_SIZE) + (l);       \
    _Pragma("unroll") for (int r = 0; r < NL; ++r) buf[r] = rec2_[64 * r];                                         \
  }
#define HB_RIC_FETCH_Q(kk, l)                                                                                      \
  {                                                                                                                \
    const d2* rec2_ = reinterpret_cast<const d2*>(b.recs + (size_t(inst) * b.Nmax + (kk)) * REC_SIZE) + NP + (l);  \
    _Pragma("unroll") for (int r = 0; r < NQ; ++r) bufq[r] = rec2_[64 * r];                                        \
  }
  double meta_nf = 0.0, meta_nz = 0.0;
  if (n > 0) {
    HB_RIC_FETCH(n - 1, cx.lane);
    const double* meta = b.recs + (size_t(inst) * b.Nmax + n - 1) * REC_SIZE + REC_META;
    meta_nf = meta[0];
    meta_nz = meta[1];
  }
#if defined(HB_ABLATE)
  // cycle-counter trace of one stage (tools/perf_quick.py --stop 197): the marks live in the slack words behind RicLds::flag, not in registers
  long long* t1_ = reinterpret_cast<long long*>(lds + RicLds::flag + 8);
#define HB_RIC1_MARK(i) if (dbg == 197 && blockIdx.x == 9 && k == 50 && cx.lane == 0) t1_[i] = __builtin_readcyclecounter();
#else
#define HB_RIC1_MARK(i)
#endif
  for (int k = n - 1; k >= 0; --k) {
    HB_RIC1_MARK(0)
    // Per-lane addresses are rebuilt every stage from an opaque copy of the lane id: as loop invariants the compiler
    // hoisted ~100 of them out of the loop and then spilled them to scratch around the Cholesky, and every scratch
    // reload drains the prefetch (s_waitcnt vmcnt(0)).
    int l = cx.lane;
    asm volatile("" : "+v"(l));
    WaveCtx cxk = cx;  // lane id the compiler cannot trace back to threadIdx: nothing derived from it is loop invariant
    cxk.lane = l;
    {
      d2* st = reinterpret_cast<d2*>(lds + RicLds::ABb) + l;
#pragma unroll
      for (int r = 0; r < NL; ++r) {
        const int p = l + 64 * r;  // rows of [P~ r~ R~ .] start 2 x 36 doubles further (K-padding rows of the A~ block)
        const int shift = (RicLds::PRr - RicLds::ABb - REC_PR) / 2;
        if (64 * r + 63 < NP_AB) st[64 * r] = buf[r];
        else if (64 * r >= NP_AB) { if (p < NP) st[64 * r + shift] = buf[r]; }
        else st[64 * r + (p < NP_AB ? 0 : shift)] = buf[r];
      }
    }
    cx.sync();
    if (HB_ABLATE_ON && dbg == 20) { if (k > 0) HB_RIC_FETCH(k - 1, l); continue; }  // profiling ablation: staging only
    // n_til: number of projected inputs of this stage (uniform; requested one stage ahead with the prefetch)
    const int n_til = int(meta_nf) + int(meta_nz);
    HB_RIC1_MARK(1)
    WaveTile<2, 2> m1;   // M1 = S [A~ b~ B~] stays in the accumulators of GEMM 1 for GEMM 2 and GEMM 3 (hb_riccati.hpp ric_phase1)
    ric_phase12(cxk, lds, b.gains + (size_t(inst) * b.Nmax + k) * GAIN_SIZE, n_til, m1, dbg);
    HB_RIC1_MARK(2)
    asm volatile("" : "+v"(l));
    cxk.lane = l;
    HB_RIC_FETCH_Q(k, l);
    {  // (requested a whole stage earlier — right after the staging stores, 254 VGPRs, no scratch — the sweep takes the same 2.06 ms:
       //  it does not wait for HBM, it is bound by its own dependent work.)
       // UNCONDITIONAL: the last stage requests its own record once more.  Under `if (k > 0)` the 40 prefetch registers were live
       // through the whole stage for the compiler (the old values "survive" the iteration that does not refill them), right across
       // the register-resident factorisation.
      const int kn = k > 0 ? k - 1 : 0;
      HB_RIC_FETCH(kn, l);
      const double* meta = b.recs + (size_t(inst) * b.Nmax + kn) * REC_SIZE + REC_META;
      meta_nf = meta[0];
      meta_nz = meta[1];
    }
    if (HB_ABLATE_ON && (dbg == 21 || dbg == 22 || dbg == 23)) continue;
    RicT3 t;
    HB_RIC1_MARK(3)
    ric_phase3_mma(cxk, lds, t, m1);
    HB_RIC1_MARK(4)
    {
      d2* Qs2 = reinterpret_cast<d2*>(lds + RicLds::Qs) + l;
#pragma unroll
      for (int r = 0; r < NQ; ++r)
        if (l + 64 * r < NPQ) Qs2[64 * r] = bufq[r];
    }
    ric_phase3_finish(cxk, lds, t);
    HB_RIC1_MARK(5)
#if defined(HB_ABLATE)
    if (dbg == 197 && blockIdx.x == 9 && k == 50 && cx.lane == 0)
      printf("ric1 trace: stage-in %lld | GEMM 1 + GEMM 2 + factor + solves %lld | fetch %lld | GEMM 3 %lld | Q~ + store %lld  (cycles)\n", t1_[1] - t1_[0], t1_[2] - t1_[1],
             t1_[3] - t1_[2], t1_[4] - t1_[3], t1_[5] - t1_[4]);
#endif
  }
#undef HB_RIC_FETCH
#undef HB_RIC_FETCH_Q
  if (cx.lane == 0) b.ric_fail[inst] = lds[RicLds::flag] != 0.0 ? 1 : 0;
}

// The backward sweep with FOUR wavefronts per instance — one per SIMD of a compute unit — for batches that leave most SIMDs idle
// in k_ric_bwd (<= 1024 instances: one single-wavefront sweep per SIMD or fewer, and the launch takes n stages x the chain of one
// stage whatever the chip could do next to it).  The stage is the same arithmetic in the same order (bit-identical gains and value
// function: every 16 x 16 output tile is accumulated by one wavefront over K exactly as in the one-wavefront form), cut by tiles:
//   staging   612 + 253 pairs over 256 threads (4 loads each instead of 14)
//   GEMM 1    M1 = S [A~ b~ B~] (+ s): four tiles, one per wavefront (12-wide stages: 2 + 2 + 1 + 1)
//   GEMM 2    Hu = B~' M1 + [P~ r~ R~]: one tile per wavefront (two or three wavefronts)
//   factor    wavefront 0 (register Cholesky + the 23 solves, as before); the others request the next record meanwhile
//   GEMM 3    T = A~' M1 + Hux' K~ + Q~ on its upper block triangle: three tiles, one per wavefront, each stores its part of S
// with a workgroup barrier between the phases (five per stage).  Buffers are not shared between phases (Ric4Lds).
// Workgroup barrier for data exchanged through LDS only: this wavefront's LDS operations have completed (lgkmcnt(0)), then s_barrier.
// __syncthreads() also waits for vmcnt(0), i.e. for every global load in flight — it would expose the latency of the record prefetch
// of the sweep at the first barrier behind it, once per stage.
__device__ __forceinline__ void block_sync_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__global__ __launch_bounds__(256, 2) void k_ric_bwd4(Batch b, int dbg) {
  __builtin_amdgcn_s_setprio(3);
  const int inst = blockIdx.x, tid = threadIdx.x;
  // Role of this wavefront in the stage (0: the factorisation).  Rotated by instance: with two instances on a CU the wavefronts with
  // the same index share a SIMD, and two factorisations — the longest, VALU-bound phase — on one SIMD while three SIMDs wait at the
  // barrier cost 25 % of the sweep (4.5 against 3.6 us per stage measured)
  const int w = __builtin_amdgcn_readfirstlane(((tid >> 6) + (blockIdx.x ^ (blockIdx.x >> 8))) & 3);
  __shared__ double lds[Ric4Lds::total];
  for (int i = tid; i < Ric4Lds::total; i += 256) lds[i] = 0.0;  // S = 0, s = 0 and every padding zero
  block_sync_lds();
  const int n = b.n_nodes[inst];
  using L = Ric4Lds;
  constexpr int NP_AB = REC_PR / 2, NP = REC_QT / 2, NPQ = (REC_QT_PACKED + 22) / 2;   // 396 pairs of [A~ b~ B~ .], 612 pairs staged, then 138 pairs of [Q~ | q~]
  static_assert(NP <= 256 * 3 && 2 * (NP + 256) <= REC_SIZE, "record layout");
  typedef double d2 __attribute__((ext_vector_type(2)));
  d2 buf[3], bufq;
#define HB_RIC4_FETCH(kk, t)                                                                                   \
  {                                                                                                            \
    const d2* rec2_ = reinterpret_cast<const d2*>(b.recs + (size_t(inst) * b.Nmax + (kk)) * REC_SIZE) + (t);   \
    _Pragma("unroll") for (int r = 0; r < 3; ++r) buf[r] = rec2_[256 * r];                                     \
    bufq = rec2_[NP];                                                                                          \
  }
  double meta_nf = 0.0, meta_nz = 0.0;
  if (n > 0) {
    HB_RIC4_FETCH(n - 1, tid);
    const double* meta = b.recs + (size_t(inst) * b.Nmax + n - 1) * REC_SIZE + REC_META;
    meta_nf = meta[0];
    meta_nz = meta[1];
  }
  double* S = lds + L::S;
  double* sv = lds + L::s;
  double* M1 = lds + L::M1;
  double* ABb = lds + L::ABb;
  double* PRr = lds + L::PRr;
  double* Hu = lds + L::Hu;
  double* Kk = lds + L::Kk;
  double* Qs = lds + L::Qs;
#if defined(HB_ABLATE)
  long long tr_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define HB_RIC4_MARK(i) if (dbg == 199 && blockIdx.x == 7 && k == 50) tr_[i] = __builtin_readcyclecounter();
#else
#define HB_RIC4_MARK(i)
#endif
  for (int k = n - 1; k >= 0; --k) {
    int t = tid;
    asm volatile("" : "+v"(t));   // (nothing derived from the thread id is a loop invariant: see k_ric_bwd)
    const WaveCtx cx(t & 63);
    HB_RIC4_MARK(0)
    {
      d2* ab2 = reinterpret_cast<d2*>(ABb);
      d2* pr2 = reinterpret_cast<d2*>(PRr);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int p = t + 256 * r;
        if (p < NP_AB) ab2[p] = buf[r];
        else if (p < NP) pr2[p - NP_AB] = buf[r];
      }
      if (t < NPQ) reinterpret_cast<d2*>(Qs)[t] = bufq;
    }
    // n_til: number of projected inputs of this stage (uniform; it came with the prefetch)
    const int n_til = int(meta_nf) + int(meta_nz);
    // The next record is requested NOW — four 16-byte loads per thread, 8 registers: the whole stage covers their latency (the
    // one-wavefront form holds 14 loads per lane and can only afford them behind its register-resident factorisation)
    {  // (unconditional — the last stage requests its own record again: see k_ric_bwd)
      const int kn = k > 0 ? k - 1 : 0;
      HB_RIC4_FETCH(kn, t);
      const double* meta = b.recs + (size_t(inst) * b.Nmax + kn) * REC_SIZE + REC_META;
      meta_nf = meta[0];
      meta_nz = meta[1];
    }
    block_sync_lds();
    HB_RIC4_MARK(1)
    if (HB_ABLATE_ON && dbg == 24) continue;   // profiling ablation: staging only
    double* gains = b.gains + (size_t(inst) * b.Nmax + k) * GAIN_SIZE;
    const bool wide = n_til > 9;   // 12 projected inputs (double support): three 16-column tiles, 12 x 12 factor
    // ---- GEMM 1: M1 = S [A~ b~ B~ .] (+ s in the vector column)
    {
      const int NC = wide ? L::LDW : 32;
      auto run = [&](auto& tl, int tm, int c0) {
        tile_init_col(cx, tl, 22 - 16 * tm, L::CV - c0, sv + 16 * tm);   // (sv + 16 .. 31 runs into M1: mapped, selected away)
        HB_RIC4_MARK(8)
        tile_mma<24, L::LDN, true, L::LDW, false, 24, true>(cx, tl, S + 16 * tm, ABb + c0, 22 - 16 * tm, NC - c0);   // S(i, k) read as S(k, i): see ric_phase1
        HB_RIC4_MARK(9)
        tile_store_rm<L::LDW>(cx, tl, 22 - 16 * tm, NC - c0, M1 + 16 * tm * L::LDW + c0);
        HB_RIC4_MARK(10)
      };
      if (!wide) {
        WaveTile<1, 1> tl;
        run(tl, w & 1, 16 * (w >> 1));
      } else if (w < 2) {
        WaveTile<1, 2> tl;
        run(tl, w, 0);
      } else {
        WaveTile<1, 1> tl;
        run(tl, w - 2, 32);
      }
    }
    block_sync_lds();
    HB_RIC4_MARK(2)
    if (HB_ABLATE_ON && dbg == 25) continue;   // ... + GEMM 1
    // ---- GEMM 2: Hu = B~' M1 + [P~ r~ R~ .]  (every element of [P~ r~ R~] is read and replaced by the lane that owns it)
    if (w < (wide ? 3 : 2)) {
      const int NC = wide ? L::LDW : 32, c0 = 16 * w;
      WaveTile<1, 1> tl;
      tile_init_rm<L::LDW>(cx, tl, NU_T, NC - c0, PRr + c0);
      tile_mma<24, L::LDW, true, L::LDW, false, 24, true>(cx, tl, ABb + L::CU, M1 + c0, NU_T, NC - c0);
      tile_store_rm<L::LDW>(cx, tl, NU_T, NC - c0, Hu + c0);
    }
    block_sync_lds();
    HB_RIC4_MARK(3)
    if (HB_ABLATE_ON && dbg == 26) continue;   // ... + GEMM 2
    // ---- factor + solves on wavefront 0.  Meanwhile wavefronts 1..3 start GEMM 3, T = Q~ + A~' M1 + Hux' K~ on its upper block
    // triangle (tiles (0,0) / (0,1) / (1,1), one each): the A~' M1 part does not need the gains — six of a tile's nine matrix
    // instructions run under the factorisation, in the same accumulator and the same order as in the one-wavefront form
    const int ti = w - 1;
    const int r0 = ti == 2 ? 16 : 0, c0 = ti == 0 ? 0 : 16;
    const int Mr = ti == 2 ? 6 : 16, Nr = ti == 0 ? 16 : 7;
    WaveTile<1, 1> t3;
    if (w == 0) {
      if (!wide) ric_factor_solve<9>(cx, Hu, Kk, lds + L::flag, gains);
      else ric_factor_solve<NU_T>(cx, Hu, Kk, lds + L::flag, gains);
    } else {
      tile_init(cx, t3, Mr, Nr, [](int, int) { return 0.0; });
      tile_mma<24, L::LDW, true, L::LDW, false, 24, true>(cx, t3, ABb + r0, M1 + c0, Mr, Nr);
    }
    HB_RIC4_MARK(4)
    block_sync_lds();
    HB_RIC4_MARK(5)
    if (HB_ABLATE_ON && dbg == 27) continue;   // ... + factor, solves | first part of GEMM 3
    // ---- rest of GEMM 3: + Hux' K~, + Q~, new S | s (mirrored)
    if (w != 0) {
      tile_mma<NU_T, L::LDW, true, L::LDN, false, NU_T, true>(cx, t3, Hu + r0, Kk + c0, Mr, Nr);
      HB_RIC4_MARK(11)
      ric_store_T<L::LDN>(cx, t3, Mr, Nr, r0, c0, S, sv, Qs, lds + L::flag + 2);
    }
    HB_RIC4_MARK(6)
    block_sync_lds();
    HB_RIC4_MARK(7)
#if defined(HB_ABLATE)
    if (dbg == 199 && blockIdx.x == 7 && k == 50 && (tid & 63) == 0)
      printf("ric4 trace role %d: stage-in %lld gemm1 %lld (init %lld mma %lld store %lld barrier %lld) gemm2 %lld | own work %lld wait %lld | gemm3b %lld (mma %lld) wait %lld  (cycles)\n", w,
             tr_[1] - tr_[0], tr_[2] - tr_[1], tr_[8] - tr_[1], tr_[9] - tr_[8], tr_[10] - tr_[9], tr_[2] - tr_[10], tr_[3] - tr_[2], tr_[4] - tr_[3], tr_[5] - tr_[4],
             tr_[6] - tr_[5], tr_[11] - tr_[5], tr_[7] - tr_[6]);
#endif
  }
#undef HB_RIC4_FETCH
  if (tid == 0) b.ric_fail[inst] = lds[Ric4Lds::flag] != 0.0 ? 1 : 0;
}

// Forward sweep, one wavefront per instance.  Two forms of the same arithmetic (hb_riccati.hpp: every dot product in four partial
// sums, (p0 + p1) + (p2 + p3)), bit-identical (test_sqp_step_identical_with_either_form_of_the_sweeps):
//   WAVE = false  a lane owns a row (riccati_fwd_node): 56 registers, a long chain of LDS reads per stage — a light resident that fills
//                 the holes other instance ranges' kernels leave; what large batches want (k_ric_fwd moves 8.7 KB per stage and is at the
//                 HBM rate, 4.8 TB/s, once a SIMD holds three or four of them);
//   WAVE = true   four lanes per row, no divergence (riccati_fwd_stage_wave): the stage is ~ 2.5 x shorter — what a batch that leaves the
//                 SIMDs one wavefront each wants (512 instances: 0.177 -> 0.11 ms, then also at the HBM rate, 4.2 TB/s).  130 registers;
//                 on 1024 .. 4096 instances in four free-running ranges it measured 1 .. 5 % SLOWER than the row form (it is a worse
//                 neighbour), hence the selection by concurrent instances in launch_ric_fwd.
// (Requesting the records more than one stage ahead — four register sets — bought nothing in either regime.)
template <bool WAVE>
__device__ __forceinline__ void ric_fwd_body(const Batch& b) {
#if defined(__HIP_DEVICE_COMPILE__)   // (the wave form of the step only exists in the device pass)
  __builtin_amdgcn_s_setprio(3);  // see k_ric_bwd
  const int inst = blockIdx.x;
  __shared__ double lds[FwdLds::total];
  const WaveCtx cx;
  for (int i = cx.lane; i < FwdLds::small; i += cx.nlanes) lds[i] = 0.0;  // dx0 = 0: x[0] is the measured state
  cx.sync();
  const int n = b.n_nodes[inst];
  // What a step reads — the [A~ b~ B~ .] rows and the recovery part of the stage record, the gains — is staged into LDS
  // with coalesced 16-byte loads, one stage ahead (WaveCtx::sync does not drain the loads in flight): the matrix-vector
  // products then run out of LDS instead of waiting for scattered global loads on the dx -> dx+ dependency chain.
  constexpr int P_AB = 12 * REC_LD / 2, P_RX = (REC_RX_END - REC_KX) / 2, P_G = GAIN_SIZE / 2;  // 216, 182, 144 pairs
  constexpr int N_AB = (P_AB + 63) / 64, N_RX = (P_RX + 63) / 64, N_G = (P_G + 63) / 64;        // 4, 3, 3 loads per lane
  typedef double d2 __attribute__((ext_vector_type(2)));
  d2 bab[N_AB], brx[N_RX], bg[N_G];
  const int l = cx.lane;
#define HB_FWD_FETCH(kk)                                                                                  \
  {                                                                                                       \
    const size_t nd_ = size_t(inst) * b.Nmax + (kk);                                                      \
    const d2* pab_ = reinterpret_cast<const d2*>(b.recs + nd_ * REC_SIZE + REC_AB) + l;                   \
    const d2* prx_ = reinterpret_cast<const d2*>(b.recs + nd_ * REC_SIZE + REC_KX) + l;                   \
    const d2* pg_ = reinterpret_cast<const d2*>(b.gains + nd_ * GAIN_SIZE) + l;                           \
    _Pragma("unroll") for (int r = 0; r < N_AB; ++r) bab[r] = (64 * r + 63 < P_AB || l + 64 * r < P_AB) ? pab_[64 * r] : d2{0.0, 0.0}; /* (the last round used to fetch 40 pairs nobody reads: 640 B of the stage's 9.3 KB) */ \
    _Pragma("unroll") for (int r = 0; r < N_RX; ++r) brx[r] = (64 * r + 63 < P_RX || l + 64 * r < P_RX) ? prx_[64 * r] : d2{0.0, 0.0}; \
    _Pragma("unroll") for (int r = 0; r < N_G; ++r) bg[r] = (64 * r + 63 < P_G || l + 64 * r < P_G) ? pg_[64 * r] : d2{0.0, 0.0}; \
  }
  if (n > 0) HB_FWD_FETCH(0);
  FwdLane L;
  if (WAVE) fwd_lane_init(l, L);
  double accp = 0.0, accm = 0.0;
  for (int k = 0; k < n; ++k) {
    {
      d2* sab = reinterpret_cast<d2*>(lds + FwdLds::AB) + l;
      d2* srx = reinterpret_cast<d2*>(lds + FwdLds::RX) + l;
      d2* sg = reinterpret_cast<d2*>(lds + FwdLds::G) + l;
#pragma unroll
      for (int r = 0; r < N_AB; ++r) if (64 * r + 63 < P_AB || l + 64 * r < P_AB) sab[64 * r] = bab[r];
#pragma unroll
      for (int r = 0; r < N_RX; ++r) if (64 * r + 63 < P_RX || l + 64 * r < P_RX) srx[64 * r] = brx[r];
#pragma unroll
      for (int r = 0; r < N_G; ++r) if (64 * r + 63 < P_G || l + 64 * r < P_G) sg[64 * r] = bg[r];
    }
    cx.sync();
    if (k + 1 < n) HB_FWD_FETCH(k + 1);
    const size_t nd = size_t(inst) * b.Nmax + k;
    double* dxo = b.dx + (size_t(inst) * (b.Nmax + 1) + k) * HB_NX;
    if (WAVE) riccati_fwd_stage_wave(cx, lds, L, accp, accm, dxo, b.du + nd * HB_NU);
    else riccati_fwd_node(cx, lds, lds + FwdLds::AB, lds + FwdLds::RX, lds + FwdLds::G, dxo, b.du + nd * HB_NU);
  }
#undef HB_FWD_FETCH
  if (WAVE) {   // (the row form keeps these sums in LDS)
    if (cx.lane < 22) lds[FwdLds::accp + cx.lane] = accp;
    else if (cx.lane < 25) lds[FwdLds::acc + cx.lane - 21] = accm;
    cx.sync();
  }
  riccati_fwd_finish(cx, lds);
  if (cx.lane < HB_NX) b.dx[(size_t(inst) * (b.Nmax + 1) + n) * HB_NX + cx.lane] = lds[FwdLds::dx + cx.lane];
  if (cx.lane < 4) b.acc[inst * 4 + cx.lane] = lds[FwdLds::acc + cx.lane];
  if (cx.lane == 0) {
    b.accepted[inst] = 0;
    b.perf[inst * 4 + 0] = lds[FwdLds::acc + 1];
    b.perf[inst * 4 + 1] = lds[FwdLds::acc + 2];
    b.perf[inst * 4 + 2] = lds[FwdLds::acc + 3];
    b.perf[inst * 4 + 3] = 0.0;
  }
#endif
}
__global__ __launch_bounds__(64) void k_ric_fwd(Batch b) { ric_fwd_body<false>(b); }
__global__ __launch_bounds__(64) void k_ric_fwd_w(Batch b) { ric_fwd_body<true>(b); }
constexpr int kRicFwdWaveMaxBatch = 512;

// ---- KKT certificate of the stage QP (hb_mpccert.hpp), on demand: hb_mpc_get_certificate.  Work buffers of the instances of `b`.
struct MpcCertBuf {
  double* node;     // [B][Nmax][CertNode::size]
  double* costate;  // [B][Nmax+1][22]
  double* cert;     // [B][MPC_CERT_SIZE]
  double* util;     // [B][Nmax][12]: u~ as hb_mpc_get_certificate returns it
};
// One wavefront per (instance, node), grid as k_lq.  The Riccati part of the record and the gains are staged with 16-byte loads, every
// load of a lane requested before the first is stored (the record is the LDS image: straight copies).  A node behind the horizon, and
// every node of an instance whose MPC call ended HB_INST_NAN, only zeroes its u~ row.
__global__ __launch_bounds__(64) void k_mpc_cert_nodes(Batch b, MpcCertBuf cb) {
  const int k = blockIdx.x, inst = blockIdx.y;
  __shared__ double lds[CertLds::total];
  const WaveCtx cx;
  const int l = cx.lane;
  const size_t nd = size_t(inst) * b.Nmax + k;
  double* out = cb.node + nd * CertNode::size;
  if (k >= b.n_nodes[inst] || b.mpc_status[inst] == HB_INST_NAN) {
    if (l < 12) cb.util[nd * 12 + l] = 0.0;
    return;
  }
  constexpr int P_REC = CERT_REC_LEN / 2, P_G = GAIN_SIZE / 2, N_REC = (P_REC + 63) / 64, N_G = (P_G + 63) / 64;   // 750, 144 pairs: 12, 3 loads per lane
  typedef double d2 __attribute__((ext_vector_type(2)));
  d2 brec[N_REC], bg[N_G];
  const d2* prec = reinterpret_cast<const d2*>(b.recs + nd * REC_SIZE) + l;
  const d2* pg = reinterpret_cast<const d2*>(b.gains + nd * GAIN_SIZE) + l;
#pragma unroll
  for (int r = 0; r < N_REC; ++r) brec[r] = (64 * r + 63 < P_REC || l + 64 * r < P_REC) ? prec[64 * r] : d2{0.0, 0.0};
#pragma unroll
  for (int r = 0; r < N_G; ++r) bg[r] = (64 * r + 63 < P_G || l + 64 * r < P_G) ? pg[64 * r] : d2{0.0, 0.0};
  const double dxv = l < 44 ? b.dx[(size_t(inst) * (b.Nmax + 1) + k) * HB_NX + l] : 0.0;   // dx_k, dx_(k+1): 44 consecutive doubles
  {
    d2* srec = reinterpret_cast<d2*>(lds + CertLds::rec) + l;
    d2* sg = reinterpret_cast<d2*>(lds + CertLds::G) + l;
#pragma unroll
    for (int r = 0; r < N_REC; ++r) if (64 * r + 63 < P_REC || l + 64 * r < P_REC) srec[64 * r] = brec[r];
#pragma unroll
    for (int r = 0; r < N_G; ++r) if (64 * r + 63 < P_G || l + 64 * r < P_G) sg[64 * r] = bg[r];
    if (l < 44) lds[l < 22 ? CertLds::dx + l : CertLds::dxn + l - 22] = dxv;
  }
  cx.sync();
  mpc_cert_node(cx, lds, k == 0, out);
  if (l < 12) cb.util[nd * 12 + l] = lds[CertLds::ut + l];
}

// One wavefront per instance, backward over the stages: per stage the 22 rows of [A~ b~ B~ .] (396 pairs, 16-byte loads) and the lane's
// entry of c_k / d_k, requested one stage ahead (WaveCtx::sync does not drain them).  Rows behind the horizon of the costate output
// are zeroed; an HB_INST_NAN instance gets a zero costate and NaN fields.
__global__ __launch_bounds__(64) void k_mpc_cert_sweep(Batch b, MpcCertBuf cb) {
  const int inst = blockIdx.x;
  __shared__ double lds[CertSweepLds::total];
  const WaveCtx cx;
  const int l = cx.lane;
  const int n = b.n_nodes[inst];
  const bool certified = b.mpc_status[inst] != HB_INST_NAN;
  double* costate = cb.costate + size_t(inst) * (b.Nmax + 1) * HB_NX;
  const double* nodes = cb.node + size_t(inst) * b.Nmax * CertNode::size;
  mpc_cert_sweep_init(cx, lds);
  for (int e = (certified ? n * HB_NX : 0) + l; e < (b.Nmax + 1) * HB_NX; e += 64) costate[e] = 0.0;   // lambda_n = 0 and the rows behind it
  if (certified) {
    constexpr int P_AB = REC_PR / 2, N_AB = (P_AB + 63) / 64;   // 396 pairs: 7 loads per lane
    typedef double d2 __attribute__((ext_vector_type(2)));
    d2 bab[N_AB];
    double cdv = 0.0;
    const int cd_off = l < 22 ? CertNode::c + l : (l >= REC_CU && l < REC_CU + 12) ? CertNode::d + l - REC_CU : -1;
#define HB_CERT_FETCH(kk)                                                                                                         \
  {                                                                                                                               \
    const d2* pab_ = reinterpret_cast<const d2*>(b.recs + (size_t(inst) * b.Nmax + (kk)) * REC_SIZE + REC_AB) + l;                \
    _Pragma("unroll") for (int r = 0; r < N_AB; ++r) bab[r] = (64 * r + 63 < P_AB || l + 64 * r < P_AB) ? pab_[64 * r] : d2{0.0, 0.0}; \
    cdv = cd_off >= 0 ? nodes[size_t(kk) * CertNode::size + cd_off] : 0.0;                                                       \
  }
    if (n > 0) HB_CERT_FETCH(n - 1);
    for (int k = n - 1; k >= 0; --k) {
      {
        d2* sab = reinterpret_cast<d2*>(lds + CertSweepLds::AB) + l;
#pragma unroll
        for (int r = 0; r < N_AB; ++r) if (64 * r + 63 < P_AB || l + 64 * r < P_AB) sab[64 * r] = bab[r];
      }
      const double cdk = cdv;
      cx.sync();
      if (k > 0) HB_CERT_FETCH(k - 1);
      mpc_cert_sweep_stage(cx, lds, [cdk](int) { return cdk; }, costate + size_t(k) * HB_NX);
    }
#undef HB_CERT_FETCH
  }
  mpc_cert_finish(cx, lds, nodes, certified ? n : 0, certified, cb.cert + size_t(inst) * MPC_CERT_SIZE);
}

// line search: value of trial point (x + alpha dx, u + alpha du), one thread per node
__global__ __launch_bounds__(64) void k_ls_eval(Batch b, const DevModel* __restrict__ M, const DevConfig* __restrict__ C,
                                                double alpha) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int inst = gid / b.Nmax, k = gid % b.Nmax;
  if (inst >= b.B) return;
  if (b.accepted[inst] || k >= b.n_nodes[inst]) return;
  const size_t nd = size_t(inst) * b.Nmax + k;
  const size_t xo = (size_t(inst) * (b.Nmax + 1) + k) * HB_NX;
  // trial point in LDS (stride 45: conflict-free per half-wave): thread-private arrays would be indexed by the rolled
  // joint loops of the model and live in scratch.  The next node's trial state is only read once per entry (defect) and
  // is formed from global memory there: 34 -> 23 KB per block, 4 -> 6 blocks per CU for this latency-bound kernel.
  __shared__ double tp[64 * 45];
  double* x = tp + threadIdx.x * 45;
  double* u = x + HB_NX;
#pragma unroll
  for (int i = 0; i < HB_NX; ++i) {
    x[i] = b.x[xo + i] + alpha * b.dx[xo + i];
    u[i] = b.u[nd * HB_NU + i] + alpha * b.du[nd * HB_NU + i];
  }
  const double* tt = b.t + size_t(inst) * (b.Nmax + 1);
  const double* xn0 = b.x + xo + HB_NX;
  const double* dxn = b.dx + xo + HB_NX;
  double o3[3];
  node_value(*M, *C, x, u, [xn0, dxn, alpha](int i) { return xn0[i] + alpha * dxn[i]; }, b.xref + nd * HB_NX, b.swing + nd * 24,
             tt[k + 1] - tt[k], b.mode[nd], o3);
  b.partial[nd * 3 + 0] = o3[0];
  b.partial[nd * 3 + 1] = o3[1];
  b.partial[nd * 3 + 2] = o3[2];
}

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return __shfl(v, 0, 64);
}

__global__ __launch_bounds__(64) void k_ls_decide(Batch b, const DevConfig* __restrict__ C, double alpha) {
  const int inst = blockIdx.x, lane = threadIdx.x;
  if (b.accepted[inst]) return;
  const int n = b.n_nodes[inst];
  double m = 0, d = 0, e = 0;
  for (int k = lane; k < n; k += 64) {
    const double* p = b.partial + (size_t(inst) * b.Nmax + k) * 3;
    m += p[0];
    d += p[1];
    e += p[2];
  }
  m = wave_sum(m);
  d = wave_sum(d);
  e = wave_sum(e);
  const double armijo = b.acc[inst * 4 + 0], base_merit = b.acc[inst * 4 + 1];
  const double base_viol = sqrt(b.acc[inst * 4 + 2] + b.acc[inst * 4 + 3]);
  const bool ok = filter_accept(*C, base_merit, base_viol, m, sqrt(d + e), alpha, armijo) && !b.ric_fail[inst];
  const size_t xo = size_t(inst) * (b.Nmax + 1) * HB_NX, uo = size_t(inst) * b.Nmax * HB_NU;
  if (!ok) {
    // refused: the backtracking tail follows.  It needs |dx|, |du| over the whole trajectory (the search gives up once alpha |dx| and
    // alpha |du| are both below sqp.deltaTol, [OCS2-knowledge] SqpSolver::takeStep "escape early") before it evaluates anything
    double nx2 = 0, nu2 = 0;
    for (int i = lane; i < (n + 1) * HB_NX; i += 64) nx2 += b.dx[xo + i] * b.dx[xo + i];
    for (int i = lane; i < n * HB_NU; i += 64) nu2 += b.du[uo + i] * b.du[uo + i];
    nx2 = wave_sum(nx2);
    nu2 = wave_sum(nu2);
    if (lane == 0) { b.ls_norm[inst * 2] = sqrt(nx2); b.ls_norm[inst * 2 + 1] = sqrt(nu2); }
    return;
  }
  // commit the step
  for (int i = lane; i < (n + 1) * HB_NX; i += 64) b.x[xo + i] += alpha * b.dx[xo + i];
  for (int i = lane; i < n * HB_NU; i += 64) b.u[uo + i] += alpha * b.du[uo + i];
  if (lane == 0) {
    b.accepted[inst] = 1;
    b.perf[inst * 4 + 0] = m;
    b.perf[inst * 4 + 1] = d;
    b.perf[inst * 4 + 2] = e;
    b.perf[inst * 4 + 3] = alpha;
  }
}

// Backtracking tail of the filter line search.  An instance that did not accept the full step tries alpha0, alpha0 * decay, ...
// >= alpha_min in that order and takes the first one the filter accepts (OCS2 FilterLinesearch); before every trial it gives up — no
// step, converged — once alpha |dx| and alpha |du| are both below sqp.deltaTol.  The trials do not depend on each other, so they are
// EVALUATED SIDE BY SIDE (k_ls_tail_eval: k_ls_eval once per step size, thread = node, per-node partials; the same node evaluation
// and the same summation order as k_ls_eval + k_ls_decide) and a second kernel walks the sequence with exactly the sequential rules (k_ls_tail_decide):
// identical decisions, but the launch takes ONE trial's time instead of up to 13 in a row (an instance that walks down to
// alpha_min used to hold the whole batch back: 2.4 ms of line search per step in the backtracking figure), and without the loop over
// the step sizes around the node evaluation the kernel no longer spills (the one-launch form carried 476 B / lane of scratch).
// Instances that accepted alpha = 1 — all of them in steady state — leave at once.
__global__ __launch_bounds__(64) void k_ls_tail_eval(Batch b, const DevModel* __restrict__ M, const DevConfig* __restrict__ C, double alpha0,
                                                     double decay, double alpha_min) {
  // (k_ls_eval with the step size of blockIdx.y; one node per thread and no loop around the node evaluation: no scratch)
  const int gid = blockIdx.x * blockDim.x + threadIdx.x, ai = blockIdx.y;
  const int inst = gid / b.Nmax, k = gid % b.Nmax;
  if (inst >= b.B) return;
  if (b.accepted[inst] || k >= b.n_nodes[inst]) return;
  double alpha = alpha0;
  for (int j = 0; j < ai; ++j) alpha *= decay;   // (the sequential search multiplies step by step: the same rounding)
  if (!(alpha >= alpha_min)) return;
  // step sizes the sequential search never reaches are not evaluated: it stops (no step) at the first alpha with alpha |dx| and
  // alpha |du| below deltaTol, and the condition is monotone in alpha — a converged instance evaluates nothing, as before
  if (alpha * b.ls_norm[inst * 2 + 1] < C->delta_tol && alpha * b.ls_norm[inst * 2] < C->delta_tol) return;
  const size_t nd = size_t(inst) * b.Nmax + k;
  const size_t xo = (size_t(inst) * (b.Nmax + 1) + k) * HB_NX;
  __shared__ double tp[64 * 45];
  double* x = tp + threadIdx.x * 45;
  double* u = x + HB_NX;
#pragma unroll
  for (int i = 0; i < HB_NX; ++i) {
    x[i] = b.x[xo + i] + alpha * b.dx[xo + i];
    u[i] = b.u[nd * HB_NU + i] + alpha * b.du[nd * HB_NU + i];
  }
  const double* tt = b.t + size_t(inst) * (b.Nmax + 1);
  const double* xn0 = b.x + xo + HB_NX;
  const double* dxn = b.dx + xo + HB_NX;
  double o3[3];
  node_value(*M, *C, x, u, [xn0, dxn, alpha](int i) { return xn0[i] + alpha * dxn[i]; }, b.xref + nd * HB_NX, b.swing + nd * 24,
             tt[k + 1] - tt[k], b.mode[nd], o3);
  double* o = b.ls_tail + ((size_t(inst) * LS_TAIL_MAX + ai) * b.Nmax + k) * 3;
  o[0] = o3[0];
  o[1] = o3[1];
  o[2] = o3[2];
}
__global__ __launch_bounds__(64) void k_ls_tail_decide(Batch b, const DevConfig* __restrict__ C, double alpha0, double decay, double alpha_min,
                                                       int n_alpha) {
  const int inst = blockIdx.x, lane = threadIdx.x;
  if (b.accepted[inst]) return;
  const int n = b.n_nodes[inst];
  const double armijo = b.acc[inst * 4 + 0], base_merit = b.acc[inst * 4 + 1];
  const double base_viol = sqrt(b.acc[inst * 4 + 2] + b.acc[inst * 4 + 3]);
  const bool ric_ok = !b.ric_fail[inst];
  // no step once alpha |dx| and alpha |du| are both below sqp.deltaTol — like reaching alpha_min, but the instance is converged, not
  // failed (accepted = 2 -> HB_INST_OK); the norms were left by k_ls_decide when it refused the full step
  const size_t xo = size_t(inst) * (b.Nmax + 1) * HB_NX, uo = size_t(inst) * b.Nmax * HB_NU;
  const double dx_norm = b.ls_norm[inst * 2], du_norm = b.ls_norm[inst * 2 + 1], delta_tol = C->delta_tol;
  double alpha = alpha0;
  for (int ai = 0; ai < n_alpha && alpha >= alpha_min; ++ai, alpha *= decay) {
    if (alpha * du_norm < delta_tol && alpha * dx_norm < delta_tol) {
      if (lane == 0) b.accepted[inst] = 2;
      return;
    }
    // (the sums of k_ls_decide, in its order: per-lane partial sums over the lane's nodes, then the wave reduction)
    double m = 0, d = 0, e = 0;
    for (int k = lane; k < n; k += 64) {
      const double* p = b.ls_tail + ((size_t(inst) * LS_TAIL_MAX + ai) * b.Nmax + k) * 3;
      m += p[0];
      d += p[1];
      e += p[2];
    }
    m = wave_sum(m);
    d = wave_sum(d);
    e = wave_sum(e);
    if (filter_accept(*C, base_merit, base_viol, m, sqrt(d + e), alpha, armijo) && ric_ok) {
      for (int i = lane; i < (n + 1) * HB_NX; i += 64) b.x[xo + i] += alpha * b.dx[xo + i];
      for (int i = lane; i < n * HB_NU; i += 64) b.u[uo + i] += alpha * b.du[uo + i];
      if (lane == 0) {
        b.accepted[inst] = 1;
        b.perf[inst * 4 + 0] = m;
        b.perf[inst * 4 + 1] = d;
        b.perf[inst * 4 + 2] = e;
        b.perf[inst * 4 + 3] = alpha;
      }
      return;
    }
  }
}

// ---- unit-level kernels -----------------------------------------------------------------------------------
__global__ void k_flow_map(int n, const DevModel* __restrict__ M, const double* x, const double* u, double* f,
                           double* pos, double* vel) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double xl[HB_NX], ul[HB_NU], fl[HB_NX];
  for (int c = 0; c < HB_NX; ++c) { xl[c] = x[i * HB_NX + c]; ul[c] = u[i * HB_NU + c]; }
  Centroidal<double> c;
  flow_map<double>(*M, xl, ul, fl, &c);
  if (f) for (int r = 0; r < HB_NX; ++r) f[i * HB_NX + r] = fl[r];
  for (int k = 0; k < HB_NC; ++k) {
    if (pos) { pos[(i * 4 + k) * 3] = xl[6] + c.foot_rel[k].x; pos[(i * 4 + k) * 3 + 1] = xl[7] + c.foot_rel[k].y; pos[(i * 4 + k) * 3 + 2] = xl[8] + c.foot_rel[k].z; }
    if (vel) { vel[(i * 4 + k) * 3] = c.foot_vel[k].x; vel[(i * 4 + k) * 3 + 1] = c.foot_vel[k].y; vel[(i * 4 + k) * 3 + 2] = c.foot_vel[k].z; }
  }
}
// one 64-lane block per sample, lane = direction
__global__ __launch_bounds__(64) void k_flow_jac(const DevModel* __restrict__ M, const double* x, const double* u, double* dfdx,
                                                 double* dfdu) {
  const int i = blockIdx.x, dir = threadIdx.x;
  if (dir >= 44) return;
  Dual1 xd[HB_NX], ud[HB_NU], fd[HB_NX];
  for (int c = 0; c < HB_NX; ++c) {
    xd[c] = Dual1(x[i * HB_NX + c], dir == c ? 1.0 : 0.0);
    ud[c] = Dual1(u[i * HB_NU + c], dir == HB_NX + c ? 1.0 : 0.0);
  }
  Centroidal<Dual1> ce;
  flow_map<Dual1>(*M, xd, ud, fd, &ce);
  double* dst = (dir < HB_NX) ? dfdx : dfdu;
  const int col = (dir < HB_NX) ? dir : dir - HB_NX;
  if (dst)
    for (int r = 0; r < HB_NX; ++r) dst[(size_t(i) * HB_NX + r) * HB_NX + col] = fd[r].d;
}

__global__ void k_centroidal_state(int n, const DevModel* __restrict__ M, const double* rbd, double* x) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) centroidal_state_from_rbd(*M, rbd + size_t(i) * HB_NRBD, x + size_t(i) * HB_NX);
}

// ---- plant stub: one wave per instance -----------------------------------------------------------------------------
struct PlantBatch {
  int B;
  double *q, *v, *anchor;  // [B][16], [B][16], [B][12]
  int* pinned;             // [B][4]
  double *lambda, *vdot;   // [B][12], [B][16]
  double* tau;             // [B][10] staging of host torques
  int* contact;            // [B][4] staging of host contact flags
  double* rbd;             // [B][32] repacked state
  double baum, eps;
  // what the last step applied (hb_plant_sense reads them; zero torque / all flags 1 before the first step)
  double* tau_last;        // [B][10]
  int* contact_last;       // [B][4]
  // sensor arrays of hb_plant_sense: quat, gyro, accel, joint pos / vel / torque [B][4|3|3|10|10|10], contact flags [B][4]
  double *s_quat, *s_gyro, *s_accel, *s_jp, *s_jv, *s_jt;
  int* s_contact;
  double *gyro_bias, *accel_bias;  // [B][3] each, or null (hb_plant_set_sensor_model)
};

__global__ __launch_bounds__(64) void k_plant(PlantBatch p, const DevModel* __restrict__ M, const double* tau, const int* contact,
                                               const int* mode, double dt, int substeps, double* res_rbd, double* res_x0,
                                               double* res_t) {
  const int i = blockIdx.x;
  __shared__ double lds[PLANT_LDS_TOTAL];
  __shared__ int cflag[HB_NC];
  const DeviceCtx cx;
  if (cx.lane < HB_NC) {
    if (contact) cflag[cx.lane] = contact[4 * i + cx.lane];
    else { bool cf[HB_NC]; mode_flags(mode[i], cf); cflag[cx.lane] = cf[cx.lane] ? 1 : 0; }
  }
  __syncthreads();
  if (cx.lane < HB_NJ) p.tau_last[10 * i + cx.lane] = tau[10 * i + cx.lane];
  if (cx.lane < HB_NC) p.contact_last[4 * i + cx.lane] = cflag[cx.lane];
  plant_step(cx, *M, p.q + 16 * i, p.v + 16 * i, p.anchor + 12 * i, p.pinned + 4 * i, tau + 10 * i, cflag, p.baum, p.eps, dt, substeps, lds,
             p.lambda + 12 * i, p.vdot + 16 * i);
  if (cx.lane == 0) {
    const double* q = p.q + 16 * i;
    const double* v = p.v + 16 * i;
    double* rbd = p.rbd + HB_NRBD * i;
    double sz, cz, sy, cy;
    sincos_t(q[3], sz, cz);
    sincos_t(q[4], sy, cy);
    for (int a = 0; a < 3; ++a) { rbd[a] = q[3 + a]; rbd[3 + a] = q[a]; rbd[HB_NV + 3 + a] = v[a]; }
    for (int j = 0; j < HB_NJ; ++j) { rbd[6 + j] = q[6 + j]; rbd[6 + HB_NV + j] = v[6 + j]; }
    // omega_world = E(zyx) rates
    rbd[HB_NV + 0] = -sz * v[4] + cy * cz * v[5];
    rbd[HB_NV + 1] = cz * v[4] + cy * sz * v[5];
    rbd[HB_NV + 2] = v[3] - sy * v[5];
    if (res_rbd) {
      for (int c = 0; c < HB_NRBD; ++c) res_rbd[HB_NRBD * i + c] = rbd[c];
      centroidal_state_from_rbd(*M, rbd, res_x0 + HB_NX * i);
      res_t[i] += dt;
    }
  }
}
__global__ void k_plant_reset(PlantBatch p, const DevModel* __restrict__ M) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.B) return;
  plant_feet(*M, p.q + 16 * i, p.anchor + 12 * i);
  for (int c = 0; c < HB_NC; ++c) { p.pinned[4 * i + c] = 0; p.contact_last[4 * i + c] = 1; }
  for (int a = 0; a < 16; ++a) p.vdot[16 * i + a] = 0.0;
  for (int a = 0; a < 12; ++a) p.lambda[12 * i + a] = 0.0;
  for (int j = 0; j < HB_NJ; ++j) p.tau_last[10 * i + j] = 0.0;
}

// ---- sensors from the plant: one thread per instance, 64 instances per workgroup ---------------------------------------------------
// The per-instance routine (hb_sensors.hpp plant_sense) reads and writes LDS rows; the workgroup moves its 64 instances' inputs and
// outputs between LDS and global memory array by array, consecutive lanes on consecutive words (the arrays are instance-major, so a
// workgroup's slice of each is one contiguous run) — a thread storing its own 10 doubles would stride the lanes 80 bytes apart.
constexpr int kSenseThreads = 64;
constexpr int kSenseIn = 16 + 16 + 3 + 10 + 3 + 3;   // q | v | vdot[0:3] | tau | gyro bias | accel bias
constexpr int kSenseOut = 4 + 3 + 3 + 10 + 10 + 10;  // quat | gyro | accel | joint pos | vel | torque
constexpr int kSenseRow = kSenseIn + kSenseOut;      // 91 doubles: an odd row length, the lanes' rows start in different LDS banks
static_assert(kSenseRow % 2 == 1, "keep the LDS row length odd");
__global__ __launch_bounds__(kSenseThreads) void k_plant_sense(PlantBatch p, const DevModel* __restrict__ M, hb_sensor_config K, int noisy,
                                                               unsigned long long count) {
  __shared__ double row[kSenseThreads * kSenseRow];
  __shared__ int cfl[kSenseThreads * HB_NC];
  const int i0 = blockIdx.x * kSenseThreads, n = min(kSenseThreads, p.B - i0), lane = threadIdx.x;
  // per-instance width w of a global array at `src`, to / from LDS column `col`
  auto load = [&](const double* src, int w, int col) {
    for (int e = lane; e < n * w; e += kSenseThreads) row[(e / w) * kSenseRow + col + e % w] = src[size_t(i0) * w + e];
  };
  auto store = [&](double* dst, int w, int col) {
    for (int e = lane; e < n * w; e += kSenseThreads) dst[size_t(i0) * w + e] = row[(e / w) * kSenseRow + col + e % w];
  };
  load(p.q, 16, 0);
  load(p.v, 16, 16);
  for (int e = lane; e < n * 3; e += kSenseThreads) row[(e / 3) * kSenseRow + 32 + e % 3] = p.vdot[size_t(i0 + e / 3) * 16 + e % 3];
  load(p.tau_last, 10, 35);
  if (p.gyro_bias) load(p.gyro_bias, 3, 45);
  if (p.accel_bias) load(p.accel_bias, 3, 48);
  for (int e = lane; e < n * HB_NC; e += kSenseThreads) cfl[e] = p.contact_last[size_t(i0) * HB_NC + e];
  __syncthreads();
  if (lane < n) {
    double* r = row + lane * kSenseRow;
    double* o = r + kSenseIn;
    const SenseOut out{o, o + 4, o + 7, o + 10, o + 20, o + 30, cfl + lane * HB_NC};  // (the flags pass through in place)
    plant_sense(M->gravity, r, r + 16, r + 32, r + 35, cfl + lane * HB_NC, K, noisy != 0, p.gyro_bias ? r + 45 : nullptr,
                p.accel_bias ? r + 48 : nullptr, K.instance_offset + uint32_t(i0 + lane), count, out);
  }
  __syncthreads();
  store(p.s_quat, 4, kSenseIn);
  store(p.s_gyro, 3, kSenseIn + 4);
  store(p.s_accel, 3, kSenseIn + 7);
  store(p.s_jp, 10, kSenseIn + 10);
  store(p.s_jv, 10, kSenseIn + 20);
  store(p.s_jt, 10, kSenseIn + 30);
  for (int e = lane; e < n * HB_NC; e += kSenseThreads) p.s_contact[size_t(i0) * HB_NC + e] = cfl[e];
}

// ---- joint command law: one thread per instance, joints in the reference's order -----------------------------------
// LeggedController.cpp:186-256 incl. the limit protection (:196-208: a joint more than 0.02 rad outside its urdf limits
// latches emergencyStopFlag_ — only while the controller is loaded — and from THAT joint on, and on every later tick, the
// command is setCommand(0, 0, 0, 1, 0), :245-248) and the unloaded-controller branch (:209-221: MPC joint targets with the
// position gains, no feed-forward).  estop / loaded are per-instance device state (hb_joint_set_flags).
__global__ void k_joint_command(WbcBatch w, const DevModel* __restrict__ M, hb_joint_gains g, double dt, int* estop, const int* loaded,
                                double* out /*[6][B][10]: posDes velDes kp kd ff torque*/) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w.B) return;
  bool cf[HB_NC];
  mode_flags(w.mode[i], cf);
  bool stop = estop[i] != 0;
  const bool is_loaded = loaded[i] != 0;
  const size_t n = size_t(w.B) * HB_NJ;
  for (int j = 0; j < HB_NJ; ++j) {
    const double q = w.rbd[size_t(i) * HB_NRBD + 6 + j], qd = w.rbd[size_t(i) * HB_NRBD + 6 + HB_NV + j];
    if (!stop && is_loaded && (q > M->q_upper[j] + 0.02 || q < M->q_lower[j] - 0.02)) stop = true;
    const int k = j < 5 ? j : j - 5;
    double pos, vel, kp, kd, ff;
    if (!is_loaded) {
      pos = w.xdes[size_t(i) * HB_NX + 12 + j];
      vel = w.udes[size_t(i) * HB_NU + 12 + j];
      kp = g.kp_position;
      kd = k == 4 ? g.kd_feet : g.kd_position;
      ff = 0.0;
    } else {
      const double qdd = w.sol[size_t(i) * HB_NWBC + 6 + j];
      ff = w.sol[size_t(i) * HB_NWBC + 28 + j];
      pos = w.xdes[size_t(i) * HB_NX + 12 + j] + 0.5 * qdd * dt * dt;
      vel = w.udes[size_t(i) * HB_NU + 12 + j] + qdd * dt;
      const bool contact = j < 5 ? cf[0] : cf[1];  // cmdContactFlag[int(j / 5)]
      if (k == 0 || k == 1) { kp = contact ? g.kp_small_stance : g.kp_small_swing; kd = g.kd_small; }
      else if (k == 4) { kp = contact ? g.kp_small_stance : g.kp_small_swing; kd = g.kd_feet; }
      else { kp = contact ? g.kp_big_stance : g.kp_big_swing; kd = g.kd_big; }
    }
    if (stop) { pos = 0.0; vel = 0.0; kp = 0.0; kd = 1.0; ff = 0.0; }
    const size_t gid = size_t(i) * HB_NJ + j;
    out[gid] = pos;
    out[n + gid] = vel;
    out[2 * n + gid] = kp;
    out[3 * n + gid] = kd;
    out[4 * n + gid] = ff;
    out[5 * n + gid] = ff + kp * (pos - q) + kd * (vel - qd);
  }
  estop[i] = stop ? 1 : 0;
}

// ---- reference generation: one thread per instance -------------------------------------------------------------
struct RefgenBatch {
  int B;
  int* n_ev;        // [B]
  double* ev;       // [B][HB_MAX_EVENTS]
  int* modes;       // [B][HB_MAX_EVENTS + 1]
  double* stance;   // [B][4][3]
  double* phases;   // [B][4][HB_MAX_EVENTS + 1][RG_PHASE]
  double* t0;       // [B]
  double* cmd;      // [B][4]
  int* status;      // [B]
  int* n_knots;     // [B]
  double* knot_t;   // [B][RG_MAX_KNOTS]
  double* knot_x;   // [B][RG_MAX_KNOTS][22]
  int init_stance;  // take the current feet as latest stance positions (first update after a reset without state)
};

// gait manager (hb_gait.hpp), ahead of k_refgen when it is enabled: one thread per instance.  Reads the observation, the time and the
// uploaded command of the pass; writes the window into the planner's schedule rows and the filtered command into the gait state.
__global__ __launch_bounds__(64) void k_gait(Batch b, RefgenBatch r, GaitBatch g, hb_gait_config K, double horizon) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.B) return;
  gait_pass(g, i, K, r.t0[i], horizon, b.x0 + size_t(i) * HB_NX, r.cmd + size_t(i) * 4, r.n_ev + i, r.ev + size_t(i) * HB_MAX_EVENTS,
            r.modes + size_t(i) * (HB_MAX_EVENTS + 1));
}
__global__ __launch_bounds__(64) void k_gait_reset(GaitBatch g, hb_gait_config K, const unsigned char* __restrict__ mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.B || (mask && !mask[i])) return;
  gait_reset_instance(g, i, K);
}
// hb_gait_insert_template: g is the view of the addressed instances
__global__ __launch_bounds__(64) void k_gait_insert(GaitBatch g, double pts, int n_switch, const double* __restrict__ sw, const int* __restrict__ modes,
                                                    const double* __restrict__ start, const double* __restrict__ final_time) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.B) return;
  gait_insert_template(g, i, pts, n_switch, sw, modes, start[i], final_time[i]);
}

// planner step: FOUR lanes per instance, one per foot (refgen_plan: the four planner loops and the leg evaluations side by side; the lane
// of foot 0 finishes with the shooting grid and the knots) — thread-per-instance the kernel was a 0.26 ms chain on 64 wavefronts
__global__ __launch_bounds__(64) void k_refgen(Batch b, RefgenBatch r, const DevModel* __restrict__ M, hb_refgen_config K, double horizon) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = gid >> 2, foot = gid & 3;
  if (i >= b.B) return;   // (a whole group of four leaves together)
  const double* x_now = b.x0 + size_t(i) * HB_NX;
  double* stance = r.stance + size_t(i) * 12;
  if (r.init_stance) {
    const Mat3<double> R0 = rg_rot_zyx(x_now + 9);
    const Vec3<double> p0(x_now[6], x_now[7], x_now[8]);
    const double* qj = x_now + 12;
    LegOut<double> L;
    leg_eval<double>(*M, foot & 1, [qj](int j) { return qj[j]; }, [](int) { return 0.0; }, L);
    st3(stance + 3 * foot, p0 + R0 * ((foot >> 1) ? L.foot[1] : L.foot[0]));
  }
  const size_t N = b.Nmax;
  const int st = refgen_plan(*M, K, r.n_ev[i], r.ev + size_t(i) * HB_MAX_EVENTS, r.modes + size_t(i) * (HB_MAX_EVENTS + 1), r.t0[i], horizon, x_now,
                             r.cmd + size_t(i) * 4, stance, r.phases + size_t(i) * 4 * (HB_MAX_EVENTS + 1) * RG_PHASE, b.Nmax, b.n_nodes + i,
                             b.t + size_t(i) * (N + 1), r.n_knots + i, r.knot_t + size_t(i) * RG_MAX_KNOTS,
                             r.knot_x + size_t(i) * RG_MAX_KNOTS * HB_NX, foot, 4);
  // status of the instance: 2 (grid too long, from the lane of foot 0) wins, else 1 if any foot reported a phase without its events
  int any = st == 1 ? 1 : 0;
  any |= __shfl_xor(any, 1, 64);
  any |= __shfl_xor(any, 2, 64);
  if (foot == 0) r.status[i] = st == 2 ? 2 : any;
}
// joint-reference IK: eight lanes per (instance, leg), eight pairs per wavefront (hb_refgen.hpp refgen_ik_group)
__global__ __launch_bounds__(64) void k_refgen_ik(Batch b, RefgenBatch r, const DevModel* __restrict__ M, hb_refgen_config K, double horizon) {
#if defined(__HIP_DEVICE_COMPILE__)  // (the routine is built from cross-lane instructions: device pass only)
  const int gid = blockIdx.x * 8 + (threadIdx.x >> 3);
  const bool valid = gid < 2 * b.B;
  const int i = valid ? gid >> 1 : 0, leg = gid & 1;
  refgen_ik_group(*M, K, valid, r.n_ev[i], r.ev + size_t(i) * HB_MAX_EVENTS, r.t0[i], horizon, b.x0 + size_t(i) * HB_NX,
                  r.phases + size_t(i) * 4 * (HB_MAX_EVENTS + 1) * RG_PHASE, r.n_knots[i], r.knot_t + size_t(i) * RG_MAX_KNOTS,
                  r.knot_x + size_t(i) * RG_MAX_KNOTS * HB_NX, leg);
#endif
}
// test hook (hb_ik_solve): n independent InverseKinematics::computeIK problems, eight lanes each
__global__ __launch_bounds__(64) void k_ik_solve(int n, const DevModel* __restrict__ M, const double* __restrict__ q16, const int* __restrict__ leg,
                                                 const double* __restrict__ des, const double* __restrict__ Rdes, double* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int gid = blockIdx.x * 8 + (threadIdx.x >> 3);
  const int p = gid < n ? gid : 0;
  IkLane L;
  ik_lane_setup(*M, leg[p], L);
  const double* q = q16 + size_t(p) * HB_NV;
  const Mat3<double> R0 = rg_rot_zyx(q + 3);
  Mat3<double> Rd;
  for (int e = 0; e < 9; ++e) Rd.m[e] = Rdes[size_t(p) * 9 + e];
  double qk = q[6 + 5 * leg[p] + (L.joint ? L.k : 0)];
  ik_solve(L, R0, Vec3<double>(q[0], q[1], q[2]), Vec3<double>(des[3 * p], des[3 * p + 1], des[3 * p + 2]), Rd, qk);
  if (gid < n && L.joint) out[size_t(p) * 5 + L.k] = qk;
#endif
}
// node tables: one thread per (instance, node), consecutive lanes = consecutive nodes.  A thread's 22 + 24 values go to LDS and the
// wavefront writes them out in memory order (the rows of 64 consecutive nodes are one contiguous block of xref and one of swing): written
// by their own threads, every store instruction touched 64 cache lines and the kernel ran at the speed of its uncoalesced stores.
__global__ __launch_bounds__(64) void k_refgen_nodes(Batch b, RefgenBatch r, hb_refgen_config K) {
  constexpr int NS = HB_NC * HB_SWING_REF, LDT = HB_NX + NS + 1;   // 22 + 24 (+ 1: the rows of two lanes start in different banks)
  static_assert(NS == 24, "swing block of a node");
  __shared__ double stage[64 * LDT];
  const int gid0 = blockIdx.x * blockDim.x, lane = threadIdx.x, gid = gid0 + lane;
  const int total = b.B * b.Nmax;
  if (gid < total) {
    const int i = gid / b.Nmax, k = gid - i * b.Nmax;
    const size_t N = b.Nmax;
    refgen_node(K, r.n_ev[i], r.ev + size_t(i) * HB_MAX_EVENTS, r.modes + size_t(i) * (HB_MAX_EVENTS + 1), r.n_knots[i],
                r.knot_t + size_t(i) * RG_MAX_KNOTS, r.knot_x + size_t(i) * RG_MAX_KNOTS * HB_NX,
                r.phases + size_t(i) * 4 * (HB_MAX_EVENTS + 1) * RG_PHASE, k, b.n_nodes[i], b.t[size_t(i) * (N + 1) + k], b.mode + gid,
                stage + lane * LDT, stage + lane * LDT + HB_NX);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int nn = total - gid0 < 64 ? total - gid0 : 64;   // nodes of this wavefront
  double* xo = b.xref + size_t(gid0) * HB_NX;
  double* so = b.swing + size_t(gid0) * NS;
  for (int e = lane; e < nn * HB_NX; e += 64) {
    const int nd = e / HB_NX, c = e - nd * HB_NX;
    xo[e] = stage[nd * LDT + c];
  }
  for (int e = lane; e < nn * NS; e += 64) {
    const int nd = e / NS, c = e - nd * NS;
    so[e] = stage[nd * LDT + HB_NX + c];
  }
}

// ---- state estimator: one wave per instance ----------------------------------------------------------------------
struct EstBatch {
  int B;
  double *xhat, *P, *yaw_last;                       // filter state [B][18], [B][18][18], [B]
  const double *quat, *w_local, *a_local, *qj, *qdj;  // inputs [B][4|3|3|10|10]
  const int* contact;                                 // [B][4]
  double *rbd, *x;                                    // outputs [B][32], [B][22]
  double *res_rbd, *res_x0;                           // resident inputs of hb_step_resident (or null)
  // hb_estimator_contact_force: low-pass state pSCgZinvlast_ [B][16], joint efforts [B][10], outputs [B][16] each, a host-given rbd [B][32]
  double *cf_z, *cf_tau, *cf_dist, *cf_out, *cf_rbd;
};

__global__ __launch_bounds__(64) void k_estimator(EstBatch e, const DevModel* __restrict__ M, hb_estimator_config K, double dt) {
  const int i = blockIdx.x;
  __shared__ double lds[EstLds::total];
  const DeviceCtx cx;
  const EstIn in{e.quat + 4 * i, e.w_local + 3 * i, e.a_local + 3 * i, e.qj + 10 * i, e.qdj + 10 * i, e.contact + 4 * i};
  estimator_update(cx, *M, K, dt, in, e.xhat + 18 * i, e.P + 324 * size_t(i), e.yaw_last + i, lds, e.rbd + HB_NRBD * i, e.x + HB_NX * i);
  if (e.res_rbd) {
    __syncthreads();  // lane 0 wrote the outputs
    for (int c = cx.lane; c < HB_NRBD; c += 64) e.res_rbd[HB_NRBD * i + c] = e.rbd[HB_NRBD * i + c];
    for (int c = cx.lane; c < HB_NX; c += 64) e.res_x0[HB_NX * i + c] = e.x[HB_NX * i + c];
  }
}
// StateEstimateBase::estContactForce for every instance, one thread each (hb_estimator.hpp contact_force_estimate); the per-leg forward
// data sits in LDS (the joint loops index it dynamically).  Not on the timed path of the update: 4096 instances take ~ 0.1 ms.
constexpr int kCfThreads = 32;
__global__ __launch_bounds__(kCfThreads) void k_contact_force(int B, const DevModel* __restrict__ M, double gama, double beta, const double* rbd,
                                                              const double* tau, double* z, double* dist, double* cf) {
  static_assert(sizeof(CfLegWork) % 8 == 0, "CfLegWork is an array of doubles");
  __shared__ double wk_raw[kCfThreads * (sizeof(CfLegWork) / 8)];   // (Vec3 has a constructor: raw storage, never read before it is written)
  const int i = blockIdx.x * kCfThreads + threadIdx.x;
  if (i >= B) return;
  contact_force_estimate(*M, gama, beta, rbd + size_t(i) * HB_NRBD, tau + size_t(i) * HB_NJ, z + size_t(i) * HB_NV, dist + size_t(i) * HB_NV,
                         cf + size_t(i) * 16, *reinterpret_cast<CfLegWork*>(wk_raw + threadIdx.x * (sizeof(CfLegWork) / 8)));
}
__global__ void k_estimator_reset(int B, double* xhat, double* P, double* yaw_last, const double* xhat0) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * 324) return;
  const int i = idx / 324, e = idx - 324 * i, r = e / 18, c = e - 18 * r;
  P[idx] = r == c ? 100.0 : 0.0;  // LinearKalmanFilter.cpp:56-57
  if (e < 18) xhat[18 * i + e] = xhat0 ? xhat0[18 * i + e] : 0.0;
  if (e == 0) yaw_last[i] = 0.0;
}

}  // namespace

// ===========================================================================================================
// host side
// ===========================================================================================================
// Error text of the last failed call, per calling thread (errno-like): the reference drives one solver from two threads
// (control thread / MPC thread, LeggedController.cpp:396-421) and each reads back only its own failures.
struct ErrSlot {
  static std::string& tl() { static thread_local std::string s; return s; }
  ErrSlot& operator=(const std::string& m) { tl() = m; return *this; }
  ErrSlot& operator=(const char* m) { tl() = m; return *this; }
  const char* c_str() const { return tl().c_str(); }
};

// Slots of hb_ctx::ev: timing points of the MPC phases (iteration 0 of a whole-batch solve) and of the WBC, then the policy
// hand-over: published, and consumed by the last policy evaluation.
enum EvSlot { EV_LQ_BEGIN, EV_LQ_END, EV_RIC_BWD_END, EV_RIC_FWD_END, EV_LS_END, EV_WBC_BEGIN, EV_WBC_END, EV_PUBLISHED, EV_POLICY_READ, EV_COUNT };
constexpr int kMaxRanges = 8;  // instance ranges (hb_set_chunks), each on a stream of its own
// Slots of hb_ctx::ev_sync, cross-stream ordering points that are NOT timing events: a resident-input writer (plant, estimator) waits
// for the MPC stream / the MPC stream for it; fork of the range streams from the MPC / WBC streams; SYNC_JOIN + c: join of range c.
enum SyncSlot { SYNC_BEFORE_WRITER, SYNC_AFTER_WRITER, SYNC_FORK_MPC, SYNC_FORK_WBC, SYNC_JOIN, SYNC_COUNT = SYNC_JOIN + kMaxRanges };

struct hb_ctx {
  int device = 0, B = 0, Nmax = 0, n_cu = 256;
  // Guards the host-side state both threads touch while ENQUEUEING work (policy hand-over flags, counters); never held across
  // a device synchronisation.
  std::mutex mtx;
  hb_model model;
  hb_config config;
  DevModel hmodel;
  DevConfig hconfig;
  DevModel* dmodel = nullptr;
  DevConfig* dconfig = nullptr;
  Batch b{};
  hipStream_t s_mpc = nullptr, s_wbc = nullptr;
  hipEvent_t ev[EV_COUNT]{};
  hipEvent_t ev_sync[SYNC_COUNT]{};
  // Pinned staging for the asynchronous forms of hb_set_resident_time / hb_estimator_update / hb_refgen_update: a caller-owned host
  // array is copied into a library-owned pinned slot and uploaded from there, so the call returns without a device
  // synchronisation and the caller's array is free again.  STAGE_DEPTH slots per array, each guarded by the event of its last upload:
  // the host can run at most STAGE_DEPTH ticks ahead of the device.
  static constexpr int STAGE_ARRAYS = 10, STAGE_DEPTH = 4;
  struct StageSlot { void* host = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool pending = false; };
  StageSlot stage[STAGE_ARRAYS][STAGE_DEPTH];
  unsigned stage_turn[STAGE_ARRAYS]{};
  // hb_tick_resident: device-side upload targets of one tick's host inputs (read early in every instance range's tick, so that
  // the next tick's upload only has to wait for that early point), the upload stream and its events
  struct TickUpload { double *quat = nullptr, *w = nullptr, *a = nullptr, *qj = nullptr, *qdj = nullptr, *tnow = nullptr, *t0 = nullptr, *cmd = nullptr; int* contact = nullptr; } up;
  hipStream_t s_up = nullptr;
  hipEvent_t ev_up = nullptr, ev_consumed[kMaxRanges]{};
  int consumed_pending = 0;
  bool grid_saved = false;  // tp / modep / np_nodes hold the grid the iterate lives on; the tables have changed since
  bool policy_read_pending = false;
  bool refs_set = false, traj_set = false, timed = false;
  std::vector<void*> allocs;
  ErrSlot err;
  WbcBatch w{};
  hb_stats stats{};
  double* x0_seq = nullptr;  // optional device-resident sequence of measured states for hb_step_resident
  int n_seq = 0, seq_idx = 0;
  // instance chunks pipelined on their own streams by hb_step_resident (independent instances: the latency-bound
  // per-instance sweeps of one chunk overlap the per-node kernels of another)
  int n_chunks = 1;
  hipStream_t s_chunk[kMaxRanges]{};
  // hipGraphs of one chunk's whole step (x0 -> SQP iteration -> publish -> policy -> WBC), one per (chunk, x0-sequence slot): at
  // small batch sizes the step is launch bound — ~25 enqueues per chunk and step against kernels of 100..900 us — and the
  // chunk streams only overlap if the host keeps them fed.  Graphs captured in epoch e are stale once a device pointer they
  // hold changes (the iterate / previous-iterate swap of the warm start, a new x0 sequence, a new chunk count).
  static constexpr int GRAPH_SLOTS = 16;
  hipGraphExec_t chunk_graph[kMaxRanges][GRAPH_SLOTS]{};
  uint64_t chunk_graph_epoch[kMaxRanges][GRAPH_SLOTS]{};
  uint64_t graph_epoch = 1;
  int64_t dbg_graph_launches = 0, dbg_direct = 0, dbg_forks = 0, dbg_captures = 0, dbg_capture_failures = 0;
  bool graph_disabled = false;   // a capture / instantiation failed once: direct launches from then on (until hb_set_chunks)
  int steady_chunked_steps = 0;   // chunked steps since the last fork: graphs are only captured in steady state
  int chunks_pending = 0;    // chunk streams of the last chunked hb_step_resident not yet joined into the library streams
  bool fork_needed = true;   // something may have been queued on the library streams since the last chunked step
  unsigned char* reset_mask = nullptr;  // [B] staging of hb_mpc_reset_masked
  double* jc_out = nullptr;  // joint command outputs [6][B][10]
  bool jc_computed = false;  // hb_joint_command has run (jc_out alone is also allocated by hb_joint_set_flags / get_emergency_stop)
  int* jc_estop = nullptr;   // [B] latched emergencyStopFlag_ per instance
  int* jc_loaded = nullptr;  // [B] loadControllerFlag_ per instance (default: loaded)
  uint64_t* lcm_cmd = nullptr;    // [B][62] low_cmd_t wire images
  uint64_t* lcm_state = nullptr;  // [B][42] low_state_t wire images
  long long* lcm_ts = nullptr;    // [B]
  int* lcm_bad = nullptr;
  PlantBatch plant{};
  bool plant_ready = false;
  // sensor model of the plant (hb_plant_set_sensor_model): sens_noisy = a configuration with at least one sigma > 0 is in force;
  // sense_count = hb_plant_sense calls since the model was set (the noise counter); sensed = the sensor arrays hold a reading of this
  // plant (cleared by hb_plant_reset)
  hb_sensor_config sens_cfg{};
  bool sens_noisy = false, sensed = false;
  uint64_t sense_count = 0;
  double *sens_gyro_bias_buf = nullptr, *sens_accel_bias_buf = nullptr;  // [B][3] each, allocated on the first non-null bias
  // reference generation (allocated on the first hb_refgen_reset)
  RefgenBatch rg{};
  hb_refgen_config rg_cfg{};
  bool rg_ready = false;
  std::vector<int> rg_have_schedule;
  // device gait manager (allocated on the first hb_gait_reset); while gait_on, k_gait writes the schedule windows
  GaitBatch gait{};
  hb_gait_config gait_cfg{};
  bool gait_on = false;
  // state estimator (allocated on the first hb_estimator_reset)
  EstBatch est{};
  hb_estimator_config est_cfg{};
  bool est_ready = false;
  // KKT certificate of the WeightedWbc QP (hb_wbc_set_certificate): allocated on the first enable; cert_last tells whether the last
  // WBC call ran the certificate kernel
  bool wbc_cert = false, cert_last = false;
  double* cert_buf = nullptr;  // [B][HB_WBC_CERT_SIZE]
  double* dual_buf = nullptr;  // [B][HB_WBC_NCONS_MAX]
  // per-level certificate of the HierarchicalWbc cascade (hb_hwbc_set_certificate): the same switch (wbc_cert / cert_last) on a
  // wbc_type = 1 context, its own buffers
  double* hcert_buf = nullptr;    // [B][HB_HWBC_LEVELS][HB_HWBC_CERT_SIZE]
  double* hxlev_buf = nullptr;    // [B][HB_HWBC_LEVELS][38]
  double* hslack_buf = nullptr;   // [B][HB_HWBC_NINEQ_MAX]
  double* hdual_buf = nullptr;    // [B][HB_HWBC_LEVELS][HB_HWBC_NINEQ_MAX]
  // KKT certificate of the MPC's stage QP (hb_mpc_get_certificate): work buffers allocated on the first call.  The records, gains and
  // step of a solve belong to the node tables and the iterate it ran on: mpc_tables_epoch counts their replacements by the host
  // (hb_mpc_set_references, hb_refgen_update, hb_mpc_reset*, hb_mpc_set_trajectory), mpc_solved_epoch is its value at the last MPC call
  // (0: none yet).
  MpcCertBuf mcert{};
  uint64_t mpc_tables_epoch = 1, mpc_solved_epoch = 0;
};

static thread_local std::string g_create_error;

#define HB_HIP(call)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess) {                                                                \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
      return HB_ERR_DEVICE;                                                                \
    }                                                                                      \
  } while (0)

// passes on the failure of a call that returns an hb status (its error text is already set)
#define HB_TRY(expr)                \
  do {                              \
    const int32_t rc_ = (expr);     \
    if (rc_ != HB_OK) return rc_;   \
  } while (0)

// Device scratch of one call of a unit-level entry point, freed on every return path.
template <class T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  // n elements, filled from the host array `from` when one is given
  hipError_t alloc(size_t n, const T* from = nullptr) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
    if (e == hipSuccess && from) e = hipMemcpy(p, from, n * sizeof(T), hipMemcpyHostToDevice);
    return e;
  }
};

template <class T>
static hipError_t dalloc(hb_ctx* ctx, T** p, size_t n) {
  hipError_t e = hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T));
  if (e == hipSuccess) {
    ctx->allocs.push_back(*p);
    e = hipMemset(*p, 0, n * sizeof(T));
    // the library's streams are non-blocking: without this, work queued on them right after a late allocation (reset mask,
    // joint-command state, LCM staging) could run BEFORE the zero fill on the null stream
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  }
  return e;
}

extern "C" {

int32_t hb_version(void) { return 202; }

const char* hb_last_error(const hb_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int32_t hb_create(const hb_model* model, const hb_config* config, int32_t batch, int32_t max_nodes, int32_t device,
                  hb_ctx** out) {
  if (!model || !config || !out || batch <= 0 || max_nodes <= 0) {
    g_create_error = "hb_create: bad argument";
    return HB_ERR_ARG;
  }
  if (!topology_supported(*model)) {
    g_create_error = "hb_create: model topology is not base + two 5-joint legs";
    return HB_ERR_ARG;
  }
  // (the struct has grown over the rounds and carries no size field: a caller built against an older, smaller hb_config makes the library
  // read past its end — fields that gate loops are therefore range-checked, and the tail word must be the documented 0)
  if (config->wbc_reg_steps < 0 || config->wbc_reg_steps > HB_WBC_REG_STEPS_MAX || config->wbc_eps_mode < 0 || config->wbc_eps_mode > 1 || (config->wbc_eps_mode == 1 && config->wbc_type != 0) || config->wbc_max_iter <= 0 ||
      !(config->wbc_eps_reg > 0.0)) {
    g_create_error = "hb_create: hb_config.wbc_reg_steps outside [0, 8], wbc_eps_mode not 0 / 1 (1: WeightedWbc only), wbc_max_iter <= 0 or wbc_eps_reg <= 0 (struct built against another header?)";
    return HB_ERR_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device >= ndev) {
    g_create_error = "hb_create: no HIP device visible (the solver has no CPU fallback)";
    return HB_ERR_NO_GPU;
  }
  hb_ctx* ctx = new hb_ctx();
  ctx->device = device;
  ctx->B = batch;
  ctx->Nmax = max_nodes;
  ctx->model = *model;
  ctx->config = *config;
  ctx->hmodel = make_dev_model(*model);
  ctx->hconfig = make_dev_config(*config, ctx->hmodel);

  auto fail = [&](const char* what, hipError_t e) {
    g_create_error = std::string("hb_create: ") + what + ": " + hipGetErrorString(e);
    for (void* p : ctx->allocs) (void)hipFree(p);
    delete ctx;
    return HB_ERR_DEVICE;
  };
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) return fail("hipSetDevice", e);
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) ctx->n_cu = ncu;
  }
  if ((e = hipStreamCreateWithFlags(&ctx->s_mpc, hipStreamNonBlocking)) != hipSuccess) return fail("stream", e);
  if ((e = hipStreamCreateWithFlags(&ctx->s_wbc, hipStreamNonBlocking)) != hipSuccess) return fail("stream", e);
  for (auto& ev : ctx->ev)
    if ((e = hipEventCreate(&ev)) != hipSuccess) return fail("event", e);
  for (auto& ev : ctx->ev_sync)
    if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return fail("event", e);
  for (auto& sc : ctx->s_chunk)
    if ((e = hipStreamCreateWithFlags(&sc, hipStreamNonBlocking)) != hipSuccess) return fail("chunk stream", e);
  const size_t B = batch, N = max_nodes;
  Batch& b = ctx->b;
  b.B = batch;
  b.Nmax = max_nodes;
#define A(ptr, n) if ((e = dalloc(ctx, &ptr, n)) != hipSuccess) return fail(#ptr, e)
  A(ctx->dmodel, 1);
  A(ctx->dconfig, 1);
  A(b.n_nodes, B);
  A(b.t, B * (N + 1));
  A(b.mode, B * N);
  A(b.xref, B * N * HB_NX);
  A(b.swing, B * N * 24);
  A(b.x, B * (N + 1) * HB_NX);
  A(b.u, B * N * HB_NU);
  A(b.x0, B * HB_NX);
  A(b.recs, B * N * REC_SIZE);
  A(b.gains, B * N * GAIN_SIZE);
  A(b.dx, B * (N + 1) * HB_NX);
  A(b.du, B * N * HB_NU);
  A(b.acc, B * 4);
  A(b.partial, B * N * 3);
  A(b.ls_tail, B * LS_TAIL_MAX * N * 3);
  A(b.ls_norm, B * 2);
  A(b.accepted, B);
  A(b.perf, B * 4);
  A(b.ric_fail, B);
  A(b.mpc_status, B);
  A(b.xp, B * (N + 1) * HB_NX);
  A(b.up, B * N * HB_NU);
  A(b.tp, B * (N + 1));
  A(b.modep, B * N);
  A(b.np_nodes, B);
  A(b.grid_dirty, B);
  A(b.lqpark, B * (N + LqPark::trip_max) * LqPark::size);
  WbcBatch& w = ctx->w;
  w.B = batch;
  A(w.t_now, B);
  A(w.rbd, B * HB_NRBD);
  A(w.walk, B);
  A(w.xdes, B * HB_NX);
  A(w.udes, B * HB_NU);
  A(w.mode, B);
  A(w.stance, B);
  A(w.sol, B * HB_NWBC);
  A(w.status, B);
  A(w.iters, B);
  A(w.px, B * (N + 1) * HB_NX);
  A(w.pu, B * N * HB_NU);
  A(w.pt, B * (N + 1));
  A(w.pmode, B * N);
  A(w.pn, B);
#undef A
  if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_hwbc), hipFuncAttributeMaxDynamicSharedMemorySize,
                               int(HoLdsDev::total * sizeof(double)))) != hipSuccess)
    return fail("k_hwbc LDS size", e);
  if ((e = hipMemcpy(ctx->dmodel, &ctx->hmodel, sizeof(DevModel), hipMemcpyHostToDevice)) != hipSuccess) return fail("model", e);
  if ((e = hipMemcpy(ctx->dconfig, &ctx->hconfig, sizeof(DevConfig), hipMemcpyHostToDevice)) != hipSuccess) return fail("config", e);
  // walking by default
  std::vector<int> ones(B, 1);
  if ((e = hipMemcpy(w.walk, ones.data(), B * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess) return fail("walk", e);
  *out = ctx;
  return HB_OK;
}

void hb_destroy(hb_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  for (void* p : ctx->allocs) (void)hipFree(p);
  for (auto& ev : ctx->ev) (void)hipEventDestroy(ev);
  for (auto& ev : ctx->ev_sync) (void)hipEventDestroy(ev);
  if (ctx->s_up) (void)hipStreamDestroy(ctx->s_up);
  if (ctx->ev_up) (void)hipEventDestroy(ctx->ev_up);
  for (auto& ev : ctx->ev_consumed)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& arr : ctx->stage)
    for (auto& sl : arr) {
      if (sl.done) (void)hipEventDestroy(sl.done);
      if (sl.host) (void)hipHostFree(sl.host);
    }
  (void)hipStreamDestroy(ctx->s_mpc);
  (void)hipStreamDestroy(ctx->s_wbc);
  for (auto& row : ctx->chunk_graph)
    for (auto& g : row)
      if (g) (void)hipGraphExecDestroy(g);
  for (auto& sc : ctx->s_chunk) (void)hipStreamDestroy(sc);
  delete ctx;
}

// Upload of a caller-owned host array through pinned staging (see hb_ctx::stage): returns as soon as the bytes are in the slot.
// Each array id belongs to one side of the two-thread split (control side: time, sensors; MPC side: t0, cmd, x0; hb_tick_resident,
// which uses all of them, is a single-thread entry point), so a ring is only ever advanced by one thread.
enum StageId { ST_TNOW = 0, ST_QUAT, ST_W, ST_A, ST_QJ, ST_QDJ, ST_CONTACT, ST_T0, ST_CMD, ST_X0 };
static int32_t stage_upload(hb_ctx* ctx, int id, void* dst, const void* src, size_t bytes, hipStream_t s) {
  hb_ctx::StageSlot& sl = ctx->stage[id][ctx->stage_turn[id]++ % hb_ctx::STAGE_DEPTH];
  if (sl.pending) { HB_HIP(hipEventSynchronize(sl.done)); sl.pending = false; }
  if (sl.cap < bytes) {
    if (sl.host) HB_HIP(hipHostFree(sl.host));
    sl.host = nullptr; sl.cap = 0;
    HB_HIP(hipHostMalloc(&sl.host, bytes, hipHostMallocDefault));
    sl.cap = bytes;
  }
  if (!sl.done) HB_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
  std::memcpy(sl.host, src, bytes);
  HB_HIP(hipMemcpyAsync(dst, sl.host, bytes, hipMemcpyHostToDevice, s));
  HB_HIP(hipEventRecord(sl.done, s));
  sl.pending = true;
  return HB_OK;
}

// The six sensor arrays of an estimator update (quaternion, angular velocity, linear acceleration, joint positions, joint
// velocities, contact flags: staging ids ST_QUAT .. ST_CONTACT) into dst[0..5] on s, through pinned staging when `staged`.
static int32_t upload_sensors(hb_ctx* ctx, const void* const dst[6], const void* const src[6], bool staged, hipStream_t s) {
  static constexpr size_t bytes_per_instance[6] = {4 * 8, 3 * 8, 3 * 8, 10 * 8, 10 * 8, 4 * sizeof(int)};
  for (int k = 0; k < 6; ++k) {
    void* d = const_cast<void*>(dst[k]);
    const size_t bytes = size_t(ctx->B) * bytes_per_instance[k];
    if (staged) HB_TRY(stage_upload(ctx, ST_QUAT + k, d, src[k], bytes, s));
    else HB_HIP(hipMemcpyAsync(d, src[k], bytes, hipMemcpyHostToDevice, s));
  }
  return HB_OK;
}

// Chunked hb_step_resident calls free-run: every chunk of instances is its own stream that goes from one step straight into the
// next (instances are independent), without a per-step join.  The join into the two library streams happens here, lazily, at
// the start of every OTHER entry point — the getters, the table updates, the joint command, hb_sync ... only know s_mpc / s_wbc —
// and the next chunked step then forks again from them.
static void lazy_join(hb_ctx* ctx) {
  if (ctx->chunks_pending == 0 && ctx->fork_needed) return;  // nothing in flight (always, without chunks): no state is touched
  for (int c = 0; c < ctx->chunks_pending; ++c) {
    (void)hipStreamWaitEvent(ctx->s_mpc, ctx->ev_sync[SYNC_JOIN + c], 0);
    (void)hipStreamWaitEvent(ctx->s_wbc, ctx->ev_sync[SYNC_JOIN + c], 0);
  }
  ctx->chunks_pending = 0;
  ctx->fork_needed = true;
}

extern "C++" {  // (templates cannot have C linkage)
// Enqueues a writer of the resident observation on s (launch()); with `fence`, between two ordering points: it starts after the work
// queued so far on the MPC stream, and the MPC stream's later work after it (the observation feeds the next solve there).
template <class F>
static int32_t resident_write(hb_ctx* ctx, hipStream_t s, bool fence, F&& launch) {
  if (fence) {
    HB_HIP(hipEventRecord(ctx->ev_sync[SYNC_BEFORE_WRITER], ctx->s_mpc));
    HB_HIP(hipStreamWaitEvent(s, ctx->ev_sync[SYNC_BEFORE_WRITER], 0));
  }
  launch();
  HB_HIP(hipGetLastError());
  if (fence) {
    HB_HIP(hipEventRecord(ctx->ev_sync[SYNC_AFTER_WRITER], s));
    HB_HIP(hipStreamWaitEvent(ctx->s_mpc, ctx->ev_sync[SYNC_AFTER_WRITER], 0));
  }
  return HB_OK;
}
}  // extern "C++"

// joint command outputs and the per-instance controller flags (allocated on first use; loaded = 1, no emergency stop)
static int32_t joint_state_alloc(hb_ctx* ctx) {
  if (ctx->jc_out) return HB_OK;
  const size_t n = size_t(ctx->B) * HB_NJ;
  HB_HIP(dalloc(ctx, &ctx->jc_out, 6 * n));
  HB_HIP(dalloc(ctx, &ctx->jc_estop, size_t(ctx->B)));
  HB_HIP(dalloc(ctx, &ctx->jc_loaded, size_t(ctx->B)));
  std::vector<int> ones(size_t(ctx->B), 1);
  HB_HIP(hipMemcpy(ctx->jc_loaded, ones.data(), ones.size() * sizeof(int), hipMemcpyHostToDevice));
  return HB_OK;
}

int32_t hb_joint_set_flags(hb_ctx* ctx, const int32_t* controller_loaded, const int32_t* emergency_stop) {
  if (ctx) lazy_join(ctx);
  if (!ctx) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
  HB_TRY(joint_state_alloc(ctx));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  if (controller_loaded) HB_HIP(hipMemcpy(ctx->jc_loaded, controller_loaded, size_t(ctx->B) * sizeof(int), hipMemcpyHostToDevice));
  if (emergency_stop) HB_HIP(hipMemcpy(ctx->jc_estop, emergency_stop, size_t(ctx->B) * sizeof(int), hipMemcpyHostToDevice));
  return HB_OK;
}

int32_t hb_joint_get_emergency_stop(hb_ctx* ctx, int32_t* emergency_stop) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !emergency_stop) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
  HB_TRY(joint_state_alloc(ctx));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  HB_HIP(hipMemcpy(emergency_stop, ctx->jc_estop, size_t(ctx->B) * sizeof(int), hipMemcpyDeviceToHost));
  return HB_OK;
}

int32_t hb_joint_command(hb_ctx* ctx, const hb_joint_gains* gains, double dt, double* pos_des, double* vel_des, double* kp, double* kd,
                         double* tau_ff, double* torque) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !gains) return HB_ERR_ARG;
  if (ctx->stats.n_wbc_solves == 0) {
    ctx->err = "hb_joint_command: no WBC solution yet";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
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

int32_t hb_plant_reset(hb_ctx* ctx, const double* q0, const double* v0, double baumgarte, double eps) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !q0 || !(baumgarte >= 0.0) || !(eps >= 0.0)) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
  const size_t B = ctx->B;
  PlantBatch& p = ctx->plant;
  if (!p.q) {
    HB_HIP(dalloc(ctx, &p.q, B * 16));
    HB_HIP(dalloc(ctx, &p.v, B * 16));
    HB_HIP(dalloc(ctx, &p.anchor, B * 12));
    HB_HIP(dalloc(ctx, &p.pinned, B * 4));
    HB_HIP(dalloc(ctx, &p.lambda, B * 12));
    HB_HIP(dalloc(ctx, &p.vdot, B * 16));
    HB_HIP(dalloc(ctx, &p.tau, B * 10));
    HB_HIP(dalloc(ctx, &p.contact, B * 4));
    HB_HIP(dalloc(ctx, &p.rbd, B * HB_NRBD));
    HB_HIP(dalloc(ctx, &p.tau_last, B * 10));
    HB_HIP(dalloc(ctx, &p.contact_last, B * 4));
    HB_HIP(dalloc(ctx, &p.s_quat, B * 4));
    HB_HIP(dalloc(ctx, &p.s_gyro, B * 3));
    HB_HIP(dalloc(ctx, &p.s_accel, B * 3));
    HB_HIP(dalloc(ctx, &p.s_jp, B * 10));
    HB_HIP(dalloc(ctx, &p.s_jv, B * 10));
    HB_HIP(dalloc(ctx, &p.s_jt, B * 10));
    HB_HIP(dalloc(ctx, &p.s_contact, B * 4));
    p.B = ctx->B;
  }
  ctx->sensed = false;
  p.baum = baumgarte;
  p.eps = eps;
  HB_HIP(hipMemcpy(p.q, q0, B * 16 * 8, hipMemcpyHostToDevice));
  if (v0) HB_HIP(hipMemcpy(p.v, v0, B * 16 * 8, hipMemcpyHostToDevice));
  else HB_HIP(hipMemset(p.v, 0, B * 16 * 8));
  hipLaunchKernelGGL(k_plant_reset, dim3((ctx->B + 63) / 64), dim3(64), 0, ctx->s_wbc, p, ctx->dmodel);
  HB_HIP(hipGetLastError());
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  ctx->plant_ready = true;
  return HB_OK;
}

int32_t hb_plant_step(hb_ctx* ctx, const double* tau, const int32_t* contact, double dt, int32_t substeps, int32_t to_resident) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !(dt > 0.0) || substeps < 1) return HB_ERR_ARG;
  if (!ctx->plant_ready) {
    ctx->err = "hb_plant_step: call hb_plant_reset first";
    return HB_ERR_STATE;
  }
  if ((!tau && !ctx->jc_computed) || (!contact && ctx->stats.n_wbc_solves == 0)) {
    ctx->err = "hb_plant_step: no device-resident torque / contact flags yet (hb_joint_command after a WBC call)";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  const size_t B = ctx->B;
  PlantBatch& p = ctx->plant;
  hipStream_t s = ctx->s_wbc;  // the plant follows the control thread
  if (tau) HB_HIP(hipMemcpyAsync(p.tau, tau, B * 10 * 8, hipMemcpyHostToDevice, s));
  if (contact) HB_HIP(hipMemcpyAsync(p.contact, contact, B * 4 * sizeof(int), hipMemcpyHostToDevice, s));
  const double* dtau = tau ? p.tau : ctx->jc_out + 5 * B * HB_NJ;
  // the resident observation feeds the next hb_mpc_solve(NULL) / hb_refgen_update(NULL) on the MPC stream
  return resident_write(ctx, s, to_resident, [&] {
    hipLaunchKernelGGL(k_plant, dim3(ctx->B), dim3(64), 0, s, p, ctx->dmodel, dtau, contact ? p.contact : nullptr, ctx->w.mode, dt, substeps,
                       to_resident ? ctx->w.rbd : nullptr, to_resident ? ctx->b.x0 : nullptr, to_resident ? ctx->w.t_now : nullptr);
  });
}

int32_t hb_plant_get_state(hb_ctx* ctx, double* q, double* v, double* rbd, double* lambda, double* vdot) {
  if (ctx) lazy_join(ctx);
  if (!ctx) return HB_ERR_ARG;
  if (!ctx->plant_ready) {
    ctx->err = "hb_plant_get_state: call hb_plant_reset first";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  const size_t B = ctx->B;
  const PlantBatch& p = ctx->plant;
  if (q) HB_HIP(hipMemcpy(q, p.q, B * 16 * 8, hipMemcpyDeviceToHost));
  if (v) HB_HIP(hipMemcpy(v, p.v, B * 16 * 8, hipMemcpyDeviceToHost));
  if (rbd) HB_HIP(hipMemcpy(rbd, p.rbd, B * HB_NRBD * 8, hipMemcpyDeviceToHost));
  if (lambda) HB_HIP(hipMemcpy(lambda, p.lambda, B * 12 * 8, hipMemcpyDeviceToHost));
  if (vdot) HB_HIP(hipMemcpy(vdot, p.vdot, B * 16 * 8, hipMemcpyDeviceToHost));
  return HB_OK;
}

int32_t hb_plant_set_sensor_model(hb_ctx* ctx, const hb_sensor_config* cfg, const double* gyro_bias, const double* accel_bias) {
  if (ctx) lazy_join(ctx);
  if (!ctx) return HB_ERR_ARG;
  if (!ctx->plant_ready) {
    ctx->err = "hb_plant_set_sensor_model: call hb_plant_reset first (the sensor arrays belong to the plant)";
    return HB_ERR_STATE;
  }
  if (cfg && !sensor_config_valid(*cfg)) {
    ctx->err = "hb_plant_set_sensor_model: every noise standard deviation must be finite and >= 0, and `reserved` 0";
    return HB_ERR_ARG;
  }
  HB_HIP(hipSetDevice(ctx->device));
  const size_t B = ctx->B;
  PlantBatch& p = ctx->plant;
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));  // (an earlier reading may still be using the biases)
  // the bias arrays are kept once allocated; a null pointer in the batch means "no bias"
  const double* src[2] = {gyro_bias, accel_bias};
  double** dst[2] = {&p.gyro_bias, &p.accel_bias};
  double** store[2] = {&ctx->sens_gyro_bias_buf, &ctx->sens_accel_bias_buf};
  for (int k = 0; k < 2; ++k) {
    if (src[k]) {
      if (!*store[k]) HB_HIP(dalloc(ctx, store[k], B * 3));
      HB_HIP(hipMemcpy(*store[k], src[k], B * 3 * 8, hipMemcpyHostToDevice));
    }
    *dst[k] = src[k] ? *store[k] : nullptr;
  }
  ctx->sens_cfg = cfg ? *cfg : hb_sensor_config{};
  ctx->sens_noisy = cfg && (cfg->orientation_noise > 0.0 || cfg->gyro_noise > 0.0 || cfg->accel_noise > 0.0 || cfg->joint_pos_noise > 0.0 ||
                            cfg->joint_vel_noise > 0.0 || cfg->joint_torque_noise > 0.0);
  ctx->sense_count = 0;
  return HB_OK;
}

int32_t hb_plant_sense(hb_ctx* ctx, double* quat, double* ang_vel_local, double* lin_acc_local, double* joint_pos, double* joint_vel,
                       double* joint_torque, int32_t* contact_flag) {
  if (ctx) lazy_join(ctx);
  if (!ctx) return HB_ERR_ARG;
  if (!ctx->plant_ready) {
    ctx->err = "hb_plant_sense: call hb_plant_reset first";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  const size_t B = ctx->B;
  const PlantBatch& p = ctx->plant;
  hipStream_t s = ctx->s_wbc;  // behind the plant step, in front of the estimator
  hipLaunchKernelGGL(k_plant_sense, dim3((ctx->B + kSenseThreads - 1) / kSenseThreads), dim3(kSenseThreads), 0, s, p, ctx->dmodel, ctx->sens_cfg,
                     ctx->sens_noisy ? 1 : 0, static_cast<unsigned long long>(ctx->sense_count));
  HB_HIP(hipGetLastError());
  ++ctx->sense_count;
  ctx->sensed = true;
  double* const outs[6] = {quat, ang_vel_local, lin_acc_local, joint_pos, joint_vel, joint_torque};
  const double* const dev[6] = {p.s_quat, p.s_gyro, p.s_accel, p.s_jp, p.s_jv, p.s_jt};
  const size_t width[6] = {4, 3, 3, 10, 10, 10};
  bool any = contact_flag != nullptr;
  for (int k = 0; k < 6; ++k)
    if (outs[k]) {
      HB_HIP(hipMemcpyAsync(outs[k], dev[k], B * width[k] * 8, hipMemcpyDeviceToHost, s));
      any = true;
    }
  if (contact_flag) HB_HIP(hipMemcpyAsync(contact_flag, p.s_contact, B * 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  if (any) HB_HIP(hipStreamSynchronize(s));  // without host outputs the call is enqueue-only
  return HB_OK;
}

int32_t hb_refgen_reset(hb_ctx* ctx, const hb_refgen_config* cfg, const double* latest_stance) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !cfg || !(cfg->dt > 0.0)) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
  const size_t B = ctx->B;
  RefgenBatch& r = ctx->rg;
  if (!r.n_ev) {
    HB_HIP(dalloc(ctx, &r.n_ev, B));
    HB_HIP(dalloc(ctx, &r.ev, B * HB_MAX_EVENTS));
    HB_HIP(dalloc(ctx, &r.modes, B * (HB_MAX_EVENTS + 1)));
    HB_HIP(dalloc(ctx, &r.stance, B * 12));
    HB_HIP(dalloc(ctx, &r.phases, B * 4 * (HB_MAX_EVENTS + 1) * RG_PHASE));
    HB_HIP(dalloc(ctx, &r.t0, B));
    HB_HIP(dalloc(ctx, &r.cmd, B * 4));
    HB_HIP(dalloc(ctx, &r.status, B));
    HB_HIP(dalloc(ctx, &r.n_knots, B));
    HB_HIP(dalloc(ctx, &r.knot_t, B * RG_MAX_KNOTS));
    HB_HIP(dalloc(ctx, &r.knot_x, B * RG_MAX_KNOTS * HB_NX));
    r.B = ctx->B;
    ctx->rg_have_schedule.assign(B, 0);
  }
  ctx->rg_cfg = *cfg;
  r.init_stance = latest_stance ? 0 : 1;
  if (latest_stance) HB_HIP(hipMemcpy(r.stance, latest_stance, B * 12 * 8, hipMemcpyHostToDevice));
  ctx->rg_ready = true;
  return HB_OK;
}

int32_t hb_refgen_set_schedule(hb_ctx* ctx, int32_t i0, int32_t cnt, const int32_t* n_events, const double* event_times,
                               const int32_t* modes) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !n_events || !event_times || !modes || i0 < 0 || cnt <= 0 || i0 + cnt > ctx->B) return HB_ERR_ARG;
  if (!ctx->rg_ready) {
    ctx->err = "hb_refgen_set_schedule: call hb_refgen_reset first";
    return HB_ERR_STATE;
  }
  if (ctx->gait_on) {
    ctx->err = "hb_refgen_set_schedule: the device gait manager writes the schedules (hb_gait_reset); call hb_gait_disable to supply them from the host";
    return HB_ERR_STATE;
  }
  for (int i = 0; i < cnt; ++i) {
    if (n_events[i] < 0 || n_events[i] > HB_MAX_EVENTS) {
      ctx->err = "hb_refgen_set_schedule: n_events out of range";
      return HB_ERR_ARG;
    }
    for (int e = 0; e <= n_events[i]; ++e) {
      const int m = modes[size_t(i) * (HB_MAX_EVENTS + 1) + e];
      if (m < 0 || m > 3) {
        ctx->err = "hb_refgen_set_schedule: mode out of range";
        return HB_ERR_ARG;
      }
    }
  }
  HB_HIP(hipSetDevice(ctx->device));
  RefgenBatch& r = ctx->rg;
  HB_HIP(hipMemcpy(r.n_ev + i0, n_events, cnt * sizeof(int), hipMemcpyHostToDevice));
  HB_HIP(hipMemcpy(r.ev + size_t(i0) * HB_MAX_EVENTS, event_times, size_t(cnt) * HB_MAX_EVENTS * 8, hipMemcpyHostToDevice));
  HB_HIP(hipMemcpy(r.modes + size_t(i0) * (HB_MAX_EVENTS + 1), modes, size_t(cnt) * (HB_MAX_EVENTS + 1) * sizeof(int), hipMemcpyHostToDevice));
  for (int i = 0; i < cnt; ++i) ctx->rg_have_schedule[i0 + i] = 1;
  return HB_OK;
}

// ---- instance-range views and the launchers shared by the whole-batch entry points and the instance ranges ----------------------
// Views: sub-batch [i0, i0 + cnt) of a batch, same layout, offset base pointers.
static Batch batch_view(const Batch& b, int i0, int cnt) {
  Batch v = b;
  const size_t N = b.Nmax, o = i0;
  v.B = cnt;
  v.n_nodes += o; v.t += o * (N + 1); v.mode += o * N; v.xref += o * N * HB_NX; v.swing += o * N * 24;
  v.x += o * (N + 1) * HB_NX; v.u += o * N * HB_NU; v.x0 += o * HB_NX; v.recs += o * N * REC_SIZE; v.gains += o * N * GAIN_SIZE;
  v.dx += o * (N + 1) * HB_NX; v.du += o * N * HB_NU; v.acc += o * 4; v.partial += o * N * 3; v.ls_tail += o * LS_TAIL_MAX * N * 3; v.ls_norm += o * 2; v.accepted += o; v.perf += o * 4;
  v.ric_fail += o; v.mpc_status += o; v.xp += o * (N + 1) * HB_NX; v.up += o * N * HB_NU; v.tp += o * (N + 1); v.modep += o * N;
  v.np_nodes += o; v.grid_dirty += o; v.lqpark += o * (N + LqPark::trip_max) * LqPark::size;
  return v;
}
static WbcBatch wbc_view(const WbcBatch& w, int Nmax, int i0, int cnt) {
  WbcBatch v = w;
  const size_t N = Nmax, o = i0;
  v.B = cnt;
  v.t_now += o; v.rbd += o * HB_NRBD; v.walk += o; v.xdes += o * HB_NX; v.udes += o * HB_NU; v.mode += o; v.stance += o;
  v.sol += o * HB_NWBC; v.status += o; v.iters += o;
  v.px += o * (N + 1) * HB_NX; v.pu += o * N * HB_NU; v.pt += o * (N + 1); v.pmode += o * N; v.pn += o;
  return v;
}
// (what k_estimator reads and writes; the resident outputs res_* are the caller's, the contact-force observer is not viewed)
static EstBatch est_view(const EstBatch& e, int i0, int cnt) {
  EstBatch v = e;
  const size_t o = i0;
  v.B = cnt;
  v.xhat += o * 18; v.P += o * 324; v.yaw_last += o; v.rbd += o * HB_NRBD; v.x += o * HB_NX;
  v.quat += o * 4; v.w_local += o * 3; v.a_local += o * 3; v.qj += o * 10; v.qdj += o * 10; v.contact += o * 4;
  return v;
}
static RefgenBatch refgen_view(const RefgenBatch& r, int i0, int cnt) {
  RefgenBatch v = r;
  const size_t o = i0;
  v.B = cnt;
  v.n_ev += o; v.ev += o * HB_MAX_EVENTS; v.modes += o * (HB_MAX_EVENTS + 1); v.stance += o * 12;
  v.phases += o * 4 * (HB_MAX_EVENTS + 1) * RG_PHASE; v.t0 += o; v.cmd += o * 4; v.status += o; v.n_knots += o;
  v.knot_t += o * RG_MAX_KNOTS; v.knot_x += o * RG_MAX_KNOTS * HB_NX;
  return v;
}
static GaitBatch gait_view(const GaitBatch& g, int i0, int cnt) {
  GaitBatch v = g;   // (slot-major arrays: the pitch stays the whole batch)
  const size_t o = i0;
  v.B = cnt;
  v.n_ev += o; v.ev += o; v.modes += o; v.tpl_n += o; v.tpl_sw += o; v.tpl_modes += o; v.last_vel += o; v.cmd += o * 4; v.hist += o;
  v.hist_n += o; v.hist_head += o; v.level += o; v.vel_abs += o; v.vel_avg += o; v.status += o;
  return v;
}

// Before the node tables of b are overwritten while an iterate exists: keeps the grid that iterate lives on (`copy`; tp / modep /
// np_nodes) and marks instances [i0, i0 + cnt) of b dirty, so that the next solve brings them onto the new tables (k_warm_shift).
static int32_t launch_grid_save(hb_ctx* ctx, const Batch& b, bool copy, int i0, int cnt, hipStream_t s) {
  const size_t B = b.B, N = b.Nmax;
  if (copy) {
    HB_HIP(hipMemcpyAsync(b.tp, b.t, B * (N + 1) * 8, hipMemcpyDeviceToDevice, s));
    HB_HIP(hipMemcpyAsync(b.modep, b.mode, B * N * sizeof(int), hipMemcpyDeviceToDevice, s));
    HB_HIP(hipMemcpyAsync(b.np_nodes, b.n_nodes, B * sizeof(int), hipMemcpyDeviceToDevice, s));
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

// Reference generation of the instances of b / r (instances [i0, i0 + b.B) of the context): planner, joint IK (when configured), node
// tables.  With the gait manager on, k_gait first: it writes the schedule window the planner reads, and the three kernels take the
// filtered command of the gait state instead of the uploaded one.
static void launch_refgen(const hb_ctx* ctx, const Batch& b, RefgenBatch r, int i0, double horizon, hipStream_t s) {
  if (ctx->gait_on) {
    const GaitBatch g = gait_view(ctx->gait, i0, b.B);
    hipLaunchKernelGGL(k_gait, dim3((b.B + 63) / 64), dim3(64), 0, s, b, r, g, ctx->gait_cfg, horizon);
    r.cmd = g.cmd;
  }
  hipLaunchKernelGGL(k_refgen, dim3((4 * b.B + 63) / 64), dim3(64), 0, s, b, r, ctx->dmodel, ctx->rg_cfg, horizon);
  if (ctx->rg_cfg.joint_ik)
    hipLaunchKernelGGL(k_refgen_ik, dim3((2 * b.B + 7) / 8), dim3(64), 0, s, b, r, ctx->dmodel, ctx->rg_cfg, horizon);
  hipLaunchKernelGGL(k_refgen_nodes, dim3((b.B * ctx->Nmax + 63) / 64), dim3(64), 0, s, b, r, ctx->rg_cfg);
}

static void launch_estimator(const hb_ctx* ctx, const EstBatch& e, double dt, hipStream_t s) {
  hipLaunchKernelGGL(k_estimator, dim3(e.B), dim3(64), 0, s, e, ctx->dmodel, ctx->est_cfg, dt);
}

// Called (on the MPC stream) before the whole batch's node tables are written: see launch_grid_save.
static int32_t save_grid_before_table_update(hb_ctx* ctx, int i0, int cnt) {
  if (!ctx->traj_set) return HB_OK;
  HB_TRY(launch_grid_save(ctx, ctx->b, !ctx->grid_saved, i0, cnt, ctx->s_mpc));
  ctx->grid_saved = true;
  return HB_OK;
}

int32_t hb_refgen_update(hb_ctx* ctx, const double* t0, double horizon, const double* x_now, const double* cmd_vel, int32_t* status) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !t0 || !cmd_vel || !(horizon > 0.0)) return HB_ERR_ARG;
  if (!ctx->rg_ready) {
    ctx->err = "hb_refgen_update: call hb_refgen_reset first";
    return HB_ERR_STATE;
  }
  for (int v : ctx->rg_have_schedule)
    if (!v && !ctx->gait_on) {
      ctx->err = "hb_refgen_update: an instance has no mode schedule (hb_refgen_set_schedule)";
      return HB_ERR_STATE;
    }
  HB_HIP(hipSetDevice(ctx->device));
  const size_t B = ctx->B;
  RefgenBatch& r = ctx->rg;
  hipStream_t s = ctx->s_mpc;  // the tables belong to the MPC side
  HB_TRY(save_grid_before_table_update(ctx, 0, ctx->B));
  if (status) {
    HB_HIP(hipMemcpyAsync(r.t0, t0, B * 8, hipMemcpyHostToDevice, s));
    HB_HIP(hipMemcpyAsync(r.cmd, cmd_vel, B * 4 * 8, hipMemcpyHostToDevice, s));
    if (x_now) HB_HIP(hipMemcpyAsync(ctx->b.x0, x_now, B * HB_NX * 8, hipMemcpyHostToDevice, s));
  } else {  // enqueue-only form (status through hb_refgen_get_status)
    HB_TRY(stage_upload(ctx, ST_T0, r.t0, t0, B * 8, s));
    HB_TRY(stage_upload(ctx, ST_CMD, r.cmd, cmd_vel, B * 4 * 8, s));
    if (x_now) HB_TRY(stage_upload(ctx, ST_X0, ctx->b.x0, x_now, B * HB_NX * 8, s));
  }
  launch_refgen(ctx, ctx->b, r, 0, horizon, s);
  HB_HIP(hipGetLastError());
  r.init_stance = 0;
  ++ctx->mpc_tables_epoch;
  if (status) {
    HB_HIP(hipMemcpyAsync(status, r.status, B * sizeof(int), hipMemcpyDeviceToHost, s));
    HB_HIP(hipStreamSynchronize(s));
  }
  ctx->refs_set = true;
  return HB_OK;
}

int32_t hb_refgen_get_status(hb_ctx* ctx, int32_t* status) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !status) return HB_ERR_ARG;
  if (!ctx->rg_ready) {
    ctx->err = "hb_refgen_get_status: call hb_refgen_reset first";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  HB_HIP(hipMemcpyAsync(status, ctx->rg.status, size_t(ctx->B) * sizeof(int), hipMemcpyDeviceToHost, ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  return HB_OK;
}

int32_t hb_refgen_get_schedule(hb_ctx* ctx, int32_t i0, int32_t cnt, int32_t* n_events, double* event_times, int32_t* modes) {
  if (ctx) lazy_join(ctx);
  if (!ctx || i0 < 0 || cnt <= 0 || i0 > ctx->B || cnt > ctx->B - i0) return HB_ERR_ARG;
  if (!ctx->rg_ready) {
    ctx->err = "hb_refgen_get_schedule: call hb_refgen_reset first";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  const RefgenBatch& r = ctx->rg;
  const size_t o = i0, n = cnt;
  if (n_events) HB_HIP(hipMemcpy(n_events, r.n_ev + o, n * sizeof(int), hipMemcpyDeviceToHost));
  if (event_times) HB_HIP(hipMemcpy(event_times, r.ev + o * HB_MAX_EVENTS, n * HB_MAX_EVENTS * 8, hipMemcpyDeviceToHost));
  if (modes) HB_HIP(hipMemcpy(modes, r.modes + o * (HB_MAX_EVENTS + 1), n * (HB_MAX_EVENTS + 1) * sizeof(int), hipMemcpyDeviceToHost));
  return HB_OK;
}

// ---- device gait manager ------------------------------------------------------------------------------------------------------
int32_t hb_gait_reset(hb_ctx* ctx, const hb_gait_config* cfg, const uint8_t* mask) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !cfg) return HB_ERR_ARG;
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
  if (!ctx->rg_ready) {
    ctx->err = "hb_gait_reset: call hb_refgen_reset first";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  HB_TRY(hb_sync(ctx));
  const size_t B = ctx->B;
  GaitBatch& g = ctx->gait;
  if (!g.n_ev) {
    HB_HIP(dalloc(ctx, &g.n_ev, B));
    HB_HIP(dalloc(ctx, &g.ev, B * HB_MAX_EVENTS));
    HB_HIP(dalloc(ctx, &g.modes, B * (HB_MAX_EVENTS + 1)));
    HB_HIP(dalloc(ctx, &g.tpl_n, B));
    HB_HIP(dalloc(ctx, &g.tpl_sw, B * (HB_GAIT_MAX_PHASES + 1)));
    HB_HIP(dalloc(ctx, &g.tpl_modes, B * HB_GAIT_MAX_PHASES));
    HB_HIP(dalloc(ctx, &g.last_vel, B * 4));
    HB_HIP(dalloc(ctx, &g.cmd, B * 4));
    HB_HIP(dalloc(ctx, &g.hist, B * GAIT_HIST));
    HB_HIP(dalloc(ctx, &g.hist_n, B));
    HB_HIP(dalloc(ctx, &g.hist_head, B));
    HB_HIP(dalloc(ctx, &g.level, B));
    HB_HIP(dalloc(ctx, &g.vel_abs, B));
    HB_HIP(dalloc(ctx, &g.vel_avg, B));
    HB_HIP(dalloc(ctx, &g.status, B));
    g.B = g.stride = ctx->B;
    mask = nullptr;   // first use: every instance starts as a fresh object
  }
  DevBuf<unsigned char> dmask;
  if (mask) HB_HIP(dmask.alloc(B, mask));
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
  if (ctx) lazy_join(ctx);
  if (!ctx) return HB_ERR_ARG;
  if (!ctx->gait_on) return HB_OK;
  HB_HIP(hipSetDevice(ctx->device));
  HB_TRY(hb_sync(ctx));
  ctx->gait_on = false;
  ++ctx->graph_epoch;
  return HB_OK;
}

int32_t hb_gait_insert_template(hb_ctx* ctx, int32_t i0, int32_t cnt, int32_t n_switch, const double* switching_times, const int32_t* modes,
                                const double* start, const double* final_time) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !switching_times || !modes || !start || !final_time || i0 < 0 || cnt <= 0 || i0 > ctx->B || cnt > ctx->B - i0) return HB_ERR_ARG;
  bool ok = n_switch >= 2 && n_switch <= HB_GAIT_MAX_PHASES + 1;
  for (int k = 0; ok && k + 1 < n_switch; ++k) ok = modes[k] >= 0 && modes[k] <= 3 && switching_times[k] < switching_times[k + 1];
  if (!ok) {
    ctx->err = "hb_gait_insert_template: 2..9 strictly increasing switching times and modes in 0..3";
    return HB_ERR_ARG;
  }
  if (!ctx->gait_on) {
    ctx->err = "hb_gait_insert_template: the device gait manager is not enabled (hb_gait_reset)";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  HB_TRY(hb_sync(ctx));
  DevBuf<double> dsw, dstart, dfinal;
  DevBuf<int> dmodes;
  HB_HIP(dsw.alloc(n_switch, switching_times));
  HB_HIP(dmodes.alloc(n_switch - 1, modes));
  HB_HIP(dstart.alloc(cnt, start));
  HB_HIP(dfinal.alloc(cnt, final_time));
  hipLaunchKernelGGL(k_gait_insert, dim3((cnt + 63) / 64), dim3(64), 0, ctx->s_mpc, gait_view(ctx->gait, i0, cnt), ctx->gait_cfg.phase_transition_stance_time,
                     n_switch, dsw.p, dmodes.p, dstart.p, dfinal.p);
  HB_HIP(hipGetLastError());
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  return HB_OK;
}

int32_t hb_gait_get_state(hb_ctx* ctx, int32_t i0, int32_t cnt, int32_t* level, double* vel_abs, double* vel_avg, double* cmd, int32_t* n_events,
                          double* event_times, int32_t* modes, int32_t* status) {
  if (ctx) lazy_join(ctx);
  if (!ctx || i0 < 0 || cnt <= 0 || i0 > ctx->B || cnt > ctx->B - i0) return HB_ERR_ARG;
  if (!ctx->gait.n_ev) {
    ctx->err = "hb_gait_get_state: call hb_gait_reset first";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  const GaitBatch& g = ctx->gait;
  const size_t o = i0, n = cnt, B = ctx->B;
  if (level) HB_HIP(hipMemcpy(level, g.level + o, n * sizeof(int), hipMemcpyDeviceToHost));
  if (vel_abs) HB_HIP(hipMemcpy(vel_abs, g.vel_abs + o, n * 8, hipMemcpyDeviceToHost));
  if (vel_avg) HB_HIP(hipMemcpy(vel_avg, g.vel_avg + o, n * 8, hipMemcpyDeviceToHost));
  if (cmd) HB_HIP(hipMemcpy(cmd, g.cmd + o * 4, n * 4 * 8, hipMemcpyDeviceToHost));
  if (n_events) HB_HIP(hipMemcpy(n_events, g.n_ev + o, n * sizeof(int), hipMemcpyDeviceToHost));
  if (status) HB_HIP(hipMemcpy(status, g.status + o, n * sizeof(int), hipMemcpyDeviceToHost));
  // the schedule is slot-major on the device: rows of the addressed instances, slot by slot, transposed on the host
  if (event_times) {
    std::vector<double> tmp(size_t(HB_MAX_EVENTS) * n);
    HB_HIP(hipMemcpy2D(tmp.data(), n * 8, g.ev + o, B * 8, n * 8, HB_MAX_EVENTS, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i)
      for (size_t k = 0; k < HB_MAX_EVENTS; ++k) event_times[i * HB_MAX_EVENTS + k] = tmp[k * n + i];
  }
  if (modes) {
    std::vector<int> tmp(size_t(HB_MAX_EVENTS + 1) * n);
    HB_HIP(hipMemcpy2D(tmp.data(), n * sizeof(int), g.modes + o, B * sizeof(int), n * sizeof(int), HB_MAX_EVENTS + 1, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i)
      for (size_t k = 0; k <= HB_MAX_EVENTS; ++k) modes[i * (HB_MAX_EVENTS + 1) + k] = tmp[k * n + i];
  }
  return HB_OK;
}

int32_t hb_mpc_get_references(hb_ctx* ctx, int32_t i0, int32_t cnt, int32_t* n_nodes, double* t, int32_t* mode, double* x_ref,
                              double* swing_ref) {
  if (ctx) lazy_join(ctx);
  if (!ctx || i0 < 0 || cnt <= 0 || i0 + cnt > ctx->B) return HB_ERR_ARG;
  if (!ctx->refs_set) {
    ctx->err = "hb_mpc_get_references: references not set";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  const size_t N = ctx->Nmax;
  const Batch& b = ctx->b;
  if (n_nodes) HB_HIP(hipMemcpy(n_nodes, b.n_nodes + i0, cnt * sizeof(int), hipMemcpyDeviceToHost));
  if (t) HB_HIP(hipMemcpy(t, b.t + i0 * (N + 1), cnt * (N + 1) * 8, hipMemcpyDeviceToHost));
  if (mode) HB_HIP(hipMemcpy(mode, b.mode + i0 * N, cnt * N * sizeof(int), hipMemcpyDeviceToHost));
  if (x_ref) HB_HIP(hipMemcpy(x_ref, b.xref + i0 * N * HB_NX, cnt * N * HB_NX * 8, hipMemcpyDeviceToHost));
  if (swing_ref) HB_HIP(hipMemcpy(swing_ref, b.swing + i0 * N * 24, cnt * N * 24 * 8, hipMemcpyDeviceToHost));
  return HB_OK;
}

int32_t hb_estimator_reset(hb_ctx* ctx, const hb_estimator_config* cfg, const double* x_hat0) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !cfg) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
  const size_t B = ctx->B;
  EstBatch& e = ctx->est;
  if (!e.xhat) {
    double *quat, *wl, *al, *qj, *qdj;
    int* contact;
    HB_HIP(dalloc(ctx, &e.xhat, B * 18));
    HB_HIP(dalloc(ctx, &e.P, B * 324));
    HB_HIP(dalloc(ctx, &e.yaw_last, B));
    HB_HIP(dalloc(ctx, &quat, B * 4));
    HB_HIP(dalloc(ctx, &wl, B * 3));
    HB_HIP(dalloc(ctx, &al, B * 3));
    HB_HIP(dalloc(ctx, &qj, B * 10));
    HB_HIP(dalloc(ctx, &qdj, B * 10));
    HB_HIP(dalloc(ctx, &contact, B * 4));
    HB_HIP(dalloc(ctx, &e.rbd, B * HB_NRBD));
    HB_HIP(dalloc(ctx, &e.x, B * HB_NX));
    HB_HIP(dalloc(ctx, &e.cf_z, B * HB_NV));
    HB_HIP(dalloc(ctx, &e.cf_tau, B * HB_NJ));
    HB_HIP(dalloc(ctx, &e.cf_dist, B * HB_NV));
    HB_HIP(dalloc(ctx, &e.cf_out, B * 16));
    HB_HIP(dalloc(ctx, &e.cf_rbd, B * HB_NRBD));
    e.quat = quat; e.w_local = wl; e.a_local = al; e.qj = qj; e.qdj = qdj; e.contact = contact;
    e.B = ctx->B;
  }
  ctx->est_cfg = *cfg;
  double* x0_dev = nullptr;
  if (x_hat0) {  // staged through the (not yet used) output buffer: 22 >= 18 doubles per instance
    x0_dev = e.x;
    HB_HIP(hipMemcpy(x0_dev, x_hat0, B * 18 * 8, hipMemcpyHostToDevice));
  }
  HB_HIP(hipMemsetAsync(e.cf_z, 0, B * HB_NV * 8, ctx->s_wbc));   // pSCgZinvlast_ = 0 (StateEstimateBase.cpp:58-59)
  const int n = int(B) * 324;
  hipLaunchKernelGGL(k_estimator_reset, dim3((n + 255) / 256), dim3(256), 0, ctx->s_wbc, int(B), e.xhat, e.P, e.yaw_last, x0_dev);
  HB_HIP(hipGetLastError());
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  ctx->est_ready = true;
  return HB_OK;
}

static void launch_contact_force(const hb_ctx* ctx, double gama, double beta, const double* rbd_dev, const double* tau_dev, hipStream_t s) {
  const EstBatch& e = ctx->est;
  hipLaunchKernelGGL(k_contact_force, dim3((ctx->B + kCfThreads - 1) / kCfThreads), dim3(kCfThreads), 0, s, ctx->B, ctx->dmodel, gama, beta, rbd_dev,
                     tau_dev, e.cf_z, e.cf_dist, e.cf_out);
}

int32_t hb_estimator_contact_force(hb_ctx* ctx, double dt, const double* rbd, const double* joint_torque, double* est_disturbance_torque,
                                   double* est_contact_force) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !joint_torque || !(dt > 0.0)) return HB_ERR_ARG;
  if (!ctx->est_ready) {
    ctx->err = "hb_estimator_contact_force: call hb_estimator_reset first (it carries the cut-off frequency and zeroes the observer state)";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  const size_t B = ctx->B;
  EstBatch& e = ctx->est;
  hipStream_t s = ctx->s_wbc;   // control-thread side, behind the estimator update it follows (LeggedController.cpp:327-345)
  if (dt > 1.0) dt = 0.002;     // (StateEstimateBase.cpp:133-134)
  const double gama = std::exp(-ctx->est_cfg.contact_force_cutoff_frequency * dt), beta = (1.0 - gama) / (gama * dt);
  HB_HIP(hipMemcpyAsync(e.cf_tau, joint_torque, B * HB_NJ * 8, hipMemcpyHostToDevice, s));
  const double* rbd_dev = e.rbd;   // NULL: the rbd state the last hb_estimator_update left on the device
  if (rbd) {
    HB_HIP(hipMemcpyAsync(e.cf_rbd, rbd, B * HB_NRBD * 8, hipMemcpyHostToDevice, s));
    rbd_dev = e.cf_rbd;
  }
  launch_contact_force(ctx, gama, beta, rbd_dev, e.cf_tau, s);
  HB_HIP(hipGetLastError());
  if (est_disturbance_torque) HB_HIP(hipMemcpyAsync(est_disturbance_torque, e.cf_dist, B * HB_NV * 8, hipMemcpyDeviceToHost, s));
  if (est_contact_force) HB_HIP(hipMemcpyAsync(est_contact_force, e.cf_out, B * 16 * 8, hipMemcpyDeviceToHost, s));
  HB_HIP(hipStreamSynchronize(s));   // (the joint efforts were read from the caller's array)
  return HB_OK;
}

// filter step on the inputs e points to (device; ctx->est: its own upload buffers), outputs as in hb_estimator_update
static int32_t estimator_run(hb_ctx* ctx, EstBatch e, double dt, int32_t to_resident, double* rbd, double* x_state) {
  const size_t B = ctx->B;
  hipStream_t s = ctx->s_wbc;
  e.res_rbd = to_resident ? ctx->w.rbd : nullptr;
  e.res_x0 = to_resident ? ctx->b.x0 : nullptr;
  HB_TRY(resident_write(ctx, s, to_resident, [&] { launch_estimator(ctx, e, dt, s); }));
  if (rbd) HB_HIP(hipMemcpyAsync(rbd, e.rbd, B * HB_NRBD * 8, hipMemcpyDeviceToHost, s));
  if (x_state) HB_HIP(hipMemcpyAsync(x_state, e.x, B * HB_NX * 8, hipMemcpyDeviceToHost, s));
  if (rbd || x_state) HB_HIP(hipStreamSynchronize(s));  // without host outputs the call is enqueue-only
  return HB_OK;
}

int32_t hb_estimator_update(hb_ctx* ctx, double dt, const double* quat, const double* ang_vel_local, const double* lin_acc_local,
                            const double* joint_pos, const double* joint_vel, const int32_t* contact_flag, int32_t to_resident,
                            double* rbd, double* x_state) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !quat || !ang_vel_local || !lin_acc_local || !joint_pos || !joint_vel || !contact_flag || !(dt > 0.0)) return HB_ERR_ARG;
  if (!ctx->est_ready) {
    ctx->err = "hb_estimator_update: call hb_estimator_reset first";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  const EstBatch& e = ctx->est;
  const void* const dst[6] = {e.quat, e.w_local, e.a_local, e.qj, e.qdj, e.contact};
  const void* const src[6] = {quat, ang_vel_local, lin_acc_local, joint_pos, joint_vel, contact_flag};
  // (enqueue-only form: the sensor arrays go through pinned staging and are the caller's again on return)
  HB_TRY(upload_sensors(ctx, dst, src, !(rbd || x_state), ctx->s_wbc));  // the estimator belongs to the control-thread side (LeggedController::update)
  return estimator_run(ctx, ctx->est, dt, to_resident, rbd, x_state);
}

// The two estimator calls on the sensor arrays hb_plant_sense left on the device.
static int32_t sensed_ready(hb_ctx* ctx, const char* who) {
  const char* why = !ctx->plant_ready ? "call hb_plant_reset first"
                    : !ctx->est_ready ? "call hb_estimator_reset first"
                    : !ctx->sensed    ? "no sensor reading on the device yet (hb_plant_sense after hb_plant_reset)"
                                      : nullptr;
  if (!why) return HB_OK;
  ctx->err = std::string(who) + ": " + why;
  return HB_ERR_STATE;
}

int32_t hb_estimator_update_resident(hb_ctx* ctx, double dt, int32_t to_resident, double* rbd, double* x_state) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !(dt > 0.0)) return HB_ERR_ARG;
  HB_TRY(sensed_ready(ctx, "hb_estimator_update_resident"));
  HB_HIP(hipSetDevice(ctx->device));
  const PlantBatch& p = ctx->plant;
  EstBatch e = ctx->est;  // the same kernel with its input pointers aimed at the plant's sensor arrays: nothing is copied
  e.quat = p.s_quat; e.w_local = p.s_gyro; e.a_local = p.s_accel; e.qj = p.s_jp; e.qdj = p.s_jv; e.contact = p.s_contact;
  return estimator_run(ctx, e, dt, to_resident, rbd, x_state);
}

int32_t hb_estimator_contact_force_resident(hb_ctx* ctx, double dt, double* est_disturbance_torque, double* est_contact_force) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !(dt > 0.0)) return HB_ERR_ARG;
  HB_TRY(sensed_ready(ctx, "hb_estimator_contact_force_resident"));
  HB_HIP(hipSetDevice(ctx->device));
  const size_t B = ctx->B;
  const EstBatch& e = ctx->est;
  hipStream_t s = ctx->s_wbc;
  if (dt > 1.0) dt = 0.002;     // (StateEstimateBase.cpp:133-134)
  const double gama = std::exp(-ctx->est_cfg.contact_force_cutoff_frequency * dt), beta = (1.0 - gama) / (gama * dt);
  launch_contact_force(ctx, gama, beta, e.rbd, ctx->plant.s_jt, s);
  HB_HIP(hipGetLastError());
  if (est_disturbance_torque) HB_HIP(hipMemcpyAsync(est_disturbance_torque, e.cf_dist, B * HB_NV * 8, hipMemcpyDeviceToHost, s));
  if (est_contact_force) HB_HIP(hipMemcpyAsync(est_contact_force, e.cf_out, B * 16 * 8, hipMemcpyDeviceToHost, s));
  if (est_disturbance_torque || est_contact_force) HB_HIP(hipStreamSynchronize(s));  // without host outputs the call is enqueue-only
  return HB_OK;
}

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
  if (ctx) lazy_join(ctx);
  if (!ctx || !gains || !low_cmd) return HB_ERR_ARG;
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
  if (ctx) lazy_join(ctx);
  if (!ctx || !low_state || !contact_flag || !(dt > 0.0)) return HB_ERR_ARG;
  if (!ctx->est_ready) {
    ctx->err = "hb_estimator_update_lcm: call hb_estimator_reset first";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
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
  HB_HIP(hipMemcpyAsync(const_cast<int*>(e.contact), contact_flag, B * 4 * sizeof(int), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_lcm_unpack_state, dim3((unsigned(words) + 255) / 256), dim3(256), 0, s, ctx->B, ctx->lcm_state,
                     lcm_fingerprint(HB_LCM_LOW_STATE), const_cast<double*>(e.quat), const_cast<double*>(e.w_local),
                     const_cast<double*>(e.a_local), const_cast<double*>(e.qj), const_cast<double*>(e.qdj), ctx->lcm_ts, ctx->lcm_bad);
  HB_HIP(hipGetLastError());
  int bad = 0;
  HB_HIP(hipMemcpyAsync(&bad, ctx->lcm_bad, sizeof(int), hipMemcpyDeviceToHost, s));
  HB_HIP(hipStreamSynchronize(s));
  if (bad) {
    ctx->err = "hb_estimator_update_lcm: a message does not carry the low_state_t fingerprint";
    return HB_ERR_ARG;
  }
  if (timestamp) HB_HIP(hipMemcpy(timestamp, ctx->lcm_ts, B * 8, hipMemcpyDeviceToHost));
  return estimator_run(ctx, ctx->est, dt, to_resident, rbd, x_state);
}

int32_t hb_estimator_get_filter(hb_ctx* ctx, double* x_hat, double* P) {
  if (ctx) lazy_join(ctx);
  if (!ctx) return HB_ERR_ARG;
  if (!ctx->est_ready) {
    ctx->err = "hb_estimator_get_filter: call hb_estimator_reset first";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  if (x_hat) HB_HIP(hipMemcpy(x_hat, ctx->est.xhat, size_t(ctx->B) * 18 * 8, hipMemcpyDeviceToHost));
  if (P) HB_HIP(hipMemcpy(P, ctx->est.P, size_t(ctx->B) * 324 * 8, hipMemcpyDeviceToHost));
  return HB_OK;
}

int32_t hb_sync(hb_ctx* ctx) {
  if (ctx) lazy_join(ctx);
  if (!ctx) return HB_ERR_ARG;
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  for (auto& sc : ctx->s_chunk) HB_HIP(hipStreamSynchronize(sc));
  if (ctx->s_up) HB_HIP(hipStreamSynchronize(ctx->s_up));
  return HB_OK;
}

int32_t hb_get_input_cost(const hb_ctx* ctx, double* R) {
  if (!ctx || !R) return HB_ERR_ARG;
  std::memset(R, 0, sizeof(double) * HB_NU * HB_NU);
  for (int i = 0; i < 12; ++i) R[i * HB_NU + i] = ctx->hconfig.R_FF_diag[i];
  for (int a = 0; a < HB_NJ; ++a)
    for (int c = 0; c < HB_NJ; ++c) R[(12 + a) * HB_NU + 12 + c] = ctx->hconfig.R_jj[a * HB_NJ + c];
  return HB_OK;
}

int32_t hb_mpc_set_references(hb_ctx* ctx, int32_t i0, int32_t cnt, const int32_t* n_nodes, const double* t,
                              const int32_t* mode, const double* x_ref, const double* swing_ref) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !n_nodes || !t || !mode || !x_ref || !swing_ref || i0 < 0 || cnt <= 0 || i0 + cnt > ctx->B) {
    if (ctx) ctx->err = "hb_mpc_set_references: bad argument";
    return HB_ERR_ARG;
  }
  for (int i = 0; i < cnt; ++i)
    if (n_nodes[i] < 1 || n_nodes[i] > ctx->Nmax) {
      ctx->err = "hb_mpc_set_references: n_nodes out of range";
      return HB_ERR_ARG;
    }
  const size_t N = ctx->Nmax;
  Batch& b = ctx->b;
  HB_HIP(hipSetDevice(ctx->device));
  HB_TRY(save_grid_before_table_update(ctx, i0, cnt));
  HB_HIP(hipMemcpyAsync(b.n_nodes + i0, n_nodes, cnt * sizeof(int), hipMemcpyHostToDevice, ctx->s_mpc));
  HB_HIP(hipMemcpyAsync(b.t + i0 * (N + 1), t, cnt * (N + 1) * 8, hipMemcpyHostToDevice, ctx->s_mpc));
  HB_HIP(hipMemcpyAsync(b.mode + i0 * N, mode, cnt * N * sizeof(int), hipMemcpyHostToDevice, ctx->s_mpc));
  HB_HIP(hipMemcpyAsync(b.xref + i0 * N * HB_NX, x_ref, cnt * N * HB_NX * 8, hipMemcpyHostToDevice, ctx->s_mpc));
  HB_HIP(hipMemcpyAsync(b.swing + i0 * N * 24, swing_ref, cnt * N * 24 * 8, hipMemcpyHostToDevice, ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));  // host buffers are caller-owned: safe to reuse on return
  ctx->refs_set = true;
  ++ctx->mpc_tables_epoch;
  return HB_OK;
}

static int32_t mpc_cold_start(hb_ctx* ctx, const double* x0, const uint8_t* mask) {
  if (!ctx->refs_set) {
    ctx->err = "hb_mpc_reset: references not set";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  const size_t B = ctx->B;
  unsigned char* dmask = nullptr;
  if (mask) {
    if (!ctx->traj_set) {
      ctx->err = "hb_mpc_reset_masked: no iterate yet (hb_mpc_reset first)";
      return HB_ERR_STATE;
    }
    if (!ctx->reset_mask) HB_HIP(dalloc(ctx, &ctx->reset_mask, B));
    dmask = ctx->reset_mask;
    HB_HIP(hipMemcpyAsync(dmask, mask, B, hipMemcpyHostToDevice, ctx->s_mpc));
  }
  if (x0) {
    if (!mask) {
      HB_HIP(hipMemcpyAsync(ctx->b.x0, x0, B * HB_NX * 8, hipMemcpyHostToDevice, ctx->s_mpc));
    } else {  // only the masked rows of the observation are replaced
      for (size_t i = 0; i < B; ++i)
        if (mask[i]) HB_HIP(hipMemcpyAsync(ctx->b.x0 + i * HB_NX, x0 + i * HB_NX, HB_NX * 8, hipMemcpyHostToDevice, ctx->s_mpc));
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
  if (ctx) lazy_join(ctx);
  if (!ctx) return HB_ERR_ARG;
  return mpc_cold_start(ctx, x0, nullptr);
}

int32_t hb_mpc_reset_masked(hb_ctx* ctx, const uint8_t* mask, const double* x0) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !mask) return HB_ERR_ARG;
  return mpc_cold_start(ctx, x0, mask);
}

int32_t hb_mpc_get_status(hb_ctx* ctx, int32_t* status) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !status) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
  HB_HIP(hipMemcpyAsync(status, ctx->b.mpc_status, size_t(ctx->B) * sizeof(int), hipMemcpyDeviceToHost, ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  return HB_OK;
}

int32_t hb_mpc_set_trajectory(hb_ctx* ctx, const double* x, const double* u) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !x || !u) return HB_ERR_ARG;
  const size_t B = ctx->B, N = ctx->Nmax;
  HB_HIP(hipSetDevice(ctx->device));
  ++ctx->mpc_tables_epoch;
  HB_HIP(hipMemcpyAsync(ctx->b.x, x, B * (N + 1) * HB_NX * 8, hipMemcpyHostToDevice, ctx->s_mpc));
  HB_HIP(hipMemcpyAsync(ctx->b.u, u, B * N * HB_NU * 8, hipMemcpyHostToDevice, ctx->s_mpc));
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

// Backward sweep of `B` instances: small launches take four wavefronts per instance (k_ric_bwd4), large ones the one-wavefront form
// (eight sweeps per CU are then the better use of the chip).  hb_config.reserved = 101 / 104 forces one / four (tests, tuning).
// `concurrent` = instances whose sweeps may be in flight at the same time (the whole batch when its instance ranges free-run on their
// own streams): what decides is how many sweeps share the chip, not the size of this launch.
static void launch_ric_bwd(hb_ctx* ctx, const Batch& b, int B, int concurrent, hipStream_t s) {
  const int sel = ctx->hconfig.debug_stop;
  const bool four = sel == 104 || (HB_ABLATE_ON && ((sel >= 24 && sel <= 27) || sel == 199)) || (sel != 101 && !(HB_ABLATE_ON && sel != 0 && sel != 198) && concurrent <= kRicBwd4MaxBatch);
  if (four) hipLaunchKernelGGL(k_ric_bwd4, dim3(B), dim3(256), 0, s, b, sel);
  else hipLaunchKernelGGL(k_ric_bwd, dim3(B), dim3(64), 0, s, b, sel);
}

// LQ approximation: trips of tlen nodes per wavefront (k_lq_trip).  Longer trips fill the lanes of the value phase better (16 nodes:
// all 64), shorter ones keep small batches spread over the chip and balance them finer: the longest trip
// that still gives every wavefront slot of the chip (12 per CU) four trips of the CONCURRENT batch — 16 nodes from 2048 instances up, 8 at
// 1024, 4 at 512 (512 x 108 on two ranges, updates/s: one-node kernel 329.7 k, 4 nodes 325.0 k, 8: 316.9 k, 16: 305.2 k).  The result does not depend on the
// choice.  hb_config.reserved = 120 + s forces 2^s, 130 + L any length L <= 16 (lengths that are no power of two measured within the
// noise of the powers of two at 512, 1024 and 4096 instances); 129 the one-node-per-wavefront kernel of rounds 1-5 (k_lq: cooperative leg
// pass; A / B only, differs from the trips by rounding).
constexpr int kLqTripsPerSlot = 4;
static int lq_trip_len(const hb_ctx* ctx, int concurrent) {
  const int sel = ctx->hconfig.debug_stop;
  if (sel >= 120 && sel <= 124) return 1 << (sel - 120);
  if (sel >= 131 && sel <= 146) return sel - 130;   // any trip length 1..16 (launch-geometry sweeps)
  const long slots = 12L * ctx->n_cu;
  for (int sh = 4; sh > 0; --sh)
    if (long(concurrent) * ((ctx->Nmax + (1 << sh) - 1) >> sh) >= kLqTripsPerSlot * slots) return 1 << sh;
  return 1;
}
static void launch_lq(hb_ctx* ctx, const Batch& b, int B, int concurrent, hipStream_t s) {
  if (ctx->hconfig.debug_stop == 129) { hipLaunchKernelGGL(k_lq, dim3(ctx->Nmax, B), dim3(64), 0, s, b, ctx->dmodel, ctx->dconfig); return; }
  const int len = lq_trip_len(ctx, concurrent);
  const int ntrip = (ctx->Nmax + len - 1) / len;
  hipLaunchKernelGGL(k_lq_trip, dim3(unsigned(ntrip) * B), dim3(64), 0, s, b, ctx->dmodel, ctx->dconfig, len);
}

// Forward sweep: the wave form while the batch leaves a SIMD one wavefront (hb_config.reserved = 111 / 114 force the row / the wave form)
static void launch_ric_fwd(hb_ctx* ctx, const Batch& b, int B, int concurrent, hipStream_t s) {
  const int sel = ctx->hconfig.debug_stop;
  if (sel == 114 || (sel != 111 && concurrent <= kRicFwdWaveMaxBatch)) hipLaunchKernelGGL(k_ric_fwd_w, dim3(B), dim3(64), 0, s, b);
  else hipLaunchKernelGGL(k_ric_fwd, dim3(B), dim3(64), 0, s, b);
}

// The SQP iterations of the instances of b on s; `timed`: iteration 0 records the phase events ev[EV_LQ_BEGIN .. EV_LS_END].
static int32_t enqueue_sqp(hb_ctx* ctx, const Batch& b, hipStream_t s, bool timed) {
  const int B = b.B, N = ctx->Nmax;
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
    hipLaunchKernelGGL(k_ls_eval, dim3((B * N + 63) / 64), dim3(64), 0, s, b, ctx->dmodel, ctx->dconfig, 1.0);
    hipLaunchKernelGGL(k_ls_decide, dim3(B), dim3(64), 0, s, b, ctx->dconfig, 1.0);
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
        hipLaunchKernelGGL(k_ls_tail_eval, dim3((B * N + 63) / 64, n_alpha), dim3(64), 0, s, b, ctx->dmodel, ctx->dconfig, a_win,
                           ctx->config.alpha_decay, ctx->config.alpha_min);
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
  HB_TRY(enqueue_sqp(ctx, ctx->b, ctx->s_mpc, true));
  std::lock_guard<std::mutex> lk(ctx->mtx);
  ctx->timed = true;
  ctx->stats.n_mpc_solves += ctx->B;
  ctx->mpc_solved_epoch = ctx->mpc_tables_epoch;
  return HB_OK;
}

int32_t hb_mpc_solve(hb_ctx* ctx, const double* x0) {
  if (ctx) lazy_join(ctx);
  if (!ctx) return HB_ERR_ARG;
  if (!ctx->refs_set || !ctx->traj_set) {
    ctx->err = "hb_mpc_solve: call hb_mpc_set_references and hb_mpc_reset/hb_mpc_set_trajectory first";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  if (x0) {
    HB_HIP(hipMemcpyAsync(ctx->b.x0, x0, size_t(ctx->B) * HB_NX * 8, hipMemcpyHostToDevice, ctx->s_mpc));
    HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  }
  return mpc_solve_batch(ctx);
}

int32_t hb_mpc_get_solution(hb_ctx* ctx, int32_t i0, int32_t cnt, double* x, double* u) {
  if (ctx) lazy_join(ctx);
  if (!ctx || i0 < 0 || cnt <= 0 || i0 + cnt > ctx->B) return HB_ERR_ARG;
  const size_t N = ctx->Nmax;
  HB_HIP(hipSetDevice(ctx->device));
  if (x) HB_HIP(hipMemcpyAsync(x, ctx->b.x + i0 * (N + 1) * HB_NX, cnt * (N + 1) * HB_NX * 8, hipMemcpyDeviceToHost, ctx->s_mpc));
  if (u) HB_HIP(hipMemcpyAsync(u, ctx->b.u + i0 * N * HB_NU, cnt * N * HB_NU * 8, hipMemcpyDeviceToHost, ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  return HB_OK;
}

int32_t hb_mpc_get_step(hb_ctx* ctx, double* dx, double* du) {
  if (ctx) lazy_join(ctx);
  if (!ctx) return HB_ERR_ARG;
  const size_t B = ctx->B, N = ctx->Nmax;
  HB_HIP(hipSetDevice(ctx->device));
  if (dx) HB_HIP(hipMemcpyAsync(dx, ctx->b.dx, B * (N + 1) * HB_NX * 8, hipMemcpyDeviceToHost, ctx->s_mpc));
  if (du) HB_HIP(hipMemcpyAsync(du, ctx->b.du, B * N * HB_NU * 8, hipMemcpyDeviceToHost, ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  return HB_OK;
}

int32_t hb_mpc_get_performance(hb_ctx* ctx, double* perf) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !perf) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
  HB_HIP(hipMemcpyAsync(perf, ctx->b.perf, size_t(ctx->B) * 4 * 8, hipMemcpyDeviceToHost, ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  return HB_OK;
}

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
static void launch_publish(const Batch& b, const WbcBatch& w, hipStream_t s) {
  const size_t cnt = b.B, N = b.Nmax;
  const size_t nx = cnt * (N + 1) * HB_NX, nu = cnt * N * HB_NU, nt = cnt * (N + 1), nm = cnt * N, nn = cnt;
  const size_t total = nx + nu + nt + nm + nn;
  const unsigned blocks = unsigned(std::min<size_t>((total + 256 * 4 - 1) / (256 * 4), 8192));   // four elements per thread, grid-stride beyond
  hipLaunchKernelGGL(k_publish, dim3(blocks), dim3(256), 0, s, b.x, b.u, b.t, b.mode, b.n_nodes, w.px, w.pu, w.pt, w.pmode, w.pn, nx, nu, nt, nm, nn);
}

int32_t hb_mpc_publish(hb_ctx* ctx) {
  if (ctx) lazy_join(ctx);
  if (!ctx) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
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
  if (ctx->config.wbc_type == 1 && ctx->wbc_cert)  // (in a range graph: chosen at capture, hb_hwbc_set_certificate re-captures)
    hipLaunchKernelGGL(k_hwbc_cert, dim3(w.B), dim3(64), (HoLdsDev::total + HoCertLds::total) * sizeof(double), s, w, ctx->dmodel, ctx->dconfig,
                       ctx->hcert_buf + size_t(i0) * HB_HWBC_LEVELS * HB_HWBC_CERT_SIZE, ctx->hxlev_buf + size_t(i0) * HB_HWBC_LEVELS * HB_NWBC,
                       ctx->hslack_buf + size_t(i0) * HB_HWBC_NINEQ_MAX, ctx->hdual_buf + size_t(i0) * HB_HWBC_LEVELS * HB_HWBC_NINEQ_MAX);
  else if (ctx->config.wbc_type == 1)
    hipLaunchKernelGGL(k_hwbc, dim3(w.B), dim3(64), HoLdsDev::total * sizeof(double), s, w, ctx->dmodel, ctx->dconfig);
  else if (ctx->wbc_cert)  // (in a range graph: chosen at capture, hb_wbc_set_certificate re-captures)
    hipLaunchKernelGGL(k_wbc_cert, dim3(w.B), dim3(64), 0, s, w, ctx->dmodel, ctx->dconfig, ctx->cert_buf + size_t(i0) * HB_WBC_CERT_SIZE,
                       ctx->dual_buf + size_t(i0) * HB_WBC_NCONS_MAX);
  else
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
  if (ctx) lazy_join(ctx);
  if (!ctx || ((t_now == nullptr) != (rbd == nullptr))) return HB_ERR_ARG;
  if (!ctx->w.policy_valid) {
    ctx->err = "hb_wbc_update: no published policy (hb_mpc_publish)";
    return HB_ERR_STATE;
  }
  const size_t B = ctx->B;
  WbcBatch& w = ctx->w;
  hipStream_t s = ctx->s_wbc;
  HB_HIP(hipSetDevice(ctx->device));
  if (t_now) {  // otherwise: the device-resident time / rbd (hb_set_resident_inputs, hb_estimator_update, hb_plant_step)
    HB_HIP(hipMemcpyAsync(w.t_now, t_now, B * 8, hipMemcpyHostToDevice, s));
    HB_HIP(hipMemcpyAsync(w.rbd, rbd, B * HB_NRBD * 8, hipMemcpyHostToDevice, s));
  }
  if (walk_flag) HB_HIP(hipMemcpyAsync(w.walk, walk_flag, B * sizeof(int), hipMemcpyHostToDevice, s));
  HB_TRY(wbc_launch(ctx, true));
  if (sol) HB_HIP(hipMemcpyAsync(sol, w.sol, B * HB_NWBC * 8, hipMemcpyDeviceToHost, s));
  if (x_des) HB_HIP(hipMemcpyAsync(x_des, w.xdes, B * HB_NX * 8, hipMemcpyDeviceToHost, s));
  if (u_des) HB_HIP(hipMemcpyAsync(u_des, w.udes, B * HB_NU * 8, hipMemcpyDeviceToHost, s));
  if (planned_mode) HB_HIP(hipMemcpyAsync(planned_mode, w.mode, B * sizeof(int), hipMemcpyDeviceToHost, s));
  if (status) HB_HIP(hipMemcpyAsync(status, w.status, B * sizeof(int), hipMemcpyDeviceToHost, s));
  HB_HIP(hipStreamSynchronize(s));
  return HB_OK;
}

int32_t hb_wbc_update_direct(hb_ctx* ctx, const double* x_des, const double* u_des, const double* rbd, const int32_t* mode,
                             const int32_t* stance_flag, double dt, double* sol, int32_t* status) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !x_des || !u_des || !rbd || !mode) return HB_ERR_ARG;
  const size_t B = ctx->B;
  WbcBatch& w = ctx->w;
  hipStream_t s = ctx->s_wbc;
  HB_HIP(hipSetDevice(ctx->device));
  HB_HIP(hipMemcpyAsync(w.xdes, x_des, B * HB_NX * 8, hipMemcpyHostToDevice, s));
  HB_HIP(hipMemcpyAsync(w.udes, u_des, B * HB_NU * 8, hipMemcpyHostToDevice, s));
  HB_HIP(hipMemcpyAsync(w.rbd, rbd, B * HB_NRBD * 8, hipMemcpyHostToDevice, s));
  HB_HIP(hipMemcpyAsync(w.mode, mode, B * sizeof(int), hipMemcpyHostToDevice, s));
  if (stance_flag) HB_HIP(hipMemcpyAsync(w.stance, stance_flag, B * sizeof(int), hipMemcpyHostToDevice, s));
  else HB_HIP(hipMemsetAsync(w.stance, 0, B * sizeof(int), s));
  HB_TRY(wbc_launch(ctx, false));
  if (sol) HB_HIP(hipMemcpyAsync(sol, w.sol, B * HB_NWBC * 8, hipMemcpyDeviceToHost, s));
  if (status) HB_HIP(hipMemcpyAsync(status, w.status, B * sizeof(int), hipMemcpyDeviceToHost, s));
  HB_HIP(hipStreamSynchronize(s));
  return HB_OK;
}

int32_t hb_set_resident_inputs(hb_ctx* ctx, const double* x0, const double* t_now, const double* rbd, const int32_t* walk_flag) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !x0 || !t_now || !rbd) return HB_ERR_ARG;
  const size_t B = ctx->B;
  HB_HIP(hipSetDevice(ctx->device));
  HB_HIP(hipMemcpy(ctx->b.x0, x0, B * HB_NX * 8, hipMemcpyHostToDevice));
  HB_HIP(hipMemcpy(ctx->w.t_now, t_now, B * 8, hipMemcpyHostToDevice));
  HB_HIP(hipMemcpy(ctx->w.rbd, rbd, B * HB_NRBD * 8, hipMemcpyHostToDevice));
  if (walk_flag) HB_HIP(hipMemcpy(ctx->w.walk, walk_flag, B * sizeof(int), hipMemcpyHostToDevice));
  return HB_OK;
}

int32_t hb_set_resident_time(hb_ctx* ctx, const double* t_now) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !t_now) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
  return stage_upload(ctx, ST_TNOW, ctx->w.t_now, t_now, size_t(ctx->B) * 8, ctx->s_wbc);  // no device synchronisation
}

int32_t hb_set_resident_x0_sequence(hb_ctx* ctx, int32_t n_seq, const double* x0_seq) {
  if (ctx) lazy_join(ctx);
  if (!ctx || n_seq < 0 || (n_seq > 0 && !x0_seq)) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
  ctx->n_seq = 0;
  ctx->seq_idx = 0;
  ++ctx->graph_epoch;
  if (n_seq == 0) return HB_OK;
  const size_t bytes = size_t(n_seq) * ctx->B * HB_NX * 8;
  if (hipMalloc(reinterpret_cast<void**>(&ctx->x0_seq), bytes) != hipSuccess) {
    ctx->err = "hb_set_resident_x0_sequence: hipMalloc failed";
    return HB_ERR_DEVICE;
  }
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
  const Batch b = batch_view(ctx->b, i0, cnt);
  const WbcBatch w = wbc_view(ctx->w, ctx->Nmax, i0, cnt);
  HB_TRY(enqueue_sqp(ctx, b, s, false));
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
}

int32_t hb_step_resident(hb_ctx* ctx, double dt) {
  if (!ctx) return HB_ERR_ARG;
  if (!ctx->refs_set || !ctx->traj_set) {
    ctx->err = "hb_step_resident: references / trajectory not initialised";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  const double* x0_next = nullptr;
  const int seq_slot = ctx->seq_idx;
  if (ctx->n_seq > 0) {
    x0_next = ctx->x0_seq + size_t(ctx->seq_idx) * ctx->B * HB_NX;
    ctx->seq_idx = (ctx->seq_idx + 1) % ctx->n_seq;
  }
  if (ctx->n_chunks <= 1) {
    lazy_join(ctx);
    if (x0_next) HB_HIP(hipMemcpyAsync(ctx->b.x0, x0_next, size_t(ctx->B) * HB_NX * 8, hipMemcpyDeviceToDevice, ctx->s_mpc));
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
      if (x0_next)
        HB_HIP(hipMemcpyAsync(ctx->b.x0 + size_t(i0) * HB_NX, x0_next + size_t(i0) * HB_NX, size_t(cnt) * HB_NX * 8, hipMemcpyDeviceToDevice, s));
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
  if (ctx->n_chunks <= 1) {  // one stream: the four calls themselves (enqueue-only forms)
    HB_TRY(hb_set_resident_time(ctx, t_now));
    HB_TRY(hb_estimator_update(ctx, dt_est, quat, ang_vel_local, lin_acc_local, joint_pos, joint_vel, contact_flag, 1, nullptr, nullptr));
    HB_TRY(hb_refgen_update(ctx, t_now, horizon, nullptr, cmd_vel, nullptr));
    return hb_step_resident(ctx, dt_wbc);
  }
  if (!ctx->est_ready || !ctx->rg_ready || !ctx->refs_set || !ctx->traj_set) {
    ctx->err = "hb_tick_resident: estimator / reference generation / references / trajectory not initialised";
    return HB_ERR_STATE;
  }
  for (int v : ctx->rg_have_schedule)
    if (!v && !ctx->gait_on) {
      ctx->err = "hb_tick_resident: an instance has no mode schedule (hb_refgen_set_schedule)";
      return HB_ERR_STATE;
    }
  HB_HIP(hipSetDevice(ctx->device));
  const size_t B = ctx->B;
  hb_ctx::TickUpload& up = ctx->up;
  if (!ctx->s_up) {
    HB_HIP(hipStreamCreateWithFlags(&ctx->s_up, hipStreamNonBlocking));
    HB_HIP(hipEventCreateWithFlags(&ctx->ev_up, hipEventDisableTiming));
    for (auto& ev : ctx->ev_consumed) HB_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HB_HIP(dalloc(ctx, &up.quat, B * 4)); HB_HIP(dalloc(ctx, &up.w, B * 3)); HB_HIP(dalloc(ctx, &up.a, B * 3));
    HB_HIP(dalloc(ctx, &up.qj, B * 10)); HB_HIP(dalloc(ctx, &up.qdj, B * 10)); HB_HIP(dalloc(ctx, &up.contact, B * 4));
    HB_HIP(dalloc(ctx, &up.tnow, B)); HB_HIP(dalloc(ctx, &up.t0, B)); HB_HIP(dalloc(ctx, &up.cmd, B * 4));
  }
  bool fork;
  HB_TRY(fork_ranges(ctx, fork));
  // this tick's host inputs: one upload, after every range has read the previous tick's
  hipStream_t su = ctx->s_up;
  for (int c = 0; c < ctx->consumed_pending; ++c) HB_HIP(hipStreamWaitEvent(su, ctx->ev_consumed[c], 0));
  const void* const dst[6] = {up.quat, up.w, up.a, up.qj, up.qdj, up.contact};
  const void* const src[6] = {quat, ang_vel_local, lin_acc_local, joint_pos, joint_vel, contact_flag};
  HB_TRY(upload_sensors(ctx, dst, src, true, su));
  HB_TRY(stage_upload(ctx, ST_TNOW, up.tnow, t_now, B * 8, su));
  HB_TRY(stage_upload(ctx, ST_T0, up.t0, t_now, B * 8, su));
  HB_TRY(stage_upload(ctx, ST_CMD, up.cmd, cmd_vel, B * 4 * 8, su));
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
    const Batch b = batch_view(ctx->b, i0, cnt);
    const WbcBatch w = wbc_view(ctx->w, ctx->Nmax, i0, cnt);
    // controller time + estimator -> resident rbd state and observation of the range
    HB_HIP(hipMemcpyAsync(w.t_now, up.tnow + i0, size_t(cnt) * 8, hipMemcpyDeviceToDevice, s));
    EstBatch e = est_view(est, i0, cnt);
    e.res_rbd = w.rbd;
    e.res_x0 = b.x0;
    launch_estimator(ctx, e, dt_est, s);
    // reference generation at the new time (the grid that is about to be replaced is kept for the warm start)
    HB_TRY(launch_grid_save(ctx, b, true, 0, cnt, s));
    launch_refgen(ctx, b, refgen_view(rg, i0, cnt), i0, horizon, s);
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
  if (ctx) lazy_join(ctx);
  if (!ctx || n_chunks < 1 || n_chunks > kMaxRanges) return HB_ERR_ARG;
  HB_TRY(hb_sync(ctx));
  ctx->n_chunks = n_chunks;
  ctx->graph_disabled = false;  // a new set of ranges gets a new chance to capture
  ++ctx->graph_epoch;
  return HB_OK;
}

int32_t hb_get_wbc_solution(hb_ctx* ctx, double* sol, int32_t* status) {
  if (ctx) lazy_join(ctx);
  if (!ctx) return HB_ERR_ARG;
  const size_t B = ctx->B;
  HB_HIP(hipSetDevice(ctx->device));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  if (sol) HB_HIP(hipMemcpy(sol, ctx->w.sol, B * HB_NWBC * 8, hipMemcpyDeviceToHost));
  if (status) HB_HIP(hipMemcpy(status, ctx->w.status, B * sizeof(int), hipMemcpyDeviceToHost));
  return HB_OK;
}

int32_t hb_wbc_set_certificate(hb_ctx* ctx, int32_t enable) {
  if (ctx) lazy_join(ctx);
  if (!ctx || enable < 0 || enable > 1) return HB_ERR_ARG;
  if (enable && ctx->config.wbc_type != 0) {
    ctx->err = "hb_wbc_set_certificate: the KKT certificate is defined for WeightedWbc only, not for HierarchicalWbc (wbc_type = 1)";
    return HB_ERR_ARG;
  }
  if (bool(enable) == ctx->wbc_cert) return HB_OK;
  HB_HIP(hipSetDevice(ctx->device));
  HB_TRY(hb_sync(ctx));
  if (enable && !ctx->cert_buf) {
    HB_HIP(dalloc(ctx, &ctx->cert_buf, size_t(ctx->B) * HB_WBC_CERT_SIZE));
    HB_HIP(dalloc(ctx, &ctx->dual_buf, size_t(ctx->B) * HB_WBC_NCONS_MAX));
  }
  ctx->wbc_cert = enable != 0;
  ++ctx->graph_epoch;  // captured range graphs hold the other WBC kernel
  return HB_OK;
}

int32_t hb_wbc_get_certificate(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, double* cert, double* dual) {
  if (ctx) lazy_join(ctx);
  if (!ctx || inst_begin < 0 || inst_count < 0 || inst_begin > ctx->B || inst_count > ctx->B - inst_begin) return HB_ERR_ARG;
  if (!ctx->cert_last || ctx->config.wbc_type != 0) {  // (a HierarchicalWbc context keeps its certificates elsewhere: hb_hwbc_get_certificate)
    ctx->err = "hb_wbc_get_certificate: certificates were off at the last WBC call (hb_wbc_set_certificate)";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  if (cert && inst_count)
    HB_HIP(hipMemcpy(cert, ctx->cert_buf + size_t(inst_begin) * HB_WBC_CERT_SIZE, size_t(inst_count) * HB_WBC_CERT_SIZE * 8, hipMemcpyDeviceToHost));
  if (dual && inst_count)
    HB_HIP(hipMemcpy(dual, ctx->dual_buf + size_t(inst_begin) * HB_WBC_NCONS_MAX, size_t(inst_count) * HB_WBC_NCONS_MAX * 8, hipMemcpyDeviceToHost));
  return HB_OK;
}

int32_t hb_hwbc_set_certificate(hb_ctx* ctx, int32_t enable) {
  if (ctx) lazy_join(ctx);
  if (!ctx || enable < 0 || enable > 1) return HB_ERR_ARG;
  if (ctx->config.wbc_type != 1) {
    ctx->err = "hb_hwbc_set_certificate: the per-level certificate is defined for HierarchicalWbc (wbc_type = 1) only; WeightedWbc has hb_wbc_set_certificate";
    return HB_ERR_ARG;
  }
  if (bool(enable) == ctx->wbc_cert) return HB_OK;
  HB_HIP(hipSetDevice(ctx->device));
  HB_TRY(hb_sync(ctx));
  if (enable && !ctx->hcert_buf) {
    HB_HIP(dalloc(ctx, &ctx->hcert_buf, size_t(ctx->B) * HB_HWBC_LEVELS * HB_HWBC_CERT_SIZE));
    HB_HIP(dalloc(ctx, &ctx->hxlev_buf, size_t(ctx->B) * HB_HWBC_LEVELS * HB_NWBC));
    HB_HIP(dalloc(ctx, &ctx->hslack_buf, size_t(ctx->B) * HB_HWBC_NINEQ_MAX));
    HB_HIP(dalloc(ctx, &ctx->hdual_buf, size_t(ctx->B) * HB_HWBC_LEVELS * HB_HWBC_NINEQ_MAX));
  }
  ctx->wbc_cert = enable != 0;
  ++ctx->graph_epoch;  // captured range graphs hold the other WBC kernel
  return HB_OK;
}

int32_t hb_hwbc_get_certificate(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, double* cert, double* x_levels, double* slack0,
                                double* dual) {
  if (ctx) lazy_join(ctx);
  if (!ctx || inst_begin < 0 || inst_count < 0 || inst_begin > ctx->B || inst_count > ctx->B - inst_begin) return HB_ERR_ARG;
  if (ctx->config.wbc_type != 1 || !ctx->cert_last) {
    ctx->err = "hb_hwbc_get_certificate: certificates were off at the last WBC call (hb_hwbc_set_certificate)";
    return HB_ERR_STATE;
  }
  HB_HIP(hipSetDevice(ctx->device));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  const size_t i0 = size_t(inst_begin), n = size_t(inst_count);
  const size_t nc = HB_HWBC_LEVELS * HB_HWBC_CERT_SIZE, nx = HB_HWBC_LEVELS * HB_NWBC, nd = HB_HWBC_LEVELS * HB_HWBC_NINEQ_MAX;
  if (cert && n) HB_HIP(hipMemcpy(cert, ctx->hcert_buf + i0 * nc, n * nc * 8, hipMemcpyDeviceToHost));
  if (x_levels && n) HB_HIP(hipMemcpy(x_levels, ctx->hxlev_buf + i0 * nx, n * nx * 8, hipMemcpyDeviceToHost));
  if (slack0 && n) HB_HIP(hipMemcpy(slack0, ctx->hslack_buf + i0 * HB_HWBC_NINEQ_MAX, n * HB_HWBC_NINEQ_MAX * 8, hipMemcpyDeviceToHost));
  if (dual && n) HB_HIP(hipMemcpy(dual, ctx->hdual_buf + i0 * nd, n * nd * 8, hipMemcpyDeviceToHost));
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
  if (ctx) lazy_join(ctx);
  if (!ctx) return HB_ERR_ARG;
  if (inst_begin < 0 || inst_count <= 0 || inst_begin > ctx->B || inst_count > ctx->B - inst_begin) {
    ctx->err = "hb_mpc_get_certificate: instance range outside the batch";
    return HB_ERR_ARG;
  }
  HB_TRY(mpc_records_current(ctx, "hb_mpc_get_certificate"));
  HB_HIP(hipSetDevice(ctx->device));
  const size_t B = ctx->B, N = ctx->Nmax, i0 = size_t(inst_begin), cnt = size_t(inst_count);
  MpcCertBuf& m = ctx->mcert;
  if (!m.node) {
    HB_HIP(dalloc(ctx, &m.node, B * N * CertNode::size));
    HB_HIP(dalloc(ctx, &m.costate, B * (N + 1) * HB_NX));
    HB_HIP(dalloc(ctx, &m.cert, B * MPC_CERT_SIZE));
    HB_HIP(dalloc(ctx, &m.util, B * N * 12));
  }
  const Batch b = batch_view(ctx->b, inst_begin, inst_count);
  const MpcCertBuf v{m.node + i0 * N * CertNode::size, m.costate + i0 * (N + 1) * HB_NX, m.cert + i0 * MPC_CERT_SIZE, m.util + i0 * N * 12};
  hipStream_t s = ctx->s_mpc;
  hipLaunchKernelGGL(k_mpc_cert_nodes, dim3(ctx->Nmax, inst_count), dim3(64), 0, s, b, v);
  hipLaunchKernelGGL(k_mpc_cert_sweep, dim3(inst_count), dim3(64), 0, s, b, v);
  HB_HIP(hipGetLastError());
  if (cert) HB_HIP(hipMemcpyAsync(cert, v.cert, cnt * MPC_CERT_SIZE * 8, hipMemcpyDeviceToHost, s));
  if (costate) HB_HIP(hipMemcpyAsync(costate, v.costate, cnt * (N + 1) * HB_NX * 8, hipMemcpyDeviceToHost, s));
  if (u_til) HB_HIP(hipMemcpyAsync(u_til, v.util, cnt * N * 12 * 8, hipMemcpyDeviceToHost, s));
  HB_HIP(hipStreamSynchronize(s));
  return HB_OK;
}

int32_t hb_mpc_get_lq(hb_ctx* ctx, int32_t inst, double* A, double* B, double* b, double* Q, double* P, double* R, double* q, double* r,
                      int32_t* n_til) {
  if (ctx) lazy_join(ctx);
  if (!ctx) return HB_ERR_ARG;
  if (inst < 0 || inst >= ctx->B) {
    ctx->err = "hb_mpc_get_lq: instance outside the batch";
    return HB_ERR_ARG;
  }
  HB_TRY(mpc_records_current(ctx, "hb_mpc_get_lq"));
  HB_HIP(hipSetDevice(ctx->device));
  const size_t N = ctx->Nmax;
  std::vector<double> recs(N * REC_SIZE);
  int n = 0;
  HB_HIP(hipMemcpyAsync(&n, ctx->b.n_nodes + inst, sizeof(int), hipMemcpyDeviceToHost, ctx->s_mpc));
  HB_HIP(hipMemcpyAsync(recs.data(), ctx->b.recs + size_t(inst) * N * REC_SIZE, recs.size() * 8, hipMemcpyDeviceToHost, ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  n = std::max(0, std::min(n, ctx->Nmax));
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

int32_t hb_get_wbc_iterations(hb_ctx* ctx, int32_t* iters) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !iters) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  HB_HIP(hipMemcpy(iters, ctx->w.iters, size_t(ctx->B) * sizeof(int), hipMemcpyDeviceToHost));
  return HB_OK;
}

int32_t hb_get_stats(hb_ctx* ctx, hb_stats* out) {
  if (ctx) lazy_join(ctx);
  if (!ctx || !out) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  float ms = 0;
  if (ctx->timed) {
    if (hipEventElapsedTime(&ms, ctx->ev[EV_LQ_BEGIN], ctx->ev[EV_LQ_END]) == hipSuccess) ctx->stats.ms_lq = ms;
    if (hipEventElapsedTime(&ms, ctx->ev[EV_LQ_END], ctx->ev[EV_RIC_BWD_END]) == hipSuccess) ctx->stats.ms_riccati_bwd = ms;
    if (hipEventElapsedTime(&ms, ctx->ev[EV_RIC_BWD_END], ctx->ev[EV_RIC_FWD_END]) == hipSuccess) ctx->stats.ms_riccati_fwd = ms;
    if (hipEventElapsedTime(&ms, ctx->ev[EV_RIC_FWD_END], ctx->ev[EV_LS_END]) == hipSuccess) ctx->stats.ms_linesearch = ms;
    if (hipEventElapsedTime(&ms, ctx->ev[EV_LQ_BEGIN], ctx->ev[EV_LS_END]) == hipSuccess) ctx->stats.ms_mpc_total = ms;
  }
  if (ctx->stats.n_wbc_solves > 0 && hipEventElapsedTime(&ms, ctx->ev[EV_WBC_BEGIN], ctx->ev[EV_WBC_END]) == hipSuccess) ctx->stats.ms_wbc = ms;
  if (ctx->stats.n_wbc_solves > 0) {
    std::vector<int> st(ctx->B);
    HB_HIP(hipMemcpy(st.data(), ctx->w.status, size_t(ctx->B) * sizeof(int), hipMemcpyDeviceToHost));
    for (int& v : ctx->stats.n_status) v = 0;
    for (int v : st)
      if (v >= 0 && v < 4) ctx->stats.n_status[v]++;
  }
  *out = ctx->stats;
  return HB_OK;
}

// ---- unit-level entry points ---------------------------------------------------------------------------
int32_t hb_eval_flow_map(hb_ctx* ctx, int32_t n, const double* x, const double* u, double* f, double* dfdx, double* dfdu) {
  if (ctx) lazy_join(ctx);
  if (!ctx || n <= 0 || !x || !u || !f) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
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
  if (ctx) lazy_join(ctx);
  if (!ctx || n <= 0 || !x || !u || !pos || !vel) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
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
  if (ctx) lazy_join(ctx);
  if (!ctx || n <= 0 || !rbd) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
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
  if (ctx) lazy_join(ctx);
  if (!ctx || n <= 0 || !q16 || !leg || !des_pos || !R_des || !out5) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
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

int32_t hb_hoqp_solve(hb_ctx* ctx, int32_t n_problems, int32_t n_vars, int32_t n_levels, const int32_t* m_eq, const int32_t* m_in,
                      const double* A, const double* b, const double* D, const double* f, double* x, double* slack, int32_t* status) {
  if (ctx) lazy_join(ctx);
  if (!ctx || n_problems <= 0 || n_vars <= 0 || n_vars > HQ_N || n_levels <= 0 || n_levels > HQ_L || !m_eq || !m_in || !A || !b || !D || !f ||
      !x || !slack || !status)
    return HB_ERR_ARG;
  for (int l = 0; l < n_levels; ++l)
    if (m_eq[l] < 0 || m_eq[l] > HQ_M || m_in[l] < 0 || m_in[l] > HQ_M) {
      ctx->err = "hb_hoqp_solve: at most 8 equality-type and 8 inequality rows per level";
      return HB_ERR_ARG;
    }
  HB_HIP(hipSetDevice(ctx->device));
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
  if (ctx) lazy_join(ctx);
  if (!ctx || !rbd || !x || n <= 0) return HB_ERR_ARG;
  HB_HIP(hipSetDevice(ctx->device));
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
  if (ctx) lazy_join(ctx);
  if (!ctx || n <= 0 || N <= 0 || nu <= 0 || nu > NU_T || n > ctx->B || N > ctx->Nmax) return HB_ERR_ARG;
  // pack stage data into node records on the host, run the same kernels the MPC uses
  const size_t Nm = ctx->Nmax;
  std::vector<double> recs(size_t(n) * Nm * REC_SIZE, 0.0);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < N; ++k) {
      double* rec = recs.data() + (size_t(i) * Nm + k) * REC_SIZE;
      const size_t sk = size_t(i) * N + k;
      for (int row = 0; row < 22; ++row) std::memcpy(rec + rec_A(row, 0), A + sk * 484 + row * 22, 22 * 8);
      for (int i = 0; i < 22; ++i)   // the record holds the upper triangle of Q~, packed
        for (int c = i; c < 22; ++c) rec[REC_QT + rec_Qidx(i, c)] = Q[sk * 484 + i * 22 + c];
      for (int row = 0; row < 22; ++row) rec[rec_b(row)] = bv[sk * 22 + row];
      std::memcpy(rec + REC_qT, q + sk * 22, 22 * 8);
      for (int row = 0; row < 22; ++row)
        for (int c = 0; c < nu; ++c) rec[rec_B(row, c)] = Bm[(sk * 22 + row) * nu + c];
      for (int a = 0; a < NU_T; ++a) {
        for (int c = 0; c < NU_T; ++c)
          rec[rec_R(a, c)] = (a < nu && c < nu) ? R[(sk * nu + a) * nu + c] : (a == c ? 1.0 : 0.0);
        if (a < nu) {
          std::memcpy(rec + rec_P(a, 0), P + (sk * nu + a) * 22, 22 * 8);
          rec[rec_r(a)] = r[sk * nu + a];
        }
      }
      rec[REC_META + 0] = double(nu);  // number of real inputs (the backward sweep picks its factor width from it)
      rec[REC_META + 1] = 0.0;
    }
  // The forward kernel reconstructs du through the projection data; for this unit entry point the reduced input
  // is returned directly, so run backward on the device and the (cheap) forward recursion on the host.
  HB_HIP(hipSetDevice(ctx->device));
  std::vector<int> nn(ctx->B, 1);
  for (int i = 0; i < n; ++i) nn[i] = N;
  HB_HIP(hipMemcpy(ctx->b.n_nodes, nn.data(), size_t(ctx->B) * sizeof(int), hipMemcpyHostToDevice));
  HB_HIP(hipMemcpy(ctx->b.recs, recs.data(), recs.size() * 8, hipMemcpyHostToDevice));
  launch_ric_bwd(ctx, ctx->b, n, n, ctx->s_mpc);
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  std::vector<double> gains(size_t(n) * Nm * GAIN_SIZE);
  HB_HIP(hipMemcpy(gains.data(), ctx->b.gains, gains.size() * 8, hipMemcpyDeviceToHost));
  ctx->refs_set = false;  // the batch buffers were clobbered
  for (int i = 0; i < n; ++i) {
    double xk[22];
    std::memcpy(xk, dx0 + size_t(i) * 22, 22 * 8);
    for (int k = 0; k < N; ++k) {
      const double* g = gains.data() + (size_t(i) * Nm + k) * GAIN_SIZE;
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

}  // extern "C"
