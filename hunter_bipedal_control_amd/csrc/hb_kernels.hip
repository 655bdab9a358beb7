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
#include "hb_contact.hpp"
#include "hb_joints.hpp"
#include "hb_sensors.hpp"
#include "hb_respawn.hpp"
#include "hb_scenario.hpp"
#include "hb_profiledraw.hpp"
#include "hb_fielddraw.hpp"
#include "hb_layout.hpp"
#include "hb_iterate.hpp"
#include "hb_wavectx.hpp"

using namespace hb;

namespace {

__global__ void k_set_x0(Batch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.B * HB_NX) return;
  const int inst = i / HB_NX, c = i % HB_NX;
  b.x[size_t(inst) * (b.Nmax + 1) * HB_NX + c] = b.x0[i];
}

// cold start of the instances the mask selects (all without one): hb_iterate.hpp cold_start_entry per (node, lane)
__global__ void k_cold_start(Batch b, const DevModel* __restrict__ M, const unsigned char* mask) {
  const int k = blockIdx.x, inst = blockIdx.y;
  const int lane = threadIdx.x;
  if (mask && !mask[inst]) return;
  if (k == 0 && lane == 0) { b.grid_dirty[inst] = 0; b.mpc_status[inst] = HB_INST_OK; }
  cold_start_entry(*M, b.n_nodes + inst, b.mode + size_t(inst) * b.Nmax, b.x0 + inst * HB_NX, k, lane, b.x + size_t(inst) * (b.Nmax + 1) * HB_NX,
                   b.u + size_t(inst) * b.Nmax * HB_NU);
}

// Warm start across MPC calls (hb_iterate.hpp warm_shift_entry): the previous call's iterate (xp, up on the grid tp / modep / np_nodes)
// is brought onto the new node tables; instances whose tables did not change are copied.
constexpr int kWarmShiftThreads = 256;
__global__ __launch_bounds__(kWarmShiftThreads) void k_warm_shift(Batch b, const DevModel* __restrict__ M) {
  // one thread per (node, entry index) of an instance, consecutive threads = consecutive entries, every lane of a wavefront has work (one
  // block per node used 44 of 64 lanes; the kernel is a chain of three dependent round trips per thread, so what it costs is wavefronts /
  // resident wavefronts).
  const int flat = blockIdx.x * kWarmShiftThreads + threadIdx.x, inst = blockIdx.y;
  const int k = flat / HB_NX, e = flat - k * HB_NX;
  const size_t N = b.Nmax;
  const WarmShiftInst w{b.Nmax, b.grid_dirty + inst, b.n_nodes + inst, b.t + size_t(inst) * (N + 1), b.mode + size_t(inst) * N, b.np_nodes + inst,
                        b.tp + size_t(inst) * (N + 1), b.modep + size_t(inst) * N, b.xp + size_t(inst) * (N + 1) * HB_NX, b.up + size_t(inst) * N * HB_NU,
                        b.x + size_t(inst) * (N + 1) * HB_NX, b.u + size_t(inst) * N * HB_NU};
  warm_shift_entry(*M, w, k, e);
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
  // (profiling build, LQT_VALUES_ONCE: the value phase runs once per trip, later launches re-use what it parked — the dense part alone on valid data)
  if (!(HB_ABLATE_ON && C->debug_stop == form::LQT_VALUES_ONCE && park[size_t(LqPark::n_feet / 4 * tlen) * 16] != 0.0)) {
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
  if (C->debug_stop == form::LQT_TRACE && blockIdx.x == 1000 && threadIdx.x == 0) {
    const long long* m = reinterpret_cast<const long long*>(lds + LqLds::total - 24);
    const long long t12 = __builtin_readcyclecounter();
    printf("lq value-phase trace (cycles): loads %lld | fwd sweep %lld | feet %lld | bwd joints %lld %lld %lld %lld %lld | stash %lld | wait %lld | value pass 0 %lld | 1 %lld | drain %lld\n",
           m[1] - m[0], m[2] - m[1], 0LL, m[3] - m[2], m[4] - m[3], m[5] - m[4], m[6] - m[5], m[7] - m[6], m[8] - m[7], m[9] - m[8], m[10] - m[9], m[11] - m[10], t12 - m[11]);
    printf("   value pass 1: stash reads %lld | point values %lld | contact point, sums %lld | hand-out %lld | park %lld\n", m[12] - m[10], m[13] - m[12], m[14] - m[13], m[15] - m[14], m[11] - m[15]);
  }
  if (C->debug_stop == form::LQT_TRACE) return;
#endif
  if (HB_ABLATE_ON && C->debug_stop >= form::LQT_VALUES && C->debug_stop <= form::LQT_VALUES_LEGS) return;   // profiling build: the value phase alone, or parts of it
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
    // (profiling build, LQT_ONE_RECORD: every node of a workgroup writes ONE record slot — the stores are issued, their lines stay in the L2)
    double* recp = b.recs + ((HB_ABLATE_ON && C->debug_stop == form::LQT_ONE_RECORD) ? size_t(blockIdx.x & 4095) : nd) * REC_SIZE;
    lq_node_dense(cx, *M, *C, in, lds, recp, [park_lds](int i) { return park_lds[i]; }, [xnext_lds](int i) { return xnext_lds[i]; });
    cx.sync();
  }
#endif
}

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
  // cycle-counter trace of one stage (tools/perf_quick.py --stop with RIC1_TRACE): the marks live in the slack words behind RicLds::flag, not in registers
  long long* t1_ = reinterpret_cast<long long*>(lds + RicLds::flag + 8);
#define HB_RIC1_MARK(i) if (dbg == form::RIC1_TRACE && blockIdx.x == 9 && k == 50 && cx.lane == 0) t1_[i] = __builtin_readcyclecounter();
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
    if (HB_ABLATE_ON && dbg == form::RIC1_STAGING) { if (k > 0) HB_RIC_FETCH(k - 1, l); continue; }  // profiling ablation: staging only
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
    if (HB_ABLATE_ON && (dbg == form::RIC1_GEMM1 || dbg == form::RIC1_GEMM2 || dbg == form::RIC1_FACTOR)) continue;
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
    if (dbg == form::RIC1_TRACE && blockIdx.x == 9 && k == 50 && cx.lane == 0)
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
#define HB_RIC4_MARK(i) if (dbg == form::RIC4_TRACE && blockIdx.x == 7 && k == 50) tr_[i] = __builtin_readcyclecounter();
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
    if (HB_ABLATE_ON && dbg == form::RIC4_STAGING) continue;   // profiling ablation: staging only
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
    if (HB_ABLATE_ON && dbg == form::RIC4_GEMM1) continue;   // ... + GEMM 1
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
    if (HB_ABLATE_ON && dbg == form::RIC4_GEMM2) continue;   // ... + GEMM 2
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
    if (HB_ABLATE_ON && dbg == form::RIC4_FACTOR) continue;   // ... + factor, solves | first part of GEMM 3
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
    if (dbg == form::RIC4_TRACE && blockIdx.x == 7 && k == 50 && (tid & 63) == 0)
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

// ---- KKT certificate of the stage QP (hb_mpccert.hpp), on demand: hb_mpc_get_certificate.  Work buffers of the instances of `b`.
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

// line search: value of trial point (x + alpha dx, u + alpha du).  Two forms: two lanes per node (the product) and one
// thread per node (k_ls_eval_node / k_ls_tail_eval_node, hb_config.reserved = LS_EVAL_NODE); they differ by rounding only.
// The full-step kernels also clear the list of refused instances k_ls_decide fills for the tail.
//
// Two lanes per node, 32 nodes per workgroup: what k_ls_eval and k_ls_tail_eval do for the node (inst, k) of the calling pair.  The
// pair's trial point goes to LDS, every second entry from each lane; the next node's trial state is only read once per entry (defect)
// and is formed from global memory there.  Both lanes of a pair call this together; lane 0 writes the three values to `out`.
__device__ __forceinline__ void ls_pair_node(const Batch& b, const DevModel& M, const DevConfig& C, double* lds, int inst, int k, double alpha,
                                             double* out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int p = threadIdx.x >> 1, h = threadIdx.x & 1;
  const size_t nd = size_t(inst) * b.Nmax + k;
  const size_t xo = (size_t(inst) * (b.Nmax + 1) + k) * HB_NX;
  double* x = lds + p * LS_PAIR_X;
  double* u = x + HB_NX;
  const WaveCtx cx;
  cx.sync();   // (a caller that loops: the partner's reads of the previous point come first)
#pragma unroll
  for (int t = 0; t < HB_NX / 2; ++t) {
    const int i = 2 * t + h;
    x[i] = b.x[xo + i] + alpha * b.dx[xo + i];
    u[i] = b.u[nd * HB_NU + i] + alpha * b.du[nd * HB_NU + i];
  }
  cx.sync();
  const double* tt = b.t + size_t(inst) * (b.Nmax + 1);
  const double* xn0 = b.x + xo + HB_NX;
  const double* dxn = b.dx + xo + HB_NX;
  double o3[3];
  node_value_pair(M, C, x, u, lds + 32 * LS_PAIR_X + threadIdx.x * LS_PAIR_FT, h, [xn0, dxn, alpha](int i) { return xn0[i] + alpha * dxn[i]; },
                  b.xref + nd * HB_NX, b.swing + nd * 24, tt[k + 1] - tt[k], b.mode[nd], o3);
  if (h == 0) {
    out[0] = o3[0];
    out[1] = o3[1];
    out[2] = o3[2];
  }
#endif
}
__global__ __launch_bounds__(64, 2) void k_ls_eval(Batch b, LsList ls, const DevModel* __restrict__ M, const DevConfig* __restrict__ C,
                                                   double alpha) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (blockIdx.x == 0 && threadIdx.x == 0) *ls.count = 0;
  const int gid = blockIdx.x * 32 + (threadIdx.x >> 1);
  const int inst = gid / b.Nmax, k = gid % b.Nmax;
  if (inst >= b.B) return;
  if (b.accepted[inst] || k >= b.n_nodes[inst]) return;
  __shared__ double lds[LS_PAIR_LDS];
  ls_pair_node(b, *M, *C, lds, inst, k, alpha, b.partial + (size_t(inst) * b.Nmax + k) * 3);
#endif
}

// one thread per node
__global__ __launch_bounds__(64) void k_ls_eval_node(Batch b, LsList ls, const DevModel* __restrict__ M, const DevConfig* __restrict__ C,
                                                double alpha) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid == 0) *ls.count = 0;
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

__global__ __launch_bounds__(64) void k_ls_decide(Batch b, LsList ls, const DevConfig* __restrict__ C, double alpha) {
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
    if (lane == 0) {
      b.ls_norm[inst * 2] = sqrt(nx2);
      b.ls_norm[inst * 2 + 1] = sqrt(nu2);
      ls.inst[atomicAdd(ls.count, 1)] = inst;   // the tail's work list (in no particular order)
    }
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
// EVALUATED SIDE BY SIDE (k_ls_tail_eval: k_ls_eval once per step size, per-node partials; the same node evaluation and the same
// summation order as k_ls_eval + k_ls_decide) and a second kernel walks the sequence with exactly the sequential rules (k_ls_tail_decide):
// identical decisions, but the launch takes ONE trial's time instead of up to 13 in a row (an instance that walks down to
// alpha_min used to hold the whole batch back: 2.4 ms of line search per step in the backtracking figure), and without the loop over
// the step sizes around the node evaluation the thread-per-node kernel does not spill (its one-launch form carried 476 B / lane of scratch).
// The product's form walks the list of refused instances k_ls_decide left: a bounded grid whose workgroups take the items (list entry,
// block of 32 nodes of that instance, step size; the step size running fastest) with a grid stride.  A workgroup LOOKS AT 64 of its items
// at once, one per lane — whether the instance is still searching, the block has nodes, the step size is one the sequential search
// reaches — and then evaluates the live ones one after the other, all lanes on one item.  A list full of instances that stop on deltaTol
// at once (a converging batch: thousands of entries, nothing to evaluate) costs a workgroup a round or two of loads instead of one
// chain of dependent loads per item; with an empty list — every instance accepted the full step: the steady state — a workgroup
// returns after one load.
__global__ __launch_bounds__(64, 2) void k_ls_tail_eval(Batch b, LsList ls, const DevModel* __restrict__ M, const DevConfig* __restrict__ C,
                                                        double alpha0, double decay, double alpha_min, int n_alpha) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int n_list = *ls.count;
  const int nblk = (b.Nmax + 31) / 32;
  const long items = long(n_list) * nblk * n_alpha, G = gridDim.x;
  const double delta_tol = C->delta_tol;
  __shared__ double lds[LS_PAIR_LDS];
  for (long base = blockIdx.x; base < items; base += 64 * G) {
    bool live = false;
    {
      const long item = base + threadIdx.x * G;
      if (item < items) {
        const int ai = int(item % n_alpha), blk = int((item / n_alpha) % nblk), inst = ls.inst[item / n_alpha / nblk];
        const int n = b.n_nodes[inst], acc = b.accepted[inst];   // (accepted: in an earlier window)
        const double dx_norm = b.ls_norm[inst * 2], du_norm = b.ls_norm[inst * 2 + 1];
        double alpha = alpha0;
        for (int j = 0; j < ai; ++j) alpha *= decay;   // (the sequential search multiplies step by step: the same rounding)
        // step sizes the sequential search never reaches are not evaluated: it stops (no step) at the first alpha with alpha |dx| and
        // alpha |du| below deltaTol, and the condition is monotone in alpha — a converged instance evaluates nothing
        live = !acc && blk * 32 < n && alpha >= alpha_min && !(alpha * du_norm < delta_tol && alpha * dx_norm < delta_tol);
      }
    }
    for (unsigned long long todo = __ballot(live); todo; todo &= todo - 1) {
      const long item = base + __builtin_ctzll(todo) * G;
      const int ai = int(item % n_alpha), blk = int((item / n_alpha) % nblk), inst = __builtin_amdgcn_readfirstlane(ls.inst[item / n_alpha / nblk]);
      double alpha = alpha0;
      for (int j = 0; j < ai; ++j) alpha *= decay;
      const int k = blk * 32 + (threadIdx.x >> 1);
      if (k < b.n_nodes[inst]) ls_pair_node(b, *M, *C, lds, inst, k, alpha, b.ls_tail + ((size_t(inst) * LS_TAIL_MAX + ai) * b.Nmax + k) * 3);
    }
  }
#endif
}
// one thread per node, one workgroup row per step size
__global__ __launch_bounds__(64) void k_ls_tail_eval_node(Batch b, const DevModel* __restrict__ M, const DevConfig* __restrict__ C, double alpha0,
                                                          double decay, double alpha_min) {
  // (k_ls_eval_node with the step size of blockIdx.y; one node per thread and no loop around the node evaluation: no scratch)
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

// ---- plant: one wave per instance --------------------------------------------------------------------------------------
// What a plant kernel's lane 0 does after its step: the new state repacked as rbd, and with res_rbd the resident rbd state, the
// resident MPC observation and the resident time advanced by dt.
__device__ __forceinline__ void plant_publish(const PlantBatch& p, const DevModel* __restrict__ M, int i, double dt, double* res_rbd,
                                              double* res_x0, double* res_t) {
  const double* q = p.q + 16 * i;
  const double* v = p.v + 16 * i;
  double* rbd = p.rbd + HB_NRBD * i;
  plant_rbd_from_state(q, v, rbd);
  if (res_rbd) {
    for (int c = 0; c < HB_NRBD; ++c) res_rbd[HB_NRBD * i + c] = rbd[c];
    centroidal_state_from_rbd(*M, rbd, res_x0 + HB_NX * i);
    res_t[i] += dt;
  }
}
// the pinned stub
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
  if (cx.lane == 0) plant_publish(p, M, i, dt, res_rbd, res_x0, res_t);
}
// ---- the hybrid actuator (hb_plant_step_hybrid / hb_plant_step_lcm): the command's law per substep ----------------------------------------
// c: the five command arrays pos_des vel_des kp kd ff, [B][10] each; a: the record of the step.  tau_last takes the last substep's torque.
struct ActuatorCmd {
  const double* a[5];
};
__device__ __forceinline__ HybridActuator actuator_of(const ActuatorCmd& c, const ActuatorBatch& a, int i, double* lds_act) {
  return HybridActuator{c.a[0] + 10 * i, c.a[1] + 10 * i, c.a[2] + 10 * i, c.a[3] + 10 * i, c.a[4] + 10 * i, a.tau_first + 10 * i, a.tau_mean + 10 * i,
                        lds_act, lds_act + HB_NJ};
}
// The lane contexts of the plant kernels: DeviceCtx under a name of its own per family, held and hybrid, so that each pair of kernels
// instantiates plant_substep / contact_substep / joints_substep for itself.  A second caller of the instantiations another kernel uses
// changes the code generated for THAT kernel (the inliner moves the body of a function into its only caller and clones it for several:
// other value order, other register allocation — k_plant came out 800 instructions shorter), and their ISA is to stay what it is.
// The level kernels and k_plant share DeviceCtx (held) and ActuatorCtx (hybrid).
struct ActuatorCtx : DeviceCtx {};
struct TerrainCtx : DeviceCtx {};
struct TerrainActuatorCtx : DeviceCtx {};
struct VariedCtx : DeviceCtx {};
struct VariedActuatorCtx : DeviceCtx {};
struct ProfileCtx : DeviceCtx {};
struct ProfileActuatorCtx : DeviceCtx {};
struct FieldCtx : DeviceCtx {};
struct FieldActuatorCtx : DeviceCtx {};
// ---- contact model 1 (hb_contact.hpp): ONE body for the twenty kernels that follow; hb_forms.hpp plant_form picks among them ----------------
// The commanded flags are recorded for hb_plant_sense and play no part in the dynamics.  A kernel passes {} / nullptr for what its form lacks.
// Five kernels still spell their instantiation out, statement for statement: through the body one lost a load and four measured slower
// than before; they forward like the others once their forms pass.
//   GROUND  0: the level ground of K | 1: an inclined plane per instance, a friction coefficient per point (hb_plant_set_terrain; ter:
//           [B][Terrain::size]) | 2: piecewise-planar ground, a facet per contact point (hb_plant_set_terrain_profile; pb: hb_layout.hpp
//           ProfileBatch).  The instance's record is staged once per step in LDS behind the form's own arrays (and the actuator's); the
//           working part of a profile record (hb_contact.hpp Profile) follows it there | 3: a height field, a facet per contact point
//           (hb_plant_set_terrain_field; fb: hb_layout.hpp FieldBatch): its header is staged where the profile's record is and its
//           working part lies at the profile's offsets; the heights stay in global memory, a point reads the four of its cell per substep.
//   MODEL   the DevModel the step reads.  0: the nominal *M | 1: Mvar[i] (hb_plant_set_model_variation; [B] records, hb_layout.hpp
//           ModelVarBatch — uniform over the workgroup, so its constants stay scalar loads; without a terrain in force the host keeps the
//           level record of the configuration in ter) | 2: Mvar ? Mvar[i] : *M, so the four profile (and field) kernels cover what the terrain and the
//           varied kernels need eight for.  plant_publish keeps the nominal M, the controller's view.
//   JOINTS  the joint model (hb_joints.hpp): joints_step; tau_last takes the saturated torque, the one the step integrates.
//   HYBRID  the actuator's law per substep (c, a) in place of the held torque tau.
template <int GROUND, int MODEL, bool JOINTS, bool HYBRID, class Ctx>
__device__ __forceinline__ void plant_ground_step(const PlantBatch& p, const ContactBatch& cb, const JointBatch& jb, const double* ter,
                                                  const ProfileBatch& pb, const ActuatorBatch& a, const ActuatorCmd& c, const hb_contact_config& K,
                                                  const hb_joint_model& J, const DevModel* M, const DevModel* Mvar, const double* tau,
                                                  const int* contact, const int* mode, double dt, int substeps, double* res_rbd, double* res_x0,
                                                  double* res_t, const FieldBatch& fb = {}) {
  constexpr int ACT = JOINTS ? JOINT_LDS_TOTAL : CONTACT_LDS_TOTAL;   // LDS: the step's arrays | the actuator's | the ground record
  constexpr int GND = ACT + (HYBRID ? ACT_LDS : 0);
  const int i = blockIdx.x;
  __shared__ double lds[GND + (GROUND == 1 ? TER_LDS : GROUND >= 2 ? PRO_LDS : 0)];
  __shared__ int all_on[HB_NC];
  const Ctx cx;
  if (cx.lane < HB_NC) {
    int flag;
    if (contact) flag = contact[4 * i + cx.lane];
    else { bool cf[HB_NC]; mode_flags(mode[i], cf); flag = cf[cx.lane] ? 1 : 0; }
    p.contact_last[4 * i + cx.lane] = flag;
    all_on[cx.lane] = 1;
  }
  if constexpr (!HYBRID && !JOINTS)
    if (cx.lane < HB_NJ) p.tau_last[10 * i + cx.lane] = tau[10 * i + cx.lane];
  if constexpr (GROUND == 1)
    if (cx.lane < TER_LDS) lds[GND + cx.lane] = ter[TER_LDS * i + cx.lane];
  if constexpr (GROUND == 2)
    for (int k = cx.lane; k < Profile::stored; k += cx.nlanes) lds[GND + k] = pb.prof[size_t(Profile::stored) * i + k];
  if constexpr (GROUND == 3)
    if (cx.lane < Field::stored) lds[GND + cx.lane] = fb.hdr[Field::stored * i + cx.lane];
  __syncthreads();
  const ContactOut out{cb.gap + 4 * i, cb.pvel + 12 * i, cb.res + i, cb.touching + 4 * i, cb.status + i};
  const ProfileIo pio = GROUND == 3 ? ProfileIo{lds + GND, fb.sel + 5 * i, fb.base + Terrain::size * i}
                                    : ProfileIo{lds + GND, pb.seg + 5 * i, pb.base + Terrain::size * i};
  const double* __restrict__ hts = GROUND == 3 ? fb.z + size_t(Field::nz) * i : nullptr;
  const DevModel& Ms = MODEL == 1 || (MODEL == 2 && Mvar) ? Mvar[i] : *M;
  const JointOut jout{jb.tau_applied + 10 * i, jb.friction_torque + 10 * i, jb.limit_torque + 10 * i, jb.res + i, jb.status + i};
  const HybridActuator act = actuator_of(c, a, i, lds + ACT);
  if constexpr (JOINTS)
    joints_step<HYBRID, GROUND>(cx, Ms, p.q + 16 * i, p.v + 16 * i, cb.imp + 12 * i, jb.imp + 20 * i, HYBRID ? nullptr : tau + 10 * i,
                                cb.use_wrench ? cb.wrench + 6 * i : nullptr, all_on, K, J, p.eps, dt, substeps, lds, p.lambda + 12 * i, p.vdot + 16 * i,
                                p.tau_last + 10 * i, out, jout, HYBRID ? &act : nullptr, GROUND ? lds + GND : nullptr, GROUND >= 2 ? &pio : nullptr, hts);
  else
    contact_step<HYBRID, GROUND>(cx, Ms, p.q + 16 * i, p.v + 16 * i, cb.imp + 12 * i, HYBRID ? nullptr : tau + 10 * i,
                                 cb.use_wrench ? cb.wrench + 6 * i : nullptr, all_on, K, p.eps, dt, substeps, lds, p.lambda + 12 * i, p.vdot + 16 * i, out,
                                 HYBRID ? &act : nullptr, GROUND ? lds + GND : nullptr, GROUND >= 2 ? &pio : nullptr, hts);
  if constexpr (HYBRID && !JOINTS)
    if (cx.lane < HB_NJ) p.tau_last[10 * i + cx.lane] = act.tau[cx.lane];   // (the lane's own entry)
  if (cx.lane == 0) plant_publish(p, M, i, dt, res_rbd, res_x0, res_t);
}
__global__ __launch_bounds__(64) void k_plant_contact(PlantBatch p, ContactBatch cb, hb_contact_config K, const DevModel* __restrict__ M,
                                                      const double* tau, const int* contact, const int* mode, double dt, int substeps,
                                                      double* res_rbd, double* res_x0, double* res_t) {
  plant_ground_step<0, 0, false, false, DeviceCtx>(p, cb, {}, nullptr, {}, {}, {}, K, {}, M, nullptr, tau, contact, mode, dt, substeps, res_rbd, res_x0, res_t);
}
__global__ __launch_bounds__(64) void k_plant_joints(PlantBatch p, ContactBatch cb, JointBatch jb, hb_contact_config K, hb_joint_model J,
                                                     const DevModel* __restrict__ M, const double* tau, const int* contact, const int* mode,
                                                     double dt, int substeps, double* res_rbd, double* res_x0, double* res_t) {
  // plant_ground_step<0, 0, true, false, DeviceCtx> written out: through the shared body this one kernel came out with one global load
  // fewer in plant_publish, and a changed count of memory instructions is where the kernels stay as they were.
  const int i = blockIdx.x;
  __shared__ double lds[JOINT_LDS_TOTAL];
  __shared__ int all_on[HB_NC];
  const DeviceCtx cx;
  if (cx.lane < HB_NC) {
    int flag;
    if (contact) flag = contact[4 * i + cx.lane];
    else { bool cf[HB_NC]; mode_flags(mode[i], cf); flag = cf[cx.lane] ? 1 : 0; }
    p.contact_last[4 * i + cx.lane] = flag;
    all_on[cx.lane] = 1;
  }
  __syncthreads();
  const ContactOut out{cb.gap + 4 * i, cb.pvel + 12 * i, cb.res + i, cb.touching + 4 * i, cb.status + i};
  const JointOut jout{jb.tau_applied + 10 * i, jb.friction_torque + 10 * i, jb.limit_torque + 10 * i, jb.res + i, jb.status + i};
  joints_step(cx, *M, p.q + 16 * i, p.v + 16 * i, cb.imp + 12 * i, jb.imp + 20 * i, tau + 10 * i, cb.use_wrench ? cb.wrench + 6 * i : nullptr,
              all_on, K, J, p.eps, dt, substeps, lds, p.lambda + 12 * i, p.vdot + 16 * i, p.tau_last + 10 * i, out, jout);
  if (cx.lane == 0) plant_publish(p, M, i, dt, res_rbd, res_x0, res_t);
}
// the pinned stub under the hybrid actuator
__global__ __launch_bounds__(64) void k_plant_hybrid(PlantBatch p, ActuatorBatch a, ActuatorCmd c, const DevModel* __restrict__ M, const int* contact,
                                                      const int* mode, double dt, int substeps, double* res_rbd, double* res_x0, double* res_t) {
  const int i = blockIdx.x;
  __shared__ double lds[PLANT_LDS_TOTAL + ACT_LDS];
  __shared__ int cflag[HB_NC];
  const ActuatorCtx cx;
  if (cx.lane < HB_NC) {
    if (contact) cflag[cx.lane] = contact[4 * i + cx.lane];
    else { bool cf[HB_NC]; mode_flags(mode[i], cf); cflag[cx.lane] = cf[cx.lane] ? 1 : 0; }
  }
  __syncthreads();
  if (cx.lane < HB_NC) p.contact_last[4 * i + cx.lane] = cflag[cx.lane];
  const HybridActuator act = actuator_of(c, a, i, lds + PLANT_LDS_TOTAL);
  plant_step<true>(cx, *M, p.q + 16 * i, p.v + 16 * i, p.anchor + 12 * i, p.pinned + 4 * i, nullptr, cflag, p.baum, p.eps, dt, substeps, lds,
                   p.lambda + 12 * i, p.vdot + 16 * i, &act);
  if (cx.lane < HB_NJ) p.tau_last[10 * i + cx.lane] = act.tau[cx.lane];   // (the lane's own entry)
  if (cx.lane == 0) plant_publish(p, M, i, dt, res_rbd, res_x0, res_t);
}
__global__ __launch_bounds__(64) void k_plant_contact_hybrid(PlantBatch p, ContactBatch cb, ActuatorBatch a, ActuatorCmd c, hb_contact_config K,
                                                              const DevModel* __restrict__ M, const int* contact, const int* mode, double dt,
                                                              int substeps, double* res_rbd, double* res_x0, double* res_t) {
  // plant_ground_step<0, 0, false, true, ActuatorCtx> written out (timing)
  const int i = blockIdx.x;
  __shared__ double lds[CONTACT_LDS_TOTAL + ACT_LDS];
  __shared__ int all_on[HB_NC];
  const ActuatorCtx cx;
  if (cx.lane < HB_NC) {
    int flag;
    if (contact) flag = contact[4 * i + cx.lane];
    else { bool cf[HB_NC]; mode_flags(mode[i], cf); flag = cf[cx.lane] ? 1 : 0; }
    p.contact_last[4 * i + cx.lane] = flag;
    all_on[cx.lane] = 1;
  }
  __syncthreads();
  const ContactOut out{cb.gap + 4 * i, cb.pvel + 12 * i, cb.res + i, cb.touching + 4 * i, cb.status + i};
  const HybridActuator act = actuator_of(c, a, i, lds + CONTACT_LDS_TOTAL);
  contact_step<true>(cx, *M, p.q + 16 * i, p.v + 16 * i, cb.imp + 12 * i, nullptr, cb.use_wrench ? cb.wrench + 6 * i : nullptr, all_on, K, p.eps, dt,
                     substeps, lds, p.lambda + 12 * i, p.vdot + 16 * i, out, &act);
  if (cx.lane < HB_NJ) p.tau_last[10 * i + cx.lane] = act.tau[cx.lane];   // (the lane's own entry)
  if (cx.lane == 0) plant_publish(p, M, i, dt, res_rbd, res_x0, res_t);
}
__global__ __launch_bounds__(64) void k_plant_joints_hybrid(PlantBatch p, ContactBatch cb, JointBatch jb, ActuatorBatch a, ActuatorCmd c,
                                                             hb_contact_config K, hb_joint_model J, const DevModel* __restrict__ M, const int* contact,
                                                             const int* mode, double dt, int substeps, double* res_rbd, double* res_x0,
                                                             double* res_t) {
  plant_ground_step<0, 0, true, true, ActuatorCtx>(p, cb, jb, nullptr, {}, a, c, K, J, M, nullptr, nullptr, contact, mode, dt, substeps, res_rbd, res_x0, res_t);
}
__global__ __launch_bounds__(64) void k_plant_terrain(PlantBatch p, ContactBatch cb, const double* __restrict__ ter, hb_contact_config K,
                                                      const DevModel* __restrict__ M, const double* tau, const int* contact, const int* mode, double dt,
                                                      int substeps, double* res_rbd, double* res_x0, double* res_t) {
  // plant_ground_step<1, 0, false, false, TerrainCtx> written out (timing)
  const int i = blockIdx.x;
  __shared__ double lds[CONTACT_LDS_TOTAL + TER_LDS];
  __shared__ int all_on[HB_NC];
  const TerrainCtx cx;
  if (cx.lane < HB_NC) {
    int flag;
    if (contact) flag = contact[4 * i + cx.lane];
    else { bool cf[HB_NC]; mode_flags(mode[i], cf); flag = cf[cx.lane] ? 1 : 0; }
    p.contact_last[4 * i + cx.lane] = flag;
    all_on[cx.lane] = 1;
  }
  if (cx.lane < HB_NJ) p.tau_last[10 * i + cx.lane] = tau[10 * i + cx.lane];
  if (cx.lane < TER_LDS) lds[CONTACT_LDS_TOTAL + cx.lane] = ter[TER_LDS * i + cx.lane];
  __syncthreads();
  const ContactOut out{cb.gap + 4 * i, cb.pvel + 12 * i, cb.res + i, cb.touching + 4 * i, cb.status + i};
  contact_step<false, true>(cx, *M, p.q + 16 * i, p.v + 16 * i, cb.imp + 12 * i, tau + 10 * i, cb.use_wrench ? cb.wrench + 6 * i : nullptr, all_on, K,
                            p.eps, dt, substeps, lds, p.lambda + 12 * i, p.vdot + 16 * i, out, nullptr, lds + CONTACT_LDS_TOTAL);
  if (cx.lane == 0) plant_publish(p, M, i, dt, res_rbd, res_x0, res_t);
}
__global__ __launch_bounds__(64) void k_plant_terrain_joints(PlantBatch p, ContactBatch cb, JointBatch jb, const double* __restrict__ ter,
                                                             hb_contact_config K, hb_joint_model J, const DevModel* __restrict__ M, const double* tau,
                                                             const int* contact, const int* mode, double dt, int substeps, double* res_rbd,
                                                             double* res_x0, double* res_t) {
  plant_ground_step<1, 0, true, false, TerrainCtx>(p, cb, jb, ter, {}, {}, {}, K, J, M, nullptr, tau, contact, mode, dt, substeps, res_rbd, res_x0, res_t);
}
__global__ __launch_bounds__(64) void k_plant_terrain_hybrid(PlantBatch p, ContactBatch cb, const double* __restrict__ ter, ActuatorBatch a,
                                                             ActuatorCmd c, hb_contact_config K, const DevModel* __restrict__ M, const int* contact,
                                                             const int* mode, double dt, int substeps, double* res_rbd, double* res_x0,
                                                             double* res_t) {
  // plant_ground_step<1, 0, false, true, TerrainActuatorCtx> written out (timing)
  const int i = blockIdx.x;
  __shared__ double lds[CONTACT_LDS_TOTAL + ACT_LDS + TER_LDS];
  __shared__ int all_on[HB_NC];
  const TerrainActuatorCtx cx;
  if (cx.lane < HB_NC) {
    int flag;
    if (contact) flag = contact[4 * i + cx.lane];
    else { bool cf[HB_NC]; mode_flags(mode[i], cf); flag = cf[cx.lane] ? 1 : 0; }
    p.contact_last[4 * i + cx.lane] = flag;
    all_on[cx.lane] = 1;
  }
  if (cx.lane < TER_LDS) lds[CONTACT_LDS_TOTAL + ACT_LDS + cx.lane] = ter[TER_LDS * i + cx.lane];
  __syncthreads();
  const ContactOut out{cb.gap + 4 * i, cb.pvel + 12 * i, cb.res + i, cb.touching + 4 * i, cb.status + i};
  const HybridActuator act = actuator_of(c, a, i, lds + CONTACT_LDS_TOTAL);
  contact_step<true, true>(cx, *M, p.q + 16 * i, p.v + 16 * i, cb.imp + 12 * i, nullptr, cb.use_wrench ? cb.wrench + 6 * i : nullptr, all_on, K, p.eps,
                           dt, substeps, lds, p.lambda + 12 * i, p.vdot + 16 * i, out, &act, lds + CONTACT_LDS_TOTAL + ACT_LDS);
  if (cx.lane < HB_NJ) p.tau_last[10 * i + cx.lane] = act.tau[cx.lane];   // (the lane's own entry)
  if (cx.lane == 0) plant_publish(p, M, i, dt, res_rbd, res_x0, res_t);
}
__global__ __launch_bounds__(64) void k_plant_terrain_joints_hybrid(PlantBatch p, ContactBatch cb, JointBatch jb, const double* __restrict__ ter,
                                                                    ActuatorBatch a, ActuatorCmd c, hb_contact_config K, hb_joint_model J,
                                                                    const DevModel* __restrict__ M, const int* contact, const int* mode, double dt,
                                                                    int substeps, double* res_rbd, double* res_x0, double* res_t) {
  plant_ground_step<1, 0, true, true, TerrainActuatorCtx>(p, cb, jb, ter, {}, a, c, K, J, M, nullptr, nullptr, contact, mode, dt, substeps, res_rbd, res_x0, res_t);
}
__global__ __launch_bounds__(64) void k_plant_varied(PlantBatch p, ContactBatch cb, const double* __restrict__ ter, hb_contact_config K,
                                                     const DevModel* __restrict__ M, const DevModel* __restrict__ Mvar, const double* tau, const int* contact,
                                                     const int* mode, double dt, int substeps, double* res_rbd, double* res_x0, double* res_t) {
  plant_ground_step<1, 1, false, false, VariedCtx>(p, cb, {}, ter, {}, {}, {}, K, {}, M, Mvar, tau, contact, mode, dt, substeps, res_rbd, res_x0, res_t);
}
__global__ __launch_bounds__(64) void k_plant_varied_joints(PlantBatch p, ContactBatch cb, JointBatch jb, const double* __restrict__ ter, hb_contact_config K,
                                                            hb_joint_model J, const DevModel* __restrict__ M, const DevModel* __restrict__ Mvar,
                                                            const double* tau, const int* contact, const int* mode, double dt, int substeps, double* res_rbd,
                                                            double* res_x0, double* res_t) {
  plant_ground_step<1, 1, true, false, VariedCtx>(p, cb, jb, ter, {}, {}, {}, K, J, M, Mvar, tau, contact, mode, dt, substeps, res_rbd, res_x0, res_t);
}
__global__ __launch_bounds__(64) void k_plant_varied_hybrid(PlantBatch p, ContactBatch cb, const double* __restrict__ ter, ActuatorBatch a, ActuatorCmd c,
                                                            hb_contact_config K, const DevModel* __restrict__ M, const DevModel* __restrict__ Mvar,
                                                            const int* contact, const int* mode, double dt, int substeps, double* res_rbd, double* res_x0,
                                                            double* res_t) {
  plant_ground_step<1, 1, false, true, VariedActuatorCtx>(p, cb, {}, ter, {}, a, c, K, {}, M, Mvar, nullptr, contact, mode, dt, substeps, res_rbd, res_x0, res_t);
}
__global__ __launch_bounds__(64) void k_plant_varied_joints_hybrid(PlantBatch p, ContactBatch cb, JointBatch jb, const double* __restrict__ ter,
                                                                   ActuatorBatch a, ActuatorCmd c, hb_contact_config K, hb_joint_model J,
                                                                   const DevModel* __restrict__ M, const DevModel* __restrict__ Mvar, const int* contact,
                                                                   const int* mode, double dt, int substeps, double* res_rbd, double* res_x0, double* res_t) {
  plant_ground_step<1, 1, true, true, VariedActuatorCtx>(p, cb, jb, ter, {}, a, c, K, J, M, Mvar, nullptr, contact, mode, dt, substeps, res_rbd, res_x0, res_t);
}
__global__ __launch_bounds__(64) void k_plant_profile(PlantBatch p, ContactBatch cb, ProfileBatch pb, hb_contact_config K, const DevModel* __restrict__ M,
                                                      const DevModel* __restrict__ Mvar, const double* tau, const int* contact, const int* mode, double dt,
                                                      int substeps, double* res_rbd, double* res_x0, double* res_t) {
  plant_ground_step<2, 2, false, false, ProfileCtx>(p, cb, {}, nullptr, pb, {}, {}, K, {}, M, Mvar, tau, contact, mode, dt, substeps, res_rbd, res_x0, res_t);
}
__global__ __launch_bounds__(64) void k_plant_profile_joints(PlantBatch p, ContactBatch cb, JointBatch jb, ProfileBatch pb, hb_contact_config K,
                                                             hb_joint_model J, const DevModel* __restrict__ M, const DevModel* __restrict__ Mvar,
                                                             const double* tau, const int* contact, const int* mode, double dt, int substeps,
                                                             double* res_rbd, double* res_x0, double* res_t) {
  plant_ground_step<2, 2, true, false, ProfileCtx>(p, cb, jb, nullptr, pb, {}, {}, K, J, M, Mvar, tau, contact, mode, dt, substeps, res_rbd, res_x0, res_t);
}
__global__ __launch_bounds__(64) void k_plant_profile_hybrid(PlantBatch p, ContactBatch cb, ProfileBatch pb, ActuatorBatch a, ActuatorCmd c,
                                                             hb_contact_config K, const DevModel* __restrict__ M, const DevModel* __restrict__ Mvar,
                                                             const int* contact, const int* mode, double dt, int substeps, double* res_rbd,
                                                             double* res_x0, double* res_t) {
  plant_ground_step<2, 2, false, true, ProfileActuatorCtx>(p, cb, {}, nullptr, pb, a, c, K, {}, M, Mvar, nullptr, contact, mode, dt, substeps, res_rbd, res_x0, res_t);
}
__global__ __launch_bounds__(64) void k_plant_profile_joints_hybrid(PlantBatch p, ContactBatch cb, JointBatch jb, ProfileBatch pb, ActuatorBatch a,
                                                                    ActuatorCmd c, hb_contact_config K, hb_joint_model J,
                                                                    const DevModel* __restrict__ M, const DevModel* __restrict__ Mvar,
                                                                    const int* contact, const int* mode, double dt, int substeps, double* res_rbd,
                                                                    double* res_x0, double* res_t) {
  // plant_ground_step<2, 2, true, true, ProfileActuatorCtx> written out (timing)
  const int i = blockIdx.x;
  __shared__ double lds[JOINT_LDS_TOTAL + ACT_LDS + PRO_LDS];
  __shared__ int all_on[HB_NC];
  const ProfileActuatorCtx cx;
  if (cx.lane < HB_NC) {
    int flag;
    if (contact) flag = contact[4 * i + cx.lane];
    else { bool cf[HB_NC]; mode_flags(mode[i], cf); flag = cf[cx.lane] ? 1 : 0; }
    p.contact_last[4 * i + cx.lane] = flag;
    all_on[cx.lane] = 1;
  }
  for (int k = cx.lane; k < Profile::stored; k += cx.nlanes) lds[JOINT_LDS_TOTAL + ACT_LDS + k] = pb.prof[size_t(Profile::stored) * i + k];
  __syncthreads();
  const ContactOut out{cb.gap + 4 * i, cb.pvel + 12 * i, cb.res + i, cb.touching + 4 * i, cb.status + i};
  const ProfileIo pio{lds + JOINT_LDS_TOTAL + ACT_LDS, pb.seg + 5 * i, pb.base + Terrain::size * i};
  const DevModel& Ms = Mvar ? Mvar[i] : *M;
  const JointOut jout{jb.tau_applied + 10 * i, jb.friction_torque + 10 * i, jb.limit_torque + 10 * i, jb.res + i, jb.status + i};
  const HybridActuator act = actuator_of(c, a, i, lds + JOINT_LDS_TOTAL);
  joints_step<true, 2>(cx, Ms, p.q + 16 * i, p.v + 16 * i, cb.imp + 12 * i, jb.imp + 20 * i, nullptr, cb.use_wrench ? cb.wrench + 6 * i : nullptr, all_on, K,
                       J, p.eps, dt, substeps, lds, p.lambda + 12 * i, p.vdot + 16 * i, p.tau_last + 10 * i, out, jout, &act, pio.pro, &pio);
  if (cx.lane == 0) plant_publish(p, M, i, dt, res_rbd, res_x0, res_t);
}
// the four forms on a height field (hb_plant_set_terrain_field): GROUND 3 of the shared body
__global__ __launch_bounds__(64) void k_plant_field(PlantBatch p, ContactBatch cb, FieldBatch fb, hb_contact_config K, const DevModel* __restrict__ M,
                                                    const DevModel* __restrict__ Mvar, const double* tau, const int* contact, const int* mode, double dt,
                                                    int substeps, double* res_rbd, double* res_x0, double* res_t) {
  plant_ground_step<3, 2, false, false, FieldCtx>(p, cb, {}, nullptr, {}, {}, {}, K, {}, M, Mvar, tau, contact, mode, dt, substeps, res_rbd, res_x0, res_t, fb);
}
__global__ __launch_bounds__(64) void k_plant_field_joints(PlantBatch p, ContactBatch cb, JointBatch jb, FieldBatch fb, hb_contact_config K,
                                                           hb_joint_model J, const DevModel* __restrict__ M, const DevModel* __restrict__ Mvar,
                                                           const double* tau, const int* contact, const int* mode, double dt, int substeps,
                                                           double* res_rbd, double* res_x0, double* res_t) {
  plant_ground_step<3, 2, true, false, FieldCtx>(p, cb, jb, nullptr, {}, {}, {}, K, J, M, Mvar, tau, contact, mode, dt, substeps, res_rbd, res_x0, res_t, fb);
}
__global__ __launch_bounds__(64) void k_plant_field_hybrid(PlantBatch p, ContactBatch cb, FieldBatch fb, ActuatorBatch a, ActuatorCmd c,
                                                           hb_contact_config K, const DevModel* __restrict__ M, const DevModel* __restrict__ Mvar,
                                                           const int* contact, const int* mode, double dt, int substeps, double* res_rbd,
                                                           double* res_x0, double* res_t) {
  plant_ground_step<3, 2, false, true, FieldActuatorCtx>(p, cb, {}, nullptr, {}, a, c, K, {}, M, Mvar, nullptr, contact, mode, dt, substeps, res_rbd, res_x0, res_t, fb);
}
__global__ __launch_bounds__(64) void k_plant_field_joints_hybrid(PlantBatch p, ContactBatch cb, JointBatch jb, FieldBatch fb, ActuatorBatch a,
                                                                  ActuatorCmd c, hb_contact_config K, hb_joint_model J,
                                                                  const DevModel* __restrict__ M, const DevModel* __restrict__ Mvar,
                                                                  const int* contact, const int* mode, double dt, int substeps, double* res_rbd,
                                                                  double* res_x0, double* res_t) {
  plant_ground_step<3, 2, true, true, FieldActuatorCtx>(p, cb, jb, nullptr, {}, a, c, K, J, M, Mvar, nullptr, contact, mode, dt, substeps, res_rbd, res_x0, res_t, fb);
}
// hb_plant_field_eval: the facet under n world points per instance of the field in force, one thread per point
__global__ __launch_bounds__(64) void k_field_eval(FieldBatch fb, int n, const double* __restrict__ xyz, int* __restrict__ facet,
                                                   double* __restrict__ records, double* __restrict__ height) {
  const long e = long(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= long(fb.B) * n) return;
  const long i = e / n;
  double rec[Terrain::size];
  facet[e] = field_facet(fb.hdr + Field::stored * i, fb.z + size_t(Field::nz) * i, xyz + 3 * e, rec);
  for (int k = 0; k < Profile::rec; ++k) records[Profile::rec * e + k] = rec[k];
  height[e] = terrain_height(rec, xyz + 3 * e);
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

// ---- episode record (hb_plant_set_episode, hb_episode.hpp): one thread per instance, behind every plant step --------------------------
// What the plant form in force left for instance i.  ter: the terrain records or null (then the plane is e_z . x = d0); cb / jb are read
// only with `ground` / `joints`; wbc_status is null before the first WBC call.
__device__ __forceinline__ EpisodeIn episode_in(const PlantBatch& p, const ContactBatch& cb, const JointBatch& jb, const double* ter, double d0,
                                                int ground, int joints, const int* wbc_status, int i) {
  EpisodeIn in{};
  in.q = p.q + 16 * i;
  in.v = p.v + 16 * i;
  in.tau_last = p.tau_last + 10 * i;
  in.n[0] = 0.0; in.n[1] = 0.0; in.n[2] = 1.0;
  in.d = d0;
  if (ter) {
    const double* r = ter + size_t(Terrain::size) * i;
    for (int a = 0; a < 3; ++a) in.n[a] = r[Terrain::T + 3 * a + 2];
    in.d = r[Terrain::d];
  }
  if (wbc_status) in.wbc_status = wbc_status + i;
  if (ground) {
    in.gap = cb.gap + 4 * i; in.lambda = p.lambda + 12 * i; in.pvel = cb.pvel + 12 * i; in.res = cb.res + i;
    in.touching = cb.touching + 4 * i; in.cstatus = cb.status + i;
  }
  if (joints) { in.jres = jb.res + i; in.jstatus = jb.status + i; }
  return in;
}
__global__ __launch_bounds__(64) void k_plant_episode_init(EpisodeBatch e, PlantBatch p, const double* __restrict__ ter, double d0) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= e.B) return;
  const EpisodeIn in = episode_in(p, ContactBatch{}, JointBatch{}, ter, d0, 0, 0, nullptr, i);
  episode_init(in, e.irec + HB_EP_NI * i, e.drec + HB_EP_ND * i);
}
__global__ __launch_bounds__(64) void k_plant_episode(EpisodeBatch e, hb_episode_config K, PlantBatch p, ContactBatch cb, JointBatch jb,
                                                      const double* __restrict__ ter, double d0, int ground, int joints, const int* wbc_status,
                                                      int* estop, double dt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= e.B) return;
  const EpisodeIn in = episode_in(p, cb, jb, ter, d0, ground, joints, wbc_status, i);
  episode_update(K, in, dt, e.irec + HB_EP_NI * i, e.drec + HB_EP_ND * i, e.trace + size_t(i) * e.trace_cap * HB_EP_TRACE_W, estop ? estop + i : nullptr);
}

// ---- respawn of ended instances (hb_plant_respawn, hb_respawn.hpp): one wavefront per instance -----------------------------------------
// Every lane reads the decision from the instance's record (the same words: wave-uniform), and a wavefront whose instance stays leaves
// after those loads.  A respawning wavefront draws its Philox blocks one per lane into LDS, lane 0 folds the record, composes and places
// the spawn state (the one sequential piece: the leg kinematics, as in k_plant_reset) and resets the gait object; then all lanes write the
// rows, consecutive lanes on consecutive words.  cb / jb / ab / est / estop / e.trace: null arrays where the subsystem has none.
// pb: the terrain profile in force (null prof: none, and nothing below differs from the placement on the plane; with one, ter is null: the
// host's plane pointer would be pb.base, which this kernel writes): lane 0 places the state
// vertically on the facets under its contact points and locates it (hb_profiledraw.hpp), the record starts over the facet under the base
// origin, and seg[5] / base[14] of the instance are written with the rows.
// FIELD (k_plant_respawn_field): fb is the height field in force (ter null, pb without a profile): lane 0 places the state vertically on the
// facets under its contact points and locates it (hb_fielddraw.hpp), the record starts over the facet under the base origin, and sel[5] /
// base[14] of the instance are written with the rows.  The form without a field compiles nothing of it and stores what it always stored.
template <bool FIELD>
__device__ __forceinline__ void plant_respawn(const RespawnBatch& rs, const hb_respawn_config& K, const EpisodeBatch& e, const PlantBatch& p,
                                              const ContactBatch& cb, const JointBatch& jb, const ActuatorBatch& ab, const EstBatch& est,
                                              const GaitBatch& g, const hb_gait_config& GK, int gait_on, const double* __restrict__ ter, double d0,
                                              const DevModel* __restrict__ M, int* estop, double* res_rbd, double* res_x0, const ProfileBatch& pb,
                                              const FieldBatch& fb) {
  const int i = blockIdx.x;
  const DeviceCtx cx;
  int* irec = e.irec + HB_EP_NI * i;
  const int cause = respawn_decide(K, irec);
  if (cause == 0) return;
  __shared__ double sh[RS_DRAW + 16 + 16 + 12 + HB_NRBD + HB_NX + 4 + Terrain::size];
  __shared__ int seg[HB_NC + 1];
  double* draw = sh;
  double* q = draw + RS_DRAW;
  double* v = q + 16;
  double* feet = v + 16;
  double* rbd = feet + 12;
  double* x0 = rbd + HB_NRBD;
  double* plane = x0 + HB_NX;
  double* base = plane + 4;
  int* itot = rs.itot + HB_RS_NI * i;
  double* drec = e.drec + HB_EP_ND * i;
  if (cx.lane < RS_BLOCKS && respawn_block_needed(K, cx.lane))
    respawn_draw_block(K, K.instance_offset + uint32_t(i), uint32_t(itot[HB_RS_I_EPISODE_INDEX] + 1), cx.lane, draw, nullptr);
  __syncthreads();
  if (cx.lane == 0) {
    respawn_fold(cause, irec, drec, itot, rs.dtot + HB_RS_ND * i);
    itot[HB_RS_I_EPISODE_INDEX] += 1;
    plane[0] = 0.0; plane[1] = 0.0; plane[2] = 1.0; plane[3] = d0;
    if (ter) {
      const double* r = ter + size_t(Terrain::size) * i;
      for (int a = 0; a < 3; ++a) plane[a] = r[Terrain::T + 3 * a + 2];
      plane[3] = r[Terrain::d];
    }
    respawn_perturb(K, rs.q_spawn + 16 * i, rs.v_spawn + 16 * i, draw, q, v);
    plant_feet(*M, q, feet);
    if constexpr (FIELD) {   // on a height field: vertically onto the facets under the points, then the locate of the placed state
      const double* fld = fb.hdr + size_t(Field::stored) * i;
      const double* hts = fb.z + size_t(Field::nz) * i;
      field_place(*M, K, fld, hts, q, feet);
      field_locate_state(fld, hts, q, feet, seg, base);
      for (int a = 0; a < 3; ++a) plane[a] = base[Terrain::T + 3 * a + 2];
      plane[3] = base[Terrain::d];
    } else if (pb.prof) {   // on a profile: vertically onto the facets under the points, then the locate of the placed state
      const double* pro = pb.prof + size_t(Profile::stored) * i;
      profile_place(*M, K, pro, q, feet);
      profile_locate_state(pro, q, feet, seg, base);
      for (int a = 0; a < 3; ++a) plane[a] = base[Terrain::T + 3 * a + 2];
      plane[3] = base[Terrain::d];
    } else {
      respawn_place(*M, K, plane, q, feet);
    }
    plant_rbd_from_state(q, v, rbd);
    centroidal_state_from_rbd(*M, rbd, x0);
    if (gait_on) gait_reset_instance(g, i, GK);
  }
  __syncthreads();
  RespawnRows r{};
  r.q = p.q + 16 * i; r.v = p.v + 16 * i; r.anchor = p.anchor + 12 * i; r.lambda = p.lambda + 12 * i; r.vdot = p.vdot + 16 * i;
  r.tau_last = p.tau_last + 10 * i; r.rbd = p.rbd + HB_NRBD * i; r.pinned = p.pinned + 4 * i; r.contact_last = p.contact_last + 4 * i;
  r.q_last = rs.q_last + 16 * i; r.v_last = rs.v_last + 16 * i;
  if (cb.imp) {
    r.c_imp = cb.imp + 12 * i; r.c_gap = cb.gap + 4 * i; r.c_pvel = cb.pvel + 12 * i; r.c_res = cb.res + i; r.c_touching = cb.touching + 4 * i;
    r.c_status = cb.status + i;
  }
  if (jb.imp) {
    r.j_imp = jb.imp + 20 * i; r.j_tau_applied = jb.tau_applied + 10 * i; r.j_friction = jb.friction_torque + 10 * i;
    r.j_limit = jb.limit_torque + 10 * i; r.j_res = jb.res + i; r.j_status = jb.status + i;
  }
  if (ab.tau_first) {
    r.a_tau_first = ab.tau_first + 10 * i; r.a_tau_mean = ab.tau_mean + 10 * i; r.a_last_ts = ab.last_ts + i;
    for (int k = 0; k < 5; ++k) r.a_rcmd[k] = ab.rcmd[k] + 10 * i;
  }
  r.estop = estop ? estop + i : nullptr;
  r.irec = irec; r.drec = drec;
  r.trace = e.trace ? e.trace + size_t(i) * e.trace_cap * HB_EP_TRACE_W : nullptr;
  r.trace_cap = e.trace_cap;
  if (est.xhat) { r.xhat = est.xhat + 18 * i; r.P = est.P + 324 * size_t(i); r.yaw_last = est.yaw_last + i; r.cf_z = est.cf_z + HB_NV * i; }
  r.res_rbd = res_rbd + HB_NRBD * i; r.res_x0 = res_x0 + HB_NX * i;
  r.rg_pending = rs.rg_pending + i; r.mpc_pending = rs.mpc_pending + i;
  respawn_write(cx, r, q, v, feet, rbd, x0, plane);
  if constexpr (FIELD) {
    for (int c = cx.lane; c < HB_NC + 1; c += cx.nlanes) fb.sel[(HB_NC + 1) * i + c] = seg[c];
    for (int k = cx.lane; k < Terrain::size; k += cx.nlanes) fb.base[size_t(Terrain::size) * i + k] = base[k];
  } else if (pb.prof) {
    for (int c = cx.lane; c < HB_NC + 1; c += cx.nlanes) pb.seg[(HB_NC + 1) * i + c] = seg[c];
    for (int k = cx.lane; k < Terrain::size; k += cx.nlanes) pb.base[size_t(Terrain::size) * i + k] = base[k];
  }
}
__global__ __launch_bounds__(64) void k_plant_respawn(RespawnBatch rs, hb_respawn_config K, EpisodeBatch e, PlantBatch p, ContactBatch cb, JointBatch jb,
                                                      ActuatorBatch ab, EstBatch est, GaitBatch g, hb_gait_config GK, int gait_on,
                                                      const double* __restrict__ ter, double d0, const DevModel* __restrict__ M, int* estop,
                                                      double* res_rbd, double* res_x0, ProfileBatch pb) {
  plant_respawn<false>(rs, K, e, p, cb, jb, ab, est, g, GK, gait_on, ter, d0, M, estop, res_rbd, res_x0, pb, FieldBatch{});
}
__global__ __launch_bounds__(64) void k_plant_respawn_field(RespawnBatch rs, hb_respawn_config K, EpisodeBatch e, PlantBatch p, ContactBatch cb,
                                                            JointBatch jb, ActuatorBatch ab, EstBatch est, GaitBatch g, hb_gait_config GK, int gait_on,
                                                            double d0, const DevModel* __restrict__ M, int* estop, double* res_rbd, double* res_x0,
                                                            FieldBatch fb) {
  plant_respawn<true>(rs, K, e, p, cb, jb, ab, est, g, GK, gait_on, nullptr, d0, M, estop, res_rbd, res_x0, ProfileBatch{}, fb);
}

// ---- field draw at respawn (hb_plant_set_field_draw, hb_fielddraw.hpp): one wavefront per instance, ahead of k_plant_respawn_field ----------
// Every lane reads k_plant_respawn's decision from the instance's still unchanged record (the same words: wave-uniform), and a wavefront
// whose instance stays leaves after those loads.  A respawning wavefront appends the log row of the finished episode (all lanes, from the
// row still in place), draws its two head blocks one per lane into LDS, lets lane 0 turn them into the row and the node parameters, and
// then generates the 256 node blocks: lane l takes blocks l + 64 m, m = 0 .. 3, four consecutive nodes each, so that a pass of the
// wavefront stores one contiguous 2 KB run of the plant's heights (and, with a map that follows, of the map's), 32 B per lane.  The heights
// never sit in LDS.  Behind a workgroup barrier lane 0 composes the stored header (field_compose: the routine of the host setter; it
// reads the four heights of the cell under the world origin back) and the map's; header, row and map header go out with consecutive
// lanes on consecutive words.  gf: the controller's field map, or without arrays where it does not follow.
__global__ __launch_bounds__(64) void k_plant_field_draw(FieldDrawBatch fd, hb_field_draw_config K, hb_respawn_config RK, RespawnBatch rs,
                                                         EpisodeBatch e, FieldBatch fb, GroundFieldBatch gf, double ground_z) {
  const int i = blockIdx.x;
  const DeviceCtx cx;
  const int* irec = e.irec + HB_EP_NI * i;
  const int cause = respawn_decide(RK, irec);
  if (cause == 0) return;
  __shared__ double sh[FD_HEAD + 2 + HB_FD_N + 3 + Field::stored + GroundField::size];
  double* u = sh;
  double* a = u + FD_HEAD;
  double* row_s = a + 2;
  double* par_s = row_s + HB_FD_N;
  double* hdr_s = par_s + 3;
  double* map_s = hdr_s + Field::stored;
  const int* itot = rs.itot + HB_RS_NI * i;
  double* row = fd.row + HB_FD_N * i;
  double* z = fb.z + size_t(Field::nz) * i;
  double* gz = gf.z ? gf.z + size_t(GroundField::nz) * i : nullptr;
  const uint32_t instance = RK.instance_offset + uint32_t(i), episode = uint32_t(itot[HB_RS_I_EPISODE_INDEX] + 1);
  if (cx.lane < 2) a[cx.lane] = K.dir[cx.lane];
  __syncthreads();
  if (K.log_capacity > 0)
    field_draw_log_append(cx, K.log_capacity, cause, a, irec, e.drec + HB_EP_ND * i, itot, row, fd.count + i,
                          fd.log + size_t(i) * fd.log_cap * HB_FD_LOG_W);
  if (cx.lane < FD_HEAD_BLOCKS) field_draw_block(K, instance, episode, cx.lane, u + 4 * cx.lane, nullptr);
  __syncthreads();
  if (cx.lane == 0) {
    const FieldDrawPar par = field_draw_head(K, u, row_s);
    par_s[0] = par.A; par_s[1] = par.p; par_s[2] = par.r;
  }
  __syncthreads();
  FieldDrawPar par;
  par.A = par_s[0]; par.p = par_s[1]; par.r = par_s[2];
#pragma unroll 1
  for (int m = 0; m < FD_NODE_BLOCKS / 64; ++m) field_draw_nodes(K, par, instance, episode, cx.lane + 64 * m, ground_z, z, gz);
  __syncthreads();   // (a workgroup-scope fence: the heights lane 0 reads back below are the ones just stored)
  if (cx.lane == 0) {
    double org[2];
    field_draw_origin(K, a, rs.q_spawn + 16 * i, org);
    field_compose(K.n_nodes, a, org, K.spacing, z, row_s + HB_FD_MUS, hdr_s);
    ground_field_compose(K.n_nodes, a, org, K.spacing, map_s);
  }
  __syncthreads();
  for (int k = cx.lane; k < Field::stored; k += cx.nlanes) fb.hdr[size_t(Field::stored) * i + k] = hdr_s[k];
  for (int k = cx.lane; k < HB_FD_N; k += cx.nlanes) row[k] = row_s[k];
  if (gz)
    for (int k = cx.lane; k < GroundField::size; k += cx.nlanes) gf.hdr[size_t(GroundField::size) * i + k] = map_s[k];
}

// ---- height scan (hb_plant_scan, hb_scan.hpp): one wavefront per instance ------------------------------------------------------------------
// The pose, the decision to skip and the decision to clear are read by every lane from the same words (wave-uniform).  The instance's 1024
// old heights are staged in LDS (8 KB, consecutive lanes on consecutive words) ahead of a workgroup barrier, so the in-place update reads
// every old height before it writes any and a node without a return finds the old height of its shifted index there.  Lane l then takes
// blocks l + 64 m, m = 0 .. 3, of each channel that is on — 16 nodes, four consecutive ones per block — so a pass of the wavefront stores
// one contiguous 2 KB run of heights, 32 B per lane, and 256 B of flags.  GROUND (hb_scan.hpp SCAN_*) is picked on the host (hb_forms.hpp
// scan_ground): gnd is the plant's ground record with gstride doubles per instance (null / 0 for the level ground), fz the heights of its
// field.  itot: RespawnBatch::itot, or null without a respawn configuration in force.
template <int GROUND>
__global__ __launch_bounds__(64) void k_plant_scan(ScanBatch sb, hb_height_scan_config K, unsigned count, const double* __restrict__ q,
                                                   const double* __restrict__ rbd, const int* __restrict__ itot, const double* __restrict__ gnd,
                                                   int gstride, const double* __restrict__ fz, GroundFieldBatch gf, double ground_z) {
  const int i = blockIdx.x;
  if (i >= sb.B) return;
  const DeviceCtx cx;
  __shared__ double old[GroundField::nz];
  __shared__ int cnt[64];
  ScanIo io;
  io.q = q + 16 * size_t(i);
  io.rbd = rbd + HB_NRBD * size_t(i);
  io.itot = itot ? itot + HB_RS_NI * size_t(i) : nullptr;
  io.gnd = gnd ? gnd + size_t(gstride) * i : nullptr;
  io.fz = fz ? fz + size_t(Field::nz) * i : nullptr;
  io.hdr = gf.hdr + size_t(GroundField::size) * i;
  io.z = gf.z + size_t(GroundField::nz) * i;
  io.k = sb.k + 2 * size_t(i);
  io.episode_seen = sb.episode_seen + i;
  io.n_returns = sb.n_returns + i;
  io.returned = sb.returned + size_t(GroundField::nz) * i;
  scan_instance<GROUND>(cx, K, K.instance_offset + uint32_t(i), count, ground_z, io, old, cnt);
}

// ---- profile draw at respawn (hb_plant_set_profile_draw, hb_profiledraw.hpp): one wavefront per instance, ahead of k_plant_respawn --------
// Every lane reads k_plant_respawn's decision from the instance's still unchanged record (the same words: wave-uniform), and a wavefront
// whose instance stays leaves after those loads.  A respawning wavefront appends the log row of the finished episode (all lanes, from the
// row still in place), draws its Philox blocks one per lane into LDS, lets lane 0 compose the knots and the row (the one sequential
// piece), composes the profile record and, with a map that follows, the map record one segment per lane (profile_compose /
// ground_compose: the routines of the host setters) and writes records, knots and row with all lanes, consecutive lanes on consecutive
// words.  gmap: GroundBatch::map, or null where the controller's map does not follow.
__global__ __launch_bounds__(64) void k_plant_profile_draw(ProfileDrawBatch pd, hb_profile_draw_config K, hb_respawn_config RK, RespawnBatch rs,
                                                           EpisodeBatch e, ProfileBatch pb, double* gmap, double ground_z) {
  const int i = blockIdx.x;
  const DeviceCtx cx;
  const int* irec = e.irec + HB_EP_NI * i;
  const int cause = respawn_decide(RK, irec);
  if (cause == 0) return;
  __shared__ double sh[PD_DRAW + 2 + 2 * PD_KNOTS + HB_PD_N + Profile::stored + Ground::size];
  __shared__ int nk;
  double* u = sh;
  double* a = u + PD_DRAW;
  double* rel = a + 2;
  double* pk = rel + PD_KNOTS;
  double* row_s = pk + PD_KNOTS;
  double* pro_s = row_s + HB_PD_N;
  double* map_s = pro_s + Profile::stored;
  const int* itot = rs.itot + HB_RS_NI * i;
  ProfileDrawRows r{};
  r.prof = pb.prof + size_t(Profile::stored) * i;
  r.knots = pd.knots + PD_KNOTS * i;
  r.row = pd.row + HB_PD_N * i;
  r.map = gmap ? gmap + size_t(Ground::size) * i : nullptr;
  if (cx.lane < 2) a[cx.lane] = K.dir[cx.lane];
  __syncthreads();
  if (K.log_capacity > 0)
    profile_draw_log_append(cx, K.log_capacity, cause, a, irec, e.drec + HB_EP_ND * i, itot, r.row, pd.count + i,
                            pd.log + size_t(i) * pd.log_cap * HB_PD_LOG_W);
  if (cx.lane < PD_BLOCKS) profile_draw_block(K, RK.instance_offset + uint32_t(i), uint32_t(itot[HB_RS_I_EPISODE_INDEX] + 1), cx.lane, u, nullptr);
  __syncthreads();
  if (cx.lane == 0) nk = profile_draw_knots(K, u, profile_draw_s0(a, rs.q_spawn + 16 * i), ground_z, rel, pk, row_s);
  __syncthreads();
  profile_compose(cx, nk, a, pk, row_s + HB_PD_MUS, pro_s);
  if (r.map) ground_compose(cx, nk, a, rel, map_s);
  profile_draw_store(cx, r, pro_s, pk, row_s, map_s);
}

// ---- scenario draw at respawn (hb_plant_set_scenario, hb_scenario.hpp): one wavefront per instance, ahead of k_plant_respawn -------------
// Every lane reads k_plant_respawn's decision from the instance's still unchanged record (the same words: wave-uniform), and a wavefront
// whose instance stays leaves after those loads.  A respawning wavefront appends the log row of the finished episode (all lanes, from the
// scen still in place), draws its Philox blocks one per lane into LDS, stages its terrain record in LDS (all lanes), lets
// lane 0 compose (the one sequential piece) and then writes terrain record, DevModel record, push record and scen with all lanes,
// consecutive lanes on consecutive words.  ter / mdl: null where no channel of the pair is on.
__global__ __launch_bounds__(64) void k_plant_scenario(ScenarioBatch sc, hb_scenario_config K, hb_respawn_config RK, RespawnBatch rs, EpisodeBatch e,
                                                       double* ter, DevModel* mdl, const DevModel* __restrict__ M, double ground_z) {
  const int i = blockIdx.x;
  const DeviceCtx cx;
  const int* irec = e.irec + HB_EP_NI * i;
  const int cause = respawn_decide(RK, irec);
  if (cause == 0) return;
  __shared__ double sh[SC_DRAW + Terrain::size + SC_MODEL_WORDS + HB_SC_N + SC_PUSH + SC_WORK];
  double* u = sh;
  double* ter_s = u + SC_DRAW;
  double* mdl_s = ter_s + Terrain::size;
  double* scen_s = mdl_s + SC_MODEL_WORDS;
  double* push_s = scen_s + HB_SC_N;
  double* work = push_s + SC_PUSH;
  const int* itot = rs.itot + HB_RS_NI * i;
  ScenarioRows r{};
  r.ter = ter ? ter + size_t(Terrain::size) * i : nullptr;
  r.mdl = mdl ? reinterpret_cast<double*>(mdl + i) : nullptr;
  r.push = sc.push + SC_PUSH * i;
  r.scen = sc.scen + HB_SC_N * i;
  if (K.log_capacity > 0)
    scenario_log_append(cx, K.log_capacity, cause, irec, e.drec + HB_EP_ND * i, itot, r.scen, sc.count + i,
                        sc.log + size_t(i) * sc.log_cap * HB_SC_LOG_W);
  if (cx.lane < SC_BLOCKS && scenario_block_needed(K, cx.lane))
    scenario_draw_block(K, RK.instance_offset + uint32_t(i), uint32_t(itot[HB_RS_I_EPISODE_INDEX] + 1), cx.lane, u, nullptr);
  if (r.ter)
    for (int a = cx.lane; a < Terrain::size; a += cx.nlanes) ter_s[a] = r.ter[a];
  __syncthreads();
  if (cx.lane == 0)   // (modelvar_compose writes the whole staged DevModel: the nominal copy, then the varied entries)
    scenario_compose(K, u, rs.q_spawn + 16 * i, ground_z, *M, ter_s, reinterpret_cast<DevModel*>(mdl_s), scen_s, push_s, work);
  __syncthreads();
  scenario_store(cx, r, ter_s, mdl_s, push_s, scen_s);
}

// The push of the scenario: one thread per instance, ahead of the plant kernel.  Writes the instance's external wrench for the step that
// follows from its push record and the STEPS of its current episode record.
__global__ __launch_bounds__(64) void k_plant_push(ScenarioBatch sc, hb_scenario_config K, EpisodeBatch e, double* wrench) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sc.B) return;
  scenario_push_wrench(K, sc.push + SC_PUSH * i, e.irec[HB_EP_NI * i + HB_EP_I_STEPS], wrench + 6 * i);
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

// What a base form of the planner or the filter passes its body for the maps of its instances: nothing.  (Both base forms stay written out
// for now, each under the instantiation it spells)
struct NoMap {};

// planner step: FOUR lanes per instance, one per foot (refgen_plan: the four planner loops and the leg evaluations side by side; the lane
// of foot 0 finishes with the shooting grid and the knots) — thread-per-instance the kernel was a 0.26 ms chain on 64 wavefronts
// init_flag (or null): per-instance "take the latest stance positions from the observation", the pending flag of a respawn
// ONE body for the three forms that follow; MAP (hb_forms.hpp) is the map the planner puts its points to, g the
// maps of the instances of b (NoMap, hb_layout.hpp GroundBatch or GroundFieldBatch).  The batches and the config come by reference: by
// value the inlined body was allocated and scheduled further from the kernels it replaces.
// SOLE = 1: the sole forms (hb_ground_set_foothold) — F the configuration, sb the choice read-back of the instances of b.  The partner
// point's stance x, y, which the init_stance block below or the planner's refresh may write in this launch, are ordered inside
// refgen_plan (fence and wave barrier, as the staging below: the four lanes of an instance share a wavefront).
template <int MAP, class G, int SOLE = 0>
__device__ __forceinline__ void refgen_step(const Batch& b, const RefgenBatch& r, const G& g, const DevModel* __restrict__ M, const hb_refgen_config& K,
                                            double horizon, const int* __restrict__ init_flag, const hb_foothold_config* F = nullptr,
                                            const SoleBatch* sb = nullptr) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = gid >> 2, foot = gid & 3;
  if (i >= b.B) return;   // (a whole group of four leaves together)
  const double* x_now = b.x0 + size_t(i) * HB_NX;
  double* stance = r.stance + size_t(i) * 12;
  if (r.init_stance || (init_flag && init_flag[i])) {
    const Mat3<double> R0 = rg_rot_zyx(x_now + 9);
    const Vec3<double> p0(x_now[6], x_now[7], x_now[8]);
    const double* qj = x_now + 12;
    LegOut<double> L;
    leg_eval<double>(*M, foot & 1, [qj](int j) { return qj[j]; }, [](int) { return 0.0; }, L);
    st3(stance + 3 * foot, p0 + R0 * ((foot >> 1) ? L.foot[1] : L.foot[0]));
  }
  const double* gnd = nullptr;
  const double* __restrict__ gz = nullptr;
  [[maybe_unused]] double hdr[GroundField::size];
  if constexpr (MAP == MAP_PROFILE) {
    // The four lanes of an instance stage its record in LDS first (16 instances x 50 doubles per wavefront): a foot puts some thirty points
    // to the map one after the other, each a scan whose loads hang on the point before, and from global memory those chains were half the
    // kernel.
    __shared__ double maps[16 * Ground::size];
    double* rec = maps + (threadIdx.x >> 2) * Ground::size;
    for (int k = foot; k < Ground::size; k += 4) rec[k] = g.map[size_t(i) * Ground::size + k];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    gnd = rec;
  } else if constexpr (MAP == MAP_FIELD) {
    // The header's eight doubles are read once into registers (field_cell indexes them statically); the heights stay in global memory —
    // 8 KB per instance, sixteen instances per wavefront: staged they would leave a CU one workgroup — and an evaluation issues its four
    // loads together.
    const double* __restrict__ gh = g.hdr + size_t(i) * GroundField::size;
#pragma unroll
    for (int k = 0; k < GroundField::size; ++k) hdr[k] = gh[k];
    gnd = hdr;
    gz = g.z + size_t(i) * GroundField::nz;
  }
  const size_t N = b.Nmax;
  int st;
  if constexpr (SOLE) {
    const RgSole sole{F, sb->shift + 2 * size_t(i), sb->defect + 2 * size_t(i), sb->level + 2 * size_t(i)};
    st = refgen_plan<MAP, 1>(*M, K, r.n_ev[i], r.ev + size_t(i) * HB_MAX_EVENTS, r.modes + size_t(i) * (HB_MAX_EVENTS + 1), r.t0[i], horizon,
                             x_now, r.cmd + size_t(i) * 4, stance, r.phases + size_t(i) * 4 * (HB_MAX_EVENTS + 1) * RG_PHASE, b.Nmax,
                             b.n_nodes + i, b.t + size_t(i) * (N + 1), r.n_knots + i, r.knot_t + size_t(i) * RG_MAX_KNOTS,
                             r.knot_x + size_t(i) * RG_MAX_KNOTS * HB_NX, foot, 4, gnd, gz, sole);
  } else {
    st = refgen_plan<MAP>(*M, K, r.n_ev[i], r.ev + size_t(i) * HB_MAX_EVENTS, r.modes + size_t(i) * (HB_MAX_EVENTS + 1), r.t0[i], horizon,
                          x_now, r.cmd + size_t(i) * 4, stance, r.phases + size_t(i) * 4 * (HB_MAX_EVENTS + 1) * RG_PHASE, b.Nmax,
                          b.n_nodes + i, b.t + size_t(i) * (N + 1), r.n_knots + i, r.knot_t + size_t(i) * RG_MAX_KNOTS,
                          r.knot_x + size_t(i) * RG_MAX_KNOTS * HB_NX, foot, 4, gnd, gz);
  }
  // status of the instance: 2 (grid too long, from the lane of foot 0) wins, else 1 if any foot reported a phase without its events
  int any = st == 1 ? 1 : 0;
  any |= __shfl_xor(any, 1, 64);
  any |= __shfl_xor(any, 2, 64);
  if (foot == 0) r.status[i] = st == 2 ? 2 : any;
}
__global__ __launch_bounds__(64) void k_refgen(Batch b, RefgenBatch r, const DevModel* __restrict__ M, hb_refgen_config K, double horizon,
                                               const int* __restrict__ init_flag) {
  // refgen_step<MAP_NONE>(b, r, NoMap{}, M, K, horizon, init_flag) written out (timing)
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = gid >> 2, foot = gid & 3;
  if (i >= b.B) return;   // (a whole group of four leaves together)
  const double* x_now = b.x0 + size_t(i) * HB_NX;
  double* stance = r.stance + size_t(i) * 12;
  if (r.init_stance || (init_flag && init_flag[i])) {
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
  int any = st == 1 ? 1 : 0;
  any |= __shfl_xor(any, 1, 64);
  any |= __shfl_xor(any, 2, 64);
  if (foot == 0) r.status[i] = st == 2 ? 2 : any;
}
// the ground form (hb_ground_set_profile; launched only while a profile map is in force)
__global__ __launch_bounds__(64) void k_refgen_ground(Batch b, RefgenBatch r, GroundBatch g, const DevModel* __restrict__ M, hb_refgen_config K,
                                                      double horizon, const int* __restrict__ init_flag) {
  refgen_step<MAP_PROFILE>(b, r, g, M, K, horizon, init_flag);
}
// the field form (hb_ground_set_field; launched only while a field map is in force)
__global__ __launch_bounds__(64) void k_refgen_gfield(Batch b, RefgenBatch r, GroundFieldBatch g, const DevModel* __restrict__ M, hb_refgen_config K,
                                                      double horizon, const int* __restrict__ init_flag) {
  refgen_step<MAP_FIELD>(b, r, g, M, K, horizon, init_flag);
}
// the sole forms of the two (hb_ground_set_foothold, mode 1; launched only while a map is in force and the mode is on)
__global__ __launch_bounds__(64) void k_refgen_ground_sole(Batch b, RefgenBatch r, GroundBatch g, const DevModel* __restrict__ M, hb_refgen_config K,
                                                           double horizon, const int* __restrict__ init_flag, hb_foothold_config F, SoleBatch sb) {
  refgen_step<MAP_PROFILE, GroundBatch, 1>(b, r, g, M, K, horizon, init_flag, &F, &sb);
}
__global__ __launch_bounds__(64) void k_refgen_gfield_sole(Batch b, RefgenBatch r, GroundFieldBatch g, const DevModel* __restrict__ M, hb_refgen_config K,
                                                           double horizon, const int* __restrict__ init_flag, hb_foothold_config F, SoleBatch sb) {
  refgen_step<MAP_FIELD, GroundFieldBatch, 1>(b, r, g, M, K, horizon, init_flag, &F, &sb);
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
// ONE body for the three forms that follow: MAP (hb_forms.hpp) is the map whose heights the foot-height rows
// measure, g the maps of the instances of e.  The profile record is read through the pointer from global memory, and so is the field
// header (four evaluations a tick, uniform over the wave); the field heights come from global memory.
template <int MAP, class G>
__device__ __forceinline__ void estimator_step(const EstBatch& e, const G& g, const DevModel* __restrict__ M, const hb_estimator_config& K, double dt) {
  const int i = blockIdx.x;
  __shared__ double lds[EstLds::total];
  const DeviceCtx cx;
  const EstIn in{e.quat + 4 * i, e.w_local + 3 * i, e.a_local + 3 * i, e.qj + 10 * i, e.qdj + 10 * i, e.contact + 4 * i};
  const double *gnd = nullptr, *gz = nullptr;
  if constexpr (MAP == MAP_PROFILE) {
    gnd = g.map + size_t(i) * Ground::size;
  } else if constexpr (MAP == MAP_FIELD) {
    gnd = g.hdr + size_t(i) * GroundField::size;
    gz = g.z + size_t(i) * GroundField::nz;
  }
  estimator_update<MAP>(cx, *M, K, dt, in, e.xhat + 18 * i, e.P + 324 * size_t(i), e.yaw_last + i, lds, e.rbd + HB_NRBD * i, e.x + HB_NX * i, gnd, gz);
  if (e.res_rbd) {
    __syncthreads();  // lane 0 wrote the outputs
    for (int c = cx.lane; c < HB_NRBD; c += 64) e.res_rbd[HB_NRBD * i + c] = e.rbd[HB_NRBD * i + c];
    for (int c = cx.lane; c < HB_NX; c += 64) e.res_x0[HB_NX * i + c] = e.x[HB_NX * i + c];
  }
}
__global__ __launch_bounds__(64) void k_estimator(EstBatch e, const DevModel* __restrict__ M, hb_estimator_config K, double dt) {
  // estimator_step<MAP_NONE>(e, NoMap{}, M, K, dt) written out (timing)
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
// the ground form (hb_ground_set_profile)
__global__ __launch_bounds__(64) void k_estimator_ground(EstBatch e, GroundBatch g, const DevModel* __restrict__ M, hb_estimator_config K, double dt) {
  estimator_step<MAP_PROFILE>(e, g, M, K, dt);
}
// the field form (hb_ground_set_field)
__global__ __launch_bounds__(64) void k_estimator_gfield(EstBatch e, GroundFieldBatch g, const DevModel* __restrict__ M, hb_estimator_config K, double dt) {
  estimator_step<MAP_FIELD>(e, g, M, K, dt);
}
// test hook (hb_ground_eval): the height function at n points, one thread each; inst[p] is the instance whose map point p is put to,
// segment[p] the segment of a profile map or the facet id of a field map
template <int MAP, class G>
__device__ __forceinline__ void ground_eval_step(int n, const G& g, const int* __restrict__ inst, const double* __restrict__ xy, double* __restrict__ height,
                                                 int* __restrict__ segment) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const double *gnd, *gz = nullptr;
  if constexpr (MAP == MAP_FIELD) {
    gnd = g.hdr + size_t(inst[p]) * GroundField::size;
    gz = g.z + size_t(inst[p]) * GroundField::nz;
  } else {
    gnd = g.map + size_t(inst[p]) * Ground::size;
  }
  int id = 0;
  height[p] = map_height<MAP>(gnd, gz, xy[2 * p], xy[2 * p + 1], &id);
  segment[p] = id;
}
__global__ __launch_bounds__(64) void k_ground_eval(int n, GroundBatch g, const int* __restrict__ inst, const double* __restrict__ xy,
                                                    double* __restrict__ height, int* __restrict__ segment) {
  ground_eval_step<MAP_PROFILE>(n, g, inst, xy, height, segment);
}
__global__ __launch_bounds__(64) void k_ground_field_eval(int n, GroundFieldBatch g, const int* __restrict__ inst, const double* __restrict__ xy,
                                                          double* __restrict__ height, int* __restrict__ segment) {
  ground_eval_step<MAP_FIELD>(n, g, inst, xy, height, segment);
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
// host side: the C ABI of include/hunter_hip.h, by subsystem (k_publish, in hb_api_wbc.hpp, is the last kernel of the translation unit)
// ===========================================================================================================
#include "hb_api_ctx.hpp"
#include "hb_api_mpc.hpp"
#include "hb_api_wbc.hpp"
#include "hb_api_refgen.hpp"
#include "hb_api_plant.hpp"
#include "hb_api_episode.hpp"
#include "hb_api_scan.hpp"
#include "hb_api_est.hpp"
#include "hb_api_lcm.hpp"
#include "hb_api_ranges.hpp"
#include "hb_api_ground.hpp"
#include "hb_api_unit.hpp"
