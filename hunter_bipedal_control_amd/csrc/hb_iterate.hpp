// The hand-over of the MPC iterate between calls, one thread's share per call: cold start (k_cold_start) and the warm start onto new
// node tables (k_warm_shift).  The kernels (hb_kernels.hip) keep the launch geometry and the per-batch bookkeeping and call these; the
// host build (tests/host_emu) loops them over all threads of a batch.  Index arithmetic and branches, no lane cooperation.
#pragma once
#include <cstddef>

#include "hb_model.hpp"

namespace hb {

HB_HD int it_min(int a, int b) { return a < b ? a : b; }
HB_HD int it_max(int a, int b) { return a > b ? a : b; }

// cold start: x_k = x0, u_k = weight compensation of mode_k (LeggedRobotInitializer.cpp:67-77).  Thread (node k, lane) of an instance
// with n intervals: mode [Nmax], x0 [HB_NX], x [Nmax + 1][HB_NX], u [Nmax][HB_NU] are the instance's arrays.  Rows beyond n are not written.
HB_HD void cold_start_entry(const DevModel& M, const int* n_nodes, const int* mode, const double* x0, int k, int lane, double* x, double* u) {
  if (k > *n_nodes) return;
  double* xk = x + size_t(k) * HB_NX;
  if (lane < HB_NX) xk[lane] = x0[lane];
  if (k < *n_nodes && lane < HB_NU) {
    bool cf[HB_NC];
    mode_flags(mode[k], cf);
    int nc = 0;
    for (int i = 0; i < HB_NC; ++i) nc += cf[i];
    double v = 0.0;
    if (lane < 12 && lane % 3 == 2 && cf[lane / 3]) v = M.total_mass * M.gravity / nc;
    u[size_t(k) * HB_NU + lane] = v;
  }
}

// One instance's arrays as k_warm_shift sees them: the new tables (n_nodes, t, mode), the grid the previous iterate lives on (np_nodes,
// tp, modep), that iterate (xp, up) and the destination (x, u).  Pointers to the instance's first element; nothing is read before it is needed.
struct WarmShiftInst {
  int Nmax;
  const int* grid_dirty;
  const int* n_nodes;
  const double* t;
  const int* mode;
  const int* np_nodes;
  const double* tp;
  const int* modep;
  const double* xp;
  const double* up;
  double* x;
  double* u;
};

// Warm start across MPC calls, thread (node k, entry e) of one instance: it moves state entry e AND input entry e of its node (the
// interval lookup is the same for both).  The previous call's iterate (xp, up on the grid tp / modep / np_nodes) is brought onto the
// new node tables — OCS2 SqpSolver::initializeStateInputTrajectories [OCS2-knowledge]: inside the previous horizon the state at every
// new node time and the input at the start of every new interval are interpolated linearly from the previous solution; beyond
// it the initializer takes over (LeggedRobotInitializer.cpp:67-77: the state is carried on, the input is the weight
// compensation of the interval's mode).  Defined here: an input is HELD instead of interpolated across a mode
// switch of the previous solution (the neighbouring node belongs to another contact configuration), and the last previous
// interval holds its input.  Instances whose tables did not change keep their iterate (plain copy of every row from the previous
// buffers: the host swapped them).
HB_HD void warm_shift_entry(const DevModel& M, const WarmShiftInst& w, int k, int e) {
  static_assert(HB_NX == HB_NU, "one thread moves entry e of the state and of the input");
  const size_t N = w.Nmax;
  if (k > int(N)) return;
  constexpr bool is_x = true, is_u = true;
  const double* xp = w.xp;
  const double* up = w.up;
  double* xk = w.x + size_t(k) * HB_NX;
  double* uk = w.u + size_t(k) * HB_NU;
  if (!*w.grid_dirty) {
    if (is_x) xk[e] = xp[size_t(k) * HB_NX + e];
    if (is_u && k < int(N)) uk[e] = up[size_t(k) * HB_NU + e];
    return;
  }
  const int n = *w.n_nodes, np = *w.np_nodes;
  if (k > n) return;
  const double* tp = w.tp;
  const int* mp = w.modep;
  const double t = w.t[k];
  // old interval that contains t: the largest i in [0, np - 1] with tp[i] <= t (0 if there is none)
  // Between two MPC calls the grid moves by a fraction of an interval, so the answer is k, k + 1 or k - 1 almost always: those three
  // candidates are tested first with loads that do not depend on one another (one round trip); the bisection (up to seven dependent
  // loads per block) is the fallback.  tp is non-decreasing: i is the answer iff tp[i] <= t and (i is the last or tp[i + 1] > t).
  // (a linear scan was a chain of up to N dependent loads per block: 0.51 ms per 4096 x 100 launch, 0.06 ms of it memory traffic)
  int lo = 0, hi = np > 0 ? np - 1 : 0;
  {
    const int last = hi;
    const int c0 = it_min(it_max(k - 1, 0), last);
    const double t0 = tp[c0], t1 = tp[it_min(c0 + 1, last)], t2 = tp[it_min(c0 + 2, last)], t3 = tp[it_min(c0 + 3, last)];
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
      mode_flags(w.mode[k], cf);
      int nc = 0;
      for (int c = 0; c < HB_NC; ++c) nc += cf[c];
      v = (e < 12 && e % 3 == 2 && cf[e / 3]) ? M.total_mass * M.gravity / nc : 0.0;
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

}  // namespace hb
