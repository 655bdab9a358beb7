// KKT certificate and costates of the projected stage QP of one robot instance (include/hunter_hip.h, HB_MPC_CERT_*), from what a solve
// leaves resident: the stage records of k_lq_trip, the gains of the backward sweep and the step of the forward sweep.  Run on demand
// (hb_mpc_get_certificate); no kernel of the update reads or writes anything here.
//   mpc_cert_node    node-parallel: u~ = K~ dx + k~, the costate source c = q~ + Q~ dx + P~' u~, the stationarity source
//                    d = r~ + P~ dx + R~ u~, the dynamics residual over all 22 rows of the record, the node's objective term and norms
//   mpc_cert_sweep_* per instance, backward:  lambda_k = c_k + A~' lambda_(k+1),  stat_k = d_k + B~' lambda_(k+1);  then the eight fields
// Every dot product is split four ways in the order of the forward sweep (fwd_sum4): partial q takes the terms q, q + 4, ...
#pragma once
#include "hb_riccati.hpp"

namespace hb {

constexpr int MPC_CERT_SIZE = 8;   // HB_MPC_CERT_SIZE
// what mpc_cert_node leaves per node for the sweep (and for the u~ output)
struct CertNode {
  static constexpr int ut = 0;     // 12
  static constexpr int c = 12;     // 22
  static constexpr int d = 34;     // 12
  static constexpr int part = 46;  // 7: objective term, dynamics residual (node 0: and |dx_0|), |r~|, |P~ dx|, |R~ u~|, max(|dx_k|, |dx_(k+1)|), |u~|
  static constexpr int size = 56;
};
constexpr int CERT_REC_LEN = REC_qT + 22;   // the Riccati part of a record: [A~ b~ B~ .] [P~ r~ R~ .] [Q~ packed | q~]
struct CertLds {
  static constexpr int rec = 0;                  // record image, REC_* layout
  static constexpr int G = CERT_REC_LEN;         // [K~ | k~ | .]
  static constexpr int dx = G + GAIN_SIZE;       // 22 (+2)
  static constexpr int dxn = dx + 24;            // 22 (+2)
  static constexpr int ut = dxn + 24;            // 12
  static constexpr int Qdx = ut + 12;            // 22 (+2)
  static constexpr int w = Qdx + 24;             // per-row terms for the node's reductions
  static constexpr int w_obj = w, w_res = w + 34, w_dx = w + 56, w_r = w + 78, w_P = w + 90, w_R = w + 102, w_u = w + 114;
  static constexpr int total = w + 128;
};
static_assert(CERT_REC_LEN % 2 == 0 && CertLds::G % 2 == 0 && GAIN_SIZE % 2 == 0, "16-byte staging");
struct CertSweepLds {
  static constexpr int AB = 0;                   // 22 rows of [A~ b~ B~ .]
  static constexpr int lam = REC_PR;             // 22 (+2): lambda_(k+1)
  static constexpr int lamn = lam + 24;          // 22 (+2)
  static constexpr int mstat = lamn + 24;        // 12: running max |stat| per input row
  static constexpr int mbtl = mstat + 12;        // 12: running max |B~' lambda| per input row
  static constexpr int mlam = mbtl + 12;         // 22 (+2): running max |lambda| per state row
  static constexpr int red = mlam + 24;          // 64 x 8: per-slot partials of the node reductions
  static constexpr int total = red + 512;
};

// max that keeps a NaN once it has seen one
HB_HD double cert_max(double a, double b) { return (b > a || b != b) ? b : a; }

// init + sum_j m(j) v(j), j < N, split four ways as the forward sweep does: partial q takes j = q, q + 4, ..., summed (p0 + p1) + (p2 + p3)
template <int N, class MF, class VF>
HB_HD double cert_dot4(double init, MF m, VF v) {
  double p[4] = {init, 0.0, 0.0, 0.0};
  constexpr int N4 = N & ~3;
#pragma unroll
  for (int j = 0; j < N4; j += 4) {
    p[0] = fma(m(j), v(j), p[0]);
    p[1] = fma(m(j + 1), v(j + 1), p[1]);
    p[2] = fma(m(j + 2), v(j + 2), p[2]);
    p[3] = fma(m(j + 3), v(j + 3), p[3]);
  }
  if (N4 < N) p[0] = fma(m(N4), v(N4), p[0]);
  if (N4 + 1 < N) p[1] = fma(m(N4 + 1), v(N4 + 1), p[1]);
  if (N4 + 2 < N) p[2] = fma(m(N4 + 2), v(N4 + 2), p[2]);
  return fwd_sum4(p);
}

// Reference staging of one node (host emulation; the kernel uses 16-byte loads): record part, gains, dx_k, dx_(k+1)
template <class Ctx>
HB_HD void mpc_cert_stage(const Ctx& cx, double* lds, const double* rec, const double* gains, const double* dx2) {
  for (int e = cx.lane; e < CERT_REC_LEN; e += cx.nlanes) lds[CertLds::rec + e] = rec[e];
  for (int e = cx.lane; e < GAIN_SIZE; e += cx.nlanes) lds[CertLds::G + e] = gains[e];
  for (int e = cx.lane; e < 44; e += cx.nlanes) lds[e < 22 ? CertLds::dx + e : CertLds::dxn + e - 22] = dx2[e];
  cx.sync();
}

// One node on its staged image; `first`: node 0, whose dynamics residual also carries |dx_0|.  out: CertNode.
template <class Ctx>
HB_HD void mpc_cert_node(const Ctx& cx, double* lds, bool first, double* out) {
  const double* rec = lds + CertLds::rec;
  const double* PR = rec + REC_PR;
  const double* Qs = rec + REC_QT;
  const double* G = lds + CertLds::G;
  const double* dx = lds + CertLds::dx;
  const double* dxn = lds + CertLds::dxn;
  double* ut = lds + CertLds::ut;
  double* Qdx = lds + CertLds::Qdx;
  // phase A (needs dx): u~ = k~ + K~ dx exactly as the forward sweep forms it; Q~ dx from the packed upper triangle
  for (int r = cx.lane; r < 12 + 22; r += cx.nlanes) {
    if (r < 12) {
      const double* row = G + r * 22;
      ut[r] = cert_dot4<22>(G[264 + r], [row](int j) { return row[j]; }, [dx](int j) { return dx[j]; });
    } else {
      const int i = r - 12;
      Qdx[i] = cert_dot4<22>(0.0, [Qs, i](int j) { return Qs[i <= j ? rec_Qidx(i, j) : rec_Qidx(j, i)]; }, [dx](int j) { return dx[j]; });
    }
  }
  cx.sync();
  // phase B: state rows (dynamics residual, c), input rows (d)
  for (int r = cx.lane; r < 22 + 12; r += cx.nlanes) {
    if (r < 22) {
      const int i = r;
      const double* row = rec + i * REC_LD;   // entry j of [dx ; u~] multiplies row[j] (j < 22) or row[j + 1]
      const double dyn = cert_dot4<34>(row[REC_CV], [row](int j) { return row[j < 22 ? j : j + 1]; },
                                       [dx, ut](int j) { return j < 22 ? dx[j] : ut[j - 22]; });
      const double ptu = cert_dot4<12>(0.0, [PR, i](int a) { return PR[a * REC_LD + i]; }, [ut](int a) { return ut[a]; });
      const double qi = Qs[REC_QT_PACKED + i];
      out[CertNode::c + i] = (qi + Qdx[i]) + ptu;
      lds[CertLds::w_obj + i] = fma(0.5, Qdx[i], qi) * dx[i];
      lds[CertLds::w_res + i] = fabs(dxn[i] - dyn);
      lds[CertLds::w_dx + i] = cert_max(fabs(dx[i]), fabs(dxn[i]));
    } else {
      const int a = r - 22;
      const double* row = PR + a * REC_LD;
      const double pdx = cert_dot4<22>(0.0, [row](int j) { return row[j]; }, [dx](int j) { return dx[j]; });
      const double ru = cert_dot4<12>(0.0, [row](int j) { return row[REC_CU + j]; }, [ut](int j) { return ut[j]; });
      const double ra = row[REC_CV], ua = ut[a];
      out[CertNode::d + a] = (ra + pdx) + ru;
      out[CertNode::ut + a] = ua;
      lds[CertLds::w_obj + 22 + a] = fma(0.5, ru, ra + pdx) * ua;
      lds[CertLds::w_r + a] = fabs(ra);
      lds[CertLds::w_P + a] = fabs(pdx);
      lds[CertLds::w_R + a] = fabs(ru);
      lds[CertLds::w_u + a] = fabs(ua);
    }
  }
  cx.sync();
  // the node's seven partials, one per lane, each a serial pass in a fixed order
  for (int f = cx.lane; f < 7; f += cx.nlanes) {
    double v = 0.0;
    if (f == 0) {
      for (int e = 0; e < 34; ++e) v += lds[CertLds::w_obj + e];
    } else if (f == 1) {
      for (int e = 0; e < 22; ++e) v = cert_max(v, lds[CertLds::w_res + e]);
      if (first)
        for (int e = 0; e < 22; ++e) v = cert_max(v, fabs(dx[e]));
    } else if (f == 5) {
      for (int e = 0; e < 22; ++e) v = cert_max(v, lds[CertLds::w_dx + e]);
    } else {
      const int base = f == 2 ? CertLds::w_r : f == 3 ? CertLds::w_P : f == 4 ? CertLds::w_R : CertLds::w_u;
      for (int e = 0; e < 12; ++e) v = cert_max(v, lds[base + e]);
    }
    out[CertNode::part + f] = v;
  }
  cx.sync();
}

// Start of the backward pass: lambda_n = 0 (no terminal cost), maxima 0
template <class Ctx>
HB_HD void mpc_cert_sweep_init(const Ctx& cx, double* lds) {
  for (int e = cx.lane; e < CertSweepLds::total - CertSweepLds::lam; e += cx.nlanes) lds[CertSweepLds::lam + e] = 0.0;
  cx.sync();
}
// One stage on the staged rows of [A~ b~ B~ .]: lane c owns column c of A~ (c < 22) or of B~ (23 <= c < 35).  cd(c) delivers the lane's
// entry of c_k (c < 22) or d_k (entry c - 23) of the node record; lam_out receives lambda_k.
template <class Ctx, class CD>
HB_HD void mpc_cert_sweep_stage(const Ctx& cx, double* lds, CD cd, double* lam_out) {
  const double* ab = lds + CertSweepLds::AB;
  const double* lam = lds + CertSweepLds::lam;
  for (int c = cx.lane; c < 35; c += cx.nlanes) {
    if (c == REC_CV) continue;
    const double acc = cert_dot4<22>(0.0, [ab, c](int i) { return ab[i * REC_LD + c]; }, [lam](int i) { return lam[i]; });
    if (c < 22) {
      const double v = cd(c) + acc;
      lds[CertSweepLds::lamn + c] = v;
      lam_out[c] = v;
      lds[CertSweepLds::mlam + c] = cert_max(lds[CertSweepLds::mlam + c], fabs(v));
    } else {
      const int a = c - REC_CU;
      lds[CertSweepLds::mstat + a] = cert_max(lds[CertSweepLds::mstat + a], fabs(cd(c) + acc));
      lds[CertSweepLds::mbtl + a] = cert_max(lds[CertSweepLds::mbtl + a], fabs(acc));
    }
  }
  cx.sync();
  for (int c = cx.lane; c < 22; c += cx.nlanes) lds[CertSweepLds::lam + c] = lds[CertSweepLds::lamn + c];
  cx.sync();
}
// The eight fields from the sweep's maxima and the node partials of the instance (`nodes`: its CertNode records).  The node reductions
// run over 64 slots (slot l takes nodes l, l + 64, ...) whatever the number of lanes, then over the slots in order.
template <class Ctx>
HB_HD void mpc_cert_finish(const Ctx& cx, double* lds, const double* nodes, int n, bool certified, double* cert) {
  double* red = lds + CertSweepLds::red;
  for (int l = cx.lane; l < 64; l += cx.nlanes) {
    double s = 0.0, m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = l; k < n; k += 64) {
      const double* p = nodes + size_t(k) * CertNode::size + CertNode::part;
      s += p[0];
#pragma unroll
      for (int f = 0; f < 6; ++f) m[f] = cert_max(m[f], p[1 + f]);
    }
    red[l * 8] = s;
#pragma unroll
    for (int f = 0; f < 6; ++f) red[l * 8 + 1 + f] = m[f];
  }
  cx.sync();
  for (int f = cx.lane; f < MPC_CERT_SIZE; f += cx.nlanes) {
    double v = 0.0;
    if (f == 0) {          // R_DYN
      for (int l = 0; l < 64; ++l) v = cert_max(v, red[l * 8 + 1]);
    } else if (f == 1) {   // R_STAT
      for (int a = 0; a < 12; ++a) v = cert_max(v, lds[CertSweepLds::mstat + a]);
    } else if (f == 2) {   // OBJ
      for (int l = 0; l < 64; ++l) v += red[l * 8];
    } else if (f == 3) {   // STEP_MAX
      for (int l = 0; l < 64; ++l) v = cert_max(v, red[l * 8 + 5]);
    } else if (f == 4) {   // U_MAX
      for (int l = 0; l < 64; ++l) v = cert_max(v, red[l * 8 + 6]);
    } else if (f == 5) {   // LAMBDA_MAX
      for (int c = 0; c < 22; ++c) v = cert_max(v, lds[CertSweepLds::mlam + c]);
    } else if (f == 6) {   // SCALE: no floor
      for (int l = 0; l < 64; ++l) v = cert_max(cert_max(v, red[l * 8 + 2]), cert_max(red[l * 8 + 3], red[l * 8 + 4]));
      for (int a = 0; a < 12; ++a) v = cert_max(v, lds[CertSweepLds::mbtl + a]);
    } else {
      v = double(n);
    }
    if (!certified) v = f == 7 ? 0.0 : __builtin_nan("");
    cert[f] = v;
  }
  cx.sync();
}

}  // namespace hb
