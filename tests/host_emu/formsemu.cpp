// TEST HARNESS: csrc/hb_forms.hpp compiled for the host, for tests/test_forms_host.py.
//   formsemu table    prints the table: "code NAME value" per single code, "range NAME first last" per family
//   formsemu check    compares decode_forms + use_ric_bwd4 / use_ric_fwd_wave / lq_trip_len with the expressions the launchers held
//                     before the header existed (copied verbatim below: `sel` is hb_config.reserved, HB_ABLATE_ON the build), for
//                     both builds, over reserved in -1 .. 260 and a grid of (concurrent, Nmax, n_cu); prints "checked N" and
//                     "mismatch ..." lines, exit status 1 if any.
#include <cstdio>
#include <cstring>
#include "../../hunter_bipedal_control_amd/csrc/hb_forms.hpp"

namespace before {   // the thresholds and the expressions as they stood in hb_kernels.hip / hb_api_mpc.hpp
constexpr int kRicBwd4MaxBatch = 512;
constexpr int kRicFwdWaveMaxBatch = 512;
constexpr int kLqTripsPerSlot = 4;
bool four(int sel, int HB_ABLATE_ON, int concurrent) {
  const bool four = sel == 104 || (HB_ABLATE_ON && ((sel >= 24 && sel <= 27) || sel == 199)) || (sel != 101 && !(HB_ABLATE_ON && sel != 0 && sel != 198) && concurrent <= kRicBwd4MaxBatch);
  return four;
}
int lq_trip_len(int sel, int concurrent, int Nmax, int n_cu) {
  if (sel >= 120 && sel <= 124) return 1 << (sel - 120);
  if (sel >= 131 && sel <= 146) return sel - 130;   // any trip length 1..16 (launch-geometry sweeps)
  const long slots = 12L * n_cu;
  for (int sh = 4; sh > 0; --sh)
    if (long(concurrent) * ((Nmax + (1 << sh) - 1) >> sh) >= kLqTripsPerSlot * slots) return 1 << sh;
  return 1;
}
bool one_node(int sel) { return sel == 129; }
bool fwd_wave(int sel, int concurrent) { return sel == 114 || (sel != 111 && concurrent <= kRicFwdWaveMaxBatch); }
}  // namespace before

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "table")) {
    for (const hb::form::Entry& e : hb::form::kTable) {
      if (e.first == e.last) std::printf("code %s %d\n", e.name, e.first);
      else std::printf("range %s %d %d\n", e.name, e.first, e.last);
    }
    return 0;
  }
  if (argc != 2 || std::strcmp(argv[1], "check")) return 2;
  const int concurrents[] = {1, 511, 512, 513, 1024, 2047, 2048, 4096}, nmaxs[] = {1, 44, 100, 108, 200}, ncus[] = {64, 256};
  long checked = 0, bad = 0;
  for (int sel = -1; sel <= 260; ++sel)
    for (int ablate = 0; ablate <= 1; ++ablate) {
      const hb::KernelForms f = hb::decode_forms(sel, ablate != 0);
      for (int c : concurrents)
        for (int N : nmaxs)
          for (int cu : ncus) {
            const bool ok = hb::use_ric_bwd4(f, c) == before::four(sel, ablate, c) && hb::use_ric_fwd_wave(f, c) == before::fwd_wave(sel, c) &&
                            (f.lq == hb::KernelForms::Lq::OneNode) == before::one_node(sel) &&
                            hb::lq_trip_len(f, c, N, cu) == before::lq_trip_len(sel, c, N, cu);
            ++checked;
            if (!ok && ++bad <= 20) std::printf("mismatch reserved %d ablate %d concurrent %d Nmax %d n_cu %d\n", sel, ablate, c, N, cu);
          }
    }
  std::printf("checked %ld\n", checked);
  return bad ? 1 : 0;
}
