// TEST HARNESS: the certificate instantiation of the HierarchicalWbc cascade (hb_hoqp.hpp, hwbc_solve<Ctx, true>) compiled for the host
// with one emulated lane, for tests/test_hwbc_certificate_host.py.  Not part of the product; the product path always runs k_hwbc_cert.
#include <vector>
#include "../../hunter_bipedal_control_amd/csrc/hb_host.hpp"
#include "../../hunter_bipedal_control_amd/csrc/hb_hoqp.hpp"

using namespace hb;
namespace {
struct HostCtx {
  int lane = 0, nlanes = 1;
  void sync() const {}
};
}  // namespace

extern "C" {
// sol in/out as in k_hwbc (kept when a kernel basis is given up); cert [3][HB_HWBC_CERT_SIZE], x_levels [3][38], slack0 [40],
// dual [3][40]; active [2][40]: the final working-set flags of the QPs of levels 1 and 2 by inequality row
void cert_hwbc(const hb_model* m, const hb_config* c, const double* xdes, const double* udes, const double* rbd, int mode, double* sol,
               int* status, double* cert, double* x_levels, double* slack0, double* dual, int* active) {
  DevModel d = make_dev_model(*m);
  DevConfig dc = make_dev_config(*c, d);
  std::vector<double> lds(HoL::total + HoCertLds::total, 0.0);
  hwbc_solve<HostCtx, true>(HostCtx{}, d, dc, xdes, udes, rbd, mode, lds.data(), sol, status, 3, cert, x_levels, slack0, dual);
  const int* act = reinterpret_cast<const int*>(lds.data() + HoL::total + HoCertLds::act);
  for (int i = 0; i < 80; ++i) active[i] = act[i];
}
}
