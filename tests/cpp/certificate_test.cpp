// Exercises the KKT certificate of include/hunter_hip.hpp's Wbc (enableCertificate, certificate, dualSolution):
//   certificate_test <params.bin> <inputs.bin> <result.bin>
//       inputs.bin (written by tests/test_cpp_certificate.py): int32 batch; xDes[B][22]; uDes[B][22]; rbd[B][32]; mode[B] (int32)
//       result.bin: sol[B][38], certificate[B][HB_WBC_CERT_SIZE], dual[B][HB_WBC_NCONS_MAX]
//   Before that it checks the refusals: certificate() before any update (HB_ERR_STATE) and enableCertificate on a
//   HierarchicalWbc context (HB_ERR_ARG).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "hunter_hip.hpp"

using namespace hunter_hip;

template <class T>
static void readv(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
}
static void writev(std::FILE* f, const vector_t& v) { std::fwrite(v.data(), sizeof(double), v.size(), f); }

int main(int argc, char** argv) {
  if (argc < 4) return 64;
  hb_model model;
  hb_config config;
  loadPackagedParameters(argv[1], model, config);
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 2;
  int32_t B = 0;
  if (std::fread(&B, sizeof(int32_t), 1, f) != 1 || B <= 0) return 2;
  vector_t xd, ud, rbd;
  std::vector<int32_t> mode;
  readv(f, xd, size_t(B) * HB_NX);
  readv(f, ud, size_t(B) * HB_NU);
  readv(f, rbd, size_t(B) * HB_NRBD);
  readv(f, mode, size_t(B));
  std::fclose(f);

  {  // refusal on HierarchicalWbc
    hb_config hc = config;
    hc.wbc_type = 1;
    Wbc hw{Context(model, hc, B, 4)};
    try {
      hw.enableCertificate(true);
      std::printf("HierarchicalWbc context accepted the certificate\n");
      return 3;
    } catch (const Error& e) {
      if (e.status() != HB_ERR_ARG) return 3;
      std::printf("hierarchical refused: status %d\n", e.status());
    }
  }
  Wbc wbc{Context(model, config, B, 4)};
  wbc.enableCertificate(true);
  try {
    wbc.certificate();
    std::printf("certificate before any update was returned\n");
    return 4;
  } catch (const Error& e) {
    if (e.status() != HB_ERR_STATE) return 4;
    std::printf("no update yet: status %d\n", e.status());
  }
  const vector_t sol = wbc.update(xd, ud, rbd, mode, 0.002);
  const vector_t cert = wbc.certificate();
  vector_t dual;
  for (int32_t i = 0; i < B; ++i) {
    const vector_t y = wbc.dualSolution(size_t(i));
    dual.insert(dual.end(), y.begin(), y.end());
  }
  std::FILE* o = std::fopen(argv[3], "wb");
  if (!o) return 2;
  writev(o, sol);
  writev(o, cert);
  writev(o, dual);
  std::fclose(o);
  std::printf("ok: %d instances, r_stat / scale of instance 0: %.3e\n", B, cert[HB_WBC_CERT_R_STAT] / cert[HB_WBC_CERT_SCALE]);
  return 0;
}
