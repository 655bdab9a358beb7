// Exercises the per-level certificate of include/hunter_hip.hpp's Wbc on a HierarchicalWbc context (enableLevelCertificate,
// levelCertificate):
//   hwbc_certificate_test <params.bin> <inputs.bin> <result.bin>
//       inputs.bin (written by tests/test_cpp_hwbc_certificate.py): int32 batch; xDes[B][22]; uDes[B][22]; rbd[B][32]; mode[B] (int32)
//       result.bin: sol[B][38], cert[B][3][HB_HWBC_CERT_SIZE], xLevels[B][3][38], slack0[B][40], dual[B][3][40]
//   Before that it checks the refusals: enableLevelCertificate on a WeightedWbc context (HB_ERR_ARG) and levelCertificate() before
//   any update (HB_ERR_STATE).
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

  {  // refusal on WeightedWbc
    Wbc ww{Context(model, config, B, 4)};
    try {
      ww.enableLevelCertificate(true);
      std::printf("WeightedWbc context accepted the level certificate\n");
      return 3;
    } catch (const Error& e) {
      if (e.status() != HB_ERR_ARG) return 3;
      std::printf("weighted refused: status %d\n", e.status());
    }
  }
  hb_config hc = config;
  hc.wbc_type = 1;
  Wbc wbc{Context(model, hc, B, 4)};
  wbc.enableLevelCertificate(true);
  try {
    wbc.levelCertificate();
    std::printf("certificate before any update was returned\n");
    return 4;
  } catch (const Error& e) {
    if (e.status() != HB_ERR_STATE) return 4;
    std::printf("no update yet: status %d\n", e.status());
  }
  const vector_t sol = wbc.update(xd, ud, rbd, mode, 0.002);
  const Wbc::LevelCertificate& c = wbc.levelCertificate();
  std::FILE* o = std::fopen(argv[3], "wb");
  if (!o) return 2;
  writev(o, sol);
  writev(o, c.cert);
  writev(o, c.xLevels);
  writev(o, c.slack0);
  writev(o, c.dual);
  std::fclose(o);
  std::printf("ok: %d instances, r_stat / scale of level 1 of instance 0: %.3e\n", B,
              c.cert[HB_HWBC_CERT_SIZE + HB_HWBC_CERT_R_STAT] / c.cert[HB_HWBC_CERT_SIZE + HB_HWBC_CERT_SCALE]);
  return 0;
}
