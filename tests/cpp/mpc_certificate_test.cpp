// Exercises the MPC certificate of include/hunter_hip.hpp (MpcMrtInterface::certificate / stageQp, ShardedSolver's forwards):
//   mpc_certificate_test <params.bin> <inputs.bin> <result.bin>
//       inputs.bin (written by tests/test_cpp_mpc_certificate.py): int32 batch, maxNodes; nNodes[B] (int32); t[B][N+1]; mode[B][N] (int32);
//                  xRef[B][N][22]; swingRef[B][N][24]; x0[B][22]
//       result.bin: cert[B][8], costate[B][N+1][22], uTil[B][N][12], then per instance A, B, b, Q, P, R, q, r ([N] stages each) and
//                   nTil[N] (as doubles)
//   Before the solve it checks the refusal: certificate() / stageQp() with no MPC call completed (HB_ERR_STATE); after it, a bad range
//   (HB_ERR_ARG) and the refusal after new references (HB_ERR_STATE).
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

template <class F>
static int statusOf(F f) {
  try {
    f();
  } catch (const Error& e) {
    return e.status();
  }
  return HB_OK;
}

int main(int argc, char** argv) {
  if (argc < 4) return 64;
  hb_model model;
  hb_config config;
  loadPackagedParameters(argv[1], model, config);
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 2;
  int32_t hdr[2] = {0, 0};
  if (std::fread(hdr, sizeof(int32_t), 2, f) != 2 || hdr[0] <= 0 || hdr[1] <= 0) return 2;
  const int32_t B = hdr[0], N = hdr[1];
  ReferenceTables refs;
  vector_t x0;
  readv(f, refs.nNodes, size_t(B));
  readv(f, refs.t, size_t(B) * (N + 1));
  readv(f, refs.mode, size_t(B) * N);
  readv(f, refs.xRef, size_t(B) * N * HB_NX);
  readv(f, refs.swingRef, size_t(B) * N * HB_NC * HB_SWING_REF);
  readv(f, x0, size_t(B) * HB_NX);
  std::fclose(f);

  ShardedSolver solver(model, config, B, N, {0});
  MpcMrtInterface& mpc = solver.shard(0);
  solver.setReferences(refs);
  solver.resetMpcNode(x0);
  int st = statusOf([&] { mpc.certificate(); });
  if (st != HB_ERR_STATE) return 3;
  std::printf("certificate before any solve: status %d\n", st);
  st = statusOf([&] { mpc.stageQp(0); });
  if (st != HB_ERR_STATE) return 3;
  std::printf("stage QP before any solve: status %d\n", st);
  solver.setCurrentObservation(x0);
  solver.advanceMpc();
  st = statusOf([&] { mpc.certificate(1, B); });
  if (st != HB_ERR_ARG) return 4;
  std::printf("bad range: status %d\n", st);
  const MpcMrtInterface::Certificate c = solver.certificate();
  const MpcMrtInterface::Certificate sub = mpc.certificate(1, 2);
  for (size_t e = 0; e < 2 * HB_MPC_CERT_SIZE; ++e)
    if (std::memcmp(&sub.cert[e], &c.cert[HB_MPC_CERT_SIZE + e], sizeof(double)) != 0) return 5;
  std::FILE* o = std::fopen(argv[3], "wb");
  if (!o) return 2;
  writev(o, c.cert);
  writev(o, c.costate);
  writev(o, c.uTil);
  for (int32_t i = 0; i < B; ++i) {
    const MpcMrtInterface::StageQp s = solver.stageQp(i);
    for (const vector_t* v : {&s.A, &s.B, &s.b, &s.Q, &s.P, &s.R, &s.q, &s.r}) writev(o, *v);
    writev(o, vector_t(s.nTil.begin(), s.nTil.end()));
  }
  std::fclose(o);
  solver.setReferences(refs);
  st = statusOf([&] { mpc.certificate(); });
  if (st != HB_ERR_STATE) return 6;
  std::printf("after new references: status %d\n", st);
  std::printf("ok: %d instances, r_stat / scale of instance 0: %.3e\n", B, c.cert[HB_MPC_CERT_R_STAT] / c.cert[HB_MPC_CERT_SCALE]);
  return 0;
}
