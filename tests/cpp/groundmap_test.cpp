// The ground map through the C++ host adapter (include/hunter_hip.hpp: ReferenceManager::setGroundProfile,
// KalmanFilterEstimate::setGroundProfile):
//   groundmap_test <params.bin>
// a map set through the reference manager comes back from hb_ground_get_profile as stored (normalised direction, knots, slopes); a second
// one set through the estimator replaces it (one map per context); a refused map leaves it in place; clearing ends it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "hunter_hip.hpp"

using namespace hunter_hip;

struct Stored {
  std::vector<int32_t> n;
  vector_t dir, knots, slopes;
};
static Stored stored(const Context& c) {
  const size_t B = size_t(c.batch());
  Stored s;
  s.n.resize(B); s.dir.resize(B * 2); s.knots.resize(B * HB_PROFILE_MAX_KNOTS * 2); s.slopes.resize(B * (HB_PROFILE_MAX_KNOTS - 1));
  c.check(hb_ground_get_profile(c.get(), s.n.data(), s.dir.data(), s.knots.data(), s.slopes.data()), "hb_ground_get_profile");
  return s;
}

int main(int argc, char** argv) {
  if (argc < 2) return 64;
  const Parameters p = loadParametersBlob(argv[1]);
  const int B = 2, N = 40;
  Context ctx(p.model, p.config, B, N);
  ReferenceManager refs(ctx, p.refgen, makeGaitConfig(p, false));
  KalmanFilterEstimate est(ctx, p.estimator);
  const size_t K = HB_PROFILE_MAX_KNOTS;
  std::vector<int32_t> n = {4, 2};
  vector_t dir = {3.0, 4.0, 0.0, -2.0}, knots(size_t(B) * K * 2, 0.0);
  const double curb[8] = {-1.0, 0.0, 0.25, 0.0, 0.28125, 0.03125, 2.0, 0.03125}, ramp[4] = {0.0, 0.0, 4.0, 0.5};
  std::memcpy(knots.data(), curb, sizeof curb);
  std::memcpy(knots.data() + K * 2, ramp, sizeof ramp);
  refs.setGroundProfile(n, dir, knots);
  Stored s = stored(ctx);
  if (s.n != n || s.knots != knots) return 3;
  if (s.dir[0] != 3.0 / 5.0 || s.dir[1] != 4.0 / 5.0 || s.dir[2] != 0.0 || s.dir[3] != -1.0) return 4;
  if (s.slopes[0] != 0.0 || s.slopes[1] != 1.0 || s.slopes[2] != 0.0 || s.slopes[3] != 0.0 || s.slopes[K - 1] != 0.125) return 5;
  // the estimator's setter writes the same map of the context
  knots[3] = knots[1] = 0.01;
  knots[5] = knots[7] = 0.04125;
  est.setGroundProfile(n, dir, knots);
  s = stored(ctx);
  if (s.knots != knots) return 6;
  // a refusal (a riser steeper than sqrt(3)) names the instance and keeps the map in force
  vector_t bad = knots;
  bad[K * 2 + 3] = 9.0;
  try {
    refs.setGroundProfile(n, dir, bad);
    return 7;
  } catch (const Error& e) {
    if (e.status() != HB_ERR_ARG || std::strstr(e.what(), "instance 1") == nullptr) return 7;
    std::printf("steep map refused: %s\n", e.what());
  }
  if (stored(ctx).knots != knots) return 8;
  // off
  refs.setGroundProfile({}, {}, {});
  try {
    stored(ctx);
    return 9;
  } catch (const Error& e) {
    if (e.status() != HB_ERR_STATE) return 9;
  }
  std::printf("ok: ground map round trip\n");
  return 0;
}
