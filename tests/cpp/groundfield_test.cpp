// The field map through the C++ host adapter (include/hunter_hip.hpp: ReferenceManager::setGroundField,
// KalmanFilterEstimate::setGroundField):
//   groundfield_test <params.bin>
// a map set through the reference manager comes back from hb_ground_get_field as stored (normalised direction, origin, spacing, node
// counts, heights); a second one set through the estimator replaces it (one map per context); a refused map leaves it in place; a profile
// map set through either adapter replaces the field map and the reverse; clearing ends it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "hunter_hip.hpp"

using namespace hunter_hip;

struct Stored {
  std::vector<int32_t> n;
  vector_t dir, origin, spacing, heights;
};
static Stored stored(const Context& c) {
  const size_t B = size_t(c.batch()), NZ = size_t(HB_FIELD_MAX_NODES) * HB_FIELD_MAX_NODES;
  Stored s;
  s.n.resize(B * 2); s.dir.resize(B * 2); s.origin.resize(B * 2); s.spacing.resize(B * 2); s.heights.resize(B * NZ);
  c.check(hb_ground_get_field(c.get(), s.n.data(), s.dir.data(), s.origin.data(), s.spacing.data(), s.heights.data()), "hb_ground_get_field");
  return s;
}

int main(int argc, char** argv) {
  if (argc < 2) return 64;
  const Parameters p = loadParametersBlob(argv[1]);
  const int B = 2, N = 40;
  Context ctx(p.model, p.config, B, N);
  ReferenceManager refs(ctx, p.refgen, makeGaitConfig(p, false));
  KalmanFilterEstimate est(ctx, p.estimator);
  const size_t P = HB_FIELD_MAX_NODES, NZ = P * P;
  std::vector<int32_t> n = {3, 2, 32, 32};
  vector_t dir = {3.0, 4.0, 0.0, -2.0}, origin = {-0.25, 0.5, -1.5, -1.5}, spacing = {0.125, 0.25, 0.09375, 0.109375}, heights(size_t(B) * NZ, 0.0);
  heights[0 * P + 1] = 0.03125; heights[1 * P + 0] = 0.015625; heights[2 * P + 1] = -0.0078125;
  for (size_t i = 0; i < P; ++i)
    for (size_t j = 0; j < P; ++j) heights[NZ + i * P + j] = 0.001 * double(i) - 0.0005 * double(j);
  refs.setGroundField(n, dir, origin, spacing, heights);
  Stored s = stored(ctx);
  if (s.n != n || s.heights != heights || s.origin != origin || s.spacing != spacing) return 3;
  if (s.dir[0] != 3.0 / 5.0 || s.dir[1] != 4.0 / 5.0 || s.dir[2] != 0.0 || s.dir[3] != -1.0) return 4;
  // the device evaluates it: a node of instance 1, and the facet under it
  {
    const int32_t inst[1] = {1};
    const double ax = 0.0, ay = -1.0, u = origin[2] + 3.0 * spacing[2], w = origin[3] + 5.0 * spacing[3];
    const double xy[2] = {u * ax - w * ay, u * ay + w * ax};
    double h = 0.0;
    int32_t facet = -1;
    ctx.check(hb_ground_eval(ctx.get(), 1, inst, xy, &h, &facet), "hb_ground_eval");
    if (h != heights[NZ + 3 * P + 5] || facet != 2 * (3 * 31 + 5)) return 5;
  }
  // the estimator's setter writes the same map of the context
  heights[1 * P + 1] = 0.01;
  est.setGroundField(n, dir, origin, spacing, heights);
  s = stored(ctx);
  if (s.heights != heights) return 6;
  // a refusal (a triangle steeper than sqrt(3)) names the instance and keeps the map in force
  vector_t bad = heights;
  bad[NZ + 7 * P + 7] = 9.0;
  try {
    refs.setGroundField(n, dir, origin, spacing, bad);
    return 7;
  } catch (const Error& e) {
    if (e.status() != HB_ERR_ARG || std::strstr(e.what(), "instance 1") == nullptr) return 7;
    std::printf("steep map refused: %s\n", e.what());
  }
  if (stored(ctx).heights != heights) return 8;
  // a profile map replaces it, through either adapter, and the reverse
  {
    const size_t K = HB_PROFILE_MAX_KNOTS;
    std::vector<int32_t> nk = {2, 2};
    vector_t pdir = {1.0, 0.0, 1.0, 0.0}, knots(size_t(B) * K * 2, 0.0);
    knots[2] = 1.0; knots[3] = 0.125; knots[K * 2 + 2] = 2.0;
    est.setGroundProfile(nk, pdir, knots);
    try {
      stored(ctx);
      return 9;
    } catch (const Error& e) {
      if (e.status() != HB_ERR_STATE) return 9;
    }
    std::vector<int32_t> got(B);
    ctx.check(hb_ground_get_profile(ctx.get(), got.data(), nullptr, nullptr, nullptr), "hb_ground_get_profile");
    if (got != nk) return 10;
    refs.setGroundField(n, dir, origin, spacing, heights);
    if (hb_ground_get_profile(ctx.get(), got.data(), nullptr, nullptr, nullptr) != HB_ERR_STATE) return 11;
    if (stored(ctx).heights != heights) return 12;
  }
  // off
  est.setGroundField({}, {}, {}, {}, {});
  try {
    stored(ctx);
    return 13;
  } catch (const Error& e) {
    if (e.status() != HB_ERR_STATE) return 13;
  }
  std::printf("ok: field map round trip\n");
  return 0;
}
