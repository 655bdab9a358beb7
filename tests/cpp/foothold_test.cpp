// The planner's foothold mode through the C++ host adapter (include/hunter_hip.hpp: ReferenceManager::setFootholdConfig,
// getFootholdConfig, getFootholdChoice):
//   foothold_test <params.bin>
// a configuration set through the reference manager comes back from hb_ground_get_foothold as given, with and without a map in force; a
// refused one (n_shift out of range) leaves it in place; mode 0 and nullptr clear it; the choice read-back is refused while the mode is
// off and reads "no foothold" before the first planner pass.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "hunter_hip.hpp"

using namespace hunter_hip;

static bool same(const hb_foothold_config& a, const hb_foothold_config& b) {
  return a.mode == b.mode && a.n_shift == b.n_shift && a.shift_step == b.shift_step && a.flat_tol == b.flat_tol;
}

int main(int argc, char** argv) {
  if (argc < 2) return 64;
  const Parameters p = loadParametersBlob(argv[1]);
  const int B = 2, N = 40;
  Context ctx(p.model, p.config, B, N);
  ReferenceManager refs(ctx, p.refgen, makeGaitConfig(p, false));
  const hb_foothold_config off{};
  if (!same(refs.getFootholdConfig(), off)) return 3;
  // legal without a map in force
  hb_foothold_config cfg{};
  cfg.mode = 1; cfg.n_shift = 3; cfg.shift_step = 0.02; cfg.flat_tol = 0.005;
  refs.setFootholdConfig(&cfg);
  if (!same(refs.getFootholdConfig(), cfg)) return 4;
  std::vector<int32_t> shift, level;
  vector_t defect;
  refs.getFootholdChoice(shift, defect, level);
  for (size_t k = 0; k < shift.size(); ++k)
    if (shift[k] != INT32_MIN || defect[k] != 0.0 || level[k] != 0) return 5;
  // a map beside it: the configuration stays
  const size_t K = HB_PROFILE_MAX_KNOTS;
  std::vector<int32_t> n = {2, 2};
  vector_t dir = {1.0, 0.0, 1.0, 0.0}, knots(size_t(B) * K * 2, 0.0);
  knots[2] = 1.0; knots[K * 2 + 2] = 1.0;
  refs.setGroundProfile(n, dir, knots);
  if (!same(refs.getFootholdConfig(), cfg)) return 6;
  // a refusal keeps the configuration in force
  hb_foothold_config bad = cfg;
  bad.n_shift = HB_FOOTHOLD_MAX_SHIFT + 1;
  try {
    refs.setFootholdConfig(&bad);
    return 7;
  } catch (const Error& e) {
    if (e.status() != HB_ERR_ARG || std::strstr(e.what(), "n_shift") == nullptr) return 7;
    std::printf("configuration refused: %s\n", e.what());
  }
  if (!same(refs.getFootholdConfig(), cfg)) return 8;
  // mode 0 with other fields set: off, stored as all zero; then on again and off by nullptr
  hb_foothold_config zero = cfg;
  zero.mode = 0;
  refs.setFootholdConfig(&zero);
  if (!same(refs.getFootholdConfig(), off)) return 9;
  try {
    refs.getFootholdChoice(shift, defect, level);
    return 10;
  } catch (const Error& e) {
    if (e.status() != HB_ERR_STATE) return 10;
  }
  refs.setFootholdConfig(&cfg);
  refs.setFootholdConfig(nullptr);
  if (!same(refs.getFootholdConfig(), off)) return 11;
  std::printf("ok: foothold configuration round trip\n");
  return 0;
}
