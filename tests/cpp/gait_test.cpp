// The two ReferenceManager constructors of include/hunter_hip.hpp side by side:
//   gait_test <params.bin>
// one context gets a vector of host GaitSchedules with the walk-gait selection on, the other an hb_gait_config (the device gait manager,
// no host gait work in preSolverRun).  Over 40 passes with a command step for two of the three instances the node tables of the two
// contexts must be the same bytes, and the commanded instances must have left gait level 0.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "hunter_hip.hpp"

using namespace hunter_hip;

struct Tables {
  std::vector<int32_t> n, mode;
  vector_t t, x, sw;
};
static Tables tables(const Context& c) {
  const size_t B = size_t(c.batch()), N = size_t(c.maxNodes());
  Tables r;
  r.n.resize(B); r.mode.resize(B * N); r.t.resize(B * (N + 1)); r.x.resize(B * N * HB_NX); r.sw.resize(B * N * HB_NC * HB_SWING_REF);
  c.check(hb_mpc_get_references(c.get(), 0, c.batch(), r.n.data(), r.t.data(), r.mode.data(), r.x.data(), r.sw.data()), "hb_mpc_get_references");
  return r;
}
template <class T>
static bool sameBytes(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 64;
  const Parameters p = loadParametersBlob(argv[1]);
  const int B = 3, N = 72, passes = 40;
  const scalar_t T = p.timeHorizon;
  Context hostCtx(p.model, p.config, B, N), devCtx(p.model, p.config, B, N);
  const GaitSchedule fresh(ModeSchedule{p.initialEventTimes, std::vector<int>(p.initialModes.begin(), p.initialModes.end())},
                           ModeSequenceTemplate{p.defaultTemplate.switchingTimes, std::vector<int>(p.defaultTemplate.modes.begin(), p.defaultTemplate.modes.end())},
                           p.phaseTransitionStanceTime);
  ReferenceManager host(hostCtx, p.refgen, std::vector<GaitSchedule>(size_t(B), fresh));
  host.setWalkGaitSelection(true);
  ReferenceManager dev(devCtx, p.refgen, makeGaitConfig(p, false));
  try {  // the schedules of the second context are the device's
    std::vector<int32_t> n(1, 0), m(HB_MAX_EVENTS + 1, 3);
    vector_t ev(HB_MAX_EVENTS, 0.0);
    devCtx.check(hb_refgen_set_schedule(devCtx.get(), 0, 1, n.data(), ev.data(), m.data()), "hb_refgen_set_schedule");
    std::printf("hb_refgen_set_schedule was accepted next to the device gait manager\n");
    return 3;
  } catch (const Error& e) {
    if (e.status() != HB_ERR_STATE) return 3;
    std::printf("host schedule refused: status %d\n", e.status());
  }
  vector_t obs(size_t(B) * HB_NX, 0.0), time(size_t(B), 0.0), cmd(size_t(B) * 4, 0.0);
  for (int i = 0; i < B; ++i) {
    for (int k = 0; k < HB_NX; ++k) obs[size_t(i) * HB_NX + k] = p.config.initial_state[k];
    obs[size_t(i) * HB_NX + 9] = 0.2 * i;
  }
  for (int k = 0; k < passes; ++k) {
    for (int i = 0; i < B; ++i) time[size_t(i)] = 0.3 + 0.01 * k;
    if (k == 10) cmd[0] = cmd[4] = 0.3;  // instances 0 and 1 are told to walk, instance 2 keeps standing
    host.preSolverRun(time, T, cmd, &obs);
    dev.preSolverRun(time, T, cmd, &obs);
    const Tables a = tables(hostCtx), b = tables(devCtx);
    if (!sameBytes(a.n, b.n) || !sameBytes(a.t, b.t) || !sameBytes(a.mode, b.mode) || !sameBytes(a.x, b.x) || !sameBytes(a.sw, b.sw)) {
      std::printf("node tables differ at pass %d\n", k);
      return 4;
    }
  }
  const std::vector<int32_t> level = devCtx.gaitLevels();
  for (int i = 0; i < B; ++i)
    if (level[size_t(i)] != host.gaitSelector(i).level() || devCtx.gaitStatus()[size_t(i)] != 0) {
      std::printf("gait level of instance %d: device %d, host %d\n", i, level[size_t(i)], host.gaitSelector(i).level());
      return 5;
    }
  if (level[0] != 1 || level[1] != 1 || level[2] != 0) return 6;
  std::printf("ok: %d passes identical, levels %d %d %d\n", passes, level[0], level[1], level[2]);
  return 0;
}
