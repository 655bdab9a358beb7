// TEST HARNESS: csrc/hb_forms.hpp compiled for the host, for tests/test_forms_host.py.
//   formsemu table    prints the table: "code NAME value" per single code, "range NAME first last" per family
//   formsemu check    compares decode_forms + use_ric_bwd4 / use_ric_fwd_wave / lq_trip_len with the expressions the launchers held
//                     before the header existed (copied verbatim below: `sel` is hb_config.reserved, HB_ABLATE_ON the build), for
//                     both builds, over reserved in -1 .. 260 and a grid of (concurrent, Nmax, n_cu); prints "checked N" and
//                     "mismatch ..." lines, exit status 1 if any.
//   formsemu plant    compares plant_form, mapped to a kernel name the way plant_launch's switch does, with the two ladders of
//                     hb_api_est.hpp (since then hb_api_plant.hpp) it replaces (their conditions copied verbatim below), over contact mode 0 / 1, the sixteen
//                     combinations of joints / terrain / variation / profile and held / hybrid; same output as check.
#include <cstdio>
#include <cstring>
#include <string>
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

// The plant: the conditions of the two ladders hb_plant_step and plant_launch_hybrid held (then in hb_api_est.hpp), rung by rung in their order;
// a rung returns the name of the kernel it launched.  `ctx` carries the five words of the context the rungs read.
struct Ctx { struct { int mode; } contact_cfg; bool joints_on, terrain_on, modelvar_on, profile_on; };
const char* plant_step(const Ctx* ctx) {
  if (ctx->contact_cfg.mode == 1 && ctx->profile_on && ctx->joints_on) return "k_plant_profile_joints";
  if (ctx->contact_cfg.mode == 1 && ctx->profile_on) return "k_plant_profile";
  if (ctx->contact_cfg.mode == 1 && ctx->modelvar_on && ctx->joints_on) return "k_plant_varied_joints";
  if (ctx->contact_cfg.mode == 1 && ctx->modelvar_on) return "k_plant_varied";
  if (ctx->contact_cfg.mode == 1 && ctx->terrain_on && ctx->joints_on) return "k_plant_terrain_joints";
  if (ctx->contact_cfg.mode == 1 && ctx->terrain_on) return "k_plant_terrain";
  if (ctx->contact_cfg.mode == 1 && ctx->joints_on) return "k_plant_joints";
  if (ctx->contact_cfg.mode == 1) return "k_plant_contact";
  return "k_plant";
}
const char* plant_launch_hybrid(const Ctx* ctx) {
  if (ctx->contact_cfg.mode == 1 && ctx->profile_on && ctx->joints_on) return "k_plant_profile_joints_hybrid";
  if (ctx->contact_cfg.mode == 1 && ctx->profile_on) return "k_plant_profile_hybrid";
  if (ctx->contact_cfg.mode == 1 && ctx->modelvar_on && ctx->joints_on) return "k_plant_varied_joints_hybrid";
  if (ctx->contact_cfg.mode == 1 && ctx->modelvar_on) return "k_plant_varied_hybrid";
  if (ctx->contact_cfg.mode == 1 && ctx->terrain_on && ctx->joints_on) return "k_plant_terrain_joints_hybrid";
  if (ctx->contact_cfg.mode == 1 && ctx->terrain_on) return "k_plant_terrain_hybrid";
  if (ctx->contact_cfg.mode == 1 && ctx->joints_on) return "k_plant_joints_hybrid";
  if (ctx->contact_cfg.mode == 1) return "k_plant_contact_hybrid";
  return "k_plant_hybrid";
}
}  // namespace before

// The kernel plant_launch (hb_api_plant.hpp) launches for a form: its switch, by name.
static std::string plant_kernel(const hb::PlantForm& f) {
  using G = hb::PlantForm::Ground;
  const char* tail = f.hybrid ? "_hybrid" : "";
  if (f.ground == G::Pinned) return std::string("k_plant") + tail;
  if (f.ground == G::Level) return std::string(f.joints ? "k_plant_joints" : "k_plant_contact") + tail;
  const char* family = f.ground == G::Terrain ? "k_plant_terrain" : f.ground == G::Varied ? "k_plant_varied" : "k_plant_profile";
  return std::string(family) + (f.joints ? "_joints" : "") + tail;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "table")) {
    for (const hb::form::Entry& e : hb::form::kTable) {
      if (e.first == e.last) std::printf("code %s %d\n", e.name, e.first);
      else std::printf("range %s %d %d\n", e.name, e.first, e.last);
    }
    return 0;
  }
  if (argc == 2 && !std::strcmp(argv[1], "plant")) {
    long checked = 0, bad = 0;
    for (int mode = 0; mode <= 1; ++mode)
      for (int flags = 0; flags < 16; ++flags)
        for (int hybrid = 0; hybrid <= 1; ++hybrid) {
          const before::Ctx c{{mode}, (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0};
          const std::string was = hybrid ? before::plant_launch_hybrid(&c) : before::plant_step(&c);
          const std::string is = plant_kernel(hb::plant_form(mode, c.joints_on, c.terrain_on, c.modelvar_on, c.profile_on, hybrid != 0));
          ++checked;
          if (was != is && ++bad) std::printf("mismatch mode %d joints %d terrain %d modelvar %d profile %d hybrid %d: %s, was %s\n", mode, c.joints_on,
                                              c.terrain_on, c.modelvar_on, c.profile_on, hybrid, is.c_str(), was.c_str());
        }
    std::printf("checked %ld\n", checked);
    return bad ? 1 : 0;
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
