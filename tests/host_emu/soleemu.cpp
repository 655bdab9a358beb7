// TEST HARNESS: the sole mode of the planner (hb_refgen.hpp refgen_plan<MAP, 1>, hb_ground_set_foothold) on both kinds of map, compiled
// for the host with one emulated lane (foot_step == 1: the one-thread form, the same code the four lanes of an instance run), for
// tests/test_sole_host.py.  gnd / gz = the instance's stored map as groundemu.cpp / groundfieldemu.cpp take it (gz null: a profile map);
// cfg null or mode 0: the per-point forms, what runs without the call.  Also the form rule of hb_forms.hpp and the argument checks the
// setter applies.  Not part of the product; the product path always runs the kernels.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "../../hunter_bipedal_control_amd/csrc/hb_host.hpp"
#include "../../hunter_bipedal_control_amd/csrc/hb_refgen.hpp"
#include "../../hunter_bipedal_control_amd/csrc/hb_forms.hpp"

using namespace hb;

extern "C" {
int se_no_foothold() { return RG_NO_FOOTHOLD; }
int se_max_shift() { return HB_FOOTHOLD_MAX_SHIFT; }
// use_sole_forms(use_ground_forms(profile, field), mode); mode < 0: the defaulted call
int se_sole_form(int profile_on, int field_on, int mode) {
  const GroundForm gf = use_ground_forms(profile_on != 0, field_on != 0);
  return mode < 0 ? int(use_sole_forms(gf)) : int(use_sole_forms(gf, mode));
}
// the setter's argument check of a configuration with mode != 0: 0 accepted, 1 refused
int se_refused(const hb_foothold_config* cfg) { return foothold_refusal(*cfg) ? 1 : 0; }
// S(cT, cH) of one pair of points -> delta, top
void se_sample(const double* gnd, const double* gz, const double* t_xy, const double* h_xy, double* out2) {
  const RgSoleSample s = gz ? rg_sole_sample<MAP_FIELD>(gnd, gz, t_xy[0], t_xy[1], h_xy[0], h_xy[1])
                            : rg_sole_sample<MAP_PROFILE>(gnd, nullptr, t_xy[0], t_xy[1], h_xy[0], h_xy[1]);
  out2[0] = s.delta;
  out2[1] = s.top;
}
// One reference-generation pass of one instance with every intermediate it leaves on the device (as ge_refgen of groundemu.cpp), and the
// choice read-back shift[2], defect[2], level[2] (left as given when the pass does not run in sole mode).
int se_refgen(const hb_model* m, const hb::RefgenConfig* k, const double* gnd, const double* gz, const hb_foothold_config* cfg, int n_ev,
              const double* ev, const int* modes, double t0, double horizon, const double* x_now, const double* cmd_vel, double* latest_stance,
              int max_nodes, int* n_nodes, double* t, int* mode, double* xref, double* swing, double* phases, int* n_knots, double* knot_t,
              double* knot_x, int* shift, double* defect, int* level) {
  const DevModel d = make_dev_model(*m);
  int nk = 0, status;
  const bool sole = cfg && cfg->mode == 1;
  const RgSole rs{cfg, shift, defect, level};
#define SE_ARGS d, *k, n_ev, ev, modes, t0, horizon, x_now, cmd_vel, latest_stance, phases, max_nodes, n_nodes, t, &nk, knot_t, knot_x, 0, 1, gnd, gz
  if (gz) status = sole ? refgen_plan<MAP_FIELD, 1>(SE_ARGS, rs) : refgen_plan<MAP_FIELD>(SE_ARGS);
  else status = sole ? refgen_plan<MAP_PROFILE, 1>(SE_ARGS, rs) : refgen_plan<MAP_PROFILE>(SE_ARGS);
#undef SE_ARGS
  RgIkWork work;
  for (int leg = 0; leg < 2; ++leg) refgen_ik_leg(d, *k, n_ev, ev, t0, horizon, x_now, phases, nk, knot_t, knot_x, leg, work);
  for (int n = 0; n < max_nodes; ++n)
    refgen_node(*k, n_ev, ev, modes, nk, knot_t, knot_x, phases, n, *n_nodes, t[n], mode + n, xref + size_t(n) * HB_NX,
                swing + size_t(n) * HB_NC * HB_SWING_REF);
  *n_knots = nk;
  return status;
}
}
