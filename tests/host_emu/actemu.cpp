// TEST HARNESS: the hybrid forms of the three plant step wrappers (hb_plant.hpp plant_step, hb_contact.hpp contact_step, hb_joints.hpp
// joints_step with the HybridActuator: the routines k_plant_hybrid / k_plant_contact_hybrid / k_plant_joints_hybrid run per instance, the last two as HYBRID forms
// of the shared body hb_kernels.hip plant_ground_step) and
// the per-item routines of the three wire kernels of the simulator end (hb_lcm.hpp), compiled for the host with one emulated lane, for
// tests/test_actuator_plant_host.py.  Not part of the product; the product path always runs the kernels.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../hunter_bipedal_control_amd/csrc/hb_host.hpp"
#include "../../hunter_bipedal_control_amd/csrc/hb_joints.hpp"
#include "../../hunter_bipedal_control_amd/csrc/hb_lcm.hpp"

using namespace hb;
namespace {
struct HostCtx {
  int lane = 0, nlanes = 1;
  void sync() const {}
};
// cmd[5][10]: pos_des vel_des kp kd ff; act[ACT_LDS]: what the kernels keep in LDS behind the form's own arrays
HybridActuator actuator(const double* cmd, double* tau_first, double* tau_mean, double* act) {
  return HybridActuator{cmd, cmd + 10, cmd + 20, cmd + 30, cmd + 40, tau_first, tau_mean, act, act + HB_NJ};
}
}  // namespace

extern "C" {
// One hybrid tick of one instance of the pinned stub.  q[16], v[16], anchor[12], pinned[4] in / out; contact[4]; tau_last[10] = what
// hb_plant_sense would report as the joint torque (the last substep's).
void ae_stub_step(const hb_model* m, double* q, double* v, double* anchor, int* pinned, const double* cmd, const int* contact, double baum,
                  double eps, double dt, int substeps, double* lambda, double* vdot, double* tau_first, double* tau_mean, double* tau_last) {
  const DevModel d = make_dev_model(*m);
  std::vector<double> lds(PLANT_LDS_TOTAL + ACT_LDS, 0.0);
  const HybridActuator act = actuator(cmd, tau_first, tau_mean, lds.data() + PLANT_LDS_TOTAL);
  plant_step<true>(HostCtx{}, d, q, v, anchor, pinned, nullptr, contact, baum, eps, dt, substeps, lds.data(), lambda, vdot, &act);
  for (int j = 0; j < HB_NJ; ++j) tau_last[j] = act.tau[j];
}
// the held-torque tick of the pinned stub (what k_plant runs per instance)
void ae_stub_step_held(const hb_model* m, double* q, double* v, double* anchor, int* pinned, const double* tau, const int* contact, double baum,
                       double eps, double dt, int substeps, double* lambda, double* vdot) {
  const DevModel d = make_dev_model(*m);
  std::vector<double> lds(PLANT_LDS_TOTAL, 0.0);
  plant_step(HostCtx{}, d, q, v, anchor, pinned, tau, contact, baum, eps, dt, substeps, lds.data(), lambda, vdot);
}
// One hybrid tick of one instance in contact model 1: the arguments of ce_step (contactemu.cpp) with the command in the torque's place.
void ae_contact_step(const hb_model* m, const hb_contact_config* K, double* q, double* v, double* imp, const double* cmd, const double* wrench,
                     double eps, double dt, int substeps, double* lambda, double* vdot, double* gap, double* pvel, double* res, int* touching,
                     int* status, double* tau_first, double* tau_mean, double* tau_last) {
  const DevModel d = make_dev_model(*m);
  const int all_on[4] = {1, 1, 1, 1};
  std::vector<double> lds(CONTACT_LDS_TOTAL + ACT_LDS, 0.0);
  const ContactOut out{gap, pvel, res, touching, status};
  const HybridActuator act = actuator(cmd, tau_first, tau_mean, lds.data() + CONTACT_LDS_TOTAL);
  contact_step<true>(HostCtx{}, d, q, v, imp, nullptr, wrench, all_on, *K, eps, dt, substeps, lds.data(), lambda, vdot, out, &act);
  for (int j = 0; j < HB_NJ; ++j) tau_last[j] = act.tau[j];
}
// One hybrid tick of one instance in contact model 1 with the joint model: the arguments of je_step (jointemu.cpp) likewise.
void ae_joints_step(const hb_model* m, const hb_contact_config* K, const hb_joint_model* J, double* q, double* v, double* imp, double* jimp,
                    const double* cmd, const double* wrench, double eps, double dt, int substeps, double* lambda, double* vdot, double* gap,
                    double* pvel, double* res, int* touching, int* status, double* tau_applied, double* friction_torque, double* limit_torque,
                    double* jres, int* jstatus, double* tau_last, double* tau_first, double* tau_mean) {
  const DevModel d = make_dev_model(*m);
  const int all_on[4] = {1, 1, 1, 1};
  std::vector<double> lds(JOINT_LDS_TOTAL + ACT_LDS, 0.0);
  const ContactOut out{gap, pvel, res, touching, status};
  const JointOut jout{tau_applied, friction_torque, limit_torque, jres, jstatus};
  const HybridActuator act = actuator(cmd, tau_first, tau_mean, lds.data() + JOINT_LDS_TOTAL);
  joints_step<true>(HostCtx{}, d, q, v, imp, jimp, nullptr, wrench, all_on, *K, *J, eps, dt, substeps, lds.data(), lambda, vdot, tau_last, out, jout,
                    &act);
}

// ---- the wire kernels' routines: k_lcm_unpack_cmd, k_lcm_pack_state, k_lcm_pack_full for one instance --------------------------------
int ae_unpack_cmd(const uint8_t* low_cmd /*[496]*/, double* cmd /*[5][10] in / out*/, uint64_t* last_ts) {
  uint64_t in[62];
  __builtin_memcpy(in, low_cmd, sizeof in);
  return lcm_accept_cmd(in, cmd, cmd + 10, cmd + 20, cmd + 30, cmd + 40, last_ts);
}
void ae_pack_low_state(int64_t timestamp, const double* quat, const double* gyro, const double* accel, const double* jp, const double* jv,
                       const double* jt, uint8_t* out /*[336]*/) {
  uint64_t w[42];
  for (int k = 0; k < 42; ++k) w[k] = __builtin_bswap64(lcm_low_state_word(k, lcm_fingerprint(HB_LCM_LOW_STATE), timestamp, quat, gyro, accel, jp, jv, jt));
  __builtin_memcpy(out, w, sizeof w);
}
void ae_pack_full_state(const hb_model* m, int64_t timestamp, const double* q, const double* v, const double* tau, uint8_t* out /*[464]*/) {
  uint64_t w[58];
  lcm_full_state(m->gravity, q, v, tau, lcm_fingerprint(HB_LCM_FULL_STATE), timestamp, w);
  __builtin_memcpy(out, w, sizeof w);
}
}
