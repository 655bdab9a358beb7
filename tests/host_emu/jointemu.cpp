// TEST HARNESS: the joint model of the ground-contact plant (hb_joints.hpp: the routine the JOINTS forms of the shared kernel body run per
// instance, hb_kernels.hip plant_ground_step; k_plant_joints is the form on level ground) compiled for the
// host with one emulated lane, for tests/test_joint_plant_host.py.  Not part of the product; the product path always runs the kernel.
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../hunter_bipedal_control_amd/csrc/hb_host.hpp"
#include "../../hunter_bipedal_control_amd/csrc/hb_joints.hpp"

using namespace hb;
namespace {
struct HostCtx {
  int lane = 0, nlanes = 1;
  void sync() const {}
};
}  // namespace

extern "C" {
int je_model_valid(const hb_joint_model* J) { return joint_model_valid(*J) ? 1 : 0; }
int je_sizeof_joint_model() { return int(sizeof(hb_joint_model)); }
// One plant tick of one instance in contact model 1 with the joint model.  q[16], v[16], imp[12], jimp[20] (friction impulses, signed stop
// impulses), status in / out; wrench[6] or null; out as hb_plant_get_state (lambda[12], vdot[16]), hb_plant_get_contact (gap[4], pvel[12],
// res, touching[4], status) and hb_plant_get_joints (tau_applied, friction_torque, limit_torque [10], jres, jstatus); tau_last[10] = what
// hb_plant_sense would report as the joint torque.
void je_step(const hb_model* m, const hb_contact_config* K, const hb_joint_model* J, double* q, double* v, double* imp, double* jimp,
             const double* tau, const double* wrench, double eps, double dt, int substeps, double* lambda, double* vdot, double* gap, double* pvel,
             double* res, int* touching, int* status, double* tau_applied, double* friction_torque, double* limit_torque, double* jres, int* jstatus,
             double* tau_last) {
  const DevModel d = make_dev_model(*m);
  const int all_on[4] = {1, 1, 1, 1};
  std::vector<double> lds(JOINT_LDS_TOTAL, 0.0);
  const ContactOut out{gap, pvel, res, touching, status};
  const JointOut jout{tau_applied, friction_torque, limit_torque, jres, jstatus};
  joints_step(HostCtx{}, d, q, v, imp, jimp, tau, wrench, all_on, *K, *J, eps, dt, substeps, lds.data(), lambda, vdot, tau_last, out, jout);
}
}
