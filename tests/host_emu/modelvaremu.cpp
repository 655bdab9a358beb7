// TEST HARNESS: the composition of an instance's varied model (csrc/hb_modelvar.hpp: the routine hb_plant_set_model_variation builds the
// uploaded image with) compiled for the host, for tests/test_modelvar_host.py.  Not part of the product.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../hunter_bipedal_control_amd/csrc/hb_host.hpp"
#include "../../hunter_bipedal_control_amd/csrc/hb_modelvar.hpp"

using namespace hb;

extern "C" {
int mv_payload_size() { return MODELVAR_PAYLOAD; }
int mv_record_bytes() { return int(sizeof(DevModel)); }
// scale[B][HB_NBODY] or null, payload[B][HB_PAYLOAD_SIZE] or null (the arguments of hb_plant_set_model_variation).  Returns 0 and per
// instance out[i] = *m with mass, com and inertia of the composed model, total_mass[i] its total_mass, rec (or null) the B composed DevModel
// records; nominal (or null) the nominal record; or 1, the first offending instance in *bad and the reason of the refusal in why[n].
int mv_compose(const hb_model* m, int B, const double* scale, const double* payload, hb_model* out, double* total_mass, void* rec, void* nominal,
               int* bad, char* why, int n) {
  const DevModel nom = make_dev_model(*m);
  if (nominal) std::memcpy(nominal, &nom, sizeof nom);
  std::vector<DevModel> img(static_cast<size_t>(B));
  if (const char* w = modelvar_compose_batch(nom, B, scale, payload, img.data(), bad)) {
    std::strncpy(why, w, size_t(n) - 1);
    why[n - 1] = 0;
    return 1;
  }
  for (int i = 0; i < B; ++i) {
    const DevModel& d = img[i];
    out[i] = *m;
    for (int b = 0; b < HB_NBODY; ++b) {
      out[i].mass[b] = d.mass[b];
      for (int a = 0; a < 3; ++a) out[i].com[b][a] = d.com[b][a];
      for (int k = 0; k < 6; ++k) out[i].inertia[b][k] = d.inertia[b][k];
    }
    total_mass[i] = d.total_mass;
  }
  if (rec) std::memcpy(rec, img.data(), sizeof(DevModel) * size_t(B));
  return 0;
}
}
