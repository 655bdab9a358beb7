// TEST HARNESS: the layout descriptions of csrc/hb_layout.hpp compiled for the host, for tests/test_layout_host.py.  Every pointer of
// every batch struct gets a fake base address (the struct's bytes are filled with one pattern, so a member the description forgets
// has one too); the program prints, per struct, what the instance-range view (i0, cnt) moved each member by — members named HERE, one
// by one, not through the description — and what the allocation of the description would request for B instances.
//   layoutemu B Nmax i0 cnt
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../hunter_bipedal_control_amd/csrc/hb_layout.hpp"

namespace {
template <class S>
S patterned() {
  S s;
  std::memset(&s, 0x10, sizeof(S));
  return s;
}
template <class T>
long moved(T* after, T* before) {
  return long((reinterpret_cast<uintptr_t>(after) - reinterpret_cast<uintptr_t>(before)) / sizeof(T));
}
template <class S>
void allocation(const char* name, S s, size_t B, size_t N) {
  size_t bytes = 0;
  fields(s, N, [&](const char* member, auto*& p, Extent e) {
    std::printf("alloc %s.%s %zu %zu\n", name, std::strchr(member, '.') + 1, B * e.n, sizeof(*p));
    bytes += B * e.n * sizeof(*p);
  });
  std::printf("bytes %s %zu\n", name, bytes);
}
}  // namespace

#define MOVED(m) std::printf("view %s.%s %ld\n", sn, #m, moved(v.m, s.m))

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const size_t B = std::atoi(argv[1]), N = std::atoi(argv[2]);
  const int i0 = std::atoi(argv[3]), cnt = std::atoi(argv[4]);
  {
    const char* sn = "Batch";
    const Batch s = patterned<Batch>(), v = view(s, N, i0, cnt);
    std::printf("scalars Batch %d %d\n", v.B, v.Nmax == s.Nmax);
    MOVED(n_nodes); MOVED(t); MOVED(mode); MOVED(xref); MOVED(swing); MOVED(x); MOVED(u); MOVED(x0); MOVED(recs); MOVED(gains); MOVED(dx); MOVED(du);
    MOVED(acc); MOVED(partial); MOVED(ls_norm); MOVED(ls_tail); MOVED(accepted); MOVED(perf); MOVED(ric_fail); MOVED(mpc_status); MOVED(xp); MOVED(up);
    MOVED(tp); MOVED(modep); MOVED(np_nodes); MOVED(grid_dirty); MOVED(lqpark);
    allocation(sn, s, B, N);
  }
  {
    const char* sn = "WbcBatch";
    const WbcBatch s = patterned<WbcBatch>(), v = view(s, N, i0, cnt);
    std::printf("scalars WbcBatch %d %d\n", v.B, std::memcmp(&v.policy_valid, &s.policy_valid, sizeof(bool)) == 0);
    MOVED(t_now); MOVED(rbd); MOVED(walk); MOVED(xdes); MOVED(udes); MOVED(mode); MOVED(stance); MOVED(sol); MOVED(status); MOVED(iters); MOVED(px);
    MOVED(pu); MOVED(pt); MOVED(pmode); MOVED(pn);
    allocation(sn, s, B, N);
  }
  {
    const char* sn = "EstBatch";
    const EstBatch s = patterned<EstBatch>(), v = view(s, N, i0, cnt);
    std::printf("scalars EstBatch %d 1\n", v.B);
    MOVED(xhat); MOVED(P); MOVED(yaw_last); MOVED(quat); MOVED(w_local); MOVED(a_local); MOVED(qj); MOVED(qdj); MOVED(contact); MOVED(rbd); MOVED(x);
    MOVED(res_rbd); MOVED(res_x0); MOVED(cf_z); MOVED(cf_tau); MOVED(cf_dist); MOVED(cf_out); MOVED(cf_rbd);
    allocation(sn, s, B, N);
  }
  {
    const char* sn = "RefgenBatch";
    const RefgenBatch s = patterned<RefgenBatch>(), v = view(s, N, i0, cnt);
    std::printf("scalars RefgenBatch %d %d\n", v.B, v.init_stance == s.init_stance);
    MOVED(n_ev); MOVED(ev); MOVED(modes); MOVED(stance); MOVED(phases); MOVED(t0); MOVED(cmd); MOVED(status); MOVED(n_knots); MOVED(knot_t); MOVED(knot_x);
    allocation(sn, s, B, N);
  }
  {
    const char* sn = "GaitBatch";
    const GaitBatch s = patterned<GaitBatch>(), v = view(s, N, i0, cnt);
    std::printf("scalars GaitBatch %d %d\n", v.B, v.stride == s.stride);
    MOVED(n_ev); MOVED(ev); MOVED(modes); MOVED(tpl_n); MOVED(tpl_sw); MOVED(tpl_modes); MOVED(last_vel); MOVED(cmd); MOVED(hist); MOVED(hist_n);
    MOVED(hist_head); MOVED(level); MOVED(vel_abs); MOVED(vel_avg); MOVED(status);
    allocation(sn, s, B, N);
  }
  {
    const char* sn = "MpcCertBuf";
    const MpcCertBuf s = patterned<MpcCertBuf>(), v = from_instance(s, N, i0);
    MOVED(node); MOVED(costate); MOVED(cert); MOVED(util);
    allocation(sn, s, B, N);
  }
  {
    const char* sn = "WbcCertBuf";
    const WbcCertBuf s = patterned<WbcCertBuf>(), v = from_instance(s, N, i0);
    MOVED(cert); MOVED(dual);
    allocation(sn, s, B, N);
  }
  {
    const char* sn = "HwbcCertBuf";
    const HwbcCertBuf s = patterned<HwbcCertBuf>(), v = from_instance(s, N, i0);
    MOVED(cert); MOVED(xlev); MOVED(slack); MOVED(dual);
    allocation(sn, s, B, N);
  }
  allocation("PlantBatch", patterned<PlantBatch>(), B, N);   // (never viewed: the plant runs on the whole batch)
  return 0;
}
