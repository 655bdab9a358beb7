// The device-resident arrays of a batch: the structs the kernels take by value and, per struct, ONE description of its arrays —
// fields(s, N, f) calls f(name, member, extent) for every device array in allocation order.  Allocation, instance-range views and
// host <-> device copies of instance ranges are derived from the description (below and hb_api_ctx.hpp); nothing else restates how
// many elements an instance owns.  Host code only, and plain C++: tests/host_emu/layoutemu.cpp compiles this header with g++.
#pragma once
#include <cstddef>

#include "hb_host.hpp"
#include "hb_mpccert.hpp"
#include "hb_wbc.hpp"
#include "hb_refgen.hpp"
#include "hb_gait.hpp"
#include "hb_contact.hpp"
#include "hb_episode.hpp"
#include "hb_modelvar.hpp"
#include "hb_ground.hpp"
#include "hb_profiledraw.hpp"
#include "hb_fielddraw.hpp"
#include "hb_scan.hpp"

namespace {
using namespace hb;

// Elements of an array that belong to one instance (n: the allocation is B * n) and the distance from one instance's data to the next
// (step: the view of the instances from i0 on starts i0 * step further).  Instance-major arrays [B][n]: step = n.
struct Extent {
  size_t n, step;
  constexpr Extent(size_t n_) : n(n_), step(n_) {}
  constexpr Extent(size_t n_, size_t step_) : n(n_), step(step_) {}
};
// [slots][B]: the pitch of a slot row is the whole batch in every view (GaitBatch::stride), consecutive instances are neighbours
constexpr Extent slot_major(size_t slots) { return Extent(slots, 1); }

#define HB_FIELD(member, ...) f(#member, member, Extent(__VA_ARGS__))

// ---------------------------------------------------------------------------------------------------------
// device-resident problem data of a batch
constexpr int LS_TAIL_MAX = HB_LS_TAIL_MAX;   // 16: step sizes the backtracking tail evaluates side by side (decay 0.5, alpha_min 1e-4: 13 of them)
struct Batch {
  int B, Nmax;
  int* n_nodes;
  double* t;
  int* mode;
  double* xref;
  double* swing;
  double* x;
  double* u;
  double* x0;
  double* recs;
  double* gains;
  double* dx;
  double* du;
  double* acc;      // armijo, base merit, base dyn, base eq
  double* partial;
  double* ls_norm;  // |dx|, |du| (l2, whole trajectory) of the instances whose full step was refused (k_ls_decide)
  double* ls_tail;  // [LS_TAIL_MAX][Nmax][3] per instance: per-node line-search partials of the backtracking step sizes, evaluated side by side
  int* accepted;
  double* perf;     // merit dyn eq step
  int* ric_fail;
  int* mpc_status;  // hb_inst_status of the last MPC call
  // iterate of the previous MPC call on ITS time grid (warm start across calls, k_warm_shift); x / u and xp / up swap roles
  double* xp;
  double* up;
  double* tp;
  int* modep;
  int* np_nodes;
  int* grid_dirty;  // the node tables changed since the iterate was last brought onto them
  double* lqpark;   // phase-1 images of the nodes, parked by the value phase of k_lq_trip
};
template <class F>
constexpr void fields(Batch& b, size_t N, F&& f) {
  HB_FIELD(b.n_nodes, 1); HB_FIELD(b.t, N + 1); HB_FIELD(b.mode, N); HB_FIELD(b.xref, N * HB_NX); HB_FIELD(b.swing, N * 24);
  HB_FIELD(b.x, (N + 1) * HB_NX); HB_FIELD(b.u, N * HB_NU); HB_FIELD(b.x0, HB_NX); HB_FIELD(b.recs, N * REC_SIZE); HB_FIELD(b.gains, N * GAIN_SIZE);
  HB_FIELD(b.dx, (N + 1) * HB_NX); HB_FIELD(b.du, N * HB_NU); HB_FIELD(b.acc, 4); HB_FIELD(b.partial, N * 3);
  HB_FIELD(b.ls_tail, LS_TAIL_MAX * N * 3); HB_FIELD(b.ls_norm, 2); HB_FIELD(b.accepted, 1); HB_FIELD(b.perf, 4); HB_FIELD(b.ric_fail, 1);
  HB_FIELD(b.mpc_status, 1); HB_FIELD(b.xp, (N + 1) * HB_NX); HB_FIELD(b.up, N * HB_NU); HB_FIELD(b.tp, N + 1); HB_FIELD(b.modep, N);
  HB_FIELD(b.np_nodes, 1); HB_FIELD(b.grid_dirty, 1); HB_FIELD(b.lqpark, (N + LqPark::trip_max) * LqPark::size);
}

// The instances whose full step the line search refused, for the backtracking tail (k_ls_decide appends, k_ls_tail_eval walks): a counter
// and the instance ids, numbered within the view.  One slot of each per instance, so that the view of an instance range starts at slots
// of its own: the range's counter is the first of them, its list can hold the whole range.  The order of the list is not deterministic.
struct LsList {
  int* count;
  int* inst;
};
template <class F>
constexpr void fields(LsList& l, size_t, F&& f) {
  HB_FIELD(l.count, 1); HB_FIELD(l.inst, 1);
}

// KKT certificate of the MPC's stage QP (hb_mpccert.hpp), on demand: work buffers of hb_mpc_get_certificate
struct MpcCertBuf {
  double* node;
  double* costate;
  double* cert;
  double* util;     // u~ as hb_mpc_get_certificate returns it
};
template <class F>
constexpr void fields(MpcCertBuf& m, size_t N, F&& f) {
  HB_FIELD(m.node, N * CertNode::size); HB_FIELD(m.costate, (N + 1) * HB_NX); HB_FIELD(m.cert, MPC_CERT_SIZE); HB_FIELD(m.util, N * 12);
}

// WbcBatch (hb_wbc.hpp): inputs and outputs of the WBC, and the published policy (PrimalSolution) its stream reads
template <class F>
constexpr void fields(WbcBatch& w, size_t N, F&& f) {
  HB_FIELD(w.t_now, 1); HB_FIELD(w.rbd, HB_NRBD); HB_FIELD(w.walk, 1); HB_FIELD(w.xdes, HB_NX); HB_FIELD(w.udes, HB_NU); HB_FIELD(w.mode, 1);
  HB_FIELD(w.stance, 1); HB_FIELD(w.sol, HB_NWBC); HB_FIELD(w.status, 1); HB_FIELD(w.iters, 1); HB_FIELD(w.px, (N + 1) * HB_NX);
  HB_FIELD(w.pu, N * HB_NU); HB_FIELD(w.pt, N + 1); HB_FIELD(w.pmode, N); HB_FIELD(w.pn, 1);
}

// KKT certificate of the WeightedWbc QP (hb_wbc_set_certificate) and per-level certificate of the HierarchicalWbc cascade
// (hb_hwbc_set_certificate): outputs of k_wbc_cert / k_hwbc_cert, allocated on the first enable
struct WbcCertBuf {
  double *cert, *dual;
};
template <class F>
constexpr void fields(WbcCertBuf& c, size_t, F&& f) {
  HB_FIELD(c.cert, HB_WBC_CERT_SIZE); HB_FIELD(c.dual, HB_WBC_NCONS_MAX);
}
struct HwbcCertBuf {
  double *cert, *xlev, *slack, *dual;   // per level | the solution after each level | the level-0 slack | multipliers of the inequality rows per level
};
template <class F>
constexpr void fields(HwbcCertBuf& c, size_t, F&& f) {
  HB_FIELD(c.cert, HB_HWBC_LEVELS * HB_HWBC_CERT_SIZE); HB_FIELD(c.xlev, HB_HWBC_LEVELS * HB_NWBC); HB_FIELD(c.slack, HB_HWBC_NINEQ_MAX);
  HB_FIELD(c.dual, HB_HWBC_LEVELS * HB_HWBC_NINEQ_MAX);
}

// ---- plant stub ------------------------------------------------------------------------------------------------------
struct PlantBatch {
  int B;
  double *q, *v, *anchor;
  int* pinned;
  double *lambda, *vdot;
  double* tau;             // staging of host torques
  int* contact;            // staging of host contact flags
  double* rbd;             // repacked state
  double baum, eps;
  // what the last step applied (hb_plant_sense reads them; zero torque / all flags 1 before the first step)
  double* tau_last;
  int* contact_last;
  // sensor arrays of hb_plant_sense: quat, gyro, accel, joint pos / vel / torque, contact flags
  double *s_quat, *s_gyro, *s_accel, *s_jp, *s_jv, *s_jt;
  int* s_contact;
  double *gyro_bias, *accel_bias;  // [B][3] each, or null: not described, hb_plant_set_sensor_model aims them at buffers of its own
};
template <class F>
constexpr void fields(PlantBatch& p, size_t, F&& f) {
  HB_FIELD(p.q, 16); HB_FIELD(p.v, 16); HB_FIELD(p.anchor, 12); HB_FIELD(p.pinned, 4); HB_FIELD(p.lambda, 12); HB_FIELD(p.vdot, 16);
  HB_FIELD(p.tau, 10); HB_FIELD(p.contact, 4); HB_FIELD(p.rbd, HB_NRBD); HB_FIELD(p.tau_last, 10); HB_FIELD(p.contact_last, 4); HB_FIELD(p.s_quat, 4);
  HB_FIELD(p.s_gyro, 3); HB_FIELD(p.s_accel, 3); HB_FIELD(p.s_jp, 10); HB_FIELD(p.s_jv, 10); HB_FIELD(p.s_jt, 10); HB_FIELD(p.s_contact, 4);
}

// ground-contact model of the plant (hb_contact.hpp), allocated by the first hb_plant_set_contact_model that selects it: impulses of
// the last substep (the warm start), the outputs of hb_plant_get_contact, the external base wrench
struct ContactBatch {
  int B;
  int use_wrench;   // hb_plant_set_external_wrench has given one
  double *imp, *gap, *pvel, *res;
  int *touching, *status;
  double* wrench;
};
template <class F>
constexpr void fields(ContactBatch& c, size_t, F&& f) {
  HB_FIELD(c.imp, 12); HB_FIELD(c.gap, 4); HB_FIELD(c.pvel, 12); HB_FIELD(c.res, 1); HB_FIELD(c.touching, 4); HB_FIELD(c.status, 1); HB_FIELD(c.wrench, 6);
}

// joint model of the ground-contact plant (hb_joints.hpp), allocated by the first hb_plant_set_joint_model that gives one: friction
// impulses and signed stop impulses of the last substep (the warm start) and the outputs of hb_plant_get_joints
struct JointBatch {
  int B;
  double *imp, *tau_applied, *friction_torque, *limit_torque, *res;
  int* status;
};
template <class F>
constexpr void fields(JointBatch& j, size_t, F&& f) {
  HB_FIELD(j.imp, 20); HB_FIELD(j.tau_applied, 10); HB_FIELD(j.friction_torque, 10); HB_FIELD(j.limit_torque, 10); HB_FIELD(j.res, 1);
  HB_FIELD(j.status, 1);
}

// per-instance terrain of the ground-contact plant (hb_plant_set_terrain), allocated by the first call that gives one: the record the
// terrain kernels stage per instance (hb_contact.hpp Terrain: frame T row-major | d | mu of the four points)
struct TerrainBatch {
  int B;
  double* ter;
};
template <class F>
constexpr void fields(TerrainBatch& t, size_t, F&& f) {
  HB_FIELD(t.ter, Terrain::size);
}

// per-instance terrain profile of the ground-contact plant (hb_plant_set_terrain_profile), allocated by the first call that gives one:
// prof: the stored part of the record the profile kernels stage per instance (hb_contact.hpp Profile: mu of the four points in a Terrain
// head | direction | number of segments | breakpoints | (T_j, d_j) per segment); seg: the segment under the four contact points and the
// base origin at the end of the last step; base: the Terrain record of the facet under the base origin there (what k_plant_episode takes
// in place of the terrain records)
struct ProfileBatch {
  int B;
  double* prof;
  int* seg;
  double* base;
};
template <class F>
constexpr void fields(ProfileBatch& t, size_t, F&& f) {
  HB_FIELD(t.prof, Profile::stored); HB_FIELD(t.seg, HB_NC + 1); HB_FIELD(t.base, Terrain::size);
}

// per-instance height field of the ground-contact plant (hb_plant_set_terrain_field), allocated by the first call that gives one: hdr: the
// stored part of the record the field kernels stage per instance (hb_contact.hpp Field: mu of the four points in a Terrain head |
// direction | origin | spacing | node counts); z: the heights, [HB_FIELD_MAX_NODES][HB_FIELD_MAX_NODES] per instance, read from global
// memory by the step; sel: the facet id under the four contact points and the base origin at the end of the last step; base: the Terrain
// record of the facet under the base origin there (what k_plant_episode takes in place of the terrain records)
struct FieldBatch {
  int B;
  double* hdr;
  double* z;
  int* sel;
  double* base;
};
template <class F>
constexpr void fields(FieldBatch& t, size_t, F&& f) {
  HB_FIELD(t.hdr, Field::stored); HB_FIELD(t.z, Field::nz); HB_FIELD(t.sel, HB_NC + 1); HB_FIELD(t.base, Terrain::size);
}

// per-instance model variation of the ground-contact plant (hb_plant_set_model_variation, hb_modelvar.hpp), allocated by the first call
// that gives one: the DevModel record each instance steps on, [B] records of sizeof(DevModel) (about 1.7 KB)
struct ModelVarBatch {
  int B;
  DevModel* mdl;
};
template <class F>
constexpr void fields(ModelVarBatch& m, size_t, F&& f) {
  HB_FIELD(m.mdl, 1);
}

// per-instance episode record of the plant (hb_plant_set_episode, hb_episode.hpp), allocated by the first call that gives a
// configuration: the integer and the double record of every instance.  The trace is [B][trace_cap][HB_EP_TRACE_W] with trace_cap the
// largest trace_capacity set so far: a run-time extent, so the set call allocates it and the description does not name it.
struct EpisodeBatch {
  int B;
  int trace_cap;
  int* irec;
  double* drec;
  double* trace;
};
template <class F>
constexpr void fields(EpisodeBatch& e, size_t, F&& f) {
  HB_FIELD(e.irec, HB_EP_NI); HB_FIELD(e.drec, HB_EP_ND);
}

// respawn of ended instances (hb_plant_set_respawn, hb_respawn.hpp), allocated by the first call that gives a configuration: the totals of
// the finished episodes (itot, dtot), the spawn state the caller gave (q_spawn, v_spawn) and the last one drawn from it (q_last, v_last),
// and the two pending flags the MPC side consumes: rg_pending (k_refgen takes the latest stance positions from the observation) and
// mpc_pending (the mask of k_cold_start in the next solve).
struct RespawnBatch {
  int B;
  int* itot;
  double *dtot, *q_spawn, *v_spawn, *q_last, *v_last;
  int* rg_pending;
  unsigned char* mpc_pending;
};
template <class F>
constexpr void fields(RespawnBatch& r, size_t, F&& f) {
  HB_FIELD(r.itot, HB_RS_NI); HB_FIELD(r.dtot, HB_RS_ND); HB_FIELD(r.q_spawn, 16); HB_FIELD(r.v_spawn, 16); HB_FIELD(r.q_last, 16);
  HB_FIELD(r.v_last, 16); HB_FIELD(r.rg_pending, 1); HB_FIELD(r.mpc_pending, 1);
}

// scenario draw at respawn (hb_plant_set_scenario, hb_scenario.hpp), allocated by the first call that gives a configuration: the parameter
// row of the current episode (scen), the push record (first pushed step or -1, F_x, F_y) and the number of logged episodes (count).  The
// log is [B][log_cap][HB_SC_LOG_W] with log_cap the largest log_capacity set so far: a run-time extent, so the set call allocates it and
// the description does not name it.
struct ScenarioBatch {
  int B;
  int log_cap;
  double *scen, *push;
  int* count;
  double* log;
};
template <class F>
constexpr void fields(ScenarioBatch& c, size_t, F&& f) {
  HB_FIELD(c.scen, HB_SC_N); HB_FIELD(c.push, 3); HB_FIELD(c.count, 1);
}

// profile draw at respawn (hb_plant_set_profile_draw, hb_profiledraw.hpp), allocated by the first call that gives a configuration: the
// parameter row of the ground every instance stands on (row), the plant's knots of that ground as (s, z) pairs, zero behind the last
// (knots: what hb_plant_get_terrain_profile returns while the device draws) and the number of logged episodes (count).  The drawn records
// themselves go to ProfileBatch::prof and, with follow_map, GroundBatch::map.  The log is [B][log_cap][HB_PD_LOG_W] with log_cap the
// largest log_capacity set so far: a run-time extent, so the set call allocates it and the description does not name it.
struct ProfileDrawBatch {
  int B;
  int log_cap;
  double *row, *knots;
  int* count;
  double* log;
};
template <class F>
constexpr void fields(ProfileDrawBatch& d, size_t, F&& f) {
  HB_FIELD(d.row, HB_PD_N); HB_FIELD(d.knots, PD_KNOTS); HB_FIELD(d.count, 1);
}

// field draw at respawn (hb_plant_set_field_draw, hb_fielddraw.hpp), allocated by the first call that gives a configuration: the parameter
// row of the ground every instance stands on (row) and the number of logged episodes (count).  The drawn fields themselves go to
// FieldBatch::hdr / z and, with follow_map, GroundFieldBatch::hdr / z.  The log is [B][log_cap][HB_FD_LOG_W] with log_cap the largest
// log_capacity set so far: a run-time extent, so the set call allocates it and the description does not name it.
struct FieldDrawBatch {
  int B;
  int log_cap;
  double* row;
  int* count;
  double* log;
};
template <class F>
constexpr void fields(FieldDrawBatch& d, size_t, F&& f) {
  HB_FIELD(d.row, HB_FD_N); HB_FIELD(d.count, 1);
}

// actuator loop of the plant and the simulator end of the LCM link (hb_plant_step_hybrid, hb_plant_step_lcm, hb_plant_sense_lcm),
// allocated on the first call that needs them — the held-torque path needs none: the record of the last hybrid step, the staging of a
// host command and the received command (pos_des vel_des kp kd ff, one array each), the timestamp filter, the wire images
struct ActuatorBatch {
  int B;
  double *tau_first, *tau_mean;
  double *cmd[5], *rcmd[5];
  uint64_t* last_ts;
  int* accepted;
  uint64_t *wire_cmd, *wire_low, *wire_full;   // low_cmd_t in, low_state_t / full_state_t out, 8-byte words
};
template <class F>
constexpr void fields(ActuatorBatch& a, size_t, F&& f) {
  HB_FIELD(a.tau_first, 10); HB_FIELD(a.tau_mean, 10);
  HB_FIELD(a.cmd[0], 10); HB_FIELD(a.cmd[1], 10); HB_FIELD(a.cmd[2], 10); HB_FIELD(a.cmd[3], 10); HB_FIELD(a.cmd[4], 10);
  HB_FIELD(a.rcmd[0], 10); HB_FIELD(a.rcmd[1], 10); HB_FIELD(a.rcmd[2], 10); HB_FIELD(a.rcmd[3], 10); HB_FIELD(a.rcmd[4], 10);
  HB_FIELD(a.last_ts, 1); HB_FIELD(a.accepted, 1); HB_FIELD(a.wire_cmd, 62); HB_FIELD(a.wire_low, 42); HB_FIELD(a.wire_full, 58);
}

// ---- reference generation ----------------------------------------------------------------------------------------------
struct RefgenBatch {
  int B;
  int* n_ev;
  double* ev;
  int* modes;
  double* stance;   // [4][3] per instance
  double* phases;   // [4][HB_MAX_EVENTS + 1][RG_PHASE] per instance
  double* t0;
  double* cmd;
  int* status;
  int* n_knots;
  double* knot_t;
  double* knot_x;
  int init_stance;  // take the current feet as latest stance positions (first update after a reset without state)
};
template <class F>
constexpr void fields(RefgenBatch& r, size_t, F&& f) {
  HB_FIELD(r.n_ev, 1); HB_FIELD(r.ev, HB_MAX_EVENTS); HB_FIELD(r.modes, HB_MAX_EVENTS + 1); HB_FIELD(r.stance, 12);
  HB_FIELD(r.phases, 4 * (HB_MAX_EVENTS + 1) * RG_PHASE); HB_FIELD(r.t0, 1); HB_FIELD(r.cmd, 4); HB_FIELD(r.status, 1); HB_FIELD(r.n_knots, 1);
  HB_FIELD(r.knot_t, RG_MAX_KNOTS); HB_FIELD(r.knot_x, RG_MAX_KNOTS * HB_NX);
}

// ground map of the controller (hb_ground_set_profile, hb_ground.hpp), allocated by the first call that gives one: the record the ground
// forms of k_refgen and k_estimator read per instance (Ground: direction | number of segments | breakpoints | heights | slopes)
struct GroundBatch {
  int B;
  double* map;
};
template <class F>
constexpr void fields(GroundBatch& g, size_t, F&& f) {
  HB_FIELD(g.map, Ground::size);
}

// field map of the controller (hb_ground_set_field, hb_ground.hpp GroundField), allocated by the first call that gives one: hdr: the eight
// doubles of an instance's header (direction | origin | spacing | node counts), which the field forms of k_refgen and k_estimator keep in
// registers / LDS; z: the heights, [HB_FIELD_MAX_NODES][HB_FIELD_MAX_NODES] per instance, read from global memory
struct GroundFieldBatch {
  int B;
  double* hdr;
  double* z;
};
template <class F>
constexpr void fields(GroundFieldBatch& g, size_t, F&& f) {
  HB_FIELD(g.hdr, GroundField::size); HB_FIELD(g.z, GroundField::nz);
}

// choice read-back of the planner's sole forms (hb_ground_set_foothold, hb_refgen.hpp RgSole), allocated by the first call that switches
// the sole mode on: per (instance, foot) the candidate taken for the first foothold the last pass planned (shift; INT32_MIN: none), its
// defect and whether the fallback levelled it.  Written by the lane of the foot's toe.
struct SoleBatch {
  int B;
  int* shift;
  double* defect;
  int* level;
};
template <class F>
constexpr void fields(SoleBatch& c, size_t, F&& f) {
  HB_FIELD(c.shift, 2); HB_FIELD(c.defect, 2); HB_FIELD(c.level, 2);
}

// height scan (hb_plant_set_height_scan, hb_scan.hpp), allocated by the first call that gives a configuration: the lattice index of grid
// node (0, 0) at the last scan (k), the episode index that scan saw (episode_seen; below zero: the map is cleared), the number of returns
// (n_returns; -1: the last scan skipped the instance) and the return flag of every node in the pitch numbering (returned).  The scanned
// map itself goes to GroundFieldBatch::hdr / z.
struct ScanBatch {
  int B;
  int* k;
  int* episode_seen;
  int* n_returns;
  unsigned char* returned;
};
template <class F>
constexpr void fields(ScanBatch& c, size_t, F&& f) {
  HB_FIELD(c.k, 2); HB_FIELD(c.episode_seen, 1); HB_FIELD(c.n_returns, 1); HB_FIELD(c.returned, GroundField::nz);
}

// GaitBatch (hb_gait.hpp): the schedule, the template, the rate limiter and the velocity history are slot-major
template <class F>
constexpr void fields(GaitBatch& g, size_t, F&& f) {
  HB_FIELD(g.n_ev, 1); HB_FIELD(g.ev, slot_major(HB_MAX_EVENTS)); HB_FIELD(g.modes, slot_major(HB_MAX_EVENTS + 1)); HB_FIELD(g.tpl_n, 1);
  HB_FIELD(g.tpl_sw, slot_major(HB_GAIT_MAX_PHASES + 1)); HB_FIELD(g.tpl_modes, slot_major(HB_GAIT_MAX_PHASES)); HB_FIELD(g.last_vel, slot_major(4));
  HB_FIELD(g.cmd, 4); HB_FIELD(g.hist, slot_major(GAIT_HIST)); HB_FIELD(g.hist_n, 1); HB_FIELD(g.hist_head, 1); HB_FIELD(g.level, 1);
  HB_FIELD(g.vel_abs, 1); HB_FIELD(g.vel_avg, 1); HB_FIELD(g.status, 1);
}

// ---- state estimator -------------------------------------------------------------------------------------------------------
struct EstBatch {
  int B;
  double *xhat, *P, *yaw_last;                        // filter state
  const double *quat, *w_local, *a_local, *qj, *qdj;  // inputs: the estimator's own upload buffers, or aimed at another struct's arrays
  const int* contact;
  double *rbd, *x;                                    // outputs
  double *res_rbd, *res_x0;                           // resident inputs of hb_step_resident (or null): the caller's, not described
  // hb_estimator_contact_force: low-pass state pSCgZinvlast_, joint efforts, the two outputs, a host-given rbd
  double *cf_z, *cf_tau, *cf_dist, *cf_out, *cf_rbd;
};
// what k_estimator reads and writes: the part an instance range views
template <class F>
constexpr void filter_fields(EstBatch& e, F&& f) {
  HB_FIELD(e.xhat, 18); HB_FIELD(e.P, 324); HB_FIELD(e.yaw_last, 1); HB_FIELD(e.quat, 4); HB_FIELD(e.w_local, 3); HB_FIELD(e.a_local, 3);
  HB_FIELD(e.qj, 10); HB_FIELD(e.qdj, 10); HB_FIELD(e.contact, 4); HB_FIELD(e.rbd, HB_NRBD); HB_FIELD(e.x, HB_NX);
}
template <class F>
constexpr void fields(EstBatch& e, size_t, F&& f) {
  filter_fields(e, f);
  HB_FIELD(e.cf_z, HB_NV);   // (the contact-force observer runs on the whole batch only)
  HB_FIELD(e.cf_tau, HB_NJ); HB_FIELD(e.cf_dist, HB_NV); HB_FIELD(e.cf_out, 16); HB_FIELD(e.cf_rbd, HB_NRBD);
}

// hb_tick_resident: device-side upload targets of one tick's host inputs (read early in every instance range's tick, so that the
// next tick's upload only has to wait for that early point)
struct TickUpload {
  double *quat, *w, *a, *qj, *qdj;
  int* contact;
  double *tnow, *t0, *cmd;
};
template <class F>
constexpr void fields(TickUpload& up, size_t, F&& f) {
  HB_FIELD(up.quat, 4); HB_FIELD(up.w, 3); HB_FIELD(up.a, 3); HB_FIELD(up.qj, 10); HB_FIELD(up.qdj, 10); HB_FIELD(up.contact, 4);
  HB_FIELD(up.tnow, 1); HB_FIELD(up.t0, 1); HB_FIELD(up.cmd, 4);
}
#undef HB_FIELD

// ---- what is derived from a description ------------------------------------------------------------------------------------
template <class S>
constexpr int n_fields() {
  S s{};
  int n = 0;
  fields(s, 1, [&n](const char*, auto*&, Extent) { ++n; });
  return n;
}
// A member the description forgets would be allocated by nobody and left at instance 0 by every view: the struct is its scalars plus
// exactly the described pointers (plus the pointers named here, which are aimed at other structs' arrays).
constexpr size_t kPtr = sizeof(void*);
static_assert(sizeof(Batch) == 2 * sizeof(int) + n_fields<Batch>() * kPtr, "describe every array of Batch in fields()");
static_assert(sizeof(LsList) == n_fields<LsList>() * kPtr, "describe every array of LsList in fields()");
static_assert(sizeof(MpcCertBuf) == n_fields<MpcCertBuf>() * kPtr, "describe every array of MpcCertBuf in fields()");
static_assert(sizeof(WbcBatch) == kPtr /*B*/ + n_fields<WbcBatch>() * kPtr + kPtr /*policy_valid*/, "describe every array of WbcBatch in fields()");
static_assert(sizeof(WbcCertBuf) == n_fields<WbcCertBuf>() * kPtr && sizeof(HwbcCertBuf) == n_fields<HwbcCertBuf>() * kPtr, "certificate buffers");
static_assert(sizeof(PlantBatch) == kPtr /*B*/ + 2 * sizeof(double) + (n_fields<PlantBatch>() + 2 /*gyro_bias, accel_bias*/) * kPtr,
              "describe every array of PlantBatch in fields()");
static_assert(sizeof(ContactBatch) == 2 * sizeof(int) + n_fields<ContactBatch>() * kPtr, "describe every array of ContactBatch in fields()");
static_assert(sizeof(JointBatch) == kPtr /*B*/ + n_fields<JointBatch>() * kPtr, "describe every array of JointBatch in fields()");
static_assert(sizeof(TerrainBatch) == kPtr /*B*/ + n_fields<TerrainBatch>() * kPtr, "describe every array of TerrainBatch in fields()");
static_assert(sizeof(ProfileBatch) == kPtr /*B*/ + n_fields<ProfileBatch>() * kPtr, "describe every array of ProfileBatch in fields()");
static_assert(sizeof(FieldBatch) == kPtr /*B*/ + n_fields<FieldBatch>() * kPtr, "describe every array of FieldBatch in fields()");
static_assert(sizeof(ModelVarBatch) == kPtr /*B*/ + n_fields<ModelVarBatch>() * kPtr, "describe every array of ModelVarBatch in fields()");
static_assert(sizeof(EpisodeBatch) == 2 * sizeof(int) + (n_fields<EpisodeBatch>() + 1 /*trace*/) * kPtr, "describe every array of EpisodeBatch in fields()");
static_assert(sizeof(RespawnBatch) == kPtr /*B*/ + n_fields<RespawnBatch>() * kPtr, "describe every array of RespawnBatch in fields()");
static_assert(sizeof(ScenarioBatch) == 2 * sizeof(int) + (n_fields<ScenarioBatch>() + 1 /*log*/) * kPtr, "describe every array of ScenarioBatch in fields()");
static_assert(sizeof(ProfileDrawBatch) == 2 * sizeof(int) + (n_fields<ProfileDrawBatch>() + 1 /*log*/) * kPtr, "describe every array of ProfileDrawBatch in fields()");
static_assert(sizeof(FieldDrawBatch) == 2 * sizeof(int) + (n_fields<FieldDrawBatch>() + 1 /*log*/) * kPtr, "describe every array of FieldDrawBatch in fields()");
static_assert(sizeof(ActuatorBatch) == kPtr /*B*/ + n_fields<ActuatorBatch>() * kPtr, "describe every array of ActuatorBatch in fields()");
static_assert(sizeof(RefgenBatch) == kPtr /*B*/ + n_fields<RefgenBatch>() * kPtr + kPtr /*init_stance*/, "describe every array of RefgenBatch in fields()");
static_assert(sizeof(GroundBatch) == kPtr /*B*/ + n_fields<GroundBatch>() * kPtr, "describe every array of GroundBatch in fields()");
static_assert(sizeof(GroundFieldBatch) == kPtr /*B*/ + n_fields<GroundFieldBatch>() * kPtr, "describe every array of GroundFieldBatch in fields()");
static_assert(sizeof(SoleBatch) == kPtr /*B*/ + n_fields<SoleBatch>() * kPtr, "describe every array of SoleBatch in fields()");
static_assert(sizeof(ScanBatch) == kPtr /*B*/ + n_fields<ScanBatch>() * kPtr, "describe every array of ScanBatch in fields()");
static_assert(sizeof(GaitBatch) == 2 * sizeof(int) + n_fields<GaitBatch>() * kPtr, "describe every array of GaitBatch in fields()");
static_assert(sizeof(EstBatch) == kPtr /*B*/ + (n_fields<EstBatch>() + 2 /*res_rbd, res_x0*/) * kPtr, "describe every array of EstBatch in fields()");
static_assert(sizeof(TickUpload) == n_fields<TickUpload>() * kPtr, "describe every array of TickUpload in fields()");

// The same struct with every described array starting at instance i0.
template <class S>
S from_instance(const S& s, size_t N, int i0) {
  S v = s;
  fields(v, N, [i0](const char*, auto*& p, Extent e) { p += size_t(i0) * e.step; });
  return v;
}
// Sub-batch [i0, i0 + cnt) of a batch: same layout, offset base pointers.
template <class S>
S view(const S& s, size_t N, int i0, int cnt) {
  S v = from_instance(s, N, i0);
  v.B = cnt;
  return v;
}
// (what k_estimator reads and writes; the resident outputs res_* are the caller's, the contact-force observer is not viewed)
inline EstBatch view(const EstBatch& e, size_t, int i0, int cnt) {
  EstBatch v = e;
  filter_fields(v, [i0](const char*, auto*& p, Extent x) { p += size_t(i0) * x.step; });
  v.B = cnt;
  return v;
}
// Extent of the array `member` of s (n = 0: s does not describe it).
template <class S, class T>
Extent extent_of(S& s, size_t N, T* const& member) {
  Extent found(0);
  fields(s, N, [&](const char*, auto*& p, Extent e) {
    if (static_cast<const void*>(&p) == static_cast<const void*>(&member)) found = e;
  });
  return found;
}

}  // namespace
