// hb_config.reserved: ONE table of every value that any site of the library reads, and the rules that turn a value into the kernel forms
// the host launches.  The field is copied into DevConfig::debug_stop (hb_host.hpp) and handed to the two backward sweeps as `dbg`;
// every comparison in the kernels and device headers uses the names below (hunter_bipedal_control_amd/abi.py mirrors them for the tools
// and tests, DESIGN.md §3.0 prints the table).  Three kinds of value share the field:
//   selectors   live in the shipped library: they force one of two bit-identical forms of a kernel (tests, tuning);
//   stops       read only by the -DHB_ABLATE profiling build (csrc/build.sh --ablate): the kernel named returns behind the phase named,
//               so that the phases can be timed and counted one by one (each stop includes everything ahead of it in code order);
//   traces      profiling build: one wavefront prints the cycle counts of its phases.
// The rules that depend on the state of the context instead (a ground map, the plant's contact model, joints, terrain, variation and
// profile, height field) stand here too: use_ground_forms, plant_form.
// Plain C++14, no HIP: tests/host_emu/formsemu.cpp compiles this header with g++.
#pragma once

namespace hb {
namespace form {

// X(identifier, value, read by, meaning)
#define HB_FORM_CODES(X) \
  X(NONE,             0, "decode_forms",                  "the product: every form picked by the number of instances in flight") \
  /* stops of the LQ approximation (k_lq; the dense part also in k_lq_trip), in code order */ \
  X(LQ_LOADS,        10, "lq_node",                       "stop: loads") \
  X(LQ_LEG_VALUES,    6, "lq_node",                       "stop: + leg value pass") \
  X(LQ_VALUE_PREPASS, 7, "lq_node",                       "stop: + value pre-pass") \
  X(LQ_DIRECTIONS,    9, "lq_node_dense",                 "stop: + direction pass (k_lq_trip: read-back of the parked image + direction pass)") \
  X(LQ_COMPOSE,       1, "lq_tail",                       "stop: + compose") \
  X(LQ_FACTOR,        2, "lq_tail",                       "stop: + Gram matrix, pivoted Cholesky") \
  X(LQ_SOLVES,        3, "lq_tail",                       "stop: + solves") \
  X(LQ_DEFECT,       30, "lq_tail",                       "stop: + defect, A~ B~ tiles") \
  X(LQ_B_COLUMNS,    31, "lq_tail",                       "stop: + B~ columns, b~") \
  X(LQ_COST,          4, "lq_tail",                       "stop: + cost") \
  X(LQ_SOFT_ROWS,     5, "lq_tail",                       "stop: + soft rows, Pj, M") \
  X(LQ_Q,            32, "lq_tail",                       "stop: + Q~ q~") \
  X(LQ_P,            33, "lq_tail",                       "stop: + P~ r~") \
  X(LQ_R,            34, "lq_tail",                       "stop: + R~ (what is left: recovery data)") \
  /* stops of the WeightedWbc solve (k_wbc), in code order */ \
  X(WBC_A_BASE,      13, "wbc_phase_a, wbc_solve",        "stop: phase A, base pass") \
  X(WBC_A_LEGS,      14, "wbc_phase_a, wbc_solve",        "stop: + leg passes") \
  X(WBC_A_FINISH,    15, "wbc_phase_a, wbc_solve",        "stop: + composition, desired base acceleration") \
  X(WBC_A,           11, "wbc_solve",                     "stop: phase A (rigid-body quantities and fills)") \
  X(WBC_B,           12, "wbc_solve",                     "stop: + phase B (cost factor, unconstrained minimiser)") \
  /* stops of the one-wavefront backward sweep (k_ric_bwd; riccati_bwd_node), in code order */ \
  X(RIC1_STAGING,    20, "k_ric_bwd",                     "stop: staging of the record only") \
  X(RIC1_GEMM1,      21, "ric_phase12, k_ric_bwd",        "stop: + GEMM 1") \
  X(RIC1_GEMM2,      22, "ric_phase12, k_ric_bwd",        "stop: + GEMM 2") \
  X(RIC1_FACTOR,     23, "riccati_bwd_node, k_ric_bwd",   "stop: + factor, solves (what is left: GEMM 3)") \
  /* stops of the four-wavefront backward sweep (k_ric_bwd4), in code order: decode_forms makes them launch that kernel */ \
  X(RIC4_STAGING,    24, "k_ric_bwd4, decode_forms",      "stop: staging only") \
  X(RIC4_GEMM1,      25, "k_ric_bwd4, decode_forms",      "stop: + GEMM 1") \
  X(RIC4_GEMM2,      26, "k_ric_bwd4, decode_forms",      "stop: + GEMM 2") \
  X(RIC4_FACTOR,     27, "k_ric_bwd4, decode_forms",      "stop: + factor, solves | first part of GEMM 3") \
  /* stops of the HierarchicalWbc cascade (k_hwbc), in code order */ \
  X(HWBC_LEVEL0,     41, "k_hwbc",                        "stop: level 0") \
  X(HWBC_KERNEL0,    43, "hwbc_solve",                    "stop: + kernel basis of level 0") \
  X(HWBC_QP1,        44, "hwbc_solve",                    "stop: + level-1 QP") \
  X(HWBC_LEVEL1,     42, "k_hwbc",                        "stop: + kernel basis of level 1 (what is left: level 2)") \
  /* selectors of the sweeps */ \
  X(RIC_BWD_ONE,    101, "decode_forms",                  "selector: one-wavefront backward sweep (k_ric_bwd)") \
  X(RIC_BWD_FOUR,   104, "decode_forms",                  "selector: four-wavefront backward sweep (k_ric_bwd4)") \
  X(RIC_FWD_ROW,    111, "decode_forms",                  "selector: row form of the forward sweep (k_ric_fwd)") \
  X(RIC_FWD_WAVE,   114, "decode_forms",                  "selector: wave form of the forward sweep (k_ric_fwd_w)") \
  /* profiling variants of k_lq_trip */ \
  X(LQT_ONE_RECORD, 117, "k_lq_trip",                     "stop: every node of a workgroup writes one record slot (stores issued, lines stay in the L2)") \
  X(LQT_TRACE,      118, "k_lq_trip, lq_trip_values",     "trace (-DHB_LQV_TRACE): cycle counts of workgroup 1000's value phase; the kernel returns behind it") \
  X(LQT_PARK_NOTHING, 119, "lq_park_out",                 "stop: the value phase computes but parks nothing (stale data is read back)") \
  X(LQT_VALUES_ONCE, 125, "k_lq_trip",                    "stop: the value phase runs once per trip, later launches reuse what it parked") \
  X(LQT_VALUES,     126, "k_lq_trip",                     "stop: the value phase alone (first of LQT_VALUES .. LQT_VALUES_LEGS)") \
  X(LQT_VALUES_FWD, 127, "k_lq_trip, lq_trip_values",     "stop: the value phase up to its forward sweep") \
  X(LQT_VALUES_LEGS, 128, "k_lq_trip, lq_trip_values",    "stop: the value phase up to its leg pass (last of LQT_VALUES ..)") \
  X(LQ_ONE_NODE,    129, "decode_forms",                  "selector: the one-node-per-wavefront kernel k_lq (differs from the trips by rounding)") \
  /* selector of the line search */ \
  X(LS_EVAL_NODE,   151, "decode_forms",                  "selector: thread-per-node line-search evaluation (k_ls_eval_node, k_ls_tail_eval_node; differs from the two-lane form by rounding)") \
  /* traces */ \
  X(RIC1_TRACE,     197, "k_ric_bwd",                     "trace: cycle counts of stage 50 of instance 9") \
  X(WBC_TRACE,      198, "wbc_solve, decode_forms",       "trace: cycle counts of the WeightedWbc solve of instance 5 (leaves the sweep's choice alone)") \
  X(RIC4_TRACE,     199, "k_ric_bwd4, decode_forms",      "trace: cycle counts of stage 50 of instance 7")

// Families of selectors, by their bounds.  X(identifier, first, last, read by, meaning): yields identifier_FIRST / identifier_LAST
#define HB_FORM_RANGES(X) \
  X(LQ_TRIP_POW2,   120, 124, "decode_forms",             "selector: LQ trips of 2^(value - first) nodes") \
  X(LQ_TRIP_LEN,    131, 146, "decode_forms",             "selector: LQ trips of value - first + 1 nodes (1 .. 16)")

enum Code : int {
#define HB_FORM_ENUM(id, value, reader, meaning) id = value,
#define HB_FORM_RANGE_ENUM(id, first, last, reader, meaning) id##_FIRST = first, id##_LAST = last,
  HB_FORM_CODES(HB_FORM_ENUM) HB_FORM_RANGES(HB_FORM_RANGE_ENUM)
#undef HB_FORM_ENUM
#undef HB_FORM_RANGE_ENUM
};

struct Entry { const char* name; int first, last; const char* reader; const char* meaning; };
constexpr Entry kTable[] = {
#define HB_FORM_ROW(id, value, reader, meaning) {#id, value, value, reader, meaning},
#define HB_FORM_RANGE_ROW(id, first, last, reader, meaning) {#id, first, last, reader, meaning},
  HB_FORM_CODES(HB_FORM_ROW) HB_FORM_RANGES(HB_FORM_RANGE_ROW)
#undef HB_FORM_ROW
#undef HB_FORM_RANGE_ROW
};

}  // namespace form

// ---------------------------------------------------------------------------------------------------------
// The forms the host launches.  Auto: picked per launch by `concurrent`, the instances whose kernels may be in flight at the same time
// (the whole batch when its instance ranges free-run on their own streams): what decides is how many share the chip, not one launch.
struct KernelForms {
  enum class Bwd { Auto, One, Four } bwd = Bwd::Auto;     // backward sweep: k_ric_bwd / k_ric_bwd4
  enum class Fwd { Auto, Row, Wave } fwd = Fwd::Auto;     // forward sweep: k_ric_fwd / k_ric_fwd_w
  enum class Lq { Trips, OneNode } lq = Lq::Trips;        // LQ approximation: k_lq_trip / k_lq
  enum class Ls { Pair, Node } ls = Ls::Pair;             // line-search evaluation: k_ls_eval, k_ls_tail_eval / k_ls_eval_node, k_ls_tail_eval_node
  int trip_len = 0;                                       // nodes per trip of k_lq_trip, forced; 0: by the batch
};

// `ablate`: the rules of the profiling build (the library passes HB_ABLATE_ON), whose stops and traces live in ONE of the two backward
// sweeps each and therefore pin it.
inline KernelForms decode_forms(int reserved, bool ablate) {
  using namespace form;
  KernelForms f;
  if (reserved == RIC_BWD_FOUR) f.bwd = KernelForms::Bwd::Four;
  else if (ablate && ((reserved >= RIC4_STAGING && reserved <= RIC4_FACTOR) || reserved == RIC4_TRACE)) f.bwd = KernelForms::Bwd::Four;   // k_ric_bwd4's own
  else if (reserved == RIC_BWD_ONE) f.bwd = KernelForms::Bwd::One;
  else if (ablate && reserved != NONE && reserved != WBC_TRACE) f.bwd = KernelForms::Bwd::One;   // any other stop: the sweep the profiles were taken on
  if (reserved == RIC_FWD_WAVE) f.fwd = KernelForms::Fwd::Wave;
  else if (reserved == RIC_FWD_ROW) f.fwd = KernelForms::Fwd::Row;
  if (reserved == LQ_ONE_NODE) f.lq = KernelForms::Lq::OneNode;
  if (reserved == LS_EVAL_NODE) f.ls = KernelForms::Ls::Node;
  if (reserved >= LQ_TRIP_POW2_FIRST && reserved <= LQ_TRIP_POW2_LAST) f.trip_len = 1 << (reserved - LQ_TRIP_POW2_FIRST);
  if (reserved >= LQ_TRIP_LEN_FIRST && reserved <= LQ_TRIP_LEN_LAST) f.trip_len = reserved - LQ_TRIP_LEN_FIRST + 1;   // (launch-geometry sweeps)
  return f;
}

// Backward sweep: small launches take four wavefronts per instance (k_ric_bwd4), large ones the one-wavefront form (eight sweeps per CU
// are then the better use of the chip).  Measured, DESIGN.md 3.2.
constexpr int kRicBwd4MaxBatch = 512;
inline bool use_ric_bwd4(const KernelForms& f, int concurrent) {
  return f.bwd == KernelForms::Bwd::Four || (f.bwd == KernelForms::Bwd::Auto && concurrent <= kRicBwd4MaxBatch);
}

// Forward sweep: the wave form while the batch leaves a SIMD one wavefront.
constexpr int kRicFwdWaveMaxBatch = 512;
inline bool use_ric_fwd_wave(const KernelForms& f, int concurrent) {
  return f.fwd == KernelForms::Fwd::Wave || (f.fwd == KernelForms::Fwd::Auto && concurrent <= kRicFwdWaveMaxBatch);
}

// Planner and filter: the ground forms (k_refgen_ground, k_estimator_ground) while a profile map is in force (hb_ground_set_profile), the
// field forms (k_refgen_gfield, k_estimator_gfield) while a field map is (hb_ground_set_field), the base forms otherwise — the base forms
// never see a map, so a context without one runs what it always ran.  One map at a time: the host never has both in force, and a field
// would go first.
// MAP_*: the map kind under its one set of names — the template argument MAP of the device routines that put a point to the map
// (hb_ground.hpp map_height, refgen_plan, rg_make_target, estimator_update and the kernel bodies) and the values of GroundForm.  They stand
// here, not in hb_ground.hpp: this header is upstream of it (hb_math.hpp) and is compiled alone as C++14.
constexpr int MAP_NONE = 0, MAP_PROFILE = 1, MAP_FIELD = 2;
enum class GroundForm { None = MAP_NONE, Profile = MAP_PROFILE, Field = MAP_FIELD };
inline GroundForm use_ground_forms(bool map_in_force, bool field_map_in_force = false) {
  return field_map_in_force ? GroundForm::Field : map_in_force ? GroundForm::Profile : GroundForm::None;
}

// Planner only: the sole forms (k_refgen_ground_sole, k_refgen_gfield_sole) while a map is in force AND the foothold configuration asks for
// soles (hb_ground_set_foothold, mode 1).  Without a map there is nothing to be consistent with: the base form runs whatever the mode, and
// a context that never made the call (mode 0) launches what it always launched.  The filter has no sole form.
inline bool use_sole_forms(GroundForm gf, int foothold_mode = 0) { return gf != GroundForm::None && foothold_mode == 1; }

// Plant step: which of the twenty-two step kernels a launch takes (hb_api_plant.hpp plant_launch names them).  Contact mode 0 is the pinned
// stub (k_plant / k_plant_hybrid), which knows neither joints nor ground; in contact model 1 a height field or a profile (one ground at a
// time: the host never has both in force) goes before a model variation (the field and profile kernels take the variation by pointer), a
// variation before a terrain (the varied kernels read the terrain array, where the
// host keeps the level record while no terrain is in force), a terrain before the level ground.  `joints` and `hybrid` pick the kernel of
// the family: joint model on, the command's law per substep instead of a held torque.
struct PlantForm {
  enum class Ground { Pinned, Level, Terrain, Varied, Profile, Field } ground;
  bool joints, hybrid;
};
inline PlantForm plant_form(int contact_mode, bool joints_on, bool terrain_on, bool modelvar_on, bool profile_on, bool hybrid,
                            bool field_on = false) {
  using G = PlantForm::Ground;
  if (contact_mode != 1) return {G::Pinned, false, hybrid};
  return {field_on ? G::Field : profile_on ? G::Profile : modelvar_on ? G::Varied : terrain_on ? G::Terrain : G::Level, joints_on, hybrid};
}

// Height scan (hb_plant_scan): which form of k_plant_scan a launch takes — the plant's ground the scan samples, by the order of plant_form
// (a height field or a profile before a terrain, a terrain before the level ground).  The values are hb_scan.hpp's SCAN_*: the template
// argument GROUND of its routines.  A model variation changes no ground: without a terrain the varied kernels step on the level record.
enum class ScanGround { None = 0, Plane = 1, Profile = 2, Field = 3 };
inline ScanGround scan_ground(bool terrain_on, bool profile_on, bool field_on) {
  return field_on ? ScanGround::Field : profile_on ? ScanGround::Profile : terrain_on ? ScanGround::Plane : ScanGround::None;
}

// LQ approximation: trips of this many nodes per wavefront (k_lq_trip).  Longer trips fill the lanes of the value phase better (16 nodes:
// all 64), shorter ones keep small batches spread over the chip and balance them finer: the longest trip that still gives every
// wavefront slot of the chip (12 per CU) four trips of the CONCURRENT batch — 16 nodes from 2048 instances up, 8 at 1024, 4 at 512
// (512 x 108 on two ranges, updates/s: one-node kernel 329.7 k, 4 nodes 325.0 k, 8: 316.9 k, 16: 305.2 k; forced lengths that are no
// power of two measured within the noise of the powers of two at 512, 1024 and 4096 instances).  The result does not depend on the choice.
constexpr int kLqTripsPerSlot = 4;
inline int lq_trip_len(const KernelForms& f, int concurrent, int Nmax, int n_cu) {
  if (f.trip_len) return f.trip_len;
  const long slots = 12L * n_cu;
  for (int sh = 4; sh > 0; --sh)
    if (long(concurrent) * ((Nmax + (1 << sh) - 1) >> sh) >= kLqTripsPerSlot * slots) return 1 << sh;
  return 1;
}

}  // namespace hb
