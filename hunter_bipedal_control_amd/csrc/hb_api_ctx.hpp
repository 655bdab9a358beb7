// Host side of libhunter_hip.so, part 1: the context, the helpers every entry point shares (errors, entry prologue, instance-range
// check, allocation on first use, copies and zero fills derived from the layout descriptions of hb_layout.hpp, the growable per-instance
// logs, the refusal texts, pinned staging, lazy join) and hb_create / hb_destroy / hb_sync / hb_get_stats.  Included by hb_kernels.hip only.
#pragma once

// Error text of the last failed call, per calling thread (errno-like): the reference drives one solver from two threads
// (control thread / MPC thread, LeggedController.cpp:396-421) and each reads back only its own failures.
struct ErrSlot {
  static std::string& tl() { static thread_local std::string s; return s; }
  ErrSlot& operator=(const std::string& m) { tl() = m; return *this; }
  ErrSlot& operator=(const char* m) { tl() = m; return *this; }
  const char* c_str() const { return tl().c_str(); }
};

// Slots of hb_ctx::ev: timing points of the MPC phases (iteration 0 of a whole-batch solve) and of the WBC, then the policy
// hand-over: published, and consumed by the last policy evaluation.
enum EvSlot { EV_LQ_BEGIN, EV_LQ_END, EV_RIC_BWD_END, EV_RIC_FWD_END, EV_LS_END, EV_WBC_BEGIN, EV_WBC_END, EV_PUBLISHED, EV_POLICY_READ, EV_COUNT };
constexpr int kMaxRanges = 8;  // instance ranges (hb_set_chunks), each on a stream of its own
// Slots of hb_ctx::ev_sync, cross-stream ordering points that are NOT timing events: a resident-input writer (plant, estimator) waits
// for the MPC stream / the MPC stream for it; fork of the range streams from the MPC / WBC streams; SYNC_JOIN + c: join of range c.
enum SyncSlot { SYNC_BEFORE_WRITER, SYNC_AFTER_WRITER, SYNC_FORK_MPC, SYNC_FORK_WBC, SYNC_JOIN, SYNC_COUNT = SYNC_JOIN + kMaxRanges };

struct hb_ctx {
  int device = 0, B = 0, Nmax = 0, n_cu = 256;
  // Guards the host-side state both threads touch while ENQUEUEING work (policy hand-over flags, counters); never held across
  // a device synchronisation.
  std::mutex mtx;
  hb_model model;
  hb_config config;
  DevModel hmodel;
  DevConfig hconfig;
  KernelForms forms;   // decoded once from config.reserved (hb_forms.hpp): which form of the LQ kernel and the sweeps is launched
  DevModel* dmodel = nullptr;
  DevConfig* dconfig = nullptr;
  Batch b{};
  LsList lslist{};   // the line search's list of refused instances, per instance range (hb_layout.hpp)
  int ls_per = 0;    // instances per range of the last MPC call (the whole batch on one stream: B): its counters are the slots 0, ls_per, ...
  hipStream_t s_mpc = nullptr, s_wbc = nullptr;
  hipEvent_t ev[EV_COUNT]{};
  hipEvent_t ev_sync[SYNC_COUNT]{};
  // Pinned staging for the asynchronous forms of hb_set_resident_time / hb_estimator_update / hb_refgen_update: a caller-owned host
  // array is copied into a library-owned pinned slot and uploaded from there, so the call returns without a device
  // synchronisation and the caller's array is free again.  STAGE_DEPTH slots per array, each guarded by the event of its last upload:
  // the host can run at most STAGE_DEPTH ticks ahead of the device.
  static constexpr int STAGE_ARRAYS = 10, STAGE_DEPTH = 4;
  struct StageSlot { void* host = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool pending = false; };
  StageSlot stage[STAGE_ARRAYS][STAGE_DEPTH];
  unsigned stage_turn[STAGE_ARRAYS]{};
  // hb_tick_resident: the upload targets of one tick's host inputs (hb_layout.hpp), the upload stream and its events
  TickUpload up{};
  hipStream_t s_up = nullptr;
  hipEvent_t ev_up = nullptr, ev_consumed[kMaxRanges]{};
  int consumed_pending = 0;
  bool grid_saved = false;  // tp / modep / np_nodes hold the grid the iterate lives on; the tables have changed since
  bool policy_read_pending = false;
  bool refs_set = false, traj_set = false, timed = false;
  std::vector<void*> allocs;
  ErrSlot err;
  WbcBatch w{};
  hb_stats stats{};
  double* x0_seq = nullptr;  // optional device-resident sequence of measured states for hb_step_resident
  int n_seq = 0, seq_idx = 0;
  // instance chunks pipelined on their own streams by hb_step_resident (independent instances: the latency-bound
  // per-instance sweeps of one chunk overlap the per-node kernels of another)
  int n_chunks = 1;
  hipStream_t s_chunk[kMaxRanges]{};
  // hipGraphs of one chunk's whole step (x0 -> SQP iteration -> publish -> policy -> WBC), one per (chunk, x0-sequence slot): at
  // small batch sizes the step is launch bound — ~25 enqueues per chunk and step against kernels of 100..900 us — and the
  // chunk streams only overlap if the host keeps them fed.  Graphs captured in epoch e are stale once a device pointer they
  // hold changes (the iterate / previous-iterate swap of the warm start, a new x0 sequence, a new chunk count).
  static constexpr int GRAPH_SLOTS = 16;
  hipGraphExec_t chunk_graph[kMaxRanges][GRAPH_SLOTS]{};
  uint64_t chunk_graph_epoch[kMaxRanges][GRAPH_SLOTS]{};
  uint64_t graph_epoch = 1;
  int64_t dbg_graph_launches = 0, dbg_direct = 0, dbg_forks = 0, dbg_captures = 0, dbg_capture_failures = 0;
  bool graph_disabled = false;   // a capture / instantiation failed once: direct launches from then on (until hb_set_chunks)
  int steady_chunked_steps = 0;   // chunked steps since the last fork: graphs are only captured in steady state
  int chunks_pending = 0;    // chunk streams of the last chunked hb_step_resident not yet joined into the library streams
  bool fork_needed = true;   // something may have been queued on the library streams since the last chunked step
  unsigned char* reset_mask = nullptr;  // [B] staging of hb_mpc_reset_masked
  double* jc_out = nullptr;  // joint command outputs [6][B][10]
  bool jc_computed = false;  // hb_joint_command has run (jc_out alone is also allocated by hb_joint_set_flags / get_emergency_stop)
  int* jc_estop = nullptr;   // [B] latched emergencyStopFlag_ per instance
  int* jc_loaded = nullptr;  // [B] loadControllerFlag_ per instance (default: loaded)
  uint64_t* lcm_cmd = nullptr;    // [B][62] low_cmd_t wire images
  uint64_t* lcm_state = nullptr;  // [B][42] low_state_t wire images
  long long* lcm_ts = nullptr;    // [B]
  int* lcm_bad = nullptr;
  PlantBatch plant{};
  bool plant_ready = false;
  // sensor model of the plant (hb_plant_set_sensor_model): sens_noisy = a configuration with at least one sigma > 0 is in force;
  // sense_count = hb_plant_sense calls since the model was set (the noise counter); sensed = the sensor arrays hold a reading of this
  // plant (cleared by hb_plant_reset)
  hb_sensor_config sens_cfg{};
  bool sens_noisy = false, sensed = false;
  uint64_t sense_count = 0;
  double *sens_gyro_bias_buf = nullptr, *sens_accel_bias_buf = nullptr;  // [B][3] each, allocated on the first non-null bias
  // contact model of the plant (hb_plant_set_contact_model): contact_cfg.mode = 1 while the ground model is in force; the arrays are
  // allocated by the first call that selects it.  Model and wrench survive hb_plant_reset.
  ContactBatch contact{};
  hb_contact_config contact_cfg{};
  // joint model of contact model 1 (hb_plant_set_joint_model): joints_on while one is in force; the arrays are allocated on first use
  JointBatch joints{};
  hb_joint_model joint_model{};
  bool joints_on = false;
  // per-instance terrain of contact model 1 (hb_plant_set_terrain): terrain_on while one is in force (the step calls then launch the
  // terrain kernels); the array is allocated on first use, terrain_host is its host image ([B][Terrain::size], what hb_plant_get_terrain reports)
  TerrainBatch terrain{};
  std::vector<double> terrain_host;
  bool terrain_on = false;
  // per-instance terrain profile of contact model 1 (hb_plant_set_terrain_profile): profile_on while one is in force (the step calls then
  // launch the profile kernels, and terrain_on is false: one ground at a time); the arrays are allocated on first use, profile_host is the
  // host image of the stored records ([B][Profile::stored]), profile_knots the knots as given ([B][HB_PROFILE_MAX_KNOTS][2], zero beyond K)
  ProfileBatch profile{};
  std::vector<double> profile_host, profile_knots;
  bool profile_on = false;
  // per-instance height field of contact model 1 (hb_plant_set_terrain_field): field_on while one is in force (the step calls then launch
  // the field kernels, and terrain_on and profile_on are false: one ground at a time); the arrays are allocated on first use, field_hdr_host
  // is the host image of the stored records ([B][Field::stored]), field_z_host that of the heights ([B][Field::nz], zero beyond (nu, nw))
  FieldBatch field{};
  std::vector<double> field_hdr_host, field_z_host;
  bool field_on = false;
  // per-instance model variation of contact model 1 (hb_plant_set_model_variation): modelvar_on while one is in force (the step calls then
  // launch the varied kernels); the records are allocated on first use, modelvar_host is their host image (what hb_plant_get_model_variation
  // reports).  Without a terrain the varied kernels read the level record of the configuration in force out of `terrain` (modelvar_level).
  ModelVarBatch modelvar{};
  std::vector<DevModel> modelvar_host;
  bool modelvar_on = false;
  // actuator loop per substep and the simulator end of the LCM link (hb_plant_step_hybrid / _lcm, hb_plant_sense_lcm): allocated on first use
  ActuatorBatch act{};
  // per-instance episode record (hb_plant_set_episode): episode_on while one is in force (every plant step is then followed by
  // k_plant_episode); the records are allocated by the first call that gives a configuration.  The configuration survives hb_plant_reset.
  EpisodeBatch episode{};
  hb_episode_config episode_cfg{};
  bool episode_on = false;
  // respawn of ended instances (hb_plant_set_respawn): respawn_on while a configuration is in force; the arrays are allocated by the first
  // call that gives one.  rs_rg_due / rs_mpc_due (under mtx): a respawn has been enqueued since the last hb_refgen_update / MPC solve, which
  // then consume the device's pending flags.  The configuration survives hb_plant_reset.
  RespawnBatch respawn{};
  hb_respawn_config respawn_cfg{};
  bool respawn_on = false, rs_rg_due = false, rs_mpc_due = false;
  // scenario draw at respawn (hb_plant_set_scenario): scenario_on while a configuration is in force; the arrays are allocated by the first
  // call that gives one.  While it is on the device owns the terrain and model records (terrain_host / modelvar_host are stale and the
  // getters read the device) and, with HB_SC_PUSH, the external wrench.
  ScenarioBatch scenario{};
  hb_scenario_config scenario_cfg{};
  bool scenario_on = false;
  // profile draw at respawn (hb_plant_set_profile_draw): profile_draw_on while a configuration is in force (profile_on is then true as
  // well, and profile_host / profile_knots / ground_host / ground_knots are stale: profile_draw_refresh_host brings them up to date);
  // profile_draw_cfg holds the direction already normalised; the arrays are allocated by the first call that gives a configuration
  ProfileDrawBatch profile_draw{};
  hb_profile_draw_config profile_draw_cfg{};
  bool profile_draw_on = false;
  // field draw at respawn (hb_plant_set_field_draw): field_draw_on while a configuration is in force (field_on is then true as well, and
  // field_hdr_host / field_z_host / gfield_hdr_host / gfield_z_host are stale: field_draw_refresh_host brings them up to date);
  // field_draw_cfg holds the direction already normalised; the arrays are allocated by the first call that gives a configuration
  FieldDrawBatch field_draw{};
  hb_field_draw_config field_draw_cfg{};
  bool field_draw_on = false;
  // height scan (hb_plant_set_height_scan): scan_on while a configuration is in force (gfield_on is then true as well, and gfield_hdr_host /
  // gfield_z_host are stale: scan_refresh_host brings them up to date); scan_cfg holds the direction already normalised; scan_count =
  // hb_plant_scan calls since the configuration was set (the noise counter); the arrays are allocated by the first call that gives one
  ScanBatch scan{};
  hb_height_scan_config scan_cfg{};
  bool scan_on = false;
  uint32_t scan_count = 0;
  // reference generation (allocated on the first hb_refgen_reset)
  RefgenBatch rg{};
  hb_refgen_config rg_cfg{};
  bool rg_ready = false;
  std::vector<int> rg_have_schedule;
  // device gait manager (allocated on the first hb_gait_reset); while gait_on, k_gait writes the schedule windows
  GaitBatch gait{};
  hb_gait_config gait_cfg{};
  bool gait_on = false;
  // ground map of the controller (hb_ground_set_profile): ground_on while one is in force (the planner and the filter then run in their
  // ground forms, hb_forms.hpp use_ground_forms); the array is allocated on first use, ground_host is the host image of the stored records
  // ([B][Ground::size]), ground_knots the knots as given ([B][HB_PROFILE_MAX_KNOTS][2], zero beyond K).  Nothing resets it but its own setter.
  GroundBatch ground{};
  std::vector<double> ground_host, ground_knots;
  bool ground_on = false;
  // field map of the controller (hb_ground_set_field): gfield_on while one is in force (the field forms then run); one map at a time, so
  // never together with ground_on.  gfield_hdr_host ([B][GroundField::size]) and gfield_z_host ([B][GroundField::nz], zero beyond
  // (nu, nw)) are the host images.  Nothing resets it but the two setters.
  GroundFieldBatch gfield{};
  std::vector<double> gfield_hdr_host, gfield_z_host;
  bool gfield_on = false;
  // foothold configuration (hb_ground_set_foothold): foothold_cfg.mode 1 while the sole mode is on (the planner then runs in its sole forms
  // whenever a map is in force, hb_forms.hpp use_sole_forms); sole: the choice read-back, allocated by the first call that switches the
  // mode on.  Nothing resets the configuration but its own setter.
  hb_foothold_config foothold_cfg{};
  SoleBatch sole{};
  // state estimator (allocated on the first hb_estimator_reset)
  EstBatch est{};
  hb_estimator_config est_cfg{};
  bool est_ready = false;
  // KKT certificate of the WeightedWbc QP (hb_wbc_set_certificate): allocated on the first enable; cert_last tells whether the last
  // WBC call ran the certificate kernel.  The per-level certificate of the HierarchicalWbc cascade (hb_hwbc_set_certificate) is the
  // same switch (wbc_cert / cert_last) on a wbc_type = 1 context, with its own buffers.
  bool wbc_cert = false, cert_last = false;
  WbcCertBuf wcert{};
  HwbcCertBuf hcert{};
  // KKT certificate of the MPC's stage QP (hb_mpc_get_certificate): work buffers allocated on the first call.  The records, gains and
  // step of a solve belong to the node tables and the iterate it ran on: mpc_tables_epoch counts their replacements by the host
  // (hb_mpc_set_references, hb_refgen_update, hb_mpc_reset*, hb_mpc_set_trajectory), mpc_solved_epoch is its value at the last MPC call
  // (0: none yet).
  MpcCertBuf mcert{};
  uint64_t mpc_tables_epoch = 1, mpc_solved_epoch = 0;
};

static thread_local std::string g_create_error;

#define HB_HIP(call)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess) {                                                                \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
      return HB_ERR_DEVICE;                                                                \
    }                                                                                      \
  } while (0)

// fails the call with `code` and the error text when cond holds
#define HB_FAIL_IF(cond, code, text) \
  do {                               \
    if (cond) {                      \
      ctx->err = text;               \
      return code;                   \
    }                                \
  } while (0)

// passes on the failure of a call that returns an hb status (its error text is already set)
#define HB_TRY(expr)                \
  do {                              \
    const int32_t rc_ = (expr);     \
    if (rc_ != HB_OK) return rc_;   \
  } while (0)

// Device scratch of one call of a unit-level entry point, freed on every return path.
template <class T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  // n elements, filled from the host array `from` when one is given
  hipError_t alloc(size_t n, const T* from = nullptr) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
    if (e == hipSuccess && from) e = hipMemcpy(p, from, n * sizeof(T), hipMemcpyHostToDevice);
    return e;
  }
};

template <class T>
static hipError_t dalloc(hb_ctx* ctx, T** p, size_t n) {
  hipError_t e = hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T));
  if (e == hipSuccess) {
    ctx->allocs.push_back(*p);
    e = hipMemset(*p, 0, n * sizeof(T));
    // the library's streams are non-blocking: without this, work queued on them right after a late allocation (reset mask,
    // joint-command state, LCM staging) could run BEFORE the zero fill on the null stream
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  }
  return e;
}

// Every array s describes (hb_layout.hpp), for the whole batch, zero-filled, in the order of the description; *failed names the array
// an allocation failed on.
template <class S>
static hipError_t alloc_fields(hb_ctx* ctx, S& s, const char** failed = nullptr) {
  hipError_t e = hipSuccess;
  fields(s, ctx->Nmax, [&](const char* name, auto*& p, Extent x) {
    if (e != hipSuccess) return;
    std::remove_const_t<std::remove_reference_t<decltype(*p)>>* q = nullptr;
    e = dalloc(ctx, &q, size_t(ctx->B) * x.n);
    p = q;
    if (e != hipSuccess && failed) *failed = name;
  });
  return e;
}

// Allocate on first use: the arrays of s are there once the LAST one of its description is (alloc_fields goes in that order), so an
// allocation that failed half way is repeated by the next call.  ensure_fields also sets s.B where s has one; *fresh: this call allocated.
template <class S>
static bool has_fields(const hb_ctx* ctx, const S& s) {
  S v = s;
  const void* last = nullptr;
  fields(v, ctx->Nmax, [&](const char*, auto*& p, Extent) { last = p; });
  return last != nullptr;
}
template <class S>
static auto set_batch_size(S& s, int B, int) -> decltype(void(s.B)) { s.B = B; }
template <class S>
static void set_batch_size(S&, int, long) {}
template <class S>
static int32_t ensure_fields(hb_ctx* ctx, S& s, bool* fresh = nullptr) {
  const bool need = !has_fields(ctx, s);
  if (fresh) *fresh = need;
  if (!need) return HB_OK;
  HB_HIP(alloc_fields(ctx, s));
  set_batch_size(s, ctx->B, 0);
  return HB_OK;
}

// Instances [i0, i0 + cnt) of the batch, cnt >= min_cnt, in a form that cannot overflow.
struct Range { int i0, cnt; };
static bool range_ok(const hb_ctx* ctx, int32_t i0, int32_t cnt, int32_t min_cnt) {
  return i0 >= 0 && cnt >= min_cnt && i0 <= ctx->B && cnt <= ctx->B - i0;
}
static Range whole(const hb_ctx* ctx) { return Range{0, ctx->B}; }

// Copy between the instances r of the array `field` of `batch` (one of its described arrays) and `other`, which starts at the first
// instance of r (device-to-device: at instance 0, it is laid out like the field).  On *s when a stream is given, blocking otherwise.
template <class S, class T>
static int32_t copy_field(hb_ctx* ctx, hipMemcpyKind kind, const void* other, S& batch, T* const& field, Range r, const hipStream_t* s) {
  const Extent e = extent_of(batch, ctx->Nmax, field);
  HB_FAIL_IF(e.n == 0 || e.step != e.n, HB_ERR_DEVICE, "internal: copy of an array its batch does not describe as instance-major");
  using V = std::remove_const_t<T>;
  V* dev = const_cast<V*>(field) + size_t(r.i0) * e.n;
  const size_t bytes = size_t(r.cnt) * e.n * sizeof(T);
  void* dst = dev;
  const void* src = other;
  if (kind == hipMemcpyDeviceToHost) { dst = const_cast<void*>(other); src = dev; }
  if (kind == hipMemcpyDeviceToDevice) src = static_cast<const T*>(other) + size_t(r.i0) * e.n;
  if (s) HB_HIP(hipMemcpyAsync(dst, src, bytes, kind, *s));
  else HB_HIP(hipMemcpy(dst, src, bytes, kind));
  return HB_OK;
}
// device -> host (pull) and host -> device (push) of a described array; a null host pointer is skipped
template <class S, class T>
static int32_t pull(hb_ctx* ctx, void* host, S& batch, T* const& field, Range r, const hipStream_t* s = nullptr) {
  return host ? copy_field(ctx, hipMemcpyDeviceToHost, host, batch, field, r, s) : HB_OK;
}
template <class S, class T>
static int32_t push(hb_ctx* ctx, const void* host, S& batch, T* const& field, Range r, const hipStream_t* s = nullptr) {
  return host ? copy_field(ctx, hipMemcpyHostToDevice, host, batch, field, r, s) : HB_OK;
}
// device -> host of a slot-major array [slots][batch.stride]: the rows of the instances r, slot by slot, transposed into host[cnt][slots]
template <class S, class T>
static int32_t pull_slot_major(hb_ctx* ctx, T* host, S& batch, T* const& field, Range r) {
  if (!host) return HB_OK;
  const size_t slots = extent_of(batch, ctx->Nmax, field).n, n = r.cnt;
  std::vector<T> tmp(slots * n);
  HB_HIP(hipMemcpy2D(tmp.data(), n * sizeof(T), field + r.i0, size_t(batch.stride) * sizeof(T), n * sizeof(T), slots, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i)
    for (size_t k = 0; k < slots; ++k) host[i * slots + k] = tmp[k * n + i];
  return HB_OK;
}
// elements of the whole batch's `field`
template <class S, class T>
static size_t field_count(hb_ctx* ctx, S& batch, T* const& field) { return size_t(ctx->B) * extent_of(batch, ctx->Nmax, field).n; }
// the whole batch's `field` back to zero: on *s when a stream is given, blocking otherwise
template <class S, class T>
static int32_t zero_field(hb_ctx* ctx, S& batch, T* const& field, const hipStream_t* s = nullptr) {
  const size_t bytes = field_count(ctx, batch, field) * sizeof(T);
  if (s) HB_HIP(hipMemsetAsync(field, 0, bytes, *s));
  else HB_HIP(hipMemset(field, 0, bytes));
  return HB_OK;
}

// Per-instance log [B][cap][W] of doubles whose extent is set at run time (episode trace, scenario log, profile-draw log: no description
// names them).  log_grow: (log, cap) to `want` rows where that is more; the allocation grows to the largest capacity asked for.
static int32_t log_grow(hb_ctx* ctx, double*& log, int& cap, int want, int W) {
  if (want <= cap) return HB_OK;
  if (log) {
    ctx->allocs.erase(std::remove(ctx->allocs.begin(), ctx->allocs.end(), static_cast<void*>(log)), ctx->allocs.end());
    HB_HIP(hipFree(log));
    log = nullptr;
    cap = 0;
  }
  HB_HIP(dalloc(ctx, &log, size_t(ctx->B) * want * W));
  cap = want;
  return HB_OK;
}
// log_zero: every row back to zero (no log: nothing), on *s when a stream is given, blocking otherwise
static int32_t log_zero(hb_ctx* ctx, double* log, int cap, int W, const hipStream_t* s = nullptr) {
  const size_t bytes = size_t(ctx->B) * cap * W * sizeof(double);
  if (log && s) HB_HIP(hipMemsetAsync(log, 0, bytes, *s));
  else if (log) HB_HIP(hipMemset(log, 0, bytes));
  return HB_OK;
}
// log_read: host[B][in_force][W] out of the device's [B][cap][W] (the device rows have the pitch of the largest capacity set so far, the
// caller's the pitch of the one in force); a null host pointer or in_force = 0 is skipped
static int32_t log_read(hb_ctx* ctx, double* host, const double* log, int cap, int in_force, int W) {
  const size_t row = size_t(in_force) * W * sizeof(double);
  if (host && row) HB_HIP(hipMemcpy2D(host, row, log, size_t(cap) * W * sizeof(double), row, size_t(ctx->B), hipMemcpyDeviceToHost));
  return HB_OK;
}

// The refusals that name their caller.  refuse_state: "who: why" (HB_ERR_STATE), nothing to refuse when why is null; refuse_config: a
// configuration's own refusal text (HB_ERR_ARG), likewise; refuse_instance: what instance i brings, with `code`.  `kept`: what stays in force.
static int32_t refuse_state(hb_ctx* ctx, const char* who, const char* why) {
  if (!why) return HB_OK;
  ctx->err = std::string(who) + ": " + why;
  return HB_ERR_STATE;
}
static int32_t refuse_config(hb_ctx* ctx, const char* who, const char* why) {
  if (!why) return HB_OK;
  ctx->err = std::string(who) + ": " + why + " (the configuration in force is kept)";
  return HB_ERR_ARG;
}
static int32_t refuse_instance(hb_ctx* ctx, int32_t code, const char* who, size_t i, const char* why, const char* kept) {
  ctx->err = std::string(who) + ": instance " + std::to_string(i) + " has " + why + " (the " + kept + " in force is kept)";
  return code;
}

// Upload of a caller-owned host array through pinned staging (see hb_ctx::stage): returns as soon as the bytes are in the slot.
// Each array id belongs to one side of the two-thread split (control side: time, sensors; MPC side: t0, cmd, x0; hb_tick_resident,
// which uses all of them, is a single-thread entry point), so a ring is only ever advanced by one thread.
enum StageId { ST_TNOW = 0, ST_QUAT, ST_W, ST_A, ST_QJ, ST_QDJ, ST_CONTACT, ST_T0, ST_CMD, ST_X0 };
template <class S, class T>
static int32_t stage_upload(hb_ctx* ctx, int id, S& batch, T* const& field, const void* src, hipStream_t s) {
  void* dst = const_cast<std::remove_const_t<T>*>(field);
  const size_t bytes = field_count(ctx, batch, field) * sizeof(T);
  hb_ctx::StageSlot& sl = ctx->stage[id][ctx->stage_turn[id]++ % hb_ctx::STAGE_DEPTH];
  if (sl.pending) { HB_HIP(hipEventSynchronize(sl.done)); sl.pending = false; }
  if (sl.cap < bytes) {
    if (sl.host) HB_HIP(hipHostFree(sl.host));
    sl.host = nullptr; sl.cap = 0;
    HB_HIP(hipHostMalloc(&sl.host, bytes, hipHostMallocDefault));
    sl.cap = bytes;
  }
  if (!sl.done) HB_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
  std::memcpy(sl.host, src, bytes);
  HB_HIP(hipMemcpyAsync(dst, sl.host, bytes, hipMemcpyHostToDevice, s));
  HB_HIP(hipEventRecord(sl.done, s));
  sl.pending = true;
  return HB_OK;
}

// The six sensor arrays of an estimator update (quaternion, angular velocity, linear acceleration, joint positions, joint
// velocities, contact flags: staging ids ST_QUAT .. ST_CONTACT) into the arrays of `batch` that dst[0..4] and `contact` name, on s;
// through pinned staging when `staged`.
template <class S, class T, class C>
static int32_t upload_sensors(hb_ctx* ctx, S& batch, T* const* const dst[5], C* const& contact, const void* const src[6], bool staged, hipStream_t s) {
  for (int k = 0; k < 5; ++k) {
    if (staged) HB_TRY(stage_upload(ctx, ST_QUAT + k, batch, *dst[k], src[k], s));
    else HB_TRY(push(ctx, src[k], batch, *dst[k], whole(ctx), &s));
  }
  if (staged) return stage_upload(ctx, ST_CONTACT, batch, contact, src[5], s);
  return push(ctx, src[5], batch, contact, whole(ctx), &s);
}

// Chunked hb_step_resident calls free-run: every chunk of instances is its own stream that goes from one step straight into the
// next (instances are independent), without a per-step join.  The join into the two library streams happens here, lazily, at
// the start of every OTHER entry point — the getters, the table updates, the joint command, hb_sync ... only know s_mpc / s_wbc —
// and the next chunked step then forks again from them.
static void lazy_join(hb_ctx* ctx) {
  if (ctx->chunks_pending == 0 && ctx->fork_needed) return;  // nothing in flight (always, without chunks): no state is touched
  for (int c = 0; c < ctx->chunks_pending; ++c) {
    (void)hipStreamWaitEvent(ctx->s_mpc, ctx->ev_sync[SYNC_JOIN + c], 0);
    (void)hipStreamWaitEvent(ctx->s_wbc, ctx->ev_sync[SYNC_JOIN + c], 0);
  }
  ctx->chunks_pending = 0;
  ctx->fork_needed = true;
}

// Enqueues a writer of the resident observation on s (launch()); with `fence`, between two ordering points: it starts after the work
// queued so far on the MPC stream, and the MPC stream's later work after it (the observation feeds the next solve there).
template <class F>
static int32_t resident_write(hb_ctx* ctx, hipStream_t s, bool fence, F&& launch) {
  if (fence) {
    HB_HIP(hipEventRecord(ctx->ev_sync[SYNC_BEFORE_WRITER], ctx->s_mpc));
    HB_HIP(hipStreamWaitEvent(s, ctx->ev_sync[SYNC_BEFORE_WRITER], 0));
  }
  launch();
  HB_HIP(hipGetLastError());
  if (fence) {
    HB_HIP(hipEventRecord(ctx->ev_sync[SYNC_AFTER_WRITER], s));
    HB_HIP(hipStreamWaitEvent(ctx->s_mpc, ctx->ev_sync[SYNC_AFTER_WRITER], 0));
  }
  return HB_OK;
}

// What every entry point does first: the context exists, the free-running instance ranges are joined into the library streams
// (lazy_join), no argument is bad (HB_ERR_ARG without an error text otherwise) — HB_ENTER_ARGS — and the context's device is current —
// HB_ENTER_DEVICE.  HB_ENTER is both; entries that report a state error before they touch the device put it between the halves.
#define HB_ENTER_ARGS(bad_args)             \
  do {                                      \
    if (!ctx) return HB_ERR_ARG;            \
    lazy_join(ctx);                         \
    if (bad_args) return HB_ERR_ARG;        \
  } while (0)
#define HB_ENTER_DEVICE() HB_HIP(hipSetDevice(ctx->device))
#define HB_ENTER(bad_args)   \
  do {                       \
    HB_ENTER_ARGS(bad_args); \
    HB_ENTER_DEVICE();      \
  } while (0)

extern "C" {

int32_t hb_version(void) { return 305; }

const char* hb_last_error(const hb_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int32_t hb_create(const hb_model* model, const hb_config* config, int32_t batch, int32_t max_nodes, int32_t device,
                  hb_ctx** out) {
  if (!model || !config || !out || batch <= 0 || max_nodes <= 0) {
    g_create_error = "hb_create: bad argument";
    return HB_ERR_ARG;
  }
  if (!topology_supported(*model)) {
    g_create_error = "hb_create: model topology is not base + two 5-joint legs";
    return HB_ERR_ARG;
  }
  // (the struct has grown over the rounds and carries no size field: a caller built against an older, smaller hb_config makes the library
  // read past its end — fields that gate loops are therefore range-checked, and the tail word must be the documented 0)
  if (config->wbc_reg_steps < 0 || config->wbc_reg_steps > HB_WBC_REG_STEPS_MAX || config->wbc_eps_mode < 0 || config->wbc_eps_mode > 1 || (config->wbc_eps_mode == 1 && config->wbc_type != 0) || config->wbc_max_iter <= 0 ||
      !(config->wbc_eps_reg > 0.0)) {
    g_create_error = "hb_create: hb_config.wbc_reg_steps outside [0, 8], wbc_eps_mode not 0 / 1 (1: WeightedWbc only), wbc_max_iter <= 0 or wbc_eps_reg <= 0 (struct built against another header?)";
    return HB_ERR_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device >= ndev) {
    g_create_error = "hb_create: no HIP device visible (the solver has no CPU fallback)";
    return HB_ERR_NO_GPU;
  }
  hb_ctx* ctx = new hb_ctx();
  ctx->device = device;
  ctx->B = batch;
  ctx->Nmax = max_nodes;
  ctx->model = *model;
  ctx->config = *config;
  ctx->hmodel = make_dev_model(*model);
  ctx->hconfig = make_dev_config(*config, ctx->hmodel);
  ctx->forms = decode_forms(config->reserved, HB_ABLATE_ON);

  auto fail = [&](const char* what, hipError_t e) {
    g_create_error = std::string("hb_create: ") + what + ": " + hipGetErrorString(e);
    for (void* p : ctx->allocs) (void)hipFree(p);
    delete ctx;
    return HB_ERR_DEVICE;
  };
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) return fail("hipSetDevice", e);
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) ctx->n_cu = ncu;
  }
  if ((e = hipStreamCreateWithFlags(&ctx->s_mpc, hipStreamNonBlocking)) != hipSuccess) return fail("stream", e);
  if ((e = hipStreamCreateWithFlags(&ctx->s_wbc, hipStreamNonBlocking)) != hipSuccess) return fail("stream", e);
  for (auto& ev : ctx->ev)
    if ((e = hipEventCreate(&ev)) != hipSuccess) return fail("event", e);
  for (auto& ev : ctx->ev_sync)
    if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return fail("event", e);
  for (auto& sc : ctx->s_chunk)
    if ((e = hipStreamCreateWithFlags(&sc, hipStreamNonBlocking)) != hipSuccess) return fail("chunk stream", e);
  const size_t B = batch;
  Batch& b = ctx->b;
  b.B = batch;
  b.Nmax = max_nodes;
  WbcBatch& w = ctx->w;
  w.B = batch;
  const char* what = "ctx->dmodel";
  if ((e = dalloc(ctx, &ctx->dmodel, 1)) != hipSuccess) return fail(what, e);
  if ((e = dalloc(ctx, &ctx->dconfig, 1)) != hipSuccess) return fail("ctx->dconfig", e);
  if ((e = alloc_fields(ctx, b, &what)) != hipSuccess || (e = alloc_fields(ctx, w, &what)) != hipSuccess ||
      (e = alloc_fields(ctx, ctx->lslist, &what)) != hipSuccess)
    return fail(what, e);
  if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_hwbc), hipFuncAttributeMaxDynamicSharedMemorySize,
                               int(HoLdsDev::total * sizeof(double)))) != hipSuccess)
    return fail("k_hwbc LDS size", e);
  if ((e = hipMemcpy(ctx->dmodel, &ctx->hmodel, sizeof(DevModel), hipMemcpyHostToDevice)) != hipSuccess) return fail("model", e);
  if ((e = hipMemcpy(ctx->dconfig, &ctx->hconfig, sizeof(DevConfig), hipMemcpyHostToDevice)) != hipSuccess) return fail("config", e);
  // walking by default
  std::vector<int> ones(B, 1);
  if ((e = hipMemcpy(w.walk, ones.data(), ones.size() * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess) return fail("walk", e);
  *out = ctx;
  return HB_OK;
}

void hb_destroy(hb_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  for (void* p : ctx->allocs) (void)hipFree(p);
  for (auto& ev : ctx->ev) (void)hipEventDestroy(ev);
  for (auto& ev : ctx->ev_sync) (void)hipEventDestroy(ev);
  if (ctx->s_up) (void)hipStreamDestroy(ctx->s_up);
  if (ctx->ev_up) (void)hipEventDestroy(ctx->ev_up);
  for (auto& ev : ctx->ev_consumed)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& arr : ctx->stage)
    for (auto& sl : arr) {
      if (sl.done) (void)hipEventDestroy(sl.done);
      if (sl.host) (void)hipHostFree(sl.host);
    }
  (void)hipStreamDestroy(ctx->s_mpc);
  (void)hipStreamDestroy(ctx->s_wbc);
  for (auto& row : ctx->chunk_graph)
    for (auto& g : row)
      if (g) (void)hipGraphExecDestroy(g);
  for (auto& sc : ctx->s_chunk) (void)hipStreamDestroy(sc);
  delete ctx;
}


int32_t hb_sync(hb_ctx* ctx) {
  HB_ENTER_ARGS(false);
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  for (auto& sc : ctx->s_chunk) HB_HIP(hipStreamSynchronize(sc));
  if (ctx->s_up) HB_HIP(hipStreamSynchronize(ctx->s_up));
  return HB_OK;
}

int32_t hb_get_input_cost(const hb_ctx* ctx, double* R) {
  if (!ctx || !R) return HB_ERR_ARG;
  std::memset(R, 0, sizeof(double) * HB_NU * HB_NU);
  for (int i = 0; i < 12; ++i) R[i * HB_NU + i] = ctx->hconfig.R_FF_diag[i];
  for (int a = 0; a < HB_NJ; ++a)
    for (int c = 0; c < HB_NJ; ++c) R[(12 + a) * HB_NU + 12 + c] = ctx->hconfig.R_jj[a * HB_NJ + c];
  return HB_OK;
}

int32_t hb_get_stats(hb_ctx* ctx, hb_stats* out) {
  HB_ENTER(!out);
  HB_HIP(hipStreamSynchronize(ctx->s_mpc));
  HB_HIP(hipStreamSynchronize(ctx->s_wbc));
  float ms = 0;
  if (ctx->timed) {
    if (hipEventElapsedTime(&ms, ctx->ev[EV_LQ_BEGIN], ctx->ev[EV_LQ_END]) == hipSuccess) ctx->stats.ms_lq = ms;
    if (hipEventElapsedTime(&ms, ctx->ev[EV_LQ_END], ctx->ev[EV_RIC_BWD_END]) == hipSuccess) ctx->stats.ms_riccati_bwd = ms;
    if (hipEventElapsedTime(&ms, ctx->ev[EV_RIC_BWD_END], ctx->ev[EV_RIC_FWD_END]) == hipSuccess) ctx->stats.ms_riccati_fwd = ms;
    if (hipEventElapsedTime(&ms, ctx->ev[EV_RIC_FWD_END], ctx->ev[EV_LS_END]) == hipSuccess) ctx->stats.ms_linesearch = ms;
    if (hipEventElapsedTime(&ms, ctx->ev[EV_LQ_BEGIN], ctx->ev[EV_LS_END]) == hipSuccess) ctx->stats.ms_mpc_total = ms;
  }
  if (ctx->stats.n_wbc_solves > 0 && hipEventElapsedTime(&ms, ctx->ev[EV_WBC_BEGIN], ctx->ev[EV_WBC_END]) == hipSuccess) ctx->stats.ms_wbc = ms;
  if (ctx->stats.n_wbc_solves > 0) {
    std::vector<int> st(ctx->B);
    HB_TRY(pull(ctx, st.data(), ctx->w, ctx->w.status, whole(ctx)));
    for (int& v : ctx->stats.n_status) v = 0;
    for (int v : st)
      if (v >= 0 && v < 4) ctx->stats.n_status[v]++;
  }
  *out = ctx->stats;
  return HB_OK;
}

}  // extern "C"
