/*
 * hunter_hip.h — C ABI of the MI355X-native batched NMPC + WBC solver for the EC-hunter80 biped.
 *
 * This is the drop-in boundary for the hot path of bridgedp/hunter_bipedal_control.
 * Every entry point names the reference interface it replaces (paths relative to the reference root).
 * Plain pointers and sizes only; no C++/torch types.  All functions return 0 on success and a
 * negative hb_status on failure (never throw); hb_last_error() gives the message.
 *
 * Conventions
 *   MPC state  x[22] = [h_lin/m (3), h_ang/m (3), base pos (3), base ZYX euler (3), joints l1..l5 r1..r5 (10)]
 *   MPC input  u[22] = [F(L_f1) F(R_f1) F(L_f2) F(R_f2) (world frame, 12), joint velocities (10)]
 *   rbd state  [32]  = [zyx(3), pos(3), q_j(10), omega_world(3), v_lin(3), qd_j(10)]
 *                      (legged_estimation/src/StateEstimateBase.cpp:73-106)
 *   WBC output [38]  = [qdd(16) | F(12) | tau(10)]            (legged_wbc/src/WbcBase.cpp:40)
 *   modes: 0 FLY, 1 R (feet 1,3 closed), 2 L (feet 0,2 closed), 3 STANCE
 *                      (legged_interface/include/legged_interface/gait/MotionPhaseDefinition.h:55-95)
 *   All matrices passed through this ABI are row-major doubles.
 *
 * Batch layout: instance-major.  Host buffers are caller-owned; device buffers are library-owned.
 * One hb_ctx drives one GPU (one process per GPU; ranks shard the batch).
 */
#ifndef HUNTER_HIP_H
#define HUNTER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HB_NX 22
#define HB_NU 22
#define HB_NV 16   /* generalized coordinates: base pos(3) + zyx(3) + joints(10) */
#define HB_NJ 10
#define HB_NC 4    /* 3-DoF point contacts */
#define HB_NBODY 11 /* base + 10 links (fixed URDF children merged into their parent) */
#define HB_NWBC 38
#define HB_NRBD 32
#define HB_SWING_REF 6 /* per foot and node: pos xyz, vel xyz of the swing reference */

typedef enum hb_status {
  HB_OK = 0,
  HB_ERR_ARG = -1,       /* bad argument (null pointer, range) */
  HB_ERR_DEVICE = -2,    /* HIP runtime error */
  HB_ERR_STATE = -3,     /* call order (e.g. solve before references were set) */
  HB_ERR_NO_GPU = -4     /* no gfx950 device visible: the product path never falls back to a CPU */
} hb_status;
/* An instance range [inst_begin, inst_begin + inst_count) that leaves the batch is HB_ERR_ARG in every entry, also where the sum overflows int32. */

/* Per-instance solver status words written by the device (SURVEY.md §5 "failure detection"). */
#define HB_INST_OK 0
#define HB_INST_MAXITER 1   /* WBC QP hit its working-set-change limit: previous solution reused
                               (legged_wbc/src/WeightedWbc.cpp:57-65); MPC: the line search reached alpha_min without
                               an acceptable step (a search that stops on deltaTol — converged — is HB_INST_OK) */
#define HB_INST_INFEASIBLE 2
#define HB_INST_NAN 3       /* non-finite value / non-positive Riccati pivot */

/* Rigid-body model, replaces PinocchioInterface built from the URDF
 * (legged_interface/src/LeggedInterface.cpp:188-200).  Body 0 is base_link, bodies 1..5 the left leg
 * links, 6..10 the right leg links; joint j connects body parent[j] to body j+1. */
typedef struct hb_model {
  int32_t parent[HB_NJ];
  double joint_origin[HB_NJ][3];   /* joint frame origin in the parent body frame (all URDF rpy are 0) */
  double joint_axis[HB_NJ][3];
  double q_lower[HB_NJ], q_upper[HB_NJ], qd_limit[HB_NJ], effort[HB_NJ];
  double mass[HB_NBODY];
  double com[HB_NBODY][3];         /* body frame */
  double inertia[HB_NBODY][6];     /* about the body COM, body axes: xx xy xz yy yz zz */
  int32_t contact_body[HB_NC];     /* order L_f1, R_f1, L_f2, R_f2 (ModelSettings.h:62) */
  double contact_offset[HB_NC][3];
  double gravity;                  /* 9.81 (legged_interface/include/legged_interface/common/utils.h:82) */
} hb_model;

/* Flattened task.info / reference.info (legged_controllers/config/hunter). */
typedef struct hb_config {
  /* sqp block, task.info:79-96 */
  double dt;
  int32_t sqp_iterations;
  int32_t wbc_type;                /* 0 WeightedWbc (LeggedController.cpp:85), 1 HierarchicalWbc */
  double g_max, g_min;             /* filter line search thresholds */
  double alpha_decay, alpha_min, gamma_c, armijo_factor; /* OCS2 FilterLinesearch defaults 0.5 1e-4 1e-6 1e-4.  Any decay in (0, 1): the
                                      backtracking step sizes decay^k >= alpha_min are evaluated 16 at a time, window after window */
  /* cost, task.info:186-253 + LeggedInterface.cpp:263-312 */
  double Q_diag[HB_NX];
  double R_task_diag[24];          /* 12 contact-force weights, 12 foot-velocity (task space) weights */
  double initial_state[HB_NX];     /* configuration at which the task-space R is pulled back to joint space */
  /* soft constraints */
  double friction_mu, friction_reg, friction_gripper, friction_hess_shift; /* FrictionConeConstraint.h:77-83 */
  double friction_barrier_mu, friction_barrier_delta;                      /* task.info:255-262 */
  double soft_swing_weight;        /* task.info:265-268 */
  double pos_limit_barrier[2], vel_limit_barrier[2], force_limit_barrier[2]; /* (mu,delta) LeggedInterface.cpp:337-339 */
  double force_limit[2];           /* [0,350] LeggedInterface.cpp:352 */
  /* equality constraints */
  double position_error_gain;      /* swing normal-velocity constraint, task.info:10 */
  double zero_vel_z_gain, zero_vel_z_offset; /* Ax(2,2)=3, b(2)=-0.06, LeggedInterface.cpp:436-444 */
  double xy_ref_gain;              /* 3, LeggedRobotPreComputation.cpp:113-116 */
  /* WBC, task.info:289-333 */
  double torque_limits[5];
  double wbc_friction_mu;
  double swing_kp, swing_kd, base_height_kp, base_height_kd, base_angular_kp, base_angular_kd;
  double weight_swing_leg, weight_base_accel, weight_contact_force;
  double wbc_eps_reg;              /* Tikhonov term of the regularised-minimiser rule */
  int32_t wbc_max_iter;            /* working-set-change limit; reference nWSR = 20 (WeightedWbc.cpp:50) */
  int32_t reserved;                /* 0.  Tests, tuning and the profiling build only: the values read are named once, in csrc/hb_forms.hpp */
  double default_joint_state[HB_NJ]; /* reference.info:7-19 */
  double delta_tol;                /* sqp.deltaTol, task.info:84: the line search gives up (no step, as at alpha_min) once
                                      alpha |dx| and alpha |du| — l2 norms over the whole trajectory — are both below it
                                      ([OCS2-knowledge] SqpSolver::takeStep "escape early"); 0 disables */
  int32_t wbc_reg_steps;           /* regularisation steps after the eps-regularised WBC solve: qpOASES Options::setToMPC() leaves
                                      numRegularisationSteps = 1 (WeightedWbc.cpp:47-48, HoQp.cpp:175-176 [qpOASES-knowledge]).  Each step is
                                      one proximal-point step x <- argmin f(x) + eps/2 |x - x_prev|^2 on the final working set; 1 removes
                                      the first-order-in-eps bias of the regularised minimiser.  0 = plain Tikhonov point */
  int32_t wbc_eps_mode;            /* 0: the Tikhonov term is wbc_eps_reg for every problem (default).  1 (WeightedWbc only): per problem,
                                      eps = |H|_F * 1e3 * DBL_EPSILON with H = A_w' A_w — what qpOASES 3.2's regulariseHessian adds to the
                                      diagonal (epsRegularisation = 1e3 EPS, Options::setToMPC; [qpOASES-knowledge]); wbc_eps_reg
                                      is then unused.  Other values and mode 1 with wbc_type = 1 are rejected by hb_create */
} hb_config;
#define HB_WBC_REG_STEPS_MAX 8     /* hb_create rejects wbc_reg_steps outside [0, HB_WBC_REG_STEPS_MAX] */

typedef struct hb_ctx hb_ctx;

/* Aggregate per-phase device time of the last hb_mpc_solve / hb_wbc_update (HIP events on the
 * library's own streams), replacing the reference's mpcTimer_/wbcTimer_ (LeggedController.cpp:359-366). */
typedef struct hb_stats {
  double ms_lq, ms_riccati_bwd, ms_riccati_fwd, ms_linesearch, ms_mpc_total;
  double ms_wbc;
  int64_t n_mpc_solves, n_wbc_solves;
  int32_t n_status[4];             /* histogram of the last WBC status words */
} hb_stats;

/* ---- lifetime -------------------------------------------------------------------------------
 * Replaces LeggedController::init -> setupLeggedInterface/setupMpc/setupMrt + WeightedWbc ctor +
 * loadTasksSetting (LeggedController.cpp:41-88,376-431).  `batch` robot instances live on HIP
 * device `device`; every instance has at most `max_nodes` shooting intervals. */
int32_t hb_create(const hb_model* model, const hb_config* config, int32_t batch, int32_t max_nodes,
                  int32_t device, hb_ctx** out);
void hb_destroy(hb_ctx* ctx);
/* Message of the last call that FAILED ON THE CALLING THREAD (errno-like, thread-local): the reference drives one solver from
 * two threads (control thread: hb_wbc_update / hb_joint_command / estimator; MPC thread: hb_refgen_update / hb_mpc_solve /
 * hb_mpc_publish — LeggedController.cpp:396-421), which this library supports for exactly that split. */
const char* hb_last_error(const hb_ctx* ctx); /* ctx may be NULL: message of the failed hb_create */

/* ---- references ------------------------------------------------------------------------------
 * Node tables produced by the reference manager before each solve, replacing what
 * SwitchedModelReferenceManager::modifyReferences (SwitchedModelReferenceManager.cpp:136-171) and the
 * OCS2 time discretisation hand to the SQP solver:
 *   n_nodes[i]            number of shooting intervals N_i <= max_nodes
 *   t[i][k], k<=N_i       node times (event times are grid nodes; interval k uses mode[i][k])
 *   mode[i][k], k<N_i     contact mode of interval k (ModeSchedule::modeAtTime just after t_k)
 *   x_ref[i][k][22]       TargetTrajectories::getDesiredState(t_k)
 *   swing_ref[i][k][4][6] SwingTrajectoryPlanner::get{X,Y,Z}{position,velocity}Constraint(foot, t_k)
 * Host arrays are strided by max_nodes(+1) as declared in hb_create. */
int32_t hb_mpc_set_references(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, const int32_t* n_nodes,
                              const double* t, const int32_t* mode, const double* x_ref,
                              const double* swing_ref);

/* Cold start: x_k = x0, u_k = weight compensation of mode_k (LeggedRobotInitializer.cpp:67-77). */
int32_t hb_mpc_reset(hb_ctx* ctx, const double* x0 /*[batch][22], or NULL: the device-resident observation*/);
/* Cold start of the instances with mask[i] != 0 only — the per-instance form of LeggedController::resetMPC / resetMpcNode
 * (LeggedController.cpp:460-465), e.g. after hb_mpc_get_status reported HB_INST_NAN for them.  x0 may be NULL (the
 * device-resident observation); otherwise only the masked rows of x0 [batch][22] are read. */
int32_t hb_mpc_reset_masked(hb_ctx* ctx, const uint8_t* mask /*[batch]*/, const double* x0);
/* Per-instance status word of the last MPC call (hb_inst_status): HB_INST_NAN = non-positive Riccati pivot or a non-finite
 * value (the step was not taken, the iterate is the previous one: the batch counterpart of the exception path of the MPC
 * thread, LeggedController.cpp:413-418), HB_INST_MAXITER = the filter line search rejected every step size. */
int32_t hb_mpc_get_status(hb_ctx* ctx, int32_t* status /*[batch]*/);
/* Warm start from caller-provided trajectories (x [batch][max_nodes+1][22], u [batch][max_nodes][22]) on the CURRENT tables.
 * Between MPC calls the library warm-starts by itself: when the node tables changed (hb_mpc_set_references /
 * hb_refgen_update) the next hb_mpc_solve first interpolates the previous iterate onto the new node times and falls back to
 * the initializer beyond the previous horizon (OCS2 SqpSolver::initializeStateInputTrajectories). */
int32_t hb_mpc_set_trajectory(hb_ctx* ctx, const double* x, const double* u);

/* ---- MPC -------------------------------------------------------------------------------------
 * One MPC call = config.sqp_iterations SQP iterations (LQ approximation, constraint projection,
 * backward/forward Riccati, filter line search) for every instance, from measured state x0.
 * Replaces MPC_MRT_Interface::advanceMpc -> SqpSolver::runImpl (LeggedController.cpp:406).
 * Asynchronous on the library's MPC stream. x0 is a host pointer [batch][22] or NULL to keep the
 * device-resident x0 (previous call). */
int32_t hb_mpc_solve(hb_ctx* ctx, const double* x0);
/* Make the last solution the active policy (MPC_MRT_Interface::updatePolicy, LeggedController.cpp:154).  Enqueue-only: five
 * device-to-device copies on the MPC stream, which the WBC stream then waits for.  Real-time note for the two-thread split: called
 * while the solve is still in flight, the copies — and with them the control thread's next hb_wbc_update — queue behind the whole
 * solve.  A caller whose control tick must never wait for the solver publishes AFTER the solve has completed: hb_mpc_solve,
 * hb_mpc_get_status (synchronises the MPC stream), hb_mpc_publish, all on the MPC thread (hunter_hip.hpp MpcMrtInterface::advanceMpc
 * does exactly that); the control thread keeps evaluating the previous policy until then, as the reference does. */
int32_t hb_mpc_publish(hb_ctx* ctx);
/* Copy trajectories to the host (PrimalSolution, LeggedController.cpp:269); any pointer may be NULL.
 * x [count][max_nodes+1][22], u [count][max_nodes][22]. Synchronises the MPC stream. */
int32_t hb_mpc_get_solution(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, double* x, double* u);
/* Per-instance performance index of the accepted step: [merit, dynamics SSE, equality SSE, step size]. */
int32_t hb_mpc_get_performance(hb_ctx* ctx, double* perf /*[batch][4]*/);

/* ---- WBC -------------------------------------------------------------------------------------
 * Evaluates the published policy at t_now (MPC_MRT_Interface::evaluatePolicy, LeggedController.cpp:155)
 * unless walk_flag[i]==0, in which case the stand-still target of LeggedController.cpp:161-173 is used;
 * then runs WbcBase::update + WeightedWbc::update (legged_wbc/src/WeightedWbc.cpp:18-66) or
 * HierarchicalWbc::update (legged_wbc/src/HierarchicalWbc.cpp:18-30) for every instance.
 * Host in: t_now[batch], rbd[batch][32] (both NULL: the device-resident time / rbd), walk_flag[batch] (NULL = all
 * walking).
 * Host out (any may be NULL): sol[batch][38], x_des[batch][22], u_des[batch][22], planned_mode[batch],
 * status[batch].  Synchronous with respect to the WBC stream when an output pointer is given. */
int32_t hb_wbc_update(hb_ctx* ctx, const double* t_now, const double* rbd, const int32_t* walk_flag,
                      double dt, double* sol, double* x_des, double* u_des, int32_t* planned_mode,
                      int32_t* status);
/* Direct form of WbcBase::update(stateDesired, inputDesired, rbdStateMeasured, mode, period)
 * (legged_wbc/include/legged_wbc/WbcBase.h:43-44), batched; host pointers. */
int32_t hb_wbc_update_direct(hb_ctx* ctx, const double* x_des, const double* u_des, const double* rbd,
                             const int32_t* mode, const int32_t* stance_flag, double dt, double* sol,
                             int32_t* status);

/* ---- joint command law ------------------------------------------------------------------------
 * The per-joint command of LeggedController::update after the WBC (LeggedController.cpp:186-257, the
 * loadControllerFlag_ branch), evaluated on the results of the last hb_wbc_update / hb_wbc_update_direct /
 * hb_step_resident that are still on the device:
 *   posDes = joints(optimizedState) + 0.5 qdd_wbc dt^2,  velDes = jointVel(optimizedInput) + qdd_wbc dt   (:186-191)
 *   (kp, kd) by joint: hip roll / yaw (0,1,5,6) small gains, ankle (4,9) small kp with kd_feet, others big gains;
 *   stance or swing kp by the planned contact flag of the leg (:223-245);  feed-forward = WBC torque
 *   torque = ff + kp (posDes - q) + kd (velDes - qd)                                                       (:252-256)
 * Limit protection (:196-208): a measured joint position (rbd) more than 0.02 rad outside the urdf limits latches the
 * instance's emergency stop — only while its controller is loaded — and from that joint on, and on every later call, the
 * command is setCommand(0, 0, 0, 1, 0) (:245-248).  Unloaded controller (:209-221): MPC joint targets with kp_position /
 * kd_position (kd_feet on the ankle joints 4, 9), no feed-forward.
 * Outputs (any may be NULL) are [batch][10]. Gains default to legged_controllers/cfg/Tutorials.cfg:6-16. */
typedef struct hb_joint_gains {
  double kp_big_stance, kp_big_swing, kd_big, kp_small_stance, kp_small_swing, kd_small, kd_feet;
  double kp_position, kd_position;   /* unloaded-controller branch (Tutorials.cfg:6-7) */
} hb_joint_gains;
/* Per-instance controller flags of the joint command law, device-resident: loadControllerFlag_ (default 1 = loaded; the
 * reference starts at 0 until /load_controller, LeggedController.cpp:489-493) and the emergency-stop latch
 * (emergencyStopFlag_, also set by the /emergency_stop topic, :477-481).  Either array may be NULL (left as is). */
int32_t hb_joint_set_flags(hb_ctx* ctx, const int32_t* controller_loaded /*[batch]*/, const int32_t* emergency_stop /*[batch]*/);
int32_t hb_joint_get_emergency_stop(hb_ctx* ctx, int32_t* emergency_stop /*[batch]*/);
int32_t hb_joint_command(hb_ctx* ctx, const hb_joint_gains* gains, double dt, double* pos_des, double* vel_des,
                         double* kp, double* kd, double* tau_ff, double* torque);

/* ---- plant stub for closed-loop rollouts ---------------------------------------------------
 * The reference closes its loop through Gazebo / MuJoCo (legged_gazebo/src/LeggedHWSim.cpp:166-192,
 * mujoco/src/main.cc:247).  This stub integrates M(q) vdot + nle = S' tau + Jc' lambda with the contact points of the
 * commanded mode pinned by acceleration-level constraints (Baumgarte gain `baumgarte`, damped normal equations with
 * relative damping `eps`), semi-implicit Euler; it does NOT enforce unilateral contact or friction limits (contact model 1 below does).
 * Coordinates: q = [pos, zyx, joints], v = [v_lin (world), ZYX rates, joint rates]. */
int32_t hb_plant_reset(hb_ctx* ctx, const double* q0 /*[batch][16]*/, const double* v0 /*[batch][16] or NULL*/,
                       double baumgarte, double eps);
/* Advance every instance by dt in `substeps` substeps.  tau[batch][10] / contact[batch][4] may be NULL: the torque of the
 * last hb_joint_command and the planned contact flags of the last WBC call, still on the device, are used.
 * to_resident != 0 repacks the new state as rbd + MPC observation into the resident inputs and advances the resident time
 * by dt, so that hb_refgen_update(x_now = NULL), hb_mpc_solve(NULL), hb_wbc_update(t_now = NULL, rbd = NULL),
 * hb_joint_command and hb_plant_step(NULL, NULL) close the loop without a host round trip. */
int32_t hb_plant_step(hb_ctx* ctx, const double* tau, const int32_t* contact, double dt, int32_t substeps,
                      int32_t to_resident);
/* State to the host (any may be NULL): q[batch][16], v[batch][16], rbd[batch][32], lambda[batch][12] (last contact
 * forces), vdot[batch][16] (last acceleration); lambda and vdot are zero between hb_plant_reset and the first step. */
int32_t hb_plant_get_state(hb_ctx* ctx, double* q, double* v, double* rbd, double* lambda, double* vdot);

/* ---- contact model of the plant: 0 = the pinned stub above (default), 1 = "ground" ------------------------------------------------
 * Model 1 has a flat ground z = ground_z, unilateral normal forces and Coulomb friction at the model's four contact points; contact is
 * decided by geometry, not by the schedule.  Per substep of length h = dt / substeps, with q, v in the plant's coordinates, all four
 * contact points always in the problem, world axes with z up:
 *  1. Rigid-body terms as in the pinned stub: M, nle, the UNMASKED 12 x 16 contact Jacobian J (rows 3c .. 3c+2 = x, y, z of point c) and
 *     the contact point positions; the gap is phi_c = z_c - ground_z.
 *  2. Free velocity v_f = v + h M^-1 (S' tau - nle + w), w = generalised force of the optional external base wrench: rows 0..2 = world
 *     force at the base origin, rows 3..5 = E(zyx)' (world moment), zero elsewhere (E: world angular velocity = E ZYX rates).
 *  3. W = J M^-1 J' + eps tr(J M^-1 J') I with eps of hb_plant_reset;  c = J v_f + b, b = 0 on tangential rows and
 *     (max(phi_c, 0) + erp min(phi_c, 0)) / h on normal rows.
 *  4. Impulses p[12], warm-started from the previous substep (zero after hb_plant_reset), by `sweeps` sweeps of projected Gauss-Seidel
 *     over the points 0, 1, 2, 3.  Within a point, with g = W p + c kept current after every change of an entry of p:
 *       normal first:     p_n <- max(0, p_n - g_n / W_nn);
 *       tangential pair:  t_a = p_a - g_a / W_aa for a = x, y (both g_a read before either entry changes); if |t| > mu p_n then
 *                         t <- t (mu p_n / |t|), zero if p_n = 0;  p_x, p_y <- t.
 *     The residual of the last sweep is max |W_ii dp_i| over its twelve updates [m/s].
 *  5. v+ = v_f + M^-1 J' p,  q+ = q + h v+.
 *  6. Outputs of a step: lambda = p / h (world forces, last substep); vdot = (v+ - v) / h (last substep: what the accelerometer of
 *     hb_plant_sense sees, impacts included); the last substep's residual; touching_c = (p_n > 0); the world velocity J v+ of every
 *     point (J of the last substep) and the gap of every point at the new q.
 * The contact flags given to hb_plant_step (host array or planned mode) play no part in the dynamics of model 1; they are still
 * recorded and handed to the estimator by hb_plant_sense as the commanded flags, which is what the reference feeds its filter
 * (LeggedController.cpp:224, 329: updateContact(cmdContactFlag)).
 * Status word per instance: HB_CONTACT_NONFINITE = non-finite state; HB_CONTACT_FALLEN = base z - ground_z < fall_height (latched until
 * hb_plant_reset; the instance goes on integrating); HB_CONTACT_UNCONVERGED = residual of the last substep > tol.
 * The model and the wrench survive hb_plant_reset, which clears impulses, outputs and status.  After a NULL model (or with the model
 * never set) hb_plant_step launches the pinned stub's kernel exactly as before; going back from model 1 to model 0 without a
 * hb_plant_reset un-pins every point, so the stub's next step anchors each commanded contact where the foot is then. */
#define HB_CONTACT_NONFINITE 1
#define HB_CONTACT_FALLEN 2
#define HB_CONTACT_UNCONVERGED 4
typedef struct hb_contact_config {
  int32_t mode;        /* 0: pinned stub (default); 1: ground */
  int32_t sweeps;      /* 1 .. 10000 */
  double mu;           /* Coulomb friction coefficient, >= 0 */
  double ground_z;     /* height of the plane */
  double erp;          /* share of a penetration removed per substep, [0, 1] */
  double tol;          /* m/s, >= 0: residual above which HB_CONTACT_UNCONVERGED is raised */
  double fall_height;  /* >= 0; 0: no fall detection */
  int32_t reserved[2]; /* 0 */
} hb_contact_config;
/* cfg NULL = model 0 (with mode 0 the other fields but `reserved` are ignored).  HB_ERR_STATE before hb_plant_reset; HB_ERR_ARG for a
 * non-finite or out-of-range field or a nonzero `reserved` (the model in force is kept). */
int32_t hb_plant_set_contact_model(hb_ctx* ctx, const hb_contact_config* cfg);
/* wrench[batch][6] = world force, world moment at the base origin, applied by every later step of model 1; NULL clears it.
 * HB_ERR_STATE before hb_plant_reset or in model 0. */
int32_t hb_plant_set_external_wrench(hb_ctx* ctx, const double* wrench);
/* Contact outputs of the last step of model 1 (any may be NULL; zero between hb_plant_reset and the first step): gap[batch][4],
 * point_vel[batch][12], residual[batch], touching[batch][4], status[batch].  HB_ERR_STATE before hb_plant_reset or in model 0. */
int32_t hb_plant_get_contact(hb_ctx* ctx, double* gap, double* point_vel, double* residual, int32_t* touching, int32_t* status);

/* ---- joint model of contact model 1: rotor inertia, viscous damping, dry friction, joint stops, torque saturation ------------------
 * One context-wide setting, off by default.  The reference's MuJoCo model gives every leg joint armature 0.1 and damping 1
 * (mujoco/model/hunter/hunter.xml:6), frictionloss 0.2 and a range (:59-124) and every motor ctrlrange +-100 (:25).  With a model in
 * force the steps 1 - 6 of contact model 1 above become, per substep of length h:
 *  1. Mh = M + diag(0_6, armature + h damping).  Every M^-1 of model 1 becomes Mh^-1.
 *  2. tau_a = clamp(tau, -torque_limit, +torque_limit);  v_f = v + h Mh^-1 (S' tau_a - nle - damping o v_joint + w).  With step 1 this
 *     is backward Euler in the damping term.
 *  3. 32 rows: 0-11 the contact rows as above; row 12 + j the friction row of joint j, Jacobian row e_{6+j}; row 22 + j the stop of joint
 *     j, Jacobian row s_j e_{6+j}, with s_j = +1, phi_j = q_j - lower_j if q_j - lower_j <= upper_j - q_j at the start of the substep,
 *     otherwise s_j = -1, phi_j = upper_j - q_j.  W = Jh Mh^-1 Jh'; the twelve contact diagonals get eps tr(contact block) as above,
 *     joint rows get no regularisation (their diagonal (Mh^-1)_jj is positive).  c = Jh v_f + b with, on stop rows,
 *     b = (max(phi, 0) + limit_erp min(phi, 0)) / h and b = 0 on friction rows.
 *  4. A sweep does the four contact points as above, then the friction rows j = 0..9: p <- clamp(p - g / W_rr, -frictionloss_j h,
 *     +frictionloss_j h), then (if `limits`) the stop rows j = 0..9: p <- max(0, p - g / W_rr); g = W p + c is kept current after every
 *     change.  Warm start of a friction row: the previous substep's p.  Of a stop row: the stored value is u_j = s_j p_j, signed in joint
 *     coordinates, and the substep starts from p_j = max(0, s_j u_j), so a change of side starts from zero.  Both are zero after
 *     hb_plant_reset.  The residual of hb_plant_get_contact keeps its meaning (the twelve contact updates, m/s); the joint residual is
 *     max |W_rr dp_r| over the joint updates of the last sweep [rad/s].
 *  5. v+ = v_f + Mh^-1 Jh' p,  q+ = q + h v+.
 *  6. Outputs per instance (hb_plant_get_joints): tau_applied[10] = tau_a; friction_torque[10] = p / h; limit_torque[10] = u / h (joint
 *     coordinates: >= 0 at a lower stop, <= 0 at an upper one); the joint residual; a status word: bit j = the stop impulse of joint j in
 *     the last substep is > 0, bit 10 + j = tau_a[j] != tau[j], HB_JOINT_UNCONVERGED = joint residual > tol.  The joint_torque of
 *     hb_plant_sense becomes tau_a, the torque the step integrated.
 * hb_plant_step holds the commanded torque over the tick; hb_plant_step_hybrid (below) evaluates the hybrid command's law per substep,
 * as the reference's simulator does per simulator step (mujoco/src/main.cc:243-249). */
#define HB_JOINT_UNCONVERGED (1 << 30)
typedef struct hb_joint_model {
  double armature[10];      /* kg m^2, >= 0: added to the joint diagonal of M */
  double damping[10];       /* N m s/rad, >= 0: viscous, implicit */
  double frictionloss[10];  /* N m, >= 0: bound of the dry-friction torque */
  double lower[10], upper[10];  /* rad, lower < upper */
  double torque_limit[10];  /* N m, > 0, +inf allowed: actuator saturation */
  double limit_erp;         /* [0, 1]: share of a limit violation removed per substep */
  double tol;               /* rad/s, >= 0: joint residual above which HB_JOINT_UNCONVERGED is raised */
  int32_t limits;           /* 0 / 1: joint stops off / on */
  int32_t reserved;         /* 0 */
} hb_joint_model;
/* model NULL switches the joint model off (hb_plant_step then launches the kernel of contact model 1 exactly as without one).
 * HB_ERR_STATE before hb_plant_reset or outside contact model 1; HB_ERR_ARG for a violated range, a non-finite field other than a +inf
 * torque limit, or a nonzero `reserved` (the model in force is kept).  The model survives hb_plant_reset, which clears its impulses,
 * outputs and status; leaving contact model 1 switches it off. */
int32_t hb_plant_set_joint_model(hb_ctx* ctx, const hb_joint_model* model);
/* Joint outputs of the last step under the joint model (any may be NULL; zero between hb_plant_reset and the first step, and without a
 * joint model): tau_applied / friction_torque / limit_torque [batch][10], residual[batch], status[batch].  HB_ERR_STATE before
 * hb_plant_reset or outside contact model 1. */
int32_t hb_plant_get_joints(hb_ctx* ctx, double* tau_applied, double* friction_torque, double* limit_torque, double* residual,
                            int32_t* status);

/* ---- per-instance terrain of contact model 1: an inclined plane per robot, a friction coefficient per contact point -----------------
 * Instance i has a plane {x : n . x = d} with unit normal n, n_z >= 0.5, and a friction coefficient mu_c >= 0 for each contact point
 * c = 0..3.  The contact frame is T = [t1 t2 n] (columns), built once by hb_plant_set_terrain on the host:
 *     t1 = (e_x - n_x n) / |e_x - n_x n|,     t2 = n x t1;      for n = e_z this is the identity exactly.
 * With a terrain in force, steps 1 - 6 of contact model 1 read as follows; everything not named stays as written there.
 *  1. J~ = blockdiag(T') J: rows 3c, 3c + 1, 3c + 2 are the t1, t2, n components of point c.  The gap is phi_c = n . x_c - d.
 *  3. W = J~ M^-1 J~' + eps tr(J~ M^-1 J~') I,  c = J~ v_f + b, b on the normal rows, from phi_c as today.
 *  4. Unchanged, with mu_c of the point in place of mu.  The impulses p are components in (t1, t2, n).
 *  5. v+ = v_f + M^-1 J~' p.
 *  6. lambda_c = T p_c / h (world forces, as today); point_vel stays the world velocity J v+; gap_c = n . x_c - d at the new q;
 *     touching_c = (p_n > 0); HB_CONTACT_FALLEN is raised when n . q[0:3] - d < fall_height.
 * Joint model: rows 0 - 11 of its 32-row problem take the same substitution, through A, the contact columns of X and Jc; the joint
 * rows are unchanged.  Arithmetic order: every product with T is the sum over the world axes in the order x, y, z (T p over t1, t2, n);
 * with T = I it returns its operand, so a terrain (0, 0, 1, ground_z) with mu = cfg.mu gives the step without a terrain, value for value.
 *
 * plane: [batch][4] = n_x n_y n_z d, or NULL for (0, 0, 1, ground_z) for every instance; mu: [batch][4], or NULL for cfg.mu for every
 * point; both defaults are snapshots of the configuration in force at the call.  Both NULL switches the terrain off: the step then
 * launches the kernels it launches without one.  n is normalised on the host before it is stored.  HB_ERR_ARG for a non-finite entry,
 * | |n| - 1 | > 1e-9, n_z < 0.5 or mu < 0 (the message names the first offending instance; the terrain in force is kept); HB_ERR_STATE
 * before hb_plant_reset or outside contact model 1.  The call clears the contact impulses (the warm start is expressed in the frame of
 * before) and nothing else.  The terrain survives hb_plant_reset and a second hb_plant_set_contact_model with mode 1; leaving model 1
 * switches it off.  cfg.mu and cfg.ground_z are not read by a step while a terrain is in force.  One ground at a time: every successful
 * call, both NULL included, ends a terrain profile (hb_plant_set_terrain_profile below) or a height field (hb_plant_set_terrain_field)
 * in force. */
int32_t hb_plant_set_terrain(hb_ctx* ctx, const double* plane /*[batch][4] or NULL*/, const double* mu /*[batch][4] or NULL*/);
/* The terrain in force (any pointer may be NULL): plane[batch][4] with the stored unit normal, mu[batch][4], frame[batch][9] = T
 * row-major.  Without a terrain: what the model in force amounts to, (0, 0, 1, ground_z), cfg.mu and the identity.  HB_ERR_STATE before
 * hb_plant_reset or outside contact model 1.  A terrain profile is no terrain of this call: with one in force it reports the level ground. */
int32_t hb_plant_get_terrain(hb_ctx* ctx, double* plane, double* mu, double* frame);

/* ---- per-instance terrain profile of contact model 1: piecewise-planar ground per robot (ramps, curbs, stairs) ------------------------
 * Instance i has a horizontal unit direction a = (a_x, a_y), K knots (s_k, z_k), 2 <= K <= HB_PROFILE_MAX_KNOTS, s strictly increasing,
 * and a friction coefficient mu_c >= 0 per contact point.  The ground is the surface z = z(s), s = a_x x + a_y y, with z(s) linear
 * between knots and the first and the last segment continued beyond their end knots.  Segment j (knots j, j + 1) has the slope
 * m_j = (z_{j+1} - z_j) / (s_{j+1} - s_j), the plane n_j = (-m_j a_x, -m_j a_y, 1) / sqrt(1 + m_j^2), d_j = n_j . (a_x s_j, a_y s_j, z_j),
 * and the 10-double record (T_j, d_j): the frame T_j of n_j exactly as hb_plant_set_terrain builds it for the plane (n_j, d_j), so a
 * one-segment profile stores, bit for bit, the record of that plane.
 * Per substep, once the world contact points x_c of the substep's start are known, point c takes the segment j_c with
 * s_{j_c} <= s(x_c) < s_{j_c + 1} (the end segments open-ended) and with it T_c, d_c.  Steps 1 - 6 of the terrain above then hold with
 * T_c, d_c of the point in place of T, d: J~ = blockdiag(T_c') J; block (c, c') of A becomes T_c' A_cc' T_c'; the contact columns of X take
 * their point's frame; phi_c = n_c . x_c - d_c; the impulses p_c are components in the point's own (t1, t2, n); lambda_c = T_c p_c / h and
 * point_vel stay world quantities (T_c of the last substep); with the joint model rows 0 - 11 take the same substitution.  The outputs
 * at q+ select again from the new positions: gap_c = n_c . x_c - d_c over the facet under point c, HB_CONTACT_FALLEN over the facet under
 * the base origin q[0:3].  Arithmetic order: as the terrain's, every product with T_c the sum over the world axes x, y, z.  So a profile
 * whose segments are all level at ground_z with mu = cfg.mu is the step without a terrain, and a one-segment profile the step of
 * hb_plant_set_terrain on the same plane, value for value.  With a model variation in force the step runs on the instance's own model.
 *
 * n_knots[batch]; dir[batch][2] (|a| > 0, normalised before it is stored); knots[batch][HB_PROFILE_MAX_KNOTS][2] = (s_k, z_k), entries
 * from n_knots on are not read; mu[batch][4] or NULL for cfg.mu (a snapshot).  n_knots, dir and knots all NULL (and mu NULL) switch the
 * profile off.  HB_ERR_ARG for K out of range, a non-finite entry, |a| = 0, a knot spacing <= 0, |m_j| > sqrt(3) (n_z < 0.5) or mu < 0 (the
 * message names the first offending instance; the profile in force is kept).  HB_ERR_STATE before hb_plant_reset, outside contact
 * model 1, and while a respawn configuration or a scenario with the slope or friction channel is in force (those two calls in turn are
 * refused while a profile is in force).  One ground at a time: setting a profile replaces a terrain of hb_plant_set_terrain or a height
 * field of hb_plant_set_terrain_field, and hb_plant_set_terrain replaces a profile; both clear the contact impulses and nothing else.  The profile survives hb_plant_reset and a
 * second hb_plant_set_contact_model with mode 1; leaving model 1 switches it off.  With an episode record in force, height and tilt of
 * the record are measured against the facet under the base origin. */
#define HB_PROFILE_MAX_KNOTS 16
int32_t hb_plant_set_terrain_profile(hb_ctx* ctx, const int32_t* n_knots /*[batch]*/, const double* dir /*[batch][2]*/,
                                     const double* knots /*[batch][HB_PROFILE_MAX_KNOTS][2]*/, const double* mu /*[batch][4] or NULL*/);
/* The profile in force (any pointer may be NULL): n_knots[batch], dir[batch][2] as stored, knots[batch][HB_PROFILE_MAX_KNOTS][2] (zero
 * from n_knots on), mu[batch][4], records[batch][HB_PROFILE_MAX_KNOTS - 1][10] = (T_j row-major, d_j) per segment (zero from n_knots - 1
 * on), segment[batch][5] = the segment under the four contact points and under the base origin at the end of the last step (at the state
 * of the last hb_plant_reset or of the set call before a step).  HB_ERR_STATE without a profile in force. */
int32_t hb_plant_get_terrain_profile(hb_ctx* ctx, int32_t* n_knots, double* dir, double* knots, double* mu, double* records, int32_t* segment);

/* ---- per-instance height field of contact model 1: two-dimensional triangulated ground per robot (cross slopes, bumps, rough ground) ---
 * Instance i has
 *   dir      a horizontal direction a = (a_x, a_y), normalised before it is stored; b = (-a_y, a_x) is the second grid axis;
 *   origin   (u0, w0): the grid coordinates of node (0, 0);
 *   spacing  (du, dw) > 0: the distance between neighbouring nodes along a and along b;
 *   n_nodes  (nu, nw), 2 <= nu, nw <= HB_FIELD_MAX_NODES;
 *   heights  z[iu][iw], the height of node (iu, iw), which lies at the world point a (u0 + iu du) + b (w0 + iw dw);
 *   mu       a friction coefficient mu_c >= 0 per contact point.
 * Selection.  A world point x has u = a . (x, y) - u0, w = b . (x, y) - w0, the cell i = clamp(floor(u / du), 0, nu - 2),
 * j = clamp(floor(w / dw), 0, nw - 2) and the cell coordinates fu = u / du - i, fw = w / dw - j (outside the grid the planes of the border
 * cell continue, as the end segments of a profile do).  Each cell is cut along the diagonal from node (i, j) to node (i + 1, j + 1): with
 * fu >= fw the facet is the lower triangle (t = 0), p = (z[i+1][j] - z[i][j]) / du, r = (z[i+1][j+1] - z[i+1][j]) / dw; otherwise the upper
 * one (t = 1), r = (z[i][j+1] - z[i][j]) / dw, p = (z[i+1][j+1] - z[i][j+1]) / du.  The facet id is 2 (i (nw - 1) + j) + t.  A NaN
 * coordinate selects facet 0 and yields a NaN record.
 * Plane.  n = (-(p a_x + r b_x), -(p a_y + r b_y), 1) / sqrt(1 + p^2 + r^2), normalised until its length rounds to 1;
 * d = n . (a (u0 + i du) + b (w0 + j dw), z[i][j]) (both triangles of a cell pass through node (i, j)); the 10-double record (T, d) is the
 * frame of n exactly as hb_plant_set_terrain builds it for the plane (n, d).  Every operation is rounded on its own; host and device run
 * one routine.  The record is computed where it is needed from the four heights of the cell: no table of facets is stored.
 * Step.  The definition of the terrain profile above holds with this facet in place of the segment: the facet of point c is selected
 * from the contact points of the substep's start, J~ = blockdiag(T_c') J, the impulses are components in the point's own frame,
 * lambda_c = T_c p_c / h and point_vel stay world quantities, the outputs select again at q+, and HB_CONTACT_FALLEN as well as height and
 * tilt of an episode record are measured over the facet under the base origin.  A field level at ground_z with mu = cfg.mu is the step
 * without a terrain.  With a model variation in force the step runs on the instance's own model.
 *
 * n_nodes[batch][2]; dir[batch][2]; origin[batch][2]; spacing[batch][2]; heights[batch][HB_FIELD_MAX_NODES][HB_FIELD_MAX_NODES], entries
 * beyond (nu, nw) are not read; mu[batch][4] or NULL for cfg.mu (a snapshot).  The five leading pointers all NULL (and mu NULL) switch
 * the field off.  HB_ERR_ARG for a count out of range, a non-finite entry, |a| = 0, a spacing <= 0, a triangle with
 * p^2 + r^2 > 3 (1 + 1e-12) (n_z < 0.5) or mu < 0 (the message names the first offending instance; the ground in force is kept).
 * HB_ERR_STATE before hb_plant_reset, outside contact model 1, and while a respawn configuration, a profile draw or a scenario with the
 * slope or friction channel is in force (those three calls in turn are refused while a field is in force).  One ground at a time: plane,
 * profile and field replace one another; setting a field clears the contact impulses and nothing else.  The field survives
 * hb_plant_reset and a second hb_plant_set_contact_model with mode 1; leaving model 1 switches it off. */
#define HB_FIELD_MAX_NODES 32
int32_t hb_plant_set_terrain_field(hb_ctx* ctx, const int32_t* n_nodes /*[batch][2]*/, const double* dir /*[batch][2]*/,
                                   const double* origin /*[batch][2]*/, const double* spacing /*[batch][2]*/,
                                   const double* heights /*[batch][HB_FIELD_MAX_NODES][HB_FIELD_MAX_NODES]*/,
                                   const double* mu /*[batch][4] or NULL*/);
/* The field in force (any pointer may be NULL): n_nodes, dir (as stored), origin, spacing, heights (zero beyond (nu, nw)) and mu as laid
 * out above, facet[batch][5] = the facet id under the four contact points and under the base origin at the end of the last step (at the
 * state of the last hb_plant_reset or of the set call before a step).  HB_ERR_STATE without a field in force. */
int32_t hb_plant_get_terrain_field(hb_ctx* ctx, int32_t* n_nodes, double* dir, double* origin, double* spacing, double* heights, double* mu,
                                   int32_t* facet);
/* Unit entry: the device's facet selection for n_points arbitrary world points per instance of the field in force.  xyz[batch][n_points][3];
 * facet_id[batch][n_points], records[batch][n_points][10] = (T row-major, d) of the facet, height[batch][n_points] = n . x - d (any output
 * may be NULL).  HB_ERR_STATE without a field in force. */
int32_t hb_plant_field_eval(hb_ctx* ctx, int32_t n_points, const double* xyz, int32_t* facet_id, double* records, double* height);

/* ---- per-instance model variation of contact model 1: a mass scale per body and a payload on the base ---------------------------------
 * Instance i steps on inertial parameters of its own; everything on the controller's side keeps the nominal model of hb_create.  The
 * nominal body b has mass m_b, centre of mass c_b in its link frame and inertia I_b about c_b (xx xy xz yy yz zz, link axes).  A
 * variation gives instance i a scale s_b > 0 per body (mass_scale, 1 if NULL) and a payload on the base, body 0 (payload, nothing if
 * NULL): mass m_p >= 0, position r of its centre of mass in the base frame, measured from the base origin, and inertia I_p about the
 * payload's own centre of mass in base axes (xx xy xz yy yz zz, positive semidefinite).
 *
 * Composition (csrc/hb_modelvar.hpp; every operation is an IEEE double operation in the order written, brackets first):
 *   links b >= 1:  m_b' = s_b m_b;   I_b'[k] = s_b I_b[k], k = 0..5;   c_b' = c_b   (a density scale)
 *   base:          ms = s_0 m_0;     m_0' = ms + m_p;     c_0'[a] = (ms c_0[a] + m_p r[a]) / m_0',  a = x, y, z
 *                  d1 = c_0 - c_0',  d2 = r - c_0'
 *                  I_0'[k] = ((s_0 I_0[k] + P(ms, d1)[k]) + I_p[k]) + P(m_p, d2)[k]
 *                  P(m, d) = m (|d|^2 1 - d d'):  |d|^2 = (d_x d_x + d_y d_y) + d_z d_z;  diagonal entry aa = m (|d|^2 - d_a d_a);
 *                  off-diagonal entry ab = m (0 - d_a d_b)
 *   total_mass' = ((0 + m_0') + m_1') + ... + m_10', in body order
 *   gravity, joint origins and axes, joint limits and contact offsets: the nominal values.
 * The unvaried instance — m_p == 0 and every s_b == 1.0 — gets a byte copy of the nominal device record instead; its total_mass is not
 * summed again.  So "no variation" is an == statement: such a context computes what the context without a variation computes.
 *
 * What uses which model.  The varied model enters the step routines of contact model 1 only (contact_step / joints_step, held and hybrid
 * form): the mass matrix, nle, X = Mh^-1 [...], W and through them every output of the step.  The repacking of the new state and the
 * resident MPC observation a step writes (centroidal_state_from_rbd), hb_plant_sense (it reads gravity), hb_plant_reset (kinematics), the
 * episode record and everything of the controller (estimator, reference generation, MPC, WBC, hb_joint_command) keep the nominal model.
 * The steps run the terrain form of the kernels (above): without a terrain on the record (0, 0, 1, ground_z), cfg.mu, T = I of the
 * configuration in force, which is the step without a terrain value for value.
 *
 * mass_scale: [batch][HB_NBODY] or NULL; payload: [batch][HB_PAYLOAD_SIZE] = m_p, r[3], I_p[6], or NULL.  Both NULL switches the variation
 * off: the step then launches the kernels it launches without one.  HB_ERR_ARG (the message names the first offending instance; the
 * variation in force is kept) for a non-finite value, s_b <= 0, m_p < 0, m_p == 0 with a nonzero I_p, or an I_p that is not positive
 * semidefinite: with a = the largest |entry| of I_p, a diagonal entry < 0, a 2 x 2 principal minor (I_aa I_bb - I_ab I_ab) < -4 eps a^2
 * or the determinant ((xx yy zz + xy yz xz) + xz xy yz) - ((xz yy xz + xy xy zz) + xx yz yz) < -64 eps a^3, eps = 2^-52 (the slack covers
 * the roundings of these expressions on entries up to a).  HB_ERR_STATE before hb_plant_reset or outside contact model 1 (the pinned stub
 * has no varied form).  The call changes the model and nothing else: the stored impulses stay a warm start, outputs and status stay, an
 * episode record is not restarted.  The variation survives hb_plant_reset and a second hb_plant_set_contact_model with mode 1; leaving
 * model 1 switches it off.  The first call allocates [batch] device records of about 1.7 KB. */
#define HB_PAYLOAD_SIZE 10 /* m_p, r[3] (base frame, from the base origin), I_p[6] = xx xy xz yy yz zz about the payload's own COM, base axes */
int32_t hb_plant_set_model_variation(hb_ctx* ctx, const double* mass_scale /*[batch][HB_NBODY] or NULL*/,
                                     const double* payload /*[batch][HB_PAYLOAD_SIZE] or NULL*/);
/* The model every instance steps on (any pointer may be NULL): mass[batch][HB_NBODY], com[batch][HB_NBODY][3],
 * inertia[batch][HB_NBODY][6], total_mass[batch], from the host's copy of the uploaded image.  Without a variation: the nominal model
 * repeated per instance.  HB_ERR_STATE before hb_plant_reset or outside contact model 1. */
int32_t hb_plant_get_model_variation(hb_ctx* ctx, double* mass, double* com, double* inertia, double* total_mass);

/* ---- hybrid step: the actuator loop per substep --------------------------------------------------------------------------------
 * The reference's controller does not send a torque but the hybrid command (joint_pos, joint_vel, kp, kd, ff_tau), and its simulator turns
 * it into a torque inside every simulator step from the simulator's own joint state (mujoco/src/main.cc:243-249).  An instance has a
 * hybrid command (pos_des, vel_des, kp, kd, ff)[10].  A hybrid step of `substeps` substeps of length h = dt / substeps evaluates
 *     tau_s[j] = ff[j] + kp[j] (pos_des[j] - q_s[6 + j]) + kd[j] (vel_des[j] - v_s[6 + j])
 * at the start of every substep s from the plant's own (q_s, v_s) (operand order of hb_joint_command's torque), and tau_s is used
 * wherever that substep of hb_plant_step uses tau: the right-hand side S' tau_s - nle (+ w) of the pinned stub and of contact model 1;
 * with the joint model tau_a = clamp(tau_s, +-torque_limit) is taken every substep.  The law is explicit (MuJoCo's Euler integrator is
 * implicit in the joint damping only, not in actuator terms; hunter.xml sets neither timestep nor integrator, so the reference runs the
 * law once per 2 ms simulator step: substeps = 1, dt = 0.002 is that rate, more substeps are finer).  Contact flags as in hb_plant_step.
 * Outputs: the torque hb_plant_sense reports and tau_applied of hb_plant_get_joints are those of the LAST substep (saturated under the
 * joint model); bit 10 + j of the joint status word is set if joint j was saturated in ANY substep of the step; tau_first[batch][10] =
 * tau_0 before saturation and tau_mean[batch][10] = the mean over the substeps of the torque integrated (tau_a with the joint model,
 * else tau_s) describe the last hybrid step: zero after hb_plant_reset, untouched by hb_plant_step.
 * The five arrays are host [batch][10].  All five NULL: the command of the last hb_joint_command is used where it lies on the device
 * (HB_ERR_STATE if there is none); some but not all NULL: HB_ERR_ARG.  contact / dt / substeps / to_resident and the state checks as for
 * hb_plant_step.  Runs on whichever plant form is in force.  Does not touch the received LCM command (hunter_lcm.h) or its timestamps. */
int32_t hb_plant_step_hybrid(hb_ctx* ctx, const double* pos_des, const double* vel_des, const double* kp, const double* kd,
                             const double* tau_ff, const int32_t* contact, double dt, int32_t substeps, int32_t to_resident);
/* tau_first / tau_mean [batch][10] of the last hybrid step and last_timestamp[batch] = the stored bits of the simulator end's timestamp
 * filter (hunter_lcm.h hb_plant_step_lcm); any may be NULL.  HB_ERR_STATE before hb_plant_reset. */
int32_t hb_plant_get_actuator(hb_ctx* ctx, double* tau_first, double* tau_mean, int64_t* last_timestamp);

/* ---- per-instance episode record and stop-on-fall ---------------------------------------------------------------------------------
 * What a rollout produced, reduced per instance on the device, so that a batch of scenarios runs thousands of ticks without a read-back
 * per tick.  Off by default.  With an episode in force the record is updated once after EVERY plant step, whatever the entry point
 * (hb_plant_step, hb_plant_step_hybrid, hb_plant_step_lcm), the plant form and to_resident, by a kernel of its own (k_plant_episode)
 * enqueued behind the plant kernel on the same stream; the plant kernels do not know of it.  An instance has an integer record
 * irec[HB_EP_NI] and a double record drec[HB_EP_ND] (fields HB_EP_I_* / HB_EP_D_* below) and up to trace_capacity trace samples.
 *
 * The update of one instance after a step of length dt; k = number of steps the record has seen before this one:
 *  1. STEPS = k + 1.  If any of q[16], v[16] is non-finite and FIRST_NONFINITE < 0: FIRST_NONFINITE = k.
 *  2. If END_TICK >= 0 the record is frozen: return.
 *  3. If the state is non-finite: END_TICK = k, END_CAUSE = HB_EP_NONFINITE, return (the tick contributes nothing).
 *  4. (n, d) = the instance's plane: the terrain's if one is in force, else (e_z, ground_z) in contact model 1, else (e_z, 0).
 *     height = n . q[0:3] - d, summed in the order x, y, z;  tilt = max(|q[4]|, |q[5]|) (pitch, roll).
 *     fallen = contact model 1 has HB_CONTACT_FALLEN in its status word, or tilt_limit > 0 and tilt > tilt_limit.
 *  5. If fallen: END_TICK = k, END_CAUSE = HB_EP_FALLEN; with stop_on_fall the instance's emergency-stop latch becomes 1; return.  The
 *     record then holds the last upright tick.
 *  6. Otherwise the tick is accumulated:  TICKS += 1;  LAST_BASE[6] = q[0:6];  HEIGHT_LAST = height, HEIGHT_MIN / HEIGHT_MAX;  TILT_MAX;
 *     TAU_MAX[j] = max |tau_last[j]| with tau_last the torque the step applied (the saturated one under the joint model, the last
 *     substep's in the hybrid forms: what hb_plant_sense reports);  WORK_ABS += dt (sum_j |tau_last[j] v[6 + j]|),  WORK_NET += dt (sum_j
 *     tau_last[j] v[6 + j]), j upwards, dt multiplied after the sum;  once a WBC call has run, with st = the WBC status word:
 *     WBC_STATUS_OR |= st, and if st != 0: WBC_FAIL_TICKS += 1 and FIRST_WBC_FAIL = k if it was < 0.
 *     Contact model 1 only, per point c:  GAP_MIN = min gap_c (one value over the four points);  FN_MAX[c] = max n . lambda_c;
 *     CONTACT_TICKS[c] += touching_c;  TOUCHDOWNS[c] counts the 0 -> 1 transitions of touching_c (the previous flags are kept in the record,
 *     PREV_TOUCHING, "not touching" at the start);  for touching points only the tangential speed |pv_c - (n . pv_c) n| of the point
 *     velocity pv_c feeds SLIP_SPEED_MAX, and a tick with any touching point faster than slip_speed: SLIP_TICKS += 1, FIRST_SLIP = k if it was
 *     < 0.  Per instance: RES_MAX = max residual;  UNCONVERGED_TICKS counts HB_CONTACT_UNCONVERGED;  CONTACT_STATUS_OR.
 *     Joint model only:  JRES_MAX,  JOINT_STATUS_OR,  CLAMP_TICKS = ticks with any of the bits 10..19 of the joint status word (a torque
 *     saturated),  STOP_TICKS = ticks with any of the bits 0..9 (a stop active).
 *     A field whose source is absent keeps its initial value.  No product is fused with a sum: the record equals the same reduction of
 *     the per-tick outputs of hb_plant_get_state / _get_contact / _get_joints value for value.
 *  7. Trace: if trace_every > 0, k % trace_every == 0 and N_TRACE < trace_capacity, one sample of HB_EP_TRACE_W doubles is appended:
 *     (k, q[0], q[1], height, q[3], q[4], q[5], number of touching points).
 * Initial values, from the plant's present state: START_POS[3] = q[0:3], LAST_BASE = q[0:6], HEIGHT_LAST = its height; HEIGHT_MIN and
 * GAP_MIN +inf, HEIGHT_MAX -inf; the other maxima 0 (they are of non-negative quantities); counts, ORs and PREV_TOUCHING 0; END_CAUSE
 * HB_EP_RUNNING; END_TICK and every FIRST_* -1.
 * The MPC status word is not in the record: it lives on the MPC stream, and reading it here would order the two streams.
 *
 * stop_on_fall: the latch is the emergencyStopFlag_ mirror of hb_joint_set_flags.  From the next hb_joint_command on the instance's
 * command is setCommand(0, 0, 0, 1, 0) (LeggedController.cpp:245-248) until the caller clears the latch with hb_joint_set_flags.
 * Nothing else about the instance changes: the plant goes on integrating it, MPC and WBC go on running on it. */
#define HB_EP_RUNNING 0
#define HB_EP_FALLEN 1
#define HB_EP_NONFINITE 2
#define HB_EP_TRACE_W 8
#define HB_EP_TRACE_MAX 4096
#define HB_EP_JOINT_STOP_BITS 0x3ff
#define HB_EP_JOINT_CLAMP_BITS 0xffc00
enum {   /* irec */
  HB_EP_I_STEPS = 0, HB_EP_I_TICKS = 1, HB_EP_I_END_TICK = 2, HB_EP_I_END_CAUSE = 3, HB_EP_I_FIRST_NONFINITE = 4, HB_EP_I_N_TRACE = 5,
  HB_EP_I_WBC_STATUS_OR = 6, HB_EP_I_WBC_FAIL_TICKS = 7, HB_EP_I_FIRST_WBC_FAIL = 8, HB_EP_I_CONTACT_TICKS = 9 /* [4] */,
  HB_EP_I_TOUCHDOWNS = 13 /* [4] */, HB_EP_I_PREV_TOUCHING = 17 /* [4] */, HB_EP_I_SLIP_TICKS = 21, HB_EP_I_FIRST_SLIP = 22,
  HB_EP_I_UNCONVERGED_TICKS = 23, HB_EP_I_CONTACT_STATUS_OR = 24, HB_EP_I_JOINT_STATUS_OR = 25, HB_EP_I_CLAMP_TICKS = 26,
  HB_EP_I_STOP_TICKS = 27, HB_EP_NI = 28
};
enum {   /* drec */
  HB_EP_D_START_POS = 0 /* [3] */, HB_EP_D_LAST_BASE = 3 /* [6] */, HB_EP_D_HEIGHT_LAST = 9, HB_EP_D_HEIGHT_MIN = 10, HB_EP_D_HEIGHT_MAX = 11,
  HB_EP_D_TILT_MAX = 12, HB_EP_D_TAU_MAX = 13 /* [10] */, HB_EP_D_WORK_ABS = 23, HB_EP_D_WORK_NET = 24, HB_EP_D_GAP_MIN = 25,
  HB_EP_D_FN_MAX = 26 /* [4] */, HB_EP_D_SLIP_SPEED_MAX = 30, HB_EP_D_RES_MAX = 31, HB_EP_D_JRES_MAX = 32, HB_EP_ND = 33
};
typedef struct hb_episode_config {
  double slip_speed;      /* m/s, >= 0: a touching point faster than this along the ground counts as slipping */
  double tilt_limit;      /* rad, >= 0; 0: none.  max(|pitch|, |roll|) above it counts as fallen (works in contact model 0 too) */
  int32_t stop_on_fall;   /* 0 / 1: the tick an instance is found fallen, its emergency-stop latch (hb_joint_set_flags) is set */
  int32_t trace_every;    /* 0: no trace; n > 0: one trace sample every n-th tick while the instance is up */
  int32_t trace_capacity; /* 0 .. HB_EP_TRACE_MAX samples per instance */
  int32_t reserved[3];    /* 0 */
} hb_episode_config;
/* cfg NULL: off.  Otherwise (re)starts the record from the plant's present state.  The configuration survives hb_plant_reset, which
 * restarts the record from the reset state; a change of contact model, joint model or terrain does not restart it.  With stop_on_fall the
 * latch array is allocated as hb_joint_set_flags allocates it.  HB_ERR_STATE before hb_plant_reset; HB_ERR_ARG for a non-finite or
 * out-of-range field or a nonzero `reserved` (the episode in force is kept). */
int32_t hb_plant_set_episode(hb_ctx* ctx, const hb_episode_config* cfg);
/* The records (any pointer may be NULL): irec[batch][HB_EP_NI], drec[batch][HB_EP_ND], trace[batch][trace_capacity][HB_EP_TRACE_W] (the
 * first N_TRACE samples of an instance are valid, the rest zero).  HB_ERR_STATE before hb_plant_reset or with no episode in force. */
int32_t hb_plant_get_episode(hb_ctx* ctx, int32_t* irec, double* drec, double* trace);

/* ---- respawn of ended instances: episode after episode on the device ------------------------------------------------------------------
 * With an episode in force, hb_plant_respawn puts every instance whose episode is over back to a spawn state, in one enqueue-only launch
 * (k_plant_respawn) on the plant's stream, ordered against the MPC stream like a plant step that writes the resident observation.  The
 * device decides WHO is put back, from the instance's episode record; the host decides WHEN, by calling.  Off by default.
 *
 * Decision for one instance (irec = its episode record):
 *   if END_TICK >= 0:  cause = END_CAUSE;  respawn iff  STEPS - (END_TICK + 1) >= hold_ticks  (the steps the record has seen after the
 *                      end step);
 *   else if max_ticks > 0 and TICKS >= max_ticks:  cause = HB_RS_TIMEOUT;  respawn (no hold);
 *   else the instance stays and NOT ONE BYTE of any of its arrays is written.
 * An instance that has ended is never a time-out, however many ticks it has.
 *
 * For a respawned instance, in this order:
 *  1. Fold of the finished record into the totals itot[HB_RS_NI] / dtot[HB_RS_ND] (HB_RS_I_* / HB_RS_D_* below):
 *       N_FALLEN / N_NONFINITE / N_TIMEOUT += 1 by cause;  TICKS_SUM += TICKS;  TICKS_MIN = TICKS if EPISODES == 0, else min;  TICKS_MAX =
 *       max;  SLIP_TICKS_SUM += SLIP_TICKS;  WBC_FAIL_TICKS_SUM += WBC_FAIL_TICKS;  STEPS_SUM += STEPS;  LAST_CAUSE = cause;  LAST_TICKS =
 *       TICKS;  EPISODES += 1;   DIST_X_SUM += LAST_BASE[0] - START_POS[0];  DIST_Y_SUM += LAST_BASE[1] - START_POS[1];  WORK_ABS_SUM +=
 *       WORK_ABS;  TILT_MAX = max(TILT_MAX, record TILT_MAX);  TAU_MAX = max over the record's TAU_MAX[0..9] and itself.
 *     Every difference and sum is rounded on its own.  Initial values (hb_plant_set_respawn with a configuration, hb_plant_reset): every
 *     total 0, TICKS_MIN included (it is the first folded TICKS from the first fold on), LAST_CAUSE HB_EP_RUNNING.
 *     Identity: for every instance, at any time,  STEPS_SUM + (STEPS of its current record) = the plant steps enqueued since the totals
 *     were last started; and EPISODE_INDEX == EPISODES, N_FALLEN + N_NONFINITE + N_TIMEOUT == EPISODES.
 *  2. Draw of the spawn state.  e = EPISODE_INDEX + 1, the index of the episode that starts (the state of hb_plant_reset is episode 0 and is
 *     never drawn).  Philox4x32-10 and Box-Muller as for hb_plant_sense (above), u = (word + 0.5) 2^-32:
 *       key = (seed low 32, seed high 32);  counter = (instance_offset + i, e, HB_RS_STREAM, block).
 *       block 0, word 0: the uniform u of the yaw offset;  q[3] = q_spawn[3] + yaw_range (2 u - 1)       (words 1-3 unused)
 *       normal n is lane n % 4 of block 1 + n / 4:  n = 0..9: q[6 + n] = q_spawn[6 + n] + joint_pos_sigma z_n   (blocks 1, 2, 3)
 *                                                   n = 12..14: v[n - 12] = v_spawn[n - 12] + base_vel_sigma z_n  (block 4)
 *     Everything else of q[16], v[16] is q_spawn / v_spawn (v_spawn NULL: zero).  A channel with range / sigma 0 leaves the given value bit
 *     for bit and its blocks are not generated.  Same seed, same instance_offset + i, same e: same bits (a shard reproduces its slice).
 *  3. Placement (place = 1): (n, d) the instance's plane by the rule of step 4 of the episode record; g = min over the four contact points
 *     c of n . p_c - d (summed x, y, z, unfused), p_c the contact points at q;  q[0:3] += (clearance - g) n.  The result is the "last
 *     spawned state" hb_plant_get_respawn returns.
 *  4. Plant: q, v;  anchor = the contact points at q, pinned 0, contact_last 1, lambda, vdot, tau_last 0 (what hb_plant_reset leaves).  Zeroed
 *     where the arrays exist: the contact model's impulses, outputs and status word (HB_CONTACT_FALLEN with it; the external wrench stays);
 *     the joint model's impulses, outputs and status; the actuator record (tau_first, tau_mean, the received command, the timestamp filter);
 *     the emergency-stop latch.  Terrain and model variation stay: they belong to the instance (a scenario in
 *     force, hb_plant_set_scenario below, has drawn them anew before this step).
 *  5. Episode: the record restarts from the new state (initial values above hb_plant_set_episode), its trace rows are zeroed, EPISODE_INDEX
 *     += 1.
 *  6. Estimator, if hb_estimator_reset has run: x_hat = (q[0:3], 0 0 0, the four contact points at q), P = 100 I (what hb_estimator_reset
 *     leaves), yaw_last = 0, low-pass state of hb_estimator_contact_force = 0.
 *  7. The plant's rbd, the resident rbd and the resident MPC observation are repacked from (q, v) as a plant step with to_resident does; the
 *     resident time is left alone.
 *  8. Two pending flags for the MPC side, each consumed once, by the next hb_refgen_update and the next hb_mpc_solve on the MPC stream:
 *     the reference generation takes the flagged instance's latest stance positions from the observation of THAT call (as for the whole
 *     batch after hb_refgen_reset(..., NULL)); the solve cold-starts the flagged instances after the warm start onto the new tables
 *     (hb_mpc_reset_masked semantics: iterate, grid_dirty, status word).
 *  9. Device gait manager, if enabled: the instance becomes a fresh object (hb_gait_reset with a mask).  Host-supplied schedules are the
 *     caller's and are left alone.
 *
 * Limits.  With a respawn configuration in force hb_step_resident and hb_tick_resident return HB_ERR_STATE (the instance-range / graph
 * paths do not consume the pending flags).  The policy published before a respawn belongs to the old episode: call hb_plant_respawn so
 * that the next tick is an MPC tick (reference generation, solve, publish), as ResidentLoop does.  With respawn off every call enqueues
 * exactly what it enqueued before. */
#define HB_RS_TIMEOUT 3          /* cause of an episode ended by max_ticks (beside HB_EP_FALLEN / HB_EP_NONFINITE) */
#define HB_RS_STREAM 0x52535031u /* third counter word of the respawn stream */
enum {   /* itot */
  HB_RS_I_EPISODES = 0, HB_RS_I_N_FALLEN = 1, HB_RS_I_N_NONFINITE = 2, HB_RS_I_N_TIMEOUT = 3, HB_RS_I_TICKS_SUM = 4, HB_RS_I_TICKS_MIN = 5,
  HB_RS_I_TICKS_MAX = 6, HB_RS_I_SLIP_TICKS_SUM = 7, HB_RS_I_WBC_FAIL_TICKS_SUM = 8, HB_RS_I_LAST_CAUSE = 9, HB_RS_I_LAST_TICKS = 10,
  HB_RS_I_EPISODE_INDEX = 11, HB_RS_I_STEPS_SUM = 12, HB_RS_NI = 13
};
enum {   /* dtot */
  HB_RS_D_DIST_X_SUM = 0, HB_RS_D_DIST_Y_SUM = 1, HB_RS_D_WORK_ABS_SUM = 2, HB_RS_D_TILT_MAX = 3, HB_RS_D_TAU_MAX = 4, HB_RS_ND = 5
};
typedef struct hb_respawn_config {
  double clearance;        /* m, >= 0: gap of the lowest contact point after placement */
  double yaw_range;        /* rad, >= 0: uniform yaw offset in [-yaw_range, yaw_range] */
  double joint_pos_sigma;  /* rad, >= 0: Gaussian perturbation of the 10 joint angles */
  double base_vel_sigma;   /* m/s, >= 0: Gaussian perturbation of the 3 linear base velocities */
  uint64_t seed;
  uint32_t instance_offset; /* global index of instance 0 of this context */
  int32_t hold_ticks;      /* >= 0: plant steps an ended instance waits after its end step */
  int32_t max_ticks;       /* >= 0; 0: none.  An instance still up with TICKS >= max_ticks is respawned as timed out */
  int32_t place;           /* 0 / 1 */
  int32_t reserved[2];     /* 0 */
} hb_respawn_config;
/* cfg NULL: off.  q_spawn[batch][16] (required with cfg), v_spawn[batch][16] or NULL = zero.  Starts the totals (initial values above);
 * "last spawned state" starts as (q_spawn, v_spawn).  The configuration survives hb_plant_reset, which restarts the totals (as does
 * hb_plant_set_episode with a configuration: the totals account for the steps of the records they folded); turning the episode off turns
 * respawn off.  HB_ERR_STATE before hb_plant_reset or with no episode in force; HB_ERR_ARG (the configuration in force
 * is kept) for a negative or non-finite clearance / yaw_range / joint_pos_sigma / base_vel_sigma, hold_ticks < 0, max_ticks < 0, place not
 * 0 / 1, a nonzero `reserved`, or cfg without q_spawn. */
int32_t hb_plant_set_respawn(hb_ctx* ctx, const hb_respawn_config* cfg, const double* q_spawn, const double* v_spawn);
/* Enqueue-only.  HB_ERR_STATE without a respawn configuration in force. */
int32_t hb_plant_respawn(hb_ctx* ctx);
/* itot[batch][HB_RS_NI], dtot[batch][HB_RS_ND], q_last / v_last [batch][16] = the last spawned state; any may be NULL.  Synchronises like
 * hb_plant_get_episode.  HB_ERR_STATE without a respawn configuration in force. */
int32_t hb_plant_get_respawn(hb_ctx* ctx, int32_t* itot, double* dtot, double* q_last, double* v_last);

/* ---- scenario draw at respawn: terrain, friction, payload, link masses and a push per episode, on the device ---------------------------
 * With a scenario in force, hb_plant_respawn draws a new scenario for every instance it respawns: a kernel of its own (k_plant_scenario)
 * enqueued ahead of k_plant_respawn in the same call reads the same decision from the still unchanged episode record, and for a
 * respawning instance, in this order, (a) appends the log row of the finished episode, (b) draws, (c) writes the instance's terrain
 * record, DevModel record, push record and parameter row scen[HB_SC_N].  k_plant_respawn is unchanged: it places the robot on the plane it
 * now finds.  An instance that stays costs the decision loads and an exit: NOT ONE BYTE of it is written.  Off by default; without a
 * scenario every call enqueues exactly what it enqueues without this block.  Episode 0 (the state of hb_plant_reset) is never drawn: it runs
 * on the terrain and the variation in force at the call.
 *
 * The draw.  Philox4x32-10, u_k = (word k + 0.5) 2^-32 as for the spawn state (above):
 *       key = (seed low 32, seed high 32) of the SCENARIO's seed;  counter = (instance_offset + i, e, HB_SC_STREAM, block),
 * instance_offset from the respawn configuration in force, e = EPISODE_INDEX + 1 the episode that starts.  Every operation below is an
 * IEEE double operation of its own in the order written, brackets first, nothing fused; there is no trigonometry, logarithm or
 * exponential in it.  Blocks are independent; a block whose channel is off is not generated.
 *   block 0, HB_SC_SLOPE:   g_x = grade_max (2 u_0 - 1),  g_y = grade_max (2 u_1 - 1);   l = sqrt((g_x g_x + g_y g_y) + 1);
 *                           n0 = ((-g_x) / l, (-g_y) / l, 1 / l);   d = (n0_x s_x + n0_y s_y) + n0_z ground_z,  (s_x, s_y) = q_spawn[0:2] of the
 *                           respawn configuration: the plane pivots under the spawn point.  The stored record (T, d) is what
 *                           hb_plant_set_terrain stores for plane = (n0, d), its own normalisation n = n0 / |n0| and the frame T included
 *                           (one routine, csrc/hb_contact.hpp terrain_plane_record, called by both).  n_z >= 1 / sqrt(3) for grade_max <= 1.
 *   block 1, HB_SC_MU:      mu_c = mu_lo + (mu_hi - mu_lo) u_c,  c = 0..3;  with mu_per_point = 0 all four points take c = 0's value.
 *   block 2, HB_SC_PAYLOAD: m_p = payload_mass_max u_0;   r[a] = payload_center[a] + payload_half_extent[a] (2 u_{1+a} - 1);   I_p = 0.
 *   blocks 3-5, HB_SC_MASS: body b uses word b % 4 of block 3 + b / 4:   s_b = 1 + mass_scale_range (2 u - 1)   (> 0 for a range < 1).
 *   block 6, HB_SC_PUSH:    start = push_start_lo + int(u_0 (push_start_hi - push_start_lo + 1))  (<= push_start_hi for every word);
 *                           F_x = push_force_max (2 u_1 - 1),  F_y = push_force_max (2 u_2 - 1).
 * With HB_SC_PAYLOAD or HB_SC_MASS the instance's DevModel record is the composition of hb_plant_set_model_variation (above,
 * csrc/hb_modelvar.hpp modelvar_compose) of the nominal model with s (1 for every body if HB_SC_MASS is off) and the payload (none if
 * HB_SC_PAYLOAD is off), bit for bit what the host setter composes from the same numbers.
 * A channel that is off leaves its part of the records bit for bit (HB_SC_SLOPE: T and d; HB_SC_MU: the four coefficients; both model
 * channels off: the DevModel record) and its entries of scen are 0.  Before an instance's first draw scen is zero with PUSH_START = -1.
 *
 * scen[HB_SC_N]: GRADE[2] = g_x g_y, MUS[4], PAYLOAD_M, PAYLOAD_R[3], SCALE[HB_NBODY], PUSH_START, PUSH_F[2].
 * Log: up to log_capacity rows of HB_SC_LOG_W doubles per instance, appended in order until full (count == log_capacity: later episodes
 * are not logged): the finished episode's index (EPISODE_INDEX before the fold), its cause, TICKS, LAST_BASE[0] - START_POS[0],
 * LAST_BASE[1] - START_POS[1], TILT_MAX of its record, then the HB_SC_N parameters it ran under (all zero, PUSH_START -1, for episode 0).
 *
 * Push.  While HB_SC_PUSH is in force the scenario owns the external wrench of contact model 1: hb_plant_set_scenario zeroes it and
 * switches it on, hb_plant_set_external_wrench returns HB_ERR_STATE, and turning the scenario off clears the wrench and switches it off.
 * Ahead of every plant kernel a kernel of its own (k_plant_push, one thread per instance) writes
 *       wrench_i = (F_x, F_y, 0, 0, 0, 0)  if the instance has a push (start >= 0) and  start <= STEPS < start + push_ticks,  else 0,
 * STEPS that of the instance's current episode record, so the first pushed step of an episode is its step number `start`.  The plant
 * kernels do not change.  hb_plant_reset sets every push record to "none" (start = -1).
 *
 * State.  HB_ERR_STATE before hb_plant_reset, outside contact model 1 or without a respawn configuration in force; HB_ERR_ARG (the
 * configuration in force is kept) for a violated range, a non-finite field or a nonzero `reserved`.  HB_SC_SLOPE or HB_SC_MU without a
 * terrain in force turns the terrain on with the level record ((0, 0, 1, ground_z), cfg.mu, T = I: the step without a terrain, value for
 * value); HB_SC_PAYLOAD or HB_SC_MASS without a variation turns the variation on with nominal copies.  While a scenario is in force
 * hb_plant_get_terrain and hb_plant_get_model_variation synchronise and read the device records (the host copies are stale); turning the
 * scenario off leaves terrain and variation in force as last drawn, and the host copies are refreshed from the device.
 * hb_plant_set_terrain / hb_plant_set_model_variation with a scenario in force overwrite the records of every instance as always; the next
 * draw overwrites them again; switching off (both arguments NULL) what the scenario draws returns HB_ERR_STATE.  Turning respawn or the episode off, or leaving model 1, turns the scenario off.  hb_plant_reset empties the
 * log and sets the push records to "none"; terrain and model records stay as last drawn, scen too.  Every call with a configuration
 * restarts scen, the push records and the log.
 * Out of scope: a draw for episode 0, payload inertia or a payload on a link, non-planar terrain, a push with a moment or more than one
 * push per episode, per-episode joint parameters, the instance-range / graph paths. */
#define HB_SC_STREAM 0x53434E31u /* third counter word; differs from HB_RS_STREAM, so the spawn-state draws keep their bits */
enum { HB_SC_SLOPE = 1, HB_SC_MU = 2, HB_SC_PAYLOAD = 4, HB_SC_MASS = 8, HB_SC_PUSH = 16 }; /* channels */
enum {   /* scen */
  HB_SC_GRADE = 0 /* [2] */, HB_SC_MUS = 2 /* [4] */, HB_SC_PAYLOAD_M = 6, HB_SC_PAYLOAD_R = 7 /* [3] */, HB_SC_SCALE = 10 /* [HB_NBODY] */,
  HB_SC_PUSH_START = 21, HB_SC_PUSH_F = 22 /* [2] */, HB_SC_N = 24
};
#define HB_SC_LOG_W (6 + HB_SC_N) /* finished episode's index, cause, TICKS, dist_x, dist_y, TILT_MAX, then its HB_SC_N parameters */
#define HB_SC_LOG_MAX 1024
typedef struct hb_scenario_config {
  uint64_t seed;
  int32_t channels;           /* OR of HB_SC_* */
  int32_t mu_per_point;       /* 0: one coefficient for the four points; 1: one each */
  double grade_max;           /* [0, 1]: each of the two ground gradients uniform in [-grade_max, grade_max] */
  double mu_lo, mu_hi;        /* 0 <= lo <= hi, finite */
  double payload_mass_max;    /* kg, >= 0 */
  double payload_center[3], payload_half_extent[3];  /* m, base frame; half extents >= 0 */
  double mass_scale_range;    /* [0, 1): s_b uniform in [1 - range, 1 + range] */
  double push_force_max;      /* N, >= 0: each horizontal component uniform in [-max, max] */
  int32_t push_start_lo, push_start_hi;  /* 0 <= lo <= hi <= 1 << 20: first pushed step of the episode */
  int32_t push_ticks;         /* >= 1 with HB_SC_PUSH */
  int32_t log_capacity;       /* 0 .. HB_SC_LOG_MAX finished episodes kept per instance */
  int32_t reserved[2];        /* 0 */
} hb_scenario_config;
/* cfg NULL: off. */
int32_t hb_plant_set_scenario(hb_ctx* ctx, const hb_scenario_config* cfg);
/* scen[batch][HB_SC_N]: the parameters every instance's current episode runs under.  Synchronises like hb_plant_get_episode.  HB_ERR_STATE
 * without a scenario in force. */
int32_t hb_plant_get_scenario(hb_ctx* ctx, double* scen);
/* count[batch] = rows logged per instance, log[batch][log_capacity][HB_SC_LOG_W] (rows behind count are zero); either may be NULL.
 * Synchronises.  HB_ERR_STATE without a scenario in force. */
int32_t hb_plant_get_scenario_log(hb_ctx* ctx, int32_t* count, double* log);

/* ---- profile draw at respawn: level ground, a curb / step-down or a flight of stairs per episode, on the device --------------------------
 * With a profile draw in force, hb_plant_respawn draws a new piecewise-planar ground (the terrain profile above) for every instance it
 * respawns: a kernel of its own (k_plant_profile_draw), enqueued ahead of k_plant_respawn (and behind k_plant_scenario if a scenario is
 * in force too) in the same call, reads the same decision from the still unchanged episode record, and for a respawning instance, in this
 * order, (a) appends the log row of the finished episode, (b) draws, (c) composes the knots and from them the stored profile record, (d)
 * writes the profile record, the knot row, the parameter row row[HB_PD_N] and, with follow_map, the record of the controller's ground map.
 * k_plant_respawn then places the robot on the profile it finds (below).  An instance that stays costs the decision loads and an exit: NOT
 * ONE BYTE of it is written.  Off by default; without a draw every call enqueues exactly what it enqueues without this block.  Episode 0
 * (the state of hb_plant_reset) is never drawn.
 *
 * The draw.  Philox4x32-10, u_k = (word k + 0.5) 2^-32 as for the scenario (above):
 *       key = (seed low 32, seed high 32) of THIS configuration's seed;  counter = (instance_offset + i, e, HB_PD_STREAM, block),
 * instance_offset from the respawn configuration in force, e = EPISODE_INDEX + 1 the episode that starts.  Every operation below is an
 * IEEE double operation of its own in the order written, brackets first, nothing fused; there is no transcendental function in it.  The
 * three blocks are independent and always generated.  a = (a_x, a_y) is the stored unit direction (dir / sqrt(dir_x dir_x + dir_y dir_y),
 * the division of the terrain profile);  s0 = a_x q_spawn[0] + a_y q_spawn[1] of the respawn configuration;  gz = ground_z of the contact
 * model.
 *   block 0:  kind = list[int(u_0 n)], list = the enabled kinds in ascending bit order, n their number;
 *             h = height_lo + (height_hi - height_lo) u_1;
 *             s_r = s0 + (at_lo + (at_hi - at_lo) u_2);
 *             steps = steps_lo + int(u_3 (steps_hi - steps_lo + 1))   (<= steps_hi for every word).
 *   block 1:  r = run_lo + (run_hi - run_lo) u_0.
 *   block 2:  mu_c = mu_lo + (mu_hi - mu_lo) u_c,  c = 0..3;  with mu_per_point = 0 all four points take c = 0's value.
 *   w = max(|h| / riser_slope, 1e-3), the width of a riser.
 * Relative knots (s, g), K of them:
 *   HB_PD_FLAT    K = 2:           (s0 - 1, 0), (s0 + 1, 0);
 *   HB_PD_CURB    K = 4:           (s_r - 1, 0), (s_r, 0), (s_r + w, h), ((s_r + w) + 1, h);
 *   HB_PD_STAIRS  K = 2 + 2 steps: (s_r - 1, 0);  for i = 0 .. steps - 1: (s_r + i r, i h), ((s_r + i r) + w, (i + 1) h);
 *                                  ((s_r + steps r) + 1, steps h)          (i, i + 1, steps converted to double, then one product).
 * The plant's knots are (s, 0 + (gz + g)); its stored record is what hb_plant_set_terrain_profile stores for K, dir, these knots and mu,
 * bit for bit (one routine, csrc/hb_contact.hpp profile_compose, behind both).  With follow_map the controller's map takes the knots
 * (s, 0 + g) and stores what hb_ground_set_profile stores for them (csrc/hb_ground.hpp ground_compose).
 *
 * row[HB_PD_N]: KIND (the bit value), HEIGHT = h (STAIRS: the rise of one step), AT = at_lo + (at_hi - at_lo) u_2 (the bracket of s_r as computed), STEPS,
 * RUN = r, MUS[4].  Entries a kind does not use are 0 (FLAT: HEIGHT, AT, STEPS, RUN; CURB: STEPS, RUN).  Before an instance's first draw
 * the row is zero (KIND 0).
 * Log: up to log_capacity rows of HB_PD_LOG_W doubles per instance, appended in order until full: the finished episode's index
 * (EPISODE_INDEX before the fold), its cause, TICKS, the progress a_x (LAST_BASE[0] - START_POS[0]) + a_y (LAST_BASE[1] - START_POS[1]),
 * TILT_MAX of its record, then the HB_PD_N parameters it ran under.
 *
 * Placement on a profile (k_plant_respawn, whenever a profile is in force at a respawn).  Step 3 of the respawn becomes vertical: contact
 * point c at p_c takes the facet j_c under it (the segment rule of the terrain profile) with (n_c, d_c);  gap_c = ((n_x x + n_y y) + n_z
 * z) - d;  D = max over c of (clearance - gap_c) / n_{c,z};  q[2] += D  (place = 0: no shift).  A vertical shift changes no s, hence no
 * facet, and the lowest gap_c becomes clearance to rounding.  On a level profile D is the shift of step 3 on the level plane, bit for
 * bit.  After placement, either way, the kernel writes the segment under the four contact points and the base origin and the Terrain
 * record of the facet under the base origin (what hb_plant_reset's host locate writes), and the new episode record measures height
 * against that facet.
 *
 * Validity.  The device cannot refuse a draw, so the set call admits only configurations all of whose draws the terrain profile accepts.
 * With |s0| <= 1e3, |at| <= 1e3, run_hi <= 1e3 and |gz| <= 1e3 every knot has |s| < 1.1e4 and |z| < 1.4e4, so a rounding moves a knot by
 * at most 2^-39 m.  s is strictly increasing: lead and tail are 1 m long, a riser is w >= 1e-3 wide, and a tread is at least run_lo - w
 * >= 1e-3 long before rounding (the third refusal below).  Treads and landings have slope exactly 0: both ends carry the same product.
 * A riser has |m| <= (|h| + 4e-12) / (w - 2e-12) <= riser_slope + 1e-8 whether w is |h| / riser_slope or the floor 1e-3; with riser_slope
 * <= 1.7, which is 1.8 % under sqrt(3), that is below the profile's limit.  K <= 2 + 2 * 7 = HB_PROFILE_MAX_KNOTS, and mu_c lies in
 * [mu_lo, mu_hi].
 * HB_ERR_ARG (the configuration in force is kept) for: a non-finite field; riser_slope outside (0, 1.7];  run_lo - max(max(|height_lo|,
 * |height_hi|) / riser_slope, 1e-3) < 1e-3;  |at_lo| or |at_hi| above 1e3;  run_hi above 1e3;  lo > hi in any range, steps outside 1 .. 7,
 * mu_lo < 0;  |dir| = 0;  kinds outside 1 .. 7;  mu_per_point or follow_map not 0 / 1;  log_capacity outside 0 .. HB_PD_LOG_MAX;  a
 * nonzero `reserved`.
 *
 * State.  HB_ERR_STATE before hb_plant_reset, outside contact model 1, without a respawn configuration in force, while a scenario with
 * HB_SC_SLOPE or HB_SC_MU is in force (the other order is refused by hb_plant_set_scenario: a profile is then in force; PAYLOAD, MASS and
 * PUSH combine freely with the draw), with follow_map and no ground map in force (set the zero map first), and when |ground_z| or the
 * |s0| of an instance's q_spawn exceeds 1e3.  Setting the draw puts every instance on the level profile (the FLAT knots around its s0,
 * cfg.mu) located at the plant's current state, replacing a terrain of hb_plant_set_terrain, clears the contact impulses as
 * hb_plant_set_terrain_profile does, and restarts the rows and the log; with follow_map the controller's map becomes the zero map over
 * the same knots, so plant and map start level together, also when the call replaces a draw in force.  A configuration in force is
 * switched off before the new one's arrays are allocated and written: HB_ERR_ARG and HB_ERR_STATE keep it, HB_ERR_DEVICE leaves the
 * draw off.  While the draw is in force hb_plant_set_terrain and every hb_plant_set_terrain_profile, the switch-off call included,
 * return HB_ERR_STATE (hb_plant_set_respawn with a configuration is refused anyway: a profile is in force), hb_plant_set_contact_model refuses a |ground_z| above 1e3 with HB_ERR_ARG, and hb_plant_get_terrain_profile,
 * hb_ground_get_profile and hb_plant_reset read the device records first (the host copies are stale).  cfg NULL, turning respawn or the
 * episode off switch the draw off: profile and map stay in force as last drawn, the host copies are refreshed, and respawn, if still on,
 * keeps placing on the profile.  Leaving model 1 switches draw and profile off.  hb_plant_reset empties the log; records and rows stay.
 * Out of scope: a draw for episode 0, a direction per episode, the instance-range / graph paths (two-dimensional ground:
 * hb_plant_set_field_draw below). */
#define HB_PD_STREAM 0x50444431u /* third counter word; differs from HB_RS_STREAM and HB_SC_STREAM */
enum { HB_PD_FLAT = 1, HB_PD_CURB = 2, HB_PD_STAIRS = 4 }; /* kinds */
enum { HB_PD_KIND = 0, HB_PD_HEIGHT = 1, HB_PD_AT = 2, HB_PD_STEPS = 3, HB_PD_RUN = 4, HB_PD_MUS = 5 /* [4] */, HB_PD_N = 9 }; /* row */
#define HB_PD_LOG_W (5 + HB_PD_N) /* finished episode's index, cause, TICKS, progress, TILT_MAX, then its HB_PD_N parameters */
#define HB_PD_LOG_MAX 1024
typedef struct hb_profile_draw_config {
  uint64_t seed;
  int32_t kinds;              /* OR of HB_PD_*, at least one */
  int32_t mu_per_point;       /* 0: one coefficient for the four points; 1: one each */
  double dir[2];              /* |dir| > 0, normalised as the terrain profile normalises it */
  double height_lo, height_hi;/* m, signed (negative: down), lo <= hi: curb height / stair rise */
  double at_lo, at_hi;        /* m along dir from the spawn point to the first riser, lo <= hi, |.| <= 1e3 */
  double riser_slope;         /* (0, 1.7] */
  int32_t steps_lo, steps_hi; /* 1 <= lo <= hi <= 7 */
  double run_lo, run_hi;      /* m, tread length incl. riser, lo <= hi <= 1e3 */
  double mu_lo, mu_hi;        /* 0 <= lo <= hi */
  int32_t follow_map;         /* 0 / 1: the controller's ground map follows the drawn profile */
  int32_t log_capacity;       /* 0 .. HB_PD_LOG_MAX finished episodes kept per instance */
  int32_t reserved[2];        /* 0 */
} hb_profile_draw_config;
/* cfg NULL: off. */
int32_t hb_plant_set_profile_draw(hb_ctx* ctx, const hb_profile_draw_config* cfg);
/* row[batch][HB_PD_N]: the parameters every instance's current ground was drawn with.  Synchronises like hb_plant_get_episode.
 * HB_ERR_STATE without a profile draw in force. */
int32_t hb_plant_get_profile_draw(hb_ctx* ctx, double* row);
/* count[batch] = rows logged per instance, log[batch][log_capacity][HB_PD_LOG_W] (rows behind count are zero); either may be NULL.
 * Synchronises.  HB_ERR_STATE without a profile draw in force. */
int32_t hb_plant_get_profile_draw_log(hb_ctx* ctx, int32_t* count, double* log);

/* ---- field draw at respawn: a 32 x 32 height field per episode, composed on the device; respawn on it --------------------------------------
 * With a field draw in force, hb_plant_respawn composes a new height field (hb_plant_set_terrain_field below) for every instance it
 * respawns: a kernel of its own (k_plant_field_draw, one wavefront per instance), enqueued ahead of k_plant_respawn (and behind
 * k_plant_scenario if a scenario is in force too) in the same call, reads the same decision from the still unchanged episode record, and
 * for a respawning instance, in this order, (a) appends the log row of the finished episode, (b) draws, (c) composes the heights and the
 * stored header, (d) writes heights, header, the parameter row row[HB_FD_N] and, with follow_map, heights and header of the controller's
 * field map (hb_ground_set_field).  k_plant_respawn then places the robot on the field it finds (below).  An instance that stays costs the
 * decision loads and an exit: NOT ONE BYTE of it is written.  Nothing crosses the bus.  Off by default; without a draw every call enqueues
 * exactly what it enqueues without this block.  Episode 0 (the state of hb_plant_reset) is never drawn.
 *
 * The draw.  Philox4x32-10, u_k = (word k + 0.5) 2^-32 as for the profile draw (above):
 *       key = (seed low 32, seed high 32) of THIS configuration's seed;  counter = (instance_offset + i, e, HB_FD_STREAM, block),
 * instance_offset from the respawn configuration in force, e = EPISODE_INDEX + 1 the episode that starts.  Every operation below is an
 * IEEE double operation of its own in the order written, brackets first, nothing fused; there is no transcendental function in it.  All
 * 258 blocks are independent and always generated.
 *   block 0:      kind = list[int(u_0 n)], list = the enabled kinds in ascending bit order, n their number;
 *                 A = amp_lo + (amp_hi - amp_lo) u_1;  p = slope_u_lo + (slope_u_hi - slope_u_lo) u_2;
 *                 r = slope_w_lo + (slope_w_hi - slope_w_lo) u_3.
 *   block 1:      mu_c = mu_lo + (mu_hi - mu_lo) u_c,  c = 0..3;  with mu_per_point = 0 all four points take c = 0's value.
 *   block 2 + k,  k = 0 .. 255:  word m is the uniform u_n of node n = 4 k + m in the PITCH numbering n = iu HB_FIELD_MAX_NODES + iw: the
 *                 draw of a node does not depend on (nu, nw).
 *   HB_FD_FLAT and HB_FD_TILT take A = 0;  HB_FD_FLAT and HB_FD_ROUGH take p = r = 0.
 * Composition.  a = (a_x, a_y) is the stored unit direction (dir / sqrt(dir_x dir_x + dir_y dir_y), the division of the terrain profile),
 * b = (-a_y, a_x), q_s = q_spawn[0:2] of the respawn configuration in force, gz = ground_z of the contact model, (nu, nw) = n_nodes,
 * (du, dw) = spacing, (cu, cw) = centre: the grid-local coordinates of the spawn point.
 *   origin:       u0 = (a_x q_s[0] + a_y q_s[1]) - cu;   w0 = ((-a_y) q_s[0] + a_x q_s[1]) - cw;
 *   node (iu, iw), iu < nu, iw < nw:   un = double(iu) du,  wn = double(iw) dw;
 *                 c = 0 if |un - cu| <= calm and |wn - cw| <= calm, else 1   (no bumps in the square around the spawn point);
 *                 g = (p (un - cu) + r (wn - cw)) + (A (2 u_n - 1)) c        (the height relative to the spawn point's level);
 *   plant:        heights[iu][iw] = 0 + (gz + g);  nodes beyond (nu, nw) store 0;
 *   map:          with follow_map the controller's field map takes 0 + g (0 beyond (nu, nw)) and the same eight header doubles
 *                 (a, u0, w0, du, dw, nu, nw).
 * What is stored — header, the facet under the world origin in its head, friction, heights — is what hb_plant_set_terrain_field stores
 * for n_nodes, dir, (u0, w0), spacing, these heights and mu, byte for byte (one routine, csrc/hb_contact.hpp field_compose, behind
 * both), and the map likewise what hb_ground_set_field stores (csrc/hb_ground.hpp ground_field_compose).
 *
 * row[HB_FD_N]: KIND (the bit value), AMPLITUDE = A, SLOPE_U = p, SLOPE_W = r, MUS[4].  Entries a kind does not use are 0 (FLAT:
 * AMPLITUDE, SLOPE_U, SLOPE_W; ROUGH: the slopes; TILT: AMPLITUDE).  Before an instance's first draw the row is zero (KIND 0).
 * Log: up to log_capacity rows of HB_FD_LOG_W doubles per instance, appended in order until full: the five leading entries of the profile
 * draw's log row (index, cause, TICKS, progress along a, TILT_MAX), then the HB_FD_N parameters the episode ran under.
 *
 * Placement on a field (k_plant_respawn, whenever a field is in force at a respawn): the vertical rule of the profile draw with the
 * field's facet in the segment's place.  Contact point c at p_c takes the facet under it (the cell and triangle rule of the height
 * field) with (n_c, d_c);  gap_c = ((n_x x + n_y y) + n_z z) - d;  D = max over c of (clearance - gap_c) / n_{c,z};  q[2] += D
 * (place = 0: no shift).  A vertical shift changes no (u, w), hence no facet.  On a level field D is the shift of step 3 on the level
 * plane, bit for bit.  After placement, either way, the kernel writes the facet ids under the four contact points and the base origin and
 * the Terrain record of the facet under the base origin (what hb_plant_reset's host locate writes), and the new episode record measures
 * height against that facet.
 *
 * Validity.  The device cannot refuse a draw, so the set call admits only configurations all of whose draws the height field accepts.
 * Let P = max(|slope_u_lo|, |slope_u_hi|), R likewise for w.  Two neighbouring nodes along u differ by p du + A (b' - b) with bump factors
 * b, b' in (-1, 1), so a triangle's u-slope is at most P + 2 amp_hi / du in magnitude and its w-slope at most R + 2 amp_hi / dw, before
 * rounding; the set call refuses unless (P + 2 amp_hi / du)^2 + (R + 2 amp_hi / dw)^2 <= 2.9.  Rounding: with spacing in [1e-3, 10], the
 * centre inside the grid and |gz| <= 1e3, |g| < 2^11 and |gz + g| < 2^12 (the grid spans at most 310 m, the slopes stay below 1.71, amp_hi below 8.6), so the eleven
 * roundings behind a stored height, each at most half an ulp of a number below 2^12, move it by less than 11 * 2^-42 < 2^-38 m, a
 * difference of two heights by less than 2^-37 m, a slope (spacing >= 1e-3) by less than 1e-8 and the sum of the two squares by
 * less than 4 * 1.71 * 1e-8 < 1e-7: far inside the 0.1 the bound 2.9 leaves below the field's limit 3.  The spacing is
 * positive, origin and heights are finite (|a . q_s|, |b . q_s| <= 1e3), the counts lie in 2 .. HB_FIELD_MAX_NODES, mu_c in [mu_lo, mu_hi].
 * HB_ERR_ARG (the configuration in force is kept) for: a non-finite field; kinds outside 1 .. 15; mu_per_point or follow_map not 0 / 1;
 * |dir| = 0; n_nodes outside 2 .. 32; spacing outside [1e-3, 10]; centre outside [0, (n - 1) spacing]; calm < 0; lo > hi in any range;
 * amp_lo < 0; mu_lo < 0; the slope bound above; log_capacity outside 0 .. HB_FD_LOG_MAX; a nonzero `reserved`.
 *
 * State.  HB_ERR_STATE before hb_plant_reset, outside contact model 1, without a respawn configuration in force, while a profile draw is
 * in force (and hb_plant_set_profile_draw while a field draw is: a height field is then in force), while a scenario with HB_SC_SLOPE or
 * HB_SC_MU is in force (the other order is refused by hb_plant_set_scenario: a field is then in force; PAYLOAD, MASS and PUSH combine
 * freely with the draw), with follow_map unless a FIELD map is in force (set the zero field map first; a profile map is refused), and
 * when |ground_z| or |a . q_s| or |b . q_s| of an instance exceeds 1e3.  Setting the draw puts every instance on the level field of the
 * configured grid (heights 0 + (gz + 0), cfg.mu) located at the plant's current state, replacing a terrain or a profile, clears the
 * contact impulses as hb_plant_set_terrain_field does, and restarts the rows and the log; with follow_map the controller's map becomes
 * the zero map over the same grid.  A configuration in force is switched off before the new one's arrays are allocated and written:
 * HB_ERR_ARG and HB_ERR_STATE keep it, HB_ERR_DEVICE leaves the draw off.  While the draw is in force hb_plant_set_terrain and every
 * hb_plant_set_terrain_field / hb_plant_set_terrain_profile, the switch-off calls included, return HB_ERR_STATE,
 * hb_plant_set_contact_model refuses a |ground_z| above 1e3 with HB_ERR_ARG, and hb_plant_get_terrain_field, hb_ground_get_field,
 * hb_plant_field_eval and hb_plant_reset read the device records first (the host copies are stale).  cfg NULL, turning respawn or the
 * episode off switch the draw off: field and map stay in force as last drawn, the host copies are refreshed, and respawn, if still on,
 * keeps placing on the field.  Leaving model 1 switches draw and field off.  hb_plant_reset empties the log; records and rows stay.
 * hb_plant_set_respawn with a field in force and hb_plant_set_terrain_field with a respawn in force stay refused: the draw is the one
 * way to a respawn on a field.
 * Out of scope: a draw for episode 0, a grid or a direction per episode, respawn on a field the host set, the instance-range / graph
 * paths, smoothed or correlated roughness. */
#define HB_FD_STREAM 0x46444431u /* third counter word; differs from HB_RS_STREAM, HB_SC_STREAM and HB_PD_STREAM */
enum { HB_FD_FLAT = 1, HB_FD_ROUGH = 2, HB_FD_TILT = 4, HB_FD_TILT_ROUGH = 8 }; /* kinds */
enum { HB_FD_KIND = 0, HB_FD_AMPLITUDE = 1, HB_FD_SLOPE_U = 2, HB_FD_SLOPE_W = 3, HB_FD_MUS = 4 /* [4] */, HB_FD_N = 8 }; /* row */
#define HB_FD_LOG_W (5 + HB_FD_N) /* finished episode's index, cause, TICKS, progress, TILT_MAX, then its HB_FD_N parameters */
#define HB_FD_LOG_MAX 1024
typedef struct hb_field_draw_config {
  uint64_t seed;
  int32_t kinds;              /* OR of HB_FD_*, at least one */
  int32_t mu_per_point;       /* 0: one coefficient for the four points; 1: one each */
  double dir[2];              /* |dir| > 0, normalised as the terrain profile normalises it */
  int32_t n_nodes[2];         /* (nu, nw), 2 .. HB_FIELD_MAX_NODES */
  double spacing[2];          /* (du, dw) m, in [1e-3, 10] */
  double centre[2];           /* grid-local (u, w) of the spawn point, inside the grid */
  double calm;                /* m, >= 0: half-width of the square around the spawn point without bumps */
  double amp_lo, amp_hi;      /* m, 0 <= lo <= hi: bump amplitude (a node moves by at most A) */
  double slope_u_lo, slope_u_hi, slope_w_lo, slope_w_hi; /* signed, lo <= hi: dz/du, dz/dw of the tilt */
  double mu_lo, mu_hi;        /* 0 <= lo <= hi */
  int32_t follow_map;         /* 0 / 1: the controller's field map follows the drawn field */
  int32_t log_capacity;       /* 0 .. HB_FD_LOG_MAX finished episodes kept per instance */
  int32_t reserved[2];        /* 0 */
} hb_field_draw_config;
/* cfg NULL: off. */
int32_t hb_plant_set_field_draw(hb_ctx* ctx, const hb_field_draw_config* cfg);
/* row[batch][HB_FD_N]: the parameters every instance's current ground was drawn with.  Synchronises like hb_plant_get_episode.
 * HB_ERR_STATE without a field draw in force. */
int32_t hb_plant_get_field_draw(hb_ctx* ctx, double* row);
/* count[batch] = rows logged per instance, log[batch][log_capacity][HB_FD_LOG_W] (rows behind count are zero); either may be NULL.
 * Synchronises.  HB_ERR_STATE without a field draw in force. */
int32_t hb_plant_get_field_draw_log(hb_ctx* ctx, int32_t* count, double* log);

/* ---- height scan: the controller's field map perceived from the plant's ground ----------------------------------------------------------
 * With a height scan in force, hb_plant_scan writes the controller's field map (hb_ground_set_field below) of every instance from the
 * ground the plant stands on, as an elevation sensor would: a robot-centred grid of limited range, noisy and with holes, registered with
 * the true or the estimated base position, that remembers what it saw once the ground is under the body.  One kernel (k_plant_scan, one
 * wavefront per instance); nothing crosses the bus.  Off by default; without a scan every call enqueues exactly what it enqueues without
 * this block, and the scan writes only the field map's arrays and its own.
 *
 * Notation for one scan of instance i.  Every line is an IEEE double operation of its own, in the order written, brackets first, nothing
 * fused.  p = q[0:3] of the plant;  e = p in register mode 0, e = the position rbd[3:6] of the resident observation in register mode 1;
 * a = the stored unit direction (dir / sqrt(dir_x dir_x + dir_y dir_y)), b = (-a_y, a_x);  (nu, nw) = n_nodes, (du, dw) = spacing;
 * gz = ground_z of the contact model.
 *   1. If any of p[0:3], e[0:3] is not finite, or |(a_x e_x + a_y e_y) / du| or |(b_x e_x + b_y e_y) / dw| is >= 2^30, the scan of this
 *      instance is skipped: header, heights, origin_index and returned stay as they are, n_returns = -1, and no float-to-int conversion of
 *      such a value is reached.
 *   2. ku = int(floor((a_x e_x + a_y e_y) / du)) - back[0];  kw likewise with b, dw, back[1];  org = (double(ku) du, double(kw) dw).  The
 *      map's header is that of hb_ground_set_field for n_nodes, a, org, spacing (csrc/hb_ground.hpp ground_field_compose).
 *   3. Node (iu, iw), iu < nu, iw < nw:  um = org_u + double(iu) du,  wm = org_w + double(iw) dw;  map point
 *      m = (a_x um + b_x wm, a_y um + b_y wm);  sample point s = m in mode 0,  s = (m - e_xy) + p_xy in mode 1.
 *   4. Truth: z_s is the height over s of the plane the plant would put a contact point at s on.  With the stored plane (n, d) of the
 *      segment of the terrain profile in force, of the instance's plane with a terrain in force, or n = e_z and d = gz otherwise:
 *      z_s = ((d - n_x s_x) - n_y s_y) / n_z.  With a height field in force the facet under s (the cell and triangle rule, one routine
 *      with the step) is read from the four stored heights of its cell, as hb_ground_eval reads a field map:
 *      z_s = z00 + e1 f1 + e2 f2 with the operands of hb_ground_set_field's height, taken from the plant's header and heights.  No unit
 *      normal lies between a stored height and the scanned one: a sample point on a node of the field returns that node's height bit for
 *      bit (through the facet's record it would return it to an ulp or two).
 *      h = z_s - gz in mode 0,  h = ((z_s - p_z) + e_z) - gz in mode 1.
 *   5. The node has a return iff (range == 0 or (s_x - p_x)^2 + (s_y - p_y)^2 <= range^2) and (dropout == 0 or u_n >= dropout).
 *   6. With a return the map stores 0 + (h + noise z_n); with noise == 0 the term is not added (0 + h): the ideal height bit for bit,
 *      whatever dropout is.
 *   7. Without a return the node keeps what the map held at that lattice node: the old height of node (iu + ku - ku_old, iw + kw - kw_old),
 *      or 0 if that index lies outside the old nu x nw or the map is cleared.  The map is cleared by hb_plant_set_height_scan (which zeroes
 *      the heights at once), by the first scan after hb_plant_reset, and, while a respawn configuration is in force, when
 *      itot[HB_RS_I_EPISODE_INDEX] of the instance differs from the value its last scan saw (the scan keeps that value per instance; the
 *      respawn kernels are not touched).  Nodes beyond (nu, nw) store 0.  The update is in place; all old heights of an instance are read
 *      before any is written.
 *   8. Philox4x32-10 and Box-Muller are those of hb_plant_sense, u = (word + 0.5) 2^-32:  key = (seed low 32, seed high 32);
 *      counter = (instance_offset + i, scan_count low 32, HB_HS_STREAM, block), scan_count = the hb_plant_scan calls since the set call
 *      (the first scan has 0).  Block k, k = 0 .. 255: the normals z_n of the nodes n = 4 k .. 4 k + 3 in the PITCH numbering
 *      n = iu HB_FIELD_MAX_NODES + iw (words (0, 1) give the first two, (2, 3) the other two); block 256 + k: word m is the uniform
 *      u_n of node 4 k + m.  A node's draw does not depend on (nu, nw); the blocks of a channel that is off (noise == 0, dropout == 0) are not
 *      generated.  A shard with instance_offset = the global index of its instance 0 reproduces its slice.
 *   9. Outputs per instance: origin_index = (ku, kw), n_returns, returned[n] (0 / 1, pitch numbering).
 * The scan does not run the steepness check of the field setters: the map's reader (ground_field_height) needs no normal, so a noisy map
 * of any steepness is valid.
 *
 * State.  hb_plant_set_height_scan returns HB_ERR_STATE before hb_plant_reset, outside contact model 1, without a FIELD map in force (set
 * the zero field map over the scan grid first, as for follow_map), while a field draw or a profile draw with follow_map is in force (their
 * set calls refuse a follow_map while a scan is in force), and with hb_set_chunks > 1 (hb_set_chunks refuses more than one while a scan is
 * in force).  While a scan is in force hb_ground_set_field and hb_ground_set_profile are refused and hb_ground_get_field reads the device
 * arrays first.  HB_ERR_ARG (the configuration in force is kept) for a field outside the ranges below or a non-finite one.  cfg NULL: off;
 * the map last written stays in force.  hb_plant_scan runs on the stream of the plant, between the ordering points of a writer of the
 * resident observation; it does not synchronise and invalidates no captured graph.  hb_plant_get_height_scan synchronises; every
 * pointer may be NULL.
 * Out of scope: yaw-aligned grids, attitude error in the registration, occlusion, the instance-range / graph paths. */
#define HB_HS_STREAM 0x48535331u /* third counter word; differs from HB_RS_STREAM, HB_SC_STREAM, HB_PD_STREAM and HB_FD_STREAM */
typedef struct hb_height_scan_config {
  int32_t n_nodes[2];     /* (nu, nw), 2 .. HB_FIELD_MAX_NODES: the scan grid = the field map it writes */
  int32_t back[2];        /* cells of the grid behind / right of the cell the registration point is in, 0 .. n - 2 */
  double dir[2];          /* direction a of the grid, |dir| > 0, normalised as the terrain profile normalises it */
  double spacing[2];      /* (du, dw) > 0 */
  double range;           /* >= 0; 0: no limit.  A node farther than this, horizontally, from the TRUE base has no return */
  double noise;           /* >= 0: standard deviation of the additive height noise per return, m */
  double dropout;         /* 0 <= dropout < 1: probability that a return is lost */
  int32_t register_mode;  /* 0: the map is registered with the plant's base position; 1: with the resident estimate (translation only) */
  int32_t reserved;       /* 0 */
  uint64_t seed;
  uint32_t instance_offset;
  int32_t pad;            /* 0 */
} hb_height_scan_config;
/* cfg NULL: off; the map last written stays in force. */
int32_t hb_plant_set_height_scan(hb_ctx* ctx, const hb_height_scan_config* cfg);
/* One scan of every instance, enqueue-only.  HB_ERR_STATE without a scan in force. */
int32_t hb_plant_scan(hb_ctx* ctx);
/* cfg: the configuration in force (dir as stored); origin_index[batch][2]; n_returns[batch]; returned[batch][32 * 32] in the pitch
 * numbering, all as the last scan left them (zero before the first).  HB_ERR_STATE without a scan in force. */
int32_t hb_plant_get_height_scan(hb_ctx* ctx, hb_height_scan_config* cfg, int32_t* origin_index, int32_t* n_returns, uint8_t* returned);

/* ---- sensors from the plant: what LeggedController::updateStateEstimation reads, computed on the device -----------
 * hb_plant_sense turns the plant's state into the sensor arrays of hb_estimator_update and leaves them on the device
 * (plant-owned arrays [batch][4|3|3|10|10|10] and int [batch][4]); hb_estimator_update_resident /
 * hb_estimator_contact_force_resident consume them where they lie, so that plant -> sensors -> estimator -> MPC -> WBC -> joint
 * command -> plant never crosses PCIe.  Per instance, from q, v, the last acceleration vdot, and the torque and contact flags the last
 * hb_plant_step applied (before the first step after hb_plant_reset: vdot = 0, torque = 0, all four flags 1):
 *   quat[4] (x y z w) of the base from the ZYX half angles (c. / s. = cos / sin of yaw/2, pitch/2, roll/2):
 *       x = cz cy sx - sz sy cx,  y = cz sy cx + sz cy sx,  z = sz cy cx - cz sy sx,  w = cz cy cx + sz sy sx,  negated if w < 0;
 *   ang_vel_local[3] = R' E(zyx) v[3:6];   lin_acc_local[3] = R' (vdot[0:3] + g e_z) with g = hb_model.gravity (specific force);
 *   joint_pos[10] = q[6:];  joint_vel[10] = v[6:];  joint_torque[10] = the torque the last hb_plant_step integrated (the host tau or the
 *   hb_joint_command torque);  contact_flag[4] = the flags that step applied.
 * Imperfections (hb_plant_set_sensor_model): constant per-instance biases on the gyroscope and the accelerometer, added first, then
 * zero-mean Gaussian noise.  The generator is Philox4x32-10, counter based, without state on the device:
 *   key = (seed low 32, seed high 32);  counter = (instance_offset + i, sense_count low 32, sense_count high 32, block), where
 *   sense_count is the number of hb_plant_sense calls of this context since hb_plant_set_sensor_model (a 64-bit host count).
 *   A block of four words gives four standard normals by Box-Muller with u = (word + 0.5) 2^-32:
 *   (w0, w1) -> r cos(2 pi u1), r sin(2 pi u1), r = sqrt(-2 ln u0); (w2, w3) likewise.  Normal n is lane n % 4 of block n / 4:
 *   orientation 0-2, gyro 3-5, accel 6-8, joint_pos 9-18, joint_vel 19-28, joint_torque 29-38.
 * A channel with sigma = 0 is the ideal value bit for bit whatever the other channels are set to; blocks no channel needs are not
 * generated.  Contact flags are never corrupted.  A seed of 0 is valid.  Same seed, same instance_offset + i, same sense_count: same
 * bits, so a shard (instance_offset = global index of its instance 0) reproduces its slice of the unsharded batch. */
typedef struct hb_sensor_config {
  double orientation_noise;   /* rad: rotation vector delta = sigma * z (3 normals), quat <- quat (x) [delta/|delta| sin(|delta|/2), cos(|delta|/2)], w >= 0 */
  double gyro_noise, accel_noise, joint_pos_noise, joint_vel_noise, joint_torque_noise;   /* standard deviations, additive */
  uint64_t seed;
  uint32_t instance_offset;   /* global index of instance 0 of this context: a shard reproduces the unsharded batch */
  int32_t reserved;           /* 0 */
} hb_sensor_config;
/* cfg NULL: ideal sensors (no noise).  gyro_bias / accel_bias [batch][3], either may be NULL = zero.  Restarts sense_count at 0.
 * The model survives hb_plant_reset.  HB_ERR_STATE before hb_plant_reset; HB_ERR_ARG for a negative or non-finite sigma or a nonzero
 * `reserved` (the model in force is kept). */
int32_t hb_plant_set_sensor_model(hb_ctx* ctx, const hb_sensor_config* cfg, const double* gyro_bias, const double* accel_bias);
/* One reading of every instance on the WBC stream, left on the device; host out (any may be NULL): quat[batch][4],
 * ang_vel_local[batch][3], lin_acc_local[batch][3], joint_pos / joint_vel / joint_torque [batch][10], contact_flag[batch][4].  With every
 * pointer NULL the call is enqueue-only.  HB_ERR_STATE before hb_plant_reset. */
int32_t hb_plant_sense(hb_ctx* ctx, double* quat, double* ang_vel_local, double* lin_acc_local, double* joint_pos, double* joint_vel,
                       double* joint_torque, int32_t* contact_flag);

/* ---- device-resident stepping (bench / rollouts; inputs already in HBM) ------------------------
 * hb_step_resident runs hb_mpc_solve(NULL) + hb_mpc_publish + WBC on device-resident t_now/rbd that
 * were uploaded once with hb_set_resident_inputs; nothing crosses PCIe. */
int32_t hb_set_resident_inputs(hb_ctx* ctx, const double* x0, const double* t_now, const double* rbd,
                               const int32_t* walk_flag);
/* The device-resident controller time alone ([batch], host).  hb_plant_step(to_resident) advances it by itself; an estimator
 * with to_resident (which replaces the resident observation and rbd state but knows no clock) leaves it to the caller.
 * Enqueue-only (pinned staging, no device synchronisation). */
int32_t hb_set_resident_time(hb_ctx* ctx, const double* t_now);
int32_t hb_step_resident(hb_ctx* ctx, double dt);
/* One whole tick on the resident state, enqueue-only: hb_set_resident_time(t_now) + hb_estimator_update(dt_est, sensors,
 * to_resident) + hb_refgen_update(t_now, horizon, x_now = the estimate, cmd_vel) + hb_step_resident(dt_wbc) — what
 * LeggedController::update and its MPC thread do per MPC period (LeggedController.cpp:137-185, 396-412) for the whole batch.  With
 * instance ranges (hb_set_chunks > 1) every range runs its slice of ALL of it on its own stream, tick after tick, without a
 * whole-batch stage between two steps; results are identical to the four calls.  Host arrays as in hb_estimator_update /
 * hb_refgen_update; they are the caller's again on return (pinned staging). */
int32_t hb_tick_resident(hb_ctx* ctx, double dt_est, const double* quat, const double* ang_vel_local, const double* lin_acc_local,
                         const double* joint_pos, const double* joint_vel, const int32_t* contact_flag, const double* t_now,
                         double horizon, const double* cmd_vel, double dt_wbc);
/* Optional: a device-resident cyclic sequence of measured states x0_seq[n_seq][batch][22]; step k of
 * hb_step_resident starts its MPC solve from x0_seq[k % n_seq] (emulates the estimator feeding a new state each
 * MPC call, LeggedController.cpp:141-144).  n_seq = 0 disables it. */
int32_t hb_set_resident_x0_sequence(hb_ctx* ctx, int32_t n_seq, const double* x0_seq);
int32_t hb_get_wbc_solution(hb_ctx* ctx, double* sol /*[batch][38]*/, int32_t* status /*[batch]*/);
/* Active-set iterations of the last WBC solve of every instance (constraint additions + drops of the dual active-set
 * method; the role of nWSR at WeightedWbc.cpp:51-55).  iters: [batch]. */
int32_t hb_get_wbc_iterations(hb_ctx* ctx, int32_t* iters /*[batch]*/);
/* KKT certificate and dual solution of the WeightedWbc QP (hb_config.wbc_type = 0), per instance, computed inside the WBC kernel
 * right after the solve.  The QP is the reference's (legged_wbc/src/WeightedWbc.cpp:24-41) WITHOUT the Tikhonov term:
 *   min 1/2 x'H x + g'x,  H = A_w'A_w, g = -A_w'b_w (every weighted task incl. the contact forces; the stance task in stance mode),
 *   rows A = [EoM 16 ; zero force 3 n_sw ; torque limits 20 ; friction pyramid 5 n_c ; 3 n_sw all-zero rows] in the order qpOASES
 *   receives them (56 / 58 / 60 rows), each an equality or "<= f",
 * evaluated at the sol the call returned (the previous solution when the solve failed).  The multipliers y are the least-squares
 * solution  argmin |Hx + g - A_W'y_W|_2  on the solver's final working set W (equalities always in W).
 * Sign convention: Hx + g - A'y = 0, y_i <= 0 on active upper-bounded rows (qpOASES getDualSolution's convention as far as known;
 * the reference never reads the dual).  dual[HB_WBC_NCONS_MAX] holds y in the row order above; rows outside W, the all-zero rows
 * and the padding are zero.
 * hb_wbc_set_certificate: 0 (default) / 1.  Every later WBC launch (hb_wbc_update, hb_wbc_update_direct, hb_step_resident,
 * hb_tick_resident, with or without hb_set_chunks) runs the certificate kernel; sol / status / iterations are bit-identical either
 * way.  Switching re-captures the range graphs.  HB_ERR_ARG when enabling on a HierarchicalWbc context (wbc_type = 1).
 * hb_wbc_get_certificate: the certificates of instances [inst_begin, inst_begin + inst_count) from the last WBC call (synchronises
 * the WBC stream); cert [count][HB_WBC_CERT_SIZE], dual [count][HB_WBC_NCONS_MAX], either may be NULL.  HB_ERR_STATE if certificates
 * were off at that call (or no WBC call ran since they were enabled). */
#define HB_WBC_CERT_R_EQ 0      /* max |A_E x - b_E| over the EoM and zero-force rows */
#define HB_WBC_CERT_R_IN 1      /* max(0, max(D x - f)) */
#define HB_WBC_CERT_R_STAT 2    /* |H x + g - A'y|_inf */
#define HB_WBC_CERT_R_DUAL 3    /* max(0, max y_i) over the inequality rows (sign violation) */
#define HB_WBC_CERT_R_COMP 4    /* max |y_i (D x - f)_i| over the inequality rows */
#define HB_WBC_CERT_N_ACTIVE 5  /* size of the final working set, equalities included */
#define HB_WBC_CERT_EPS 6       /* the Tikhonov term the problem was solved with (wbc_eps_reg, or the norm-scaled value) */
#define HB_WBC_CERT_SCALE 7     /* max(1, |g|_inf, |H x|_inf): relative figures are r / scale */
#define HB_WBC_CERT_SIZE 8
#define HB_WBC_NCONS_MAX 60
int32_t hb_wbc_set_certificate(hb_ctx* ctx, int32_t enable);
int32_t hb_wbc_get_certificate(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, double* cert /*[count][8]*/,
                               double* dual /*[count][60]*/);
/* Per-level optimality certificate of the HierarchicalWbc cascade (hb_config.wbc_type = 1), per instance, computed inside the WBC kernel
 * right after the solve.  Levels k = 0, 1, 2 with the tasks A_k x = b_k of HierarchicalWbc.cpp:23-27 and the shared
 * inequality rows D x <= f of level 0 (torque limits 20, friction pyramid 5 n_c; n_in <= HB_HWBC_NINEQ_MAX), WITHOUT the Tikhonov terms
 * and without the 1e-12 Hessian shift:
 *   x_k       the solution after level k (x_2 = the returned sol);  v0 = (D x_0 - f)_+ the level-0 slack;  g_k = A_k'(A_k x_k - b_k);
 *   Q_k       an ORTHONORMAL basis of the level's search space: Q_0 = I, Q_1 spans kernel(A_0), Q_2 spans kernel([A_0; A_1]) (thin QR of
 *             the kernel bases the cascade holds), so no figure depends on the basis the solver happened to use;
 *   y_k       the multipliers of the inequality rows, g - D'y = 0, y <= 0 on active rows: y_0 = -v0 (the slacked rows' multipliers are
 *             the slack), y_k = argmin |Q_k'(g_k - D_W'y_W)|_2 on the final working set W of the level's QP for k >= 1, zero outside W.
 * A level the cascade did not reach (a kernel basis was given up: status != 0, previous solution kept) is judged at the returned sol
 * with N_FREE = N_ACTIVE = 0, y = 0 and the UNPROJECTED |g_k|_2 as R_STAT, so it never looks certified; every field stays finite.
 * hb_hwbc_set_certificate: 0 (default) / 1.  Every later WBC launch (hb_wbc_update, hb_wbc_update_direct, hb_step_resident,
 * hb_tick_resident, with or without hb_set_chunks) runs the certificate kernel; sol / status and the resident outputs are bit-identical
 * either way.  Switching re-captures the range graphs.  HB_ERR_ARG on a WeightedWbc context (wbc_type = 0: hb_wbc_set_certificate).
 * hb_hwbc_get_certificate: instances [inst_begin, inst_begin + inst_count) of the last WBC call (synchronises the WBC stream);
 * cert [count][3][HB_HWBC_CERT_SIZE], x_levels [count][3][38], slack0 [count][40] (v0), dual [count][3][40] (y_k by inequality row),
 * any may be NULL; rows >= n_in are zero.  HB_ERR_STATE if certificates were off at that call (or no WBC call ran since they were
 * enabled), HB_ERR_ARG for a bad range. */
#define HB_HWBC_LEVELS 3
#define HB_HWBC_NINEQ_MAX 40
#define HB_HWBC_CERT_RES_OWN 0    /* |A_k x_k - b_k|_2: the optimum of this priority */
#define HB_HWBC_CERT_RES_FINAL 1  /* |A_k x_2 - b_k|_2: what the returned solution achieves */
#define HB_HWBC_CERT_R_HIER 2     /* max_{j<k} |A_j (x_k - x_{k-1})|_inf: the step of this level seen by every higher task; 0 for k = 0 */
#define HB_HWBC_CERT_R_IN 3       /* max(0, max(D x_k - f - v0)) */
#define HB_HWBC_CERT_R_STAT 4     /* |Q_k'(g_k - D'y_k)|_2 */
#define HB_HWBC_CERT_R_DUAL 5     /* max(0, max y_k) (sign violation) */
#define HB_HWBC_CERT_R_COMP 6     /* max |y_k o (D x_k - f - v0)| */
#define HB_HWBC_CERT_N_FREE 7     /* columns of Q_k (38, 10..12, <= 6) */
#define HB_HWBC_CERT_N_ACTIVE 8   /* |W| (level 0: rows with v0 > 0) */
#define HB_HWBC_CERT_SCALE 9      /* max(1, |A_k'b_k|_inf, |A_k'A_k x_k|_inf): R_STAT, R_DUAL, R_COMP are read relative to it */
#define HB_HWBC_CERT_SIZE 10
int32_t hb_hwbc_set_certificate(hb_ctx* ctx, int32_t enable);
int32_t hb_hwbc_get_certificate(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, double* cert /*[count][3][10]*/,
                                double* x_levels /*[count][3][38]*/, double* slack0 /*[count][40]*/, double* dual /*[count][3][40]*/);
/* KKT certificate, costates and stage-QP export of the MPC's Riccati solve, per instance, ON DEMAND: there is no switch, and
 * hb_mpc_solve / hb_step_resident / hb_tick_resident enqueue nothing for it; the two certificate kernels run inside
 * hb_mpc_get_certificate on what a solve leaves on the device (the projected stage records, the gains, the step).
 *
 * The certificate covers one instance with n intervals.  The data are those of the LAST SQP iteration of the last MPC call, as
 * stored in the records.  Padded input columns are included: R~ = I, zero elsewhere, so they contribute exactly zero.  The start
 * state is dx_0 as stored (the solve makes it 0).
 *   u~_k = K~_k dx_k + k~_k, 12 entries, recomputed from the gains and dx: what the forward sweep applied.
 *   Costates, backward over the stages:  lambda_n = 0 (there is no terminal cost: the backward sweep starts from S = 0),
 *       lambda_k = q~_k + Q~_k dx_k + P~_k' u~_k + A~_k' lambda_(k+1),
 *   the multiplier of dx_(k+1) = A~_k dx_k + B~_k u~_k + b~_k in the Lagrangian
 *       cost + sum lambda_(k+1)' (A~ dx + B~ u~ + b~ - dx_(k+1));    lambda_0 = dV/dx_0.
 *   R_DYN uses all 22 rows of the record; the forward sweep forms the joint rows 12..21 in closed form, so this residual is the
 *   cross-check between the two forms the two sweeps use.  R_STAT is the input stationarity; state stationarity holds by
 *   construction of lambda.  OBJ is the QP objective at the step; it has no sign guarantee (b~ != 0).  SCALE has NO floor at 1: the
 *   stage costs carry a factor dt, so a floor would hide 300 x on a standing robot; R_STAT is read relative to SCALE.
 * An instance whose status word of that MPC call is HB_INST_NAN is not certified: N_NODES = 0, fields 0-6 NaN, its costate and u~
 * rows zero.  HB_INST_MAXITER is certified as usual (the line search rejected the step, but the QP solution is what it is).
 * Out of scope: the unprojected problem and the multipliers of the equality constraints (C, D, e are not in the record), the
 * nonlinear problem's KKT, the WBC (hb_wbc_set_certificate / hb_hwbc_set_certificate).
 *
 * hb_mpc_get_certificate: joins the instance-range streams as the other getters do, runs the certificate kernels for
 * [inst_begin, inst_begin + inst_count) on the MPC stream, synchronises it and copies.  cert [count][HB_MPC_CERT_SIZE],
 * costate [count][max_nodes+1][22] (lambda_0 .. lambda_n), u_til [count][max_nodes][12]; any may be NULL; rows k >= n_i (costate: k > n_i)
 * are zero.  The work buffers are allocated on the first call.
 * hb_mpc_get_lq: the stage QP of one instance, unpacked on the host into dense row-major arrays in the standard OCP-QP layout
 * (A, B, b, Q, S = P, R, q, r: what HPIPM takes), n_til = projected inputs per stage; any pointer may be NULL; rows k >= n are zero.
 * hb_mpc_get_recovery: the rest of the same instance's records, copied as stored: what turns the projected input u~ of the stage QP back
 * into the full input step, and what the line search reads.  The stage QP above is the unprojected node LQ (dynamics A, B, b; cost
 * Q, P, R, q, r, scaled by dt; equality constraints C dx + D du + e = 0) after the change of input variables
 *       du = T u~ + K dx + k      (du [22]: 12 contact forces, foot by foot, then 10 joint rates)
 *   T [22][12]: column a < n_f is the unit vector of the a-th force row of the contact feet, taken in foot order (3 rows per contact
 *       foot of the mode); column n_f + b, b < n_z, holds Z[:, b] under the joint-rate rows 12..21; the columns behind n_f + n_z are zero.
 *       The columns of T span the null space of D.
 *   K [22][22] = [0 ; Kx] and k [22] = [dF ; ke]: dF = -F on the swing feet (their force is constrained to zero) and 0 on the contact
 *       feet; (Kx, ke) is the basic least-squares solution of the velocity rows of the constraints for the joint rates.
 *   Hence A~ = A + B K, B~ = B T, b~ = b + B k, R~ = T'RT (+ I on the padding), P~ = T'(P + R K), Q~ = Q + K'P + P'K + K'RK,
 *   r~ = T'(r + R k), q~ = q + K'r + (P' + K'R) k.
 *   Kx [max_nodes][10][22], ke [..][10], Z [..][10][6] (columns >= n_z zero), dF [..][12], qf [..][22] and rf [..][22] (the unprojected
 *   cost gradients q and r, scaled by dt), meta [..][6] (n_f, n_z, mode, cost dt, dyn_sse dt = dt |b|^2, eq_sse dt = dt |e|^2),
 *   dt [max_nodes] (interval length), dq [..][10] (the joint rows of b); any pointer may be NULL; rows k >= n are zero.
 * hb_mpc_get_linesearch: the state of the filter line search of the LAST SQP iteration of the last MPC call for the instances
 * [inst_begin, inst_begin + inst_count), copied as the kernels left it (read only: nothing is launched and nothing changes):
 *   acc [count][4]: the Armijo directional derivative sum_k qf_k'dx_k + rf_k'du_k, then the baseline merit, dyn_sse, eq_sse (each a sum
 *       of the records' meta[3..5] in node order) -- what the filter compares every trial with;
 *   partial [count][max_nodes][3]: per node (dt cost, dt |defect|^2, dt |eq|^2) at the trial point x + dx, u + du (step size 1);
 *   ls_tail [count][HB_LS_TAIL_MAX][max_nodes][3]: the same at the step sizes of the LAST window of the backtracking tail that
 *       evaluated the instance: row j of window w holds step size alpha_decay^(16 w + j + 1) (running product).  A window evaluates
 *       at most HB_LS_TAIL_MAX step sizes >= alpha_min and none below the deltaTol stop; the rows behind them, the rows of nodes
 *       k >= n and every row of an instance that accepted earlier keep what an earlier window, iteration or call wrote (stale);
 *   ls_norm [count][2]: |dx|_2 over (n + 1) 22 entries and |du|_2 over n 22 entries, written when the full step is refused (stale
 *       for an instance that accepted it);
 *   accepted [count]: 0 = no step size accepted (alpha_min reached, or Riccati failure), 1 = step taken, 2 = stopped on deltaTol;
 *   ric_fail [count]: 1 = the backward sweep met a non-positive pivot.
 *   Any pointer may be NULL.  The sums the decisions were taken on are per lane l the sum over nodes l, l + 64, ... followed by the
 *   wave reduction v[l] += v[l + off], off = 32 .. 1; hb_mpc_get_performance returns them for the accepted step size.
 * hb_mpc_get_linesearch_refused: *count = how many instances of the batch that iteration refused the full step of and handed to the
 *   backtracking tail (the length of the tail's work list; Riccati failures included).
 * All five: HB_ERR_STATE when no MPC call has completed, or when the node tables or the iterate were replaced since the last one
 * (hb_mpc_set_references, hb_refgen_update, hb_mpc_reset, hb_mpc_reset_masked, hb_mpc_set_trajectory); HB_ERR_ARG on a bad range. */
#define HB_LS_TAIL_MAX 16         /* step sizes one window of the backtracking tail evaluates side by side */
#define HB_MPC_CERT_R_DYN 0       /* max(|dx_0|_inf, max_k |dx_(k+1) - (A~_k dx_k + B~_k u~_k + b~_k)|_inf) */
#define HB_MPC_CERT_R_STAT 1      /* max_k |r~_k + P~_k dx_k + R~_k u~_k + B~_k' lambda_(k+1)|_inf */
#define HB_MPC_CERT_OBJ 2         /* sum_k q~'dx + r~'u~ + 1/2 dx'Q~dx + u~'P~dx + 1/2 u~'R~u~ */
#define HB_MPC_CERT_STEP_MAX 3    /* max_k |dx_k|_inf */
#define HB_MPC_CERT_U_MAX 4       /* max_k |u~_k|_inf */
#define HB_MPC_CERT_LAMBDA_MAX 5  /* max_k |lambda_k|_inf */
#define HB_MPC_CERT_SCALE 6       /* max_k max(|r~_k|_inf, |P~_k dx_k|_inf, |R~_k u~_k|_inf, |B~_k' lambda_(k+1)|_inf) */
#define HB_MPC_CERT_N_NODES 7     /* the n covered; 0 = not certified */
#define HB_MPC_CERT_SIZE 8
int32_t hb_mpc_get_certificate(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, double* cert /*[count][8]*/,
                               double* costate /*[count][max_nodes+1][22] or NULL*/, double* u_til /*[count][max_nodes][12] or NULL*/);
int32_t hb_mpc_get_lq(hb_ctx* ctx, int32_t inst, double* A /*[max_nodes][22][22]*/, double* B /*[..][22][12]*/, double* b /*[..][22]*/,
                      double* Q /*[..][22][22], full symmetric*/, double* P /*[..][12][22]*/, double* R /*[..][12][12]*/,
                      double* q /*[..][22]*/, double* r /*[..][12]*/, int32_t* n_til /*[max_nodes]*/);
int32_t hb_mpc_get_recovery(hb_ctx* ctx, int32_t inst, double* Kx /*[max_nodes][10][22]*/, double* ke /*[..][10]*/, double* Z /*[..][10][6]*/,
                            double* dF /*[..][12]*/, double* qf /*[..][22]*/, double* rf /*[..][22]*/, double* meta /*[..][6]*/,
                            double* dt /*[max_nodes]*/, double* dq /*[..][10]*/);
int32_t hb_mpc_get_linesearch(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, double* acc /*[count][4]*/,
                              double* partial /*[count][max_nodes][3]*/, double* ls_tail /*[count][16][max_nodes][3]*/,
                              double* ls_norm /*[count][2]*/, int32_t* accepted /*[count]*/, int32_t* ric_fail /*[count]*/);
int32_t hb_mpc_get_linesearch_refused(hb_ctx* ctx, int32_t* count);
/* Pipelining of hb_step_resident: the batch is cut into n_chunks (1..8) instance ranges, each a linear
 * MPC -> publish -> WBC sequence on its own HIP stream so that the per-instance sweeps of one range overlap the
 * per-node kernels of another.  Results are identical for every n_chunks; hb_get_stats phase times are only
 * recorded with n_chunks = 1 (the default).
 * THREADING: hb_tick_resident and hb_step_resident with n_chunks > 1 are SINGLE-THREAD entry points — they share the pinned
 * staging rings and the lazy range join with the enqueue-only calls (hb_set_resident_time, hb_estimator_update, hb_refgen_update),
 * which are not locked.  The two-thread split of hb_last_error's note (MPC thread / control thread) applies to n_chunks = 1 and
 * the non-resident entry points only; do not mix it with chunked stepping on one context. */
int32_t hb_set_chunks(hb_ctx* ctx, int32_t n_chunks);

/* ---- state estimator (the step immediately before the path every tick) ------------------
 * Batched KalmanFilterEstimate::update (legged_estimation/src/LinearKalmanFilter.cpp:72-184): 18-state
 * [base pos, base vel, 4 foot positions] / 28-measurement linear Kalman filter on leg kinematics, preceded by the
 * sensor packing of StateEstimateBase::{updateJointStates, updateImu} (StateEstimateBase.cpp:73-106) and followed by
 * the centroidal-state conversion + yaw unwrapping of LeggedController::updateStateEstimation
 * (LeggedController.cpp:331-334).  The filter state (xHat[18], P[18][18], last yaw) is device-resident per
 * instance.  ROS topics / tf (updateFromTopic) and the contact-force estimator are not part of this entry point. */
typedef struct hb_estimator_config {  /* task.info kalmanFilter block (:336-345); LinearKalmanFilter.h:50-56 */
  double foot_radius;
  double imu_process_noise_position, imu_process_noise_velocity, foot_process_noise_position;
  double foot_sensor_noise_position, foot_sensor_noise_velocity, foot_height_sensor_noise;
  /* task.info contactForceEsimation block (:347-351), StateEstimateBase::loadSettings (StateEstimateBase.cpp:365-377) */
  double contact_force_cutoff_frequency;   /* lambda of the momentum observer's low pass (hb_estimator_contact_force) */
  double contact_threshold;                /* normal force above which estContactState would call a leg "in contact" (:206-226) */
} hb_estimator_config;
/* (Re)initialise: xHat = x_hat0 (or zeros if NULL), P = 100 I, last yaw = 0 (LinearKalmanFilter.cpp:31-60). */
int32_t hb_estimator_reset(hb_ctx* ctx, const hb_estimator_config* cfg, const double* x_hat0 /*[batch][18] or NULL*/);
/* One filter step for every instance.  Host in: quat[batch][4] (x y z w), ang_vel_local[batch][3],
 * lin_acc_local[batch][3], joint_pos[batch][10], joint_vel[batch][10], contact_flag[batch][4] (contact order
 * L_f1 R_f1 L_f2 R_f2).  Host out (either may be NULL): rbd[batch][32] (the vector WbcBase::update takes),
 * x_state[batch][22] (the MPC observation state).  to_resident != 0 additionally stores both into the
 * device-resident inputs of hb_step_resident, so that estimate -> MPC -> WBC never leaves the GPU.
 * With rbd == NULL and x_state == NULL the call is ENQUEUE-ONLY (sensor arrays through pinned staging, no device
 * synchronisation; see hb_refgen_update). */
int32_t hb_estimator_update(hb_ctx* ctx, double dt, const double* quat, const double* ang_vel_local,
                            const double* lin_acc_local, const double* joint_pos, const double* joint_vel,
                            const int32_t* contact_flag, int32_t to_resident, double* rbd, double* x_state);
/* StateEstimateBase::setCmdTorque + estContactForce (legged_estimation/src/StateEstimateBase.cpp:130-206), which
 * LeggedController::updateStateEstimation runs every tick behind the filter update (LeggedController.cpp:344-345): a
 * generalised-momentum observer for the disturbance torque (low pass exp(-cutoff dt) from hb_estimator_config, state per
 * instance on the device, zeroed by hb_estimator_reset) and, per leg, the minimum-norm wrench at its first contact frame
 * (L_f1 / R_f1).  rbd [batch][32] or NULL = the state the last hb_estimator_update left on the device;
 * joint_torque [batch][10] = the measured joint efforts.  Out (either may be NULL): est_disturbance_torque [batch][16]
 * (estDisturbancetorque_), est_contact_force [batch][16] = [wrench leg 0 (force 3, moment 3) | wrench leg 1 | |F0| |F1| |
 * |W0| |W1|] (estContactforce_).  In the reference nothing reads these values (estContactState, their only reader, is
 * never called); they are provided for the same diagnostics. */
int32_t hb_estimator_contact_force(hb_ctx* ctx, double dt, const double* rbd, const double* joint_torque,
                                   double* est_disturbance_torque, double* est_contact_force);
/* The two calls above on the arrays the last hb_plant_sense left on the device — no sensor crosses PCIe, nothing is copied: the same
 * filter kernel reads the plant's sensor arrays in place.  hb_estimator_update_resident is hb_estimator_update (rbd / x_state /
 * to_resident as there; without host outputs enqueue-only); hb_estimator_contact_force_resident is
 * hb_estimator_contact_force(rbd = NULL) on the sensed joint torque (without host outputs enqueue-only).  Both run on the WBC
 * stream.  HB_ERR_STATE before hb_plant_reset, before hb_estimator_reset, or before the first hb_plant_sense after hb_plant_reset. */
int32_t hb_estimator_update_resident(hb_ctx* ctx, double dt, int32_t to_resident, double* rbd, double* x_state);
int32_t hb_estimator_contact_force_resident(hb_ctx* ctx, double dt, double* est_disturbance_torque, double* est_contact_force);
/* Filter state to the host (either may be NULL): x_hat[batch][18], P[batch][18][18]. */
int32_t hb_estimator_get_filter(hb_ctx* ctx, double* x_hat, double* P);

/* ---- reference generation on the device ---------------------------------------------------
 * What SwitchedModelReferenceManager::modifyReferences (SwitchedModelReferenceManager.cpp:136-171) produces before
 * every MPC call, for the whole batch, written straight into the node tables hb_mpc_set_references would upload:
 * 2-knot target from cmd_vel (TargetTrajectoriesPublisher.h:101-131), event-clipped shooting grid, swing planner
 * (footholds: SwingTrajectoryPlanner::calNextFootPos; x/y/z multi-node cubic splines: genSwingTrajs,
 * SwingTrajectoryPlanner.cpp:164-358).  The gait scheduler (GaitSchedule.cpp:57-161, a few integers and event times per
 * instance) runs on the host by default — its output, the mode schedule, is an input (hb_refgen_set_schedule) — or on the device
 * (hb_gait_reset, below).  With joint_ik the targets are resampled
 * every 0.15 s and their joint part replaced by the inverse kinematics of the planned foot positions
 * (calculateJointRef), warm-started knot to knot. */
#define HB_MAX_EVENTS 64
typedef struct hb_refgen_config {  /* reference.info comHeight / defaultJointState, task.info swing_trajectory_config */
  double dt, com_height, next_position_z, swing_height, swing_time_scale;
  double feet_bias[HB_NC][3];      /* (feet_bias_x1|x2, +-feet_bias_y, feet_bias_z) in contact order */
  double default_joints[HB_NJ];
  int32_t joint_ik;                /* 1: per-knot joint reference by inverse kinematics (calculateJointRef,
                                      SwitchedModelReferenceManager.cpp:251-300; InverseKinematics.cpp:20-231), 0: defaultJointState */
  int32_t reserved;
} hb_refgen_config;
/* Planner state: latest_stance[batch][4][3] (SwingTrajectoryPlanner::latestStanceposition_), or NULL to take the
 * current foot positions at the first hb_refgen_update. */
int32_t hb_refgen_reset(hb_ctx* ctx, const hb_refgen_config* cfg, const double* latest_stance);
/* Mode schedule of instances [inst_begin, inst_begin + inst_count): n_events[i] <= HB_MAX_EVENTS event times
 * (strictly increasing) and n_events[i] + 1 modes; arrays strided by HB_MAX_EVENTS / HB_MAX_EVENTS + 1. */
int32_t hb_refgen_set_schedule(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, const int32_t* n_events,
                               const double* event_times, const int32_t* modes);
/* Generate the references of every instance for the horizon [t0[i], t0[i] + horizon].  x_now[batch][22] is the
 * observation (NULL: the device-resident x0, e.g. the estimator's output); cmd_vel[batch][4] = (vx, vy, vz, yaw rate).
 * status[batch] (may be NULL): 0 ok, 1 a swing phase runs out of the schedule, 2 grid longer than max_nodes.
 * With status == NULL the call is ENQUEUE-ONLY: the host arrays are copied into library-owned pinned staging (they are the
 * caller's again on return), no device synchronisation takes place, and the status words are read later with
 * hb_refgen_get_status — a driver that feeds a batch every tick can then run a few ticks ahead of the device.
 * With joint_ik the joint reference has one knot every 0.15 s, floor(horizon / 0.15) + 1 of them, and the library holds 22: a horizon
 * of 22 * 0.15 - 1e-9 = 3.3 s or more is HB_ERR_ARG (here and in hb_tick_resident; nothing is enqueued, the tables keep their
 * contents) — the reference resamples without a bound, and tables on fewer knots would differ from its tables under status 0.
 * Without joint_ik the horizon is bounded by max_nodes alone (status 2). */
int32_t hb_refgen_update(hb_ctx* ctx, const double* t0, double horizon, const double* x_now, const double* cmd_vel,
                         int32_t* status);
/* Status words of the last hb_refgen_update (synchronises). */
int32_t hb_refgen_get_status(hb_ctx* ctx, int32_t* status /*[batch]*/);
/* The mode-schedule window the last reference-generation pass read, for instances [inst_begin, inst_begin + inst_count): what
 * hb_refgen_set_schedule uploaded, or, with the device gait manager on, what it wrote.  n_events [count], event_times
 * [count][HB_MAX_EVENTS], modes [count][HB_MAX_EVENTS + 1]; any pointer may be NULL.  Synchronises. */
int32_t hb_refgen_get_schedule(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, int32_t* n_events, double* event_times,
                               int32_t* modes);

/* ---- device-resident gait manager ---------------------------------------------------------------------------------
 * The gait scheduler and the command-driven gait selection of the reference manager, per instance, on the device: GaitSchedule::
 * {insertModeSequenceTemplate, getModeSchedule, tileModeSequenceTemplate} (legged_interface/src/gait/GaitSchedule.cpp:57-161),
 * SwitchedModelReferenceManager::{calculateVelAbs, walkGait, findInsertModeSequenceTemplateTimer}
 * (legged_interface/src/SwitchedModelReferenceManager.cpp:173-249, gaitType_ == 0) and the cmd_vel rate limiter
 * (legged_controllers/include/legged_controllers/TargetTrajectoriesPublisher.h:97-129).  While it is enabled, every reference-generation
 * pass (hb_refgen_update, hb_tick_resident) first runs one more kernel that, per instance and in the reference's order
 * (SwitchedModelReferenceManager.cpp:145-158):
 *   1. rate-limits the incoming request (filter_cmd = 1; limits 0.1, 0.05, -, 0.3 per pass, linear z forced to 0),
 *   2. takes the window getModeSchedule(t0 - T, t0 + 2 T) of the instance's persistent schedule (T = horizon) — this is the mode
 *      schedule the planner of the same pass reads,
 *   3. evaluates calculateVelAbs on the first target state built from the observation and the filtered command, and the 50-sample
 *      average velAvg_,
 *   4. applies the walkGait thresholds (<= 0.02 level 0, (0.03, 0.4) level 1, >= 0.4 level 3),
 *   5. on a level change to 0 / 1 inserts the stance / trot template at the first window event >= t0, up to t0 + T; it takes
 *      effect from the next pass.  Level 3 inserts nothing; without a window event >= t0 the level changes and nothing is inserted.
 * The reference-generation kernels then read the FILTERED command.  Event times are bit-identical to the host classes of
 * hunter_hip.hpp / gait.py.  A schedule that would exceed HB_MAX_EVENTS events sets the instance's gait status to 1: its window stays
 * as the previous pass wrote it and its gait state stops advancing until hb_gait_reset; other instances are unaffected.
 * Not part of it: gaitType_ == 2 (trotGait), the /gait_type topic and the early / late-contact buffers. */
#define HB_GAIT_MAX_INIT_EVENTS 8
#define HB_GAIT_MAX_PHASES 8
typedef struct hb_gait_config {
  double phase_transition_stance_time;                      /* gait.info / task.info phaseTransitionStanceTime: one value per context */
  double init_event_times[HB_GAIT_MAX_INIT_EVENTS];         /* initialModeSchedule: 1 <= n_init_events <= 8 strictly increasing times */
  double template_switching_times[HB_GAIT_MAX_PHASES + 1];  /* defaultModeSequenceTemplate: n_template_phases + 1 increasing times */
  int32_t n_init_events;
  int32_t init_modes[HB_GAIT_MAX_INIT_EVENTS + 1];          /* n_init_events + 1 modes */
  int32_t n_template_phases;                                /* 1..8 */
  int32_t template_modes[HB_GAIT_MAX_PHASES];
  int32_t filter_cmd;              /* 1: cmd_vel arguments are raw requests, rate-limited on the device once per pass; 0: already filtered */
  int32_t reserved;                /* 0 */
} hb_gait_config;
/* Allocates on first use (that call initialises every instance), (re)initialises every instance — or, with mask [batch] != NULL, the
 * instances with mask[i] != 0 — to a fresh
 * reference object (the initial schedule and default template of cfg, gait level 0, empty velocity history, lastVel_ = 0, status 0) and
 * enables the manager.  cfg's context-wide values (phase_transition_stance_time, filter_cmd) always take effect.  HB_ERR_STATE before
 * hb_refgen_reset.  Enabling re-captures the range graphs. */
int32_t hb_gait_reset(hb_ctx* ctx, const hb_gait_config* cfg, const uint8_t* mask);
/* Back to host-supplied schedules (hb_refgen_set_schedule; the window of the last pass stays in place until then).  While the manager
 * is enabled hb_refgen_set_schedule returns HB_ERR_STATE. */
int32_t hb_gait_disable(hb_ctx* ctx);
/* The direct form of insertModeSequenceTemplate(template, start[i], final[i]) for instances [inst_begin, inst_begin + inst_count):
 * n_switch switching times (2..9) and n_switch - 1 modes — e.g. a named gait of gait.info.  The template becomes the instance's tiling
 * template; the gait level is not touched.  Synchronises. */
int32_t hb_gait_insert_template(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, int32_t n_switch, const double* switching_times,
                                const int32_t* modes, const double* start /*[count]*/, const double* final_time /*[count]*/);
/* Gait state of instances [inst_begin, inst_begin + inst_count) (any pointer may be NULL): level [count] (gaitLevel_), vel_abs / vel_avg
 * [count], cmd [count][4] (the filtered command), the persistent schedule n_events [count], event_times [count][HB_MAX_EVENTS], modes
 * [count][HB_MAX_EVENTS + 1], status [count] (0, or 1 after an overflow).  Synchronises. */
int32_t hb_gait_get_state(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, int32_t* level, double* vel_abs, double* vel_avg,
                          double* cmd, int32_t* n_events, double* event_times, int32_t* modes, int32_t* status);
/* ---- ground map of the controller: footholds, command target and filter foot heights on a per-instance height profile ---------------
 * Without a map the planner, the command target and the filter take the ground for the level plane (heights next_position_z,
 * com_height and 0).  A map gives instance i a horizontal unit direction a = (a_x, a_y) and K knots (s_k, g_k), 2 <= K <=
 * HB_PROFILE_MAX_KNOTS, s strictly increasing: the shape of the plant's terrain profile (hb_plant_set_terrain_profile) without its
 * friction, and under the same checks, so a plant profile is always a valid map.  The heights g are RELATIVE to that level ground: g = 0
 * everywhere is the world without a map.  The map is independent of the plant's ground (a wrong map can be given on purpose).
 * Height function  G_i(x, y):  s = a_x x + a_y y (two products, one sum);  j = the last k in 1 .. K - 2 with s >= s_k, else 0 (the end
 * segments open-ended, the scan of the plant's profile);  G = g_j + m_j (s - s_j)  with  m_j = (g_{j+1} - g_j) / (s_{j+1} - s_j)  computed
 * once by the set call.  Every operation is rounded on its own (no fused multiply-add): a level segment returns g_j bit for bit, a NaN
 * argument returns NaN.
 * While a map is in force the planner step and the filter step run in their ground forms (other kernels; the forms without a map are
 * untouched), which differ from the level ones in exactly these operands:
 *   latest stance position of a foot in contact, after its x, y refresh:   z = G(x, y) + next_position_z
 *   foothold p_n of a swing phase (calNextFootPos):                        z = G(p_n.x, p_n.y) + next_position_z
 *   centrifugal term of the foothold:                                      sqrt((body.z - G(body.x, body.y)) / 9.81) in place of sqrt(body.z / 9.81)
 *   first target knot:      x_now[8] moves towards  com_height + G(x_now[6], x_now[7])  by at most 0.04
 *   second target knot:     tgt[8] = com_height + G(tgt[6], tgt[7])
 *   filter measurement rows 24 .. 27 (foot heights):  y[24 + f] = G(xh[6 + 3 f], xh[7 + 3 f])  at the PREDICTED state xh, all four feet;
 *                           the x 100 noise of a foot off the ground and the measurement matrix stay as they are.
 * The friction cone, the end-effector constraint rows (world z), the joint-reference IK and the node tables take what the planner wrote.
 *
 * n_knots[batch]; dir[batch][2] (|a| > 0, normalised before it is stored); knots[batch][HB_PROFILE_MAX_KNOTS][2] = (s_k, g_k), entries
 * from n_knots on are not read.  All three NULL switch the map off.  HB_ERR_ARG for K out of range, a non-finite entry, |a| = 0, a knot
 * spacing <= 0 or |m_j| > sqrt(3) (the message names the first offending instance; the map in force is kept).  Legal any time after
 * hb_create; synchronises, takes effect from the next pass, and switching a map on or off re-captures the range graphs.  The map
 * survives hb_refgen_reset, hb_estimator_reset, hb_plant_reset and a respawn. */
int32_t hb_ground_set_profile(hb_ctx* ctx, const int32_t* n_knots /*[batch]*/, const double* dir /*[batch][2]*/,
                              const double* knots /*[batch][HB_PROFILE_MAX_KNOTS][2]*/);
/* The map in force (any pointer may be NULL): n_knots[batch], dir[batch][2] as stored, knots[batch][HB_PROFILE_MAX_KNOTS][2] (zero from
 * n_knots on), slopes[batch][HB_PROFILE_MAX_KNOTS - 1] = m_j (zero from n_knots - 1 on).  HB_ERR_STATE without a map in force. */
int32_t hb_ground_get_profile(hb_ctx* ctx, int32_t* n_knots, double* dir, double* knots, double* slopes);
/* ---- ground map of the controller as a two-dimensional height field ------------------------------------------------------------------
 * A field map gives instance i the grid of a plant height field (hb_plant_set_terrain_field) without its friction: a horizontal unit
 * direction a = (a_x, a_y) with b = (-a_y, a_x), an origin (u0, w0), spacings (du, dw) > 0, node counts 2 <= nu, nw <= HB_FIELD_MAX_NODES
 * and heights g[iu][iw], under the same checks (the plant's routine is run on the map with no friction, the triangle bound
 * p^2 + r^2 <= 3 (1 + 1e-12) included), so a plant field is always a valid map.  The heights are RELATIVE to the level ground the
 * controller has always assumed: g = 0 everywhere is the world without a map.  The map is independent of the plant's ground.
 * Height function  G_i(x, y),  every operation rounded on its own (no fused multiply-add), the cell and triangle exactly the plant's
 * (one routine, csrc/hb_contact.hpp field_cell, serves the plant's facet and this function):
 *   u = (a_x x + a_y y) - u0;   w = (b_x x + b_y y) - w0;   su = u / du;   sw = w / dw
 *   i = su >= 1 ? (su < nu - 2 ? int(su) : nu - 2) : 0;   j likewise from sw and nw   (a NaN fails every comparison: cell 0)
 *   fu = su - i;   fw = sw - j;   t = fu < fw ? 1 : 0     (beyond the grid fu, fw leave [0, 1]: the border cell's planes continue)
 *   g00 = g[i][j], g01 = g[i][j + 1], g10 = g[i + 1][j], g11 = g[i + 1][j + 1]
 *   t = 0 (fu >= fw, the lower triangle):   G = g00 + (g10 - g00) fu + (g11 - g10) fw      (left to right)
 *   t = 1 (the upper triangle):             G = g00 + (g01 - g00) fw + (g11 - g01) fu
 * A level cell returns g00 bit for bit; a NaN coordinate selects facet 0 and returns NaN.  The facet id is the plant's,
 * 2 (i (nw - 1) + j) + t.
 * While a field map is in force the planner step and the filter step run in their field forms (k_refgen_gfield, k_estimator_gfield;
 * the forms without a map and the profile forms are untouched), which differ from the level ones in exactly the six operands listed
 * above hb_ground_set_profile, with this G in place of the profile's, per contact point.
 *
 * n_nodes[batch][2] = (nu, nw); dir[batch][2] (|a| > 0, normalised before it is stored); origin[batch][2]; spacing[batch][2];
 * heights[batch][HB_FIELD_MAX_NODES][HB_FIELD_MAX_NODES], entries beyond (nu, nw) are not read.  All five NULL switch the map off.
 * HB_ERR_ARG for a node count out of range, a non-finite entry, |a| = 0, a spacing <= 0 or a triangle steeper than sqrt(3) (the message
 * names the first offending instance; the map in force is kept).  One map at a time: hb_ground_set_profile and hb_ground_set_field
 * replace one another (all-NULL in either switches the map in force off), and each getter returns HB_ERR_STATE while the other kind
 * is in force.  A profile draw with follow_map (hb_plant_set_profile_draw) writes profile records: it and a field map refuse one another
 * with HB_ERR_STATE, in either order.  Legal any time after hb_create; synchronises, takes effect from the next pass, and every change of
 * kind (on, off, profile <-> field) re-captures the range graphs.  The map survives hb_refgen_reset, hb_estimator_reset, hb_plant_reset
 * and a respawn. */
int32_t hb_ground_set_field(hb_ctx* ctx, const int32_t* n_nodes /*[batch][2]*/, const double* dir /*[batch][2]*/,
                            const double* origin /*[batch][2]*/, const double* spacing /*[batch][2]*/,
                            const double* heights /*[batch][HB_FIELD_MAX_NODES][HB_FIELD_MAX_NODES]*/);
/* The field map in force (any pointer may be NULL): n_nodes[batch][2], dir[batch][2] as stored, origin, spacing [batch][2],
 * heights[batch][HB_FIELD_MAX_NODES][HB_FIELD_MAX_NODES] (zero beyond (nu, nw)).  HB_ERR_STATE unless a field map is in force. */
int32_t hb_ground_get_field(hb_ctx* ctx, int32_t* n_nodes, double* dir, double* origin, double* spacing, double* heights);
/* ---- sole-consistent footholds on the ground map, with edge avoidance -------------------------------------------------------------------
 * On a map the planner puts every contact point to the ground on its own (the operands above hb_ground_set_profile).  The toe and the
 * heel of one rigid sole are two such points: with a riser or a bump between them they are planned at different heights, a pitch the
 * ground does not have.  Mode 1 of this configuration (one per context, off by default) plans the two points of a foot as ONE sole.  It
 * acts only while a map is in force, in forms of the planner of their own (k_refgen_ground_sole, k_refgen_gfield_sole: no other kernel
 * changes), and differs from the per-point forms in exactly the two operands below; the centrifugal term, the two target knots, the
 * filter's height rows, the cone and the end-effector rows stay as they are.
 * Foot l in {0, 1} has the contact points T = l (contact f1, the toe) and H = l + 2 (f2, the heel); the two carry the same contact flag
 * in every mode.  G is the height function of the map in force, npz = next_position_z.
 * Sole sample  S(cT, cH) -> (delta, top)  of two points (x, y):  the five sample points  c_q = cH + (q / 4) (cT - cH), q = 0 .. 4, per
 * coordinate (q / 4 exact, one difference, one product, one sum);  h_q = G(c_q);  the chord  ch_q = h_0 + (q / 4) (h_4 - h_0);  the defect
 * delta = max over q = 1 .. 3 of |h_q - ch_q|;  top = max over q = 0 .. 4 of h_q.  Every operation is rounded on its own (no fused
 * multiply-add).  A NaN among the h_q makes delta (and top) NaN, and a NaN delta is never accepted.
 *   latest stance position of a foot in contact, after the x, y refresh of its points:  (delta, top) = S(ls_T.xy, ls_H.xy), not shifted;
 *       delta <= flat_tol:  ls_P.z = G(ls_P.xy) + npz  for P = T, H (the per-point values);  otherwise both  ls_P.z = top + npz, a level
 *       sole on its highest sample.  (The memory of a foot in the air keeps its x, y and is put to the map in the same way.)
 *   foothold of a swing phase (calNextFootPos):  pT, pH = the nominal footholds of the two points by the per-point formula (they differ in
 *       feet_bias only);  e = (pT - pH).xy / |(pT - pH).xy|  (length = sqrt(dx dx + dy dy); zero or non-finite: no shifting, n_shift taken
 *       as 0);  candidate k moves both points by the same vector,  c_k(P) = P.xy + (k shift_step) e,  with  (delta_k, top_k) =
 *       S(c_k(pT), c_k(pH));  the candidates are tried in the order  k = 0, +1, -1, +2, -2, .., +n_shift, -n_shift  and the first with
 *       delta_k <= flat_tol is accepted:  P.xy = c_k(P),  P.z = G(c_k(P)) + npz  — on a single plane today's foothold bit for bit.  If
 *       none is accepted, k* = the candidate of the smallest delta_k (the earliest in the order among equals; a NaN loses against any
 *       number), both points move to c_k*(P) and both get  z = top_k* + npz  (levelled).  The shifted foothold is the take-off point of the
 *       next swing phase, as footholds chain today.
 * mode 0: per contact point; 1: per sole.  n_shift: candidates to either side of the nominal foothold.  shift_step [m].  flat_tol [m]. */
#define HB_FOOTHOLD_MAX_SHIFT 8
typedef struct hb_foothold_config {
  int32_t mode;        /* 0: per contact point (the behaviour without this call); 1: per sole */
  int32_t n_shift;     /* 0 .. HB_FOOTHOLD_MAX_SHIFT: candidates to either side of the nominal foothold */
  double  shift_step;  /* [m], > 0 when n_shift > 0 */
  double  flat_tol;    /* [m], >= 0 */
} hb_foothold_config;
/* cfg NULL or mode 0: off (the stored configuration becomes all zero).  HB_ERR_ARG for a mode outside {0, 1}, n_shift outside
 * 0 .. HB_FOOTHOLD_MAX_SHIFT, a non-finite or non-positive shift_step with n_shift > 0, a negative or non-finite flat_tol; a refused
 * call keeps the configuration in force.  Legal any time after hb_create, with or without a map in force (it takes effect while one
 * is, with every producer of the map: the two setters, a draw with follow_map, the height scan); synchronises, takes effect from the next
 * pass, and switching the mode on or off re-captures the range graphs.  The configuration survives hb_refgen_reset, hb_estimator_reset,
 * hb_plant_reset and a respawn. */
int32_t hb_ground_set_foothold(hb_ctx* ctx, const hb_foothold_config* cfg);
/* The configuration in force (all zero while off). */
int32_t hb_ground_get_foothold(hb_ctx* ctx, hb_foothold_config* out);
/* What the last planner pass in sole mode decided, per (instance, foot l), for the FIRST foothold it planned for that foot (any pointer
 * may be NULL; [count][2]): shift = the k taken, or INT32_MIN if the pass planned no foothold for the foot (defect 0, level 0 then);
 * defect = delta_k of that candidate; level = 1 if the fallback levelled the pair, else 0.  Switching the mode on clears the read-back
 * to "no foothold"; a pass that does not run in sole mode (no map in force) leaves it as it is.  Synchronises.  HB_ERR_STATE while the
 * mode is off. */
int32_t hb_ground_get_foothold_choice(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, int32_t* shift /*[count][2]*/,
                                      double* defect /*[count][2]*/, int32_t* level /*[count][2]*/);
/* Node tables back to the host (any pointer may be NULL); layouts as in hb_mpc_set_references. */
int32_t hb_mpc_get_references(hb_ctx* ctx, int32_t inst_begin, int32_t inst_count, int32_t* n_nodes, double* t,
                              int32_t* mode, double* x_ref, double* swing_ref);

/* ---- misc ------------------------------------------------------------------------------------ */
int32_t hb_sync(hb_ctx* ctx);
int32_t hb_get_stats(hb_ctx* ctx, hb_stats* out);
/* Joint-space input cost R (22x22) built at init from R_task_diag (LeggedInterface.cpp:263-290). */
int32_t hb_get_input_cost(const hb_ctx* ctx, double* R /*[22][22]*/);
/* Library/ABI version: major*10000 + minor*100 + patch. */
int32_t hb_version(void);

/* ---- unit-level entry points used by the parity tests (each is one HIP kernel launch) ----------- */
/* Centroidal flow map and its Jacobians (PinocchioCentroidalDynamicsAD, LeggedRobotDynamicsAD.cpp:57-70). */
int32_t hb_eval_flow_map(hb_ctx* ctx, int32_t n, const double* x, const double* u, double* f /*[n][22]*/,
                         double* dfdx /*[n][22][22] or NULL*/, double* dfdu /*[n][22][22] or NULL*/);
/* Foot positions / velocities (PinocchioEndEffectorKinematicsCppAd, EndEffectorLinearConstraint.cpp:105-128). */
int32_t hb_eval_foot_kinematics(hb_ctx* ctx, int32_t n, const double* x, const double* u,
                                double* pos /*[n][4][3]*/, double* vel /*[n][4][3]*/);
/* Rigid-body quantities of WbcBase::updateMeasured (WbcBase.cpp:70-120): M[16][16], nle[16], J[12][16], dJv[12]. */
int32_t hb_eval_rbd(hb_ctx* ctx, int32_t n, const double* rbd, double* M, double* nle, double* J, double* dJv);
/* MPC observation state from the rbd state: x = [A(q) v / m, base pose, joints]
 * (CentroidalModelRbdConversions::computeCentroidalStateFromRbdModel, call site LeggedController.cpp:332); no yaw
 * unwrapping. */
int32_t hb_centroidal_state_from_rbd(hb_ctx* ctx, int32_t n, const double* rbd /*[n][32]*/, double* x /*[n][22]*/);
/* Solve a batch of equality-free LQ problems (n <= batch, N <= max_nodes, nu <= 12 inputs per stage) with the
 * Riccati backward kernel (HPIPM's role).  Stage data row-major: A[n][N][22][22], B[n][N][22][nu],
 * b[n][N][22], Q[n][N][22][22], R[n][N][nu][nu], P[n][N][nu][22], q[n][N][22], r[n][N][nu], dx0[n][22].
 * Clobbers the MPC reference tables of the context (call hb_mpc_set_references again afterwards). */
int32_t hb_riccati_solve(hb_ctx* ctx, int32_t n, int32_t N, int32_t nu, const double* A, const double* B,
                         const double* b, const double* Q, const double* R, const double* P, const double* q,
                         const double* r, const double* dx0, double* dx /*[n][N+1][22]*/, double* du /*[n][N][nu]*/);
/* The gains of the Riccati backward sweep alone, on caller-given stage data with per-stage widths: n <= batch instances, N[i] stages
 * (1 <= N[i] <= max_nodes), stage k of instance i with n_f[i][k] + n_z[i][k] in {6, 9, 12} real inputs (the two numbers go to the record's
 * width words as the LQ stage writes them).  Every array is [n][max_nodes][...] with the input index padded to 12: A [..][22][22],
 * B [..][22][12], b [..][22], Q [..][22][22], R [..][12][12], P [..][12][22], q [..][22], r [..][12]; of B, R, P, r the leading
 * n_f + n_z columns / rows are read, stages k >= N[i] are not read at all.  Records are packed as hb_riccati_solve packs them (R~ padded
 * with I, B~, P~, r~ with zeros); the record of every stage k >= N[i] and of every instance n .. batch-1 is filled with quiet NaNs and the
 * whole gains buffer with the bit pattern HB_RIC_GAINS_SENTINEL_BITS before the launch, so that K, k show which slots the sweep wrote and
 * whether anything behind a horizon reached its arithmetic.  The sweep is the product's (hb_config.reserved picks its form as everywhere).
 * Outputs: K [n][max_nodes][12][22], k [n][max_nodes][12] (u~ = k + K dx), ric_fail [n] (1: a pivot of some stage was not positive).
 * Clobbers the MPC reference tables of the context like hb_riccati_solve. */
#define HB_RIC_GAINS_SENTINEL_BITS 0x7ff85e471e100001ULL
int32_t hb_riccati_gains(hb_ctx* ctx, int32_t n, const int32_t* N, const int32_t* n_f, const int32_t* n_z, const double* A,
                         const double* B, const double* b, const double* Q, const double* R, const double* P, const double* q,
                         const double* r, double* K, double* k, int32_t* ric_fail);
/* Generic hierarchical QP cascade on small dense tasks (HoQp.cpp:21-198; HoQp.h:24-89): n_problems independent stacks of
 * n_levels <= 3 tasks {A x = b in the least-squares sense, D x <= f with slack} on n_vars <= 8 variables, m_eq[l] / m_in[l]
 * <= 8 rows per level (the same shape for every problem).  Blocks are padded: A, D [n_problems][3][8][8] row-major, b, f
 * [n_problems][3][8].  Outputs: x [n_problems][3][8] = solution after each level (HoQp::getSolutions of that level),
 * slack [n_problems][3][8] = the level's own slack (HoQp::getStackedSlackSolutions tail), status [n_problems] = hb_inst_status.
 * The device counterpart of the reference's unit test legged_wbc/test/HoQp_test.cpp:18-55; runs the building blocks of the
 * HierarchicalWbc kernel (hb_config.wbc_type = 1) on plain matrices. */
int32_t hb_hoqp_solve(hb_ctx* ctx, int32_t n_problems, int32_t n_vars, int32_t n_levels, const int32_t* m_eq, const int32_t* m_in,
                      const double* A, const double* b, const double* D, const double* f, double* x, double* slack, int32_t* status);
/* Diagnostics of the chunked hb_step_resident: out4 = [graph launches, directly enqueued chunk steps, forks from the library streams,
 * graph captures] since hb_create. */
int32_t hb_debug_chunk_counters(hb_ctx* ctx, int64_t* out4);
/* out2 = [graph captures / instantiations that FAILED since hb_create, 1 if this context has therefore given up on graphs and steps
 * its ranges with direct launches (until the next hb_set_chunks)].  A failed capture is not retried on every step. */
int32_t hb_debug_graph_state(hb_ctx* ctx, int64_t* out2);
/* n independent inverse-kinematics problems of the joint-reference generator (InverseKinematics::computeIK(init_q, leg, pos, R_des),
 * legged_interface/src/foot_planner/InverseKinematics.cpp:36-231): q16[n][16] = [base pos, zyx, joints] start configurations,
 * leg[n] in {0 left, 1 right}, des_pos[n][3] target of contact f1 of the leg, R_des[n][9] row-major desired foot rotation;
 * out5[n][5] = the leg's joint angles.  Runs the lane-cooperative device routine that hb_refgen_update uses per knot; it is
 * the entry the reference-compiled golden vectors (tests/golden/ref_ik.json) are checked through. */
int32_t hb_ik_solve(hb_ctx* ctx, int32_t n, const double* q16, const int32_t* leg, const double* des_pos, const double* R_des, double* out5);
/* The height function of the ground map in force (hb_ground_set_profile) at n points, one kernel launch: point p is put to the map of
 * instance inst[p] (0 <= inst[p] < batch), xy[n][2]; height[n] = G(x, y), segment[n] = j (either may be NULL, not both).  Runs the device
 * routine the ground forms of the planner and the filter call.  HB_ERR_STATE without a map in force. */
int32_t hb_ground_eval(hb_ctx* ctx, int32_t n, const int32_t* inst, const double* xy, double* height, int32_t* segment);
/* QP step of the last SQP iteration (before the line search scaled it): dx[batch][max_nodes+1][22],
 * du[batch][max_nodes][22]; either may be NULL. */
int32_t hb_mpc_get_step(hb_ctx* ctx, double* dx, double* du);

#ifdef __cplusplus
}
#endif
#endif /* HUNTER_HIP_H */
