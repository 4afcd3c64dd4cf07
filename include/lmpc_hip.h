/*
 * lmpc_hip.h -- C ABI of the MI355X-native batched LMPC solve path.
 *
 * Drop-in boundary for the per-step optimisation of MPC-Berkeley/Racing-LMPC-ROS2:
 *   lmpc::mpc::racing_mpc::RacingMPC::solve        src/mpc/racing_mpc/src/racing_mpc.cpp:209-372
 *   (problem definition                            src/mpc/racing_mpc/src/racing_mpc.cpp:31-202,442-543)
 *   SingleTrackPlanarModel::compile_dynamics       src/vehicle_dynamics_models/single_track_planar_model/src/single_track_planar_model.cpp:195-418
 *   SafeSetManager::query(SSQuery)                 src/vehicle_dynamics_models/racing_trajectory/src/safe_set.cpp:153-180
 *   RacingTrajectory::global_to_frenet / frenet_to_global  src/vehicle_dynamics_models/racing_trajectory/src/racing_trajectory.cpp:122-236
 *
 * Conventions
 *   - Plain C: pointers and sizes only.  No exception crosses this boundary: every
 *     entry point returns LMPC_OK (0) or a negative lmpc_status code; the message is
 *     kept on the handle (lmpc_last_error).
 *   - All `*_batch` array arguments are DEVICE pointers (HBM) unless a parameter is
 *     documented as host.  The caller owns every buffer; the library owns only the
 *     handle (constants, the safe-set copy, a linearisation workspace) and the spline tracks it hands out.  Launches go to
 *     the stream set by lmpc_set_stream.  After lmpc_reserve(max_batch) no `*_batch` call
 *     with batch <= max_batch allocates.
 *   - Batched layout is struct-of-arrays with the batch axis fastest:
 *         field[component][knot][batch]   ->   ((c * n_knots) + i) * batch + b
 *     so a wavefront's loads along the batch axis coalesce.
 *   - State  x = [s, e_y, e_psi, vx, vy, omega]  (base_vehicle_model.hpp:32-40),
 *     input  u = [u_lon, steer]                  (single_track_planar_model.hpp:62-66);
 *     N counts knot points: X is 6 x N, U and dU are 2 x (N-1) (racing_mpc.cpp:43-45).
 *   - A handle is not re-entrant (the reference holds traj_mutex_ across solve,
 *     racing_mpc_node.cpp:158,360); distinct handles (one per GPU) are independent.
 *   - Streams.  Every kernel launch, memset and asynchronous copy of an entry point goes to the handle's stream (lmpc_set_stream),
 *     never to the null stream.  An entry point whose array arguments are device pointers is ASYNCHRONOUS unless its comment says
 *     otherwise: it enqueues and returns, and neither waits for the stream nor reads device data on the host.  An entry point that
 *     takes or returns HOST arrays, or that allocates or frees device memory (the create / destroy calls, lmpc_set_safe_set,
 *     lmpc_set_regression_laps and lmpc_fleet_ss_set_regression with their _rows forms, lmpc_reserve, a first call that grows a
 *     workspace), is BLOCKING: it waits for the handle's stream where its comment says so, and the runtime's allocator may wait for
 *     the whole device.  Five of them -- lmpc_set_safe_set, lmpc_set_regression_laps, lmpc_set_regression_laps_rows,
 *     lmpc_fleet_ss_load, lmpc_fleet_ss_get_laps -- move their host arrays with
 *     the synchronous hipMemcpy (a copy on the null stream that has finished when it returns), between waits on the handle's
 *     stream: behind the first wait nothing of the handle is in flight, and what they enqueue afterwards goes to the handle's
 *     stream again.  The rest only read or set host values of the handle.  The three lists are in INTEGRATION.md;
 *     tests/stream_cases.py holds one class per prototype and tests/test_gpu_streams.py holds every entry point to it on a stream
 *     that is held by a timed gate (the two entry points of lmpc_hip_rows.h: tests/test_stream_table_rows.py and
 *     tests/test_gpu_streams_rows.py).
 */
#ifndef LMPC_HIP_H_
#define LMPC_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LMPC_NX 6
#define LMPC_NU 2

/* return codes of the entry points */
typedef enum lmpc_status {
  LMPC_OK = 0,
  LMPC_ERR_ARGUMENT = -1,      /* null pointer, bad size, unsupported option          */
  LMPC_ERR_RUNTIME = -2,       /* HIP runtime error (message in lmpc_last_error)      */
  LMPC_ERR_UNSUPPORTED = -3    /* valid reference configuration not built yet         */
} lmpc_status;

/* per-problem status written by lmpc_solve_batch (replaces "X_optm absent from out",
 * racing_mpc.cpp:343-371 / racing_mpc_node.cpp:322-332) */
#define LMPC_SOLVE_OPTIMAL 0
#define LMPC_SOLVE_MAX_ITER 1   /* the iteration cap -- or (fp64) stopped short of the stated accuracy: the interior point reached its
                                   floor and the active-set polish was refused by a consistent held set whose multiplier steps do
                                   not settle, i.e. the problem's linear algebra is noisier than the 1e-6 contract (low speed x
                                   long horizon: the RK4 step map is unstable there), or (round 6) it stopped at its stall rule while its
                                   Newton step would still have moved the iterate by more than 1e-6 (scaled) and the polish did not
                                   verify the point; the iterate is returned, not vouched for */
#define LMPC_SOLVE_INFEASIBLE 2 /* x_ic outside [x_min, x_max] at knot 0, row residual stalls, NaN */
#define LMPC_SOLVE_UNVERIFIED 3 /* lmpc_solve_batch_mixed with lmpc_config.polish = 1 only: the fp32 iteration did not reach an
                                   answer it could verify -- polish refused, out of iterations, or infeasible by its
                                   single-precision residuals (the default two-pass solve re-solves these in fp64, which has
                                   the last word, and never reports 3) */

/* vehicle_model_factory.cpp:31-49 -- same selector names; only the first is built as a controller's model (lmpc_create); the
 * third is built as a PLANT only, lmpc_hip_dtrack.h */
#define LMPC_MODEL_SINGLE_TRACK_PLANAR 0
#define LMPC_MODEL_KINEMATIC_BICYCLE 1
#define LMPC_MODEL_DOUBLE_TRACK_PLANAR 2
#define LMPC_INTEGRATOR_RK4 0
#define LMPC_INTEGRATOR_EULER 1

/* The ~25 scalars compile_dynamics/add_nlp_constraints read
 * (base_vehicle_model_config.hpp:30-154, single_track_planar_model.hpp:31-43). */
typedef struct lmpc_vehicle {
  int32_t model_id;      /* LMPC_MODEL_SINGLE_TRACK_PLANAR                                */
  int32_t integrator;    /* modeling.integrator_type: LMPC_INTEGRATOR_RK4 (0) | LMPC_INTEGRATOR_EULER (1)
                            (single_track_planar_model.cpp:357-368; lmpc_utils/src/utils.cpp:88-123)     */
  double m;              /* chassis.total_mass                                            */
  double Jzz;            /* chassis.moi                                                   */
  double l;              /* chassis.wheel_base                                            */
  double cg_ratio;       /* chassis.cg_ratio  (lr = cg_ratio * l)                         */
  double h;              /* chassis.cg_height                                             */
  double b;              /* chassis.b  (body width, boundary margin adds b/2)             */
  double fr;             /* chassis.fr (rolling resistance)                               */
  double kd;             /* powertrain.kd  (front drive share)                            */
  double kb;             /* front_brake.bias                                              */
  double cd;             /* aero.drag_coeff                                               */
  double Af;             /* aero.frontal_area                                             */
  double rho;            /* aero.air_density                                              */
  double cl_f;           /* aero.cl_f                                                     */
  double cl_r;           /* aero.cl_r                                                     */
  double mu;             /* single_track_planar.mu                                        */
  double Bf, Cf;         /* front_tyre.pacejka_b / pacejka_c                              */
  double Br, Cr;         /* rear_tyre.pacejka_b / pacejka_c                               */
  double Fd_max, Fb_max; /* single_track_planar.fd_max / fb_max                           */
  double Td, Tb;         /* single_track_planar.td / tb                                   */
  double max_steer;      /* steer.max_steer                                               */
  double max_steer_rate; /* steer.max_steer_rate                                          */
} lmpc_vehicle;

/* RacingMPCConfig (racing_mpc_config.hpp:37-82), numeric fields only. */
typedef struct lmpc_config {
  int32_t N;                  /* knot points                                                */
  int32_t learning;           /* 0 tracking MPC, 1 LMPC (safe-set terminal set + cost)      */
  int32_t num_ss_pts;         /* S                                                          */
  int32_t num_ss_pts_per_lap; /* K                                                          */
  int32_t max_lap_stored;
  int32_t max_iter;           /* interior-point iteration cap (<=0: default 60)             */
  int32_t polish;             /* active-set polish of the interior-point answer, the role of OSQP's polish = true
                                 (racing_mpc.cpp:90-95): 0 (default) on, < 0 off; 1: on, and lmpc_solve_batch_mixed
                                 leaves out its fp64 pass -- problems whose fp32 answer it could not verify keep
                                 status LMPC_SOLVE_UNVERIFIED (diagnostics)                    */
  int32_t reserved;           /* (keeps `tol` 8-byte aligned; set to 0)                      */
  double tol;                 /* complementarity tolerance (<=0: default 3e-14)             */
  double margin;
  double q_contour, q_heading, q_vel, q_vy, q_vyaw, q_boundary;
  double R[4];                /* row-major 2x2                                              */
  double R_d[4];
  double x_max[LMPC_NX], x_min[LMPC_NX]; /* +-INFINITY allowed                              */
  double u_max[LMPC_NU], u_min[LMPC_NU];
  double convex_hull_slack[LMPC_NX]; /* cost weights of the hull residual x_T - SS lambda (racing_mpc.cpp:493-499); a zero
                                        component leaves that component of the residual free; ALL zero is the hard
                                        equality x_T = SS lambda of :500-502, see LMPC_HARD_HULL_WEIGHT            */
  double max_vel_ref_diff;
} lmpc_config;

/* Hard convex-hull equality (all-zero convex_hull_slack, racing_mpc.cpp:500-502).  The terminal block eliminates the hull
 * residual eps = x_T - SS lambda through its weight (E^-1 in the Schur complement); the equality is the limit E^-1 -> 0,
 * taken numerically: the residual carries the weight LMPC_HARD_HULL_WEIGHT, at which the answer is within 1e-7 (scaled)
 * of the equality-constrained optimum (eps = multiplier / (2 weight); measured against the dense oracle with eps pinned
 * to zero, tests/test_gpu_mixed_lmpc.py) and the two-level elimination still has two decades of headroom (it breaks down
 * past 1e13).  A problem whose terminal state cannot reach the hull -- infeasible upstream -- is left with a residual the
 * weight does not close: scaled |eps|_inf > LMPC_HARD_HULL_RESIDUAL reports LMPC_SOLVE_INFEASIBLE.  fp64 only: the
 * single-precision and mixed entry points refuse it (LMPC_ERR_UNSUPPORTED). */
#define LMPC_HARD_HULL_WEIGHT 1e11
#define LMPC_HARD_HULL_RESIDUAL 1e-5

/* Closed track as uniform periodic tables over [0, L): sample j sits at s = j*L/M.
 * Lookup is periodic linear interpolation.  (The reference interpolates cubic
 * B-splines of a 17-column table, racing_trajectory.cpp:25-120 -- out of scope;
 * the tables are what RacingMPCNode samples at racing_mpc_node.cpp:261-266.) */
typedef struct lmpc_track {
  double L;
  int32_t M;
  int32_t reserved;
  const double* curvature;   /* device, M                                                  */
  const double* bound_left;  /* device, M  (signed lateral offset, > 0)                    */
  const double* bound_right; /* device, M  (signed lateral offset, < 0)                    */
  const double* vel;         /* device, M                                                  */
} lmpc_track;

typedef struct lmpc_handle lmpc_handle;

/* Builds the parametric problem once, as RacingMPC::RacingMPC does
 * (racing_mpc.cpp:31-202).  `device` is the HIP device ordinal. */
int lmpc_create(const lmpc_config* cfg, const lmpc_vehicle* veh, int device, lmpc_handle** out);
/* On failure *out may still be non-NULL so that lmpc_last_error(*out) can be read; destroy it.  lmpc_create allocates (blocking, no
 * stream yet); lmpc_destroy waits for the handle's stream before it frees anything. */
void lmpc_destroy(lmpc_handle* h);
const char* lmpc_last_error(const lmpc_handle* h);

/* Run subsequent launches on `hip_stream` (a hipStream_t).  A new handle uses the device's
 * default (null) stream; NULL selects it again.  Host-only: nothing is enqueued and nothing is waited for.  Work is ordered only
 * WITHIN the handle's current stream: the handle's workspace, staging buffers and stores (safe set, regression tables, fleet rings,
 * filter, controllers) are shared by all of its calls, whatever stream each was issued on, so a caller who moves a handle to another
 * stream while work of the old one may still run orders the two streams itself (an event, or a wait of one stream on the other) --
 * the handle keeps no state tied to a stream and inserts no dependency of its own.  For streams that run CONCURRENTLY use one handle
 * per stream, as bench.py does. */
int lmpc_set_stream(lmpc_handle* h, void* hip_stream);
/* Block until everything queued on the handle's stream has finished (synchronises the handle's stream). */
int lmpc_synchronize(lmpc_handle* h);

/* discrete_dynamics_jacobian for every stage of every problem
 * (single_track_planar_model.cpp:377-387, called at racing_mpc.cpp:173-182):
 *   X_ref [6][N][B], U_ref [2][N-1][B], T_ref [N-1][B], curvatures [N][B]  ->
 *   A [6][6][N-1][B] (row, col), Bm [6][2][N-1][B], g [6][N-1][B].                          */
int lmpc_linearize_batch(lmpc_handle* h, int32_t batch, const double* X_ref, const double* U_ref,
                         const double* T_ref, const double* curvatures, double* A, double* Bm,
                         double* g);

/* RacingMPC::solve for `batch` independent problems (racing_mpc.cpp:209-372).
 *   in : x_ic [6][B], u_ic [2][B], X_ref [6][N][B], U_ref [2][N-1][B], T_ref [N-1][B],
 *        bound_left/bound_right/curvatures/vel_ref [N][B], total_length (scalar, host value)
 *        T_ref is per stage and per problem, every entry > 0: t_i = T_ref[i][b] is the integration step from knot i to knot i + 1
 *        and the step of stage i's rate row u_{i-1} + dU_i t_i = u_i, u_{-1} = u_ic (racing_mpc.cpp:190-196), in every entry point.
 *        ss_x [6][S][B], ss_j [S][B]  (learning only, already padded/truncated to S and
 *        with J - J[0] applied: racing_mpc.cpp:263-280; NULL for tracking)
 *   out: X_optm [6][N][B], U_optm [2][N-1][B], dU_optm [2][N-1][B],
 *        convex_combi_optm [S][B] (learning; may be NULL),
 *        status [B] (LMPC_SOLVE_*), iters [B] (the reference's stats["iter_count"]),
 *        kkt [4][B] optional: inf-norm of the last primal step, largest row residual,
 *        complementarity mu, boundary slack sigma.                                           */
int lmpc_solve_batch(lmpc_handle* h, int32_t batch, const double* x_ic, const double* u_ic,
                     const double* X_ref, const double* U_ref, const double* T_ref,
                     const double* bound_left, const double* bound_right, const double* curvatures,
                     const double* vel_ref, double total_length, const double* ss_x,
                     const double* ss_j, double* X_optm, double* U_optm, double* dU_optm,
                     double* convex_combi_optm, int32_t* status, int32_t* iters, double* kkt);

/* lmpc_solve_batch with the reference's warm-start inputs USED (racing_mpc.cpp:293-305: X_optm_ref, U_optm_ref, dU_optm_ref; in
 * the node they are the previous solution shifted by one knot, racing_mpc_node.cpp:245-254 -- the arrays lmpc_shift_batch writes).
 * X_optm_ref [6][N][B], U_optm_ref [2][N-1][B] (dU_optm_ref is implied: u_i = u_{i-1} + t_i dU_i is a row of the QP); they may alias
 * X_ref / U_ref, as they do in the node.  Before any interior point the kernel tries an ACTIVE-SET solve on the plan: the plan
 * made dynamically exact about this call's linearisation, its active bounds taken as the working set, the equality-constrained
 * QP solved and its KKT conditions verified (the polish's machinery; at most two repairs of the set).  Accepted -- 92 .. 96 % of
 * the periods of a closed loop -- the answer is the optimum the cold solve finds (same 1e-6 contract; measured 1e-11 apart) for
 * about two iterations' worth of work instead of seven; `iters` then counts the rounds (1 or 2).  Refused, the call IS
 * lmpc_solve_batch (the rounds spent are added to `iters`).  A bad plan costs time, never correctness: nothing is returned that
 * has not passed the KKT test of this problem.  fp64 tracking problem; learning handles: lmpc_solve_batch_warm_ss below.
 * With lmpc_config.polish < 0 (the polish switched off) there is no active-set machinery to try the plan with: the call is a cold
 * lmpc_solve_batch, silently -- lmpc_get_warm_accepted then reports 0 for every problem. */
int lmpc_solve_batch_warm(lmpc_handle* h, int32_t batch, const double* x_ic, const double* u_ic, const double* X_ref, const double* U_ref,
                          const double* T_ref, const double* bound_left, const double* bound_right, const double* curvatures,
                          const double* vel_ref, double total_length, const double* X_optm_ref, const double* U_optm_ref, double* X_optm,
                          double* U_optm, double* dU_optm, int32_t* status, int32_t* iters, double* kkt);

/* The same for the LEARNING problem (round 6; racing_mpc.cpp:281 `set_initial(convex_combi_, convex_combi_optm_ref)` and :293-305
 * apply to the learning controller too).  One more piece of the plan: convex_combi_optm_ref [S][B], the simplex weights of the plan's
 * terminal point ALIGNED WITH THIS CALL'S safe-set points (entry j weighs point j of ss_x / ss_idx).  Their support is the working
 * set of the simplex rows -- free where the weight is positive, held at zero elsewhere --, the weights start the multiplier steps, the
 * stage rows' working set is read off (X_optm_ref, U_optm_ref) as above; the candidate is verified against the KKT conditions of this
 * problem (simplex rows included) and repaired, or the cold solve runs.  The safe set as arrays (ss_x, ss_j; ss_idx NULL) or by
 * reference (ss_idx from lmpc_ss_query_idx_batch on this handle; ss_x, ss_j NULL).  The query returns its neighbours nearest first, so
 * from one control period to the next the POSITION of a point in the set changes: lmpc_shift_lambda_batch below carries the previous
 * solution's weights over by the identity of the points.  convex_combi_optm_ref NULL (or all zero): the cold solve.  fp64; horizons up
 * to N = 60 (longer: the cold solve).  lmpc_get_warm_accepted tells which problems took the short route. */
int lmpc_solve_batch_warm_ss(lmpc_handle* h, int32_t batch, const double* x_ic, const double* u_ic, const double* X_ref, const double* U_ref,
                             const double* T_ref, const double* bound_left, const double* bound_right, const double* curvatures,
                             const double* vel_ref, double total_length, const double* ss_x, const double* ss_j, const int32_t* ss_idx,
                             const double* X_optm_ref, const double* U_optm_ref, const double* convex_combi_optm_ref, double* X_optm,
                             double* U_optm, double* dU_optm, double* convex_combi_optm, int32_t* status, int32_t* iters, double* kkt);

/* convex_combi_optm_ref for lmpc_solve_batch_warm_ss when the safe set goes by reference: lambda_prev [S][B] of the previous
 * solution on the codes ss_idx_prev [S][B] it was solved on -> lambda_ref [S][B] on this period's codes ss_idx.  From one period to
 * the next a support point of the optimum stays, moves one recorded sample along its lap, or two (measured in the LMPC experiment):
 * every support point (weight > 1e-9) is placed on the sample `advance` steps on when that is among the new neighbours, else on
 * the point itself, else `advance` + 1 steps on -- at most six positive entries per problem, what the solver's terminal block keeps
 * explicit; a support point none of whose candidates is in the new set drops out (the solver renormalises).  An active-set start
 * needs the support RIGHT: in the LMPC experiment this guess is (advance = 1; four repair rounds) for a quarter of the periods, and
 * the rest pay the refused rounds on top of their cold solve -- closed_loop.run_lmpc leaves it off by default.
 * Both code arrays must come from lmpc_ss_query_idx_batch against the store CURRENTLY set (lmpc_set_safe_set): the codes are
 * decoded with its lap lengths.  ss_idx_prev is one query older than ss_idx, so no generation is checked; a code that names no row
 * of the store (-1, a row at or past the store's total, a fourth copy) is read as "no point" -- it carries no weight and receives
 * none.  The support is read in ascending position, its first eight entries count, and weights that land on one point add in
 * that order (fp64): the result is reproducible bit for bit.
 * No counterpart upstream: the reference hands the previous weights to OSQP by position.  All pointers DEVICE. */
int lmpc_shift_lambda_batch(lmpc_handle* h, int32_t batch, const int32_t* ss_idx_prev, const double* lambda_prev, const int32_t* ss_idx,
                            int32_t advance, double* lambda_ref);

/* accepted [batch] (DEVICE, int32): 1 where the most recent warm solve of this batch size on this handle (lmpc_solve_batch_warm,
 * lmpc_solve_batch_warm_ss) returned the active-set attempt's answer, 0 where the cold solve ran (refused attempt, or no warm kernel
 * for the configuration).  Written by the kernel itself.  The flags belong to
 * the LAST solve: any later cold solve through this handle (lmpc_solve_batch, _mixed, _ss_idx, _f32, lmpc_solve_full_dynamics_batch)
 * clears them, and a `batch` other than the warm solve's -- a smaller one included: there is no prefix of the flags -- gets zeros. */
int lmpc_get_warm_accepted(lmpc_handle* h, int32_t batch, int32_t* accepted);

/* Mixed precision (BASELINE configs[4]: "mixed fp32/fp64 KKT"): same arguments, layouts and fp64 arrays as
 * lmpc_solve_batch.  In fp64: the linearisation (discrete_dynamics_jacobian), the error-dynamics regression onto it when
 * lmpc_set_regression_laps is in effect, the centring of the abscissa on x_ic[0], the 2x2 pivots of the Riccati
 * recursion, the results and -- learning = 1 -- the simplex rows and the whole terminal elimination of the safe-set
 * block (racing_mpc.cpp:484-504).  In fp32: the stage records in LDS, the Riccati factor and sweeps and the stage rows --
 * half the LDS footprint, so twice the resident problems per CU where fp64 is capacity-bound.  Horizons: every N the
 * fp64 entry accepts for the tracking problem (iac_car_tracking_mpc.param.yaml ships N = 80); N <= 23 for the learning
 * problem.  A configuration without a reduced-precision kernel -- the learning problem at N >= 24 (barc_lmpc.param.yaml ships
 * N = 40: measured slower than fp64 in this layout), the hard hull equality -- is SOLVED IN FP64 by this entry (round 6;
 * it was LMPC_ERR_UNSUPPORTED): same results and statuses as lmpc_solve_batch, and lmpc_last_solve_precision() reports
 * LMPC_PRECISION_F64 for the call, so a caller iterating over horizons needs no special case and can still tell what ran
 * (lmpc_query_launch_for(h, LMPC_PRECISION_MIXED, ..) keeps answering LMPC_ERR_UNSUPPORTED for such a handle: "no mixed kernel").
 * Two passes when lmpc_config.polish = 0 (the default): the fp32 kernel ends with the active-set polish and a KKT test of
 * its answer (rows 1e-5, multipliers -1e-3, last step 1e-4, scaled); every problem whose answer did not pass -- polish
 * refused, out of iterations, infeasible by single-precision residuals -- is solved again by the fp64 kernel behind it,
 * which writes the fp64 entry's own answer and status over it (a percent of a batch).  Stated accuracy (scaled, against the fp64
 * answer; tests/tolerances.py): 1e-3 on every problem of the tracking configurations and of the learning problem on states near the
 * stored laps; on the learning workload of SURVEY.md 8(d) (random initial states) 1e-3 at the 99.99 % quantile and 5e-3 on every
 * problem -- a few problems per 32768 pass the single-precision KKT test with the weights of two or three nearly exchangeable
 * safe-set points off in the third digit (1.2 .. 3.4e-3 measured); away from the BASELINE shapes (every N, 96 / 160 points) 2e-3 on
 * every problem of 1024 per horizon, single problems up to 2.9e-3 at 4096 per horizon (profiles/r06_dispatch_sweep_4096.txt).
 * lmpc_solve_batch_f32 has no fp64 pass behind it: 1e-3 on the BASELINE shape (N = 40, every problem of 8192); over every horizon
 * from 3 to 81 at 4096 problems each (profiles/r06_dispatch_sweep_4096.txt) the worst single problems are 2.0 .. 2.2e-3 (N = 36, 75)
 * and at two horizons one problem of 4096 that the fp64 kernel solves is not solved.
 * Fit for well-scaled problems (IAC) and for the learning problem, NOT for the BARC
 * tracking problem at low speed, whose soft boundary needs complementarity below 1e-9.
 * polish < 0: one pass, the fp32 interior point's own answers (faster, a tail of problems up to 3e-2 away). */
int lmpc_solve_batch_mixed(lmpc_handle* h, int32_t batch, const double* x_ic, const double* u_ic,
                           const double* X_ref, const double* U_ref, const double* T_ref,
                           const double* bound_left, const double* bound_right, const double* curvatures,
                           const double* vel_ref, double total_length, const double* ss_x,
                           const double* ss_j, double* X_optm, double* U_optm, double* dU_optm,
                           double* convex_combi_optm, int32_t* status, int32_t* iters, double* kkt);

/* How many times a warm start (lmpc_solve_batch_warm, lmpc_solve_host_warm) may repair its working set before it is refused and
 * the cold start takes over: 1 .. 4 (the polish's own limit), or 0 for the default.  No counterpart upstream.  A round costs about
 * one interior-point iteration; a refused attempt has spent its rounds on top of the cold solve that follows, so it is the longest
 * job of its batch, and an accepted one the shortest.  In the closed loop at N = 20, 68 % of the attempts are accepted in the first
 * round, 95 % within two, 98 % within three, 99 % within four (N = 60: 22 / 73 / 82 / 89 %).  The default goes by the batch: 2
 * rounds while the batch is less than four times what the device holds at once (its duration is that of the longest jobs: refuse
 * early), 4 rounds beyond (throughput counts: every cold solve saved pays).  The answer does not depend on the setting -- an
 * accepted attempt is the optimum, a refused one falls back to the cold solve --; `iters` does: an accepted attempt reports its
 * rounds, a refused one its rounds + the cold solve's iterations. */
int lmpc_set_warm_rounds(lmpc_handle* h, int32_t rounds);

/* Single precision (BASELINE configs[3]: "IAC Putnam tracking MPC, N=40, ..., fp32"): the tracking problem with every
 * array in float and the interior point / Riccati recursion in fp32 (the linearisation is evaluated in fp64 and
 * rounded).  Same layouts and meaning as lmpc_solve_batch, no safe-set arguments; kkt [4][B] optional.  The abscissa
 * is carried relative to x_ic[0] inside the kernel (the QP is invariant to that shift), so a 2.8 km lap keeps its
 * resolution.  Stopping rule: complementarity <= max(tol, 2e-6), row residuals <= 1e-4, then the active-set polish in
 * fp32 (lmpc_config.polish >= 0).  There is no fp64 pass behind this entry (its arrays are float): an answer the polish
 * could not verify keeps status OPTIMAL at the interior point's accuracy.  Measured against fp64 on the IAC problem:
 * worst 4.6e-4 (scaled). */
int lmpc_solve_batch_f32(lmpc_handle* h, int32_t batch, const float* x_ic, const float* u_ic, const float* X_ref,
                         const float* U_ref, const float* T_ref, const float* bound_left, const float* bound_right,
                         const float* curvatures, const float* vel_ref, float* X_optm, float* U_optm, float* dU_optm,
                         int32_t* status, int32_t* iters, float* kkt);

/* RacingMPC::solve for ONE problem with HOST pointers in the reference's own (CasADi DM,
 * column-major) layout: X_ref is 6 x N with a knot's state contiguous, U_ref 2 x (N-1), the
 * per-knot rows are plain arrays.  Stages the data through buffers owned by the handle, runs
 * lmpc_solve_batch with batch = 1 and waits.  lmpc_solve_host synchronises the handle's stream, as do the other single-problem host
 * entry points below, lmpc_solve_host_warm, lmpc_solve_host_warm_ss and lmpc_solve_full_dynamics_host.  This is what the C++ facade (RacingMPC class,
 * racing-lmpc-ros2_amd/host/) calls.  ss_x is 6 x S column-major, ss_j has S entries
 * (learning only; NULL otherwise); convex_combi_optm may be NULL. */
int lmpc_solve_host(lmpc_handle* h, const double* x_ic, const double* u_ic, const double* X_ref,
                    const double* U_ref, const double* T_ref, const double* bound_left,
                    const double* bound_right, const double* curvatures, const double* vel_ref,
                    double total_length, const double* ss_x, const double* ss_j, double* X_optm,
                    double* U_optm, double* dU_optm, double* convex_combi_optm, int32_t* status,
                    int32_t* iters);

/* lmpc_solve_batch_warm for ONE problem with HOST pointers (layouts of lmpc_solve_host; X_optm_ref 6 x N, U_optm_ref 2 x (N-1)
 * column-major): what the facade's RacingMPC::solve calls when the warm-start keys are present and the controller has solved before. */
int lmpc_solve_host_warm(lmpc_handle* h, const double* x_ic, const double* u_ic, const double* X_ref, const double* U_ref,
                         const double* T_ref, const double* bound_left, const double* bound_right, const double* curvatures,
                         const double* vel_ref, double total_length, const double* X_optm_ref, const double* U_optm_ref, double* X_optm,
                         double* U_optm, double* dU_optm, int32_t* status, int32_t* iters);

/* lmpc_solve_batch_warm_ss for ONE problem with HOST pointers (layouts of lmpc_solve_host; convex_combi_optm_ref S values): what the
 * facade's RacingMPC::solve calls for a learning controller when `convex_combi_optm_ref` is among the inputs (racing_mpc.cpp:281). */
int lmpc_solve_host_warm_ss(lmpc_handle* h, const double* x_ic, const double* u_ic, const double* X_ref, const double* U_ref,
                            const double* T_ref, const double* bound_left, const double* bound_right, const double* curvatures,
                            const double* vel_ref, double total_length, const double* ss_x, const double* ss_j, const double* X_optm_ref,
                            const double* U_optm_ref, const double* convex_combi_optm_ref, double* X_optm, double* U_optm, double* dU_optm,
                            double* convex_combi_optm, int32_t* status, int32_t* iters);

/* RacingMPC(full_dynamics = true)::solve for a batch (racing_mpc.cpp:67-84: IPOPT on the problem whose dynamics rows are
 * x_{i+1} = f_d(x_i, u_i, k_i, t_i), :162-166, instead of their linearisation; the node uses it for its very first
 * solve, racing_mpc_node.cpp:299-314).  Sequential QPs over the batched kernels, globalised by a backtracking line search
 * on the l1 merit function cost + nu |dynamics defect|_1 (csrc/lmpc_sqp_kernel.hip): linearise about the iterate, solve
 * the QP, step, until the QP's own step falls below step_tol (scaled) or max_sqp QPs are spent.  A QP that is infeasible
 * about a new iterate (the step outran its linearisation) moves the iterate half way back and is linearised again, up to
 * 6 times in a row, before the problem stops with that status.  The iterate starts at
 * (X_ref, U_ref) -- the node hands its zero-input rollout, racing_mpc_node.cpp:210-235 -- with dU = 0, lambda = 0.
 * DEVICE pointers, layouts of lmpc_solve_batch.  Outputs: the iterate reached; status [B] = status of the last QP solved
 * for the problem; iters [B] = interior-point iterations summed over the QPs solved while the problem was still moving;
 * sqp_iters [B] = those QPs (steps taken + back-offs); sqp_move [B] = scaled |X_QP - X| of the last QP, the step it
 * proposed whatever part of it the line search took (converged iff <= step_tol); defect [B] =
 * |x_{i+1} - f_d(x_i, u_i)|_inf / scale_x of the iterate returned, after a step and after a back-off alike.  A problem that
 * never took a step -- its first QP failed -- returns the start unchanged (dU = 0, lambda = 0) with sqp_iters = 1, that QP's
 * status, sqp_move = +inf (never <= step_tol) and defect = 0: no defect is evaluated for it.  A learning handle needs ss_x and
 * ss_j (LMPC_ERR_ARGUMENT otherwise, before anything is written).  The first call for a batch size allocates a work area (like
 * lmpc_reserve).  Blocking: it synchronises the handle's stream once per QP (it has to know whether any problem is still moving). */
int lmpc_solve_full_dynamics_batch(lmpc_handle* h, int32_t batch, const double* x_ic, const double* u_ic, const double* X_ref,
                                   const double* U_ref, const double* T_ref, const double* bound_left,
                                   const double* bound_right, const double* curvatures, const double* vel_ref,
                                   double total_length, const double* ss_x, const double* ss_j, int32_t max_sqp,
                                   double step_tol, double* X_optm, double* U_optm, double* dU_optm,
                                   double* convex_combi_optm, int32_t* status, int32_t* iters, int32_t* sqp_iters,
                                   double* sqp_move, double* defect);

/* The same for ONE problem with HOST pointers (layouts of lmpc_solve_host): what the facade's
 * RacingMPC(config, model, full_dynamics = true) calls.  sqp_move / defect may be NULL. */
int lmpc_solve_full_dynamics_host(lmpc_handle* h, const double* x_ic, const double* u_ic, const double* X_ref,
                                  const double* U_ref, const double* T_ref, const double* bound_left,
                                  const double* bound_right, const double* curvatures, const double* vel_ref,
                                  double total_length, const double* ss_x, const double* ss_j, int32_t max_sqp,
                                  double step_tol, double* X_optm, double* U_optm, double* dU_optm,
                                  double* convex_combi_optm, int32_t* status, int32_t* iters, int32_t* sqp_iters,
                                  double* sqp_move, double* defect);

/* Safe set store: SafeSetManager::add_lap / SSTrajectory::process_lap_data
 * (safe_set.cpp:116-151).  HOST pointers: laps oldest first, lap j has n_pts[j] samples,
 * x is the concatenation of the laps' [n_pts[j]][6] row-major state tables.  The library
 * builds the +-L unrolled copies and the cost-to-go J on the device.  Blocking: synchronises the handle's stream (a query may still
 * read the old store), frees and allocates, and the upload has finished when it returns. */
int lmpc_set_safe_set(lmpc_handle* h, int32_t n_laps, const int32_t* n_pts, const double* x,
                      double total_length);

/* One query, HOST pointers, for the C++ facade's SafeSetManager::query: query[2] = (s, e_y); ss_x column-major
 * 6 x S and ss_j [S] as lmpc_ss_query_batch produces them (padded, J - J[0]); *j0 (optional) = the J[0] that was
 * subtracted, so that SSResult::J = ss_j + j0 on the first *n_found points.  Synchronises the handle's stream. */
int lmpc_ss_query_host(lmpc_handle* h, const double* query, double* ss_x, double* ss_j, int32_t* n_found, double* j0);

/* Error-dynamics regression on the recorded laps: RegQuery / RegResult (safe_set.hpp:57-88),
 * SSTrajectory::query(RegQuery) (safe_set.cpp:56-114), SafeSetManager::query(RegQuery) (:182-245) -- BASELINE
 * config 5.  For every linearisation point a kernel-weighted ridge regression of the nominal model's one-step error
 * over the lap samples within dist_max of [X_ref[in_state]; U_ref[in_ctrl]] is added onto (A, B, g):
 *   K_j = 0.75/h (1 - (d_j/h)^2)^2,  M = [z_j' 1],  R_r = (M'KM + 1e-3 I)^-1 M'K y_r,
 *   A[r, in_state] += R_r[0:ns],  B[r, in_ctrl] += R_r[ns:ns+nc],  g[r] += R_r[-1],
 * with y_r,j = x_{j+1}[r] - f_d(x_j, u_j, k_j, t_{j+1} - t_j)[r], so that the corrected model's one-step error on the
 * recorded samples is the least-squares residual (it shrinks).  The reference never calls this query and two of its
 * expressions do not type-check as written; the reading taken (same index lists for every regressed row, nominal step
 * evaluated on the full recorded state, residual of the regressed row) is documented in oracle/regression.py.
 * AS WRITTEN upstream the step is dt_j = t_j - t_{j+1} < 0 (process_lap_data, safe_set.cpp:130-135: the nominal model is
 * integrated backwards) and b = -M'K y (:229-231): the correction then points away from the data -- which is consistent
 * with the query having no caller.  `as_written = 1` reproduces exactly that for comparison; the default (0) is the
 * physically meaningful regression, and only that one should be switched on in front of a solve.
 * Built for (n_in_state + n_in_ctrl, n_out) = (5, 3) -- rows vx, vy, yaw rate on (vx, vy, yaw rate; u) -- and (8, 6). */
typedef struct lmpc_regression_spec {
  int32_t n_out;       /* reg_out_state_idxs: one state index per regressed row */
  int32_t out[6];
  int32_t n_in_state;  /* reg_in_state_idxs */
  int32_t in_state[6];
  int32_t n_in_ctrl;   /* reg_in_control_idxs */
  int32_t in_ctrl[2];
  int32_t as_written;  /* 0: dt = t_{j+1} - t_j, b = +M'K y (default); 1: the reference's literal signs (see above) */
  double dist_max;     /* RegQuery::dist_max, the kernel bandwidth h */
} lmpc_regression_spec;

/* HOST pointers, laps concatenated as in lmpc_set_safe_set: x [n][6], u [n][2], k [n] (curvature), t [n] (time
 * stamps) -- the lap_.x/u/k/t of SSTrajectory.  n_laps = 0 or spec = NULL switches the regression off.  While it is
 * on, lmpc_solve_batch applies it between its linearisation and its QP kernel.  With laps it is refused (LMPC_ERR_ARGUMENT)
 * while lmpc_fleet_ss_set_regression is in effect.  Blocking: synchronises the handle's stream before the old tables are freed and
 * again behind the kernels that build the new ones. */
int lmpc_set_regression_laps(lmpc_handle* h, int32_t n_laps, const int32_t* n_pts, const double* x, const double* u,
                             const double* k, const double* t, const lmpc_regression_spec* spec);

/* RegResult{A, B, C} for a batch: adds the regression onto A [6][6][N-1][B], Bm [6][2][N-1][B], g [6][N-1][B]
 * (the arrays of lmpc_linearize_batch; DEVICE pointers), linearisation points X_ref [6][N][B], U_ref [2][N-1][B]. */
int lmpc_regress_batch(lmpc_handle* h, int32_t batch, const double* X_ref, const double* U_ref, double* A, double* Bm,
                       double* g);

/* SafeSetManager::query(SSQuery) + the pad/truncate and J - J[0] of RacingMPC::solve
 * (safe_set.cpp:153-180, trajectory_kd_tree.cpp:53-63, racing_mpc.cpp:249-280):
 *   query [2][B] = (s, e_y) of X_ref[:, N-1] after abscissa alignment  ->
 *   ss_x [6][S][B], ss_j [S][B] (J - J[0]), n_found [B] (points before padding).           */
int lmpc_ss_query_batch(lmpc_handle* h, int32_t batch, const double* query, double* ss_x,
                        double* ss_j, int32_t* n_found);

/* The same query BY REFERENCE (round 5; no counterpart upstream, where the query returns copies, safe_set.cpp:153-180): instead
 * of the 7 S doubles per query of (ss_x, ss_j) the kernel leaves S int32 codes, ss_idx [S][B],
 *     code = (row of the point in the concatenated lap store of lmpc_set_safe_set) * 4 + rep,   rep = 0 / 1 / 2: the copy of the
 *            lap shifted by -L / 0 / +L (SSTrajectory::process_lap_data, :122-128);  -1: no point (nothing stored, NaN query)
 * padded with the last point's code (racing_mpc.cpp:263-272), and lmpc_solve_batch_ss_idx gathers the points from the store
 * itself: 640 B per query at S = 160 instead of 8960 B written here and read back by the QP kernel.  Same neighbours in the same
 * order as lmpc_ss_query_batch (one kernel, two output forms); the solve on them gives bit for bit the same result. */
int lmpc_ss_query_idx_batch(lmpc_handle* h, int32_t batch, const double* query, int32_t* ss_idx, int32_t* n_found);

/* lmpc_solve_batch (precision = LMPC_PRECISION_F64) or lmpc_solve_batch_mixed (LMPC_PRECISION_MIXED) for the learning problem with
 * the safe set by reference: ss_idx [S][B] from lmpc_ss_query_idx_batch ON THIS HANDLE, against the store lmpc_set_safe_set left
 * on it.  The store must be the one the query ran against: after another lmpc_set_safe_set (or without a query on this handle) the
 * call is refused with LMPC_ERR_ARGUMENT, and a code that names no row of the store is read as "no point" (-1), never out of bounds.
 * Everything else as lmpc_solve_batch. */
int lmpc_solve_batch_ss_idx(lmpc_handle* h, int32_t batch, int32_t precision, const double* x_ic, const double* u_ic, const double* X_ref,
                            const double* U_ref, const double* T_ref, const double* bound_left, const double* bound_right,
                            const double* curvatures, const double* vel_ref, double total_length, const int32_t* ss_idx, double* X_optm,
                            double* U_optm, double* dU_optm, double* convex_combi_optm, int32_t* status, int32_t* iters, double* kkt);

/* Cold-start input preparation of RacingMPCNode::on_step_timer
 * (racing_mpc_node.cpp:210-235,261-292): U_ref = 1e-9, X_ref rolled out with the RK4
 * model and the track curvature at each knot, references sampled from the track tables,
 * vel_ref clamped to vx +- max_vel_ref_diff and the speed limit.
 *   in : x_ic [6][B], dt, speed_scale, speed_limit
 *   out: X_ref [6][N][B], U_ref [2][N-1][B], T_ref [N-1][B], bound_left, bound_right,
 *        curvatures, vel_ref [N][B]                                                         */
int lmpc_prepare_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, const double* x_ic,
                       double dt, double speed_scale, double speed_limit, double* X_ref,
                       double* U_ref, double* T_ref, double* bound_left, double* bound_right,
                       double* curvatures, double* vel_ref);

/* The same cold start for the problems whose last solve failed only (status[b] != 0), in place: the arrays of the
 * others are left as they are.  What re-launching the node does for one car (racing_mpc_node.cpp:210-235), for a
 * closed-loop batch that keeps going without a host round trip: call it on the output of lmpc_shift_batch.         */
int lmpc_prepare_failed_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, const double* x_ic,
                              const int32_t* status, double dt, double speed_scale, double speed_limit,
                              double* X_ref, double* U_ref, double* T_ref, double* bound_left,
                              double* bound_right, double* curvatures, double* vel_ref);

/* Warm-start shift of RacingMPCNode::on_step_timer (racing_mpc_node.cpp:245-254, 261-292): the previous
 * solution moves one knot forward, the last input is repeated, the last state is rolled out with the model
 * and the references are re-sampled at the shifted abscissa.  Per problem, `status` (may be NULL) selects the
 * previous solution (X_sol, U_sol; status 0) or the previous reference (X_old, U_old) when the solve failed
 * (racing_mpc_node.cpp:322-332).  Outputs must not alias inputs. */
int lmpc_shift_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, const double* X_sol,
                     const double* U_sol, const double* X_old, const double* U_old, const int32_t* status,
                     double dt, double speed_scale, double speed_limit, double* X_ref, double* U_ref,
                     double* T_ref, double* bound_left, double* bound_right, double* curvatures,
                     double* vel_ref);

/* Plant step of RacingSimulator::step (racing_simulator.cpp:46-69,97-112): x [6][B] advanced in place by
 * `n_sub` RK4 sub-steps of dt_sim with u [2][B] held, curvature looked up at the current abscissa, abscissa
 * wrapped into [0, L). */
int lmpc_plant_step_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, double* x,
                          const double* u, double dt_sim, int32_t n_sub);

/* Everything between two solves of a closed loop in ONE launch: what RacingMPCNode::on_step_timer does with a solve's result and
 * what the simulator does with the node's command, for a batch of cars.  Per car:
 *   the input applied  -- the plan's first input U_optm[:, 0], or after a failed solve (status != 0) the first input of the plan the
 *                         solve started from, U_ref[:, 0] (racing_mpc_node.cpp:322-332); written to u_prev [2][B] (the next u_ic);
 *   the plant          -- lmpc_plant_step_batch on x [6][B] in place (racing_simulator.cpp:46-69,97-112);
 *   the next inputs    -- lmpc_shift_batch (racing_mpc_node.cpp:245-254) from the solution, or from the old plan after a failed
 *                         solve; with restart_failed != 0 a car whose solve failed is instead prepared from a cold start at its
 *                         new state (lmpc_prepare_failed_batch; racing_mpc_node.cpp:210-235) -- X_ref, U_ref, T_ref, bound_left,
 *                         bound_right, curvatures, vel_ref are updated IN PLACE (they must not alias X_optm / U_optm);
 *   bookkeeping        -- optional accumulators, any of them NULL: distance [B] += abscissa travelled (unwrapped), worst_excess [B]
 *                         = max(itself, excursion of the body beyond the track edge at the new state against the bounds of knot 0),
 *                         n_fail [B] += 1 after a failed solve, *n_accepted += number of cars with status 0 whose warm start was
 *                         accepted (the warm kernel's own flag, lmpc_get_warm_accepted).  It counts only when the last solve on
 *                         this handle was lmpc_solve_batch_warm / _warm_ss of the same batch size; after any other solve it adds 0
 *                         (`iters` is no longer read; it must still be non-NULL where n_accepted is given).
 * The same arithmetic as the three entry points it replaces -- bit for bit, except that the last knot of a shifted solution (one model
 * step from the knot before it) may differ by 1 - 2 ulp, the compiler contracting the inlined model differently in the two kernels
 * (tests/test_gpu_loop.py) --; a period of a closed loop is then
 * three launches -- linearisation, QP, this -- instead of ~45.  SOA result layout only.  All pointers DEVICE. */
int lmpc_loop_advance_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, const int32_t* status, const int32_t* iters,
                            const double* X_optm, const double* U_optm, double* x, double* u_prev, double dt, double dt_sim,
                            int32_t n_sub, double speed_scale, double speed_limit, int32_t restart_failed, double* X_ref,
                            double* U_ref, double* T_ref, double* bound_left, double* bound_right, double* curvatures,
                            double* vel_ref, double* distance, double* worst_excess, int64_t* n_fail, uint64_t* n_accepted);

/* Layout of the RESULT arrays X_optm, U_optm, dU_optm of lmpc_solve_batch and lmpc_solve_batch_mixed AS THE CALLER INVOKES THEM
 * (inputs, status, iters, kkt and convex_combi_optm are not affected).  Nothing else follows the setting: lmpc_solve_batch_f32,
 * lmpc_solve_full_dynamics_batch (its inner QPs feed the line search and the next linearisation), the single-problem host
 * entry points (lmpc_solve_host, lmpc_solve_full_dynamics_host: column-major host arrays either way) and lmpc_shift_batch
 * (which READS a solution) always use the default layout.  LMPC_LAYOUT_SOA (default): [component][knot][batch], what batch-parallel
 * consumers (lmpc_shift_batch, lmpc_plant_step_batch, a result gather) read coalesced.  LMPC_LAYOUT_AOS: [batch][knot]
 * [component] -- per problem the reference's own DM layout (column-major 6 x N, 2 x (N-1); racing_mpc.cpp:347-349), for a
 * consumer that takes one problem's plan at a time; one wavefront's 196 results then leave as full cache lines instead of
 * eight-byte stores at stride B (measured HBM write traffic of the QP kernel: profiles/r03_*). */
#define LMPC_LAYOUT_SOA 0
#define LMPC_LAYOUT_AOS 1
int lmpc_set_output_layout(lmpc_handle* h, int32_t layout);

/* Grow the handle's device workspace (stage linearisations, 432 B per stage per problem; the list of a mixed solve's
 * unverified problems; the polish's save area, 10 N - 4 values per problem) so that no later *_batch call with
 * batch <= max_batch allocates.  lmpc_solve_batch_f32 needs none of the fp64 workspace: it grows its own fp32 workspace and
 * the save area on the first call for a batch size.  Blocking when it grows anything: the stream is drained before a buffer it may
 * still read is released (the same holds for the first *_batch call of a larger batch on a handle that was not reserved). */
int lmpc_reserve(lmpc_handle* h, int32_t max_batch);

/* Launch order of the QP kernel's workgroups (no counterpart upstream: a scheduling aid for closed-loop batches).  The
 * hardware starts workgroups in index order and a batch of 4096 fills the GPU twice, so the kernel's duration is that of
 * the problems that happen to start last.  With `order` -- DEVICE int32 [batch], a permutation of 0 .. batch-1 (not
 * checked: an entry outside the range skips that workgroup, a repeated one leaves another problem's outputs untouched) --
 * workgroup w solves problem order[w]; lmpc_launch_order_from_iters fills it from the iteration counts of the previous
 * solve of the same cars, longest first (runs on the handle's stream, graph-capturable).  Results per problem do not
 * depend on the order.  The order applies to lmpc_solve_batch* calls of exactly `batch` problems; calls with any other
 * batch size (and the single-problem host entry points) keep the default XCD-aware mapping.  order = NULL restores the
 * default for every size.  The pointer is kept, not copied: it must stay valid, and must not be rewritten while a solve
 * that reads it is in flight (one buffer per stream). */
int lmpc_set_launch_order(lmpc_handle* h, const int32_t* order, int32_t batch);
int lmpc_launch_order_from_iters(lmpc_handle* h, int32_t batch, const int32_t* iters, int32_t* order);

/* Library/kernel facts for harnesses: bytes of LDS one problem occupies, threads per problem. */
int lmpc_query_launch(const lmpc_handle* h, int32_t* lds_bytes_per_problem,
                      int32_t* threads_per_problem);

/* Occupancy of the QP kernel as the runtime reports it: resident problems (= wavefronts) per CU. */
int lmpc_query_residency(lmpc_handle* h, int32_t* problems_per_cu);

/* The same two facts for the kernel a given entry point launches: LMPC_PRECISION_F64 (lmpc_solve_batch),
 * LMPC_PRECISION_F32 (lmpc_solve_batch_f32) or LMPC_PRECISION_MIXED (the fp32 iteration of lmpc_solve_batch_mixed; its fp64
 * second pass is the F64 kernel).  LMPC_ERR_UNSUPPORTED when that entry point has no kernel for the handle's (N, num_ss_pts). */
#define LMPC_PRECISION_F64 0
#define LMPC_PRECISION_F32 1
#define LMPC_PRECISION_MIXED 2
int lmpc_query_launch_for(lmpc_handle* h, int32_t precision, int32_t* lds_bytes_per_problem, int32_t* problems_per_cu);

/* Wavefronts per problem of the cold fp64 tracking solve (lmpc_solve_batch; no counterpart upstream): 0 (default) the library's choice
 * by horizon, 1 one wavefront per problem (every configuration), 2 two wavefronts per problem on one LDS record -- the inequality
 * rows dealt to 128 lanes, the Riccati chains on the first wave (csrc/lmpc_solve_w2.hip.h): built for N >= 24; where it is not
 * built (N <= 23, the learning problem, reduced precision, the warm start) the setting is ignored.  Same algorithm, same
 * contract; the answers differ from the one-wave kernel's by the order of a few wave-wide sums (1e-12). */
int lmpc_set_waves_per_problem(lmpc_handle* h, int32_t waves);

/* The precision the most recent batched solve on this handle ran in: LMPC_PRECISION_MIXED after lmpc_solve_batch_mixed (or
 * lmpc_solve_batch_ss_idx with that precision) where a reduced-precision kernel exists for the handle's (N, num_ss_pts),
 * LMPC_PRECISION_F64 where the entry fell back to the fp64 kernels (above), LMPC_PRECISION_F32 after lmpc_solve_batch_f32. */
int lmpc_last_solve_precision(const lmpc_handle* h, int32_t* precision);

/* Per-kernel timing for benchmarks: when enabled, lmpc_solve_batch brackets its two launches
 * with HIP events on the handle's stream; lmpc_last_kernel_ms waits for them and returns the
 * durations of the linearisation kernel and of the QP kernel of the most recent call (blocking: it waits for those events, that is,
 * for the solve they bracket; lmpc_enable_timing itself is host-only). */
int lmpc_enable_timing(lmpc_handle* h, int32_t on);
int lmpc_last_kernel_ms(lmpc_handle* h, float* linearize_ms, float* solve_ms);

/* Fleet safe set: one SafeSetRecorder and one SafeSetManager PER CAR, on the device.  Upstream every controller owns both
 * (RacingMPC::solve calls ss_recorder_->step and ss_manager_->query on its own members, racing_mpc.cpp:246-255), so a fleet of B
 * controllers is B recorders and B stores; lmpc_set_safe_set above is ONE store shared by every query of a handle.
 *   per car: a ring of lmpc_config.max_lap_stored closed laps (boost::circular_buffer, safe_set.cpp:139-151), the open lap being
 *   recorded (last_x_ / last_u_ / last_k_ / last_t_, :278-322), the recorder's flags and lap_count, and -- no counterpart upstream --
 *   n_dropped and the durations of the last closed laps; per sample x[6], u[2], k, t, what the reference writes to its lap files.
 * lmpc_fleet_ss_create allocates batch x (max_lap_stored + 1) x max_pts_per_lap samples of 80 bytes (4096 cars x 6 x 1024: 2.0 GB;
 * lmpc_fleet_ss_bytes tells what it took) and replaces an earlier store; sizes that would overflow are LMPC_ERR_ARGUMENT, an
 * allocation the device refuses LMPC_ERR_RUNTIME (no store is left then).  max_lap_stored must be positive.  lmpc_destroy frees the
 * store; lmpc_fleet_ss_reset empties every car without reallocating (asynchronous, on the handle's stream).
 * DEPARTURE from the reference, whose laps are unbounded: a lap slot holds max_pts_per_lap samples.  An open lap that reaches that
 * many stops storing and is marked overflowed; when it closes it is NOT added to the ring, evicts nothing, and n_dropped[b] goes up
 * by one (lap_count and the duration are kept as for any lap).  Nothing is ever written outside a car's slots.
 * Every call names the store's own batch (LMPC_ERR_ARGUMENT otherwise, and without a store).  The store serves the array form of the
 * safe set only: the by-reference codes (lmpc_ss_query_idx_batch, lmpc_solve_batch_ss_idx, lmpc_solve_batch_warm_ss with ss_idx,
 * lmpc_shift_lambda_batch) name rows of the shared store and have no fleet form.  The error-dynamics regression has one:
 * lmpc_fleet_ss_set_regression / lmpc_fleet_ss_regress_batch below (lmpc_set_regression_laps stays one store per handle).
 * lmpc_fleet_ss_create and lmpc_fleet_ss_destroy are blocking: an existing store is released only after the handle's stream has been
 * waited for (destroy synchronises the handle's stream), and they allocate / free; the zero-fill of a new store is enqueued on the
 * handle's stream.  lmpc_fleet_ss_bytes is host-only. */
int lmpc_fleet_ss_create(lmpc_handle* h, int32_t batch, int32_t max_pts_per_lap);
int lmpc_fleet_ss_destroy(lmpc_handle* h);
int lmpc_fleet_ss_reset(lmpc_handle* h);
int lmpc_fleet_ss_bytes(const lmpc_handle* h, int64_t* bytes); /* 0 without a store */

/* SafeSetRecorder::step (safe_set.cpp:278-322) for every car, one launch, one thread per car, asynchronous on the handle's stream
 * without a host round trip (legal inside a captured control period): x [6][B], u [2][B], k [B] (curvature) DEVICE, t and
 * total_length host values.  The first sample of a car only seeds its abscissa; a lap closes when s_prev - s > total_length / 2;
 * the first, partial lap is discarded; a closed lap is pushed into the car's ring (the oldest leaves a full ring) and the closing
 * sample starts the next lap -- including the reference's quirk that jitter across the start line makes very short laps.
 * active [B] (DEVICE, may be NULL): 0 skips the car for this sample (e.g. a diverged state, at the caller's choice). */
int lmpc_fleet_ss_record_batch(lmpc_handle* h, int32_t batch, const double* x, const double* u, const double* k, double t,
                               double total_length, const int32_t* active);

/* lmpc_ss_query_batch with query b run against car b's ring, newest lap first: same outputs (ss_x [6][S][B], ss_j [S][B] = J - J[0],
 * n_found [B]), padding, truncation, tie rule and NaN behaviour, bit-equal on equal stores; a car without a closed lap gives
 * n_found = 0 and zero-filled outputs.  The results go to lmpc_solve_batch / lmpc_solve_batch_mixed as ss_x, ss_j.  The laps are
 * unrolled by the total_length of the last lmpc_fleet_ss_record_batch / lmpc_fleet_ss_load.  num_ss_pts_per_lap <= 64. */
int lmpc_fleet_ss_query_batch(lmpc_handle* h, int32_t batch, const double* query, double* ss_x, double* ss_j, int32_t* n_found);

/* SafeSetRecorder::load (safe_set.cpp:260-276) for car `car`, or for every car with car = -1.  HOST pointers, laps oldest first and
 * concatenated as in lmpc_set_regression_laps: x [n][6], u [n][2], k [n], t [n].  The laps are pushed into the ring behind those it
 * holds (an open lap stays open); lap_count grows by n_laps; no duration is recorded for them.  A lap longer than the store's
 * max_pts_per_lap is refused (LMPC_ERR_ARGUMENT, nothing loaded).  Synchronises the handle's stream. */
int lmpc_fleet_ss_load(lmpc_handle* h, int32_t car, int32_t n_laps, const int32_t* n_pts, const double* x, const double* u,
                       const double* k, const double* t, double total_length);

/* One car's closed laps, oldest first, to HOST arrays (tests, lap files, inspection): *n_laps, n_pts [max_lap_stored], and the
 * concatenated x [n][6], u [n][2], k [n], t [n], each optional.  Call it with the sample arrays NULL for the sizes, then with
 * arrays of sum(n_pts) samples.  Synchronises the handle's stream. */
int lmpc_fleet_ss_get_laps(lmpc_handle* h, int32_t car, int32_t* n_laps, int32_t* n_pts, double* x, double* u, double* k, double* t);

/* Per-car counters to DEVICE arrays [B], any of them NULL: laps in the ring, the recorder's lap_count (every crossing and every
 * loaded lap), laps dropped for their length, and the duration of the last lap closed by the recorder -- t at the closing crossing
 * minus t of the lap's first sample, 0 before the first.  Asynchronous on the handle's stream. */
int lmpc_fleet_ss_stats(lmpc_handle* h, int32_t batch, int32_t* laps_in_ring, int32_t* lap_count, int32_t* n_dropped,
                        double* last_lap_time);

/* Everything between two solves of a FLEET LMPC period in ONE launch: what lmpc_loop_advance_batch does for the tracking loop, for
 * the experiment in which every car learns from its own laps (each car a RacingMPCNode with its own SafeSetRecorder and
 * SafeSetManager, driven by the tracking controller until its ring holds warm_laps laps and by the learning controller after).  The
 * per-car phase, the lap book and the next k-NN query point live on the device; the host may run many periods without reading
 * anything.  Called on the LEARNING handle (the one that owns the fleet store); the tracking controller is a second handle with the
 * same N and vehicle, and only its results come here.  Per car b, in this order:
 *   1 the solution     -- sel = phase[b] as it stands at entry (0 tracking, 1 learning) picks (X_trk, U_trk, status_trk) or (X_lrn,
 *                         U_lrn, status_lrn), X [6][N][B], U [2][N-1][B], status [B]; a triple may be absent (all three NULL: that
 *                         controller did not run), and a car of an absent triple counts as a failed solve;
 *   2 input and plant  -- as lmpc_loop_advance_batch: U_sel[:, 0], or U_ref[:, 0] after a failed solve (racing_mpc_node.cpp:322-332),
 *                         written to u_prev [2][B]; n_sub sub-steps of dt_sim on x [6][B] in place (racing_simulator.cpp:46-69,97-112),
 *                         with the vehicle *plant (HOST, may be NULL: the handle's) -- a plant that differs from the controllers'
 *                         model is what gives the per-car regression something to learn; the optional accumulators distance [B],
 *                         worst_excess [B] (against knot 0 of the bounds of the period just driven), n_fail [B], any of them NULL;
 *   3 the next inputs  -- the shift of the solution (racing_mpc_node.cpp:245-254), the shift of the old plan in place after a failed
 *                         solve, or with restart_failed != 0 the cold start at the new state (:210-235, 261-292), with the phase's
 *                         own speed_scale[sel], speed_limit[sel], max_vel_ref_diff[sel] (each controller node has its own) and the
 *                         handle's vehicle; X_ref [6][N][B], U_ref [2][N-1][B], T_ref [N-1][B], bound_left, bound_right, curvatures,
 *                         vel_ref [N][B] are updated IN PLACE (they must not alias a solution);
 *   4 x_ic [6][B]      -- the new state; for sel = 1 projected onto the handle's [x_min, x_max] (the state box also binds knot 0,
 *                         racing_mpc.cpp:147,201);
 *   5 the recorder     -- lmpc_fleet_ss_record_batch with (new state, input applied, track curvature at the new abscissa, t) and
 *                         the track's L (RacingMPC::solve, racing_mpc.cpp:246): seeding, the discarded partial lap, the close, the
 *                         eviction, the overflowed lap dropped, the duration ring;
 *   6 the lap book     -- when that sample closed a lap and lap_count before it was >= 1: lap_time [n_rec][B] and lap_kind
 *                         [n_rec][B] at slot lap_count_before - 1 get the lap's duration and sel (slots >= n_rec are not written),
 *                         n_learn[b] += sel, and counters[1] += 1 when n_learn[b] reaches learn_laps;
 *   7 the phase        -- with switch_phase != 0: phase[b] 0 -> 1 when the car's ring holds >= warm_laps laps, counters[0] += 1.
 *                         With switch_phase == 0 no phase changes (the host that polls every p periods passes it only then, so
 *                         that which controllers it launches stays true until it looks again);
 *   8 query [2][B]     -- the point lmpc_fleet_ss_query_batch is asked next: (s, e_y) of the last knot of the new X_ref, s aligned
 *                         with the new (unprojected) abscissa by align_abscissa (racing_mpc.cpp:219-223,249-254).
 * HEAD-ONLY call: with all six solution pointers NULL steps 1 - 3 are skipped -- no input, no plant, the references stay as
 * lmpc_prepare_batch left them -- and steps 4 - 8 run on x as given with u_prev as the recorded input: period 0.
 * phase, n_learn [B], lap_kind [n_rec][B], counters [2] are int32, caller-owned and zero-filled for a fresh experiment, as are
 * lap_time, x_ic and query; counters are monotone and never zeroed here: cars that have entered the learning phase, cars that have
 * their learn_laps.  The same arithmetic as the entry points it replaces (tests/test_gpu_fleet_loop.py: bit for bit but for the
 * last knot's one-step rollout, as lmpc_loop_advance_batch).  Asynchronous on the handle's stream; allocates nothing and reads
 * nothing back.  LMPC_ERR_ARGUMENT, with nothing written: no fleet store or a batch other than its; a NULL required pointer or a bad
 * track; one or two members of a solution triple NULL; dt, dt_sim not positive, n_sub, warm_laps, learn_laps or n_rec < 1; a plant
 * whose model_id or integrator is not built; references aliasing a solution.  LMPC_ERR_UNSUPPORTED with LMPC_LAYOUT_AOS on the
 * handle.  All pointers DEVICE except plant. */
typedef struct lmpc_fleet_loop {
  const double* X_trk;         /* the tracking controller's solution, or all three NULL */
  const double* U_trk;
  const int32_t* status_trk;
  const double* X_lrn;         /* the learning controller's solution, or all three NULL */
  const double* U_lrn;
  const int32_t* status_lrn;
  double* x;                   /* [6][B] in place */
  double* u_prev;              /* [2][B] */
  double* X_ref;
  double* U_ref;
  double* T_ref;
  double* bound_left;
  double* bound_right;
  double* curvatures;
  double* vel_ref;
  double dt, dt_sim, t;        /* control period, plant sub-step, the time stamp of the sample recorded */
  double speed_scale[2], speed_limit[2], max_vel_ref_diff[2]; /* [0] tracking, [1] learning */
  int32_t n_sub, restart_failed, warm_laps, learn_laps, switch_phase, n_rec;
  const lmpc_vehicle* plant;   /* HOST, may be NULL */
  int32_t* phase;              /* [B] */
  int32_t* n_learn;            /* [B] */
  double* lap_time;            /* [n_rec][B] */
  int32_t* lap_kind;           /* [n_rec][B] */
  int32_t* counters;           /* [2] */
  double* x_ic;                /* [6][B] */
  double* query;               /* [2][B] */
  double* distance;            /* [B], optional */
  double* worst_excess;        /* [B], optional */
  int64_t* n_fail;             /* [B], optional */
} lmpc_fleet_loop;
int lmpc_fleet_loop_advance_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, const lmpc_fleet_loop* io);

/* Per-car error-dynamics regression: SafeSetManager::query(RegQuery) (safe_set.cpp:182-245) as B controllers call it, each on the
 * laps of its OWN SafeSetManager -- lmpc_set_regression_laps / lmpc_regress_batch above with query (b, i) run against the closed laps
 * in car b's ring at the time of each call.  Same spec, same arithmetic, same two sign conventions (the comment at
 * lmpc_regression_spec); the weights are always formed from sum (z - q)^2.  Only closed laps in the ring count: not the open lap
 * being recorded, not a lap dropped for its length, not a lap the ring has evicted.
 * lmpc_fleet_ss_set_regression uploads NO data.  It validates the spec exactly as lmpc_set_regression_laps does ((features, rows)
 * other than (5, 3) and (8, 6): LMPC_ERR_UNSUPPORTED; an index out of range or dist_max <= 0: LMPC_ERR_ARGUMENT), needs a fleet store
 * (LMPC_ERR_ARGUMENT without one) and allocates, per car, a packed table of max_lap_stored x (max_pts_per_lap - 1) samples rounded
 * up to four, 8 (features + rows + 1) bytes each -- 72 for (5, 3), 120 for (8, 6); 4096 cars x 5 x 1023 x 72: 1.5 GB;
 * lmpc_fleet_ss_bytes includes it -- and nothing later allocates.  The tables are filled on the device, in front of each use, for
 * the cars whose ring has changed since their last fill (a lap closed or was loaded: lap_count moved on); the caller does nothing
 * for that and no call reads the device.  Calling it again with another spec re-validates and refills (it synchronises the
 * handle's stream only when the table's size changes).  spec = NULL switches it off and frees the table, as do lmpc_fleet_ss_create
 * (which replaces the store) and lmpc_fleet_ss_destroy.  It is refused (LMPC_ERR_ARGUMENT) while lmpc_set_regression_laps is in
 * effect, and lmpc_set_regression_laps with laps is refused while this is: a handle corrects its model from one source.
 * While it is on: every fp64 / mixed batched solve (lmpc_solve_batch, _mixed, _warm, _warm_ss, _ss_idx, the QPs of
 * lmpc_solve_full_dynamics_batch) applies it between its linearisation and its QP kernel, where lmpc_set_regression_laps applies
 * the shared one, and must name the store's batch -- another batch is LMPC_ERR_ARGUMENT before anything is written; the
 * single-problem host entries (lmpc_solve_host*, lmpc_solve_full_dynamics_host) are a batch of one and follow the same rule;
 * lmpc_solve_batch_f32 returns LMPC_ERR_UNSUPPORTED. */
int lmpc_fleet_ss_set_regression(lmpc_handle* h, const lmpc_regression_spec* spec);

/* lmpc_regress_batch with query (b, i) run against car b's own ring: adds RegResult{A, B, C} onto A [6][6][N-1][B],
 * Bm [6][2][N-1][B], g [6][N-1][B] (the arrays of lmpc_linearize_batch; DEVICE pointers), linearisation points X_ref [6][N][B],
 * U_ref [2][N-1][B].  batch must be the store's.  A car without a closed lap, and a query with no sample inside the bandwidth,
 * leave their entries bit-identical (safe_set.cpp:207-210).  Two launches, asynchronous on the handle's stream, no host round trip
 * and no allocation (legal inside a captured control period). */
int lmpc_fleet_ss_regress_batch(lmpc_handle* h, int32_t batch, const double* X_ref, const double* U_ref, double* A, double* Bm,
                                double* g);

/* The regression with one feature list per regressed row, shared (lmpc_set_regression_laps_rows) and per car
 * (lmpc_fleet_ss_set_regression_rows), and its spec lmpc_regression_rows_spec: declared in lmpc_hip_rows.h. */
#include "lmpc_hip_rows.h"
#include "lmpc_hip_cars.h"
#include "lmpc_hip_dtrack.h"
/* The fused fleet LMPC period on the double-track table (lmpc_fleet_loop_advance_dtrack_batch): declared in lmpc_hip_fleet_dtrack.h. */
#include "lmpc_hip_fleet_dtrack.h"
/* The double-track controller model (lmpc_linearize_dtrack_batch, lmpc_dtrack_set_controller_model, lmpc_dtrack_get_controller_model):
 * declared in lmpc_hip_dtrack_model.h. */
#include "lmpc_hip_dtrack_model.h"
/* The per-car single-track controller model (lmpc_linearize_cars_batch, lmpc_cars_set_controller_model, lmpc_cars_get_controller_model):
 * declared in lmpc_hip_cars_model.h. */
#include "lmpc_hip_cars_model.h"
/* The fused estimated period (sensors, EKF, projection, plant and shift in one launch; its io struct lmpc_estimated_loop): declared
 * in lmpc_hip_estimated.h. */
#include "lmpc_hip_estimated.h"

/* Spline track: RacingTrajectory's interpolants on the device (racing_trajectory.cpp:25-120) and the two conversions built on them.
 * The five interpolating not-a-knot cubics -- x, y, speed, left and right boundary offset over the abscissa of the waypoints, closed by
 * the last three waypoints in front (-L) and the first four behind (+L), :48-59 -- are fitted on the HOST, once per track
 * (RacingTrajectory::to_spline_track in racing-lmpc-ros2_amd/host/ and racing_trajectory.py), and handed over as piecewise polynomials:
 *   L              total length
 *   breaks [P+1]   the extended waypoint abscissae, strictly increasing
 *   coef [5][P][4] a, b, c, d of  a + b h + c h^2 + d h^3,  h = s - breaks[piece];  curves in the order x, y, vel, left, right
 *   wp_x, wp_y, wp_s [n_wp]   the waypoints and their abscissae (the projection's unseeded start; their median spacing is its step bound)
 * lmpc_spline_track_create takes HOST pointers, uploads once and synchronises the handle's stream; the track belongs to the device of
 * the handle that made it and is used with handles on that device.  lmpc_spline_track_destroy waits for the handle's stream first.
 * Every evaluation is at align_abscissa(s, L/2, L) (:98), on the piece whose left break is the last one <= that (end pieces extrapolate).
 * Rules of the entries below: launches go on the handle's stream; data pointers are DEVICE pointers; argument errors return
 * LMPC_ERR_ARGUMENT with a message on the handle; no call allocates. */
typedef struct lmpc_spline_track lmpc_spline_track;
int lmpc_spline_track_create(lmpc_handle* h, double L, int32_t P, const double* breaks, const double* coef, int32_t n_wp,
                             const double* wp_x, const double* wp_y, const double* wp_s, lmpc_spline_track** track);
int lmpc_spline_track_destroy(lmpc_handle* h, lmpc_spline_track* track);

/* The interpolants at n abscissae s [n] (any value: wrapped): out [7][n] = x, y, yaw, curvature, left, right, vel --
 * x/y/yaw/curvature/left_boundary/right_boundary/velocity_interpolation_function (racing_trajectory.cpp:100-118), the curvature being
 * the expression as written there, x' y'' - y' x'' / sqrt((x'^2 + y'^2)^3) (:108-110). */
int lmpc_track_sample_batch(lmpc_handle* h, const lmpc_spline_track* track, int32_t n, const double* s, double* out);

/* The four tables of an lmpc_track with M samples, s_j = j L / M, filled on the device (curvature, bound_left, bound_right, vel: DEVICE
 * [M]) -- what RacingMPCNode samples per knot (racing_mpc_node.cpp:261-266) without the host evaluating 4 M interpolants. */
int lmpc_spline_track_tabulate(lmpc_handle* h, const lmpc_spline_track* track, int32_t M, double* curvature, double* bound_left,
                               double* bound_right, double* vel);

/* RacingTrajectory::global_to_frenet for a batch (racing_trajectory.cpp:137-186, 204-236; RacingMPCNode::on_step_timer,
 * racing_mpc_node.cpp:181-185; racing_simulator_node.cpp:60-65):  pose [3][B] = (x, y, yaw)  ->  frenet [3][B] = (s, t, xi) with s in
 * [0, L], and status [B].  Start of the search per pose: s0[b] when s0 != NULL and (seeded == NULL or seeded[b] != 0) and s0[b] is
 * finite -- `initialize_with_previous`, :204-212 --, otherwise the abscissa of the nearest waypoint, first index on ties (the kd-tree
 * lookup, :213-216).  Upstream the scalar problem goes to CasADi's sqpmethod (:144-169); here it is a safeguarded Newton iteration on
 * its first-order condition (r(s) - p) . r'(s) = 0 -- steps bounded by two waypoint spacings, halved while the residual grows, 30 at
 * most -- which stops at a step below 1e-13 max(1, L); the answer is the root nearest the start, to the accuracy of the spline
 * evaluation (measured against an independent root finder: tests/test_gpu_track.py).  A pose's result depends on that pose, its own
 * start and the track only (no value crosses lanes), so a call is reproducible bit for bit and independent of its neighbours. */
#define LMPC_TRACK_OK 0
#define LMPC_TRACK_NOT_CONVERGED 1 /* the iteration cap was reached; the last iterate is returned                       */
#define LMPC_TRACK_BAD_INPUT 2     /* x, y or yaw not finite; s, t, xi are NaN                                           */
int lmpc_global_to_frenet_batch(lmpc_handle* h, const lmpc_spline_track* track, int32_t B, const double* pose, const double* s0,
                                const int32_t* seeded, double* frenet, int32_t* status);

/* RacingTrajectory::frenet_to_global for a batch (racing_trajectory.cpp:122-134, 194-202; frenet_to_global_function().map(N),
 * racing_mpc_node.cpp:50,460; racing_simulator_node.cpp:273-278): rows 0 - 2 (s, e_y, e_psi) of an SOA state array X [6][n][B] -- a plan
 * X_optm, or n = 1 for car states x [6][B] --  ->  pose [3][n][B] = (x, y, yaw), yaw in (-pi, pi]. */
int lmpc_frenet_to_global_batch(lmpc_handle* h, const lmpc_spline_track* track, int32_t B, int32_t n, const double* X, double* pose);

/* Batched extended Kalman filter: EKFStateEstimator (state_estimators/ekf_state_estimator, ekf_state_estimator.cpp:112-214), ONE
 * FILTER PER CAR on the device, fp64, over the handle's vehicle.  State [X, Y, yaw, vx, vy, omega]: the dynamics are the handle's
 * single-track model at curvature k = 0, where the Frenet rows (s, e_y, e_psi) are the global ones -- what the reference's rk4_
 * with {"k", 0.0} is (:47, :142).  One update, per car:
 *   dt = (timestamp_ns - last timestamp) 1e-9, one scalar per call, shared by the batch;
 *   x_p = f_d(x, u, 0, dt) (RK4, or Euler with lmpc_vehicle.integrator), F = d x_p / d x, P_p = F P F' + Q -- Q once per update,
 *   whatever dt is (:146);
 *   y = z - h(x_p, z), S = H P_p H' + R, K = P_p H' S^-1, x = x_p + K y, P = (I - K H) P_p -- the non-symmetric form as written
 *   (:190); all 36 entries of P are kept and nothing is symmetrised;
 *   x is clipped to [x_min, x_max] (:199-202), P is not touched by the clip.
 * Kept as written upstream:
 *   - a timestamp that jumps back only sets the time (initialize, :132-135): the negative dt computed before it is still used to
 *     integrate, x and P are NOT reset (:108-109 are comments), and the yaml key reset_on_timestamp_jump is read by nobody;
 *   - check_cov (:238-264) visits column 0 only (its inner loop advances i): R(i,0) < 0 becomes 0 for every row i, then R(0,0) <= 0
 *     becomes 1e-6; a negative R(1,1) is left alone.  It is applied to the kernel's copy; the caller's R is never written;
 *   - any NaN or Inf in a car's z or R gives that car the pure prediction (:158-167) -- how a per-car sensor dropout is expressed; the
 *     car's slice of K is then left as it was, and is what Kz_out reports.
 * Observations: where the reference registers arbitrary CasADi h(x, z), an observation here is an ordered list of 1 .. 6 distinct
 * state rows, registered before lmpc_ekf_initialize and addressed by the id registration returns (0, 1, ...).  h selects those rows;
 * a selected yaw (row 2) is first aligned to the measurement with lmpc::utils::align_yaw(x_p[2], z) (utils.hpp:25-31), which is what
 * h's second argument serves upstream; H is the selection matrix.  The gains of all observations sit side by side in K [6][sum nz]
 * in the order of registration (:95-98); an update overwrites the columns of its own observation only.  obs_id = -1: pure prediction.
 * Not upstream (the fleet needs them): per-car start of x and P (lmpc_ekf_set_state; NULL broadcasts the config's x0 / P0, which
 * lmpc_ekf_create also does), and the per-car flags below.
 * Store, owned by the handle, batch axis fastest: x [6][B], u [2][B] (zero at creation), P [36][B] row-major, K [6][sum nz][B].
 * lmpc_ekf_create and every lmpc_ekf_register_observation allocate (the latter synchronises the handle's stream); nothing else does.
 * Array arguments are DEVICE pointers; launches and copies go on the handle's stream; every call names the store's batch.
 * LMPC_ERR_ARGUMENT, nothing written, message in lmpc_last_error (the reference's sentence where it throws):
 *   registration after lmpc_ekf_initialize (EKFAlreadyInitializedException); nz outside 1 .. 6, a row outside 0 .. 5 or twice;
 *   lmpc_ekf_initialize with nothing registered (NoObservationRegisteredException); an update before it (EKFUninitializedException);
 *   an id that was not returned by registration (ObservationNameNotFoundException); another batch than the store's; no store.
 * WHERE IT HOLDS: the single-track model is stiff at low speed (BARC: lateral and yaw modes near -102 / vx and -216 / vx per second),
 * and RK4 leaves its stability region when 216 dt / vx > 2.78.  Below that bound -- for the BARC car: vx >= 1.5 m/s with updates of
 * 12.5 ms or less -- fp64 and extended-precision runs of the filter agree to 3e-15 over 800 updates, and that is the regime every
 * test is pinned to.  Outside it (the reference's sample start x0 ~ 1e-3, P0 = 1e3 is) the filter is sensitive to rounding and two
 * correct implementations need not agree. */
typedef struct lmpc_ekf_config {
  double x0[LMPC_NX];  /* start estimate (ekf.x0)                                  */
  double P0[36];       /* start covariance, row-major                             */
  double Q[36];        /* process noise added per update, row-major               */
  double x_min[LMPC_NX], x_max[LMPC_NX]; /* the clip; +-INFINITY allowed          */
} lmpc_ekf_config;
#define LMPC_EKF_FLAG_FALLBACK 1   /* NaN / Inf in this car's z or R: it took the pure prediction */
#define LMPC_EKF_FLAG_R_REPAIRED 2 /* check_cov changed the kernel's copy of this car's R         */
#define LMPC_EKF_FLAG_NOT_FINITE 4 /* this car's new estimate or covariance is not finite         */
int lmpc_ekf_create(lmpc_handle* h, int32_t batch, const lmpc_ekf_config* cfg); /* replaces an earlier filter; blocking (allocates) */
int lmpc_ekf_destroy(lmpc_handle* h);                                           /* waits for the handle's stream.  lmpc_destroy does it too */
int lmpc_ekf_register_observation(lmpc_handle* h, int32_t nz, const int32_t* rows /* HOST [nz] */, int32_t* obs_id);
int lmpc_ekf_initialize(lmpc_handle* h, int64_t timestamp_ns); /* host-only: the time of the last update is a host value of the handle */
int lmpc_ekf_set_state(lmpc_handle* h, int32_t batch, const double* x /* [6][B] or NULL */, const double* P /* [36][B] or NULL */);
int lmpc_ekf_update_control(lmpc_handle* h, int32_t batch, const double* u /* [2][B] */);
/* z [nz][B], R [nz][nz][B] (both ignored with obs_id = -1); x_out [6][B], P_out [36][B], Kz_out [6][nz][B] (not written with
 * obs_id = -1), flags [B]: any of the four NULL.  Two launches (one with obs_id = -1), asynchronous, no host round trip. */
int lmpc_ekf_update_batch(lmpc_handle* h, int32_t batch, int32_t obs_id, const double* z, const double* R, int64_t timestamp_ns,
                          double* x_out, double* P_out, double* Kz_out, int32_t* flags);
/* The store: x [6][B], P [36][B], K [6][sum nz][B] to DEVICE arrays (asynchronous copies); the time of the last update and
 * `initialized` to HOST values.  Any pointer NULL. */
int lmpc_ekf_get(lmpc_handle* h, int32_t batch, double* x, double* P, double* K, int64_t* timestamp_ns, int32_t* initialized);

/* Batched time-varying LQR: RacingLQR::solve (mpc/racing_lqr, racing_lqr.cpp:45-96), ONE CONTROLLER PER CAR on the device, fp64,
 * over the handle's vehicle at curvature k = 0 (dynamics_jacobian() and rk4_ are called without k: rows 0 - 2 are global X, Y, yaw,
 * as in the filter above).  Per car, with P = Qf and k = N-2 .. 0:
 *   (Ac, Bc) = df/dx, df/du of the CONTINUOUS dynamics at (X_ref[:,k], U_ref[:,k]);
 *   [A B; 0 I] = expm([Ac Bc; 0 0] dt), the exact zero-order hold (lmpc_utils/src/utils.cpp:52-65);
 *   K_k = solve(R + B'PB, B'PA), a general 2 x 2 solve;   P <- Q + A'P(A - B K_k), not symmetrised;
 * then X[:,0] = x_ic, U[:,k] = U_ref[:,k] - K_k (X[:,k] - X_ref[:,k]) (the yaw difference is not wrapped, as written) and
 * X[:,k+1] = rk4(f, X[:,k], U[:,k], dt, k = 0) -- ALWAYS RK4: the class builds its own integrator (racing_lqr.cpp:36) and does not
 * read lmpc_vehicle.integrator.  Q, R, Qf are general dense matrices, row-major; nothing makes or assumes them symmetric.  There
 * are no input or state bounds.  N is the controller's own, independent of the handle's horizon; N = 2 is the smallest problem.
 * Not upstream: the batch, K and P0 = P after the last step as outputs, and the per-car flag.
 * expm: the matrix is halved until its infinity norm is at most 1/2, a Taylor polynomial of degree 14, then squared back.  The
 * halvings are limited to 20; a stage whose norm is larger than 2^19, or not finite, is given NaN and its car ends flagged.  Every
 * loop count is a constant or N, so a NaN or huge input cannot lengthen a solve, and one car's NaN never touches another car.
 * Only lmpc_lqr_create allocates (the workspace of max_batch cars, 60 (N-1) max_batch + 76 doubles; it synchronises the handle's
 * stream).  Array arguments are DEVICE pointers, batch axis fastest; a solve is two launches on the handle's stream, no host round trip.
 * LMPC_ERR_ARGUMENT, nothing written: N < 2, dt <= 0 or not finite, max_batch < 1, batch outside 1 .. max_batch, a null required
 * pointer, a solve without a controller.
 * WHERE IT HOLDS: an LQR has no bounds, and the rollout is RK4 on the stiff single-track model: past 216 dt / vx = 2.78 (BARC) the
 * integration itself is unstable, and a reference the car cannot stay near (BARC N = 81 at dt = 0.01; IAC from 15 m/s with metre
 * offsets) makes the closed loop sensitive to rounding.  The tests are pinned to references where fp64 and extended precision agree. */
typedef struct lmpc_lqr_config {
  int32_t N;        /* knot points, >= 2 */
  int32_t reserved; /* 0 */
  double dt;
  double Q[36];     /* row-major */
  double R[4];
  double Qf[36];
} lmpc_lqr_config;
#define LMPC_LQR_FLAG_NOT_FINITE 1 /* this car's X_optm, U_optm, K or P0 holds a NaN or Inf */
int lmpc_lqr_create(lmpc_handle* h, int32_t max_batch, const lmpc_lqr_config* cfg); /* allocates the workspace; replaces an earlier one */
int lmpc_lqr_destroy(lmpc_handle* h);                                               /* waits for the handle's stream.  lmpc_destroy does it too */
int lmpc_lqr_solve_batch(lmpc_handle* h, int32_t batch, const double* x_ic /* [6][B] */, const double* X_ref /* [6][N][B] */,
                         const double* U_ref /* [2][N-1][B] */, double* X_optm /* [6][N][B] */, double* U_optm /* [2][N-1][B] */,
                         double* K /* [2][6][N-1][B] or NULL */, double* P0 /* [36][B] or NULL */, int32_t* flags /* [B] or NULL */);

/* Batched vanilla controller: VanillaController::solve (controllers/vanilla_controller, vanilla_controller.cpp:49-109) with its
 * PidController (lmpc_utils/src/pid_controller.cpp:83-127), ONE CONTROLLER PER CAR on the device, fp64, one lane per car.  Per car, on
 * the state x = (s, e_y, e_psi, vx, vy, omega):
 *   pose (x, y, yaw) = frenet_to_global(s, e_y, e_psi), the arithmetic of lmpc_frenet_to_global_batch;   v = hypot(vx, vy);
 *   la = clamp(v lookahead_speed_ratio, min_lookahead_distance, max_lookahead_distance);   s_la = align_abscissa(s + la, L/2, L);
 *   (x_la, y_la) = the centre line at s_la;   dir = atan2(y_la - y, x_la - x);   alpha = dir - yaw wrapped into (-pi, pi] as
 *   atan2(sin d, cos d) (upstream goes through tf2 quaternions, lmpc_transform_helper.cpp:63-75: the same angle);
 *   STEER = clamp(atan(2 wheel_base sin(alpha) / la), -max_steer, max_steer);
 *   PID on e = vel_ref - v with the controller's dt: a NaN e returns NaN and leaves the state; else last_error <- error, error <- e,
 *   integral <- clamp(integral + e dt, min_i, max_i), cmd = k_p e + k_i integral + k_d (error - last_error) / dt (the first call
 *   sees e / dt, as upstream), cmd <= min_cmd -> min_cmd, cmd >= max_cmd -> max_cmd;
 *   aero = 0.5 rho A cd v^2, down = aero (cl_f + cl_r), roll = fr (m 9.81 + down) (9.81: that file's own GRAVITY, not the model's
 *   9.8), F = m cmd + roll + aero;   (FD, FB) = F > 0 ? (F, 0) : (0, F);   u_out [3][B] = (FD, FB, STEER), newtons and radians.
 * Not upstream, for the fleet: the batch; the node's fold u_a = |FD| > |FB| ? FD : FB (vanilla_controller_node.cpp:118-122) and the
 * command on this library's two-control layout, u_model [2][B] = (u_a force_to_lon, STEER); vel_ref = NULL, which takes the track's
 * velocity interpolant at the car's abscissa times speed_scale (speed_scale = 1: what the node passes, :104); the per-car flag; and
 * lmpc_vanilla_rollout_batch, which runs controller and plant for `periods` control periods in one launch.
 * force_to_lon: in the model fd + fb = 1000 u_lon exactly (single_track_planar_model.cpp:215-216; the two blending weights add to
 * one), so 1e-3 hands the plant the total force the controller asked for; 1.0 is upstream's chain as written, newtons into a model
 * whose unit is kN.
 * The flag LMPC_VANILLA_FLAG_NOT_FINITE marks a car whose u_out holds a NaN or Inf; its PID state is left as it was and no other
 * car's bits change.  An abscissa beyond LMPC_VANILLA_LAPS_MAX laps is given a NaN u_out (align_abscissa has lost its digits long
 * before 1e300 and would wrap it to a finite 0).  Every loop count is a constant, n_sub or periods: no input lengthens a launch.
 * lmpc_vanilla_rollout_batch: per period the decision above at the current state, then n_sub plant sub-steps of dt_sim with the
 * arithmetic of lmpc_plant_step_batch (the |vx| < 1e-6 guard, curvature from the lmpc_track table at the current abscissa, the
 * model's integrator, the abscissa wrap).  Every output is optional: X_log [6][periods][B] the state the decision was taken at,
 * U_log [2][periods][B] the u_model applied, k_log [periods][B] the table's curvature at that state -- what
 * lmpc_fleet_ss_record_batch takes -- and the accumulators distance [B] (+= the unwrapped abscissa travelled) and worst_excess [B]
 * (max with max(e_y + b/2 - left, right - (e_y - b/2)) after the period, the bounds from the table at the abscissa of the decision),
 * as lmpc_loop_advance_batch defines them.  x [6][B] is updated in place.  A car whose decision, or whose state after the plant, is
 * not finite is flagged and frozen for the rest of the launch: that period is undone (x and the PID state stay as they were before
 * it, nothing is accumulated) and its logs are NaN from that period on.  flags is written (0 or the flag), not accumulated.
 * Only lmpc_vanilla_create allocates (3 doubles per car; it synchronises the handle's stream); every other call names the store's
 * batch.  Array arguments are DEVICE pointers, batch axis fastest; launches go on the handle's stream.
 * LMPC_ERR_ARGUMENT, nothing written, message in lmpc_last_error: no store, another batch than the store's, a null required pointer
 * or track, a track of another device, periods < 1, n_sub < 1, dt_sim or dt not positive and finite, min_lookahead_distance <= 0
 * or > max_lookahead_distance, min_i > max_i, min_cmd > max_cmd (std::clamp is undefined there), batch < 1. */
typedef struct lmpc_vanilla_config {
  double lookahead_speed_ratio, min_lookahead_distance, max_lookahead_distance;
  double k_p, k_i, k_d, min_cmd, max_cmd, min_i, max_i; /* lon_kp, lon_ki, lon_kd, lon_min_acc, lon_max_acc, lon_ki_min, lon_ki_max */
  double dt;            /* the PID's dt (vanilla_controller.dt) */
  double force_to_lon;  /* newtons -> model command; 1e-3 physical, 1.0 as written upstream */
} lmpc_vanilla_config;
#define LMPC_VANILLA_FLAG_NOT_FINITE 1 /* this car's u_out holds a NaN or Inf (rollout: or its state after the plant does) */
#define LMPC_VANILLA_LAPS_MAX 1e9      /* |s| > LMPC_VANILLA_LAPS_MAX L: u_out is NaN */
int lmpc_vanilla_create(lmpc_handle* h, int32_t batch, const lmpc_vanilla_config* cfg); /* per-car PID state, zeroed; replaces an earlier one */
int lmpc_vanilla_destroy(lmpc_handle* h);                                               /* waits for the handle's stream.  lmpc_destroy does it too */
int lmpc_vanilla_reset(lmpc_handle* h, int32_t batch, const double* integral /* [B] or NULL: 0 */); /* error and last_error <- 0; asynchronous */
int lmpc_vanilla_get(lmpc_handle* h, int32_t batch, double* integral, double* error, double* last_error); /* DEVICE [B], any NULL */
int lmpc_vanilla_solve_batch(lmpc_handle* h, int32_t batch, const lmpc_spline_track* track, const double* x_ic /* [6][B] */,
                             const double* vel_ref /* [B] or NULL */, double speed_scale, double* u_out /* [3][B] */,
                             double* u_model /* [2][B] or NULL */, int32_t* flags /* [B] or NULL */);
int lmpc_vanilla_rollout_batch(lmpc_handle* h, int32_t batch, const lmpc_spline_track* track, const lmpc_track* table, double* x /* [6][B] */,
                               int32_t periods, double dt_sim, int32_t n_sub, double speed_scale, double* X_log, double* U_log, double* k_log,
                               double* distance, double* worst_excess, int32_t* flags);

/* The rollout of a fleet: a plant per car and the fleet recorder in the period loop (behind the types its prototype names). */
#include "lmpc_hip_vanilla_fleet.h"

#ifdef __cplusplus
}
#endif
#endif /* LMPC_HIP_H_ */
