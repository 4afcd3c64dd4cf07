/*
 * lmpc_hip_cars_model.h -- THE PER-CAR SINGLE-TRACK CONTROLLER MODEL: the discrete Jacobian of the single-track planar model, problem b
 * linearised on vehicle b of the handle's car table (lmpc_hip_cars.h), and the switch that puts every batched solve on it.  Part of
 * the C ABI of lmpc_hip.h, which includes this file behind lmpc_hip_dtrack_model.h (include lmpc_hip.h, not this file alone); every
 * convention of that header holds here -- return codes, device pointers, the stream rule.  The stream class of the three entry
 * points: lmpc_linearize_cars_batch is asynchronous on the handle's stream; lmpc_cars_set_controller_model and
 * lmpc_cars_get_controller_model are HOST-ONLY, they touch a flag of the handle and nothing on the device.
 * tests/test_stream_table_cars_model.py holds one class per prototype of this file and tests/test_gpu_streams_cars_model.py holds
 * them to it on a stream that is held by a timed gate.
 *
 * What it is for: the baseline of the parametric-mismatch experiment, every car of the heterogeneous fleet driven by a controller
 * that knows its car.  Against it a Monte-Carlo run over model mismatch can tell what the safe set and the regression recovered from
 * what a controller on the right vehicle would have had anyway.  The QP kernels read one linearisation record per (problem, stage)
 * and accept any dense stage model in it, so a Jacobian on car b's own vehicle, written into that record, puts every solve kernel on
 * that vehicle unchanged.
 *
 * The map that is linearised is lmpc_linearize_batch's, from the same model text: ONE step of dt = T_ref[i][b] of the single-track
 * planar model with u and k = curvatures[i][b] held, RK4, or Euler where vehicle b's integrator says so (it may differ from car to
 * car).  Outputs: A = d Phi / d x, Bm = d Phi / d u, g = Phi(x_ref, u_ref) - A x_ref - Bm u_ref.  The fields of the table that the
 * dynamics read are m, Jzz, l, cg_ratio, h, fr, kd, kb, cd, Af, rho, cl_f, cl_r, mu, Bf, Cf, Br, Cr and the integrator.
 *
 * WHAT STAYS ON THE HANDLE'S VEHICLE while the switch is on:
 *  - the actuator and rate boxes of the solve kernels: the table's Fd_max, Fb_max, Td, Tb, max_steer and max_steer_rate are ignored
 *    by this feature, and so is its b;
 *  - the reference rollouts: lmpc_prepare_batch, the shift's one-step rollout and the cold restart, alone and in their fused forms
 *    (they only produce reference points, and any model may be linearised about a reference point);
 *  - the body width of worst_excess;
 *  - the EKF, the LQR and the vanilla controller.
 * lmpc_fleet_loop_advance_batch keeps reading the table for its plant, as lmpc_hip_cars.h states it.
 *
 * NOT BUILT on this model: the sequential-QP path (lmpc_solve_full_dynamics_batch / _host: its line search evaluates the defects on
 * the handle's vehicle), ShardedSolver, a facade class, and the error-dynamics regressions (their tables hold residuals against the
 * handle's vehicle).
 */
#ifndef LMPC_HIP_CARS_MODEL_H_
#define LMPC_HIP_CARS_MODEL_H_

#ifndef LMPC_HIP_H_
#error "include lmpc_hip.h: it includes lmpc_hip_cars_model.h"
#endif

/* lmpc_linearize_batch with problem b on vehicle b of the car table: X_ref [6][N][B], U_ref [2][N-1][B], T_ref [N-1][B],
 * curvatures [N][B] (the first N-1 knots are read) in, A [6][6][N-1][B], Bm [6][2][N-1][B], g [6][N-1][B] out; fp64 DEVICE pointers.
 * One launch on the handle's stream; allocates nothing; works whether the switch below is on or off.  With every car of the table on
 * the handle's vehicle it writes what lmpc_linearize_batch writes.  LMPC_ERR_ARGUMENT, with nothing written: no table
 * (lmpc_cars_set_vehicles), a batch other than the table's, a NULL pointer. */
int lmpc_linearize_cars_batch(lmpc_handle* h, int32_t batch, const double* X_ref, const double* U_ref, const double* T_ref,
                              const double* curvatures, double* A, double* Bm, double* g);

/* The switch.  While it is on, everything that goes through a batched solve -- lmpc_solve_batch, _mixed, _warm, _warm_ss, _ss_idx,
 * and lmpc_solve_batch_f32 through the single-precision instantiation of the kernel above (fp64 arithmetic, float arrays) --
 * linearises with the kernel above where it linearises with lmpc_linearize_kernel otherwise; everything behind the linearisation is
 * what it is without the switch, and the first number of lmpc_last_kernel_ms times the kernel above.  Such a call must name the
 * table's batch: another batch is LMPC_ERR_ARGUMENT with nothing written.  The single-problem host entries (lmpc_solve_host, _warm,
 * _warm_ss) are a batch of one and follow the same rule: they solve on vehicle 0 of a table of one vehicle and are LMPC_ERR_ARGUMENT
 * with any other table.  lmpc_solve_full_dynamics_batch and lmpc_solve_full_dynamics_host return LMPC_ERR_UNSUPPORTED.
 * on != 0 needs a table: LMPC_ERR_ARGUMENT without one.  It is LMPC_ERR_UNSUPPORTED while lmpc_set_regression_laps / _rows or
 * lmpc_fleet_ss_set_regression / _rows is in effect, and those four, called with laps or a spec, are LMPC_ERR_UNSUPPORTED while the
 * switch is on: a handle corrects one model.  It is LMPC_ERR_UNSUPPORTED while lmpc_dtrack_set_controller_model
 * (lmpc_hip_dtrack_model.h) is on, and that switch is LMPC_ERR_UNSUPPORTED while this one is on: of the two, the one turned on second
 * is refused.  A refused call leaves switches, tables and regression as they were.
 * lmpc_cars_set_vehicles(h, 0, NULL), which frees the table, switches the model off; replacing the table keeps it on.
 * Host-only: no device work, no stream. */
int lmpc_cars_set_controller_model(lmpc_handle* h, int32_t on);

/* *on = 1 while the switch is on, else 0.  LMPC_ERR_ARGUMENT for a NULL argument.  Host-only. */
int lmpc_cars_get_controller_model(const lmpc_handle* h, int32_t* on);

#endif  /* LMPC_HIP_CARS_MODEL_H_ */
