/*
 * lmpc_hip_dtrack_model.h -- THE DOUBLE-TRACK CONTROLLER MODEL: the discrete Jacobian of the four-wheel model of lmpc_hip_dtrack.h,
 * problem b linearised on vehicle b of the handle's double-track table, and the switch that puts every fp64 and mixed batched solve
 * on it.  Part of the C ABI of lmpc_hip.h, which includes this file behind lmpc_hip_fleet_dtrack.h (include lmpc_hip.h, not this
 * file alone); every convention of that header holds here -- return codes, device pointers, the stream rule.  The stream class of
 * the three entry points: lmpc_linearize_dtrack_batch is asynchronous on the handle's stream; lmpc_dtrack_set_controller_model and
 * lmpc_dtrack_get_controller_model are HOST-ONLY, they touch a flag of the handle and nothing on the device.
 * tests/test_stream_table_dtrack_model.py holds one class per prototype of this file and tests/test_gpu_streams_dtrack_model.py
 * holds them to it on a stream that is held by a timed gate.
 *
 * What it is for: the baseline of the structural-mismatch experiment, the four-wheel car driven by a controller that knows the car.
 * The QP kernels read one linearisation record per (problem, stage) and accept dense rows in it; the plant layout
 * x = [s, e_y, e_psi, vx, vy, omega], u = [LON, STEER] is the QP's own.  A double-track discrete Jacobian in that layout, written
 * into that record, puts every fp64 and mixed solve kernel on the four-wheel model unchanged, and, the table being per car, every
 * problem on its own vehicle.
 *
 * The map that is linearised:  Phi(x, u; k, dt) = out(step_native(in(x), u, k, dt))
 *  - `in` and `out` are the conversions of lmpc_hip_dtrack.h decision 2 (v = hypot(vx, vy), beta = atan2(vy, vx) and back), the
 *    controls are mapped by decision 3;
 *  - ONE step of dt = T_ref[i][b] with u and k = curvatures[i][b] held: RK4, or Euler where vehicle b's integrator says so.  No
 *    curvature lookup, no abscissa wrap, no sub-steps: those belong to the plant;
 *  - gamma_y is solved in every evaluation of the dynamics by LMPC_DTRACK_NEWTON Newton iterations from 0, as the plant solves it; its
 *    derivative comes from the implicit-function theorem at the iterate, d gamma = -g_theta / g_gamma;
 *  - THE SPEED GUARD: where hypot(vx, vy) < 1e-6 the evaluation uses v = 1e-6, for the value and in the derivatives of `in`
 *    (d v = 0, d beta = (vx d vy - vy d vx) / 1e-12).  The outputs there are finite; they describe a car that does not yet move.
 *  Outputs: A = d Phi / d x, Bm = d Phi / d u, g = Phi(x_ref, u_ref) - A x_ref - Bm u_ref, exact derivatives of the kernel's own
 *  arithmetic (forward mode, operation by operation), not differences.
 *
 * WHAT STAYS ON THE HANDLE'S SINGLE-TRACK VEHICLE while the switch is on: the actuator and rate boxes, the state projection, the
 * shift's one-step rollout, the cold restart, the EKF, the LQR and the vanilla controller.  Their rollouts only produce reference
 * points, and any model may be linearised about a reference point.
 *
 * NOT BUILT on this model: the single-precision solve (lmpc_solve_batch_f32), the sequential-QP path
 * (lmpc_solve_full_dynamics_batch / _host), ShardedSolver, a facade class, and the error-dynamics regression (its tables hold
 * residuals against the single-track model).  lmpc_create with model_id LMPC_MODEL_DOUBLE_TRACK_PLANAR stays LMPC_ERR_UNSUPPORTED: a
 * handle is made on a single-track vehicle, and the four-wheel vehicles arrive through the table.
 */
#ifndef LMPC_HIP_DTRACK_MODEL_H_
#define LMPC_HIP_DTRACK_MODEL_H_

#ifndef LMPC_HIP_H_
#error "include lmpc_hip.h: it includes lmpc_hip_dtrack_model.h"
#endif

/* lmpc_linearize_batch on the double-track model, problem b on vehicle b of the table: X_ref [6][N][B], U_ref [2][N-1][B],
 * T_ref [N-1][B], curvatures [N][B] (the first N-1 knots are read) in, A [6][6][N-1][B], Bm [6][2][N-1][B], g [6][N-1][B] out; DEVICE
 * pointers.  One launch on the handle's stream; allocates nothing; works whether the switch below is on or off.  LMPC_ERR_ARGUMENT,
 * with nothing written: no table (lmpc_dtrack_set_vehicles), a batch other than the table's, a NULL pointer. */
int lmpc_linearize_dtrack_batch(lmpc_handle* h, int32_t batch, const double* X_ref, const double* U_ref, const double* T_ref,
                                const double* curvatures, double* A, double* Bm, double* g);

/* The switch.  While it is on, everything that goes through the batched fp64 / mixed solve -- lmpc_solve_batch, _mixed, _warm,
 * _warm_ss, _ss_idx -- linearises with the kernel above where it linearises with lmpc_linearize_kernel otherwise; everything behind
 * the linearisation is what it is without the switch, and the first number of lmpc_last_kernel_ms times the kernel above.  Such a
 * call must name the table's batch: another batch is LMPC_ERR_ARGUMENT with nothing written.  The single-problem host entries
 * (lmpc_solve_host, _warm, _warm_ss) are a batch of one and follow the same rule: they solve on vehicle 0 of a table of one vehicle
 * and are LMPC_ERR_ARGUMENT with any other table.  lmpc_solve_batch_f32, lmpc_solve_full_dynamics_batch and
 * lmpc_solve_full_dynamics_host return LMPC_ERR_UNSUPPORTED.
 * on != 0 needs a table: LMPC_ERR_ARGUMENT without one.  It is LMPC_ERR_UNSUPPORTED while lmpc_set_regression_laps / _rows or
 * lmpc_fleet_ss_set_regression / _rows is in effect, and those four, called with laps or a spec, are LMPC_ERR_UNSUPPORTED while the
 * switch is on: a handle corrects one model.  A refused call leaves switch, table and regression as they were.
 * lmpc_dtrack_set_vehicles(h, 0, NULL), which frees the table, switches the model off; replacing the table keeps it on.
 * Host-only: no device work, no stream. */
int lmpc_dtrack_set_controller_model(lmpc_handle* h, int32_t on);

/* *on = 1 while the switch is on, else 0.  LMPC_ERR_ARGUMENT for a NULL argument.  Host-only. */
int lmpc_dtrack_get_controller_model(const lmpc_handle* h, int32_t* on);

#endif  /* LMPC_HIP_DTRACK_MODEL_H_ */
