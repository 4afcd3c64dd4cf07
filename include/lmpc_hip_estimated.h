/*
 * lmpc_hip_estimated.h -- THE FUSED ESTIMATED PERIOD: everything between two solves of the closed loop in which the controller sees
 * the plant only through sensors and the batched extended Kalman filter (closed_loop.run_estimated), in one launch.  Part of the C
 * ABI of lmpc_hip.h, which includes this file behind lmpc_hip_cars_model.h (include lmpc_hip.h, not this file alone); every
 * convention of that header holds here -- return codes, device pointers, the stream rule.  The stream class of the one entry point:
 * lmpc_loop_advance_estimated_batch is asynchronous on the handle's stream; it allocates nothing and reads nothing back.
 * tests/test_stream_table_estimated.py holds one class per prototype of this file and tests/test_gpu_streams_estimated.py holds it
 * to that on a stream that is held by a timed gate.
 *
 * What it replaces: lmpc_loop_advance_batch steps the plant from the state the controller was given, so a loop whose controller is
 * given an ESTIMATE went through the unfused entry points -- two lmpc_plant_step_batch, lmpc_ekf_update_control, two
 * lmpc_ekf_update_batch, lmpc_frenet_to_global_batch, lmpc_global_to_frenet_batch, lmpc_shift_batch, lmpc_prepare_failed_batch --
 * and the element-wise operations between them.  This call keeps two states per car, the TRUTH x (Frenet frame, known to the plant
 * alone) and the filter's estimate (global frame, in the handle's EKF store), and does, per car and in this order, each step with
 * the arithmetic of the entry point it replaces:
 *   1 the input applied: U_optm[:, 0], or U_ref[:, 0] where status != 0; it goes to u_prev and to the filter's control
 *     (lmpc_ekf_update_control); n_fail += 1 on a failed solve;
 *   2 the truth advances n_sub / 2 sub-steps of dt_sim (lmpc_plant_step_batch);
 *   3 the velocity observation z = x[rows of obs_vel] + noise_vel, and the filter's update by it over
 *     dt_v = (double)(t_vel_ns - last) * 1e-9, `last` the time of the filter's last update (lmpc_ekf_update_batch's expression and clock);
 *   4 the truth advances the other n_sub / 2 sub-steps; distance accumulates the unwrapped abscissa travelled over both halves,
 *     worst_excess is taken against knot 0 of the incoming bounds (as lmpc_loop_advance_batch does);
 *   5 the pose observation: the pose of the truth (lmpc_frenet_to_global_batch), z = pose[rows of obs_pose] + noise_pose, a yaw row
 *     wrapped by atan2(sin z, cos z); the update by it over dt_p = (double)(t_pose_ns - t_vel_ns) * 1e-9; the filter's clock becomes
 *     t_pose_ns.  A NaN in a car's noise makes its z NaN and the car takes the pure prediction -- the filter's own rule for a
 *     dropped-out sensor (LMPC_EKF_FALLBACK); nothing is added to it here;
 *   6 sq_err[r][b] += (estimate - truth)^2 in the global frame, the yaw difference wrapped;
 *   7 the projection of the estimate's pose (lmpc_global_to_frenet_batch) started from the incoming x_ic[0] (a non-finite one: from
 *     the nearest waypoint); the result is x_ic rows 0 - 2 and goes to track_status; x_ic rows 3 - 5 are the filter's;
 *   8 the next references: lmpc_shift_batch from the solution where the solve succeeded; after a failed solve the in-place shift of
 *     the old plan, or with restart_failed != 0 lmpc_prepare_failed_batch AT THE NEW x_ic -- the estimate, never the truth.
 * The rollouts (plant, shift, cold restart), the filter and the body width of worst_excess use the handle's vehicle.
 *
 * obs_vel is a registered observation (lmpc_ekf_register_observation) of 1 - 3 rows within {3, 4, 5}, obs_pose one of 1 - 3 rows
 * within {0, 1, 2}; anything else is LMPC_ERR_UNSUPPORTED.  The filter must be initialised (lmpc_ekf_initialize) and its store's
 * batch is the call's.
 *
 * NOT BUILT: the estimator inside the fleet LMPC period, per-car or double-track vehicles in this call, ShardedSolver, a device-side
 * random generator (the noise arrives in arrays).
 */
#ifndef LMPC_HIP_ESTIMATED_H_
#define LMPC_HIP_ESTIMATED_H_

#ifndef LMPC_HIP_H_
#error "include lmpc_hip.h: it includes lmpc_hip_estimated.h"
#endif

/* (the spline track of lmpc_hip.h, which documents it further down; the same typedef, repeated as C11 allows) */
typedef struct lmpc_spline_track lmpc_spline_track;

/* Everything the call takes beside the handle, the batch and the two tracks.  DEVICE pointers, fp64 unless stated, the batch axis
 * fastest; N is the handle's horizon, nz_v / nz_p the row counts of obs_vel / obs_pose. */
typedef struct lmpc_estimated_loop {
  const double* X_optm;  const double* U_optm;  const int32_t* status;   /* the solve's result, SOA layout */
  double* x;             /* [6][B] the TRUTH (Frenet), advanced in place                                   */
  double* u_prev;        /* [2][B] out: the input applied (the next u_ic)                                  */
  double* x_ic;          /* [6][B] in: the state the solve was given (row 0 seeds the projection);
                                   out: the new estimate, rows 0-2 projected to the Frenet frame, rows 3-5 the filter's */
  double *X_ref, *U_ref, *T_ref, *bound_left, *bound_right, *curvatures, *vel_ref;   /* updated in place */
  double dt, dt_sim, speed_scale, speed_limit;
  int32_t n_sub, restart_failed, obs_vel, obs_pose;
  int64_t t_vel_ns, t_pose_ns;
  const double* noise_vel;   const double* R_vel;    /* [nz_v][B], [nz_v][nz_v][B] */
  const double* noise_pose;  const double* R_pose;   /* [nz_p][B], [nz_p][nz_p][B] */
  /* optional, any of them NULL */
  double* x_est;  double* z_vel;  double* z_pose;      /* [6][B] global estimate; the measurements formed */
  int32_t* ekf_flags;  int32_t* track_status;          /* [B] accumulators: |= and max                    */
  double* distance;  double* worst_excess;  int64_t* n_fail;  double* sq_err;   /* [B], [B], [B], [6][B] accumulators */
} lmpc_estimated_loop;

/* One estimated period behind a solve, steps 1 - 8 above, for `batch` cars on `track` (the tables the plant and the references
 * read) and `spline` (the interpolants the two frame changes read; of the same track).  One launch on the handle's stream;
 * asynchronous; allocates nothing, reads nothing back; the handle's EKF store and clock advance as by lmpc_ekf_update_control and
 * two lmpc_ekf_update_batch.
 * LMPC_ERR_ARGUMENT, with nothing written and the clock unmoved: no filter (lmpc_ekf_create), a filter that is not initialised, a
 * batch other than its store's; an unknown observation id; a NULL io, required pointer, track or spline (or a spline of another
 * device); dt or dt_sim not positive; n_sub odd or below 2; X_ref == X_optm or U_ref == U_optm.
 * LMPC_ERR_UNSUPPORTED, the same way: LMPC_LAYOUT_AOS on the handle; either controller-model switch on (lmpc_cars_set_controller_model,
 * lmpc_dtrack_set_controller_model: this call rolls out on the handle's vehicle); observation rows outside the two families above. */
int lmpc_loop_advance_estimated_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track,
                                      const lmpc_spline_track* spline, const lmpc_estimated_loop* io);

#endif  /* LMPC_HIP_ESTIMATED_H_ */
