/*
 * lmpc_hip_dtrack.h -- a DOUBLE-TRACK PLANT: one four-wheel vehicle per car on the device, the double-track table, and the plant
 * step that reads it.  Part of the C ABI of lmpc_hip.h, which includes this file (include lmpc_hip.h, not this file alone); every
 * convention of that header holds here -- return codes, device pointers, the stream rule.  The stream class of the three entry
 * points: lmpc_dtrack_set_vehicles and lmpc_dtrack_get_vehicles are BLOCKING, they move HOST arrays with the synchronous hipMemcpy
 * behind a wait on the handle's stream; lmpc_plant_step_dtrack_batch is asynchronous.  tests/test_stream_table_dtrack.py holds one
 * class per prototype of this file and tests/test_gpu_streams_dtrack.py holds them to it on a stream that is held by a timed gate.
 *
 * What it is for: model mismatch that is STRUCTURAL, not parametric.  The car table of lmpc_hip_cars.h steps every car with the
 * controllers' own single-track equations and other numbers; this plant is DoubleTrackPlanarModel::compile_dynamics
 * (double_track_planar_model.cpp:163-347): four tyres, a lateral load transfer gamma_y that feeds back into the tyre forces, and
 * the tyre curve's falloff (pacejka_e) and load-sensitivity (pacejka_eps / pacejka_fz0) terms.  This header is the PLANT; a handle's
 * controllers are single-track unless lmpc_dtrack_set_controller_model (lmpc_hip_dtrack_model.h) puts the batched fp64 / mixed
 * solves on the four-wheel model of this table, problem b on vehicle b.  lmpc_create with model_id LMPC_MODEL_DOUBLE_TRACK_PLANAR
 * stays LMPC_ERR_UNSUPPORTED, and no entry point of lmpc_hip.h itself reads the table while that switch is off:
 * lmpc_fleet_loop_advance_batch, lmpc_loop_advance_batch, lmpc_vanilla_rollout_batch and the sharded solver are what they are
 * without this header, table or no table.  Entry points with headers of their own do read it: the vanilla rollout of a fleet with
 * LMPC_VANILLA_PLANT_DTRACK (lmpc_hip_vanilla_fleet.h), the fused fleet LMPC period on four-wheel cars,
 * lmpc_fleet_loop_advance_dtrack_batch (lmpc_hip_fleet_dtrack.h), and the linearisation of the controller model,
 * lmpc_linearize_dtrack_batch (lmpc_hip_dtrack_model.h).
 *
 * The model, as the reference writes it (quirks included): GRAVITY 9.8; BOTH Fz_f and Fz_r carry lr in their static term
 * (:230,234); ax carries no air density and v_dot does (:227,260); the slip-angle denominators are v cos(beta) -/+ 0.5 tw omega
 * (:240-245); Fy_ij = mu Fz_ij (1 + eps Fz_ij / Fz0) sin(C atan(B a - E (B a - atan(B a)))) (:248-255); v_dot, beta_dot, omega_dot
 * at :258-267; Frenet form s_dot = v cos(phi + beta) / (1 - e_y k), e_y_dot = v sin(phi + beta), phi_dot = omega - k s_dot
 * (:270-277).  Native state [s, e_y, e_psi, omega, beta, v].  The NLP rows of add_nlp_constraints (friction circle, power,
 * (fd fb)^2) are constraints of a controller, not plant dynamics, and are not here.
 *
 * Four things the reference leaves open, decided here:
 *  1. THE LATERAL LOAD TRANSFER gamma_y.  The reference means the root of
 *       g(gamma) = gamma - h / (0.5 (tw_f + tw_r)) (Fy_rl + Fy_rr + (Fx_fl + Fx_fr) sin(delta) + (Fy_fl + Fy_fr) cos(delta)) = 0
 *     (:316-322); its own rootfinder call cannot be constructed (free symbols remain in g).  Built here: the root, solved afresh
 *     in EVERY evaluation of the continuous dynamics (four per RK4 step), by Newton from gamma = 0 with the analytic derivative --
 *     g is a quadratic in gamma, the sin(...) factors do not depend on it -- and LMPC_DTRACK_NEWTON iterations, always: no
 *     data-dependent exit.
 *  2. THE OUTER LAYOUT is the project's plant layout, x [6][B] = [s, e_y, e_psi, vx, vy, omega] and u [2][B] = [LON, STEER].
 *     Converted once on entry, v = hypot(vx, vy), beta = atan2(vy, vx); all n_sub sub-steps run in the native state; converted back
 *     once on exit, vx = v cos(beta), vy = v sin(beta).
 *  3. THE CONTROLS.  The reference's double track takes (fd, fb, delta); so that both plants answer the same controller output, the
 *     two-control layout is mapped as the single-track dynamics map it (single_track_planar_model.cpp:215-216):
 *     fd = u_L (0.5 tanh(u_L) + 0.5) 1000, fb = u_L (0.5 tanh(-u_L) + 0.5) 1000, delta = u[1].
 *  4. GUARD, CURVATURE, WRAP, per sub-step and in this order: if v < 1e-6 then v = 1e-6; the curvature looked up at the current
 *     abscissa; the integrator step (RK4 or Euler per car, from the vehicle's integrator); the abscissa wrapped into [0, L) --
 *     lookup and wrap are lmpc_plant_step_batch's.  The guard reads the SIGNED native v.  Only a car at the guard can take v
 *     below zero (rolling resistance with no drive, within one sub-step); the exit conversion hands it out as (|v|, beta + pi),
 *     the same motion, so a following CALL sees a slow car rolling backwards and leaves it, where a following sub-step of the
 *     same call lifts v to 1e-6.  For every other car n_sub sub-steps in one call and in n_sub calls differ by the rounding of
 *     the conversion alone.
 */
#ifndef LMPC_HIP_DTRACK_H_
#define LMPC_HIP_DTRACK_H_

#ifndef LMPC_HIP_H_
#error "include lmpc_hip.h: it includes lmpc_hip_dtrack.h"
#endif

#define LMPC_DTRACK_NEWTON 5 /* Newton iterations on gamma_y per evaluation of the dynamics */

typedef struct lmpc_vehicle_dt {
  lmpc_vehicle base;       /* model_id must be LMPC_MODEL_DOUBLE_TRACK_PLANAR; mu is double_track_planar.mu;
                              integrator RK4 | EULER; the actuator-limit fields are carried, not read */
  double tw_f, tw_r;       /* chassis.tw_f / tw_r */
  double kroll_f;          /* double_track_planar.kroll_f */
  double Ef, Fz0_f, eps_f; /* front_tyre.pacejka_e / pacejka_fz0 / pacejka_eps */
  double Er, Fz0_r, eps_r; /* rear_tyre.* */
} lmpc_vehicle_dt;         /* sizeof == 8 + 34 * 8 */

/* The double-track table: veh is a HOST array of `batch` vehicles, copied to the device as a structure of arrays (each of the 34
 * doubles of lmpc_vehicle_dt as [batch], and the integrator as int32 [batch]: a wave's 64 cars read a field as one contiguous
 * run).  The handle holds one table, independent of the car table of lmpc_hip_cars.h; a new one replaces it, whatever its batch.
 * veh = NULL or batch = 0 switches the table off and frees it (and with it the controller model of lmpc_hip_dtrack_model.h, which a
 * replaced table keeps); lmpc_destroy frees it too.  Every vehicle must have model_id
 * LMPC_MODEL_DOUBLE_TRACK_PLANAR, integrator LMPC_INTEGRATOR_RK4 or LMPC_INTEGRATOR_EULER (it may differ from car to car),
 * tw_f + tw_r > 0 and Fz0_f, Fz0_r other than 0; anything else, or batch < 0, is LMPC_ERR_ARGUMENT and the table in effect before
 * the call stays in effect, untouched.  Blocking: it synchronises the handle's stream before the older table is freed, and copies
 * with the synchronous hipMemcpy. */
int lmpc_dtrack_set_vehicles(lmpc_handle* h, int32_t batch, const lmpc_vehicle_dt* veh);

/* The table read back to a HOST array of `batch` vehicles (checks, checkpoints): what lmpc_dtrack_set_vehicles was given, field
 * for field.  LMPC_ERR_ARGUMENT without a table, with a batch other than the table's or veh = NULL.  Blocking: it synchronises the
 * handle's stream and copies with the synchronous hipMemcpy. */
int lmpc_dtrack_get_vehicles(lmpc_handle* h, int32_t batch, lmpc_vehicle_dt* veh);

/* The plant step on the double-track model, car b stepped by vehicle b of the table: x [6][B] advanced in place by n_sub sub-steps
 * of dt_sim with u [2][B] held, as decided above.  gamma_y_or_null, [B]: when not NULL it receives the gamma_y solved in the first
 * evaluation of the dynamics of the last sub-step, in newtons -- a diagnostic, and the direct handle on the Newton solve; x is the
 * same to the bit with or without it.  One launch on the handle's stream; allocates nothing.  LMPC_ERR_ARGUMENT, with nothing
 * written: no table, a batch other than the table's, a NULL x, u or track, a bad track, dt_sim not positive, n_sub < 1. */
int lmpc_plant_step_dtrack_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, double* x, const double* u, double dt_sim,
                                 int32_t n_sub, double* gamma_y_or_null);

#endif  /* LMPC_HIP_DTRACK_H_ */
