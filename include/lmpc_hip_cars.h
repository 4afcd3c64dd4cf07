/*
 * lmpc_hip_cars.h -- a HETEROGENEOUS FLEET: one plant vehicle per car on the device, the car table, and the plant step that reads it.
 * Part of the C ABI of lmpc_hip.h, which includes this file (include lmpc_hip.h, not this file alone); every convention of that
 * header holds here -- return codes, device pointers, the stream rule.  The stream class of the three entry points:
 * lmpc_cars_set_vehicles and lmpc_cars_get_vehicles are BLOCKING, they move HOST arrays with the synchronous hipMemcpy behind a wait
 * on the handle's stream; lmpc_plant_step_cars_batch is asynchronous.  tests/test_stream_table_cars.py holds one class per prototype
 * of this file and tests/test_gpu_streams_cars.py holds them to it on a stream that is held by a timed gate.
 *
 * What it is for: a Monte-Carlo run over model mismatch in ONE process on ONE handle -- each car's grip, mass and tyre parameters
 * drawn separately, each controller learning from its own laps (the per-car safe set and the per-car error-dynamics regression of
 * lmpc_hip.h) how ITS car differs from the nominal model.  This header is the PLANT.  The controllers share one model, the handle's
 * lmpc_vehicle, unless lmpc_cars_set_controller_model (lmpc_hip_cars_model.h) puts the batched solves on this table, problem b
 * linearised on vehicle b: the baseline of the experiment, a controller that knows its car.  Even then only the LINEARISATION is per
 * car: the actuator and rate boxes of the solve kernels, the reference rollouts (lmpc_prepare_batch, lmpc_shift_batch and their
 * fused forms) and the body width of worst_excess stay on the handle's vehicle.  So do lmpc_loop_advance_batch,
 * lmpc_vanilla_rollout_batch and the sharded solver: they step every car with one vehicle, table or no table.
 */
#ifndef LMPC_HIP_CARS_H_
#define LMPC_HIP_CARS_H_

#ifndef LMPC_HIP_H_
#error "include lmpc_hip.h: it includes lmpc_hip_cars.h"
#endif

/* The car table: veh is a HOST array of `batch` vehicles, copied to the device as a structure of arrays (each of the 25 doubles of
 * lmpc_vehicle as [batch], and the integrator as int32 [batch]: a wave's 64 cars read a field as one contiguous run).  The handle
 * holds one table; a new one replaces it, whatever its batch.  veh = NULL or batch = 0 switches the table off and frees it;
 * lmpc_destroy frees it too.  Every vehicle must have model_id LMPC_MODEL_SINGLE_TRACK_PLANAR and integrator LMPC_INTEGRATOR_RK4 or
 * LMPC_INTEGRATOR_EULER (it may differ from car to car); anything else, or batch < 0, is LMPC_ERR_ARGUMENT and the table in effect
 * before the call stays in effect, untouched.  Blocking: it synchronises the handle's stream before the older table is freed, and
 * copies with the synchronous hipMemcpy.
 * While a table is set, lmpc_fleet_loop_advance_batch steps car b's plant (its step 2) with vehicle b: the table's batch must be
 * the fleet store's and lmpc_fleet_loop.plant must be NULL -- the call has one source for its plant --, either violation is
 * LMPC_ERR_ARGUMENT before anything is written.  Everything else in that call keeps the handle's vehicle: the rollouts of the
 * references (the shift's last knot, the in-place shift, the cold restart) and the body width in worst_excess.  Without a table the
 * call is what it is without this header.  Besides it, lmpc_plant_step_cars_batch below and the fleet rollout of
 * lmpc_hip_vanilla_fleet.h with LMPC_VANILLA_PLANT_CARS, the table is read by lmpc_hip_cars_model.h: lmpc_linearize_cars_batch, and the batched solves while lmpc_cars_set_controller_model is on.
 * veh = NULL or batch = 0 switches that controller model off with the table; a replaced table keeps it.  The same call on four-wheel cars is
 * lmpc_fleet_loop_advance_dtrack_batch of lmpc_hip_fleet_dtrack.h, whose plant is the double-track table of lmpc_hip_dtrack.h: by
 * the same rule it is refused (LMPC_ERR_ARGUMENT) while a car table is set. */
int lmpc_cars_set_vehicles(lmpc_handle* h, int32_t batch, const lmpc_vehicle* veh);

/* The table read back to a HOST array of `batch` vehicles (checks, checkpoints): what lmpc_cars_set_vehicles was given, field for
 * field.  LMPC_ERR_ARGUMENT without a table, with a batch other than the table's or veh = NULL.  Blocking: it synchronises the
 * handle's stream and copies with the synchronous hipMemcpy. */
int lmpc_cars_get_vehicles(lmpc_handle* h, int32_t batch, lmpc_vehicle* veh);

/* lmpc_plant_step_batch with car b stepped by vehicle b of the table: x [6][B] advanced in place by n_sub sub-steps of dt_sim with
 * u [2][B] held, each car with its own vehicle's integrator (RK4 or Euler), the |vx| < 1e-6 guard, the curvature looked up at the
 * current abscissa, the abscissa wrapped into [0, L).  The same text as lmpc_plant_step_batch's sub-step; with every car on the
 * handle's vehicle the two agree to the last bits (tests/test_gpu_plant_cars.py).  One launch on the handle's stream; allocates
 * nothing.  LMPC_ERR_ARGUMENT, with nothing written: no table, a batch other than the table's, a NULL pointer or a bad track,
 * dt_sim not positive, n_sub < 1. */
int lmpc_plant_step_cars_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, double* x, const double* u, double dt_sim,
                               int32_t n_sub);

#endif  /* LMPC_HIP_CARS_H_ */
