/*
 * lmpc_hip_fleet_dtrack.h -- THE FUSED FLEET LMPC PERIOD ON FOUR-WHEEL CARS: lmpc_fleet_loop_advance_batch with step 2's plant the
 * double-track step on vehicle b of the handle's double-track table.  Part of the C ABI of lmpc_hip.h, which includes this file
 * behind lmpc_fleet_loop and lmpc_hip_dtrack.h (include lmpc_hip.h, not this file alone); every convention of that header holds here
 * -- return codes, device pointers, the stream rule.  The one entry point is asynchronous on the handle's stream.
 * tests/test_stream_table_fleet_dtrack.py holds one class per prototype of this file and tests/test_gpu_streams_fleet_dtrack.py
 * holds the entry point to it on a stream that is held by a timed gate.
 *
 * What it is for: the structural-mismatch experiment at fleet size, device-resident from the first period to the last learning
 * lap.  The warm laps of four-wheel cars come from lmpc_vanilla_rollout_fleet_batch with LMPC_VANILLA_PLANT_DTRACK
 * (lmpc_hip_vanilla_fleet.h), the head-only call below records where they ended, and every learning period is one call of this
 * entry point between the solves: the single-track controllers learn, car by car, how their four-wheel plant differs from their model.
 *
 * Per car the call is lmpc_fleet_loop_advance_batch, step for step and bit for bit, except step 2's plant:
 *  - THE PLANT is lmpc_plant_step_dtrack_batch's step with four-wheel vehicle b of the double-track table
 *    (lmpc_dtrack_set_vehicles): the conversion to the native state on entry, then per sub-step the guard on the signed v, the
 *    curvature lookup, RK4 or Euler from the car's own integrator, LMPC_DTRACK_NEWTON Newton iterations on gamma_y in every
 *    evaluation of the dynamics with no data-dependent exit, the wrap; the conversion back on exit.  The same operations in the same
 *    order; the compiler may contract them differently than in the stand-alone kernel, so the state agrees with
 *    lmpc_plant_step_dtrack_batch's to rounding (tests/test_gpu_fleet_loop_dtrack.py: 1e-11, that entry point's own bound), not
 *    to the bit.
 *  - EVERYTHING ELSE keeps the handle's single-track vehicle: the reference rollouts of the shift, the in-place shift and the cold
 *    restart, the half width in worst_excess, the projection of x_ic, the recorder, the lap book, the phase, the query.
 *  - ONE SOURCE FOR THE PLANT, lmpc_hip_cars.h's rule: io->plant must be NULL and no car table may be set.
 *  - HEAD-ONLY (all six solution pointers NULL): there is no plant.  The call is lmpc_fleet_loop_advance_batch's head-only call,
 *    bit for bit, and gamma_y is not written.
 * lmpc_fleet_loop is unchanged, in layout and in size.  Allocates nothing and reads nothing back.
 */
#ifndef LMPC_HIP_FLEET_DTRACK_H_
#define LMPC_HIP_FLEET_DTRACK_H_

#ifndef LMPC_HIP_H_
#error "include lmpc_hip.h: it includes lmpc_hip_fleet_dtrack.h"
#endif

/* One launch on the handle's stream.  gamma_y_or_null, [B]: when not NULL it receives, for every car, the gamma_y solved in the
 * first evaluation of the dynamics of the last sub-step, in newtons, as lmpc_plant_step_dtrack_batch hands it out; x and every other
 * output are the same to the bit with or without it.  LMPC_ERR_ARGUMENT, nothing written, message in lmpc_last_error: every
 * argument case of lmpc_fleet_loop_advance_batch; no double-track table; a table whose batch is not the fleet store's; io->plant
 * not NULL; a car table (lmpc_cars_set_vehicles) set at the same time.  LMPC_ERR_UNSUPPORTED with LMPC_LAYOUT_AOS on the handle. */
int lmpc_fleet_loop_advance_dtrack_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, const lmpc_fleet_loop* io,
                                         double* gamma_y_or_null /* DEVICE [B] */);

#endif  /* LMPC_HIP_FLEET_DTRACK_H_ */
