/*
 * lmpc_hip_vanilla_fleet.h -- THE VANILLA ROLLOUT OF A FLEET: lmpc_vanilla_rollout_batch with a plant per car and the fleet safe
 * set's recorder inside the period loop, one launch for many control periods.  Part of the C ABI of lmpc_hip.h, which includes this
 * file behind the lmpc_vanilla_* prototypes (include lmpc_hip.h, not this file alone); every convention of that header holds here
 * -- return codes, device pointers, the stream rule.  The one entry point is asynchronous on the handle's stream.
 * tests/test_stream_table_vanilla_fleet.py holds one class per prototype of this file and tests/test_gpu_streams_vanilla_fleet.py
 * holds the entry point to it on a stream that is held by a timed gate.
 *
 * What it is for: the first laps of a fleet LMPC experiment, driven on the plant each car will learn on.  Pure pursuit + PID needs
 * no QP; a fleet whose cars have vehicles of their own (lmpc_hip_cars.h) or four wheels (lmpc_hip_dtrack.h) gets its warm laps in
 * ceil(periods / chunk) launches, recorded per car as lmpc_fleet_loop_advance_batch records, and goes straight to the learning
 * controller.
 *
 * Per car and period the call is lmpc_vanilla_rollout_batch except where stated:
 *  - THE DECISION reads the HANDLE's vehicle and the vanilla store (lmpc_vanilla_create), whatever the plant: the controllers of a
 *    handle share one model, and lmpc_vanilla_solve_batch followed by a plant step stays the unfused composition of a period.
 *    The half width in worst_excess is the handle's vehicle's too.
 *  - THE PLANT.  LMPC_VANILLA_PLANT_HANDLE: lmpc_vanilla_rollout_batch's, bit for bit.  _CARS: the same arithmetic with vehicle b
 *    of the car table, the car's integrator honoured (lmpc_plant_step_cars_batch's step).  _DTRACK: lmpc_plant_step_dtrack_batch's
 *    step with four-wheel vehicle b of the double-track table -- the conversion on entry and exit of each period, the guard, the
 *    lookup, the Newton iterations on gamma_y, the wrap.
 *  - THE RECORDER.  A live period is one with a finite decision and a finite state after the plant.  With record other than
 *    LMPC_VANILLA_RECORD_NONE every live period p hands one sample to car b's recorder of the fleet store (lmpc_fleet_ss_create;
 *    SafeSetRecorder::step as lmpc_fleet_ss_record_batch runs it): the state x_p the decision was taken at, an input, the table's
 *    curvature at x_p[0] (k_log's value), the time stamp (double)(period0 + p) * dt, the table's L.  The input is, with _APPLIED, the
 *    one applied FROM x_p (U_log's value: closed_loop.run_vanilla's convention), with _ARRIVED the one that led TO x_p (the
 *    previous period's, and for p = 0 the caller's u_prev: RacingMPC::solve's (x_ic, u_ic), lmpc_fleet_loop_advance_batch's
 *    convention).  A car is not recorded from the period that freezes it on.  The final state, x after the last period, is not
 *    recorded: the next launch, or the head-only call of the LMPC loop, records it.  A recording call notes the table's L for the
 *    fleet query, as lmpc_fleet_ss_record_batch does.
 *  - CHUNKS.  Two launches of 32 periods, the second with period0 advanced by 32, leave the bits of one launch of 64 in every
 *    output, in u_prev and in the fleet store.
 * Every loop count is a constant, n_sub or periods; no lane reads another car's data; no LDS, no cross-lane operation.  Allocates
 * nothing and reads nothing back.
 */
#ifndef LMPC_HIP_VANILLA_FLEET_H_
#define LMPC_HIP_VANILLA_FLEET_H_

#ifndef LMPC_HIP_H_
#error "include lmpc_hip.h: it includes lmpc_hip_vanilla_fleet.h"
#endif

#define LMPC_VANILLA_PLANT_HANDLE 0  /* the handle's vehicle: lmpc_vanilla_rollout_batch's plant */
#define LMPC_VANILLA_PLANT_CARS   1  /* car b stepped by vehicle b of the car table (lmpc_cars_set_vehicles) */
#define LMPC_VANILLA_PLANT_DTRACK 2  /* car b stepped by four-wheel vehicle b of the double-track table */
#define LMPC_VANILLA_RECORD_NONE    0
#define LMPC_VANILLA_RECORD_APPLIED 1 /* sample p = (x_p, the input applied FROM x_p): run_vanilla's convention */
#define LMPC_VANILLA_RECORD_ARRIVED 2 /* sample p = (x_p, the input that led TO x_p): RacingMPC::solve's (x_ic, u_ic),
                                         what lmpc_fleet_loop_advance_batch records */
typedef struct lmpc_vanilla_fleet_rollout {
  double* x;             /* [6][B] in place */
  double* u_prev;        /* [2][B] in/out: in, the input applied before period 0 (read for ARRIVED only); out, the last input
                            applied (unchanged for a car frozen in period 0).  Required for ARRIVED, else optional */
  int32_t periods, n_sub, plant, record;
  double dt_sim, speed_scale;
  int64_t period0;       /* the time stamp of sample p is (double)(period0 + p) * dt: one multiplication */
  double dt;             /* read only when record != NONE */
  double *X_log, *U_log, *k_log, *distance, *worst_excess;   /* as lmpc_vanilla_rollout_batch, all optional */
  int32_t* flags;        /* [B] optional */
} lmpc_vanilla_fleet_rollout; /* sizeof == 112 */

/* One launch on the handle's stream.  LMPC_ERR_ARGUMENT, nothing written, message in lmpc_last_error: every argument case of
 * lmpc_vanilla_rollout_batch (no vanilla store, another batch than the store's, a null or foreign track, a null or empty table,
 * periods < 1, n_sub < 1, dt_sim not positive and finite); a NULL io or io->x; a plant or record value not listed above; _CARS or
 * _DTRACK without that table or with a table of another batch; record other than _NONE without a fleet store, with a store of
 * another batch, or with dt not positive and finite; period0 < 0; _ARRIVED with u_prev NULL. */
int lmpc_vanilla_rollout_fleet_batch(lmpc_handle* h, int32_t batch, const lmpc_spline_track* track, const lmpc_track* table,
                                     const lmpc_vanilla_fleet_rollout* io);

#endif  /* LMPC_HIP_VANILLA_FLEET_H_ */
