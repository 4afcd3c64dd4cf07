// lmpc_fleet_loop.h -- what lmpc_fleet_loop_kernel (csrc/lmpc_fleet_loop_kernel.hip) takes beside the caller's lmpc_fleet_loop, the
// fleet store and the track: the handle's constants it needs, pre-digested on the host (lmpc_fleet_loop_advance_batch in
// csrc/lmpc_capi.hip), passed by value.
#ifndef LMPC_FLEET_LOOP_H_
#define LMPC_FLEET_LOOP_H_

#include <hip/hip_runtime.h>

#include "lmpc_fleet_ss.h"
#include "lmpc_hip.h"

struct lmpc_fleet_loop_consts {
  int N;                        // knot points
  double x_min[6], x_max[6];    // the handle's state box: what x_ic of a learning car is projected onto
  lmpc_vehicle veh;             // the handle's vehicle: the rollouts of the references, the body width of worst_excess
  lmpc_vehicle plant;           // the plant's vehicle: lmpc_fleet_loop.plant, or the handle's
};

// <false>: every car's plant is consts.plant.  <true>: lmpc_fleet_loop.plant is the DEVICE car table of csrc/lmpc_cars.h, a table
// of the store's batch, and car b's plant is vehicle b (consts.plant is not read).
template <bool CARS>
__global__ void lmpc_fleet_loop_kernel(lmpc_fleet_loop_consts, lmpc_fleet_store, lmpc_track, lmpc_fleet_loop);

#endif  // LMPC_FLEET_LOOP_H_
