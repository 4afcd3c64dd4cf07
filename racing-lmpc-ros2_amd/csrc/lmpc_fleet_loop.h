// lmpc_fleet_loop.h -- what lmpc_fleet_loop_kernel (csrc/lmpc_fleet_loop_kernel.hip) takes beside the caller's lmpc_fleet_loop, the
// fleet store and the track: the handle's constants it needs, pre-digested on the host (lmpc_fleet_loop_advance_batch and
// lmpc_fleet_loop_advance_dtrack_batch in csrc/lmpc_capi.hip), passed by value.
#ifndef LMPC_FLEET_LOOP_H_
#define LMPC_FLEET_LOOP_H_

#include <hip/hip_runtime.h>

#include <type_traits>

#include "lmpc_fleet_ss.h"
#include "lmpc_hip.h"

struct lmpc_fleet_loop_consts {
  int N;                        // knot points
  double x_min[6], x_max[6];    // the handle's state box: what x_ic of a learning car is projected onto
  lmpc_vehicle veh;             // the handle's vehicle: the rollouts of the references, the body width of worst_excess
  lmpc_vehicle plant;           // the plant's vehicle: lmpc_fleet_loop.plant, or the handle's
};

// The double-track instantiation's constants: the same, and behind them the DEVICE double-track table of csrc/lmpc_dtrack.h (a
// table of the store's batch) and the optional gamma_y [B].  A type of its own, so that the two other instantiations keep the
// parameter list -- and with it the kernel arguments' offsets -- they had (`plant` is not read by this one).
struct lmpc_fleet_loop_consts_dt : lmpc_fleet_loop_consts {
  const double* table;
  double* gamma_y;              // DEVICE [B] or null
};

// The plant of step 2, the kernel's template parameter.
//   LMPC_FLEET_PLANT_HANDLE: every car's plant is consts.plant.
//   LMPC_FLEET_PLANT_CARS:   lmpc_fleet_loop.plant is the DEVICE car table of csrc/lmpc_cars.h, a table of the store's batch, and
//                            car b's plant is vehicle b (consts.plant is not read).
//   LMPC_FLEET_PLANT_DTRACK: car b's plant is the four-wheel vehicle b of consts.table, stepped as lmpc_plant_dtrack_kernel steps it
//                            (lmpc_fleet_loop.plant is null).
constexpr int LMPC_FLEET_PLANT_HANDLE = 0, LMPC_FLEET_PLANT_CARS = 1, LMPC_FLEET_PLANT_DTRACK = 2;
template <int PLANT>
using lmpc_fleet_loop_consts_of = std::conditional_t<PLANT == LMPC_FLEET_PLANT_DTRACK, lmpc_fleet_loop_consts_dt, lmpc_fleet_loop_consts>;

template <int PLANT>
__global__ void lmpc_fleet_loop_kernel(lmpc_fleet_loop_consts_of<PLANT>, lmpc_fleet_store, lmpc_track, lmpc_fleet_loop);

#endif  // LMPC_FLEET_LOOP_H_
