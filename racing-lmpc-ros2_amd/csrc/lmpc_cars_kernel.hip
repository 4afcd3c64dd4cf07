// lmpc_cars_kernel.hip -- lmpc_plant_step_cars_batch: lmpc_plant_kernel with car b stepped by vehicle b of the handle's car table
// (csrc/lmpc_cars.h), for a fleet whose cars differ in grip, mass and tyres while their controllers share one model.
//
// One lane per car, 256 to a workgroup, as lmpc_plant_kernel.  A lane loads its vehicle -- 25 coalesced loads of 8 bytes and one of
// 4 per car, once per call, into registers -- and its state, runs the plant's sub-steps and stores the state.  No LDS, no barrier,
// no cross-lane operation; no lane reads another car's data, and a lane past the batch returns before it reads anything.
// Every loop count is nsub or a constant.
#include <hip/hip_runtime.h>

#include "lmpc_cars.h"
#include "lmpc_loop_steps.hip.h"

// The plant's sub-steps, OUT OF LINE and in the form of lmpc_plant_kernel's body -- vehicle and table by value, the scratch arrays
// its own -- around the one text of lmpc_loop_steps.hip.h: fleet_loop_plant's form (lmpc_fleet_loop_kernel.hip) and vanilla_plant's
// (lmpc_vanilla_kernel.hip), so that the contraction inside the inlined model does not depend on the caller.
__device__ __noinline__ void cars_plant(lmpc_vehicle veh, lmpc_track trk, double* __restrict__ x_io, double u0, double u1, double dt_sim, int nsub) {
  double x[6], xn[6];
  const double u[2] = {u0, u1};
#pragma unroll
  for (int k = 0; k < 6; ++k) x[k] = x_io[k];
  LMPC_PLANT_SUBSTEPS(veh, trk, x, u, dt_sim, nsub, xn)
#pragma unroll
  for (int k = 0; k < 6; ++k) x_io[k] = x[k];
}

__global__ __launch_bounds__(256) void lmpc_plant_cars_kernel(const double* __restrict__ tab, int B, lmpc_track trk, double* __restrict__ x_io,
                                                              const double* __restrict__ u_in, double dt_sim, int nsub) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  lmpc_vehicle veh;
  lmpc_car_vehicle(tab, B, b, veh);
  double x[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) x[k] = x_io[(size_t)k * B + b];
  cars_plant(veh, trk, x, u_in[b], u_in[(size_t)B + b], dt_sim, nsub);
#pragma unroll
  for (int k = 0; k < 6; ++k) x_io[(size_t)k * B + b] = x[k];
}
