// lmpc_dtrack_kernel.hip -- lmpc_plant_step_dtrack_batch: the plant step on the DOUBLE-TRACK planar model, car b stepped by vehicle
// b of the handle's double-track table (csrc/lmpc_dtrack.h).  Restates DoubleTrackPlanarModel::compile_dynamics
// (double_track_planar_model.cpp:163-347, use_frenet = true) with what include/lmpc_hip_dtrack.h decides where the reference leaves
// a choice open: the lateral load transfer by a fixed count of Newton iterations in every evaluation, the outer (vx, vy) layout,
// the two-control mapping of the single-track model, and the simulator's guard / lookup / wrap per sub-step.  The device dynamics
// and one car's step are csrc/lmpc_dtrack_dynamics.hip.h, shared with the fleet rollout of lmpc_vanilla_kernel.hip.
//
// One lane per car, 256 to a workgroup, as lmpc_plant_cars_kernel.  A lane loads its vehicle -- 34 coalesced loads of 8 bytes and
// one of 4 per car, once per call, into registers --, its state and its inputs, runs the sub-steps in the native state
// [s, e_y, e_psi, omega, beta, v] and stores the state.  No LDS, no barrier, no cross-lane operation; no lane reads another car's
// data, and a lane past the batch returns before it reads anything.  Every loop count is nsub, LMPC_DTRACK_NEWTON or a constant: an
// Euler car runs the four stages too and keeps x + dt k1.  The continuous dynamics stand ONCE in the code, inside a stage loop that
// is not unrolled: four tyres times four transcendental chains are a lot of live state, and one copy of them is what keeps the
// kernel out of scratch (DESIGN.md section 4 has the register count).
//
// A translation unit of its own (csrc/Makefile): the kernel and its launcher, called from lmpc_capi.hip through lmpc_dtrack.h.
#include <hip/hip_runtime.h>

#include "lmpc_dtrack.h"
#include "lmpc_dtrack_dynamics.hip.h"
#include "lmpc_track.hip.h"

__global__ __launch_bounds__(256) void lmpc_plant_dtrack_kernel(const double* __restrict__ tab, int B, lmpc_track trk, double* __restrict__ x_io,
                                                                const double* __restrict__ u_in, double dt_sim, int nsub,
                                                                double* __restrict__ gamma_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  lmpc_vehicle_dt veh;
  dtrack_vehicle(tab, B, b, veh);
#define LMPC_DTRACK_XIO_(k) x_io[(size_t)(k) * B + b]
  LMPC_DTRACK_STEP_CAR(veh, trk, LMPC_DTRACK_XIO_, u_in[b], u_in[(size_t)B + b], dt_sim, nsub)
#undef LMPC_DTRACK_XIO_
  if (gamma_out) gamma_out[b] = gamma_first;
}

hipError_t lmpc_dtrack_launch_step(hipStream_t stream, const double* tab, int B, const lmpc_track& trk, double* x, const double* u,
                                   double dt_sim, int n_sub, double* gamma_y) {
  hipLaunchKernelGGL(lmpc_plant_dtrack_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, tab, B, trk, x, u, dt_sim, n_sub, gamma_y);
  return hipGetLastError();
}
