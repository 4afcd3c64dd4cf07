// lmpc_cars.h -- the car table of include/lmpc_hip_cars.h: one lmpc_vehicle per car on the device, as the kernels that step a plant
// read it (lmpc_plant_cars_kernel in csrc/lmpc_cars_kernel.hip; lmpc_fleet_loop_kernel.hip's table instantiation) and as the host
// layer packs it (lmpc_cars_set_vehicles / lmpc_cars_get_vehicles in csrc/lmpc_capi.hip).
//
// Layout: structure of arrays, ONE allocation.  The doubles of lmpc_vehicle in the order of LMPC_VEHICLE_DOUBLES below, [field][B],
// and behind them the integrator, int32 [B]:
//     tab[f * B + b]                         field f of car b
//     ((const int*)(tab + NF * B))[b]        car b's integrator
// A wave's 64 cars read each field as one contiguous run of 512 bytes (the integrators: 256), once per car per call; no LDS.  The
// model_id is not stored: the setter admits LMPC_MODEL_SINGLE_TRACK_PLANAR only.  One base pointer names the whole table, so that
// lmpc_fleet_loop_advance_batch can hand it to its kernel in the (otherwise blanked) lmpc_fleet_loop.plant and the kernel's
// arguments keep their layout.
#ifndef LMPC_CARS_H_
#define LMPC_CARS_H_

#include <hip/hip_runtime.h>

#include "lmpc_hip.h"

// every double of lmpc_vehicle, in the order of the struct
#define LMPC_VEHICLE_DOUBLES(X)                                                                                                      \
  X(m) X(Jzz) X(l) X(cg_ratio) X(h) X(b) X(fr) X(kd) X(kb) X(cd) X(Af) X(rho) X(cl_f) X(cl_r) X(mu) X(Bf) X(Cf) X(Br) X(Cr) X(Fd_max) \
  X(Fb_max) X(Td) X(Tb) X(max_steer) X(max_steer_rate)

#define LMPC_CARS_COUNT_(name) +1
constexpr int lmpc_cars_fields = 0 LMPC_VEHICLE_DOUBLES(LMPC_CARS_COUNT_);
#undef LMPC_CARS_COUNT_
static_assert(sizeof(lmpc_vehicle) == 2 * sizeof(int32_t) + lmpc_cars_fields * sizeof(double), "LMPC_VEHICLE_DOUBLES names every double of lmpc_vehicle");

// doubles in the allocation of a table of B cars (the integrators take B ints behind the fields: B / 2 doubles, rounded up)
inline size_t lmpc_cars_doubles(size_t B) { return (size_t)lmpc_cars_fields * B + (B + 1) / 2; }

// car b's vehicle from a table of B cars
__device__ __forceinline__ void lmpc_car_vehicle(const double* __restrict__ tab, int B, int b, lmpc_vehicle& v) {
  int f = 0;
#define LMPC_CARS_LOAD_(name) v.name = tab[(size_t)(f++) * B + b];
  LMPC_VEHICLE_DOUBLES(LMPC_CARS_LOAD_)
#undef LMPC_CARS_LOAD_
  v.model_id = LMPC_MODEL_SINGLE_TRACK_PLANAR;
  v.integrator = reinterpret_cast<const int*>(tab + (size_t)lmpc_cars_fields * B)[b];
}

__global__ void lmpc_plant_cars_kernel(const double* tab, int B, lmpc_track trk, double* x_io, const double* u_in, double dt_sim, int nsub);

#endif  // LMPC_CARS_H_
