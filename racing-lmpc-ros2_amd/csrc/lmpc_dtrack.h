// lmpc_dtrack.h -- the double-track table of include/lmpc_hip_dtrack.h: one lmpc_vehicle_dt per car on the device, as
// lmpc_plant_dtrack_kernel reads it (csrc/lmpc_dtrack_kernel.hip) and as the host layer packs it (lmpc_dtrack_set_vehicles /
// lmpc_dtrack_get_vehicles in csrc/lmpc_capi.hip, through lmpc_dtrack_pack / lmpc_dtrack_unpack below).
//
// Layout: structure of arrays, ONE allocation, csrc/lmpc_cars.h's.  The doubles of lmpc_vehicle_dt in the order of
// LMPC_VEHICLE_DT_DOUBLES below, [field][B], and behind them the integrator, int32 [B]:
//     tab[f * B + b]                         field f of car b
//     ((const int*)(tab + NF * B))[b]        car b's integrator
// A wave's 64 cars read each field as one contiguous run of 512 bytes (the integrators: 256), once per car per call; no LDS.  The
// model_id is not stored: the setter admits LMPC_MODEL_DOUBLE_TRACK_PLANAR only.
#ifndef LMPC_DTRACK_H_
#define LMPC_DTRACK_H_

#include <hip/hip_runtime.h>

#include "lmpc_hip.h"

// every double of lmpc_vehicle_dt, in the order of the struct
#define LMPC_VEHICLE_DT_DOUBLES(X)                                                                                                  \
  X(base.m) X(base.Jzz) X(base.l) X(base.cg_ratio) X(base.h) X(base.b) X(base.fr) X(base.kd) X(base.kb) X(base.cd) X(base.Af)         \
  X(base.rho) X(base.cl_f) X(base.cl_r) X(base.mu) X(base.Bf) X(base.Cf) X(base.Br) X(base.Cr) X(base.Fd_max) X(base.Fb_max)         \
  X(base.Td) X(base.Tb) X(base.max_steer) X(base.max_steer_rate) X(tw_f) X(tw_r) X(kroll_f) X(Ef) X(Fz0_f) X(eps_f) X(Er) X(Fz0_r)   \
  X(eps_r)

#define LMPC_DTRACK_COUNT_(name) +1
constexpr int lmpc_dtrack_fields = 0 LMPC_VEHICLE_DT_DOUBLES(LMPC_DTRACK_COUNT_);
#undef LMPC_DTRACK_COUNT_
static_assert(sizeof(lmpc_vehicle_dt) == 2 * sizeof(int32_t) + lmpc_dtrack_fields * sizeof(double) && lmpc_dtrack_fields == 34,
              "LMPC_VEHICLE_DT_DOUBLES names every double of lmpc_vehicle_dt");

// doubles in the allocation of a table of B cars (the integrators take B ints behind the fields: B / 2 doubles, rounded up)
inline size_t lmpc_dtrack_doubles(size_t B) { return (size_t)lmpc_dtrack_fields * B + (B + 1) / 2; }

// B vehicles into a host image of the table, host [lmpc_dtrack_doubles(B)] (any padding int is zeroed), and back
inline void lmpc_dtrack_pack(const lmpc_vehicle_dt* veh, size_t B, double* host) {
  int* const integ = reinterpret_cast<int*>(host + (size_t)lmpc_dtrack_fields * B);
  if (B & 1) host[lmpc_dtrack_doubles(B) - 1] = 0.0;
  for (size_t b = 0; b < B; ++b) {
    size_t f = 0;
#define LMPC_DTRACK_PACK_(name) host[(f++) * B + b] = veh[b].name;
    LMPC_VEHICLE_DT_DOUBLES(LMPC_DTRACK_PACK_)
#undef LMPC_DTRACK_PACK_
    integ[b] = veh[b].base.integrator;
  }
}

inline void lmpc_dtrack_unpack(const double* host, size_t B, lmpc_vehicle_dt* veh) {
  const int* const integ = reinterpret_cast<const int*>(host + (size_t)lmpc_dtrack_fields * B);
  for (size_t b = 0; b < B; ++b) {
    size_t f = 0;
#define LMPC_DTRACK_UNPACK_(name) veh[b].name = host[(f++) * B + b];
    LMPC_VEHICLE_DT_DOUBLES(LMPC_DTRACK_UNPACK_)
#undef LMPC_DTRACK_UNPACK_
    veh[b].base.model_id = LMPC_MODEL_DOUBLE_TRACK_PLANAR;
    veh[b].base.integrator = integ[b];
  }
}

// Defined in lmpc_dtrack_kernel.hip, a translation unit of its own (adding it leaves the device code of the other units as it
// was).  One launch on `stream`: tab is a table of B cars, x [6][B] in place, u [2][B], gamma_y [B] or null.
__attribute__((visibility("hidden"))) hipError_t lmpc_dtrack_launch_step(hipStream_t stream, const double* tab, int B, const lmpc_track& trk,
                                                                         double* x, const double* u, double dt_sim, int n_sub,
                                                                         double* gamma_y);

#endif  // LMPC_DTRACK_H_
