// lmpc_vanilla.h -- the batched vanilla controller, one per car (csrc/lmpc_vanilla_kernel.hip; entry points lmpc_vanilla_* in
// csrc/lmpc_capi.hip).  Restates VanillaController::solve (vanilla_controller.cpp:49-109: pure pursuit for the steering, a PID on
// the speed for the longitudinal force) and PidController::update (lmpc_utils/src/pid_controller.cpp:83-127) as written; the
// formulas are at lmpc_vanilla_create in include/lmpc_hip.h.
//
// alpha, the angle from the car's yaw to the direction of the lookahead point: upstream takes it through tf2 quaternions
// (TransformHelper::calc_yaw_difference, lmpc_transform_helper.cpp:63-75: the yaw of q(dir) q(yaw)^-1); here it is
// atan2(sin d, cos d) of d = dir - yaw, the same angle in (-pi, pi].
//
// Not upstream (a fleet needs them): the batch; the node's fold of (FD, FB) into one signed force (vanilla_controller_node.cpp:118-122)
// and the command on this library's two-control layout, u_model = (u_a force_to_lon, STEER); the reference speed taken from the
// spline's velocity interpolant when the caller passes none; the per-car flag; and the rollout kernel, which runs controller and
// plant (the arithmetic of lmpc_plant_kernel) for `periods` control periods in one launch and can log what the fleet recorder takes.
//
// Handle-owned store (lmpc_vanilla_create): pid [3][B] = integral | error | last_error, zeroed.
#ifndef LMPC_VANILLA_H_
#define LMPC_VANILLA_H_

#include <hip/hip_runtime.h>

#include "lmpc_device.h"
#include "lmpc_fleet_ss.h"
#include "lmpc_track.hip.h"

#define LMPC_VANILLA_GRAVITY 9.81  // vanilla_controller.cpp:27 -- that file's own constant, not the model's 9.8

struct lmpc_vanilla_store {
  int batch = 0;  // 0: no store
  lmpc_vanilla_config cfg{};
  double* pid = nullptr;  // [3][batch]
};

struct lmpc_vanilla_rollout_io {  // the caller's arrays, batch fastest; every pointer but x may be null
  double* x;             // [6][B], in place
  double* X_log;         // [6][periods][B]
  double* U_log;         // [2][periods][B]
  double* k_log;         // [periods][B]
  double* distance;      // [B], accumulated
  double* worst_excess;  // [B], accumulated (max)
  int* flags;            // [B]
};

struct lmpc_vanilla_fleet_io {  // what lmpc_vanilla_rollout_fleet_batch adds to the rollout (include/lmpc_hip_vanilla_fleet.h)
  const double* table;   // the car table (csrc/lmpc_cars.h) or the double-track table (csrc/lmpc_dtrack.h) of B cars; null: the handle's vehicle
  double* u_prev;        // [2][B] or null: in (where arrived), the input applied before period 0; out, the last input applied
  int arrived;           // the recorder takes the input that led TO the sample (else the one applied FROM it)
  long long period0;     // sample p is stamped (double)(period0 + p) * dt
  double dt;
};

// Defined in lmpc_vanilla_kernel.hip, a translation unit of its own.  One launch each on `stream`.
__attribute__((visibility("hidden"))) hipError_t lmpc_vanilla_launch_solve(hipStream_t stream, const lmpc_vanilla_store& st, const lmpc_vehicle& veh,
                                                                           const lmpc_spline_view& track, int batch, const double* x_ic,
                                                                           const double* vel_ref, double speed_scale, double* u_out,
                                                                           double* u_model, int* flags);
__attribute__((visibility("hidden"))) hipError_t lmpc_vanilla_launch_rollout(hipStream_t stream, const lmpc_vanilla_store& st, const lmpc_vehicle& veh,
                                                                             const lmpc_spline_view& track, const lmpc_track& table, int batch,
                                                                             int periods, double dt_sim, int n_sub, double speed_scale,
                                                                             const lmpc_vanilla_rollout_io& io);
// plant: LMPC_VANILLA_PLANT_*; record: whether `fs` (car b's recorder and ring, of `batch` cars) is fed
__attribute__((visibility("hidden"))) hipError_t lmpc_vanilla_launch_fleet(hipStream_t stream, const lmpc_vanilla_store& st, const lmpc_vehicle& veh,
                                                                           const lmpc_spline_view& track, const lmpc_track& table, int batch,
                                                                           int periods, double dt_sim, int n_sub, double speed_scale,
                                                                           const lmpc_vanilla_rollout_io& io, int plant, bool record,
                                                                           const lmpc_vanilla_fleet_io& fx, const lmpc_fleet_store& fs);

#endif  // LMPC_VANILLA_H_
