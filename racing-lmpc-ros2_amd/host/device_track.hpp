// device_track.hpp -- RacingTrajectory's conversions for a batch, on the device: a small owner of an lmpc_spline_track
// (include/lmpc_hip.h) made from a host RacingTrajectory, with the batch methods of the C ABI.  Where the reference converts one
// pose per call (RacingTrajectory::global_to_frenet / frenet_to_global, racing_trajectory.cpp:194-236), a fleet converts all of its
// cars with one launch.  Array arguments are DEVICE pointers in the batch-fastest layout of lmpc_hip.h; launches go on the
// handle's stream; the methods throw std::runtime_error with the handle's message on failure.
#ifndef LMPC_HOST_DEVICE_TRACK_HPP_
#define LMPC_HOST_DEVICE_TRACK_HPP_

#include <cstdint>

#include "lmpc_hip.h"
#include "racing_trajectory.hpp"

namespace lmpc {
namespace vehicle_model {
namespace racing_trajectory {

class DeviceRacingTrajectory {
 public:
  // fits nothing: exports the host track's splines (RacingTrajectory::to_spline_track) and uploads them once
  DeviceRacingTrajectory(lmpc_handle* handle, const RacingTrajectory& track);
  ~DeviceRacingTrajectory();
  DeviceRacingTrajectory(const DeviceRacingTrajectory&) = delete;
  DeviceRacingTrajectory& operator=(const DeviceRacingTrajectory&) = delete;

  // pose [3][B] = (x, y, yaw) -> frenet [3][B] = (s, t, xi), status [B] (LMPC_TRACK_*); s0 / seeded may be null (lmpc_global_to_frenet_batch)
  void global_to_frenet_batch(int32_t B, const double* pose, const double* s0, const int32_t* seeded, double* frenet, int32_t* status) const;
  // rows 0 - 2 of X [6][n][B] -> pose [3][n][B]
  void frenet_to_global_batch(int32_t B, int32_t n, const double* X, double* pose) const;
  // s [n] -> out [7][n] = x, y, yaw, curvature, left, right, vel
  void sample_batch(int32_t n, const double* s, double* out) const;
  // the four tables of an lmpc_track with M samples (device arrays [M])
  void tabulate(int32_t M, double* curvature, double* bound_left, double* bound_right, double* vel) const;

  const double& total_length() const { return total_length_; }
  const lmpc_spline_track* get() const { return track_; }

 private:
  void check(int rc, const char* what) const;
  lmpc_handle* h_;
  lmpc_spline_track* track_ = nullptr;
  double total_length_ = 0.0;
};

}  // namespace racing_trajectory
}  // namespace vehicle_model
}  // namespace lmpc
#endif
