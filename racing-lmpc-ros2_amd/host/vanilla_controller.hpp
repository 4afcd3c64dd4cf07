// vanilla_controller.hpp -- C++ facade with the reference's class surface over the batched vanilla controller of the C ABI
// (lmpc_vanilla_*, include/lmpc_hip.h), for ONE car.
//
// Mirrors lmpc::mpc::vanilla_controller::VanillaController (vanilla_controller.hpp): VanillaController(config, model, track),
// get_config(), solve(in, out, stats) with keys "x_ic" 6 x 1, "u_ic" (read for its presence, as upstream reads it and uses nothing of
// it) and "vel_ref" 1 x 1 -> "u_out" 3 x 1 = (FD, FB, STEER) in newtons and radians, and get_model().  What differs: `DM` is the
// project's dense matrix (dm.hpp), the model is the vehicle's parameter block, `stats` is a string -> double map, and the object is a
// batch of one on the device -- a fleet calls the C ABI directly with its batch.  The PID state lives on the device, one per
// object, as upstream's pid_controller_ member does.  No HIP type appears here.
#ifndef LMPC_HOST_VANILLA_CONTROLLER_HPP_
#define LMPC_HOST_VANILLA_CONTROLLER_HPP_

#include <cstdint>
#include <map>
#include <memory>
#include <string>

#include "device_track.hpp"
#include "dm.hpp"
#include "lmpc_hip.h"
#include "racing_mpc.hpp"
#include "racing_trajectory.hpp"

namespace lmpc {
namespace mpc {
namespace vanilla_controller {

using lmpc::DM;
using lmpc::DMDict;
using lmpc::mpc::racing_mpc::VehicleModel;
using lmpc::vehicle_model::racing_trajectory::DeviceRacingTrajectory;
using lmpc::vehicle_model::racing_trajectory::RacingTrajectory;

typedef std::map<std::string, double> Dict;

enum VanillaControllerStepMode { STEP, CONTINUOUS };

// utils::PidCoefficients (lmpc_utils/pid_controller.hpp)
struct PidCoefficients {
  double k_p = 0.0, k_i = 0.0, k_d = 0.0;
  double min_cmd = 0.0, max_cmd = 0.0;
  double min_i = 0.0, max_i = 0.0;
};

// VanillaControllerConfig (vanilla_controller_config.hpp), the reference's field names and defaults
struct VanillaControllerConfig {
  typedef std::shared_ptr<VanillaControllerConfig> SharedPtr;
  double lookahead_speed_ratio = 1.0;
  double min_lookahead_distance = 1.0;
  double max_lookahead_distance = 10.0;
  PidCoefficients lon_pid_coeffs;
  double dt = 0.1;
  VanillaControllerStepMode step_mode = VanillaControllerStepMode::STEP;
  // (not upstream) newtons -> this library's model command, lmpc_vanilla_config.force_to_lon: 1e-3 physical, 1.0 as written upstream
  double force_to_lon = 1e-3;
};

class VanillaController {
 public:
  typedef std::shared_ptr<VanillaController> SharedPtr;
  typedef std::unique_ptr<VanillaController> UniquePtr;

  // Throws std::runtime_error when the library refuses the config, the vehicle, the track or the device.
  explicit VanillaController(VanillaControllerConfig::SharedPtr controller_config, VehicleModel::SharedPtr model,
                             RacingTrajectory::SharedPtr track, int device = 0);
  ~VanillaController();
  VanillaController(const VanillaController&) = delete;
  VanillaController& operator=(const VanillaController&) = delete;

  const VanillaControllerConfig& get_config() const;
  // A missing key throws std::out_of_range, a wrong shape std::invalid_argument.
  void solve(const DMDict& in, DMDict& out, Dict& stats);
  VehicleModel& get_model();
  // (not upstream) the command on the two-control layout, 2 x 1 = (u_a force_to_lon, STEER), and the flags (LMPC_VANILLA_FLAG_*) of
  // the last solve; the PID state (integral, error, last_error); reset: the integral as given, error and last_error zero
  // (lmpc_vanilla_reset)
  const DM& get_latest_model_command() const { return u_model_; }
  int32_t get_latest_flags() const { return flags_; }
  void get_pid_state(double& integral, double& error, double& last_error);
  void reset(double integral_error = 0.0);

 private:
  void check(int rc, const char* what) const;
  VanillaControllerConfig::SharedPtr config_;
  VehicleModel::SharedPtr model_;
  RacingTrajectory::SharedPtr track_;
  lmpc_handle* h_ = nullptr;
  std::unique_ptr<DeviceRacingTrajectory> dev_track_;
  void* dev_ = nullptr;  // x_ic [6] | vel_ref | u_out [3] | u_model [2] | pid [3] | flags
  DM u_model_;
  int32_t flags_ = 0;
};

}  // namespace vanilla_controller
}  // namespace mpc
}  // namespace lmpc
#endif
