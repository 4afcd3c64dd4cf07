// ekf_state_estimator.hpp -- C++ facade with the reference's class surface over the batched filter of the C ABI (lmpc_ekf_*,
// include/lmpc_hip.h), for ONE car.
//
// Mirrors lmpc::state_estimator::ekf_state_estimator::EKFStateEstimator (ekf_state_estimator.hpp:103-204): register_observation,
// initialize, update_observation(optional name, in, out) with keys "z", "R", "timestamp" -> "x", "P", "K", "Kz", update_control, the
// getters and the five exception types with their sentences.  What differs: an observation is registered by the state rows it
// selects (the library has no CasADi h; a yaw row is aligned to its measurement), `DM` is the project's dense matrix (dm.hpp), and
// the object is a batch of one on the device -- a fleet calls the C ABI directly with its batch.  Everything kept as written
// upstream (the backward timestamp, check_cov's column 0, the NaN / Inf fallback, the clip) is documented at lmpc_ekf_create.
// No HIP type appears here; the implementation stages its few dozen doubles through one device buffer.
#ifndef LMPC_HOST_EKF_STATE_ESTIMATOR_HPP_
#define LMPC_HOST_EKF_STATE_ESTIMATOR_HPP_

#include <cstdint>
#include <exception>
#include <map>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "dm.hpp"
#include "lmpc_hip.h"
#include "racing_mpc.hpp"

namespace lmpc {
namespace state_estimator {
namespace ekf_state_estimator {

using lmpc::DM;
using lmpc::DMDict;
using lmpc::mpc::racing_mpc::VehicleModel;

// EKFStateEstimatorConfig (ekf_state_estimator_config.hpp): the numeric fields live in the C struct.
struct EKFStateEstimatorConfig {
  typedef std::shared_ptr<EKFStateEstimatorConfig> SharedPtr;
  lmpc_ekf_config c{};
};

class EKFUninitializedException : public std::exception {
 public:
  const char* what() const noexcept override { return "Call EKFStateEstimator::initialize() before making any observation updates."; }
};

class EKFAlreadyInitializedException : public std::exception {
 public:
  const char* what() const noexcept override { return "Changes to observations are not allowed after the filter is initialized."; }
};

class NoObservationRegisteredException : public std::exception {
 public:
  const char* what() const noexcept override { return "No observation has been registered for the filter."; }
};

class ObservationNameAlreadyExistsException : public std::exception {
 public:
  explicit ObservationNameAlreadyExistsException(const std::string& name)
      : msg_("The observation name \"" + name + "\" has already been registered.") {}
  const char* what() const noexcept override { return msg_.c_str(); }

 protected:
  std::string msg_;
};

class ObservationNameNotFoundException : public std::exception {
 public:
  explicit ObservationNameNotFoundException(const std::string& name) : msg_("The observation name \"" + name + "\" is not found.") {}
  const char* what() const noexcept override { return msg_.c_str(); }

 protected:
  std::string msg_;
};

class EKFStateEstimator {
 public:
  typedef std::shared_ptr<EKFStateEstimator> SharedPtr;
  typedef std::unique_ptr<EKFStateEstimator> UniquePtr;
  typedef std::optional<std::string> StrOpt;

  // Throws std::runtime_error when the library refuses the vehicle or the device.
  explicit EKFStateEstimator(EKFStateEstimatorConfig::SharedPtr ekf_config, VehicleModel::SharedPtr model, int device = 0);
  ~EKFStateEstimator();
  EKFStateEstimator(const EKFStateEstimator&) = delete;
  EKFStateEstimator& operator=(const EKFStateEstimator&) = delete;

  const EKFStateEstimatorConfig& get_config() const;
  VehicleModel& get_model();
  const bool& is_initialized() const;

  // rows: the 1 .. 6 distinct state rows (0 .. 5) the observation selects, in the order of z (std::invalid_argument otherwise).
  // Throws EKFAlreadyInitializedException / ObservationNameAlreadyExistsException as upstream.
  void register_observation(const std::string& name, const std::vector<int>& rows);
  // Throws NoObservationRegisteredException.  A second call only sets the time: x and P are not reset (as upstream).
  void initialize(const int64_t& timestamp);
  // in: "z" nz x 1, "R" nz x nz, "timestamp" (ns); no name: pure prediction ("z", "R" not read).  out: "x" 6 x 1, "P" 6 x 6, "K" the
  // gain of all observations 6 x sum nz, "Kz" this observation's columns (all of K without a name, as upstream's empty Slice).
  // Throws EKFUninitializedException / ObservationNameNotFoundException; a missing key throws std::out_of_range.
  void update_observation(const StrOpt& name, const DMDict& in, DMDict& out);
  void update_control(const DM& u);

  const int64_t& get_latest_timestamp() const;
  const DM& get_latest_estimate() const;
  const DM& get_latest_estimate_covariance() const;
  const DM& get_latest_kalman_gain() const;
  // (not upstream) the per-car flags of the last update: LMPC_EKF_FLAG_*
  int32_t get_latest_flags() const { return flags_; }

 private:
  void check(int rc, const char* what) const;
  struct Obs {
    int id, nz, koff;
  };
  EKFStateEstimatorConfig::SharedPtr config_;
  VehicleModel::SharedPtr model_;
  lmpc_handle* h_ = nullptr;
  void* dev_ = nullptr;  // u [2] | z [6] | R [36] | x [6] | P [36] | Kz [36] | flags | K [6][sum nz], allocated by initialize
  bool initialized_ = false;
  std::map<std::string, Obs> obs_;
  int nzsum_ = 0;
  DM x_, u_, P_, K_;
  int64_t nanosec_ = 0;
  int32_t flags_ = 0;
};

}  // namespace ekf_state_estimator
}  // namespace state_estimator
}  // namespace lmpc
#endif
