// ekf_state_estimator.cpp -- see ekf_state_estimator.hpp.
#include "ekf_state_estimator.hpp"

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>

namespace lmpc {
namespace state_estimator {
namespace ekf_state_estimator {

namespace {
// offsets (in doubles) into the staging buffer
constexpr std::size_t OFF_U = 0, OFF_Z = 2, OFF_R = 8, OFF_X = 44, OFF_P = 50, OFF_KZ = 86, OFF_FLAGS = 122, OFF_K = 123;

void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
}  // namespace

void EKFStateEstimator::check(int rc, const char* what) const {
  if (rc != LMPC_OK) throw std::runtime_error(std::string(what) + " -> " + std::to_string(rc) + ": " + lmpc_last_error(h_));
}

EKFStateEstimator::EKFStateEstimator(EKFStateEstimatorConfig::SharedPtr ekf_config, VehicleModel::SharedPtr model, int device)
    : config_(ekf_config), model_(model), x_(6, 1), u_(2, 1), P_(6, 6), K_(6, 0) {
  if (!config_ || !model_) throw std::invalid_argument("EKFStateEstimator: null config or model");
  // the handle carries the vehicle; its controller part is not used (the smallest problem the library accepts)
  lmpc_config c{};
  const double inf = std::numeric_limits<double>::infinity();
  c.N = 3;
  for (int k = 0; k < 4; ++k) c.R[k] = c.R_d[k] = (k % 3 == 0) ? 1.0 : 0.0;
  for (int k = 0; k < 6; ++k) c.x_max[k] = inf, c.x_min[k] = -inf;
  for (int k = 0; k < 2; ++k) c.u_max[k] = inf, c.u_min[k] = -inf;
  c.max_vel_ref_diff = 1.0;
  const int rc = lmpc_create(&c, &model_->v, device, &h_);
  if (rc != LMPC_OK) {
    const std::string msg = h_ ? lmpc_last_error(h_) : "allocation failed";
    if (h_) lmpc_destroy(h_);
    h_ = nullptr;
    throw std::runtime_error("lmpc_create -> " + std::to_string(rc) + ": " + msg);
  }
  const int rc2 = lmpc_ekf_create(h_, 1, &config_->c);
  if (rc2 != LMPC_OK) {
    const std::string msg = lmpc_last_error(h_);
    lmpc_destroy(h_);
    h_ = nullptr;
    throw std::runtime_error("lmpc_ekf_create -> " + std::to_string(rc2) + ": " + msg);
  }
  for (int i = 0; i < 6; ++i) {
    x_(i, 0) = config_->c.x0[i];
    for (int j = 0; j < 6; ++j) P_(i, j) = config_->c.P0[i * 6 + j];
  }
}

EKFStateEstimator::~EKFStateEstimator() {
  if (h_) lmpc_destroy(h_);  // waits for the handle's stream
  if (dev_) (void)hipFree(dev_);
}

const EKFStateEstimatorConfig& EKFStateEstimator::get_config() const { return *config_; }
VehicleModel& EKFStateEstimator::get_model() { return *model_; }
const bool& EKFStateEstimator::is_initialized() const { return initialized_; }
const int64_t& EKFStateEstimator::get_latest_timestamp() const { return nanosec_; }
const DM& EKFStateEstimator::get_latest_estimate() const { return x_; }
const DM& EKFStateEstimator::get_latest_estimate_covariance() const { return P_; }
const DM& EKFStateEstimator::get_latest_kalman_gain() const { return K_; }

void EKFStateEstimator::register_observation(const std::string& name, const std::vector<int>& rows) {
  if (initialized_) throw EKFAlreadyInitializedException();
  if (obs_.count(name)) throw ObservationNameAlreadyExistsException(name);
  std::vector<int32_t> r(rows.begin(), rows.end());
  int32_t id = -1;
  if (lmpc_ekf_register_observation(h_, static_cast<int32_t>(r.size()), r.data(), &id) != LMPC_OK)
    throw std::invalid_argument(lmpc_last_error(h_));
  obs_[name] = Obs{id, static_cast<int>(r.size()), nzsum_};
  nzsum_ += static_cast<int>(r.size());
  K_ = DM(6, static_cast<std::size_t>(nzsum_));  // K_ grows by nz zero columns; nothing has been written into it yet
}

void EKFStateEstimator::initialize(const int64_t& timestamp) {
  if (obs_.empty()) throw NoObservationRegisteredException();
  check(lmpc_ekf_initialize(h_, timestamp), "lmpc_ekf_initialize");
  if (!dev_) hip_check(hipMalloc(&dev_, (OFF_K + 6 * static_cast<std::size_t>(nzsum_)) * sizeof(double)), "hipMalloc");
  initialized_ = true;
  nanosec_ = timestamp;
}

void EKFStateEstimator::update_control(const DM& u) {
  if (u.data.size() != 2) throw std::invalid_argument("update_control: u is 2 x 1");
  u_ = u;
}

void EKFStateEstimator::update_observation(const StrOpt& name, const DMDict& in, DMDict& out) {
  if (!initialized_) throw EKFUninitializedException();
  if (name.has_value() && obs_.count(name.value()) == 0) throw ObservationNameNotFoundException(name.value());
  const Obs ob = name.has_value() ? obs_.at(name.value()) : Obs{-1, 0, 0};
  const int nz = ob.nz;
  const int64_t time_ns = static_cast<int64_t>(static_cast<double>(in.at("timestamp")));
  double* d = static_cast<double*>(dev_);
  double host[OFF_K] = {0.0};
  host[OFF_U] = u_.data[0], host[OFF_U + 1] = u_.data[1];
  if (nz) {
    const DM &z = in.at("z"), &R = in.at("R");
    if (z.data.size() != static_cast<std::size_t>(nz) || R.rows != static_cast<std::size_t>(nz) || R.cols != static_cast<std::size_t>(nz))
      throw std::invalid_argument("update_observation: z is nz x 1 and R nz x nz");
    for (int a = 0; a < nz; ++a) {
      host[OFF_Z + a] = z.data[a];
      for (int c = 0; c < nz; ++c) host[OFF_R + a * nz + c] = R(a, c);
    }
  }
  hip_check(hipMemcpy(d, host, OFF_X * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
  check(lmpc_ekf_update_control(h_, 1, d + OFF_U), "lmpc_ekf_update_control");
  check(lmpc_ekf_update_batch(h_, 1, ob.id, nz ? d + OFF_Z : nullptr, nz ? d + OFF_R : nullptr, time_ns, d + OFF_X, d + OFF_P,
                              nz ? d + OFF_KZ : nullptr, reinterpret_cast<int32_t*>(d + OFF_FLAGS)),
        "lmpc_ekf_update_batch");
  check(lmpc_ekf_get(h_, 1, nullptr, nullptr, d + OFF_K, nullptr, nullptr), "lmpc_ekf_get");
  check(lmpc_synchronize(h_), "lmpc_synchronize");
  std::vector<double> back(OFF_K + 6 * static_cast<std::size_t>(nzsum_));
  hip_check(hipMemcpy(back.data(), d, back.size() * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy");
  for (int i = 0; i < 6; ++i) {
    x_(i, 0) = back[OFF_X + i];
    for (int j = 0; j < 6; ++j) P_(i, j) = back[OFF_P + i * 6 + j];
    for (int c = 0; c < nzsum_; ++c) K_(i, c) = back[OFF_K + static_cast<std::size_t>(i) * nzsum_ + c];
  }
  int32_t fl = 0;
  std::memcpy(&fl, &back[OFF_FLAGS], sizeof(fl));
  flags_ = fl;
  DM Kz(6, static_cast<std::size_t>(nz ? nz : nzsum_));
  for (int i = 0; i < 6; ++i)
    for (std::size_t c = 0; c < Kz.cols; ++c) Kz(i, c) = K_(i, (nz ? ob.koff : 0) + c);
  out["x"] = x_;
  out["P"] = P_;
  out["K"] = K_;
  out["Kz"] = Kz;
  nanosec_ = time_ns;
}

}  // namespace ekf_state_estimator
}  // namespace state_estimator
}  // namespace lmpc
