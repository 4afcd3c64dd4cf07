// vanilla_controller.cpp -- see vanilla_controller.hpp.
#include "vanilla_controller.hpp"

#include <hip/hip_runtime_api.h>

#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>

namespace lmpc {
namespace mpc {
namespace vanilla_controller {

namespace {
void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
// offsets (in doubles) into the staging buffer
constexpr std::size_t OFF_X = 0, OFF_VREF = 6, OFF_UOUT = 7, OFF_UMODEL = 10, OFF_PID = 12, OFF_FLAGS = 15, TOTAL = 16;
}  // namespace

void VanillaController::check(int rc, const char* what) const {
  if (rc != LMPC_OK) throw std::runtime_error(std::string(what) + " -> " + std::to_string(rc) + ": " + lmpc_last_error(h_));
}

VanillaController::VanillaController(VanillaControllerConfig::SharedPtr controller_config, VehicleModel::SharedPtr model,
                                     RacingTrajectory::SharedPtr track, int device)
    : config_(controller_config), model_(model), track_(track) {
  if (!config_ || !model_ || !track_) throw std::invalid_argument("VanillaController: null config, model or track");
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
  lmpc_vanilla_config vc{};
  const PidCoefficients& p = config_->lon_pid_coeffs;
  vc.lookahead_speed_ratio = config_->lookahead_speed_ratio;
  vc.min_lookahead_distance = config_->min_lookahead_distance;
  vc.max_lookahead_distance = config_->max_lookahead_distance;
  vc.k_p = p.k_p, vc.k_i = p.k_i, vc.k_d = p.k_d;
  vc.min_cmd = p.min_cmd, vc.max_cmd = p.max_cmd, vc.min_i = p.min_i, vc.max_i = p.max_i;
  vc.dt = config_->dt;
  vc.force_to_lon = config_->force_to_lon;
  try {
    check(lmpc_vanilla_create(h_, 1, &vc), "lmpc_vanilla_create");
    dev_track_.reset(new DeviceRacingTrajectory(h_, *track_));
  } catch (...) {
    dev_track_.reset();
    lmpc_destroy(h_);
    h_ = nullptr;
    throw;
  }
}

VanillaController::~VanillaController() {
  dev_track_.reset();        // (waits for the handle's stream)
  if (h_) lmpc_destroy(h_);
  if (dev_) (void)hipFree(dev_);
}

const VanillaControllerConfig& VanillaController::get_config() const { return *config_; }
VehicleModel& VanillaController::get_model() { return *model_; }

void VanillaController::solve(const DMDict& in, DMDict& out, Dict& stats) {
  (void)stats;
  const DM &x_ic = in.at("x_ic"), &vel_ref = in.at("vel_ref");
  (void)in.at("u_ic");
  if (x_ic.data.size() != 6 || vel_ref.data.size() < 1) throw std::invalid_argument("VanillaController::solve: x_ic is 6 x 1 and vel_ref 1 x 1");
  if (!dev_) hip_check(hipMalloc(&dev_, TOTAL * sizeof(double)), "hipMalloc");
  double* d = static_cast<double*>(dev_);
  double host[TOTAL] = {};
  for (std::size_t r = 0; r < 6; ++r) host[OFF_X + r] = x_ic.data[r];
  host[OFF_VREF] = vel_ref.data[0];
  hip_check(hipMemcpy(d, host, OFF_UOUT * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
  check(lmpc_vanilla_solve_batch(h_, 1, dev_track_->get(), d + OFF_X, d + OFF_VREF, 1.0, d + OFF_UOUT, d + OFF_UMODEL,
                                 reinterpret_cast<int32_t*>(d + OFF_FLAGS)),
        "lmpc_vanilla_solve_batch");
  check(lmpc_synchronize(h_), "lmpc_synchronize");
  hip_check(hipMemcpy(host, d, TOTAL * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy");
  DM u_out(3, 1);
  for (std::size_t r = 0; r < 3; ++r) u_out(r, 0) = host[OFF_UOUT + r];
  u_model_ = DM(2, 1);
  for (std::size_t r = 0; r < 2; ++r) u_model_(r, 0) = host[OFF_UMODEL + r];
  int32_t fl = 0;
  std::memcpy(&fl, &host[OFF_FLAGS], sizeof(fl));
  flags_ = fl;
  out["u_out"] = u_out;
}

void VanillaController::get_pid_state(double& integral, double& error, double& last_error) {
  if (!dev_) hip_check(hipMalloc(&dev_, TOTAL * sizeof(double)), "hipMalloc");
  double* d = static_cast<double*>(dev_);
  check(lmpc_vanilla_get(h_, 1, d + OFF_PID, d + OFF_PID + 1, d + OFF_PID + 2), "lmpc_vanilla_get");
  check(lmpc_synchronize(h_), "lmpc_synchronize");
  double host[3];
  hip_check(hipMemcpy(host, d + OFF_PID, sizeof(host), hipMemcpyDeviceToHost), "hipMemcpy");
  integral = host[0], error = host[1], last_error = host[2];
}

void VanillaController::reset(double integral_error) {
  if (!dev_) hip_check(hipMalloc(&dev_, TOTAL * sizeof(double)), "hipMalloc");
  double* d = static_cast<double*>(dev_);
  hip_check(hipMemcpy(d + OFF_PID, &integral_error, sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
  check(lmpc_vanilla_reset(h_, 1, d + OFF_PID), "lmpc_vanilla_reset");
  check(lmpc_synchronize(h_), "lmpc_synchronize");
}

}  // namespace vanilla_controller
}  // namespace mpc
}  // namespace lmpc
