// racing_lqr.cpp -- see racing_lqr.hpp.
#include "racing_lqr.hpp"

#include <hip/hip_runtime_api.h>

#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

namespace lmpc {
namespace mpc {
namespace racing_lqr {

namespace {
void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
}  // namespace

void RacingLQR::check(int rc, const char* what) const {
  if (rc != LMPC_OK) throw std::runtime_error(std::string(what) + " -> " + std::to_string(rc) + ": " + lmpc_last_error(h_));
}

RacingLQR::RacingLQR(RacingLQRConfig::SharedPtr mpc_config, VehicleModel::SharedPtr model, int device) : config_(mpc_config), model_(model) {
  if (!config_ || !model_) throw std::invalid_argument("RacingLQR: null config or model");
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
  const int rc2 = lmpc_lqr_create(h_, 1, &config_->c);
  if (rc2 != LMPC_OK) {
    const std::string msg = lmpc_last_error(h_);
    lmpc_destroy(h_);
    h_ = nullptr;
    throw std::runtime_error("lmpc_lqr_create -> " + std::to_string(rc2) + ": " + msg);
  }
}

RacingLQR::~RacingLQR() {
  if (h_) lmpc_destroy(h_);  // waits for the handle's stream
  if (dev_) (void)hipFree(dev_);
}

const RacingLQRConfig& RacingLQR::get_config() const { return *config_; }
VehicleModel& RacingLQR::get_model() { return *model_; }

void RacingLQR::solve(const DMDict& in, DMDict& out) {
  const DM &x_ic = in.at("x_ic"), &X_ref = in.at("X_ref"), &U_ref = in.at("U_ref");
  const std::size_t N = static_cast<std::size_t>(config_->c.N), M = N - 1;
  if (x_ic.data.size() != 6 || X_ref.rows != 6 || X_ref.cols != N || U_ref.rows != 2 || U_ref.cols != M)
    throw std::invalid_argument("RacingLQR::solve: x_ic is 6 x 1, X_ref 6 x N and U_ref 2 x (N-1)");
  // offsets (in doubles) into the staging buffer; with a batch of one the device layout [row][knot] is the row-major matrix
  const std::size_t OFF_XIC = 0, OFF_XREF = 6, OFF_UREF = OFF_XREF + 6 * N, OFF_X = OFF_UREF + 2 * M, OFF_U = OFF_X + 6 * N,
                    OFF_K = OFF_U + 2 * M, OFF_P0 = OFF_K + 12 * M, OFF_FLAGS = OFF_P0 + 36, TOTAL = OFF_FLAGS + 1;
  if (!dev_) hip_check(hipMalloc(&dev_, TOTAL * sizeof(double)), "hipMalloc");
  double* d = static_cast<double*>(dev_);
  std::vector<double> host(TOTAL, 0.0);
  for (std::size_t r = 0; r < 6; ++r) {
    host[OFF_XIC + r] = x_ic.data[r];
    for (std::size_t k = 0; k < N; ++k) host[OFF_XREF + r * N + k] = X_ref(r, k);
  }
  for (std::size_t r = 0; r < 2; ++r)
    for (std::size_t k = 0; k < M; ++k) host[OFF_UREF + r * M + k] = U_ref(r, k);
  hip_check(hipMemcpy(d, host.data(), OFF_X * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
  check(lmpc_lqr_solve_batch(h_, 1, d + OFF_XIC, d + OFF_XREF, d + OFF_UREF, d + OFF_X, d + OFF_U, d + OFF_K, d + OFF_P0,
                             reinterpret_cast<int32_t*>(d + OFF_FLAGS)),
        "lmpc_lqr_solve_batch");
  check(lmpc_synchronize(h_), "lmpc_synchronize");
  hip_check(hipMemcpy(host.data(), d, TOTAL * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy");
  DM X(6, N), U(2, M), u(2, 1);
  K_ = DM(2, 6 * M);
  P0_ = DM(6, 6);
  for (std::size_t r = 0; r < 6; ++r)
    for (std::size_t k = 0; k < N; ++k) X(r, k) = host[OFF_X + r * N + k];
  for (std::size_t r = 0; r < 2; ++r) {
    for (std::size_t k = 0; k < M; ++k) {
      U(r, k) = host[OFF_U + r * M + k];
      for (std::size_t c = 0; c < 6; ++c) K_(r, 6 * k + c) = host[OFF_K + (r * 6 + c) * M + k];
    }
    u(r, 0) = U(r, 0);
  }
  for (std::size_t i = 0; i < 6; ++i)
    for (std::size_t j = 0; j < 6; ++j) P0_(i, j) = host[OFF_P0 + i * 6 + j];
  int32_t fl = 0;
  std::memcpy(&fl, &host[OFF_FLAGS], sizeof(fl));
  flags_ = fl;
  out["u"] = u;
  out["U_optm"] = U;
  out["X_optm"] = X;
}

}  // namespace racing_lqr
}  // namespace mpc
}  // namespace lmpc
