// racing_lqr.hpp -- C++ facade with the reference's class surface over the batched LQR of the C ABI (lmpc_lqr_*,
// include/lmpc_hip.h), for ONE car.
//
// Mirrors lmpc::mpc::racing_lqr::RacingLQR (racing_lqr.hpp): RacingLQR(config, model), get_config(), solve(in, out) with keys
// "x_ic" 6 x 1, "X_ref" 6 x N, "U_ref" 2 x (N-1) -> "u" 2 x 1, "U_optm" 2 x (N-1), "X_optm" 6 x N, and get_model().  What differs:
// `DM` is the project's dense matrix (dm.hpp), the model is the vehicle's parameter block, and the object is a batch of one on the
// device -- a fleet calls the C ABI directly with its batch.  What is kept as written upstream (curvature 0, RK4 whatever the
// vehicle's integrator, no wrapped yaw, general Q / R / Qf) is documented at lmpc_lqr_create.  No HIP type appears here.
#ifndef LMPC_HOST_RACING_LQR_HPP_
#define LMPC_HOST_RACING_LQR_HPP_

#include <cstdint>
#include <memory>

#include "dm.hpp"
#include "lmpc_hip.h"
#include "racing_mpc.hpp"

namespace lmpc {
namespace mpc {
namespace racing_lqr {

using lmpc::DM;
using lmpc::DMDict;
using lmpc::mpc::racing_mpc::VehicleModel;

// RacingLQRConfig (racing_lqr_config.hpp: N, dt, Q, R, Qf): the fields live in the C struct, matrices row-major.
struct RacingLQRConfig {
  typedef std::shared_ptr<RacingLQRConfig> SharedPtr;
  lmpc_lqr_config c{};
};

class RacingLQR {
 public:
  typedef std::shared_ptr<RacingLQR> SharedPtr;
  typedef std::unique_ptr<RacingLQR> UniquePtr;

  // Throws std::runtime_error when the library refuses the config, the vehicle or the device.
  explicit RacingLQR(RacingLQRConfig::SharedPtr mpc_config, VehicleModel::SharedPtr model, int device = 0);
  ~RacingLQR();
  RacingLQR(const RacingLQR&) = delete;
  RacingLQR& operator=(const RacingLQR&) = delete;

  const RacingLQRConfig& get_config() const;
  // A missing key throws std::out_of_range, a wrong shape std::invalid_argument.
  void solve(const DMDict& in, DMDict& out);
  VehicleModel& get_model();
  // (not upstream) "K" 2 x 6(N-1), K_k in columns 6k .. 6k+5, and "P0" 6 x 6 of the last solve; its flags: LMPC_LQR_FLAG_*
  const DM& get_latest_gains() const { return K_; }
  const DM& get_latest_cost_to_go() const { return P0_; }
  int32_t get_latest_flags() const { return flags_; }

 private:
  void check(int rc, const char* what) const;
  RacingLQRConfig::SharedPtr config_;
  VehicleModel::SharedPtr model_;
  lmpc_handle* h_ = nullptr;
  void* dev_ = nullptr;  // x_ic [6] | X_ref [6][N] | U_ref [2][N-1] | X_optm [6][N] | U_optm [2][N-1] | K [2][6][N-1] | P0 [36] | flags
  DM K_, P0_;
  int32_t flags_ = 0;
};

}  // namespace racing_lqr
}  // namespace mpc
}  // namespace lmpc
#endif
