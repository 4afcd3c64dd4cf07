// device_track.cpp -- see device_track.hpp.
#include "device_track.hpp"

#include <stdexcept>
#include <string>

namespace lmpc {
namespace vehicle_model {
namespace racing_trajectory {

void DeviceRacingTrajectory::check(int rc, const char* what) const {
  if (rc != LMPC_OK) throw std::runtime_error(std::string(what) + " -> " + std::to_string(rc) + ": " + lmpc_last_error(h_));
}

DeviceRacingTrajectory::DeviceRacingTrajectory(lmpc_handle* handle, const RacingTrajectory& track) : h_(handle) {
  if (!h_) throw std::invalid_argument("DeviceRacingTrajectory: null handle");
  RacingTrajectory::SplineTrack st;
  track.to_spline_track(st);
  total_length_ = st.L;
  check(lmpc_spline_track_create(h_, st.L, static_cast<int32_t>(st.breaks.size() - 1), st.breaks.data(), st.coef.data(),
                                 static_cast<int32_t>(st.wp_s.size()), st.wp_x.data(), st.wp_y.data(), st.wp_s.data(), &track_),
        "lmpc_spline_track_create");
}

DeviceRacingTrajectory::~DeviceRacingTrajectory() { (void)lmpc_spline_track_destroy(h_, track_); }

void DeviceRacingTrajectory::global_to_frenet_batch(int32_t B, const double* pose, const double* s0, const int32_t* seeded, double* frenet,
                                                    int32_t* status) const {
  check(lmpc_global_to_frenet_batch(h_, track_, B, pose, s0, seeded, frenet, status), "lmpc_global_to_frenet_batch");
}

void DeviceRacingTrajectory::frenet_to_global_batch(int32_t B, int32_t n, const double* X, double* pose) const {
  check(lmpc_frenet_to_global_batch(h_, track_, B, n, X, pose), "lmpc_frenet_to_global_batch");
}

void DeviceRacingTrajectory::sample_batch(int32_t n, const double* s, double* out) const {
  check(lmpc_track_sample_batch(h_, track_, n, s, out), "lmpc_track_sample_batch");
}

void DeviceRacingTrajectory::tabulate(int32_t M, double* curvature, double* bound_left, double* bound_right, double* vel) const {
  check(lmpc_spline_track_tabulate(h_, track_, M, curvature, bound_left, bound_right, vel), "lmpc_spline_track_tabulate");
}

}  // namespace racing_trajectory
}  // namespace vehicle_model
}  // namespace lmpc
