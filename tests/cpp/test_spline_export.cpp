// Prints RacingTrajectory::to_spline_track (what lmpc_spline_track_create takes) for tests/test_track_spline.py; plain g++, no GPU.
// usage: test_spline_export <track file>
// output: "L h_bar P n_wp", then one line each: breaks [P + 1], coef [5][P][4], wp_x, wp_y, wp_s
#include <cstdio>
#include <string>
#include <vector>

#include "racing_trajectory.hpp"

static void line(const std::vector<double>& v) {
  for (double a : v) std::printf("%.17g ", a);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const lmpc::vehicle_model::racing_trajectory::RacingTrajectory track{std::string(argv[1])};
  lmpc::vehicle_model::racing_trajectory::RacingTrajectory::SplineTrack st;
  track.to_spline_track(st);
  std::printf("%.17g %.17g %zu %zu\n", st.L, st.h_bar, st.breaks.size() - 1, st.wp_s.size());
  line(st.breaks);
  line(st.coef);
  line(st.wp_x);
  line(st.wp_y);
  line(st.wp_s);
  return 0;
}
