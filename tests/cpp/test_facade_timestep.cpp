// RacingMPC::solve on a time step that differs from stage to stage (T_ref / T_optm_ref are vectors upstream: racing_mpc.cpp:85).
// First call: the node's first call, the reference doubles as the warm start and T_optm_ref = T_ref (the cold host entry behind it).
// Second call: the first call's plan as the warm start and ANOTHER non-uniform T_optm_ref (the warm host entry behind it).
// Both answers are held to what the C ABI's batched call returned on the same arrays, which the Python side computed and wrote.
// usage: test_facade_timestep <problem.txt>   (written by tests/test_gpu_timestep.py)
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <limits>

#include "racing_mpc.hpp"

using namespace lmpc::mpc::racing_mpc;

static DM read_dm(std::ifstream& f) {
  std::size_t r, c;
  f >> r >> c;
  DM m(r, c);
  for (auto& v : m.data) f >> v;
  return m;
}

// max scaled |got - want| over X, U and dU
static double worst(DMDict& out, const DM& Xe, const DM& Ue, const DM& dUe, std::size_t N) {
  const double sx[6] = {2000.0, 10.0, 0.1, 80.0, 2.0, 2.0}, su[2] = {10.0, 0.3};
  double e = 0;
  for (std::size_t i = 0; i < N; ++i)
    for (int k = 0; k < 6; ++k) e = std::fmax(e, std::fabs(out["X_optm"](k, i) - Xe(k, i)) / sx[k]);
  for (std::size_t i = 0; i + 1 < N; ++i)
    for (int k = 0; k < 2; ++k) {
      e = std::fmax(e, std::fabs(out["U_optm"](k, i) - Ue(k, i)) / su[k]);
      e = std::fmax(e, std::fabs(out["dU_optm"](k, i) - dUe(k, i)) / su[k]);
    }
  return e;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  int N;
  double total_length, tol;
  f >> N >> total_length >> tol;
  auto cfg = std::make_shared<RacingMPCConfig>();
  auto veh = std::make_shared<VehicleModel>();
  const double inf = std::numeric_limits<double>::infinity();
  // BARC vehicle + tracking MPC (param/barc/*.yaml, param/racing_mpc/barc_tracking_mpc.param.yaml), as tests/cpp/test_facade.cpp
  lmpc_vehicle& v = veh->v;
  v.m = 2.2187; v.Jzz = 0.02723; v.l = 0.324; v.cg_ratio = 0.5; v.h = 0.07; v.b = 0.281; v.fr = 0.012;
  v.kd = 0.0; v.kb = 0.5; v.cd = 0.0; v.Af = 1.0; v.rho = 1.2; v.cl_f = 0.0; v.cl_r = 0.0; v.mu = 0.9;
  v.Bf = 5.0; v.Cf = 2.28; v.Br = 5.0; v.Cr = 2.28; v.Fd_max = 15.0; v.Fb_max = -15.0; v.Td = 0.1; v.Tb = 0.1;
  v.max_steer = 0.314159; v.max_steer_rate = 10.0;
  lmpc_config& c = cfg->c;
  c.N = N; c.learning = 0; c.num_ss_pts = 96; c.num_ss_pts_per_lap = 32; c.max_lap_stored = 3;
  c.margin = 0.1; c.q_contour = 1.0; c.q_heading = 1.0; c.q_vel = 0.2; c.q_vy = 1e-3; c.q_vyaw = 1e-3; c.q_boundary = 20.0;
  const double R[4] = {0.01, 0, 0, 0.01};
  for (int k = 0; k < 4; ++k) { c.R[k] = R[k]; c.R_d[k] = R[k]; }
  const double xmax[6] = {inf, inf, inf, 6.0, 1.0, 3.0}, xmin[6] = {-inf, -inf, -inf, 0.1, -1.0, -3.0};
  for (int k = 0; k < 6; ++k) { c.x_max[k] = xmax[k]; c.x_min[k] = xmin[k]; c.convex_hull_slack[k] = 20.0; }
  c.u_max[0] = 0.01; c.u_max[1] = 0.33; c.u_min[0] = -0.01; c.u_min[1] = -0.33; c.max_vel_ref_diff = 1.0;

  RacingMPC mpc(cfg, veh);
  DMDict in, out, out2;
  Dict stats;
  for (const char* key : {"x_ic", "u_ic", "X_ref", "U_ref", "T_ref", "bound_left", "bound_right", "curvatures", "vel_ref"})
    in[key] = read_dm(f);
  const DM T2 = read_dm(f);
  const DM X1 = read_dm(f), U1 = read_dm(f), dU1 = read_dm(f), X2 = read_dm(f), U2 = read_dm(f), dU2 = read_dm(f);
  if (!f) { std::puts("FAIL: short problem file"); return 2; }
  in["t_ic"] = DM(0.0);
  in["total_length"] = DM(total_length);
  in["X_optm_ref"] = in["X_ref"];
  in["U_optm_ref"] = in["U_ref"];
  in["dU_optm_ref"] = DM(2, static_cast<std::size_t>(N) - 1);
  in["T_optm_ref"] = in["T_ref"];
  mpc.solve(in, out, stats);
  if (!out.count("X_optm") || stats["warm_start"] != 0.0) { std::puts("FAIL: first call"); return 1; }
  const double e1 = worst(out, X1, U1, dU1, N);
  // the second call: T_ref stays (it must NOT be read when T_optm_ref is given), T_optm_ref is the other vector
  in["X_optm_ref"] = out["X_optm"];
  in["U_optm_ref"] = out["U_optm"];
  in["dU_optm_ref"] = out["dU_optm"];
  in["T_optm_ref"] = T2;
  mpc.solve(in, out2, stats);
  if (!out2.count("X_optm") || stats["warm_start"] != 1.0) { std::puts("FAIL: second call"); return 1; }
  const double e2 = worst(out2, X2, U2, dU2, N), e12 = worst(out2, X1, U1, dU1, N);
  std::printf("first call (T_ref) %.3e  second call (another T_optm_ref, warm) %.3e  second call against the first answer %.3e\n", e1, e2, e12);
  const bool ok = e1 < tol && e2 < tol && e12 > 1e3 * tol;  // (the two time-step vectors have different optima: the file says so)
  std::puts(ok ? "PASS" : "FAIL: tolerance");
  return ok ? 0 : 1;
}
