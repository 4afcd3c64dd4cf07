// lmpc_dtrack_kernel.hip -- lmpc_plant_step_dtrack_batch: the plant step on the DOUBLE-TRACK planar model, car b stepped by vehicle
// b of the handle's double-track table (csrc/lmpc_dtrack.h).  Restates DoubleTrackPlanarModel::compile_dynamics
// (double_track_planar_model.cpp:163-347, use_frenet = true) with what include/lmpc_hip_dtrack.h decides where the reference leaves
// a choice open: the lateral load transfer by a fixed count of Newton iterations in every evaluation, the outer (vx, vy) layout,
// the two-control mapping of the single-track model, and the simulator's guard / lookup / wrap per sub-step.
//
// One lane per car, 256 to a workgroup, as lmpc_plant_cars_kernel.  A lane loads its vehicle -- 34 coalesced loads of 8 bytes and
// one of 4 per car, once per call, into registers --, its state and its inputs, runs the sub-steps in the native state
// [s, e_y, e_psi, omega, beta, v] and stores the state.  No LDS, no barrier, no cross-lane operation; no lane reads another car's
// data, and a lane past the batch returns before it reads anything.  Every loop count is nsub, LMPC_DTRACK_NEWTON or a constant: an
// Euler car runs the four stages too and keeps x + dt k1.  The continuous dynamics stand ONCE in the code, inside a stage loop that
// is not unrolled: four tyres times four transcendental chains are a lot of live state, and one copy of them is what keeps the
// kernel out of scratch (DESIGN.md section 4 has the register count).
//
// A translation unit of its own (csrc/Makefile): the kernel and its launcher, called from lmpc_capi.hip through lmpc_dtrack.h.
#include <hip/hip_runtime.h>

#include "lmpc_dtrack.h"
#include "lmpc_track.hip.h"

#define LMPC_DTRACK_GRAVITY 9.8  // double_track_planar_model.cpp: GRAVITY

namespace {

// car b's vehicle from a table of B cars
__device__ __forceinline__ void dtrack_vehicle(const double* __restrict__ tab, int B, int b, lmpc_vehicle_dt& v) {
  int f = 0;
#define LMPC_DTRACK_LOAD_(name) v.name = tab[(size_t)(f++) * B + b];
  LMPC_VEHICLE_DT_DOUBLES(LMPC_DTRACK_LOAD_)
#undef LMPC_DTRACK_LOAD_
  v.base.model_id = LMPC_MODEL_DOUBLE_TRACK_PLANAR;
  v.base.integrator = reinterpret_cast<const int*>(tab + (size_t)lmpc_dtrack_fields * B)[b];
}

// what depends on the inputs only (held over the call)
struct dtrack_uterms {
  double Fxf, Fxr;  // one front / one rear tyre's longitudinal force (:218-224; left = right)
  double fsum;      // fd + fb
  double sd, cd;    // sin / cos(delta)
  double de;        // delta
};

// sin(C atan(B a - E (B a - atan(B a)))) (:248-255), the factor of Fy that does not depend on the load
__device__ __forceinline__ double dtrack_magic(double Bp, double Cp, double Ep, double a) {
  const double Ba = Bp * a;
  return sin(Cp * atan(Ba - Ep * (Ba - atan(Ba))));
}

// x_dot = f(x, u, k) in the native state x = [s, e_y, e_psi, omega, beta, v] (f does not read s), and the gamma_y it solved
__device__ __forceinline__ void dtrack_f(const lmpc_vehicle_dt& p, const dtrack_uterms& ut, const double* x, double k, double* f,
                                         double& gamma_y) {
  const lmpc_vehicle& c = p.base;
  const double ey = x[1], phi = x[2], om = x[3], beta = x[4], v = x[5];
  const double m = c.m, l = c.l, lr = c.cg_ratio * l, lf = l - lr;
  const double vsq = v * v;
  const double ax = (ut.fsum - 0.5 * c.cd * c.Af * vsq - c.fr * m * LMPC_DTRACK_GRAVITY) / m;  // :227 (no air density, as written)
  // :230-235 -- BOTH static terms carry lr, as written
  const double Fzf = 0.5 * m * LMPC_DTRACK_GRAVITY * lr / (lf + lr) - 0.5 * c.h / (lf + lr) * m * ax + 0.25 * c.cl_f * c.rho * c.Af * vsq;
  const double Fzr = 0.5 * m * LMPC_DTRACK_GRAVITY * lr / (lf + lr) + 0.5 * c.h / (lf + lr) * m * ax + 0.25 * c.cl_r * c.rho * c.Af * vsq;
  double sb, cb;
  sincos(beta, &sb, &cb);
  // :240-245
  const double nf = lf * om + v * sb, nr = lr * om - v * sb, vc = v * cb;
  const double S_fl = dtrack_magic(c.Bf, c.Cf, p.Ef, ut.de - atan(nf / (vc - 0.5 * p.tw_f * om)));
  const double S_fr = dtrack_magic(c.Bf, c.Cf, p.Ef, ut.de - atan(nf / (vc + 0.5 * p.tw_f * om)));
  const double S_rl = dtrack_magic(c.Br, c.Cr, p.Er, atan(nr / (vc - 0.5 * p.tw_r * om)));
  const double S_rr = dtrack_magic(c.Br, c.Cr, p.Er, atan(nr / (vc + 0.5 * p.tw_r * om)));
  // the lateral load transfer (:316-322): Newton on g(gamma) = gamma - cg (Fy_rl + Fy_rr + 2 Fx_f sin(delta) + (Fy_fl + Fy_fr) cos(delta))
  // from gamma = 0, Fy_ij = mu Fz_ij (1 + e Fz_ij) S_ij with Fz_ij = Fz -/+ kappa gamma (:232-237, :248-255): a quadratic in gamma
  const double kf = p.kroll_f, kr = 1.0 - p.kroll_f;
  const double ef = p.eps_f / p.Fz0_f, er = p.eps_r / p.Fz0_r;
  const double cg = c.h / (0.5 * (p.tw_f + p.tw_r));
  double gam = 0.0, Fy_f = 0.0, Fy_r = 0.0, Fy_fd = 0.0;  // Fy_fl + Fy_fr, Fy_rl + Fy_rr, Fy_fl - Fy_fr at the current gamma
#pragma unroll 1
  for (int it = 0; it <= LMPC_DTRACK_NEWTON; ++it) {
    const double Fz_fl = Fzf - kf * gam, Fz_fr = Fzf + kf * gam, Fz_rl = Fzr - kr * gam, Fz_rr = Fzr + kr * gam;
    const double Fy_fl = c.mu * Fz_fl * (1.0 + ef * Fz_fl) * S_fl, Fy_fr = c.mu * Fz_fr * (1.0 + ef * Fz_fr) * S_fr;
    const double Fy_rl = c.mu * Fz_rl * (1.0 + er * Fz_rl) * S_rl, Fy_rr = c.mu * Fz_rr * (1.0 + er * Fz_rr) * S_rr;
    Fy_f = Fy_fl + Fy_fr;
    Fy_r = Fy_rl + Fy_rr;
    Fy_fd = Fy_fl - Fy_fr;
    if (it < LMPC_DTRACK_NEWTON) {  // (the last trip only evaluates the forces at the solved gamma: the count is a constant)
      const double g = gam - cg * (Fy_r + 2.0 * ut.Fxf * ut.sd + Fy_f * ut.cd);
      const double dF = c.mu * kf * ((1.0 + 2.0 * ef * Fz_fr) * S_fr - (1.0 + 2.0 * ef * Fz_fl) * S_fl);
      const double dR = c.mu * kr * ((1.0 + 2.0 * er * Fz_rr) * S_rr - (1.0 + 2.0 * er * Fz_rl) * S_rl);
      gam -= g / (1.0 - cg * (dR + dF * ut.cd));
    }
  }
  gamma_y = gam;
  // :258-267 with Fx_fl = Fx_fr = Fxf, Fx_rl = Fx_rr = Fxr (their differences are exact zeros)
  double sdb, cdb;
  sincos(ut.de - beta, &sdb, &cdb);
  const double drag = 0.5 * c.cd * c.rho * c.Af * vsq;
  f[5] = 1.0 / m * (2.0 * ut.Fxr * cb + 2.0 * ut.Fxf * cdb + Fy_r * sb - Fy_f * sdb - drag * cb);
  f[4] = -om + 1.0 / (m * v) * (-2.0 * ut.Fxr * sb + 2.0 * ut.Fxf * sdb + Fy_r * cb + Fy_f * cdb + drag * sb);
  f[3] = 1.0 / c.Jzz * (-Fy_r * lr + Fy_fd * ut.sd * p.tw_f / 2.0 + (Fy_f * ut.cd + 2.0 * ut.Fxf * ut.sd) * lf);
  // :270-277
  double sp, cp;
  sincos(phi + beta, &sp, &cp);
  f[0] = v * cp / (1.0 - ey * k);
  f[1] = v * sp;
  f[2] = om - k * f[0];
}

}  // namespace

__global__ __launch_bounds__(256) void lmpc_plant_dtrack_kernel(const double* __restrict__ tab, int B, lmpc_track trk, double* __restrict__ x_io,
                                                                const double* __restrict__ u_in, double dt_sim, int nsub,
                                                                double* __restrict__ gamma_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  lmpc_vehicle_dt veh;
  dtrack_vehicle(tab, B, b, veh);
  const lmpc_vehicle& c = veh.base;
  const bool euler = c.integrator == LMPC_INTEGRATOR_EULER;
  dtrack_uterms ut;
  {
    const double ul = u_in[b];
    const double th = tanh(ul);
    const double fd = ul * (0.5 * th + 0.5) * 1000.0;  // single_track_planar_model.cpp:215
    const double fb = ul * (0.5 - 0.5 * th) * 1000.0;  // :216 (tanh(-u) = -tanh(u))
    const double lr = c.cg_ratio * c.l, lf = c.l - lr;
    ut.Fxf = 0.5 * c.kd * fd + 0.5 * c.kb * fb - 0.5 * c.fr * c.m * LMPC_DTRACK_GRAVITY * lr / c.l;                  // :218
    ut.Fxr = 0.5 * (1 - c.kd) * fd + 0.5 * (1.0 - c.kb) * fb - 0.5 * c.fr * c.m * LMPC_DTRACK_GRAVITY * lf / c.l;  // :221
    ut.fsum = fd + fb;
    ut.de = u_in[(size_t)B + b];
    sincos(ut.de, &ut.sd, &ut.cd);
  }
  // the outer layout [s, e_y, e_psi, vx, vy, omega] to the native state, once
  double x[6];
  {
    const double vx = x_io[(size_t)3 * B + b], vy = x_io[(size_t)4 * B + b];
    x[0] = x_io[b];
    x[1] = x_io[(size_t)B + b];
    x[2] = x_io[(size_t)2 * B + b];
    x[3] = x_io[(size_t)5 * B + b];
    x[4] = atan2(vy, vx);
    x[5] = hypot(vx, vy);
  }
  double gamma_first = 0.0;
  for (int j = 0; j < nsub; ++j) {
    if (x[5] < 1e-6) x[5] = 1e-6;
    const double kap = track_lookup(trk.curvature, trk.M, trk.L, x[0]);
    // classic RK4 with u, k held (lmpc_utils utils.cpp:88-108), the stages in one loop around one copy of the dynamics:
    // xs = x + cs kprev with cs = 0, dt/2, dt/2, dt; acc = k1 + 2 k2 + 2 k3 + k4 summed in that order
    double kprev[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, k1[6];
#pragma unroll 1
    for (int st = 0; st < 4; ++st) {
      const double cs = (st == 0) ? 0.0 : (st == 3) ? dt_sim : dt_sim / 2.0;
      const double w = (st == 1 || st == 2) ? 2.0 : 1.0;
      double xs[6], gam;
#pragma unroll
      for (int r = 0; r < 6; ++r) xs[r] = (st == 0) ? x[r] : x[r] + cs * kprev[r];
      dtrack_f(veh, ut, xs, kap, kprev, gam);
      if (st == 0) {
        gamma_first = gam;
#pragma unroll
        for (int r = 0; r < 6; ++r) k1[r] = acc[r] = kprev[r];
      } else {
#pragma unroll
        for (int r = 0; r < 6; ++r) acc[r] += w * kprev[r];
      }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) x[r] = euler ? x[r] + dt_sim * k1[r] : x[r] + dt_sim / 6 * acc[r];  // utils.cpp:110-123 | :88-108
    // align_abscissa(s, L / 2, L), LMPC_PLANT_SUBSTEPS' text
    const double s1 = x[0], s2 = trk.L / 2.0;
    const double kk = fabs(s2 - s1) + trk.L / 2.0;
    const double ll = kk - fmod(kk, trk.L);
    x[0] = s1 + ll * ((s2 > s1) - (s2 < s1));
  }
  double sb, cb;
  sincos(x[4], &sb, &cb);
  x_io[b] = x[0];
  x_io[(size_t)B + b] = x[1];
  x_io[(size_t)2 * B + b] = x[2];
  x_io[(size_t)3 * B + b] = x[5] * cb;
  x_io[(size_t)4 * B + b] = x[5] * sb;
  x_io[(size_t)5 * B + b] = x[3];
  if (gamma_out) gamma_out[b] = gamma_first;
}

hipError_t lmpc_dtrack_launch_step(hipStream_t stream, const double* tab, int B, const lmpc_track& trk, double* x, const double* u,
                                   double dt_sim, int n_sub, double* gamma_y) {
  hipLaunchKernelGGL(lmpc_plant_dtrack_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, tab, B, trk, x, u, dt_sim, n_sub, gamma_y);
  return hipGetLastError();
}
