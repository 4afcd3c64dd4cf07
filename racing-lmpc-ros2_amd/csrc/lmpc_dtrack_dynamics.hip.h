// lmpc_dtrack_dynamics.hip.h -- the DOUBLE-TRACK planar model on the device, as the kernels that step it share it: car b's vehicle
// from the double-track table (csrc/lmpc_dtrack.h), the continuous dynamics with the Newton solve of the lateral load transfer, and
// one call's worth of sub-steps for one car (lmpc_plant_dtrack_kernel in lmpc_dtrack_kernel.hip; the double-track instantiations of
// lmpc_vanilla_fleet_kernel in lmpc_vanilla_kernel.hip).  Restates DoubleTrackPlanarModel::compile_dynamics
// (double_track_planar_model.cpp:163-347, use_frenet = true) with what include/lmpc_hip_dtrack.h decides where the reference leaves
// a choice open.  One text: the kernels that share it compute a step with the same operations in the same order.
#ifndef LMPC_DTRACK_DYNAMICS_HIP_H_
#define LMPC_DTRACK_DYNAMICS_HIP_H_

#include <hip/hip_runtime.h>

#include "lmpc_dtrack.h"
#include "lmpc_track.hip.h"

#define LMPC_DTRACK_GRAVITY 9.8  // double_track_planar_model.cpp: GRAVITY

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

// One call of the plant for one car, as a MACRO: one text, expanded where it is used (lmpc_loop_steps.hip.h says why the plant
// bodies of this library are macros: which products the compiler contracts inside the inlined model depends on the code around it,
// and behind a function lmpc_plant_dtrack_kernel contracted six products fewer than it had).  veh: the car's lmpc_vehicle_dt; trk: the
// lmpc_track; XIO(k): component k of the car's state in the outer layout [s, e_y, e_psi, vx, vy, omega], read once and written once;
// ul, de: expressions for the inputs (LON, STEER), evaluated once; dt_sim, nsub.  Declares in the scope it is expanded in: c, euler,
// ut, x (the native state), gamma_first (the gamma_y solved in the first evaluation of the dynamics of the last sub-step), sb, cb.
#define LMPC_DTRACK_STEP_CAR(veh, trk, XIO, ul_in, de_in, dt_sim, nsub)                                                              \
  const lmpc_vehicle& c = veh.base;                                                                                                   \
  const bool euler = c.integrator == LMPC_INTEGRATOR_EULER;                                                                           \
  dtrack_uterms ut;                                                                                                                   \
  {                                                                                                                                   \
    const double ul = ul_in;                                                                                                          \
    const double th = tanh(ul);                                                                                                       \
    const double fd = ul * (0.5 * th + 0.5) * 1000.0;  /* single_track_planar_model.cpp:215 */                                        \
    const double fb = ul * (0.5 - 0.5 * th) * 1000.0;  /* :216 (tanh(-u) = -tanh(u)) */                                               \
    const double lr = c.cg_ratio * c.l, lf = c.l - lr;                                                                                \
    ut.Fxf = 0.5 * c.kd * fd + 0.5 * c.kb * fb - 0.5 * c.fr * c.m * LMPC_DTRACK_GRAVITY * lr / c.l;                  /* :218 */       \
    ut.Fxr = 0.5 * (1 - c.kd) * fd + 0.5 * (1.0 - c.kb) * fb - 0.5 * c.fr * c.m * LMPC_DTRACK_GRAVITY * lf / c.l;  /* :221 */         \
    ut.fsum = fd + fb;                                                                                                                \
    ut.de = de_in;                                                                                                                    \
    sincos(ut.de, &ut.sd, &ut.cd);                                                                                                    \
  }                                                                                                                                   \
  /* the outer layout [s, e_y, e_psi, vx, vy, omega] to the native state, once */                                                     \
  double x[6];                                                                                                                        \
  {                                                                                                                                   \
    const double vx = XIO(3), vy = XIO(4);                                                                                            \
    x[0] = XIO(0);                                                                                                                    \
    x[1] = XIO(1);                                                                                                                    \
    x[2] = XIO(2);                                                                                                                    \
    x[3] = XIO(5);                                                                                                                    \
    x[4] = atan2(vy, vx);                                                                                                             \
    x[5] = hypot(vx, vy);                                                                                                             \
  }                                                                                                                                   \
  double gamma_first = 0.0;                                                                                                           \
  for (int j = 0; j < nsub; ++j) {                                                                                                    \
    if (x[5] < 1e-6) x[5] = 1e-6;                                                                                                     \
    const double kap = track_lookup(trk.curvature, trk.M, trk.L, x[0]);                                                               \
    /* classic RK4 with u, k held (lmpc_utils utils.cpp:88-108), the stages in one loop around one copy of the dynamics: */           \
    /* xs = x + cs kprev with cs = 0, dt/2, dt/2, dt; acc = k1 + 2 k2 + 2 k3 + k4 summed in that order */                             \
    double kprev[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, k1[6];                                 \
    _Pragma("unroll 1") for (int st = 0; st < 4; ++st) {                                                                              \
      const double cs = (st == 0) ? 0.0 : (st == 3) ? dt_sim : dt_sim / 2.0;                                                          \
      const double w = (st == 1 || st == 2) ? 2.0 : 1.0;                                                                              \
      double xs[6], gam;                                                                                                              \
      _Pragma("unroll") for (int r = 0; r < 6; ++r) xs[r] = (st == 0) ? x[r] : x[r] + cs * kprev[r];                                  \
      dtrack_f(veh, ut, xs, kap, kprev, gam);                                                                                         \
      if (st == 0) {                                                                                                                  \
        gamma_first = gam;                                                                                                            \
        _Pragma("unroll") for (int r = 0; r < 6; ++r) k1[r] = acc[r] = kprev[r];                                                      \
      } else {                                                                                                                        \
        _Pragma("unroll") for (int r = 0; r < 6; ++r) acc[r] += w * kprev[r];                                                         \
      }                                                                                                                               \
    }                                                                                                                                 \
    _Pragma("unroll") for (int r = 0; r < 6; ++r) x[r] = euler ? x[r] + dt_sim * k1[r] : x[r] + dt_sim / 6 * acc[r]; /* utils.cpp:110-123 | :88-108 */\
    /* align_abscissa(s, L / 2, L), LMPC_PLANT_SUBSTEPS' text */                                                                      \
    const double s1 = x[0], s2 = trk.L / 2.0;                                                                                         \
    const double kk = fabs(s2 - s1) + trk.L / 2.0;                                                                                    \
    const double ll = kk - fmod(kk, trk.L);                                                                                           \
    x[0] = s1 + ll * ((s2 > s1) - (s2 < s1));                                                                                         \
  }                                                                                                                                   \
  double sb, cb;                                                                                                                      \
  sincos(x[4], &sb, &cb);                                                                                                             \
  XIO(0) = x[0];                                                                                                                      \
  XIO(1) = x[1];                                                                                                                      \
  XIO(2) = x[2];                                                                                                                      \
  XIO(3) = x[5] * cb;                                                                                                                 \
  XIO(4) = x[5] * sb;                                                                                                                 \
  XIO(5) = x[3];

#endif  // LMPC_DTRACK_DYNAMICS_HIP_H_
