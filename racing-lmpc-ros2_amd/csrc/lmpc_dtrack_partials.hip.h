// lmpc_dtrack_partials.hip.h -- the DOUBLE-TRACK planar model with its first derivatives, for lmpc_linearize_dtrack_kernel
// (csrc/lmpc_dtrack_model_kernel.hip).  The continuous dynamics are those of csrc/lmpc_dtrack_dynamics.hip.h, restated here on a
// value-and-tangents number (dtm_dual<K>) so that the plant and rollout kernels that expand that header keep their instructions.
// Every derivative is the exact derivative of the arithmetic written here, carried forward operation by operation; nothing is a
// difference.
//
// What is differentiated, and with respect to what.  f does not read s; rows 0..2 (the Frenet kinematics) read e_y, e_psi, beta, v,
// and row 2 omega, and their partials are five closed-form numbers (dtm_kin).  Rows 3..5 -- omega_dot, beta_dot, v_dot: the FORCE
// BLOCK, four tyres and the lateral load transfer -- read theta = (omega, beta, v, u_L, delta); dtm_force carries K of those five
// tangents at a time, theta[first .. first + K).
//
// The lateral load transfer gamma_y is solved as dtrack_f solves it, LMPC_DTRACK_NEWTON Newton iterations from 0 on values alone;
// its tangent comes from the implicit-function theorem AT THE ITERATE, d gamma = -g_theta / g_gamma, with g_theta the tangent of g
// at gamma held and g_gamma the derivative the Newton step forms.
#ifndef LMPC_DTRACK_PARTIALS_HIP_H_
#define LMPC_DTRACK_PARTIALS_HIP_H_

#include <hip/hip_runtime.h>

#include "lmpc_dtrack.h"
#include "lmpc_dtrack_dynamics.hip.h"  // LMPC_DTRACK_GRAVITY, dtrack_vehicle, dtrack_magic (none of its text changes)

// a value and K tangents
template <int K>
struct dtm_dual {
  double v, d[K];
};

#define DTM_EACH _Pragma("unroll") for (int j = 0; j < K; ++j)
#define DTM_FN template <int K> __device__ __forceinline__ dtm_dual<K>
#define DTM_D const dtm_dual<K>&

DTM_FN dtm_const(double v) {
  dtm_dual<K> r;
  r.v = v;
  DTM_EACH r.d[j] = 0.0;
  return r;
}
// theta[slot] as a variable, where the tangents carried are theta[first .. first + K)
DTM_FN dtm_var(double v, int slot, int first) {
  dtm_dual<K> r;
  r.v = v;
  DTM_EACH r.d[j] = (first + j == slot) ? 1.0 : 0.0;
  return r;
}
// phi(a) with the value and the derivative of phi at a.v given
DTM_FN dtm_chain(DTM_D a, double val, double der) {
  dtm_dual<K> r;
  r.v = val;
  DTM_EACH r.d[j] = der * a.d[j];
  return r;
}
DTM_FN operator+(DTM_D a, DTM_D b) {
  dtm_dual<K> r;
  r.v = a.v + b.v;
  DTM_EACH r.d[j] = a.d[j] + b.d[j];
  return r;
}
DTM_FN operator-(DTM_D a, DTM_D b) {
  dtm_dual<K> r;
  r.v = a.v - b.v;
  DTM_EACH r.d[j] = a.d[j] - b.d[j];
  return r;
}
DTM_FN operator-(DTM_D a) {
  dtm_dual<K> r;
  r.v = -a.v;
  DTM_EACH r.d[j] = -a.d[j];
  return r;
}
DTM_FN operator+(DTM_D a, double b) {
  dtm_dual<K> r = a;
  r.v = a.v + b;
  return r;
}
DTM_FN operator+(double b, DTM_D a) { return a + b; }
DTM_FN operator-(DTM_D a, double b) {
  dtm_dual<K> r = a;
  r.v = a.v - b;
  return r;
}
DTM_FN operator-(double b, DTM_D a) {
  dtm_dual<K> r;
  r.v = b - a.v;
  DTM_EACH r.d[j] = -a.d[j];
  return r;
}
DTM_FN operator*(DTM_D a, DTM_D b) {
  dtm_dual<K> r;
  r.v = a.v * b.v;
  DTM_EACH r.d[j] = a.d[j] * b.v + a.v * b.d[j];
  return r;
}
DTM_FN operator*(double b, DTM_D a) {
  dtm_dual<K> r;
  r.v = b * a.v;
  DTM_EACH r.d[j] = b * a.d[j];
  return r;
}
DTM_FN operator*(DTM_D a, double b) { return b * a; }
DTM_FN operator/(DTM_D a, DTM_D b) {
  dtm_dual<K> r;
  const double q = a.v / b.v;
  r.v = q;
  DTM_EACH r.d[j] = (a.d[j] - q * b.d[j]) / b.v;
  return r;
}
DTM_FN operator/(DTM_D a, double b) {
  dtm_dual<K> r;
  r.v = a.v / b;
  DTM_EACH r.d[j] = a.d[j] / b;
  return r;
}
DTM_FN dtm_atan(DTM_D a) { return dtm_chain(a, atan(a.v), 1.0 / (1.0 + a.v * a.v)); }
template <int K>
__device__ __forceinline__ void dtm_sincos(DTM_D a, dtm_dual<K>& s, dtm_dual<K>& c) {
  double sv, cv;
  sincos(a.v, &sv, &cv);
  s = dtm_chain(a, sv, cv);
  c = dtm_chain(a, cv, -sv);
}
// dtrack_magic, sin(C atan(B a - E (B a - atan(B a)))), with its derivative in a
DTM_FN dtm_magic(double Bp, double Cp, double Ep, DTM_D a) {
  const double Ba = Bp * a.v;
  const double inner = Ba - Ep * (Ba - atan(Ba));
  const double dinner = Bp - Ep * (Bp - Bp / (1.0 + Ba * Ba));
  double sv, cv;
  sincos(Cp * atan(inner), &sv, &cv);
  return dtm_chain(a, sv, cv * Cp / (1.0 + inner * inner) * dinner);
}

// what depends on the inputs only, with the derivatives in u_L (the forces) and the steering angle's sine and cosine (held over the
// four stages); lmpc_hip_dtrack.h decision 3 maps the two controls
struct dtm_uterms {
  double Fxf, Fxr, fsum;     // dtrack_uterms' three
  double dFxf, dFxr, dfsum;  // d / d u_L
  double sd, cd, de;
};

__device__ __forceinline__ void dtm_u_terms(const lmpc_vehicle& c, double ul, double de, dtm_uterms& ut) {
  const double th = tanh(ul), sech2 = 1.0 - th * th;
  const double fd = ul * (0.5 * th + 0.5) * 1000.0;  // single_track_planar_model.cpp:215
  const double fb = ul * (0.5 - 0.5 * th) * 1000.0;  // :216
  const double dfd = ((0.5 * th + 0.5) + ul * 0.5 * sech2) * 1000.0;
  const double dfb = ((0.5 - 0.5 * th) - ul * 0.5 * sech2) * 1000.0;
  const double lr = c.cg_ratio * c.l, lf = c.l - lr;
  ut.Fxf = 0.5 * c.kd * fd + 0.5 * c.kb * fb - 0.5 * c.fr * c.m * LMPC_DTRACK_GRAVITY * lr / c.l;
  ut.Fxr = 0.5 * (1 - c.kd) * fd + 0.5 * (1.0 - c.kb) * fb - 0.5 * c.fr * c.m * LMPC_DTRACK_GRAVITY * lf / c.l;
  ut.fsum = fd + fb;
  ut.dFxf = 0.5 * c.kd * dfd + 0.5 * c.kb * dfb;
  ut.dFxr = 0.5 * (1 - c.kd) * dfd + 0.5 * (1.0 - c.kb) * dfb;
  ut.dfsum = dfd + dfb;
  ut.de = de;
  sincos(de, &ut.sd, &ut.cd);
}

// the partials of rows 0..2 at one point: f0 = v cos(phi + beta) / (1 - e_y k), f1 = v sin(phi + beta), f2 = omega - k f0
struct dtm_kin {
  double f0_ey, f0_ang, f0_v;  // d f0 / d e_y, / d e_psi = / d beta, / d v
  double f1_ang, f1_v;         // d f1 / d e_psi = / d beta, / d v
};

// rows 0..2 of x_dot at the native point x = [s, e_y, e_psi, omega, beta, v], and their partials
__device__ __forceinline__ void dtm_kinematics(const double* x, double k, double* f, dtm_kin& J) {
  const double ey = x[1], phi = x[2], om = x[3], beta = x[4], v = x[5];
  double sp, cp;
  sincos(phi + beta, &sp, &cp);
  const double den = 1.0 - ey * k;
  f[0] = v * cp / den;
  f[1] = v * sp;
  f[2] = om - k * f[0];
  J.f0_ey = f[0] * k / den;
  J.f0_ang = -v * sp / den;
  J.f0_v = cp / den;
  J.f1_ang = v * cp;
  J.f1_v = sp;
}

// The force block: rows 3..5 of x_dot (omega_dot, beta_dot, v_dot) at (omega, beta, v), with the tangents theta[first .. first + K)
// of theta = (omega, beta, v, u_L, delta).  out[0..2] = f[3], f[4], f[5].
template <int K>
__device__ __forceinline__ void dtm_force(const lmpc_vehicle_dt& p, const dtm_uterms& ut, double om_, double beta_, double v_, int first,
                                          dtm_dual<K>* out) {
  typedef dtm_dual<K> D;
  const lmpc_vehicle& c = p.base;
  const D om = dtm_var<K>(om_, 0, first), beta = dtm_var<K>(beta_, 1, first), v = dtm_var<K>(v_, 2, first);
  const D ul = dtm_var<K>(0.0, 3, first), de = dtm_var<K>(ut.de, 4, first);  // (u_L enters through its three forces only)
  const D Fxf = dtm_chain(ul, ut.Fxf, ut.dFxf), Fxr = dtm_chain(ul, ut.Fxr, ut.dFxr), fsum = dtm_chain(ul, ut.fsum, ut.dfsum);
  const D sd = dtm_chain(de, ut.sd, ut.cd), cd = dtm_chain(de, ut.cd, -ut.sd);
  const double m = c.m, l = c.l, lr = c.cg_ratio * l, lf = l - lr;
  const D vsq = v * v;
  const D ax = (fsum - (0.5 * c.cd * c.Af) * vsq - c.fr * m * LMPC_DTRACK_GRAVITY) / m;  // :227
  // :230-235 -- BOTH static terms carry lr, as written
  const double Fz0 = 0.5 * m * LMPC_DTRACK_GRAVITY * lr / (lf + lr), hx = 0.5 * c.h / (lf + lr) * m;
  const D Fzf = Fz0 - hx * ax + (0.25 * c.cl_f * c.rho * c.Af) * vsq;
  const D Fzr = Fz0 + hx * ax + (0.25 * c.cl_r * c.rho * c.Af) * vsq;
  D sb, cb;
  dtm_sincos(beta, sb, cb);
  // :240-245
  const D vsb = v * sb, vc = v * cb;
  const D nf = lf * om + vsb, nr = lr * om - vsb;
  const D hf = (0.5 * p.tw_f) * om, hr = (0.5 * p.tw_r) * om;
  const D S_fl = dtm_magic(c.Bf, c.Cf, p.Ef, de - dtm_atan(nf / (vc - hf)));
  const D S_fr = dtm_magic(c.Bf, c.Cf, p.Ef, de - dtm_atan(nf / (vc + hf)));
  const D S_rl = dtm_magic(c.Br, c.Cr, p.Er, dtm_atan(nr / (vc - hr)));
  const D S_rr = dtm_magic(c.Br, c.Cr, p.Er, dtm_atan(nr / (vc + hr)));
  // the lateral load transfer (:316-322), dtrack_f's Newton iteration on the values
  const double kf = p.kroll_f, kr = 1.0 - p.kroll_f;
  const double ef = p.eps_f / p.Fz0_f, er = p.eps_r / p.Fz0_r;
  const double cg = c.h / (0.5 * (p.tw_f + p.tw_r));
  double gam = 0.0, g_gam = 1.0;
#pragma unroll 1
  for (int it = 0; it <= LMPC_DTRACK_NEWTON; ++it) {
    const double Fz_fl = Fzf.v - kf * gam, Fz_fr = Fzf.v + kf * gam, Fz_rl = Fzr.v - kr * gam, Fz_rr = Fzr.v + kr * gam;
    const double dF = c.mu * kf * ((1.0 + 2.0 * ef * Fz_fr) * S_fr.v - (1.0 + 2.0 * ef * Fz_fl) * S_fl.v);
    const double dR = c.mu * kr * ((1.0 + 2.0 * er * Fz_rr) * S_rr.v - (1.0 + 2.0 * er * Fz_rl) * S_rl.v);
    g_gam = 1.0 - cg * (dR + dF * ut.cd);
    if (it < LMPC_DTRACK_NEWTON) {  // (the last trip only forms g_gamma at the solved gamma)
      const double Fy_f = c.mu * Fz_fl * (1.0 + ef * Fz_fl) * S_fl.v + c.mu * Fz_fr * (1.0 + ef * Fz_fr) * S_fr.v;
      const double Fy_r = c.mu * Fz_rl * (1.0 + er * Fz_rl) * S_rl.v + c.mu * Fz_rr * (1.0 + er * Fz_rr) * S_rr.v;
      const double g = gam - cg * (Fy_r + 2.0 * ut.Fxf * ut.sd + Fy_f * ut.cd);
      gam -= g / g_gam;
    }
  }
  // the tyre forces at gamma with its tangent still to come: Fy_ij = mu Fz_ij (1 + e Fz_ij) S_ij, Fz_ij = Fz -/+ kappa gamma.  With
  // gamma HELD, the tangent of g is g_theta; d gamma = -g_theta / g_gamma then enters every Fy_ij through d Fy_ij / d gamma.
  D Fy_f, Fy_r, Fy_fd;
  {
    const D Fz_fl = Fzf - kf * gam, Fz_fr = Fzf + kf * gam, Fz_rl = Fzr - kr * gam, Fz_rr = Fzr + kr * gam;
    const D Fy_fl = (c.mu * Fz_fl) * (1.0 + ef * Fz_fl) * S_fl, Fy_fr = (c.mu * Fz_fr) * (1.0 + ef * Fz_fr) * S_fr;
    const D Fy_rl = (c.mu * Fz_rl) * (1.0 + er * Fz_rl) * S_rl, Fy_rr = (c.mu * Fz_rr) * (1.0 + er * Fz_rr) * S_rr;
    Fy_f = Fy_fl + Fy_fr;
    Fy_r = Fy_rl + Fy_rr;
    Fy_fd = Fy_fl - Fy_fr;
    const D g = gam - cg * (Fy_r + 2.0 * (Fxf * sd) + Fy_f * cd);
    // d Fy / d gamma per axle: front sum, rear sum, front difference
    const double sFl = c.mu * kf * (1.0 + 2.0 * ef * Fz_fl.v) * S_fl.v, sFr = c.mu * kf * (1.0 + 2.0 * ef * Fz_fr.v) * S_fr.v;
    const double sRl = c.mu * kr * (1.0 + 2.0 * er * Fz_rl.v) * S_rl.v, sRr = c.mu * kr * (1.0 + 2.0 * er * Fz_rr.v) * S_rr.v;
    DTM_EACH {
      const double dgam = -g.d[j] / g_gam;
      Fy_f.d[j] += (sFr - sFl) * dgam;
      Fy_r.d[j] += (sRr - sRl) * dgam;
      Fy_fd.d[j] += (-sFl - sFr) * dgam;
    }
  }
  // :258-267 with Fx_fl = Fx_fr = Fxf, Fx_rl = Fx_rr = Fxr
  D sdb, cdb;
  dtm_sincos(de - beta, sdb, cdb);
  const D drag = (0.5 * c.cd * c.rho * c.Af) * vsq;
  out[2] = (1.0 / m) * (2.0 * (Fxr * cb) + 2.0 * (Fxf * cdb) + Fy_r * sb - Fy_f * sdb - drag * cb);
  out[1] = -om + (dtm_const<K>(1.0) / (m * v)) * (-2.0 * (Fxr * sb) + 2.0 * (Fxf * sdb) + Fy_r * cb + Fy_f * cdb + drag * sb);
  out[0] = (1.0 / c.Jzz) * (-lr * Fy_r + (0.5 * p.tw_f) * (Fy_fd * sd) + lf * (Fy_f * cd + 2.0 * (Fxf * sd)));
}

#undef DTM_EACH
#undef DTM_FN
#undef DTM_D

#endif  // LMPC_DTRACK_PARTIALS_HIP_H_
