"""The plain reference of the double-track plant (include/lmpc_hip_dtrack.h): a numpy restatement of
DoubleTrackPlanarModel::compile_dynamics written line by line against double_track_planar_model.cpp:163-347 (use_frenet = true),
with the four decisions of that header, and the draws the tests of the plant share.

ONE deliberate difference from the kernel makes it an independent check of the kernel's Newton iteration: gamma_y is the CLOSED-FORM
root of g(gamma) = gamma - h / (0.5 (tw_f + tw_r)) (Fy_rl + Fy_rr + (Fx_fl + Fx_fr) sin(delta) + (Fy_fl + Fy_fr) cos(delta)), which
is a quadratic a gamma^2 + b gamma + c in gamma -- the root that is continuous from gamma = 0 (the one that stays finite as a -> 0),
c / q with q = -(b + sign(b) sqrt(b^2 - 4 a c)) / 2.

Lookup and wrap are oracle.scenario.track_lookup and oracle.dynamics.align_abscissa.  A vehicle is a flat dict with
presets.barc_double_track's keys; one call steps a batch of cars that share one vehicle."""
from __future__ import annotations

import numpy as np

from oracle import dynamics as D, scenario as S

GRAVITY = 9.8  # double_track_planar_model.cpp: GRAVITY


def controls(u):
    """(fd, fb, delta) of the two-control layout, as the single-track dynamics map it (single_track_planar_model.cpp:215-216)."""
    ul = u[..., 0]
    return ul * (0.5 * np.tanh(ul) + 0.5) * 1000.0, ul * (0.5 * np.tanh(-ul) + 0.5) * 1000.0, u[..., 1]


def tyre_terms(x, u, p):
    """What the lateral forces are built from, at the native state x = [s, e_y, e_psi, omega, beta, v] (..., 6): the four
    longitudinal forces, the axle loads before the transfer, and the four load-independent factors sin(C atan(...))."""
    omega, beta, v = x[..., 3], x[..., 4], x[..., 5]
    fd, fb, delta = controls(u)
    v_sq = v ** 2
    kd_f, kb_f, m, l = p["kd"], p["kb"], p["m"], p["l"]
    lr = p["cg_ratio"] * l
    lf = l - lr
    twf, twr, fr, hcog = p["tw_f"], p["tw_r"], p["fr"], p["h"]
    rho, A, cd = p["rho"], p["Af"], p["cd"]
    # :218-224
    Fx_f = 0.5 * kd_f * fd + 0.5 * kb_f * fb - 0.5 * fr * m * GRAVITY * lr / l
    Fx_r = 0.5 * (1 - kd_f) * fd + 0.5 * (1.0 - kb_f) * fb - 0.5 * fr * m * GRAVITY * lf / l
    # :227
    ax = (fd + fb - 0.5 * cd * A * v_sq - fr * m * GRAVITY) / m
    # :230-235 (both static terms carry lr, as written)
    Fz_f = 0.5 * m * GRAVITY * lr / (lf + lr) - 0.5 * hcog / (lf + lr) * m * ax + 0.25 * p["cl_f"] * rho * A * v_sq
    Fz_r = 0.5 * m * GRAVITY * lr / (lf + lr) + 0.5 * hcog / (lf + lr) * m * ax + 0.25 * p["cl_r"] * rho * A * v_sq
    # :240-245
    a_fl = delta - np.arctan((lf * omega + v * np.sin(beta)) / (v * np.cos(beta) - 0.5 * twf * omega))
    a_fr = delta - np.arctan((lf * omega + v * np.sin(beta)) / (v * np.cos(beta) + 0.5 * twf * omega))
    a_rl = np.arctan((lr * omega - v * np.sin(beta)) / (v * np.cos(beta) - 0.5 * twr * omega))
    a_rr = np.arctan((lr * omega - v * np.sin(beta)) / (v * np.cos(beta) + 0.5 * twr * omega))

    def magic(B, C, E, a):  # the factor of :248-255 that does not depend on the load
        return np.sin(C * np.arctan(B * a - E * (B * a - np.arctan(B * a))))

    S_ij = (magic(p["Bf"], p["Cf"], p["Ef"], a_fl), magic(p["Bf"], p["Cf"], p["Ef"], a_fr),
            magic(p["Br"], p["Cr"], p["Er"], a_rl), magic(p["Br"], p["Cr"], p["Er"], a_rr))
    return Fx_f, Fx_r, Fz_f, Fz_r, S_ij


def loads(Fz_f, Fz_r, gamma_y, p):
    """:232-237, (fl, fr, rl, rr)"""
    kroll_f = p["kroll_f"]
    return (Fz_f - kroll_f * gamma_y, Fz_f + kroll_f * gamma_y, Fz_r - (1.0 - kroll_f) * gamma_y, Fz_r + (1.0 - kroll_f) * gamma_y)


def lateral_forces(Fz_ij, S_ij, p):
    """:248-255, (fl, fr, rl, rr)"""
    mu = p["mu"]
    e = (p["eps_f"], p["eps_f"], p["eps_r"], p["eps_r"])
    Fz0 = (p["Fz0_f"], p["Fz0_f"], p["Fz0_r"], p["Fz0_r"])
    return tuple(mu * Fz * (1.0 + e[i] * Fz / Fz0[i]) * S_ij[i] for i, Fz in enumerate(Fz_ij))


def residual(gamma_y, x, u, p):
    """g(gamma_y) of :316-318, from the forces as written."""
    Fx_f, _, Fz_f, Fz_r, S_ij = tyre_terms(x, u, p)
    Fy = lateral_forces(loads(Fz_f, Fz_r, gamma_y, p), S_ij, p)
    delta = u[..., 1]
    return gamma_y - p["h"] / (0.5 * (p["tw_f"] + p["tw_r"])) * (Fy[2] + Fy[3] + (Fx_f + Fx_f) * np.sin(delta) + (Fy[0] + Fy[1]) * np.cos(delta))


def gamma_closed_form(Fx_f, Fz_f, Fz_r, S_ij, delta, p):
    """The root of g continuous from gamma = 0.  With F the axle load, sigma = -/+ 1 (left / right), kappa the axle's share of the
    transfer and e = eps / Fz0:  Fy_ij = mu S_ij ((F + e F^2) + sigma kappa (1 + 2 e F) gamma + e kappa^2 gamma^2)."""
    cg = p["h"] / (0.5 * (p["tw_f"] + p["tw_r"]))
    cd_, sd_ = np.cos(delta), np.sin(delta)
    F = (Fz_f, Fz_f, Fz_r, Fz_r)
    sigma = (-1.0, 1.0, -1.0, 1.0)
    kappa = (p["kroll_f"], p["kroll_f"], 1.0 - p["kroll_f"], 1.0 - p["kroll_f"])
    e = (p["eps_f"] / p["Fz0_f"], p["eps_f"] / p["Fz0_f"], p["eps_r"] / p["Fz0_r"], p["eps_r"] / p["Fz0_r"])
    w = (cd_, cd_, 1.0, 1.0)
    a = sum(-cg * w[i] * p["mu"] * S_ij[i] * e[i] * kappa[i] ** 2 for i in range(4))
    b = 1.0 + sum(-cg * w[i] * p["mu"] * S_ij[i] * sigma[i] * kappa[i] * (1.0 + 2.0 * e[i] * F[i]) for i in range(4))
    c = -cg * (sum(w[i] * p["mu"] * S_ij[i] * (F[i] + e[i] * F[i] ** 2) for i in range(4)) + 2.0 * Fx_f * sd_)
    q = -0.5 * (b + np.where(b < 0, -1.0, 1.0) * np.sqrt(b * b - 4.0 * a * c))
    return c / q


def f_continuous(x, u, k, p):
    """x_dot (..., 6) in the native state, gamma_y, and Fz_ij (fl, fr, rl, rr)."""
    py, phi, omega, beta, v = x[..., 1], x[..., 2], x[..., 3], x[..., 4], x[..., 5]
    _, _, delta = controls(u)
    v_sq = v ** 2
    m, Jzz, l = p["m"], p["Jzz"], p["l"]
    lr = p["cg_ratio"] * l
    lf = l - lr
    twf, twr, rho, A, cd = p["tw_f"], p["tw_r"], p["rho"], p["Af"], p["cd"]
    Fx_f, Fx_r, Fz_f, Fz_r, S_ij = tyre_terms(x, u, p)
    Fx_fl, Fx_fr, Fx_rl, Fx_rr = Fx_f, Fx_f, Fx_r, Fx_r
    gamma_y = gamma_closed_form(Fx_f, Fz_f, Fz_r, S_ij, delta, p)
    Fz_ij = loads(Fz_f, Fz_r, gamma_y, p)
    Fy_fl, Fy_fr, Fy_rl, Fy_rr = lateral_forces(Fz_ij, S_ij, p)
    # :258-267
    v_dot = 1.0 / m * ((Fx_rl + Fx_rr) * np.cos(beta) + (Fx_fl + Fx_fr) * np.cos(delta - beta) + (Fy_rl + Fy_rr) * np.sin(beta)
                       - (Fy_fl + Fy_fr) * np.sin(delta - beta) - 0.5 * cd * rho * A * v_sq * np.cos(beta))
    beta_dot = -omega + 1.0 / (m * v) * (-(Fx_rl + Fx_rr) * np.sin(beta) + (Fx_fl + Fx_fr) * np.sin(delta - beta)
                                         + (Fy_rl + Fy_rr) * np.cos(beta) + (Fy_fl + Fy_fr) * np.cos(delta - beta)
                                         + 0.5 * cd * rho * A * v_sq * np.sin(beta))
    omega_dot = 1.0 / Jzz * ((Fx_rr - Fx_rl) * twr / 2 - (Fy_rl + Fy_rr) * lr
                             + ((Fx_fr - Fx_fl) * np.cos(delta) + (Fy_fl - Fy_fr) * np.sin(delta)) * twf / 2.0
                             + ((Fy_fl + Fy_fr) * np.cos(delta) + (Fx_fl + Fx_fr) * np.sin(delta)) * lf)
    # :270-277
    vx = v * np.cos(phi + beta) / (1 - py * k)
    vy = v * np.sin(phi + beta)
    phi_dot = omega - k * vx
    return np.stack([vx, vy, phi_dot, omega_dot, beta_dot, v_dot], axis=-1), gamma_y, Fz_ij


def step_native(x, u, k, dt, p):
    """lmpc_utils utils.cpp:88-108 (RK4) or :110-123 (Euler, for a vehicle with integrator "euler" / 1) on the native state."""
    k1 = f_continuous(x, u, k, p)[0]
    if p.get("integrator", "rk4") in ("euler", 1):
        return x + dt * k1
    k2 = f_continuous(x + dt / 2.0 * k1, u, k, p)[0]
    k3 = f_continuous(x + dt / 2.0 * k2, u, k, p)[0]
    k4 = f_continuous(x + dt * k3, u, k, p)[0]
    return x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)


def to_native(x):
    """[s, e_y, e_psi, vx, vy, omega] -> [s, e_y, e_psi, omega, beta, v]"""
    return np.stack([x[..., 0], x[..., 1], x[..., 2], x[..., 5], np.arctan2(x[..., 4], x[..., 3]), np.hypot(x[..., 3], x[..., 4])], axis=-1)


def from_native(z):
    return np.stack([z[..., 0], z[..., 1], z[..., 2], z[..., 5] * np.cos(z[..., 4]), z[..., 5] * np.sin(z[..., 4]), z[..., 3]], axis=-1)


def plant_step(p, track, x, u, dt_sim, n_sub=1):
    """lmpc_plant_step_dtrack_batch on cars that share the vehicle p: x (B, 6) in the plant layout, u (B, 2).  Returns the new
    states and the gamma_y of the first evaluation of the last sub-step."""
    L = float(track["L"])
    z = to_native(np.array(x, dtype=np.float64))
    u = np.asarray(u, dtype=np.float64)
    gamma_y = None
    for _ in range(n_sub):
        z[:, 5] = np.where(z[:, 5] < 1e-6, 1e-6, z[:, 5])
        k = S.track_lookup(track["curvature"], z[:, 0], L)
        gamma_y = f_continuous(z, u, k, p)[1]
        z = step_native(z, u, k, dt_sim, p)
        z[:, 0] = D.align_abscissa(z[:, 0], L / 2.0, L)
    return from_native(z), gamma_y


# the same car seen in a mirror: e_y, e_psi, vy, omega and STEER negated (and the track's curvature with them)
MIRROR_X, MIRROR_U = np.array([1.0, -1.0, -1.0, 1.0, -1.0, -1.0]), np.array([1.0, -1.0])


# ---- the draws ----
DT_SIM, N_SUB = 0.0125, 2
SLOW, LINE, EULER = 5, 11, (7, 12)   # the car under the speed guard, the car within a sub-step of the start line, the two Euler cars


def barc_kinds(base):
    """by b % 3: the preset; mu = 0.7; kroll_f = 0.35 with Ef = Er = 0.6"""
    return (dict(base), dict(base, mu=0.7), dict(base, kroll_f=0.35, Ef=0.6, Er=0.6))


def barc_draws(pkg, B, L):
    """tests/test_gpu_plant_cars.py's draws -- workloads.sample_initial_states("barc", ...) with seed 31 inside the BARC input bounds
    -- its start-line car, and the car under the guard.  The guard holds v at 1e-6, where the slip equation's 1 / (m v) makes any
    lateral motion stiffer than a step of this size resolves (no implementation reproduces another there); the guard car is
    therefore drawn with NO lateral motion -- vy = omega = STEER = 0, where beta_dot and omega_dot are exact zeros on both sides --
    and pulls away at the largest LON of the bounds.  (With LON = 0 rolling resistance takes its native v BELOW zero in the first
    sub-step.  The exit conversion hands such a car out as (|v|, beta + pi), the same motion, but the guard tells the two apart: a
    further sub-step of the same call lifts v = -1.5e-3 to 1e-6, a second call sees v = +1.5e-3 and leaves it.  That is the
    guard as include/lmpc_hip_dtrack.h decides it, noted there; a car that pulls away never meets it.)"""
    from oracle import params as P, qp as Q
    u_lo, u_hi, _, _ = Q.effective_bounds(P.barc_tracking_mpc(20), P.barc_vehicle())
    x, u = pkg.workloads.sample_initial_states("barc", B, L, u_lo, u_hi, 31)
    x[SLOW, 3:6] = 3e-7, 0.0, 0.0
    u[SLOW] = u_hi[0], 0.0
    x[LINE, 0], x[LINE, 3] = L - 0.2 * x[LINE, 3] * DT_SIM, abs(x[LINE, 3])   # crosses the line in its first sub-step
    veh = [barc_kinds(pkg.presets.barc_double_track())[b % 3] for b in range(B)]
    for b in EULER:
        veh[b] = dict(veh[b], integrator="euler")
    return x, u, veh


def iac_track(pkg):
    """workloads.synthetic_track("putnam") with the curvature held to |k| <= 0.01"""
    tr = dict(pkg.workloads.synthetic_track("putnam"))
    tr["curvature"] = np.clip(tr["curvature"], -0.01, 0.01)
    return tr


def iac_draws(B, L, seed=31):
    """The IAC-scale set: vx ~ U(15, 70), u_L ~ U(-2, 2); the rest as workloads.sample_initial_states("putnam", ...)."""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(0.0, L, B), rng.uniform(-1.5, 1.5, B), rng.normal(0.0, 0.05, B), rng.uniform(15.0, 70.0, B),
                  rng.normal(0.0, 0.5, B), rng.normal(0.0, 0.1, B)], axis=-1)
    u = np.stack([rng.uniform(-2.0, 2.0, B), rng.normal(0.0, 0.02, B)], axis=-1)
    return x, u


def reference(track, x, u, veh, dt_sim=DT_SIM, n_sub=N_SUB):
    """plant_step once per distinct vehicle on that vehicle's cars: (states (B, 6), gamma_y (B,))."""
    want, gam = np.full((len(veh), 6), np.nan), np.full(len(veh), np.nan)
    groups = {}
    for b, v in enumerate(veh):
        groups.setdefault(tuple(sorted(v.items())), []).append(b)
    for cars in groups.values():
        want[cars], gam[cars] = plant_step(veh[cars[0]], track, x[cars], u[cars], dt_sim, n_sub)
    return want, gam
