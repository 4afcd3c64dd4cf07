"""The plain reference of the double-track controller model (include/lmpc_hip_dtrack_model.h): a torch float64 restatement of
tests/dtrack_cases.py -- f_continuous, step_native, to_native, from_native, with the CLOSED-FORM root for gamma_y where the kernel
iterates -- whose Jacobians come from torch.autograd, one vehicle per group of problems.  The Jacobian of the kernel's arithmetic is
never derived from the kernel.  Also here: the draws of tests/test_gpu_dtrack_model.py and the table of the fixtures
tests/golden/dense_dtrack_*.npz (generator: tests/golden/make_dtrack_model_fixtures.py).

The map that is differentiated is Phi(x, u; k, dt) = from_native(step_native(to_native(x), u, k, dt)) in the plant layout
x = [s, e_y, e_psi, vx, vy, omega], u = [LON, STEER]; to_native holds v at 1e-6 from below, the header's speed guard."""
from __future__ import annotations

import numpy as np
import torch

import dense_cases as DC
import dtrack_cases as DT
from oracle import params as P, scenario as S

GRAVITY = DT.GRAVITY
F64 = torch.float64


# ---- dtrack_cases.py in torch (the same lines, the same order) ----
def controls(u):
    ul = u[..., 0]
    return ul * (0.5 * torch.tanh(ul) + 0.5) * 1000.0, ul * (0.5 * torch.tanh(-ul) + 0.5) * 1000.0, u[..., 1]


def f_continuous(x, u, k, p):
    """dtrack_cases.f_continuous: x_dot (..., 6) in the native state [s, e_y, e_psi, omega, beta, v]."""
    py, phi, omega, beta, v = x[..., 1], x[..., 2], x[..., 3], x[..., 4], x[..., 5]
    fd, fb, delta = controls(u)
    v_sq = v ** 2
    m, Jzz, l = p["m"], p["Jzz"], p["l"]
    lr = p["cg_ratio"] * l
    lf = l - lr
    twf, twr, fr, hcog = p["tw_f"], p["tw_r"], p["fr"], p["h"]
    rho, A, cd = p["rho"], p["Af"], p["cd"]
    Fx_f = 0.5 * p["kd"] * fd + 0.5 * p["kb"] * fb - 0.5 * fr * m * GRAVITY * lr / l
    Fx_r = 0.5 * (1 - p["kd"]) * fd + 0.5 * (1.0 - p["kb"]) * fb - 0.5 * fr * m * GRAVITY * lf / l
    ax = (fd + fb - 0.5 * cd * A * v_sq - fr * m * GRAVITY) / m
    Fz_f = 0.5 * m * GRAVITY * lr / (lf + lr) - 0.5 * hcog / (lf + lr) * m * ax + 0.25 * p["cl_f"] * rho * A * v_sq
    Fz_r = 0.5 * m * GRAVITY * lr / (lf + lr) + 0.5 * hcog / (lf + lr) * m * ax + 0.25 * p["cl_r"] * rho * A * v_sq
    sb, cb = torch.sin(beta), torch.cos(beta)
    a_fl = delta - torch.atan((lf * omega + v * sb) / (v * cb - 0.5 * twf * omega))
    a_fr = delta - torch.atan((lf * omega + v * sb) / (v * cb + 0.5 * twf * omega))
    a_rl = torch.atan((lr * omega - v * sb) / (v * cb - 0.5 * twr * omega))
    a_rr = torch.atan((lr * omega - v * sb) / (v * cb + 0.5 * twr * omega))

    def magic(B, C, E, a):
        return torch.sin(C * torch.atan(B * a - E * (B * a - torch.atan(B * a))))

    S_ij = (magic(p["Bf"], p["Cf"], p["Ef"], a_fl), magic(p["Bf"], p["Cf"], p["Ef"], a_fr),
            magic(p["Br"], p["Cr"], p["Er"], a_rl), magic(p["Br"], p["Cr"], p["Er"], a_rr))
    # gamma_closed_form
    cg = hcog / (0.5 * (twf + twr))
    cd_, sd_ = torch.cos(delta), torch.sin(delta)
    F = (Fz_f, Fz_f, Fz_r, Fz_r)
    sigma = (-1.0, 1.0, -1.0, 1.0)
    kappa = (p["kroll_f"], p["kroll_f"], 1.0 - p["kroll_f"], 1.0 - p["kroll_f"])
    e = (p["eps_f"] / p["Fz0_f"], p["eps_f"] / p["Fz0_f"], p["eps_r"] / p["Fz0_r"], p["eps_r"] / p["Fz0_r"])
    w = (cd_, cd_, 1.0, 1.0)
    mu = p["mu"]
    a = sum(-cg * w[i] * mu * S_ij[i] * e[i] * kappa[i] ** 2 for i in range(4))
    b = 1.0 + sum(-cg * w[i] * mu * S_ij[i] * sigma[i] * kappa[i] * (1.0 + 2.0 * e[i] * F[i]) for i in range(4))
    c = -cg * (sum(w[i] * mu * S_ij[i] * (F[i] + e[i] * F[i] ** 2) for i in range(4)) + 2.0 * Fx_f * sd_)
    q = -0.5 * (b + torch.where(b < 0, -1.0, 1.0) * torch.sqrt(b * b - 4.0 * a * c))
    gamma_y = c / q
    # loads, lateral_forces
    Fz_ij = (Fz_f - kappa[0] * gamma_y, Fz_f + kappa[0] * gamma_y, Fz_r - kappa[2] * gamma_y, Fz_r + kappa[2] * gamma_y)
    eps = (p["eps_f"], p["eps_f"], p["eps_r"], p["eps_r"])
    Fz0 = (p["Fz0_f"], p["Fz0_f"], p["Fz0_r"], p["Fz0_r"])
    Fy_fl, Fy_fr, Fy_rl, Fy_rr = (mu * Fz * (1.0 + eps[i] * Fz / Fz0[i]) * S_ij[i] for i, Fz in enumerate(Fz_ij))
    Fx_fl, Fx_fr, Fx_rl, Fx_rr = Fx_f, Fx_f, Fx_r, Fx_r
    v_dot = 1.0 / m * ((Fx_rl + Fx_rr) * cb + (Fx_fl + Fx_fr) * torch.cos(delta - beta) + (Fy_rl + Fy_rr) * sb
                       - (Fy_fl + Fy_fr) * torch.sin(delta - beta) - 0.5 * cd * rho * A * v_sq * cb)
    beta_dot = -omega + 1.0 / (m * v) * (-(Fx_rl + Fx_rr) * sb + (Fx_fl + Fx_fr) * torch.sin(delta - beta)
                                         + (Fy_rl + Fy_rr) * cb + (Fy_fl + Fy_fr) * torch.cos(delta - beta)
                                         + 0.5 * cd * rho * A * v_sq * sb)
    omega_dot = 1.0 / Jzz * ((Fx_rr - Fx_rl) * twr / 2 - (Fy_rl + Fy_rr) * lr
                             + ((Fx_fr - Fx_fl) * cd_ + (Fy_fl - Fy_fr) * sd_) * twf / 2.0
                             + ((Fy_fl + Fy_fr) * cd_ + (Fx_fl + Fx_fr) * sd_) * lf)
    vx = v * torch.cos(phi + beta) / (1 - py * k)
    vy = v * torch.sin(phi + beta)
    phi_dot = omega - k * vx
    return torch.stack([vx, vy, phi_dot, omega_dot, beta_dot, v_dot], dim=-1)


def step_native(x, u, k, dt, p):
    k1 = f_continuous(x, u, k, p)
    dtc = dt[..., None]
    if p.get("integrator", "rk4") in ("euler", 1):
        return x + dtc * k1
    k2 = f_continuous(x + dtc / 2.0 * k1, u, k, p)
    k3 = f_continuous(x + dtc / 2.0 * k2, u, k, p)
    k4 = f_continuous(x + dtc * k3, u, k, p)
    return x + dtc / 6 * (k1 + 2 * k2 + 2 * k3 + k4)


def to_native(x, guard=True):
    v = torch.hypot(x[..., 3], x[..., 4])
    if guard:
        v = torch.where(v < 1e-6, torch.full_like(v, 1e-6), v)
    return torch.stack([x[..., 0], x[..., 1], x[..., 2], x[..., 5], torch.atan2(x[..., 4], x[..., 3]), v], dim=-1)


def from_native(z):
    return torch.stack([z[..., 0], z[..., 1], z[..., 2], z[..., 5] * torch.cos(z[..., 4]), z[..., 5] * torch.sin(z[..., 4]), z[..., 3]], dim=-1)


def phi(x, u, k, dt, p):
    """The map the kernel linearises, on torch tensors: x (M, 6), u (M, 2), k (M,), dt (M,)."""
    return from_native(step_native(to_native(x), u, k, dt, p))


def jacobians(x, u, k, dt, p):
    """numpy in, numpy out: A (M, 6, 6) = d Phi / d x, Bm (M, 6, 2) = d Phi / d u, g (M, 6) = Phi - A x - Bm u, by autograd (the
    points are independent: one backward pass per row of Phi gives that row of every point's Jacobian)."""
    xt = torch.tensor(np.asarray(x), dtype=F64, requires_grad=True)
    ut = torch.tensor(np.asarray(u), dtype=F64, requires_grad=True)
    kt, dtt = torch.tensor(np.asarray(k), dtype=F64), torch.tensor(np.asarray(dt), dtype=F64)
    y = phi(xt, ut, kt, dtt, p)
    rows = [torch.autograd.grad(y[:, r].sum(), (xt, ut), retain_graph=True) for r in range(6)]
    A = torch.stack([r[0] for r in rows], dim=1).numpy()
    Bm = torch.stack([r[1] for r in rows], dim=1).numpy()
    g = y.detach().numpy() - np.einsum("mrc,mc->mr", A, np.asarray(x)) - np.einsum("mrc,mc->mr", Bm, np.asarray(u))
    return A, Bm, g


def groups(veh):
    """cars by distinct vehicle"""
    out = {}
    for b, v in enumerate(veh):
        out.setdefault(tuple(sorted(v.items())), []).append(b)
    return list(out.values())


def reference(inp, veh):
    """What lmpc_linearize_dtrack_batch writes for the inputs `inp` (batch axis last) and the table `veh`: A [6, 6, N-1, B],
    Bm [6, 2, N-1, B], g [6, N-1, B]; autograd once per distinct vehicle on that vehicle's problems."""
    X, U, T, kap = (np.asarray(inp[k], dtype=np.float64) for k in ("X_ref", "U_ref", "T_ref", "curvatures"))
    NS, B = U.shape[1], U.shape[2]
    A, Bm, g = np.full((6, 6, NS, B), np.nan), np.full((6, 2, NS, B), np.nan), np.full((6, NS, B), np.nan)
    for cars in groups(veh):
        x = X[:, :NS, cars].transpose(2, 1, 0).reshape(-1, 6)
        u = U[:, :, cars].transpose(2, 1, 0).reshape(-1, 2)
        a, b, c = jacobians(x, u, kap[:NS, cars].T.reshape(-1), T[:, cars].T.reshape(-1), veh[cars[0]])
        n = len(cars)
        A[:, :, :, cars] = a.reshape(n, NS, 6, 6).transpose(2, 3, 1, 0)
        Bm[:, :, :, cars] = b.reshape(n, NS, 6, 2).transpose(2, 3, 1, 0)
        g[:, :, cars] = c.reshape(n, NS, 6).transpose(2, 1, 0)
    return A, Bm, g


def qp_model(ref):
    """reference()'s arrays as oracle.qp.build_qp(lin=...) takes them, per problem: A [B, N-1, 6, 6], Bm [B, N-1, 6, 2], g [B, N-1, 6]"""
    A, Bm, g = ref
    return A.transpose(3, 2, 0, 1), Bm.transpose(3, 2, 0, 1), g.transpose(2, 1, 0)


def numpy_step(x, u, k, dt, p):
    """The same map through tests/dtrack_cases.py (numpy; dt a scalar or one number per point)."""
    z = DT.to_native(np.asarray(x, dtype=np.float64))
    z[..., 5] = np.where(z[..., 5] < 1e-6, 1e-6, z[..., 5])
    dt = np.asarray(dt, dtype=np.float64)
    return DT.from_native(DT.step_native(z, np.asarray(u, dtype=np.float64), k, dt[..., None] if dt.ndim else dt, p))


def richardson(x, u, k, dt, p, h=1e-4):
    """(A, Bm) of numpy_step by Richardson-extrapolated central differences of step h and h / 2 (error O(h^4))."""
    xu = np.concatenate([np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)], axis=1)

    def central(step):
        cols = []
        for c in range(8):
            e = np.zeros(8)
            e[c] = step
            hi, lo = xu + e, xu - e
            cols.append((numpy_step(hi[:, :6], hi[:, 6:], k, dt, p) - numpy_step(lo[:, :6], lo[:, 6:], k, dt, p)) / (2.0 * step))
        return np.stack(cols, axis=2)

    J = (4.0 * central(h / 2.0) - central(h)) / 3.0
    return J[:, :, :6], J[:, :, 6:]


# ---- the fixtures: tests/golden/dense_dtrack_<name>.npz ----
# name: (dense_cases family, N, problems, what it covers)
FIXTURES = {
    "dtrack_trk_n20": ("trk", 20, 48, "48 of barc_tracking_n20: one wave"),
    "dtrack_trk_n41": ("trk", 41, 16, "barc_tracking_mpc(41) on the trk family's draws: the smallest two-wave horizon"),
    "dtrack_iac_n40": ("iac", 40, 16, "16 of iac_tracking_n40: IAC scale"),
    "dtrack_lrn_n20_s160": ("lrn", 20, 32, "32 of barc_lmpc_n20_s160: learning, safe set as in that build"),
}
EULER_PROBLEM = 7
MIN_DISTANCE = 1e-4   # every fixture optimum is further than this (scaled, X / U / dU) from the single-track optimum of its inputs
MAX_CERTIFICATE = 1e-9


def fixture_vehicles(pkg, name):
    """by b % 3: the preset; mu = 0.7 (BARC) or 0.7 x preset (IAC); kroll_f = 0.35 with Ef = Er = 0.6 -- and problem 7 on Euler"""
    family, _, count, _ = FIXTURES[name]
    base = pkg.presets.iac_double_track() if family == "iac" else pkg.presets.barc_double_track()
    kinds = (dict(base), dict(base, mu=0.7 * base["mu"] if family == "iac" else 0.7), dict(base, kroll_f=0.35, Ef=0.6, Er=0.6))
    veh = [kinds[b % 3] for b in range(count)]
    veh[EULER_PROBLEM] = dict(veh[EULER_PROBLEM], integrator="euler")
    return veh


def presets(pkg, name):
    """(config, vehicle) dicts of the handle that solves the fixture"""
    family, N, _, _ = FIXTURES[name]
    if family == "trk":
        return pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle()
    if family == "iac":
        return pkg.presets.iac_tracking_mpc(N), pkg.presets.iac_vehicle()
    return pkg.presets.barc_lmpc(N, 5), pkg.presets.barc_vehicle()


def build(pkg, name):
    """-> cfg, veh (the oracle's), inp (batch axis last, the fixture's problems), ss_x, ss_j (None for tracking), table (vehicle dicts)"""
    family, N, count, _ = FIXTURES[name]
    dense = {("trk", 20): "barc_tracking_n20", ("iac", 40): "iac_tracking_n40", ("lrn", 20): "barc_lmpc_n20_s160"}.get((family, N))
    if dense is not None:
        cfg, veh, inp, ss_x, ss_j = DC.build(pkg, dense)
        inp = {k: (np.ascontiguousarray(v[..., :count]) if isinstance(v, np.ndarray) else v) for k, v in inp.items()}
        if ss_x is not None:
            ss_x, ss_j = np.ascontiguousarray(ss_x[..., :count]), np.ascontiguousarray(ss_j[..., :count])
    else:   # the trk family's draws at another horizon
        assert family == "trk"
        tr = pkg.workloads.synthetic_track("barc")
        cfg, veh = P.barc_tracking_mpc(N), P.barc_vehicle()
        x, u = pkg.workloads.sample_initial_states("barc", DC.BATCH, tr["L"], [-0.01, -0.314159], [0.01, 0.314159], seed=0)
        inp, ss_x, ss_j = S.cold_start_inputs(cfg, veh, tr, x[:count], u[:count], 0.025), None, None
    return cfg, veh, inp, ss_x, ss_j, fixture_vehicles(pkg, name)


def digest(inp, ss_x, ss_j, model):
    """dense_cases.digest of the inputs, and per problem the sum of |.| over the reference model (A, Bm, g) the optimum was solved on"""
    A, Bm, g = model
    return DC.digest(inp, ss_x, ss_j), np.abs(A).sum(axis=(1, 2, 3)) + np.abs(Bm).sum(axis=(1, 2, 3)) + np.abs(g).sum(axis=(1, 2))


# ---- the draws of tests/test_gpu_dtrack_model.py ----
EULER = DT.EULER
SLOW = (5, 1)   # (problem, stage) of the knot under the speed guard in the BARC draws


def lin_draws(pkg, kind, B, N, seed=41):
    """Linearisation points that are no trajectory: every stage of every problem an independent draw.  BARC: dtrack_cases.barc_draws'
    distribution (workloads.sample_initial_states inside the BARC input bounds), vehicles by b % 3 with two Euler cars, and one knot
    with (vx, vy) = (3e-7, 0).  IAC: dtrack_cases.iac_draws on the preset.  T_ref per stage and per problem in [0.5, 1.5] x 0.025;
    curvatures drawn on their own, away from the track's values."""
    from oracle import qp as Q
    rng = np.random.default_rng(seed + 1000 * N + B)
    M = B * N
    if kind == "barc":
        L = float(pkg.workloads.synthetic_track("barc")["L"])
        u_lo, u_hi, _, _ = Q.effective_bounds(P.barc_tracking_mpc(20), P.barc_vehicle())
        x, u = pkg.workloads.sample_initial_states("barc", M, L, u_lo, u_hi, seed + N)
        veh = [DT.barc_kinds(pkg.presets.barc_double_track())[b % 3] for b in range(B)]
        for b in EULER:
            veh[b] = dict(veh[b], integrator="euler")
        kmax = 0.8
    else:
        x, u = DT.iac_draws(M, float(DT.iac_track(pkg)["L"]), seed + N)
        veh = [pkg.presets.iac_double_track()] * B
        kmax = 0.01
    X = np.ascontiguousarray(x.reshape(N, B, 6).transpose(2, 0, 1))
    U = np.ascontiguousarray(u.reshape(N, B, 2)[: N - 1].transpose(2, 0, 1))
    if kind == "barc":
        X[3:6, SLOW[1], SLOW[0]] = 3e-7, 0.0, 0.0
    inp = {"X_ref": X, "U_ref": U, "T_ref": 0.025 * rng.uniform(0.5, 1.5, (N - 1, B)), "curvatures": rng.uniform(-kmax, kmax, (N, B))}
    return inp, veh
