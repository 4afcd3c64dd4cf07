"""The plain reference of the per-car single-track controller model (include/lmpc_hip_cars_model.h): the oracle's own discrete Jacobian,
oracle.dynamics.rk4_jacobian_analytic, called stage by stage with car b's Vehicle -- for a car on Euler, whose weights that function
does not know, the same hand-derived partials (oracle.dynamics.f_and_partials) in A = I + dt Fx, Bm = dt Fu.  The complex-step
Jacobian rk4_jacobian_cs, which goes through oracle.dynamics.rk4 and so through either integrator, is the independent cross-check
(tests/test_cars_model_reference.py).  The product's own linearisation is never a reference here.  Also here: the three kinds of car,
the draws of tests/test_gpu_cars_model.py and the table of the fixtures tests/golden/dense_cars_*.npz (generator:
tests/golden/make_cars_model_fixtures.py)."""
from __future__ import annotations

import dataclasses

import numpy as np

import dense_cases as DC
from oracle import dynamics as D, params as P, qp as Q, scenario as S

KEYS = ("X_ref", "U_ref", "T_ref", "curvatures")


def kinds(base):
    """Three cars, none the handle's preset `base`, all three changed only in fields the dynamics read: less grip and more mass; the
    centre of gravity moved back and a larger yaw inertia; other tyre curves on a higher centre of gravity."""
    return (dict(base, mu=0.7 * base["mu"], m=1.15 * base["m"]),
            dict(base, cg_ratio=base["cg_ratio"] + 0.08, Jzz=1.4 * base["Jzz"]),
            dict(base, Bf=0.7 * base["Bf"], Cf=0.9 * base["Cf"], Br=0.75 * base["Br"], Cr=0.92 * base["Cr"], h=1.5 * base["h"]))


def oracle_vehicle(d) -> P.Vehicle:
    """a vehicle dict of the binding as the oracle's Vehicle ("integrator" "rk4" | "euler", or 0 | 1 as the table reads back)"""
    integ = d["integrator"] if isinstance(d["integrator"], str) else ("rk4", "euler")[d["integrator"]]
    return P.Vehicle(**dict({f.name: d[f.name] for f in dataclasses.fields(P.Vehicle) if f.name != "integrator"}, integrator=integ))


def stage_jacobian(x, u, k, dt, v: P.Vehicle):
    """(A, Bm, g) of one step of the oracle's model on vehicle v at the points x (..., 6), u (..., 2)"""
    if v.integrator == "euler":
        f, Fx, Fu = D.f_and_partials(np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64), k, v)
        dt_ = np.broadcast_to(np.asarray(dt, dtype=np.float64), np.shape(x)[:-1])[..., None]
        A, Bm = np.eye(6) + dt_[..., None] * Fx, dt_[..., None] * Fu
        return A, Bm, x + dt_ * f - np.einsum("...ij,...j->...i", A, x) - np.einsum("...ij,...j->...i", Bm, u)
    return D.rk4_jacobian_analytic(x, u, k, dt, v)[:3]


def groups(veh):
    """cars by distinct vehicle"""
    out = {}
    for b, v in enumerate(veh):
        out.setdefault(tuple(sorted(v.items())), []).append(b)
    return list(out.values())


def reference(inp, veh, jac=stage_jacobian):
    """What lmpc_linearize_cars_batch writes for the inputs `inp` (batch axis last) and the table `veh`: A [6, 6, N-1, B],
    Bm [6, 2, N-1, B], g [6, N-1, B]; stage by stage, each distinct vehicle on its own problems."""
    X, U, T, kap = (np.asarray(inp[k], dtype=np.float64) for k in KEYS)
    NS, B = U.shape[1], U.shape[2]
    A, Bm, g = np.full((6, 6, NS, B), np.nan), np.full((6, 2, NS, B), np.nan), np.full((6, NS, B), np.nan)
    for cars in groups(veh):
        v = oracle_vehicle(veh[cars[0]])
        for i in range(NS):
            a, b, c = jac(X[:, i, cars].T, U[:, i, cars].T, kap[i, cars], T[i, cars], v)
            A[:, :, i, cars], Bm[:, :, i, cars], g[:, i, cars] = a.transpose(1, 2, 0), b.transpose(1, 2, 0), c.T
    return A, Bm, g


def qp_model(ref):
    """reference()'s arrays as oracle.qp.build_qp(lin=...) takes them, per problem: A [B, N-1, 6, 6], Bm [B, N-1, 6, 2], g [B, N-1, 6]"""
    A, Bm, g = ref
    return A.transpose(3, 2, 0, 1), Bm.transpose(3, 2, 0, 1), g.transpose(2, 1, 0)


# ---- the fixtures: tests/golden/dense_cars_<name>.npz ----
# name: (dense_cases family, N, problems, what it covers)
FIXTURES = {
    "cars_trk_n20": ("trk", 20, 48, "48 of barc_tracking_n20: the one-wave kernel"),
    "cars_trk_n41": ("trk", 41, 16, "barc_tracking_mpc(41) on the trk family's draws: the smallest two-wave horizon"),
    "cars_lrn_n20_s160": ("lrn", 20, 16, "16 of barc_lmpc_n20_s160: the learning kernel, safe set as in that build"),
    "cars_iac_n40": ("iac", 40, 16, "16 of iac_tracking_n40: IAC scale"),
}
EULER_PROBLEMS = (4, 8)   # a car of the second kind and one of the third
MIN_DISTANCE = 1e-4       # every fixture optimum is further than this (scaled X / U / dU: 100 x TOL_XU) from the optimum on the handle's vehicle
MAX_CERTIFICATE = 1e-9


def fleet(base, count, euler=EULER_PROBLEMS):
    veh = [kinds(base)[b % 3] for b in range(count)]
    for b in euler:
        if b < count:
            veh[b] = dict(veh[b], integrator="euler")
    return veh


def fixture_vehicles(pkg, name):
    family, _, count, _ = FIXTURES[name]
    return fleet(pkg.presets.iac_vehicle() if family == "iac" else pkg.presets.barc_vehicle(), count)


def presets(pkg, name):
    """(config, vehicle) dicts of the handle that solves the fixture"""
    family, N, _, _ = FIXTURES[name]
    if family == "trk":
        return pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle()
    if family == "iac":
        return pkg.presets.iac_tracking_mpc(N), pkg.presets.iac_vehicle()
    return pkg.presets.barc_lmpc(N, 5), pkg.presets.barc_vehicle()


def build(pkg, name):
    """-> cfg, veh (the oracle's, the HANDLE's vehicle), inp (batch axis last, the fixture's problems), ss_x, ss_j (None for tracking),
    table (vehicle dicts)"""
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


# ---- the draws of tests/test_gpu_cars_model.py ----
EULER = (7, 12)   # the two Euler cars of the draws (where the batch holds them)


def lin_draws(pkg, B, N, seed=43):
    """Linearisation points that are no trajectory: every stage of every problem an independent draw of
    workloads.sample_initial_states inside the BARC input bounds; vehicles by b % 3 with the two Euler cars; T_ref per stage and per
    problem in [0.5, 1.5] x 0.025; curvatures drawn on their own, away from the track's values."""
    rng = np.random.default_rng(seed + 1000 * N + B)
    M = B * N
    L = float(pkg.workloads.synthetic_track("barc")["L"])
    u_lo, u_hi, _, _ = Q.effective_bounds(P.barc_tracking_mpc(20), P.barc_vehicle())
    x, u = pkg.workloads.sample_initial_states("barc", M, L, u_lo, u_hi, seed + N)
    X = np.ascontiguousarray(x.reshape(N, B, 6).transpose(2, 0, 1))
    U = np.ascontiguousarray(u.reshape(N, B, 2)[: N - 1].transpose(2, 0, 1))
    inp = {"X_ref": X, "U_ref": U, "T_ref": 0.025 * rng.uniform(0.5, 1.5, (N - 1, B)), "curvatures": rng.uniform(-0.8, 0.8, (N, B))}
    return inp, fleet(pkg.presets.barc_vehicle(), B, EULER)
