"""The batched time-varying LQR restated in plain numpy, and the scenarios its tests run (tests/test_lqr_reference.py,
tests/test_gpu_lqr.py, tests/golden/lqr_one_car.npz).

`solve` is RacingLQR::solve (racing_lqr.cpp:45-96) for B cars at once on the oracle's single-track model with k = 0: per stage the
continuous Jacobian at (X_ref[:,k], U_ref[:,k]), [A B; 0 I] = expm([Ac Bc; 0 0] dt), K_k = solve(R + B'PB, B'PA),
P <- Q + A'P(A - B K_k) -- Q, R, Qf general, nothing symmetrised -- then the rollout U = U_ref - K (X - X_ref) (no wrapped yaw)
through an RK4 that is always RK4, whatever the vehicle's integrator says.

T = np.float64 is the reference of the device tests: oracle.dynamics.f_and_partials, scipy.linalg.expm (a Pade method, so
independent of the device's Taylor series), np.linalg.solve.  T = np.longdouble is its extended-precision twin -- the Jacobian by
complex-step differentiation in clongdouble, expm by a scaled Taylor series with squaring, the 2 x 2 solve and the recursion in
longdouble, the rollout in float64 under the twin's gains -- which measures how far rounding alone moves the answer.

WHERE IT HOLDS: the LQR has no bounds and the model is stiff at low speed (RK4 unstable past 216 dt / vx = 2.78 for BARC), so
the scenarios are chosen (below) and tests/test_lqr_reference.py checks the choice on every car.
"""
from __future__ import annotations

import numpy as np

from oracle import dynamics as D
from oracle import params as OP

NOT_FINITE = 1

# Measured by tests/test_lqr_reference.py on exactly the batches the device tests use (B = 67 per scenario, B = 8 on the loop),
# errors elementwise |d| / max(1, |reference|):
#   restatement vs twin, worst over SCENARIOS and the general-matrix case:   X 1.2e-14   U 2.5e-14   K 4.4e-14   P0 3.8e-14
#   run_lqr loop (8 BARC cars, N = 21, 25 periods):                          X 2.2e-16   U 9.5e-17
# Two seeds were replaced after that measurement, as the rule below demands: ("barc", 41, 0.01, 14) holds one car whose open-loop
# reference brakes to vx = 0 (twin distance 7e-10) and ("iac", 81, 0.05, 17) one whose reference spins (1e-7, 130 m off).
TOL_TWIN = 1e-13       # the worst of the first line, rounded up to a power of ten
TOL = 1e4 * TOL_TWIN   # device against restatement: 1e-9; above 1e-8 a scenario would be too ill-conditioned and be replaced
TOL_TWIN_LOOP = 1e-15  # the second line, rounded up
TOL_LOOP = 1e4 * TOL_TWIN_LOOP
MAX_DEVIATION = {"barc": 2.0, "iac": 20.0}  # max |X_optm - X_ref| a scenario's car may reach [m, rad, m/s]

# (vehicle, N, dt, seed), every one at B = 67 on the device
SCENARIOS = (("barc", 2, 0.01, 11), ("barc", 3, 0.01, 12), ("barc", 21, 0.01, 13), ("barc", 41, 0.01, 24), ("barc", 65, 0.005, 15),
             ("iac", 40, 0.025, 16), ("iac", 81, 0.05, 27))
B_TEST = 67


def vehicle(kind: str):
    return OP.barc_vehicle() if kind == "barc" else OP.iac_vehicle()


def config(N: int, dt: float, Q=None, R=None, Qf=None) -> dict:
    """param/sample_lqr.param.yaml's weights on the two-control layout (presets.sample_lqr)."""
    return {"N": int(N), "dt": float(dt), "Q": np.eye(6) if Q is None else np.asarray(Q, dtype=np.float64),
            "R": np.eye(2) if R is None else np.asarray(R, dtype=np.float64),
            "Qf": np.diag([10.0, 10.0, 10.0, 1.0, 1.0, 10.0]) if Qf is None else np.asarray(Qf, dtype=np.float64)}


def general_config(N: int, dt: float, seed: int = 5) -> dict:
    """Non-symmetric Q and Qf, a full non-symmetric R."""
    rng = np.random.default_rng(seed)
    Q = np.eye(6) + 0.2 * rng.uniform(-1, 1, (6, 6))
    Qf = np.diag([10.0, 10.0, 10.0, 1.0, 1.0, 10.0]) + 0.3 * rng.uniform(-1, 1, (6, 6))
    return config(N, dt, Q=Q, R=np.array([[1.0, 0.3], [-0.2, 1.5]]), Qf=Qf)


def rk4(veh, x, u, dt):
    """utils::rk4_function with k = 0 (utils.cpp:88-108): never Euler."""
    k1 = D.f_continuous(x, u, 0.0, veh)
    k2 = D.f_continuous(x + dt / 2.0 * k1, u, 0.0, veh)
    k3 = D.f_continuous(x + dt / 2.0 * k2, u, 0.0, veh)
    k4 = D.f_continuous(x + dt * k3, u, 0.0, veh)
    return x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)


def euler_rollout(veh, cfg, x_ic, X_ref, U_ref, K):
    """The rollout with x + dt f in place of RK4 under given gains K [B, 2, 6, N-1]: what a controller that followed an Euler
    vehicle's integrator would return."""
    N, dt = cfg["N"], cfg["dt"]
    X = np.empty_like(X_ref)
    X[:, :, 0] = x_ic
    for k in range(N - 1):
        u = U_ref[:, :, k] - np.einsum("bij,bj->bi", K[:, :, :, k], X[:, :, k] - X_ref[:, :, k])
        X[:, :, k + 1] = X[:, :, k] + dt * D.f_continuous(X[:, :, k], u, 0.0, veh)
    return X


def jacobian(veh, x, u, T=np.float64):
    """(Ac [B, 6, 6], Bc [B, 6, 2]) of the continuous dynamics at curvature 0."""
    if T is np.float64:
        _, Fx, Fu = D.f_and_partials(x, u, 0.0, veh)
        return Fx, Fu
    CT, h = np.clongdouble, T(1e-40)
    xc, uc = x.astype(CT), u.astype(CT)
    Ac, Bc = np.empty(x.shape[:-1] + (6, 6), dtype=T), np.empty(x.shape[:-1] + (6, 2), dtype=T)
    for j in range(6):
        xp = xc.copy()
        xp[..., j] += 1j * h
        Ac[..., :, j] = D.f_continuous(xp, uc, T(0.0), veh).imag / h
    for j in range(2):
        up = uc.copy()
        up[..., j] += 1j * h
        Bc[..., :, j] = D.f_continuous(xc, up, T(0.0), veh).imag / h
    return Ac, Bc


def expm_taylor(M, T=np.longdouble, degree: int = 30):
    """expm of M [B, n, n] by scaling to an infinity norm below 1/4, a Taylor series and squaring, in T."""
    M = M.astype(T)
    nrm = float(np.abs(M).sum(axis=-1).max())
    s = max(0, int(np.ceil(np.log2(max(nrm, 1e-300) / 0.25))))
    Ms = M / T(2.0) ** s
    E = np.broadcast_to(np.eye(M.shape[-1], dtype=T), M.shape).copy()
    term = E.copy()
    for j in range(1, degree + 1):
        term = term @ Ms / T(j)
        E = E + term
    for _ in range(s):
        E = E @ E
    return E


def discretize(Ac, Bc, dt, T=np.float64):
    """c2d_function (lmpc_utils/src/utils.cpp:52-65): the top 6 x 8 block of expm([[Ac, Bc], [0, 0]] dt)."""
    M = np.zeros(Ac.shape[:-2] + (8, 8), dtype=T)
    M[..., :6, :6] = Ac * T(dt)
    M[..., :6, 6:] = Bc * T(dt)
    if T is np.float64:
        from scipy.linalg import expm
        E = expm(M)
    else:
        E = expm_taylor(M, T)
    return E[..., :6, :6], E[..., :6, 6:]


def solve2(S, G, T):
    """solve(S, G) for S [B, 2, 2], G [B, 2, 6]."""
    if T is np.float64:
        return np.linalg.solve(S, G)
    det = S[:, 0, 0] * S[:, 1, 1] - S[:, 0, 1] * S[:, 1, 0]
    inv = np.stack([np.stack([S[:, 1, 1], -S[:, 0, 1]], -1), np.stack([-S[:, 1, 0], S[:, 0, 0]], -1)], -2) / det[:, None, None]
    return inv @ G


def solve(veh, cfg: dict, x_ic, X_ref, U_ref, T=np.float64) -> dict:
    """B cars.  x_ic [B, 6], X_ref [B, 6, N], U_ref [B, 2, N-1] -> float64 {"X_optm" [B, 6, N], "U_optm" [B, 2, N-1], "u" [B, 2],
    "K" [B, 2, 6, N-1], "P0" [B, 6, 6], "A" [B, N-1, 6, 6], "B" [B, N-1, 6, 2], "flags" [B]}."""
    N, dt = int(cfg["N"]), float(cfg["dt"])
    x_ic, X_ref, U_ref = (np.asarray(a, dtype=np.float64) for a in (x_ic, X_ref, U_ref))
    nb = x_ic.shape[0]
    assert X_ref.shape == (nb, 6, N) and U_ref.shape == (nb, 2, N - 1) and N >= 2
    Q, R, Qf = (np.asarray(cfg[k]).astype(T) for k in ("Q", "R", "Qf"))
    P = np.broadcast_to(Qf, (nb, 6, 6)).copy()
    K = np.zeros((nb, 2, 6, N - 1), dtype=T)
    As, Bs = np.zeros((nb, N - 1, 6, 6), dtype=T), np.zeros((nb, N - 1, 6, 2), dtype=T)
    with np.errstate(all="ignore"):
        for k in range(N - 2, -1, -1):
            Ac, Bc = jacobian(veh, X_ref[:, :, k].astype(T), U_ref[:, :, k].astype(T), T)
            A, Bd = discretize(Ac, Bc, dt, T)
            Bt, At = np.swapaxes(Bd, 1, 2), np.swapaxes(A, 1, 2)
            Kk = solve2(R + Bt @ P @ Bd, Bt @ P @ A, T)
            P = Q + At @ P @ (A - Bd @ Kk)
            K[:, :, :, k], As[:, k], Bs[:, k] = Kk, A, Bd
        K64 = K.astype(np.float64)
        X, U = np.empty((nb, 6, N)), np.empty((nb, 2, N - 1))
        X[:, :, 0] = x_ic
        for k in range(N - 1):
            U[:, :, k] = U_ref[:, :, k] - np.einsum("bij,bj->bi", K64[:, :, :, k], X[:, :, k] - X_ref[:, :, k])
            X[:, :, k + 1] = rk4(veh, X[:, :, k], U[:, :, k], dt)
    P0 = P.astype(np.float64)
    fin = np.isfinite(X).all(axis=(1, 2)) & np.isfinite(U).all(axis=(1, 2)) & np.isfinite(K64).all(axis=(1, 2, 3)) & np.isfinite(P0).all(axis=(1, 2))
    return {"X_optm": X, "U_optm": U, "u": U[:, :, 0].copy(), "K": K64, "P0": P0, "A": As.astype(np.float64), "B": Bs.astype(np.float64),
            "flags": np.where(fin, 0, NOT_FINITE).astype(np.int32)}


def reference_trajectory(kind: str, M: int, dt: float, B: int, seed: int, veh=None):
    """A reference of M knots that is itself an open-loop RK4 rollout (k = 0) of its U_ref from a random start, and x_ic = the start
    plus a small offset.  Returns (veh, x_ic [B, 6], X_ref [B, 6, M], U_ref [B, 2, M-1]).
      barc: vx in [1.5, 3], yaw ~ N(0, 0.3^2), vy ~ N(0, 0.05^2), omega ~ N(0, 0.2^2), positions in [-1, 1]; u_lon ~ N(0, 0.003^2)
            held, steer 0.1 sin(8 t + phi); offset [0.1, 0.1, 0.03, 0.1, 0.02, 0.1] N(0, 1)
      iac:  vx in [32, 48], the same yaw, vy ~ N(0, 0.2^2), omega ~ N(0, 0.05^2); u_lon ~ N(0, 0.2^2) held, steer 0.03 sin(0.3 i + phi);
            offset [1, 0.5, 0.02, 2, 0.2, 0.05] N(0, 1)"""
    veh = vehicle(kind) if veh is None else veh   # (another vehicle of the same scale)
    rng = np.random.default_rng(seed)
    barc = kind == "barc"
    x = np.zeros((B, 6))
    x[:, 0], x[:, 1] = rng.uniform(-1, 1, B), rng.uniform(-1, 1, B)
    x[:, 2] = rng.normal(0, 0.3, B)
    x[:, 3] = rng.uniform(1.5, 3.0, B) if barc else rng.uniform(32.0, 48.0, B)
    x[:, 4] = rng.normal(0, 0.05 if barc else 0.2, B)
    x[:, 5] = rng.normal(0, 0.2 if barc else 0.05, B)
    ulon = rng.normal(0, 0.003 if barc else 0.2, B)
    ph = rng.uniform(0, 6.28, B)
    off = np.array([0.1, 0.1, 0.03, 0.1, 0.02, 0.1]) if barc else np.array([1.0, 0.5, 0.02, 2.0, 0.2, 0.05])
    x_ic = x + off * rng.normal(0, 1, (B, 6))
    X_ref, U_ref = np.empty((B, 6, M)), np.empty((B, 2, M - 1))
    X_ref[:, :, 0] = x
    for i in range(M - 1):
        steer = 0.1 * np.sin(8.0 * (i * dt) + ph) if barc else 0.03 * np.sin(0.3 * i + ph)
        U_ref[:, :, i] = np.stack([ulon, steer], axis=1)
        X_ref[:, :, i + 1] = rk4(veh, X_ref[:, :, i], U_ref[:, :, i], dt)
    return veh, x_ic, X_ref, U_ref


def scenario(kind: str, N: int, dt: float, seed: int, B: int = B_TEST, general: bool = False, veh=None) -> dict:
    veh, x_ic, X_ref, U_ref = reference_trajectory(kind, N, dt, B, seed, veh)
    return {"kind": kind, "veh": veh, "cfg": general_config(N, dt) if general else config(N, dt), "x_ic": x_ic, "X_ref": X_ref, "U_ref": U_ref}


GENERAL = ("barc", 21, 0.01, 18)  # the non-symmetric case of the device tests: scenario(*GENERAL, general=True)
LOOP = {"B": 8, "N": 21, "dt": 0.01, "steps": 25, "seed": 19}


def loop_scenario() -> dict:
    """run_lqr's case: 8 BARC cars, N = 21, 25 periods over one long reference."""
    M = LOOP["steps"] + LOOP["N"] - 1
    veh, x_ic, X_traj, U_traj = reference_trajectory("barc", M, LOOP["dt"], LOOP["B"], LOOP["seed"])
    return {"kind": "barc", "veh": veh, "cfg": config(LOOP["N"], LOOP["dt"]), "x0": x_ic, "X_traj": X_traj, "U_traj": U_traj, "steps": LOOP["steps"]}


def run_loop(sc: dict, T=np.float64):
    """closed_loop.run_lqr over the restatement: (X [B, 6, steps+1], U [B, 2, steps])."""
    N, steps = sc["cfg"]["N"], sc["steps"]
    x = sc["x0"].copy()
    X, U = [x], []
    for t in range(steps):
        r = solve(sc["veh"], sc["cfg"], x, sc["X_traj"][:, :, t:t + N], sc["U_traj"][:, :, t:t + N - 1], T)
        U.append(r["u"])
        x = r["X_optm"][:, :, 1]
        X.append(x)
    return np.stack(X, axis=2), np.stack(U, axis=2)


def err(got, ref) -> float:
    """The worst elementwise |d| / max(1, |reference|); a NaN on either side is infinite."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    e = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    return float(np.where(np.isfinite(e), e, np.inf).max()) if e.size else 0.0


_CACHE: dict = {}


def reference(key):
    """The float64 restatement on a scenario, computed once per process and shared (treat as read-only).  key: an entry of
    SCENARIOS, or GENERAL + ("general",)."""
    if key not in _CACHE:
        sc = scenario(*key[:4], general=len(key) > 4)
        _CACHE[key] = (sc, solve(sc["veh"], sc["cfg"], sc["x_ic"], sc["X_ref"], sc["U_ref"]))
    return _CACHE[key]
