"""The batched extended Kalman filter restated in plain numpy, and the scenario its tests run (tests/test_ekf_reference.py,
tests/test_gpu_ekf.py, tests/golden/ekf_one_car.npz).

`Filter` is EKFStateEstimator::update_observation (ekf_state_estimator.cpp:112-214) for B cars at once, built on the oracle's
single-track model with k = 0 (oracle.dynamics.rk4 / rk4_jacobian_analytic): prediction through the RK4 (or Euler) map, F P F' + Q,
the correction in the non-symmetric form as written, the NaN / Inf fallback per car, check_cov with its column-0 quirk, the clip,
the side-by-side gain storage, and a timestamp that may jump back (the negative dt is used).  An observation is an ordered list of
state rows; a yaw row is aligned to its measurement (lmpc_utils/utils.hpp:25-31).

T = np.float64 is the reference of the device tests.  T = np.longdouble is its extended-precision twin -- the model in longdouble,
F by complex-step differentiation in clongdouble, S^-1 refined by two Newton steps -- which measures how far rounding alone moves
the answer (the reference's own sensitivity).

WHERE IT HOLDS: the model is stiff at low speed (BARC: modes near -102 / vx and -216 / vx per second; RK4 is unstable past
216 dt / vx = 2.78), so the scenario keeps vx >= 1.5 m/s and updates at 5 ms; there the two precisions agree to a few 1e-15.
"""
from __future__ import annotations

import numpy as np

from oracle import dynamics as D
from oracle import params as OP

FALLBACK, R_REPAIRED, NOT_FINITE = 1, 2, 4

SD0 = np.array([0.5, 0.5, 0.3, 0.5, 0.2, 0.5])
Q_DIAG = np.array([1e-4, 1e-4, 1e-4, 1e-2, 1e-2, 1e-2])
X_MAX = np.array([np.inf, np.inf, np.inf, 6.0, 1.5, 20.0])
SIG_VEL = np.array([0.05, 0.05])
SIG_POSE = np.array([0.02, 0.02, 0.01])
ROWS_VEL, ROWS_POSE = (3, 5), (0, 1, 2)
TOL = 1e-10      # device against the fp64 restatement: |dx|, |dP|, |dK|
TOL_TWIN = 1e-13  # the restatement against its extended-precision twin on the scenario


def config(x0=None, P0=None, Q=None, x_min=None, x_max=None) -> dict:
    return {"x0": np.zeros(6) if x0 is None else np.asarray(x0, dtype=np.float64),
            "P0": np.diag(SD0 ** 2) if P0 is None else np.asarray(P0, dtype=np.float64),
            "Q": np.diag(Q_DIAG) if Q is None else np.asarray(Q, dtype=np.float64),
            "x_min": -X_MAX if x_min is None else np.asarray(x_min, dtype=np.float64),
            "x_max": X_MAX if x_max is None else np.asarray(x_max, dtype=np.float64)}


def align_yaw(yaw_1, yaw_2):
    d = yaw_1 - yaw_2
    return np.arctan2(np.sin(d), np.cos(d)) + yaw_2


def check_cov(R):
    """check_cov as written (:238-264) on a copy: the inner loop advances i, so only column 0 is visited.  R [B, nz, nz].
    Returns (R', repaired [B])."""
    R = R.copy()
    rep = np.zeros(R.shape[0], dtype=bool)
    for i in range(R.shape[1]):
        neg = R[:, i, 0] < 0.0
        R[neg, i, 0] = 0.0
        rep |= neg
        if i == 0:
            npos = R[:, 0, 0] <= 0.0
            R[npos, 0, 0] = 1e-6
            rep |= npos
    return R, rep


class Filter:
    """B filters in arrays with the batch axis FIRST: x [B, 6], u [B, 2], P [B, 6, 6], K [B, 6, sum nz]."""

    def __init__(self, veh, cfg: dict, B: int, T=np.float64):
        self.veh, self.T, self.B = veh, T, B
        self.Q = cfg["Q"].astype(T)
        self.x_min, self.x_max = cfg["x_min"], cfg["x_max"]
        self.x0, self.P0 = cfg["x0"], cfg["P0"]
        self.obs, self.nzsum = [], 0
        self.initialized, self.ns = False, 0
        self.u = np.zeros((B, 2), dtype=T)
        self.K = np.zeros((B, 6, 0), dtype=T)
        self.set_state()

    def set_state(self, x=None, P=None):
        self.x = np.tile(self.x0, (self.B, 1)).astype(self.T) if x is None else np.array(x, dtype=self.T)
        self.P = np.tile(self.P0, (self.B, 1, 1)).astype(self.T) if P is None else np.array(P, dtype=self.T)

    def register_observation(self, rows) -> int:
        rows = [int(r) for r in rows]
        if self.initialized:
            raise RuntimeError("Changes to observations are not allowed after the filter is initialized.")
        if not 1 <= len(rows) <= 6 or len(set(rows)) != len(rows) or min(rows) < 0 or max(rows) > 5:
            raise ValueError("1 .. 6 distinct rows of 0 .. 5")
        self.obs.append((rows, self.nzsum))
        self.nzsum += len(rows)
        self.K = np.concatenate([self.K, np.zeros((self.B, 6, len(rows)), dtype=self.T)], axis=2)
        return len(self.obs) - 1

    def initialize(self, timestamp_ns: int):
        if not self.obs:
            raise RuntimeError("No observation has been registered for the filter.")
        self.initialized, self.ns = True, int(timestamp_ns)

    def update_control(self, u):
        self.u = np.array(u, dtype=self.T)

    def _predict(self, dt):
        T, veh = self.T, self.veh
        if T is np.float64:
            xp = D.rk4(self.x, self.u, 0.0, dt, veh)
            if getattr(veh, "integrator", "rk4") == "euler":
                F = np.eye(6) + dt * D.f_and_partials(self.x, self.u, 0.0, veh)[1]
            else:
                F = D.rk4_jacobian_analytic(self.x, self.u, 0.0, dt, veh)[0]
        else:
            CT = np.clongdouble
            xp = D.rk4(self.x, self.u, T(0.0), T(dt), veh)
            F = np.empty((self.B, 6, 6), dtype=T)
            for j in range(6):
                xc = self.x.astype(CT)
                xc[:, j] += 1j * T(1e-40)
                F[:, :, j] = D.rk4(xc, self.u.astype(CT), T(0.0), T(dt), veh).imag / T(1e-40)
        return xp, F @ self.P @ np.swapaxes(F, 1, 2) + self.Q

    def update(self, obs_id: int, z, R, timestamp_ns: int):
        """One update of every filter.  z [B, nz], R [B, nz, nz] (None with obs_id = -1).  Returns (x [B, 6], P [B, 6, 6],
        Kz [B, 6, nz] or None, flags [B])."""
        if not self.initialized:
            raise RuntimeError("Call EKFStateEstimator::initialize() before making any observation updates.")
        if not -1 <= obs_id < len(self.obs):
            raise KeyError(obs_id)
        T = self.T
        dt = float(int(timestamp_ns) - self.ns) * 1e-9   # a jump back only sets the time upstream: the negative dt is used (:130-146)
        xp, Pp = self._predict(dt)
        flags = np.zeros(self.B, dtype=np.int32)
        Kz = None
        if obs_id < 0:
            xn, Pn = xp, Pp
        else:
            rows, koff = self.obs[obs_id]
            nz = len(rows)
            z64, R64 = np.asarray(z, dtype=np.float64), np.asarray(R, dtype=np.float64)
            bad = ~(np.isfinite(z64).all(axis=1) & np.isfinite(R64).all(axis=(1, 2)))
            zz = np.where(bad[:, None], 0.0, z64).astype(T)
            Rc, rep = check_cov(np.where(bad[:, None, None], np.eye(nz), R64))
            Rc = Rc.astype(T)
            H = np.zeros((nz, 6), dtype=T)
            H[np.arange(nz), rows] = 1
            hx = xp[:, rows].copy()
            for a, r in enumerate(rows):
                if r == 2:
                    hx[:, a] = align_yaw(hx[:, a], zz[:, a])
            y = zz - hx
            S = H @ Pp @ H.T + Rc
            Sinv = np.linalg.inv(S.astype(np.float64)).astype(T)
            if T is not np.float64:
                for _ in range(2):
                    Sinv = Sinv @ (2 * np.eye(nz, dtype=T) - S @ Sinv)
            K = Pp @ H.T @ Sinv
            xn = xp + np.einsum("bij,bj->bi", K, y)
            Pn = (np.eye(6, dtype=T) - K @ H) @ Pp
            xn[bad], Pn[bad] = xp[bad], Pp[bad]
            good = ~bad
            self.K[good, :, koff:koff + nz] = K[good]
            Kz = self.K[:, :, koff:koff + nz].copy()
            flags |= np.where(bad, FALLBACK, 0).astype(np.int32) | np.where(rep & good, R_REPAIRED, 0).astype(np.int32)
        xn = np.clip(xn, self.x_min, self.x_max).astype(T)
        fin = np.isfinite(xn.astype(np.float64)).all(axis=1) & np.isfinite(Pn.astype(np.float64)).all(axis=(1, 2))
        flags |= np.where(fin, 0, NOT_FINITE).astype(np.int32)
        self.x, self.P, self.ns = xn, Pn, int(timestamp_ns)
        return xn.copy(), Pn.copy(), Kz, flags


def scenario(B: int, periods: int = 400, seed: int = 3, dt_ns: int = 10_000_000, veh=None, lon=None):
    """The issue's scenario for B cars: BARC vehicle, period 10 ms; per period the control u = (0.0008 + 0.001 sin(1.3 t + phi),
    0.2 sin(0.9 t + phi)), a velocity observation (rows 3, 5; sigma 0.05) at mid-period and a pose observation (rows 0, 1, 2; sigma
    0.02, 0.02, 0.01; yaw wrapped to (-pi, pi]) at the period, the pose dropped (NaN in z[0]) for 10 % of the cars; truth starts at
    vx ~ U(1.5, 2.5), yaw ~ U(-3, 3); the filters start at truth + 0.5 N(0, 1) sd0 (vx floored at 0.5) with P0 = diag(sd0^2).
    Returns {"veh", "cfg", "x0" [B, 6], "P0" [B, 6, 6], "updates": list of (obs, z [B, nz], R [B, nz, nz], u [B, 2], timestamp_ns),
    "truth": [periods, B, 6]} -- obs 0 is the velocity observation, 1 the pose.  `lon`: another u_lon, a function of (period k, phi [B])."""
    veh = OP.barc_vehicle() if veh is None else veh
    rng = np.random.default_rng(seed)
    dt = dt_ns * 1e-9
    xt = np.zeros((B, 6))
    xt[:, 0], xt[:, 1] = rng.uniform(-1, 1, B), rng.uniform(-1, 1, B)
    xt[:, 2], xt[:, 3] = rng.uniform(-3, 3, B), rng.uniform(1.5, 2.5, B)
    x0 = xt + 0.5 * rng.normal(0, 1, (B, 6)) * SD0
    x0[:, 3] = np.maximum(x0[:, 3], 0.5)
    ph = rng.uniform(0, 6.28, B)
    Rv = np.tile(np.diag(SIG_VEL ** 2), (B, 1, 1))
    Rp = np.tile(np.diag(SIG_POSE ** 2), (B, 1, 1))
    updates, truth = [], []
    for k in range(periods):
        t = k * dt
        u = np.stack([0.0008 + 0.001 * np.sin(1.3 * t + ph) if lon is None else lon(k, ph), 0.2 * np.sin(0.9 * t + ph)], axis=1)
        xt = D.rk4(xt, u, 0.0, dt / 2, veh)
        zv = xt[:, list(ROWS_VEL)] + rng.normal(0, SIG_VEL, (B, 2))
        updates.append((0, zv, Rv, u, k * dt_ns + dt_ns // 2))
        xt = D.rk4(xt, u, 0.0, dt / 2, veh)
        zp = xt[:, :3] + rng.normal(0, SIG_POSE, (B, 3))
        zp[:, 2] = np.arctan2(np.sin(zp[:, 2]), np.cos(zp[:, 2]))
        zp[rng.random(B) < 0.1, 0] = np.nan
        updates.append((1, zp, Rp, u, (k + 1) * dt_ns))
        truth.append(xt.copy())
    return {"veh": veh, "cfg": config(), "x0": x0, "P0": np.tile(np.diag(SD0 ** 2), (B, 1, 1)), "updates": updates,
            "truth": np.array(truth)}


def new_filter(sc: dict, T=np.float64, B: int | None = None) -> Filter:
    """A Filter on the scenario's vehicle and config with its two observations registered, seeded and initialised at t = 0."""
    B = sc["x0"].shape[0] if B is None else B
    f = Filter(sc["veh"], sc["cfg"], B, T)
    assert f.register_observation(ROWS_VEL) == 0 and f.register_observation(ROWS_POSE) == 1
    f.set_state(sc["x0"][:B], sc["P0"][:B])
    f.initialize(0)
    return f


def run(sc: dict, T=np.float64, B: int | None = None):
    """The scenario through a Filter: the list of (x, P, Kz, flags) after every update, as float64."""
    B = sc["x0"].shape[0] if B is None else B
    f = new_filter(sc, T, B)
    out = []
    for obs, z, R, u, ns in sc["updates"]:
        f.update_control(u[:B])
        x, P, Kz, fl = f.update(obs, z[:B], R[:B], ns)
        out.append((x.astype(np.float64), P.astype(np.float64), Kz.astype(np.float64), fl))
    return out


def spd(rng, B: int, nz: int, scale: float = 0.05):
    """Dense random symmetric positive definite R [B, nz, nz] with positive entries in column 0 (check_cov leaves it alone)."""
    A = rng.normal(0, 1, (B, nz, nz))
    R = scale ** 2 * (np.eye(nz) * nz + 0.3 * (A @ np.swapaxes(A, 1, 2)) / nz)
    R[:, :, 0] = np.abs(R[:, :, 0])
    R[:, 0, :] = R[:, :, 0]
    return R
