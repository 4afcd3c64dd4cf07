"""lmpc_vanilla_rollout_fleet_batch (include/lmpc_hip_vanilla_fleet.h) restated in plain numpy from what exists, and the fleets its
tests run (tests/test_vanilla_fleet_reference.py, tests/test_gpu_vanilla_fleet.py).

Per period: vanilla_cases.decide with the HANDLE's vehicle; the plant -- vanilla_cases.plant with car b's vehicle ("handle", "cars")
or dtrack_cases.plant_step with car b's four-wheel vehicle ("dtrack"), run once per distinct vehicle on that vehicle's cars --; the
logs, accumulators and the freeze of vanilla_cases.rollout; and, for the live cars, one safe_set.SafeSetRecorder.step per car into a
safe_set.SafeSetManager whose laps are capped like the device store's slots (HostFleet), by either convention: "applied", the input
applied FROM the sample's state, or "arrived", the input that led TO it.
"""
from __future__ import annotations

import copy

import numpy as np

import dtrack_cases as DC
import vanilla_cases as VC
from oracle import params as OP

B_TEST, PERIODS = VC.B_TEST, VC.PERIODS
CAR_MU, CAR_M, EULER = (0.7, 0.85, 1.0), (1.0, 1.1, 1.2), (7, 12)   # by b % 3: mu x, m x; the two Euler cars
PLANTS = ("handle", "cars", "dtrack")
RING = 3            # laps per car in the store (max_lap_stored of the solvers the tests make)

# Measured by tests/test_vanilla_fleet_reference.py on exactly the batch the device test uses (the BARC scenario, B = 67, 64 periods,
# the double-track fleet below), elementwise vanilla_cases.err over x, X_log, U_log, k_log, distance, worst_excess and the PID state:
# the restatement with dtrack_cases' closed-form gamma_y root against the same restatement with LMPC_DTRACK_NEWTON = 5 Newton
# iterations from gamma = 0 (decision 1 of include/lmpc_hip_dtrack.h):                                     1.5e-14 (X_log)
TOL_TWIN_DTRACK = 1e-13                 # that line, rounded up to a power of ten
TOL_DTRACK = 1e4 * TOL_TWIN_DTRACK      # device against restatement, the rule vanilla_cases.TOL_ROLLOUT was made by; above 1e-8 the
#                                         scenario would be replaced, not the tolerance widened


# ---- the fleets ----
def car_factors(B: int):
    return [(CAR_MU[b % 3], CAR_M[b % 3], "euler" if b in EULER else "rk4") for b in range(B)]


def car_vehicles(sc: dict, B: int, mixed: bool = True):
    """Car b's oracle.params vehicle: the scenario's with mu and m scaled by b % 3, cars 7 and 12 on Euler; mixed=False: the
    scenario's vehicle for every car."""
    out = []
    for mu, m, integ in car_factors(B):
        v = copy.copy(sc["veh"])
        if mixed:
            v.mu, v.m, v.integrator = sc["veh"].mu * mu, sc["veh"].m * m, integ
        out.append(v)
    return out


def car_vehicle_dicts(pkg, sc: dict, B: int, mixed: bool = True):
    """The same fleet as Solver.set_car_vehicles takes it."""
    base = dict(pkg.presets.barc_vehicle() if sc["vehicle"] == "barc" else pkg.presets.iac_vehicle(), **sc["veh_over"])
    if not mixed:
        return [dict(base) for _ in range(B)]
    return [dict(base, mu=base["mu"] * mu, m=base["m"] * m, integrator=integ) for mu, m, integ in car_factors(B)]


def dtrack_vehicles(pkg, B: int):
    """Car b's four-wheel vehicle, by b % 3: dtrack_cases.barc_kinds of the BARC preset."""
    kinds = DC.barc_kinds(pkg.presets.barc_double_track())
    return [kinds[b % 3] for b in range(B)]


def _groups(vehicles):
    """Cars by distinct vehicle: [(vehicle, [cars])]."""
    found = {}
    for b, v in enumerate(vehicles):
        key = tuple(sorted((v if isinstance(v, dict) else vars(v)).items()))
        found.setdefault(key, (v, []))[1].append(b)
    return list(found.values())


# ---- the recorder: one SafeSetRecorder / SafeSetManager per car, the slots capped like the store's ----
class HostFleet:
    """tests/test_gpu_fleet_ss.py's host_fleet, fed sample by sample: a lap longer than `cap` samples is not added (n_dropped)."""

    def __init__(self, pkg, B: int, cap: int, ring: int = RING):
        SS = pkg.safe_set

        class Capped(SS.SafeSetManager):
            def __init__(self):
                super().__init__(ring)
                self.n_dropped, self.t_first, self.lengths = 0, None, []

            def add_lap(self, lx, lu, lk, lt, total_length):
                self.t_first = float(np.asarray(lt).reshape(-1)[0])
                n = np.asarray(lx).reshape(-1, 6).shape[0]
                self.lengths.append(n)
                if n > cap:
                    self.n_dropped += 1
                    return
                super().add_lap(lx, lu, lk, lt, total_length)

        self.man = [Capped() for _ in range(B)]
        self.rec = [SS.SafeSetRecorder(m) for m in self.man]
        self.last = np.zeros(B)

    def step(self, b: int, x, u, k, t, L):
        if self.rec[b].step(x, u, k, t, L):
            self.last[b] = t - self.man[b].t_first

    def stats(self) -> dict:
        return {"laps_in_ring": np.array([len(m.laps) for m in self.man], dtype=np.int32),
                "lap_count": np.array([r.lap_count for r in self.rec], dtype=np.int32),
                "n_dropped": np.array([m.n_dropped for m in self.man], dtype=np.int32), "last_lap_time": self.last.copy()}

    def laps(self, b: int):
        return list(self.man[b].laps)

    def lap_lengths(self, b: int):
        """Samples of every closed lap of car b, dropped ones included."""
        return list(self.man[b].lengths)


# ---- the double-track restatement's second opinion on gamma_y: the kernel's iteration ----
def gamma_newton(Fx_f, Fz_f, Fz_r, S_ij, delta, p, count: int = 5):
    """LMPC_DTRACK_NEWTON iterations from gamma = 0 with the analytic derivative (tests/test_dtrack_reference.py's restatement of
    them), in dtrack_cases.gamma_closed_form's place."""
    cg = p["h"] / (0.5 * (p["tw_f"] + p["tw_r"]))
    ef, er, kf, kr = p["eps_f"] / p["Fz0_f"], p["eps_r"] / p["Fz0_r"], p["kroll_f"], 1.0 - p["kroll_f"]
    gam = np.zeros_like(Fz_f)
    for _ in range(count):
        Fz = DC.loads(Fz_f, Fz_r, gam, p)
        Fy = DC.lateral_forces(Fz, S_ij, p)
        g = gam - cg * (Fy[2] + Fy[3] + (Fx_f + Fx_f) * np.sin(delta) + (Fy[0] + Fy[1]) * np.cos(delta))
        dF = p["mu"] * kf * ((1.0 + 2.0 * ef * Fz[1]) * S_ij[1] - (1.0 + 2.0 * ef * Fz[0]) * S_ij[0])
        dR = p["mu"] * kr * ((1.0 + 2.0 * er * Fz[3]) * S_ij[3] - (1.0 + 2.0 * er * Fz[2]) * S_ij[2])
        gam = gam - g / (1.0 - cg * (dR + dF * np.cos(delta)))
    return gam


class newton_gamma:
    """Within the block dtrack_cases solves gamma_y by the kernel's Newton iterations instead of the closed form."""

    def __enter__(self):
        self.saved, DC.gamma_closed_form = DC.gamma_closed_form, gamma_newton

    def __exit__(self, *exc):
        DC.gamma_closed_form = self.saved


# ---- the entry point ----
def plant_step(plant: str, veh, vehicles, trk: dict, x, u, dt_sim, n_sub: int):
    if plant == "handle":
        return VC.plant(veh, trk, x, u, dt_sim, n_sub, np.float64)
    out = np.empty_like(x)
    table = {"curvature": trk["table"]["curvature"], "L": trk["L"]}
    for v, cars in _groups(vehicles):
        if plant == "cars":
            out[cars] = VC.plant(v, trk, x[cars], u[cars], dt_sim, n_sub, np.float64)
        else:
            out[cars] = DC.plant_step(v, table, x[cars], u[cars], dt_sim, n_sub)[0]
    return out


def rollout(veh, cfg: dict, trk: dict, x0, pid: dict, periods: int, dt_sim: float, n_sub: int, speed_scale: float, plant: str = "handle",
            vehicles=None, record=None, fleet: HostFleet | None = None, period0: int = 0, dt=None, u_prev=None, distance=None,
            worst_excess=None) -> dict:
    """lmpc_vanilla_rollout_fleet_batch for B cars: vanilla_cases.rollout's dictionary and "u_prev" [B, 2] (the last input applied;
    the argument's row for a car that never moved).  vehicles: car b's plant vehicle for "cars" (oracle.params vehicles) and
    "dtrack" (dicts).  record: None, "applied" or "arrived", into `fleet`, stamped (period0 + p) * dt."""
    assert plant in PLANTS and record in (None, "applied", "arrived")
    T = np.float64
    x = np.asarray(x0).astype(T)
    B = x.shape[0]
    pid = {k: np.asarray(v).astype(T) for k, v in pid.items()}
    tab, L, M = trk["table"], T(trk["L"]), trk["table"]["M"]
    X_log, U_log, k_log = np.full((B, 6, periods), np.nan), np.full((B, 2, periods), np.nan), np.full((B, periods), np.nan)
    dist = np.zeros(B) if distance is None else np.array(distance, dtype=T)
    worst = np.full(B, -np.inf) if worst_excess is None else np.array(worst_excess, dtype=T)
    up = np.zeros((B, 2)) if u_prev is None else np.array(u_prev, dtype=T)
    frozen = np.zeros(B, dtype=bool)
    half_b = T(veh.b) / T(2.0)
    with np.errstate(all="ignore"):
        for p in range(periods):
            o = VC.decide(veh, cfg, trk, x, pid, None, speed_scale, T)
            live = ~frozen & (o["flags"] == 0)
            xs_in = np.where(live[:, None], x, T(1.0))
            u = np.where(live[:, None], o["u_model"], T(0.0))
            xs = plant_step(plant, veh, vehicles, trk, xs_in, u, dt_sim, n_sub)
            live &= np.isfinite(xs).all(axis=1)
            frozen = ~live
            kap = VC.table_lookup(tab["curvature"], M, L, x[:, 0], T)
            X_log[live, :, p], U_log[live, :, p], k_log[live, p] = x[live], o["u_model"][live], kap[live]
            if record is not None:
                t = float(period0 + p) * dt
                for b in np.flatnonzero(live):
                    fleet.step(b, x[b], up[b] if record == "arrived" else o["u_model"][b], kap[b], t, float(L))
            up = np.where(live[:, None], o["u_model"], up)
            ds = xs[:, 0] - x[:, 0]
            dist += np.where(live, np.where(ds < -L / 2, ds + L, ds), T(0.0))
            bl, br = VC.table_lookup(tab["bound_left"], M, L, x[:, 0], T), VC.table_lookup(tab["bound_right"], M, L, x[:, 0], T)
            exc = np.maximum(xs[:, 1] + half_b - bl, br - (xs[:, 1] - half_b))
            worst = np.where(live, np.maximum(worst, exc), worst)
            x = np.where(live[:, None], xs, x)
            pid = {k: np.where(live, o["pid"][k], pid[k]) for k in pid}
    return {"x": x, "pid": pid, "X_log": X_log, "U_log": U_log, "k_log": k_log, "distance": dist, "worst_excess": worst,
            "flags": np.where(frozen, VC.NOT_FINITE, 0).astype(np.int32), "u_prev": up}


_CACHE: dict = {}


def reference(pkg, plant: str, periods: int = PERIODS, B: int = B_TEST, mixed: bool = True):
    """The restatement on the BARC scenario from a zero PID state, no recorder; computed once per process and shared (read-only)."""
    key = (plant, periods, B, mixed)
    if key not in _CACHE:
        sc = VC.scenario("barc", B)
        vehicles = None if plant == "handle" else car_vehicles(sc, B, mixed) if plant == "cars" else dtrack_vehicles(pkg, B)
        _CACHE[key] = rollout(sc["veh"], sc["cfg"], sc["trk"], sc["x0"], VC.zero_pid(B), periods, sc["dt_sim"], sc["n_sub"], sc["speed_scale"],
                              plant=plant, vehicles=vehicles)
    return _CACHE[key]
