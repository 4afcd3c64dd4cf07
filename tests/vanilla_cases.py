"""The batched vanilla controller (pure pursuit + PID) and its fused rollout restated in plain numpy, and the scenarios their tests run
(tests/test_vanilla_reference.py, tests/test_gpu_vanilla.py, tests/golden/vanilla_one_car.npz).

`decide` is VanillaController::solve (vanilla_controller.cpp:49-109) with PidController::update (pid_controller.cpp:83-127) for B cars
at once, plus what lmpc_vanilla_solve_batch adds for the fleet (the node's fold, u_model, the reference speed from the spline, the
flag); `rollout` is lmpc_vanilla_rollout_batch: per period the decision, then n_sub plant sub-steps (oracle.dynamics.rk4 with the
curvature of the uniform table at the current abscissa, the |vx| < 1e-6 guard, the abscissa wrap), the logs, distance, worst_excess
and the freeze of a car that turns non-finite.  The track is racing_trajectory.RacingTrajectory's exported splines and tables.

T = np.float64 is the reference of the device tests.  T = np.longdouble is its extended-precision twin: the same splines and tables
(they are the problem's data) evaluated in longdouble, every transcendental, the PID, the model and the whole closed loop carried in
longdouble -- which measures how far rounding alone moves the answer, over exactly the periods the device tests run.
"""
from __future__ import annotations

import copy

import numpy as np

import track_cases as TC
from __graft_entry__ import load_package
from oracle import dynamics as D
from oracle import params as OP

NOT_FINITE = 1
GRAVITY = 9.81      # vanilla_controller.cpp:27, not the model's 9.8
LAPS_MAX = 1e9      # LMPC_VANILLA_LAPS_MAX
B_TEST = 67         # one full wave and a partial one
PERIODS = 64
TABLE_M = 1024

# Measured by tests/test_vanilla_reference.py on exactly the batches the device tests use (B = 67 per scenario), errors elementwise
# |d| / max(1, |reference|), restatement against its longdouble twin, worst over SCENARIOS:
#   one decision (u_out, u_model, PID state; vel_ref NULL and given):            6.8e-14 (synthetic: forces of kN)
#   the rollout, 64 periods (x, X_log, U_log, k_log, distance, worst_excess, PID): 8.9e-13 (synthetic, X_log)
TOL_TWIN = 1e-13            # the first line, rounded up to a power of ten
TOL = 1e4 * TOL_TWIN        # device against restatement, one decision
TOL_TWIN_ROLLOUT = 1e-12    # the second line, rounded up
TOL_ROLLOUT = 1e4 * TOL_TWIN_ROLLOUT   # above 1e-8 a scenario would be too ill-conditioned and be replaced

_PKG = None


def pkg():
    global _PKG
    if _PKG is None:
        _PKG = load_package()
    return _PKG


# ---- the track: exported splines and tables, evaluated in T ----
_TRACKS: dict = {}


def track(name: str) -> dict:
    """{"spline": to_spline_track(), "table": to_track_table(TABLE_M), "L", "tr": the RacingTrajectory} of "barc" or "synthetic"."""
    if name not in _TRACKS:
        tr = pkg().racing_trajectory.RacingTrajectory(TC.table("barc" if name == "barc" else "synthetic"))
        _TRACKS[name] = {"spline": tr.to_spline_track(), "table": tr.to_track_table(TABLE_M), "L": tr.total_length, "tr": tr}
    return _TRACKS[name]


def mod(s, L):
    """align_abscissa(s, L/2, L) (lmpc_utils/utils.hpp:35-41)."""
    k = np.abs(L / 2 - s) + L / 2
    return s + (k - np.fmod(k, L)) * np.sign(L / 2 - s)


def spline_eval(sp: dict, s, T):
    """The interpolants at the wrapped abscissa, in T: x, y, x', y', vel (last piece whose left break is <= it, Horner)."""
    L = T(sp["L"])
    br, co = sp["breaks"].astype(T), sp["coef"].astype(T)
    sm = mod(s, L)
    i = np.clip(np.searchsorted(sp["breaks"], sm.astype(np.float64), side="right") - 1, 0, br.size - 2)
    h = sm - br[i]
    a, b, c, e = (co[:, i, j] for j in range(4))
    val = a + h * (b + h * (c + h * e))
    d1 = b + h * (T(2.0) * c + T(3.0) * h * e)
    return {"x": val[0], "y": val[1], "dx": d1[0], "dy": d1[1], "vel": val[2]}


def table_lookup(tab, M: int, L, s, T):
    """track_lookup (lmpc_prep_kernels): periodic linear interpolation on a uniform table."""
    tab = tab.astype(T)
    u = np.fmod(s, L)
    u = np.where(u < 0, u + L, u)
    u = u / (L / T(M))
    fl = np.floor(u)
    fr = u - fl
    i0 = np.nan_to_num(fl.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64) % M
    i1 = np.where(i0 + 1 == M, 0, i0 + 1)
    return tab[i0] * (T(1.0) - fr) + tab[i1] * fr


def clamp(v, lo, hi):
    """std::clamp: a NaN passes through."""
    return np.where(v < lo, lo, np.where(hi < v, hi, v))


def pid_update(cfg: dict, pid: dict, e, T):
    """PidController::update for B cars: (cmd, new state); a NaN error returns NaN and leaves the state as it was."""
    dt = T(cfg["dt"])
    nan_e = np.isnan(e)
    last = np.where(nan_e, pid["last_error"], pid["error"])
    err = np.where(nan_e, pid["error"], e)
    integ = np.where(nan_e, pid["integral"], clamp(pid["integral"] + e * dt, T(cfg["min_i"]), T(cfg["max_i"])))
    cmd = e * T(cfg["k_p"]) + integ * T(cfg["k_i"]) + (err - last) / dt * T(cfg["k_d"])
    cmd = np.where(cmd <= T(cfg["min_cmd"]), T(cfg["min_cmd"]), np.where(cmd >= T(cfg["max_cmd"]), T(cfg["max_cmd"]), cmd))
    cmd = np.where(nan_e, T(np.nan), cmd)
    return cmd, {"integral": integ, "error": err, "last_error": last}


def zero_pid(B: int, T=np.float64) -> dict:
    return {k: np.zeros(B, dtype=T) for k in ("integral", "error", "last_error")}


def decide(veh, cfg: dict, trk: dict, x, pid: dict, vel_ref=None, speed_scale: float = 1.0, T=np.float64) -> dict:
    """One control decision for B cars.  x [B, 6]; pid: {"integral", "error", "last_error"} [B]; vel_ref [B] or None (the spline's
    velocity interpolant at the car's abscissa times speed_scale) -> {"u_out" [B, 3] = (FD, FB, STEER), "u_model" [B, 2], "pid" the
    state after the call (unchanged where flagged), "flags" [B], and the intermediates "la", "alpha", "cmd", "F"} in T."""
    x = np.asarray(x).astype(T)
    sp = trk["spline"]
    L = T(sp["L"])
    with np.errstate(all="ignore"):
        s, ey, epsi = x[:, 0], x[:, 1], x[:, 2]
        r = spline_eval(sp, s, T)
        yaw0 = np.arctan2(r["dy"], r["dx"])
        px, py = r["x"] - np.sin(yaw0) * ey, r["y"] + np.cos(yaw0) * ey
        dd = yaw0 + epsi
        yaw = np.arctan2(np.sin(dd), np.cos(dd)) + T(0.0)
        v = np.hypot(x[:, 3], x[:, 4])
        la = clamp(v * T(cfg["lookahead_speed_ratio"]), T(cfg["min_lookahead_distance"]), T(cfg["max_lookahead_distance"]))
        q = spline_eval(sp, mod(s + la, L), T)
        d = np.arctan2(q["y"] - py, q["x"] - px) - yaw
        alpha = np.arctan2(np.sin(d), np.cos(d))
        steer = clamp(np.arctan(T(2.0) * T(veh.l) * np.sin(alpha) / la), T(-veh.max_steer), T(veh.max_steer))
        vref = r["vel"] * T(speed_scale) if vel_ref is None else np.asarray(vel_ref).astype(T)
        cmd, new = pid_update(cfg, pid, vref - v, T)
        aero = T(0.5) * T(veh.rho) * T(veh.Af) * T(veh.cd) * v * v
        down = aero * (T(veh.cl_f) + T(veh.cl_r))
        roll = T(veh.fr) * (T(veh.m) * T(GRAVITY) + down)
        F = T(veh.m) * cmd + roll + aero
        lost = ~(np.abs(s) <= T(LAPS_MAX) * L)
        F, steer = np.where(lost, T(np.nan), F), np.where(lost, T(np.nan), steer)
        FD, FB = np.where(F > 0, F, T(0.0)), np.where(F > 0, T(0.0), F)
        ua = np.where(np.abs(FD) > np.abs(FB), FD, FB)
        u_out = np.stack([FD, FB, steer], axis=1)
        u_model = np.stack([ua * T(cfg["force_to_lon"]), steer], axis=1)
        fin = np.isfinite(u_out.astype(np.float64)).all(axis=1)
    keep = {k: np.where(fin, new[k], pid[k]) for k in new}
    return {"u_out": u_out, "u_model": u_model, "pid": keep, "flags": np.where(fin, 0, NOT_FINITE).astype(np.int32),
            "la": la, "alpha": alpha, "cmd": cmd, "F": F}


def plant(veh, trk: dict, x, u, dt_sim, n_sub: int, T):
    """lmpc_plant_kernel: n_sub sub-steps of dt_sim with the input held."""
    tab, L = trk["table"], T(trk["L"])
    x = x.copy()
    for _ in range(n_sub):
        x[:, 3] = np.where(np.abs(x[:, 3]) < T(1e-6), np.copysign(T(1e-6), x[:, 3]), x[:, 3])
        kap = table_lookup(tab["curvature"], tab["M"], L, x[:, 0], T)
        x = D.rk4(x, u, kap, T(dt_sim), veh)
        x[:, 0] = mod(x[:, 0], L)
    return x


def rollout(veh, cfg: dict, trk: dict, x0, pid: dict, periods: int, dt_sim: float, n_sub: int, speed_scale: float, T=np.float64,
            distance=None, worst_excess=None) -> dict:
    """lmpc_vanilla_rollout_batch for B cars: float64 {"x" [B, 6], "pid", "X_log" [B, 6, periods], "U_log" [B, 2, periods], "k_log"
    [B, periods], "distance" [B], "worst_excess" [B] (accumulated onto the arguments; 0 and -inf when None), "flags" [B]}."""
    x = np.asarray(x0).astype(T)
    B = x.shape[0]
    pid = {k: np.asarray(v).astype(T) for k, v in pid.items()}
    tab, L, M = trk["table"], T(trk["L"]), trk["table"]["M"]
    X_log, U_log, k_log = np.full((B, 6, periods), np.nan, dtype=T), np.full((B, 2, periods), np.nan, dtype=T), np.full((B, periods), np.nan, dtype=T)
    # the accumulators continue from the caller's values, sample by sample, as the kernel's do
    dist = (np.zeros(B) if distance is None else np.asarray(distance, dtype=np.float64)).astype(T)
    worst = (np.full(B, -np.inf) if worst_excess is None else np.asarray(worst_excess, dtype=np.float64)).astype(T)
    frozen = np.zeros(B, dtype=bool)
    half_b = T(veh.b) / T(2.0)
    with np.errstate(all="ignore"):
        for p in range(periods):
            o = decide(veh, cfg, trk, x, pid, None, speed_scale, T)
            live = ~frozen & (o["flags"] == 0)
            # (the plant of a car that is not live runs on a harmless stand-in; its result is discarded)
            xs_in = np.where(live[:, None], x, T(1.0))
            u = np.where(live[:, None], o["u_model"], T(0.0))
            xs = plant(veh, trk, xs_in, u, dt_sim, n_sub, T)
            live &= np.isfinite(xs.astype(np.float64)).all(axis=1)
            frozen = ~live
            X_log[live, :, p], U_log[live, :, p] = x[live], o["u_model"][live]
            k_log[live, p] = table_lookup(tab["curvature"], M, L, x[:, 0], T)[live]
            ds = xs[:, 0] - x[:, 0]
            dist += np.where(live, np.where(ds < -L / 2, ds + L, ds), T(0.0))
            bl, br = table_lookup(tab["bound_left"], M, L, x[:, 0], T), table_lookup(tab["bound_right"], M, L, x[:, 0], T)
            exc = np.maximum(xs[:, 1] + half_b - bl, br - (xs[:, 1] - half_b))
            worst = np.where(live, np.maximum(worst, exc), worst)
            x = np.where(live[:, None], xs, x)
            pid = {k: np.where(live, o["pid"][k], pid[k]) for k in pid}
    f64 = lambda a: np.asarray(a).astype(np.float64)   # noqa: E731
    return {"x": f64(x), "pid": {k: f64(v) for k, v in pid.items()}, "X_log": f64(X_log), "U_log": f64(U_log), "k_log": f64(k_log),
            "distance": f64(dist), "worst_excess": f64(worst), "flags": np.where(frozen, NOT_FINITE, 0).astype(np.int32)}


# ---- scenarios ----
def barc_config(**over) -> dict:
    """The BARC scenario's controller: lookahead 0.2 s of travel between 0.2 and 10 m (upstream's 1 m minimum cuts the corners of this
    15.6 m lap by more than a metre; at 0.3 s / 0.3 m ten of 67 bodies still cross an edge by up to 9 mm, so the lookahead was shrunk
    until tests/test_vanilla_reference.py's gate passed), a PI speed controller, controller dt = the control period."""
    c = dict(lookahead_speed_ratio=0.2, min_lookahead_distance=0.2, max_lookahead_distance=10.0, k_p=1.0, k_i=0.1, k_d=0.0,
             min_cmd=-5.0, max_cmd=5.0, min_i=-3.0, max_i=3.0, dt=0.025, force_to_lon=1e-3)
    c.update(over)
    return c


# name -> (track, vehicle, vehicle overrides, controller config, control period, n_sub, speed_scale, seed)
def _scenarios() -> dict:
    p2 = pkg().presets.vanilla_controller_2()
    return {
        # BARC, the issue's scenario
        "barc": ("barc", "barc", {}, barc_config(), 0.025, 2, 0.5, 31),
        # the synthetic 2.4 km track with the IAC car: lookahead 0.5 s of travel between 5 and 40 m, speeds 15 - 25 m/s
        "synthetic": ("synthetic", "iac", {}, barc_config(lookahead_speed_ratio=0.5, min_lookahead_distance=5.0, max_lookahead_distance=40.0),
                      0.025, 2, 0.5, 32),
        # vanilla_controller_2.param.yaml as shipped (k_d = 0.1: the first call's derivative kick e / dt; the PID's dt = 0.1 is not the
        # control period), on the track its 3 - 40 m lookahead is made for
        "preset2": ("synthetic", "iac", {}, p2, 0.025, 2, 0.5, 33),
        # force_to_lon = 1.0, upstream's chain as written: newtons arrive as kN, so a user of that chain has gains (and a rolling
        # resistance) a thousand times smaller -- the BARC scenario with k_p, k_i, the clamps and fr scaled by 1e-3
        "force1": ("barc", "barc", {"fr": 0.012e-3},
                   barc_config(k_p=1e-3, k_i=1e-4, min_cmd=-5e-3, max_cmd=5e-3, min_i=-3.0, max_i=3.0, force_to_lon=1.0), 0.025, 2, 0.5, 34),
    }


SCENARIOS = ("barc", "synthetic", "preset2", "force1")
_SC: dict = {}


def scenario(name: str, B: int = B_TEST) -> dict:
    """Starts: s uniform on the lap, |e_y| <= 0.1 (1 on the synthetic track), |e_psi| <= 0.1 (0.05), vx in [1, 2] (15 - 25), vy,
    omega = 0."""
    key = (name, B)
    if key not in _SC:
        tname, vname, over, cfg, dt, n_sub, scale, seed = _scenarios()[name]
        veh = copy.copy(OP.barc_vehicle() if vname == "barc" else OP.iac_vehicle())
        for k, v in over.items():
            setattr(veh, k, v)
        trk = track(tname)
        rng = np.random.default_rng(seed)
        big = tname != "barc"
        x0 = np.zeros((B, 6))
        x0[:, 0] = rng.uniform(0.0, trk["L"], B)
        # e_y within the bound above AND within half the room the body has at that abscissa (the BARC track is 0.19 m to its edge at
        # its narrowest and the body 0.14 m to its side: a start at 0.1 m there is outside before the controller has acted)
        s0 = x0[:, 0]
        room = np.minimum(trk["tr"].left_boundary(s0), -trk["tr"].right_boundary(s0)) - veh.b / 2.0
        x0[:, 1] = rng.uniform(-1.0, 1.0, B) * np.minimum(1.0 if big else 0.1, 0.5 * room)
        x0[:, 2] = rng.uniform(-1.0, 1.0, B) * (0.05 if big else 0.1)
        x0[:, 3] = rng.uniform(15.0, 25.0, B) if big else rng.uniform(1.0, 2.0, B)
        vel_ref = rng.uniform(15.0, 25.0, B) if big else rng.uniform(0.5, 2.5, B)
        _SC[key] = {"name": name, "track": tname, "trk": trk, "vehicle": vname, "veh_over": dict(over), "veh": veh, "cfg": dict(cfg),
                    "dt": dt, "n_sub": n_sub, "dt_sim": dt / n_sub, "speed_scale": scale, "x0": x0, "vel_ref": vel_ref}
    return _SC[key]


def err(got, ref) -> float:
    """The worst elementwise |d| / max(1, |reference|); a NaN or Inf on one side only is infinite, matching ones agree."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.shape != ref.shape:
        return float("inf")
    same = (np.isnan(got) & np.isnan(ref)) | (got == ref)
    with np.errstate(all="ignore"):
        e = np.where(same, 0.0, np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))
    return float(np.where(np.isfinite(e), e, np.inf).max()) if e.size else 0.0


ROLLOUT_KEYS = ("x", "X_log", "U_log", "k_log", "distance", "worst_excess")
PID_KEYS = ("integral", "error", "last_error")


def rollout_err(got: dict, ref: dict) -> float:
    return max([err(got[k], ref[k]) for k in ROLLOUT_KEYS] + [err(got["pid"][k], ref["pid"][k]) for k in PID_KEYS])


def decision_err(got: dict, ref: dict) -> float:
    return max([err(got[k], ref[k]) for k in ("u_out", "u_model")] + [err(got["pid"][k], ref["pid"][k]) for k in PID_KEYS])


_CACHE: dict = {}


def reference(name: str, what: str = "rollout", periods: int = PERIODS, T=np.float64, B: int = B_TEST):
    """The restatement on a scenario, computed once per process and shared (treat as read-only).  what: "rollout" (from a zero PID
    state), "decide" (vel_ref NULL) or "decide_ref" (the scenario's vel_ref)."""
    key = (name, what, periods if what == "rollout" else 0, T, B)
    if key not in _CACHE:
        sc = scenario(name, B)
        if what == "rollout":
            _CACHE[key] = rollout(sc["veh"], sc["cfg"], sc["trk"], sc["x0"], zero_pid(B), periods, sc["dt_sim"], sc["n_sub"], sc["speed_scale"], T)
        else:
            r = decide(sc["veh"], sc["cfg"], sc["trk"], sc["x0"], zero_pid(B, T), sc["vel_ref"] if what == "decide_ref" else None,
                       sc["speed_scale"], T)
            _CACHE[key] = {"u_out": r["u_out"].astype(np.float64), "u_model": r["u_model"].astype(np.float64),
                           "pid": {k: v.astype(np.float64) for k, v in r["pid"].items()}, "flags": r["flags"]}
    return _CACHE[key]
