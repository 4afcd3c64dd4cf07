"""Timing of the vanilla rollout of a fleet, lmpc_vanilla_rollout_fleet_batch (profiles/vanilla_fleet.md takes this script's output).

B BARC cars of the "barc" scenario of tests/vanilla_cases.py driven for `--periods` control periods and recorded into the fleet safe
set, wall clock from the call to a device synchronisation behind it, `--reps` alternating repetitions after one warm-up of each,
median (min .. max); the store and the PID state are reset outside the clock.
  handle: (f) Solver.vanilla_rollout_fleet(plant="handle", record="applied") in chunks of 64
          (p) closed_loop.run_vanilla(fused=True, fleet_record=True), chunk 64: the same rings by one rollout launch per chunk, the logs
              written to memory and one lmpc_fleet_ss_record_batch per period reading them back
  cars / dtrack: (f) the fused call with that plant, record="arrived"
                 (p) per period lmpc_vanilla_solve_batch, lmpc_plant_step_cars_batch / lmpc_plant_step_dtrack_batch, the curvature
                     lookup in torch and lmpc_fleet_ss_record_batch: the only way to the same laps without the fused call
  warm phase (context, other laps): closed_loop.warm_up_vanilla to `warm_laps` laps in every ring, against the tracking MPC's warm laps
          (closed_loop.run_lmpc_fleet_fused with the phase switch out of reach (warm_laps = 100), poll 16) for --track-periods periods

    python scratch/vanilla_fleet_timing.py [--batch 4096] [--periods 1024] [--reps 5] [--track-periods 1100] [--out FILE.md]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
from __graft_entry__ import load_package  # noqa: E402

import vanilla_cases as VC  # noqa: E402
import vanilla_fleet_cases as FC  # noqa: E402


def timed(calls: dict, reps: int, before):
    """Alternating repetitions after one warm-up of each: {key: [seconds]}."""
    t = {key: [] for key in calls}
    for i in range(-1, reps):
        for key, fn in calls.items():
            before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= 0:
                t[key].append(time.perf_counter() - t0)
    return t


def fmt(sec):
    ms = np.array(sec) * 1e3
    return "%.1f (%.1f .. %.1f), spread %.1f %%" % (np.median(ms), ms.min(), ms.max(), 100.0 * (ms.max() - ms.min()) / np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--periods", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--track-periods", type=int, default=1100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = load_package()
    B, P = a.batch, a.periods
    sc = VC.scenario("barc", B=B)
    dt, n_sub, scale, L = sc["dt"], sc["n_sub"], sc["speed_scale"], float(sc["trk"]["L"])
    solver = pkg.Solver(pkg.presets.barc_lmpc(20, 3), pkg.presets.barc_vehicle(), device=0)
    spline, table = solver.spline_track(sc["trk"]["spline"]), solver.device_track(sc["trk"]["table"])
    x0 = torch.as_tensor(np.ascontiguousarray(sc["x0"].T), device=solver.device)
    u0 = torch.zeros((2, B), dtype=torch.float64, device=solver.device)
    solver.vanilla_create(sc["cfg"], B)
    solver.fleet_ss_create(B, 512)
    rings = {}

    def before():
        solver.vanilla_reset(B)
        solver.fleet_ss_reset()

    def fused(plant, record):
        x, up = x0.clone(), u0.clone()
        for p0 in range(0, P, 64):
            solver.vanilla_rollout_fleet(spline, table, x, min(64, P - p0), dt / n_sub, n_sub, plant=plant, record=record, period0=p0, dt=dt,
                                         u_prev=up, speed_scale=scale)
        rings[plant, "f"] = solver.fleet_ss_stats(B)

    def parent_handle():
        pkg.closed_loop.run_vanilla(solver, table, spline, x0, P, dt=dt, n_sub=n_sub, speed_scale=scale, chunk=64, fused=True, fleet_record=True)
        rings["handle", "p"] = solver.fleet_ss_stats(B)

    def per_period(plant):
        x, up, out = x0.clone(), u0.clone(), None
        step = solver.plant_step_cars if plant == "cars" else solver.plant_step_dtrack
        for p in range(P):
            out = solver.vanilla_solve(spline, x, None, speed_scale=scale, out=out)
            kap = pkg.closed_loop._table_lookup(table["curvature"], int(table["M"]), L, x[0])
            solver.fleet_ss_record(x, up, kap, p * dt, L)
            step(table, x, out["u_model"], dt / n_sub, n_sub)
            up.copy_(out["u_model"])
        rings[plant, "p"] = solver.fleet_ss_stats(B)

    lines = ["%d BARC cars x %d periods, chunk 64, %d alternating repetitions after one warm-up; wall clock ms, median (min .. max)" % (B, P, a.reps), "",
             "| plant | fused call | without it | ratio of medians | same lap counts |", "|---|---|---|---|---|"]
    for plant in FC.PLANTS:
        solver.set_car_vehicles(FC.car_vehicle_dicts(pkg, sc, B) if plant == "cars" else None)
        solver.set_dtrack_vehicles(FC.dtrack_vehicles(pkg, B) if plant == "dtrack" else None)
        record = "applied" if plant == "handle" else "arrived"
        calls = {"f": lambda: fused(plant, record), "p": parent_handle if plant == "handle" else (lambda: per_period(plant))}
        t = timed(calls, a.reps, before)
        same = all(torch.equal(rings[plant, "f"][k], rings[plant, "p"][k]) for k in ("laps_in_ring", "lap_count", "n_dropped"))
        lines.append("| %s, %s | %s | %s | %.1fx | %s (laps in ring %d .. %d) |"
                     % (plant, record, fmt(t["f"]), fmt(t["p"]), np.median(t["p"]) / np.median(t["f"]), same,
                        int(rings[plant, "f"]["laps_in_ring"].min()), int(rings[plant, "f"]["laps_in_ring"].max())))
    solver.set_car_vehicles(None)
    solver.set_dtrack_vehicles(None)

    # the warm phase of the fleet experiment: pure pursuit at the scenario's speed scale against the tracking MPC at 0.7 (other laps)
    tracker = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    seen = {}

    def warm_vanilla():
        seen["v"] = pkg.closed_loop.warm_up_vanilla(solver, table, spline, x0, u0, 2, dt=dt, n_sub=n_sub, speed_scale=scale, chunk=64)

    def warm_tracking():
        seen["t"] = pkg.closed_loop.run_lmpc_fleet_fused(tracker, solver, table, x0, u0, warm_laps=100, learn_laps=1, dt=dt, n_sub=n_sub,
                                                         max_steps=a.track_periods, max_pts_per_lap=512, poll=16)

    def before_warm():
        solver.vanilla_create(sc["cfg"], B)
        solver.fleet_ss_create(B, 512)

    t = timed({"v": warm_vanilla, "t": warm_tracking}, min(a.reps, 3), before_warm)
    lines += ["", "warm phase to 2 laps in every ring (context: the laps differ), wall clock ms:", "",
              "| way | periods | ms | laps in ring at the end | cars flagged / failed solves | worst boundary excess, m |", "|---|---|---|---|---|---|",
              "| warm_up_vanilla, chunk 64, speed scale %.2f | %d | %s | %d .. %d | %d | %.3f |"
              % (scale, seen["v"]["periods"], fmt(t["v"]), int(seen["v"]["laps_in_ring"].min()), int(seen["v"]["laps_in_ring"].max()),
                 int((seen["v"]["flags"] != 0).sum()), float(seen["v"]["worst_excess"].max())),
              "| tracking MPC N = 20 at 0.7, run_lmpc_fleet_fused poll 16 | %d | %s | %d .. %d | %d | %.3f |"
              % (seen["t"]["steps"], fmt(t["t"]), int(seen["t"]["laps_in_ring"].min()), int(seen["t"]["laps_in_ring"].max()),
                 int(seen["t"]["n_fail"].sum()), float(seen["t"]["worst_excess"].max()))]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
