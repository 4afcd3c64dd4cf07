"""What the car table (include/lmpc_hip_cars.h) costs, on 4096 BARC cars, N = 20 (profiles/fleet_plants.md is this script's output):

  --mode plant    lmpc_plant_kernel (Solver.plant_step) against lmpc_plant_cars_kernel (Solver.plant_step_cars, three kinds of
                  vehicle by b % 3): HIP events around `launches` launches enqueued behind a delay on the stream (the device's time, not the
                  host's rate of issue), alternating, `repeats` times.
  --mode advance  lmpc_fleet_loop_advance_batch alone, one prepared batch's tracking solution applied again and again: the kernel
                  without a table against its table instantiation, the same way.
  --mode period   closed_loop.run_lmpc_fleet_fused for `steps` periods (default 727: one discarded partial lap, one tracking lap,
                  one learning lap) without a table and with one -- every car on the handle's vehicle, so that both runs drive the
                  same laps and differ only in the kernel instantiation and its 26 loads per car --, alternating, `repeats` times;
                  a host clock around a final synchronise, as scratch/fleet_lmpc_fused_timing.py.
  --mode period --no-table   the run without a table only: what a build without the car table can run (LMPC_HIP_LIBRARY names
                  another build of the library; alternate processes for an A/B against it).

    python scratch/fleet_plants_timing.py --mode plant|advance|period [--cars 4096] [--repeats 3] [--launches 500] [--steps 727] [--no-table]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

N, DT = 20, 0.025


_PER_MS = [0.0]


def hold(ms):
    """A finite delay on the current stream (torch.cuda._sleep, calibrated once with two events), so that the launches timed behind it
    are all enqueued while it lasts and the events see the device's time for them, not the host's rate of issue."""
    if not _PER_MS[0]:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(20_000_000)
        b.record()
        torch.cuda.synchronize()
        _PER_MS[0] = 20_000_000 / a.elapsed_time(b)
    torch.cuda._sleep(int(ms * _PER_MS[0]))


def timed(launches, fn, hold_ms):
    """us per launch of `launches` calls of fn() behind a delay of hold_ms; also the host's time to issue them (ms), which must be
    below hold_ms for the figure to be the device's."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    hold(hold_ms)
    a.record()
    t0 = time.perf_counter()
    for j in range(launches):
        fn(j)
    host_ms = 1e3 * (time.perf_counter() - t0)
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / launches, host_ms


def kinds(pkg, n):
    base = pkg.presets.barc_vehicle()
    three = (base, dict(base, mu=0.7), dict(base, mu=0.8 * base["mu"], m=1.1 * base["m"]))
    return [three[b % 3] for b in range(n)]


def plant(pkg, B, repeats, launches):
    s = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
    tr = pkg.workloads.synthetic_track("barc")
    trk = s.device_track(tr)
    x, u = pkg.workloads.sample_initial_states("barc", B, tr["L"], [-0.01, -0.3], [0.01, 0.3], seed=0)
    x0, ua = torch.as_tensor(x.T.copy(), device="cuda"), torch.as_tensor(u.T.copy(), device="cuda")
    s.set_car_vehicles(kinds(pkg, B))
    calls = {"lmpc_plant_kernel": s.plant_step, "lmpc_plant_cars_kernel": s.plant_step_cars}
    us = {k: [] for k in calls}
    for r in range(repeats + 1):          # (repeat 0 is the warm-up)
        for name, fn in calls.items():
            xs = x0.clone()
            t, host_ms = timed(launches, lambda j: fn(trk, xs, ua, DT / 2, 2), 60.0)
            assert host_ms < 60.0, host_ms
            if r:
                us[name].append(t)
    for name, v in us.items():
        print("%-24s %d cars, n_sub 2: %s us per launch (median %.2f, spread %.1f %%)"
              % (name, B, " ".join("%.2f" % t for t in v), np.median(v), 100 * (max(v) - min(v)) / np.median(v)))
    s.close()


def period(pkg, B, repeats, steps, no_table):
    tr = pkg.workloads.synthetic_track("barc")
    rng = np.random.default_rng(0)
    x0 = np.stack([np.full(B, 0.5), rng.uniform(-0.05, 0.05, B), np.zeros(B), np.full(B, 2.0), np.zeros(B), np.zeros(B)])
    x0, u0 = torch.as_tensor(x0, device="cuda"), torch.zeros((2, B), dtype=torch.float64, device="cuda")

    def one(table, max_steps):
        tracker = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
        learner = pkg.Solver(pkg.presets.barc_lmpc(N, 3), pkg.presets.barc_vehicle(), device=0)
        kw = dict(warm_laps=1, learn_laps=1, warm_speed_scale=0.7, max_steps=max_steps, poll=1)
        if table:
            kw["plants"] = [pkg.presets.barc_vehicle()] * B
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pkg.closed_loop.run_lmpc_fleet_fused(tracker, learner, tr, x0, u0, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        tracker.close(), learner.close()
        return res, wall

    one(False, 20)      # warm-up: lazy initialisation, allocator
    runs = (False,) if no_table else (False, True)
    if not no_table:    # what a run with a table pays once, inside its timed region: B structs filled in Python, one blocking upload
        sv = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
        for what, fleet in (("B distinct dicts", [pkg.presets.barc_vehicle() for _ in range(B)]), ("one dict B times", [pkg.presets.barc_vehicle()] * B)):
            t0 = time.perf_counter()
            sv.set_car_vehicles(fleet)
            t1 = time.perf_counter()
            sv.set_car_vehicles(None)
            print("set_car_vehicles of %d cars, %s, once per run: %.1f ms (clearing it: %.2f ms)" % (B, what, 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)))
        sv.close()
    rate = {t: [] for t in runs}
    for r in range(repeats):
        for t in runs:
            res, wall = one(t, steps)
            rate[t].append(res["steps"] / wall)
            print("repeat %d %-10s %5d periods %7.3f s %8.1f periods/s, failed solves %d"
                  % (r, "table" if t else "no table", res["steps"], wall, res["steps"] / wall, int(res["n_fail"].sum())), flush=True)
    for t, v in rate.items():
        print("%-10s median %.1f periods/s, spread %.2f %%" % ("table" if t else "no table", np.median(v), 100 * (max(v) - min(v)) / np.median(v)))


def advance(pkg, B, repeats, launches):
    """lmpc_fleet_loop_advance_batch alone, with and without a table: the tracking controller's solution of one prepared batch, applied
    `launches` times back to back (the references shift on, the plan stays: the call moves plans, it does not judge them)."""
    tr = pkg.workloads.synthetic_track("barc")
    tracker = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
    learner = pkg.Solver(pkg.presets.barc_lmpc(N, 3), pkg.presets.barc_vehicle(), device=0)
    trk = tracker.device_track(tr)
    rng = np.random.default_rng(0)
    x0 = np.stack([np.full(B, 0.5), rng.uniform(-0.05, 0.05, B), np.zeros(B), np.full(B, 2.0), np.zeros(B), np.zeros(B)])
    x0, u0 = torch.as_tensor(x0, device="cuda"), torch.zeros((2, B), dtype=torch.float64, device="cuda")
    inp0 = tracker.prepare(trk, x0, DT, speed_scale=0.7)
    inp0["x_ic"], inp0["u_ic"] = x0, u0
    sol = tracker.solve(inp0)
    us = {False: [], True: []}
    for r in range(repeats + 1):          # (repeat 0 is the warm-up)
        for table in (False, True):
            learner.fleet_ss_create(B, 1024)
            learner.set_car_vehicles([pkg.presets.barc_vehicle()] * B if table else None)
            state = learner.fleet_loop_state(B, 4)
            inp = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in inp0.items()}
            x, u = x0.clone(), u0.clone()
            t, host_ms = timed(launches, lambda j: learner.fleet_loop_advance(trk, inp, sol, None, x, u, state, dt=DT, dt_sim=DT / 2, n_sub=2, t=DT * j,
                                                                              speed_scale=(0.7, 1.0), warm_laps=1, learn_laps=1, switch_phase=False), 100.0)
            assert host_ms < 100.0, host_ms
            if r:
                us[table].append(t)
    learner.set_car_vehicles(None)
    for table, v in us.items():
        print("%s %d cars: %s us per launch (median %.2f, spread %.1f %%)"
              % ("lmpc_fleet_loop_kernel<true>, table   " if table else "lmpc_fleet_loop_kernel<false>, no table", B, " ".join("%.2f" % t for t in v), np.median(v), 100 * (max(v) - min(v)) / np.median(v)))
    tracker.close(), learner.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("plant", "period", "advance"), required=True)
    ap.add_argument("--cars", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--steps", type=int, default=727)
    ap.add_argument("--no-table", action="store_true")
    a = ap.parse_args()
    pkg = load_package()
    print("library:", pkg.capi.library_path())
    if a.mode == "plant":
        plant(pkg, a.cars, a.repeats, a.launches)
    elif a.mode == "advance":
        advance(pkg, a.cars, a.repeats, min(a.launches, 200))
    else:
        period(pkg, a.cars, a.repeats, a.steps, a.no_table)


if __name__ == "__main__":
    main()
