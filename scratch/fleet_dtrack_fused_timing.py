"""What the fused fleet LMPC period on four-wheel cars costs and does (profiles/fleet_dtrack_fused.md is this script's output), on
4096 BARC cars, N = 20, n_sub = 2, by the method of scratch/fleet_plants_timing.py: HIP events around launches enqueued behind a
delay on the stream (the device's time, not the host's rate of issue), alternating repeats, the spread stated.

  --mode advance     lmpc_fleet_loop_advance_batch with a car table against lmpc_fleet_loop_advance_dtrack_batch, one prepared batch's
                     tracking solution applied again and again (three kinds of vehicle by b % 3 in both tables).
  --mode replaced    the kernels the double-track instantiation replaces in closed_loop.run_lmpc_fleet(plants_dt=), each timed the
                     same way in the same process: the two shifts (Solver.shift on the tracker and on the learner), the plant step
                     (Solver.plant_step_dtrack), the record (fleet_ss_record) and the stats (fleet_ss_stats); and their sum.
  --mode period      closed_loop.run_lmpc_fleet_fused(plants_dt=) against closed_loop.run_lmpc_fleet(plants_dt=) over the same
                     `steps` periods (default 200), alternating, a host clock around a final synchronise.
  --mode experiment  64 cars, the three kinds of tests/test_gpu_fleet_dtrack.py, one warm lap by the vanilla controller (warmup=)
                     and one learning lap with the per-car regression on: laps closed per car, failed solves, worst boundary excess,
                     lap times.  Recorded, not judged.

    python scratch/fleet_dtrack_fused_timing.py --mode advance|replaced|period|experiment [--cars 4096] [--repeats 3] [--launches 200] [--steps 200]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package  # noqa: E402
from fleet_plants_timing import kinds, timed  # noqa: E402  (the same delay and the same events)

import vanilla_cases as VC  # noqa: E402
import vanilla_fleet_cases as FC  # noqa: E402

N, DT = 20, 0.025


def report(name, v):
    print("%-46s %s us per launch (median %.2f, spread %.1f %%)" % (name, " ".join("%.2f" % t for t in v), np.median(v), 100 * (max(v) - min(v)) / np.median(v)))
    return float(np.median(v))


def batch(pkg, B):
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
    torch.cuda.synchronize()
    return tr, tracker, learner, trk, x0, u0, inp0, sol


def advance(pkg, B, repeats, launches):
    tr, tracker, learner, trk, x0, u0, inp0, sol = batch(pkg, B)
    cars, dtrack = kinds(pkg, B), FC.dtrack_vehicles(pkg, B)
    us = {False: [], True: []}
    for r in range(repeats + 1):          # (repeat 0 is the warm-up)
        for dt_ in (False, True):
            learner.fleet_ss_create(B, 1024)
            learner.set_car_vehicles(None if dt_ else cars)
            learner.set_dtrack_vehicles(dtrack if dt_ else None)
            state = learner.fleet_loop_state(B, 4)
            inp = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in inp0.items()}
            x, u = x0.clone(), u0.clone()
            t, host_ms = timed(launches, lambda j: learner.fleet_loop_advance(trk, inp, sol, None, x, u, state, dt=DT, dt_sim=DT / 2, n_sub=2, t=DT * j,
                                                                              speed_scale=(0.7, 1.0), warm_laps=1, learn_laps=1, switch_phase=False,
                                                                              dtrack=dt_), 100.0)
            assert host_ms < 100.0, host_ms
            assert bool(torch.isfinite(x).all())
            if r:
                us[dt_].append(t)
    learner.set_car_vehicles(None), learner.set_dtrack_vehicles(None)
    a = report("lmpc_fleet_loop_kernel, car table, %d cars" % B, us[False])
    b = report("lmpc_fleet_loop_kernel, double-track table, %d cars" % B, us[True])
    print("double-track minus car table: %.2f us" % (b - a))
    tracker.close(), learner.close()


def replaced(pkg, B, repeats, launches):
    tr, tracker, learner, trk, x0, u0, inp0, sol = batch(pkg, B)
    L = float(tr["L"])
    learner.set_dtrack_vehicles(FC.dtrack_vehicles(pkg, B))
    u_apply = sol["U_optm"][:, 0, :].contiguous()
    kap = torch.zeros(B, dtype=torch.float64, device="cuda")
    stats = {"laps_in_ring": torch.zeros(B, dtype=torch.int32, device="cuda"), "lap_count": torch.zeros(B, dtype=torch.int32, device="cuda"),
             "n_dropped": torch.zeros(B, dtype=torch.int32, device="cuda"), "last_lap_time": torch.zeros(B, dtype=torch.float64, device="cuda")}
    xs = x0.clone()
    calls = {
        "shift, tracker (lmpc_shift_batch)": lambda j: tracker.shift(trk, inp0, sol, DT, speed_scale=0.7),
        "shift, learner (lmpc_shift_batch)": lambda j: learner.shift(trk, inp0, sol, DT, speed_scale=1.0),
        "plant (lmpc_plant_dtrack_kernel)": lambda j: learner.plant_step_dtrack(trk, xs, u_apply, DT / 2, 2),
        "record (lmpc_fleet_ss_record_batch)": lambda j: learner.fleet_ss_record(xs, u_apply, kap, DT * j, L),
        "stats (lmpc_fleet_ss_stats)": lambda j: learner.fleet_ss_stats(B, out=stats),
    }
    us = {k: [] for k in calls}
    for r in range(repeats + 1):          # (repeat 0 is the warm-up)
        for name, fn in calls.items():
            learner.fleet_ss_create(B, 1024)
            xs.copy_(x0)
            t, host_ms = timed(launches, fn, 100.0)
            assert host_ms < 100.0, (name, host_ms)
            if r:
                us[name].append(t)
    total = sum(report(name, v) for name, v in us.items())
    sums = [sum(us[k][i] for k in us) for i in range(repeats)]
    print("sum of the five: median of medians %.2f us; per repeat %s (spread %.1f %%)"
          % (total, " ".join("%.2f" % s for s in sums), 100 * (max(sums) - min(sums)) / np.median(sums)))
    learner.set_dtrack_vehicles(None)
    tracker.close(), learner.close()


def period(pkg, B, repeats, steps):
    tr = pkg.workloads.synthetic_track("barc")
    rng = np.random.default_rng(0)
    x0 = np.stack([np.full(B, 0.5), rng.uniform(-0.05, 0.05, B), np.zeros(B), np.full(B, 2.0), np.zeros(B), np.zeros(B)])
    x0, u0 = torch.as_tensor(x0, device="cuda"), torch.zeros((2, B), dtype=torch.float64, device="cuda")
    plants_dt = FC.dtrack_vehicles(pkg, B)

    def one(fused, max_steps):
        tracker = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
        learner = pkg.Solver(pkg.presets.barc_lmpc(N, 3), pkg.presets.barc_vehicle(), device=0)
        fn = pkg.closed_loop.run_lmpc_fleet_fused if fused else pkg.closed_loop.run_lmpc_fleet
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn(tracker, learner, tr, x0, u0, max_steps=max_steps, plants_dt=plants_dt, **({"poll": 1} if fused else {}))
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        tracker.close(), learner.close()
        return res, wall

    for fused in (True, False):
        one(fused, 10)      # warm-up: lazy initialisation, allocator
    rate = {True: [], False: []}
    for r in range(repeats):
        for fused in (True, False):
            res, wall = one(fused, steps)
            rate[fused].append(res["steps"] / wall)
            print("repeat %d %-8s %5d periods %7.3f s %8.1f periods/s, failed solves %d"
                  % (r, "fused" if fused else "unfused", res["steps"], wall, res["steps"] / wall, int(res["n_fail"].sum())), flush=True)
    for fused, v in rate.items():
        print("%-8s median %.1f periods/s, spread %.2f %%" % ("fused" if fused else "unfused", np.median(v), 100 * (max(v) - min(v)) / np.median(v)))
    print("fused / unfused: %.2f" % (np.median(rate[True]) / np.median(rate[False])))


def experiment(pkg, B, steps):
    sc = VC.scenario("barc", B)
    base = pkg.presets.barc_double_track()
    three = (base, dict(base, mu=0.7), dict(base, kroll_f=0.35, Ef=0.6, Er=0.6))      # tests/test_gpu_fleet_dtrack.py's kinds
    plants_dt = [three[b % 3] for b in range(B)]
    tracker = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
    learner = pkg.Solver(pkg.presets.barc_lmpc(N, 3), pkg.presets.barc_vehicle(), device=0)
    warmup = dict(config=sc["cfg"], spline=sc["trk"]["spline"], speed_scale=sc["speed_scale"], chunk=64, max_periods=2048)
    x0 = torch.as_tensor(np.ascontiguousarray(sc["x0"].T), device="cuda")
    u0 = torch.zeros((2, B), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = pkg.closed_loop.run_lmpc_fleet_fused(tracker, learner, sc["trk"]["table"], x0, u0, warm_laps=1, learn_laps=1, dt=sc["dt"], n_sub=sc["n_sub"],
                                               max_steps=steps, poll=8, regression={"dist_max": 0.6}, plants_dt=plants_dt, warmup=warmup)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    w = res["warmup"]
    nf, exc = res["n_fail"].cpu().numpy(), res["worst_excess"].cpu().numpy()
    print("%d cars, warm-up %d periods (lap_count after it: min %d, max %d), loop %d periods (%s), %.1f s wall"
          % (B, w["periods"], w["lap_count"].min(), w["lap_count"].max(), res["steps"], "ended on its own" if res["steps"] < steps else "stopped at max_steps", wall))
    print("finite final states: %s; laps dropped for their length: %d" % (bool(torch.isfinite(res["x"]).all()), int(res["n_dropped"].sum())))
    for kind in range(3):
        cars = np.arange(B)[np.arange(B) % 3 == kind]
        laps = [len(res["lap_times"][b]) for b in cars]
        lrn = [t for b in cars for t, k in zip(res["lap_times"][b], res["lap_kind"][b]) if k == "lmpc"]
        trk_ = [t for b in cars for t, k in zip(res["lap_times"][b], res["lap_kind"][b]) if k == "tracking"]
        fmt = lambda v: ("%.2f .. %.2f s (%d)" % (min(v), max(v), len(v))) if v else "none"   # noqa: E731
        print("kind %d (%d cars): laps closed after the warm-up per car %d .. %d; learning laps %s; tracking laps %s; failed solves per car "
              "%d .. %d (median %d); worst boundary excess %.3f .. %.3f m (median %.3f)"
              % (kind, len(cars), min(laps), max(laps), fmt(lrn), fmt(trk_), nf[cars].min(), nf[cars].max(), int(np.median(nf[cars])),
                 exc[cars].min(), exc[cars].max(), float(np.median(exc[cars]))))
    tracker.close(), learner.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("advance", "replaced", "period", "experiment"), required=True)
    ap.add_argument("--cars", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=None)
    a = ap.parse_args()
    pkg = load_package()
    print("library:", pkg.capi.library_path().name, "| mode", a.mode)
    if a.mode == "advance":
        advance(pkg, a.cars or 4096, a.repeats, a.launches)
    elif a.mode == "replaced":
        replaced(pkg, a.cars or 4096, a.repeats, a.launches)
    elif a.mode == "period":
        period(pkg, a.cars or 4096, a.repeats, a.steps or 200)
    else:
        experiment(pkg, a.cars or 64, a.steps or 1500)


if __name__ == "__main__":
    main()
