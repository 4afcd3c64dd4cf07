"""What one launch of the double-track plant step costs (profiles/dtrack_plant.md is this script's output): lmpc_plant_dtrack_kernel
(Solver.plant_step_dtrack, three kinds of four-wheel car by b % 3, gamma_y written) beside lmpc_plant_cars_kernel
(Solver.plant_step_cars, three kinds of single-track car) and lmpc_plant_kernel (Solver.plant_step) on the same states, 4096 BARC
cars, n_sub = 2.  scratch/fleet_plants_timing.py's method: HIP events around `launches` launches enqueued behind a delay on the
stream (the device's time, not the host's rate of issue), the three kernels alternating, `repeats` times after one warm-up round.

    python scratch/dtrack_plant_timing.py [--cars 4096] [--repeats 5] [--launches 500]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scratch"))
from __graft_entry__ import load_package  # noqa: E402
from fleet_plants_timing import DT, N, kinds, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cars", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=500)
    a = ap.parse_args()
    pkg = load_package()
    B = a.cars
    s = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
    tr = pkg.workloads.synthetic_track("barc")
    trk = s.device_track(tr)
    x, u = pkg.workloads.sample_initial_states("barc", B, tr["L"], [-0.01, -0.3], [0.01, 0.3], seed=0)
    x0, ua = torch.as_tensor(x.T.copy(), device="cuda"), torch.as_tensor(u.T.copy(), device="cuda")
    gam = torch.zeros(B, dtype=torch.float64, device="cuda")
    s.set_car_vehicles(kinds(pkg, B))
    base = pkg.presets.barc_double_track()
    three = (base, dict(base, mu=0.7), dict(base, kroll_f=0.35, Ef=0.6, Er=0.6))
    s.set_dtrack_vehicles([three[b % 3] for b in range(B)])
    calls = {"lmpc_plant_kernel": lambda xs: s.plant_step(trk, xs, ua, DT / 2, 2),
             "lmpc_plant_cars_kernel": lambda xs: s.plant_step_cars(trk, xs, ua, DT / 2, 2),
             "lmpc_plant_dtrack_kernel": lambda xs: s.plant_step_dtrack(trk, xs, ua, DT / 2, 2, gam)}
    us = {k: [] for k in calls}
    for r in range(a.repeats + 1):          # (repeat 0 is the warm-up)
        for name, fn in calls.items():
            xs = x0.clone()
            t, host_ms = timed(a.launches, lambda j: fn(xs), 60.0)
            assert host_ms < 60.0, host_ms
            if r == 1:
                print("%-26s after %d launches with the inputs held: %d of %d cars finite" % (name, a.launches, int(torch.isfinite(xs).all(dim=0).sum()), B))
            if r:
                us[name].append(t)
    for name, v in us.items():
        print("%-26s %d cars, n_sub 2: %s us per launch (median %.2f, spread %.1f %%)"
              % (name, B, " ".join("%.2f" % t for t in v), np.median(v), 100 * (max(v) - min(v)) / np.median(v)))
    s.close()


if __name__ == "__main__":
    main()
