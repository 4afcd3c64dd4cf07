"""Timing of the fleet's first laps with the batched vanilla controller (profiles/vanilla_rollout.md takes this script's output).

B BARC cars of the "barc" scenario of tests/vanilla_cases.py (the tested controller, track and starts, generated for B cars) driven for
`--periods` control periods, wall clock from the call to a device synchronisation behind it, `--reps` alternating repetitions after
one warm-up of each, median (min .. max):
  (f) closed_loop.run_vanilla(fused=True, chunk=64): ceil(periods / 64) launches of lmpc_vanilla_rollout_batch
  (u) closed_loop.run_vanilla(fused=False): one lmpc_vanilla_solve_batch, one lmpc_plant_step_batch and the bookkeeping in torch per period
  (m) the parent's way to the same laps, as context: closed_loop.run with the tracking MPC (N = 20) on the same cars at the same
      speed scale -- linearise, QP solve and lmpc_loop_advance_batch per period
(m) is another controller (a QP with bounds, a 20-knot plan): the figure is what the laps cost before, not a like-for-like kernel
comparison.  Logs are on in (f) and (u): they are what the recorder needs.

    python scratch/vanilla_timing.py [--batch 4096] [--periods 480] [--reps 5] [--out FILE.md]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--periods", type=int, default=480)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = load_package()
    B, P = a.batch, a.periods
    sc = VC.scenario("barc", B=B)
    solver = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    spline, table = solver.spline_track(sc["trk"]["spline"]), solver.device_track(sc["trk"]["table"])
    x0 = torch.as_tensor(np.ascontiguousarray(sc["x0"].T), device=solver.device)
    u0 = torch.zeros((2, B), dtype=torch.float64, device=solver.device)
    solver.vanilla_create(sc["cfg"], B)
    last = {}

    def call(key):
        if key == "m":
            last[key] = pkg.closed_loop.run(solver, table, x0, u0, P, dt=sc["dt"], n_sub=sc["n_sub"], speed_scale=sc["speed_scale"])
        else:
            solver.vanilla_reset(B)
            last[key] = pkg.closed_loop.run_vanilla(solver, table, spline, x0, P, dt=sc["dt"], n_sub=sc["n_sub"], speed_scale=sc["speed_scale"],
                                                    chunk=64, fused=key == "f")

    t = {key: [] for key in "fum"}
    for i in range(-1, a.reps):
        for key in "fum":
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(key)
            torch.cuda.synchronize()
            if i >= 0:
                t[key].append(time.perf_counter() - t0)
    L = sc["trk"]["L"]
    names = {"f": "(f) run_vanilla fused, chunk 64", "u": "(u) run_vanilla unfused", "m": "(m) closed_loop.run, tracking MPC N = 20"}
    lines = ["%d BARC cars x %d periods, %d repetitions" % (B, P, a.reps), "",
             "| path | wall clock ms, median (min .. max) | M car-steps/s | launches per period | laps driven, mean | cars flagged / failed solves |",
             "|---|---|---|---|---|---|"]
    for key in "fum":
        ms = np.array(t[key]) * 1e3
        r = last[key]
        laps = float(r["distance"].mean()) / L
        bad = int((r["flags"] != 0).sum()) if key != "m" else int(r["n_fail"].sum())
        launches = {"f": "%.3f" % (-(-P // 64) / P), "u": "2 + ~30 element-wise", "m": "3"}[key]
        lines.append("| %s | %.1f (%.1f .. %.1f) | %.2f | %s | %.2f | %d |" % (names[key], np.median(ms), ms.min(), ms.max(), B * P / np.median(ms) / 1e3,
                                                                             launches, laps, bad))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
