"""Timing of the spline-track kernels for profiles/track_project.md: unseeded and seeded projection and frenet_to_global of an N = 20
plan at 4096 and 32768 poses on both tracks of tests/track_cases.py (device events, median of 200 calls after 20 warm-up calls),
run_global's period beside run's, and the C++-equivalent host projection rate for context (Python class, a few poses).
usage: python scratch/track_timing.py [out_file]"""
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package  # noqa: E402
import track_cases as TC  # noqa: E402

pkg = load_package()
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout


def say(*a):
    print(*a, file=out, flush=True)
    if out is not sys.stdout:
        print(*a, flush=True)


def event_median(fn, calls=200, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


solver = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
say("device", torch.cuda.get_device_name(0))
for name in ("barc", "synthetic"):
    tr = pkg.racing_trajectory.RacingTrajectory(TC.table(name))
    dev = solver.spline_track(tr)
    for B in (4096, 32768):
        frenet, pose, _ = TC.poses(tr, B)
        pose_d = torch.as_tensor(pose, device="cuda")
        s0 = torch.as_tensor(frenet[0] + np.random.default_rng(5).uniform(-1, 1, B) * dev.h_bar, device="cuda")
        buf = (torch.empty((3, B), dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"))
        X = torch.zeros((6, 20, B), dtype=torch.float64, device="cuda")
        X[:3] = torch.as_tensor(frenet, device="cuda")[:, None, :]
        pg = torch.empty((3, 20, B), dtype=torch.float64, device="cuda")
        for label, fn in (("project unseeded", lambda: solver.global_to_frenet(dev, pose_d, out=buf)),
                          ("project seeded", lambda: solver.global_to_frenet(dev, pose_d, s0=s0, out=buf)),
                          ("frenet_to_global N=20", lambda: solver.frenet_to_global(dev, X, out=pg))):
            med, lo, hi = event_median(fn)
            say("%-9s B %5d  %-22s median %7.1f us  (min %.1f, max %.1f)" % (name, B, label, med, lo, hi))
    # host projection for context: the Python class on one thread
    frenet, pose, _ = TC.poses(tr, 64)
    t0 = time.perf_counter()
    for b in range(64):
        tr.global_to_frenet(*[float(v) for v in pose[:, b]])
    say("%-9s host Python global_to_frenet: %.2f ms per pose" % (name, (time.perf_counter() - t0) / 64 * 1e3))

# the closed loop: run against run_global, 4096 cars on the BARC track, eager launches, wall clock over 200 periods
tr = pkg.racing_trajectory.RacingTrajectory(TC.BARC)
dev, tab = solver.spline_track(tr), tr.to_track_table(1024)
B = 4096
rng = np.random.default_rng(1)
s0 = rng.uniform(0, tab["L"], B)
x0 = torch.as_tensor(np.stack([s0, rng.uniform(-0.05, 0.05, B), np.zeros(B), 0.8 * np.interp(s0, np.arange(1024) * tab["L"] / 1024, tab["vel"]),
                               np.zeros(B), np.zeros(B)]), device="cuda")
u0 = torch.zeros((2, B), dtype=torch.float64, device="cuda")
for label, fn in (("run", lambda: pkg.closed_loop.run(solver, tab, x0, u0, steps=200)),
                  ("run_global", lambda: pkg.closed_loop.run_global(solver, tab, dev, x0, u0, steps=200))):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / 200 * 1e3)
    say("closed loop %-10s 4096 cars: %.3f ms per period (eager, wall clock, best of 3: %s)" % (label, min(ts), ["%.3f" % t for t in ts]))
