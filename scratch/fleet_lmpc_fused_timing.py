"""Period rate of the fleet LMPC experiment, unfused (closed_loop.run_lmpc_fleet) against fused (run_lmpc_fleet_fused, poll 1 and
16): 4096 BARC cars, N = 20, warm_laps = 1, learn_laps = 1.  The step count is what run_lmpc_fleet needs to finish; every timed run
then gets that count as max_steps.  The runs alternate; a host clock around a final synchronise (profiles/fleet_lmpc_fused.md is
this script's output plus a kernel trace taken in a run of its own with --only).

    python scratch/fleet_lmpc_fused_timing.py [--cars 4096] [--repeats 3] [--only unfused|fused1|fused16] [--steps K] [--out FILE.md]
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


def one(pkg, kind, tr, x0, u0, max_steps):
    tracker = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
    learner = pkg.Solver(pkg.presets.barc_lmpc(N, 3), pkg.presets.barc_vehicle(), device=0)
    kw = dict(warm_laps=1, learn_laps=1, warm_speed_scale=0.7, max_steps=max_steps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if kind == "unfused":
        res = pkg.closed_loop.run_lmpc_fleet(tracker, learner, tr, x0, u0, **kw)
    else:
        res = pkg.closed_loop.run_lmpc_fleet_fused(tracker, learner, tr, x0, u0, poll=int(kind[5:]), **kw)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    tracker.close(), learner.close()
    return res, wall


def laps(res):
    per = [[int(round(v / DT)) for v in t] for t in res["lap_times"]]
    first = np.array([p[0] if len(p) > 0 else -1 for p in per])
    second = np.array([p[1] if len(p) > 1 else -1 for p in per])
    return per[0], first, second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cars", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = load_package()
    B = a.cars
    tr = pkg.workloads.synthetic_track("barc")
    rng = np.random.default_rng(0)
    x0 = np.stack([np.full(B, 0.5), rng.uniform(-0.05, 0.05, B), np.zeros(B), np.full(B, 2.0), np.zeros(B), np.zeros(B)])
    x0, u0 = torch.as_tensor(x0, device="cuda"), torch.zeros((2, B), dtype=torch.float64, device="cuda")
    one(pkg, "fused1", tr, x0, u0, 20)      # warm-up: lazy initialisation, allocator
    if a.only:
        res, wall = one(pkg, a.only, tr, x0, u0, a.steps or 4000)
        print("%s: %d periods, %.2f s, %.1f periods/s" % (a.only, res["steps"], wall, res["steps"] / wall))
        return
    steps = a.steps
    if not steps:
        res, wall = one(pkg, "unfused", tr, x0, u0, 4000)
        steps = res["steps"]
        print("run_lmpc_fleet finishes in %d periods (%.2f s)" % (steps, wall), flush=True)
    kinds = ("unfused", "fused1", "fused16")
    walls, last = {k: [] for k in kinds}, {}
    for r in range(a.repeats):
        for k in kinds:
            res, wall = one(pkg, k, tr, x0, u0, steps)
            walls[k].append((res["steps"], wall))
            last[k] = res
            print("repeat %d %-8s %5d periods %7.3f s %8.1f periods/s" % (r, k, res["steps"], wall, res["steps"] / wall), flush=True)
    lines = ["| run | periods | wall s (each repeat) | periods/s (each repeat) | median periods/s | M car-steps/s |", "|---|---|---|---|---|---|"]
    med = {}
    for k in kinds:
        rate = [s / w for s, w in walls[k]]
        med[k] = float(np.median(rate))
        lines.append("| %s | %s | %s | %s | %.1f | %.3f |" % (k, " ".join(str(s) for s, _ in walls[k]), " ".join("%.3f" % w for _, w in walls[k]),
                                                       " ".join("%.1f" % v for v in rate), med[k], med[k] * B / 1e6))
    lines += ["", "fused poll 1 / unfused: %.2fx; fused poll 16 / unfused: %.2fx (medians of %d alternating repeats, %d cars, max_steps %d)"
              % (med["fused1"] / med["unfused"], med["fused16"] / med["unfused"], a.repeats, B, steps), ""]
    lines += ["| run | car 0 laps (periods) | tracking lap over cars min / median / max | learning lap min / median / max | cars with both laps | n_fail total |",
              "|---|---|---|---|---|---|"]
    for k in kinds:
        car0, first, second = laps(last[k])
        both = second >= 0
        f, s = first[both], second[both]
        lines.append("| %s | %s | %d / %d / %d | %d / %d / %d | %d of %d | %d |" % (k, car0, f.min(), np.median(f), f.max(), s.min(), np.median(s), s.max(),
                                                                                 int(both.sum()), B, int(last[k]["n_fail"].sum())))
    text = "\n".join(lines) + "\n"
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
