"""Periods per second of closed_loop.run_estimated_fused against closed_loop.run_estimated (profiles/estimated_fused.md).

B cars on the BARC track, N = 20, `--periods` periods a run; after one warm-up run of each loop, `--repeats` alternating runs of the
two, each between two HIP events on the stream (the runs end in a device synchronise), medians reported.  Both runs include their own
set-up (filter, cold start): a few launches against `periods` periods.  --mode fused | unfused runs one loop only (for a kernel
trace: rocprofv3 --kernel-trace --stats -- python scratch/estimated_fused_timing.py --mode fused --repeats 1).
Needs an MI355X; prints one JSON line."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--periods", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mode", choices=("both", "fused", "unfused"), default="both")
    args = ap.parse_args()
    import torch

    from __graft_entry__ import load_package
    pkg = load_package()
    sv = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    tr = pkg.racing_trajectory.RacingTrajectory(ROOT / "tests" / "golden" / "barc_track" / "15_barc_optm.txt")
    spline, tab = sv.spline_track(tr), tr.to_track_table(1024)
    B = args.batch
    rng = np.random.default_rng(2)
    x0 = torch.as_tensor(np.stack([rng.uniform(0, tab["L"], B), rng.uniform(-0.05, 0.05, B), np.zeros(B), rng.uniform(1.5, 2.5, B), np.zeros(B),
                                   np.zeros(B)]), device="cuda")
    u0 = torch.zeros((2, B), dtype=torch.float64, device="cuda")
    loops = {"unfused": pkg.closed_loop.run_estimated, "fused": pkg.closed_loop.run_estimated_fused}
    if args.mode != "both":
        loops = {args.mode: loops[args.mode]}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        res = fn(sv, tab, spline, x0, u0, args.periods, seed=4)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3, res

    last = {}
    for name, fn in loops.items():   # warm-up: code objects, workspaces, the allocator's pools
        _, last[name] = timed(fn)
    sec = {name: [] for name in loops}
    for _ in range(args.repeats):
        for name, fn in loops.items():
            t, last[name] = timed(fn)
            sec[name].append(t)
    out = {"batch": B, "periods": args.periods, "repeats": args.repeats}
    for name in loops:
        med = statistics.median(sec[name])
        out[name] = {"median_s": med, "periods_per_s": args.periods / med, "ms_per_period": 1e3 * med / args.periods,
                     "runs_s": [round(t, 4) for t in sec[name]], "failed_solves": int(last[name]["n_fail"].sum()),
                     "rms_error": [round(float(v), 4) for v in last[name]["rms_error"]]}
    if len(loops) == 2:
        out["fused_over_unfused"] = out["fused"]["periods_per_s"] / out["unfused"]["periods_per_s"]
        same = (last["fused"]["n_fail"] == 0) & (last["unfused"]["n_fail"] == 0)
        out["cars_without_a_failed_solve"] = int(same.sum())
        out["max_abs_truth_difference_on_them"] = float((last["fused"]["x"] - last["unfused"]["x"]).abs()[:, same].max())
    print(json.dumps(out))
    spline.close()
    sv.close()


if __name__ == "__main__":
    main()
