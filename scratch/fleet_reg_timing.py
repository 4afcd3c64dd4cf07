"""Timing of the per-car regression against the shared one (profiles/fleet_regression.md takes this script's output).

Per car 5 laps x 440 samples (workloads.synthetic_laps with the noise of workloads.regression_sample_pairs: 2195 samples with a
successor), spec (5, 3) on the bench's features, dist_max 0.6; queries = the references lmpc_prepare_batch builds from states near the
laps.  For B = 4096 and 32768 cars and N = 20 and 40, after a warm-up, `--reps` alternating calls, each between two HIP events, medians:
  (a) lmpc_regress_batch on ONE shared store of the same 2195 samples (plus one far sample pair that makes lmpc_set_regression_laps
      select the EXACT instance, the arithmetic the per-car kernel always uses)
  (b) lmpc_fleet_ss_regress_batch with nothing changed: the pack kernel's early return + lmpc_fleet_regress_kernel
  (c) the same right after every stamp was invalidated (lmpc_fleet_ss_set_regression with the same spec): every car repacks
An event pair around one entry point cannot split its two launches, so the script reports (b), (c) and (c) - (b) = the cost of
repacking every car; the pack kernel's early return alone is the minimum of lmpc_fleet_reg_pack_kernel in a kernel trace of this
script (rocprofv3 --kernel-trace --stats -- python scratch/fleet_reg_timing.py --reps 20), its maximum the full repack.

    python scratch/fleet_reg_timing.py [--reps 100] [--batches 4096,32768] [--horizons 20,40] [--out FILE.md]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--batches", default="4096,32768")
    ap.add_argument("--horizons", default="20,40")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = load_package()
    tr = pkg.workloads.synthetic_track("barc")
    L = float(tr["L"])
    rng = np.random.default_rng(7)
    laps = []
    for x in pkg.workloads.synthetic_laps(tr):
        n = x.shape[0]
        x = x + rng.normal(0, 1, (n, 6)) * np.array([0.0, 0.02, 0.02, 0.1, 0.03, 0.2])
        u = np.stack([rng.uniform(-0.005, 0.005, n), rng.uniform(-0.15, 0.15, n)], axis=1)
        k = np.interp(x[:, 0], np.arange(tr["M"]) * L / tr["M"], tr["curvature"], period=L)
        laps.append((x, u, k, 0.03 * np.arange(n)))
    cap = max(l[0].shape[0] for l in laps)
    far = (np.tile([0.0, 0.0, 0.0, 100.0, 0.0, 0.0], (2, 1)), np.zeros((2, 2)), np.zeros(2), np.array([0.0, 0.03]))
    rows = sum(l[0].shape[0] - 1 for l in laps)
    lines = ["| B | N | (a) shared, EXACT us | (b) per car, nothing changed us | (c) per car, every car repacks us | (c) - (b) us | (b) / (a) | 64 / (N - 1) |",
             "|---|---|---|---|---|---|---|---|"]
    for N in [int(v) for v in a.horizons.split(",")]:
        cfg = dict(pkg.presets.barc_tracking_mpc(N), max_lap_stored=len(laps))
        for B in [int(v) for v in a.batches.split(",")]:
            shared = pkg.Solver(cfg, pkg.presets.barc_vehicle(), device=0)
            shared.set_regression_laps(laps + [far], dist_max=0.6)
            fleet = pkg.Solver(cfg, pkg.presets.barc_vehicle(), device=0)
            fleet.fleet_ss_create(B, cap)
            fleet.fleet_ss_load(laps, L, car=-1)
            fleet.fleet_ss_set_regression(dist_max=0.6)
            x0, _ = pkg.workloads.sample_states_near_laps([l[0] for l in laps], B, L, seed=3)
            inp = fleet.prepare(tr, np.ascontiguousarray(x0.T), 0.025)
            A0, B0, g0 = fleet.linearize(inp)
            Aa, Ba, ga = shared.regress(inp, A0.clone(), B0.clone(), g0.clone())
            Ab, Bb, gb = fleet.fleet_ss_regress(inp, A0.clone(), B0.clone(), g0.clone())
            torch.cuda.synchronize()
            agree = float((Aa - Ab).abs().max() / (1 + Aa.abs().max()))
            touched = float(((Ab - A0).abs().amax(dim=(0, 1)) > 0).double().mean())
            ev = {key: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)] for key in "abc"}
            for i in range(-5, a.reps):
                for key in "abc":
                    if key == "c":
                        fleet.fleet_ss_set_regression(dist_max=0.6)   # the same spec: every stamp stale (two memsets, outside the events)
                    fn = (lambda: shared.regress(inp, Aa, Ba, ga)) if key == "a" else (lambda: fleet.fleet_ss_regress(inp, Ab, Bb, gb))
                    if i >= 0:
                        ev[key][i][0].record()
                    fn()
                    if i >= 0:
                        ev[key][i][1].record()
            torch.cuda.synchronize()
            us = {key: float(np.median([s.elapsed_time(e) for s, e in ev[key]])) * 1e3 for key in "abc"}
            lines.append("| %d | %d | %.0f | %.0f | %.0f | %.0f | %.2f | %.2f |" % (B, N, us["a"], us["b"], us["c"], us["c"] - us["b"], us["b"] / us["a"],
                                                                              64.0 / (N - 1)))
            print(lines[-1], "  (agreement %.1e, %.0f %% of the queries touched, %d rows per car, table %.2f GB)" % (
                agree, 100 * touched, rows, (fleet.fleet_ss_bytes()) / 1e9), flush=True)
            shared.close()
            fleet.close()
            del Aa, Ba, ga, Ab, Bb, gb, A0, B0, g0, inp
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
