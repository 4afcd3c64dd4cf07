"""Timing of the fleet safe-set kernels against the shared-store query (profiles/fleet_ss_query.md is this script's output).

(a) lmpc_ss_query_batch on workloads.synthetic_laps (5 laps x 440 samples), S = 160, K = 32
(b) lmpc_fleet_ss_query_batch with the same laps loaded into every car and the same queries
(c) lmpc_fleet_ss_record_batch
for B = 4096 and 32768: after a warm-up the kernels alternate, each call between two HIP events, `--reps` times; medians.
The fleet kernel's algorithmic bytes are counted from the shapes: 16 B x (samples of the car's laps) in, 56 S B out, and the
gathered points (48 B each: 16 of the key plane, 32 of the point plane).

    python scratch/fleet_ss_timing.py [--reps 200] [--batches 4096,32768] [--out FILE.md]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

COPY_BW, PEAK_BW = 6.29e12, 8.0e12   # measured copy bandwidth and HBM peak of the MI355X, bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batches", default="4096,32768")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = load_package()
    tr = pkg.workloads.synthetic_track("barc")
    L = float(tr["L"])
    laps_x = pkg.workloads.synthetic_laps(tr)
    laps = [(x, np.zeros((x.shape[0], 2)), np.zeros(x.shape[0]), 0.03 * np.arange(x.shape[0])) for x in laps_x]
    n_sum, cap = sum(x.shape[0] for x in laps_x), max(x.shape[0] for x in laps_x)
    cfg = pkg.presets.barc_lmpc(20, len(laps))
    S, K = int(cfg["num_ss_pts"]), int(cfg["num_ss_pts_per_lap"])
    lines = ["# Fleet safe-set kernels: timing", "",
             "%d laps x %d samples per car, S = %d, K = %d; medians of %d alternating calls between HIP events (scratch/fleet_ss_timing.py)." % (
                 len(laps), cap, S, K, a.reps), "",
             "| B | (a) shared-store query us | (b) fleet query us | (c) fleet record us | (b) bytes per query | (b) GB/s | of 6.29 TB/s copy | of 8 TB/s peak | extra distinct MB | extra / 6.29 TB/s us | (b) - (a) us |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for B in [int(v) for v in a.batches.split(",")]:
        shared = pkg.Solver(cfg, pkg.presets.barc_vehicle(), device=0)
        shared.set_safe_set(laps_x, L)
        fleet = pkg.Solver(cfg, pkg.presets.barc_vehicle(), device=0)
        nbytes = fleet.fleet_ss_create(B, cap)
        fleet.fleet_ss_load(laps, L, car=-1)
        rng = np.random.default_rng(1)
        q = torch.as_tensor(np.stack([rng.uniform(0, L, B), rng.uniform(-0.1, 0.1, B)]), device="cuda")
        out_a = shared.ss_query(q)
        out_b = fleet.fleet_ss_query(q)
        torch.cuda.synchronize()
        same = all(torch.equal(x, y) for x, y in zip(out_a, out_b))
        # the recorder on a store of its own, so that the queried rings stay as loaded: cars advancing 0.04 per period
        rec = pkg.Solver(cfg, pkg.presets.barc_vehicle(), device=0)
        rec.fleet_ss_create(B, cap)
        xs = torch.as_tensor(rng.normal(size=(6, B)), device="cuda")
        xs[0] = torch.as_tensor(rng.uniform(0, L, B), device="cuda")
        us, ks = torch.zeros((2, B), dtype=torch.float64, device="cuda"), torch.zeros(B, dtype=torch.float64, device="cuda")
        ev = {key: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)] for key in "abc"}
        for i in range(-10, a.reps):
            xs[0] = torch.remainder(xs[0] + 0.04, L)
            for key, fn in (("a", lambda: shared.ss_query(q, out=out_a)), ("b", lambda: fleet.fleet_ss_query(q, out=out_b)),
                            ("c", lambda: rec.fleet_ss_record(xs, us, ks, 0.03 * (i + 10), L))):
                if i >= 0:
                    ev[key][i][0].record()
                fn()
                if i >= 0:
                    ev[key][i][1].record()
        torch.cuda.synchronize()
        us_ = {key: float(np.median([s.elapsed_time(e) for s, e in ev[key]])) * 1e3 for key in "abc"}
        per_query = 16 * n_sum + 56 * S + 48 * S
        extra = B * (16 * n_sum + 48 * S)     # what (b) must fetch from HBM and (a) finds in L2: every car's own keys and points
        rate = B * per_query / (us_["b"] * 1e-6)
        lines.append("| %d | %.1f | %.1f | %.1f | %d | %.0f | %.1f %% | %.1f %% | %.1f | %.1f | %.1f |" % (
            B, us_["a"], us_["b"], us_["c"], per_query, rate / 1e9, 100 * rate / COPY_BW, 100 * rate / PEAK_BW, extra / 1e6,
            extra / COPY_BW * 1e6, us_["b"] - us_["a"]))
        print(lines[-1], "| results bit-equal:", same, "| store bytes", nbytes, flush=True)
        assert same
        for s in (shared, fleet, rec):
            s.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        Path(a.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
