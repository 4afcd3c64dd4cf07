"""The LMPC experiment with every car learning from its own laps (closed_loop.run_lmpc_fleet) on the x0 of
tests/test_gpu_path.py::test_lmpc_experiment_lap_times_improve: per car the tracking and learning lap times, n_fail and
worst_excess, as a table (profiles/fleet_lmpc_experiment.md is this script's output).

    python scratch/fleet_lmpc_experiment.py [--out FILE.md]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = load_package()
    N, B, warm_laps, learn_laps, dt = 20, 64, 2, 4, 0.025
    tracker = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
    learner = pkg.Solver(pkg.presets.barc_lmpc(N, 3), pkg.presets.barc_vehicle(), device=0)
    tr = pkg.workloads.synthetic_track("barc")
    rng = np.random.default_rng(0)
    x0 = np.stack([np.full(B, 0.5), rng.uniform(-0.05, 0.05, B), np.zeros(B), np.full(B, 2.0), np.zeros(B), np.zeros(B)])
    x0[:, 0] = [0.5, 0.0, 0.0, 2.0, 0.0, 0.0]
    t0 = time.time()
    res = pkg.closed_loop.run_lmpc_fleet(tracker, learner, tr, torch.as_tensor(x0, device="cuda"), torch.zeros((2, B), dtype=torch.float64, device="cuda"),
                                         warm_laps=warm_laps, learn_laps=learn_laps, warm_speed_scale=0.7)
    torch.cuda.synchronize()
    wall = time.time() - t0
    nf, exc = res["n_fail"].cpu().numpy(), res["worst_excess"].cpu().numpy()
    nd, lir = res["n_dropped"].cpu().numpy(), res["laps_in_ring"].cpu().numpy()
    short = [b for b in range(B) if len(res["lap_times"][b]) < warm_laps + learn_laps or res["lap_kind"][b].count("lmpc") < learn_laps]
    lines = ["# LMPC experiment, every car on its own safe set", "",
             "closed_loop.run_lmpc_fleet, %d cars, N = %d, %d tracking laps at speed scale 0.7 then %d learning laps, dt = %.3f s "
             "(scratch/fleet_lmpc_experiment.py).  %d control periods, %.1f s wall.  Lap times in control periods (time / dt); e_y(0) is "
             "the car's initial lateral offset.  worst_excess <= 0: the body never left the track." % (B, N, warm_laps, learn_laps, dt, res["steps"], wall), "",
             "Cars that did not complete %d + %d laps: %s." % (warm_laps, learn_laps, ", ".join(map(str, short)) if short else "none"),
             "Laps dropped for their length: %d.  Laps in every ring at the end: %s." % (int(nd.sum()), sorted(set(lir.tolist()))), "",
             "| car | e_y(0) | tracking laps | learning laps | last / first learning lap | n_fail | worst_excess m |", "|---|---|---|---|---|---|---|"]
    ratios = []
    for b in range(B):
        per = [int(round(v / dt)) for v in res["lap_times"][b]]
        trk = [p for p, kd in zip(per, res["lap_kind"][b]) if kd == "tracking"]
        lrn = [p for p, kd in zip(per, res["lap_kind"][b]) if kd == "lmpc"][:learn_laps]
        ratio = lrn[-1] / lrn[0] if len(lrn) >= 2 else float("nan")
        ratios.append(ratio)
        lines.append("| %d | %+.4f | %s | %s | %.3f | %d | %+.4f |" % (b, x0[1, b], " ".join(map(str, trk)), " ".join(map(str, lrn)), ratio, nf[b], exc[b]))
    lines += ["", "Over the cars: n_fail max %d, mean %.2f; worst_excess max %+.4f m; last / first learning lap min %.3f, median %.3f, max %.3f." % (
        nf.max(), nf.mean(), exc.max(), np.nanmin(ratios), np.nanmedian(ratios), np.nanmax(ratios))]
    text = "\n".join(lines) + "\n"
    if a.out:
        Path(a.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
