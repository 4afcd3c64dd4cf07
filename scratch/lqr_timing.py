"""Timing of the batched time-varying LQR (profiles/lqr.md takes this script's output).

Per case (vehicle, B, N, dt), after a warm-up, `--reps` alternating calls, each between two HIP events, medians:
  (s) lmpc_lqr_solve_batch: both launches, K and P0 written to caller arrays
  (d) its first launch alone is not separable through the ABI; it is estimated by (s) at the same B with N = 2 -- one stage's
      discretisation, one stage of recursion and rollout -- and reported as context
  (q) the yardstick of the same session: the tracking QP solve (lmpc_solve_batch) of the same vehicle, B and N on a cold start
The LQR runs the scenarios of tests/lqr_cases.py (a reference that is an RK4 rollout, x_ic beside it), so the arithmetic is the
tested one.  The QP figure is context only: it is another problem (bounds, an interior-point iteration).

    python scratch/lqr_timing.py [--reps 50] [--cases barc:4096:20:0.01,iac:4096:81:0.05,barc:64:81:0.005] [--out FILE.md]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
from __graft_entry__ import load_package  # noqa: E402

import lqr_cases as LC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--cases", default="barc:4096:20:0.01,iac:4096:81:0.05,barc:64:81:0.005")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = load_package()
    lines = ["| vehicle | B | N | dt | (s) LQR solve us | (d) the same at N = 2 us | (q) tracking QP solve us | flagged cars |", "|---|---|---|---|---|---|---|---|"]
    for case in a.cases.split(","):
        kind, B, N, dt = case.split(":")
        B, N, dt = int(B), int(N), float(dt)
        barc = kind == "barc"
        vehd = pkg.presets.barc_vehicle() if barc else pkg.presets.iac_vehicle()
        cfgd = pkg.presets.barc_tracking_mpc(N) if barc else pkg.presets.iac_tracking_mpc(N)
        solver, small = pkg.Solver(cfgd, vehd, device=0), pkg.Solver(cfgd, vehd, device=0)
        dev = lambda arr: torch.as_tensor(np.ascontiguousarray(np.moveaxis(np.asarray(arr, dtype=np.float64), 0, -1)), device=solver.device)  # noqa: E731
        sc = LC.scenario(kind, N, dt, seed=1, B=B)
        solver.lqr_create(sc["cfg"], B)
        small.lqr_create(LC.config(2, dt), B)
        args = [dev(sc[k]) for k in ("x_ic", "X_ref", "U_ref")]
        args2 = [args[0], args[1][:, :2].contiguous(), args[2][:, :1].contiguous()]
        out = solver.lqr_solve(*args, gains=True)
        out2 = small.lqr_solve(*args2, gains=True)
        tr = pkg.workloads.synthetic_track("barc" if barc else "putnam")
        lo, hi = ([-0.01, -0.314159], [0.01, 0.314159]) if barc else ([-10.0, -0.314159], [5.0, 0.314159])
        xs, _ = pkg.workloads.sample_initial_states("barc" if barc else "putnam", B, tr["L"], lo, hi, seed=0)
        inp = solver.prepare(tr, np.ascontiguousarray(xs.T), 0.025)
        inp["u_ic"] = torch.zeros((2, B), dtype=torch.float64, device=solver.device)
        qp_out = solver.alloc_outputs(B)

        def call(key):
            if key == "s":
                solver.lqr_solve(*args, out=out)
            elif key == "d":
                small.lqr_solve(*args2, out=out2)
            else:
                solver.solve(inp, qp_out)

        ev = {key: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)] for key in "sdq"}
        for i in range(-5, a.reps):
            for key in "sdq":
                if i >= 0:
                    ev[key][i][0].record()
                call(key)
                if i >= 0:
                    ev[key][i][1].record()
        torch.cuda.synchronize()
        us = {key: float(np.median([s.elapsed_time(e) for s, e in ev[key]])) * 1e3 for key in "sdq"}
        lines.append("| %s | %d | %d | %g | %.1f | %.1f | %.1f | %d |" % (kind, B, N, dt, us["s"], us["d"], us["q"], int((out["flags"] != 0).sum())))
        print(lines[-1], "QP status != 0:", int((qp_out["status"] != 0).sum()), flush=True)
        solver.close()
        small.close()
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
