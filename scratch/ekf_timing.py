"""Timing of the batched extended Kalman filter (profiles/ekf.md takes this script's output).

For B = 4096 and 32768 cars, after a warm-up, `--reps` alternating calls, each between two HIP events, medians:
  (p) lmpc_ekf_update_batch with obs_id = -1: the prediction kernel alone
  (v) a 2-row update (rows 3, 5): prediction + lmpc_ekf_correct_kernel<2>
  (q) a 3-row update (rows 0, 1, 2, the yaw row aligned): prediction + lmpc_ekf_correct_kernel<3>
  (l) the yardstick of the same session: lmpc_linearize_batch (the C-ABI layout, W = 1 kernel) over B threads of work -- B / 2
      problems of the smallest horizon the library accepts, N = 3, i.e. two stages each.  One thread there evaluates the same four
      RK4 points and pushes eight tangent columns; the prediction kernel pushes twelve and moves 72 + 72 doubles of P.
The filters run the scenario of tests/ekf_cases.py (vx 1.5 .. 2.5, updates 5 ms apart), so the arithmetic is the tested one; the
outputs are written to caller arrays, as the closed loop asks for them.

    python scratch/ekf_timing.py [--reps 100] [--batches 4096,32768] [--out FILE.md]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
from __graft_entry__ import load_package  # noqa: E402

import ekf_cases as EC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--batches", default="4096,32768")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = load_package()
    tr = pkg.workloads.synthetic_track("barc")
    lines = ["| B | (p) prediction us | (v) 2-row update us | (q) 3-row update us | (l) linearise, B threads us | (p) / (l) |", "|---|---|---|---|---|---|"]
    for B in [int(v) for v in a.batches.split(",")]:
        sc = EC.scenario(B, periods=1)
        solver = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
        small = pkg.Solver(pkg.presets.barc_tracking_mpc(3), pkg.presets.barc_vehicle(), device=0)
        dev = lambda arr: torch.as_tensor(np.ascontiguousarray(np.moveaxis(np.asarray(arr, dtype=np.float64), 0, -1)), device=solver.device)  # noqa: E731
        cfg = sc["cfg"]
        solver.ekf_create(B, cfg["x0"], cfg["P0"], cfg["Q"], cfg["x_min"], cfg["x_max"])
        o_v, o_p = solver.ekf_register_observation(EC.ROWS_VEL), solver.ekf_register_observation(EC.ROWS_POSE)
        x0, P0 = dev(sc["x0"]), dev(sc["P0"])
        (_, zv, Rv, u, _), (_, zp, Rp, _, _) = sc["updates"]
        zv, Rv, zp, Rp, u = dev(zv), dev(Rv), dev(np.nan_to_num(zp, nan=0.1)), dev(Rp), dev(u)
        solver.ekf_update_control(u)
        solver.ekf_initialize(0)
        kw = dict(dtype=torch.float64, device=solver.device)
        flags = torch.empty((B,), dtype=torch.int32, device=solver.device)
        out = {2: (torch.empty((6, B), **kw), torch.empty((6, 6, B), **kw), torch.empty((6, 2, B), **kw), flags),
               3: (torch.empty((6, B), **kw), torch.empty((6, 6, B), **kw), torch.empty((6, 3, B), **kw), flags)}
        xs, _ = pkg.workloads.sample_initial_states("barc", B // 2, tr["L"], [-0.01, -0.314159], [0.01, 0.314159], seed=0)
        inp = small.prepare(tr, np.ascontiguousarray(xs.T), 0.025)
        ns = [0]

        def call(key):
            if key == "l":
                small.linearize(inp)
                return
            ns[0] += 5_000_000
            if key == "p":
                solver.ekf_update(-1, None, None, ns[0], out=(out[2][0], out[2][1], None, flags))
            elif key == "v":
                solver.ekf_update(o_v, zv, Rv, ns[0], out=out[2])
            else:
                solver.ekf_update(o_p, zp, Rp, ns[0], out=out[3])

        ev = {key: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)] for key in "pvql"}
        for i in range(-5, a.reps):
            for key in "pvql":
                if key != "l":
                    solver.ekf_set_state(x0, P0)   # every timed update starts from the scenario's start (the seed kernel runs before the first event)
                if i >= 0:
                    ev[key][i][0].record()
                call(key)
                if i >= 0:
                    ev[key][i][1].record()
        torch.cuda.synchronize()
        us = {key: float(np.median([s.elapsed_time(e) for s, e in ev[key]])) * 1e3 for key in "pvql"}
        lines.append("| %d | %.1f | %.1f | %.1f | %.1f | %.2f |" % (B, us["p"], us["v"], us["q"], us["l"], us["p"] / us["l"]))
        print(lines[-1], flush=True)
        solver.close()
        small.close()
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
