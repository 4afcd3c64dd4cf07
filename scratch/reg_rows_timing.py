"""Times the one-list (5, 3) regression kernel, the per-row kernel (three 4-feature lists, three equal 5-feature lists) and three
one-row passes of the same lists on bench.py's config-5 shape: batch 32768, N = 20, 5 BARC laps as two-sample laps (2200 samples)."""
import sys
import numpy as np
import torch
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package

pkg = load_package()
N, B = 20, int(sys.argv[1]) if len(sys.argv) > 1 else 32768
dev = "cuda"
tr = pkg.workloads.synthetic_track("barc")
solver = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), 0)
pv = dict(pkg.presets.barc_vehicle())
pv["mu"] *= 0.85
plant = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pv, 0)
laps = pkg.workloads.synthetic_laps(tr, 5)
reg_laps = pkg.workloads.regression_sample_pairs(
    tr, laps, lambda xa, ua: plant.plant_step(tr, torch.as_tensor(xa.T.copy(), device=dev), torch.as_tensor(ua.T.copy(), device=dev), 0.03).cpu().numpy().T)
plant.close()
out = {}
R444 = {3: ((3, 4, 5), (0,)), 4: ((3, 4, 5), (1,)), 5: ((3, 4, 5), (1,))}
R555 = {r: ((3, 4, 5), (0, 1)) for r in (3, 4, 5)}
SPECS = [("one-list (5, 3)", dict()), ("rows 4/4/4", dict(rows=R444)), ("rows 5/5/5", dict(rows=R555))] + \
        [("one row %d of 4/4/4" % r, dict(rows={r: R444[r]})) for r in (3, 4, 5)]
for data in ("spec", "near"):
    if data == "spec":
        x, u = pkg.workloads.sample_initial_states("barc", B, tr["L"], [-0.01, -0.314159], [0.01, 0.314159], seed=0)
    else:
        x, u = pkg.workloads.sample_states_near_laps(laps, B, tr["L"], seed=0)
    inp = solver.prepare(tr, x.T.copy(), 0.025)
    A0, B0, g0 = solver.linearize(inp)
    times = {name: [] for name, _ in SPECS}
    for rep in range(5):            # alternating: every spec once per round, five rounds
        for name, kw in SPECS:
            solver.set_regression_laps(reg_laps, dist_max=0.6, **kw)
            A, Bm, g = A0.clone(), B0.clone(), g0.clone()
            for _ in range(2):
                solver.regress(inp, A, Bm, g)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                solver.regress(inp, A, Bm, g)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / 10)
    # how many (query, row) pairs are corrected at all
    solver.set_regression_laps(reg_laps, dist_max=0.6, rows=R444)
    A, Bm, g = solver.regress(inp, A0.clone(), B0.clone(), g0.clone())
    touched = float(((g - g0)[3:] != 0).double().mean())
    print("queries: %s, %d x %d, %d samples; share of (query, row) pairs corrected: %.3f" % (data, B, N - 1, len(reg_laps), touched))
    for name, _ in SPECS:
        t = np.array(times[name])
        print("  %-22s median %.3f ms  (min %.3f, max %.3f; 5 rounds of 10 launches)" % (name, np.median(t), t.min(), t.max()))
    three = sum(np.median(times["one row %d of 4/4/4" % r]) for r in (3, 4, 5))
    print("  three one-row passes    %.3f ms  against one fused pass %.3f ms" % (three, np.median(times["rows 4/4/4"])))
solver.close()
