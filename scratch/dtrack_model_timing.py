"""What the double-track controller model costs (profiles/dtrack_model.md is this script's output), on 4096 BARC problems, N = 20, by
the method of scratch/fleet_dtrack_fused_timing.py: HIP events around launches enqueued behind a delay on the stream (the device's
time, not the host's rate of issue), five alternating repeats, the spread stated.

  --mode linearize   lmpc_linearize_dtrack_kernel (lmpc_linearize_dtrack_batch, three kinds of vehicle by b % 3) against
                     lmpc_linearize_kernel (lmpc_linearize_batch) on the same 4096 x 19 stages, outputs preallocated.
  --mode solve       the batch-4096, N = 20 tracking solve (lmpc_solve_batch: linearisation + QP kernel) with the switch on and with it
                     off, the same cold start.
  --mode period      closed_loop.run_lmpc_fleet_fused(plants_dt=) with and without controllers_dt= over the same `steps` periods
                     (default 200), alternating, a host clock around a final synchronise.

    python scratch/dtrack_model_timing.py --mode linearize|solve|period [--cars 4096] [--repeats 5] [--launches 100] [--steps 200]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package  # noqa: E402
from fleet_plants_timing import timed  # noqa: E402  (the same delay and the same events)

import vanilla_fleet_cases as FC  # noqa: E402

N, DT = 20, 0.025


def report(name, v):
    print("%-52s %s us per launch (median %.2f, spread %.1f %%)" % (name, " ".join("%.2f" % t for t in v), np.median(v), 100 * (max(v) - min(v)) / np.median(v)))
    return float(np.median(v))


def batch(pkg, B):
    tr = pkg.workloads.synthetic_track("barc")
    s = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
    trk = s.device_track(tr)
    x, u = pkg.workloads.sample_initial_states("barc", B, tr["L"], [-0.01, -0.314159], [0.01, 0.314159], seed=0)
    inp = s.prepare(trk, x.T.copy(), DT)
    inp["u_ic"] = torch.as_tensor(u.T.copy(), device="cuda")
    s.set_dtrack_vehicles(FC.dtrack_vehicles(pkg, B))
    torch.cuda.synchronize()
    return tr, s, inp


def linearize(pkg, B, repeats, launches):
    tr, s, inp = batch(pkg, B)
    kw = dict(dtype=torch.float64, device="cuda")
    out = (torch.empty((6, 6, N - 1, B), **kw), torch.empty((6, 2, N - 1, B), **kw), torch.empty((6, N - 1, B), **kw))
    lib, C = s.lib, pkg.capi.C
    p = [C.c_void_p(inp[k].data_ptr()) for k in ("X_ref", "U_ref", "T_ref", "curvatures")] + [C.c_void_p(t.data_ptr()) for t in out]
    calls = {"lmpc_linearize_kernel (single-track)": lambda j: lib.lmpc_linearize_batch(s._h, C.c_int32(B), *p),
             "lmpc_linearize_dtrack_kernel (double-track)": lambda j: lib.lmpc_linearize_dtrack_batch(s._h, C.c_int32(B), *p)}
    s.use_current_stream()
    us = {k: [] for k in calls}
    for r in range(repeats + 1):          # (repeat 0 is the warm-up)
        for name, fn in calls.items():
            t, host_ms = timed(launches, fn, 100.0)
            assert host_ms < 100.0, (name, host_ms)
            assert bool(torch.isfinite(out[0]).all())
            if r:
                us[name].append(t)
    a, b = (report("%s, %d x %d stages" % (name, B, N - 1), v) for name, v in us.items())
    print("double-track / single-track: %.2f" % (b / a))
    s.close()


def solve(pkg, B, repeats, launches):
    tr, s, inp = batch(pkg, B)
    inp = dict(inp, L=float(tr["L"]))
    out = s.alloc_outputs(B)
    us = {False: [], True: []}
    for r in range(repeats + 1):
        for on in (False, True):
            s.set_dtrack_controller_model(on)
            t, host_ms = timed(launches, lambda j: s.solve(inp, out), 200.0)
            assert host_ms < 200.0, host_ms
            failed = int((out["status"] != 0).sum())
            assert failed <= B // 100, failed   # (random x0: a car or two of 4096 start outside what the boxes allow, on either model)
            if r:
                us[on].append(t)
            if r == repeats:
                print("switch %s: iterations mean %.2f max %d, failed solves %d of %d"
                      % ("on" if on else "off", float(out["iters"].float().mean()), int(out["iters"].max()), failed, B))
    a = report("lmpc_solve_batch, switch off, %d problems" % B, us[False])
    b = report("lmpc_solve_batch, switch on, %d problems" % B, us[True])
    print("on minus off: %.2f us (%.1f %%)" % (b - a, 100 * (b - a) / a))
    # where the difference sits: the handle's own events around the linearisation and around the QP kernel, one solve at a time
    s.enable_timing(True)
    for on in (False, True):
        s.set_dtrack_controller_model(on)
        ms = []
        for _ in range(repeats + 1):
            s.solve(inp, out)
            ms.append(s.last_kernel_ms())
        lin, qp = np.median([m[0] for m in ms[1:]]), np.median([m[1] for m in ms[1:]])
        print("switch %-3s lmpc_last_kernel_ms: linearisation %.1f us, QP kernel %.1f us (medians of %d single solves)" % ("on" if on else "off", 1e3 * lin, 1e3 * qp, repeats))
    s.close()


def period(pkg, B, repeats, steps):
    tr = pkg.workloads.synthetic_track("barc")
    rng = np.random.default_rng(0)
    x0 = np.stack([np.full(B, 0.5), rng.uniform(-0.05, 0.05, B), np.zeros(B), np.full(B, 2.0), np.zeros(B), np.zeros(B)])
    x0, u0 = torch.as_tensor(x0, device="cuda"), torch.zeros((2, B), dtype=torch.float64, device="cuda")
    veh = FC.dtrack_vehicles(pkg, B)

    def one(model, max_steps):
        tracker = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
        learner = pkg.Solver(pkg.presets.barc_lmpc(N, 3), pkg.presets.barc_vehicle(), device=0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pkg.closed_loop.run_lmpc_fleet_fused(tracker, learner, tr, x0, u0, max_steps=max_steps, plants_dt=veh, poll=1,
                                                   **({"controllers_dt": veh} if model else {}))
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        tracker.close(), learner.close()
        return res, wall

    for model in (True, False):
        one(model, 10)      # warm-up: lazy initialisation, allocator
    rate = {True: [], False: []}
    for r in range(repeats):
        for model in (True, False):
            res, wall = one(model, steps)
            rate[model].append(res["steps"] / wall)
            print("repeat %d %-28s %5d periods %7.3f s %8.1f periods/s, failed solves %d"
                  % (r, "double-track controllers" if model else "single-track controllers", res["steps"], wall, res["steps"] / wall,
                     int(res["n_fail"].sum())), flush=True)
    for model, v in rate.items():
        print("%-28s median %.1f periods/s, spread %.2f %%" % ("double-track controllers" if model else "single-track controllers", np.median(v),
                                                               100 * (max(v) - min(v)) / np.median(v)))
    print("double-track / single-track controllers: %.3f" % (np.median(rate[True]) / np.median(rate[False])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("linearize", "solve", "period"), required=True)
    ap.add_argument("--cars", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    pkg = load_package()
    print("library:", pkg.capi.library_path().name, "| mode", a.mode)
    if a.mode == "linearize":
        linearize(pkg, a.cars, a.repeats, a.launches)
    elif a.mode == "solve":
        solve(pkg, a.cars, a.repeats, a.launches)
    else:
        period(pkg, a.cars, a.repeats, a.steps)


if __name__ == "__main__":
    main()
