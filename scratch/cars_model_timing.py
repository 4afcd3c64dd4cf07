"""What the per-car single-track controller model costs (profiles/cars_model.md is this script's output), on 4096 BARC problems, N = 20,
by the method of scratch/dtrack_model_timing.py: HIP events around launches enqueued behind a delay on the stream (the device's time,
not the host's rate of issue), five alternating repeats, the spread stated.

  --mode linearize   lmpc_linearize_cars_kernel (lmpc_linearize_cars_batch, three kinds of vehicle by b % 3, two cars on Euler) against
                     lmpc_linearize_kernel (lmpc_linearize_batch) on the same 4096 x 19 stages, outputs preallocated; then the float
                     instantiation of both, which has no entry point of its own, by the handle's events around the linearisation of
                     lmpc_solve_batch_f32 with the switch on and off.
  --mode solve       the batch-4096, N = 20 tracking solve (lmpc_solve_batch: linearisation + QP kernel) with the switch on and with it
                     off, the same cold start.
  --mode period      closed_loop.run_lmpc_fleet_fused(plants=) with and without controllers= over the same `steps` periods (default
                     200), alternating, a host clock around a final synchronise.

  --mode pipeline    bench.py's three-stream pipeline of batch-4096 solves with the switch on and off on a table of the handle's vehicle:
                     what it costs that this kernel has no 256-register W = 2 build (a host clock around `steps` solves).

    python scratch/cars_model_timing.py --mode linearize|solve|period|pipeline [--cars 4096] [--repeats 5] [--launches 100] [--steps 200]
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

import cars_model_cases as MC  # noqa: E402

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
    s.set_car_vehicles(MC.fleet(pkg.presets.barc_vehicle(), B))
    torch.cuda.synchronize()
    return tr, s, inp


def handle_events(s, call, repeats, what):
    """medians of lmpc_last_kernel_ms over single calls, in us"""
    s.enable_timing(True)
    ms = []
    for _ in range(repeats + 1):
        call()
        ms.append(s.last_kernel_ms())
    s.enable_timing(False)
    lin, qp = [1e3 * m[0] for m in ms[1:]], [1e3 * m[1] for m in ms[1:]]
    print("%-44s lmpc_last_kernel_ms: linearisation %.1f us (min %.1f max %.1f), QP kernel %.1f us (medians of %d single calls)"
          % (what, np.median(lin), min(lin), max(lin), np.median(qp), repeats))
    return float(np.median(lin))


def linearize(pkg, B, repeats, launches):
    tr, s, inp = batch(pkg, B)
    kw = dict(dtype=torch.float64, device="cuda")
    out = (torch.empty((6, 6, N - 1, B), **kw), torch.empty((6, 2, N - 1, B), **kw), torch.empty((6, N - 1, B), **kw))
    lib, C = s.lib, pkg.capi.C
    p = [C.c_void_p(inp[k].data_ptr()) for k in ("X_ref", "U_ref", "T_ref", "curvatures")] + [C.c_void_p(t.data_ptr()) for t in out]
    calls = {"lmpc_linearize_kernel (the handle's vehicle)": lambda j: lib.lmpc_linearize_batch(s._h, C.c_int32(B), *p),
             "lmpc_linearize_cars_kernel (car b's vehicle)": lambda j: lib.lmpc_linearize_cars_batch(s._h, C.c_int32(B), *p)}
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
    print("per car / handle: %.2f" % (b / a))
    # the workspace forms in front of a solve, fp64 and float io, by the handle's own events
    inp = dict(inp, L=float(tr["L"]))
    out64 = s.alloc_outputs(B)
    for on in (False, True):
        s.set_cars_controller_model(on)
        handle_events(s, lambda: s.solve(inp, out64), 2 * repeats, "lmpc_solve_batch, switch %s" % ("on" if on else "off"))
        handle_events(s, lambda: s.solve_f32(inp), 2 * repeats, "lmpc_solve_batch_f32, switch %s" % ("on" if on else "off"))
    s.close()


def solve(pkg, B, repeats, launches):
    tr, s, inp = batch(pkg, B)
    inp = dict(inp, L=float(tr["L"]))
    out = s.alloc_outputs(B)
    us = {False: [], True: []}
    for r in range(repeats + 1):
        for on in (False, True):
            s.set_cars_controller_model(on)
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
    for on in (False, True):
        s.set_cars_controller_model(on)
        handle_events(s, lambda: s.solve(inp, out), repeats, "switch %s" % ("on" if on else "off"))
    s.close()


def period(pkg, B, repeats, steps):
    tr = pkg.workloads.synthetic_track("barc")
    rng = np.random.default_rng(0)
    x0 = np.stack([np.full(B, 0.5), rng.uniform(-0.05, 0.05, B), np.zeros(B), np.full(B, 2.0), np.zeros(B), np.zeros(B)])
    x0, u0 = torch.as_tensor(x0, device="cuda"), torch.zeros((2, B), dtype=torch.float64, device="cuda")
    veh = MC.fleet(pkg.presets.barc_vehicle(), B)

    names = {True: "per-car controllers", False: "one controller model"}

    def one(model, max_steps, events=False):
        tracker = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
        learner = pkg.Solver(pkg.presets.barc_lmpc(N, 3), pkg.presets.barc_vehicle(), device=0)
        tracker.enable_timing(events)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pkg.closed_loop.run_lmpc_fleet_fused(tracker, learner, tr, x0, u0, max_steps=max_steps, plants=veh, poll=1,
                                                   **({"controllers": veh} if model else {}))
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        if events:   # the handle's events around the last period's linearisation and QP kernel (a run of its own: not timed)
            print("%-24s last period of the tracking controller: linearisation %.1f us, QP kernel %.1f us" % ((names[model],) + tuple(1e3 * m for m in tracker.last_kernel_ms())))
        tracker.close(), learner.close()
        return res, wall

    for model in (True, False):
        one(model, 10)      # warm-up: lazy initialisation, allocator
    rate = {True: [], False: []}
    for r in range(repeats):
        for model in (True, False):
            res, wall = one(model, steps)
            rate[model].append(res["steps"] / wall)
            print("repeat %d %-24s %5d periods %7.3f s %8.1f periods/s, failed solves %d"
                  % (r, names[model], res["steps"], wall, res["steps"] / wall, int(res["n_fail"].sum())), flush=True)
    for model, v in rate.items():
        print("%-24s median %.1f periods/s, spread %.2f %%" % (names[model], np.median(v), 100 * (max(v) - min(v)) / np.median(v)))
    print("per-car / one model: %.3f" % (np.median(rate[True]) / np.median(rate[False])))
    for model in (True, False):
        one(model, steps, events=True)


def pipeline(pkg, B, repeats, steps):
    """What the missing W = 2 build costs: bench.py's pipeline -- consecutive solves alternating between three streams, one handle
    each -- with the switch on and off on a table in which EVERY car is the handle's vehicle, so that the records, the QP kernel's work
    and the iterations are the same and only the linearisation kernel differs (256-register W = 2 form of lmpc_linearize_kernel, which
    fits beside a resident wave of the QP kernel, against the W = 1 lmpc_linearize_cars_kernel).  fp64 and single precision."""
    tr = pkg.workloads.synthetic_track("barc")
    x, u = pkg.workloads.sample_initial_states("barc", B, tr["L"], [-0.01, -0.314159], [0.01, 0.314159], seed=0)
    solvers = [pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0) for _ in range(3)]
    inp = solvers[0].prepare(solvers[0].device_track(tr), x.T.copy(), DT)
    inp["u_ic"] = torch.as_tensor(u.T.copy(), device="cuda")
    inp["L"] = float(tr["L"])
    inp32 = {k: (v.float().contiguous() if hasattr(v, "float") else v) for k, v in inp.items()}
    for sv in solvers:
        sv.set_car_vehicles([pkg.presets.barc_vehicle()] * B)
    streams = [torch.cuda.Stream() for _ in solvers]
    outs = [sv.alloc_outputs(B) for sv in solvers]
    outs32 = [sv.solve_f32(inp32) for sv in solvers]
    torch.cuda.synchronize()

    def run(on, f32, n):
        for sv in solvers:
            sv.set_cars_controller_model(on)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n):
            j = k % 3
            with torch.cuda.stream(streams[j]):
                solvers[j].solve_f32(inp32, outs32[j]) if f32 else solvers[j].solve(inp, outs[j])
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / n

    for f32 in (False, True):
        us = {False: [], True: []}
        for r in range(repeats + 1):
            for on in (False, True):
                t = run(on, f32, steps)
                if r:
                    us[on].append(t)
        a = report("%s, three streams, switch off" % ("lmpc_solve_batch_f32" if f32 else "lmpc_solve_batch"), us[False])
        b = report("%s, three streams, switch on" % ("lmpc_solve_batch_f32" if f32 else "lmpc_solve_batch"), us[True])
        print("on minus off: %.2f us a step (%.1f %%)" % (b - a, 100 * (b - a) / a))
    for sv in solvers:
        sv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("linearize", "solve", "period", "pipeline"), required=True)
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
    elif a.mode == "pipeline":
        pipeline(pkg, a.cars, a.repeats, a.steps)
    else:
        period(pkg, a.cars, a.repeats, a.steps)


if __name__ == "__main__":
    main()
