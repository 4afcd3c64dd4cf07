"""Closed-loop Monte-Carlo harness: thousands of cars driven by the batched MPC, entirely on the device.

One control period per iteration, as the reference's two nodes do it (step mode):
  RacingMPCNode::on_step_timer   shift previous plan, re-sample references, solve   (racing_mpc_node.cpp:236-320)
  RacingSimulatorNode / ::step   plant RK4 with the first input of the plan          (racing_simulator.cpp:97-112)
Everything (prepare / shift / linearise / solve / plant) is a HIP kernel behind the C ABI; this module only
sequences the calls and keeps a few statistics.  SURVEY.md 8d config 1 is this loop with batch = 1.
"""
from __future__ import annotations


def run(solver, track: dict, x0, u0, steps: int, dt: float = 0.025, n_sub: int = 2, speed_scale: float = 0.9,
        record_every: int = 0, restart_failed: bool = True, graph: bool = False, longest_first: bool = False, warm: bool = False,
        warm_rounds: int = 0, fused: bool = True):
    """x0 [6][B], u0 [2][B] (torch, device).  Returns final state and statistics (torch tensors on device).

    One control period = solve, apply the first input of the plan (on failure: of the shifted previous plan,
    racing_mpc_node.cpp:322-332), plant step, statistics, warm-start shift; a car whose QP failed is re-prepared from a
    cold start at its current state, as re-launching the node would (racing_mpc_node.cpp:210-235) -- a stale plan would
    make the next QP fail too.  Nothing in a period reads device data on the host.

    graph=True captures the period once as a HIP graph and replays it: a period is ~25 small launches around the QP
    kernel, and eager dispatch (~2 ms of host time) costs more than the 0.9 ms the GPU needs for them.

    warm=True solves with lmpc_solve_batch_warm: the shifted previous plan (what `inp["X_ref"]`, `inp["U_ref"]` hold from the second
    period on, racing_mpc_node.cpp:245-254) is tried as an active-set solve before any interior point.  Returns the share of
    solves that took that route as "warm_hit_rate" (iters <= 4: an attempt has four rounds at most and a refused one reports its
    rounds + the cold solve's iterations, five at least).  warm_rounds: lmpc_set_warm_rounds for this run (0: the library's default
    by batch size); the handle is back on the default afterwards.

    fused=True (default) does everything behind the solve -- input selection, plant step, statistics, shift or cold restart -- with
    one launch, lmpc_loop_advance_batch; fused=False goes through lmpc_plant_step_batch, lmpc_shift_batch, lmpc_prepare_failed_batch
    and torch element-wise operations (~45 launches per period), the same arithmetic (tests/test_gpu_loop.py: bit for bit but for 1 - 2 ulp on the last knot's rollout).

    longest_first=True launches the QP kernel's workgroups in the order of the previous period's iteration counts, longest
    first (lmpc_set_launch_order): a car's count changes little from one period to the next, and the long problems then
    no longer start last in the second residency round."""
    import torch

    trk = solver.device_track(track)
    L = float(track["L"])
    x = x0.clone()
    u_prev = u0.clone()
    B = x.shape[1]
    inp = solver.prepare(trk, x, dt, speed_scale=speed_scale)          # cold start (racing_mpc_node.cpp:210-235)
    out = solver.alloc_outputs(B)
    dist = torch.zeros(B, dtype=torch.float64, device=x.device)         # abscissa travelled (unwrapped)
    worst_excess = torch.zeros(B, dtype=torch.float64, device=x.device)  # max lateral excursion beyond the track edge
    n_fail = torch.zeros(B, dtype=torch.int64, device=x.device)
    hits = torch.zeros((), dtype=torch.int64, device=x.device)
    half_b = float(solver.vehicle["b"]) / 2.0
    keys = ("X_ref", "U_ref", "T_ref", "bound_left", "bound_right", "curvatures", "vel_ref")
    trace = []
    if warm:
        solver.set_warm_rounds(warm_rounds)
    order = None
    if longest_first:
        order = torch.arange(B, dtype=torch.int32, device=x.device)
        solver.set_launch_order(order)

    def period():
        inp["x_ic"] = x
        inp["u_ic"] = u_prev
        solver.solve(inp, out, warm=True if warm else None)
        if order is not None:
            solver.launch_order_from_iters(out["iters"], order)   # for the next period (in place: the pointer is registered)
        if fused:
            solver.loop_advance(trk, inp, out, x, u_prev, dt, dt / n_sub, n_sub, speed_scale=speed_scale, restart_failed=restart_failed,
                                distance=dist, worst_excess=worst_excess, n_fail=n_fail, n_accepted=hits if warm else None)
            return
        if warm:
            hits.add_(((out["status"] == 0) & (out["iters"] <= 4)).sum())   # (an attempt has 4 rounds at most; a cold solve takes 5 iterations at least)
        ok = out["status"] == 0
        n_fail.add_((~ok).to(torch.int64))
        u_apply = torch.where(ok[None, :], out["U_optm"][:, 0, :], inp["U_ref"][:, 0, :]).contiguous()
        s_before = x[0].clone()
        solver.plant_step(trk, x, u_apply, dt / n_sub, n_sub)
        ds = x[0] - s_before
        dist.add_(torch.where(ds < -L / 2, ds + L, ds))
        exc = torch.maximum(x[1] + half_b - inp["bound_left"][0], inp["bound_right"][0] - (x[1] - half_b))
        torch.maximum(worst_excess, exc, out=worst_excess)
        u_prev.copy_(u_apply)
        nxt = solver.shift(trk, inp, out, dt, speed_scale=speed_scale)
        if restart_failed:
            solver.prepare_failed(trk, x, out["status"], nxt, dt, speed_scale=speed_scale)
        for key in keys:
            inp[key].copy_(nxt[key])

    if not graph:
        for k in range(steps):
            period()
            if record_every and k % record_every == 0:
                trace.append(x.clone())
    else:
        if record_every:
            raise ValueError("record_every is not available with graph=True")
        done = 0
        side = torch.cuda.Stream(device=x.device)
        side.wait_stream(torch.cuda.current_stream(x.device))
        with torch.cuda.stream(side):           # warm-up outside the capture: workspace allocation, lazy initialisation
            if steps > 0:
                period()
                done = 1
        torch.cuda.current_stream(x.device).wait_stream(side)
        if steps > done:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                period()
            done += 1                               # (the capture does not execute; the first replay is that period)
            g.replay()
            for _ in range(steps - done):
                g.replay()
    if order is not None:
        torch.cuda.synchronize(x.device)
        solver.set_launch_order(None)
    if warm and warm_rounds:
        solver.set_warm_rounds(0)
    return {"x": x, "distance": dist, "worst_excess": worst_excess, "n_fail": n_fail, "trace": trace,
            "warm_hit_rate": (float(hits) / (B * max(steps, 1))) if warm else None}


def run_global(solver, track: dict, spline, x0, u0, steps: int, dt: float = 0.025, n_sub: int = 2, speed_scale: float = 0.9,
               restart_failed: bool = True, warm: bool = False):
    """`run` (fused) with the state crossing the GLOBAL frame every period, as it does between the reference's simulator node and its
    controller node: after lmpc_loop_advance_batch the cars' (s, e_y, e_psi) go to poses (x, y, yaw) with lmpc_frenet_to_global_batch
    (racing_simulator_node.cpp:273-278), the poses are projected back with lmpc_global_to_frenet_batch started from the abscissa they
    came from (racing_mpc_node.cpp:181-185, initialize_with_previous), and the result replaces x[0:3] -- two more launches per period,
    no host round trip.  `spline`: Solver.spline_track of the track whose tables `track` holds.  Returns run's statistics and
    "track_status": int32 [B], the largest projection status a car has seen (0: every projection converged)."""
    import torch

    trk = solver.device_track(track)
    x, u_prev = x0.clone(), u0.clone()
    B = x.shape[1]
    inp = solver.prepare(trk, x, dt, speed_scale=speed_scale)
    out = solver.alloc_outputs(B)
    kw = dict(dtype=torch.float64, device=x.device)
    dist, worst_excess = torch.zeros(B, **kw), torch.zeros(B, **kw)
    n_fail = torch.zeros(B, dtype=torch.int64, device=x.device)
    hits = torch.zeros((), dtype=torch.int64, device=x.device)
    pose, frenet = torch.empty((3, B), **kw), torch.empty((3, B), **kw)
    status = torch.empty(B, dtype=torch.int32, device=x.device)
    track_status = torch.zeros(B, dtype=torch.int32, device=x.device)
    for _ in range(steps):
        inp["x_ic"], inp["u_ic"] = x, u_prev
        solver.solve(inp, out, warm=True if warm else None)
        solver.loop_advance(trk, inp, out, x, u_prev, dt, dt / n_sub, n_sub, speed_scale=speed_scale, restart_failed=restart_failed,
                            distance=dist, worst_excess=worst_excess, n_fail=n_fail, n_accepted=hits if warm else None)
        solver.frenet_to_global(spline, x, out=pose)
        solver.global_to_frenet(spline, pose, s0=x[0], out=(frenet, status))
        x[0:3].copy_(frenet)
        torch.maximum(track_status, status, out=track_status)
    return {"x": x, "distance": dist, "worst_excess": worst_excess, "n_fail": n_fail, "track_status": track_status,
            "warm_hit_rate": (float(hits) / (B * max(steps, 1))) if warm else None}


SENSORS = {"sig_vel": (0.05, 0.05), "sig_pose": (0.02, 0.02, 0.01), "dropout": 0.1, "sd0": (0.5, 0.5, 0.3, 0.5, 0.2, 0.5),
           "Q": (1e-4, 1e-4, 1e-4, 1e-2, 1e-2, 1e-2), "clip": (6.0, 1.5, 20.0)}


def run_estimated(solver, track: dict, spline, x0, u0, steps: int, dt: float = 0.025, n_sub: int = 2, speed_scale: float = 0.9,
                  restart_failed: bool = True, sensors: dict | None = None, seed: int = 0, record_trace: bool = False):
    """The sensor -> estimate -> projection -> solve -> plant chain: `run_global` with the controller fed by the batched extended Kalman
    filter (lmpc_ekf_*, one filter per car on the device) instead of the plant's exact state.  The filter's state is the global one,
    [X, Y, yaw, vx, vy, omega].  Per period:
      the estimate is projected to the Frenet frame (lmpc_global_to_frenet_batch, started from its previous abscissa) and is the
      controller's x_ic; solve; the first input of the plan (on failure: of the shifted previous plan) goes to the plant AND to the
      filter (update_control);
      the TRUTH advances half a period (lmpc_plant_step_batch) and its (vx, omega) plus noise is the velocity observation (rows 3, 5);
      it advances the other half, goes to a pose (lmpc_frenet_to_global_batch), and pose plus noise -- yaw in (-pi, pi], x = NaN for the
      cars whose pose drops out this period -- is the pose observation (rows 0, 1, 2);
      the next period's inputs are the shifted plan (lmpc_shift_batch) and, for a car whose solve failed, a cold start AT THE NEW
      ESTIMATE (lmpc_prepare_failed_batch).  The controller never sees the truth.
    These are the unfused entry points: lmpc_loop_advance_batch steps the plant from the state the controller was given.
    sensors: overrides of SENSORS -- noise sigmas, the dropout rate, the start's standard deviations sd0 (the filters start at truth +
    0.5 N(0, 1) sd0 with vx floored at 0.5, P0 = diag(sd0^2)), the diagonal of Q, the clip of (vx, vy, omega).  The noise comes from a
    torch.Generator on the device seeded with `seed`.  n_sub must be even.  The model is stiff at low speed (include/lmpc_hip.h at
    lmpc_ekf_create): keep the cars above 1.5 m/s for estimates that do not depend on rounding.
    Returns run_global's statistics (of the truth), "x_est" [6][B] the last estimate, "rms_error" [6] the RMS of estimate - truth in
    the global frame over all cars and periods (yaw difference wrapped), "ekf_flags" int32 [B] the OR of every update's flags, and
    "x_est0" / "P0" / "ekf_config" the filters' start; record_trace=True adds "trace": per update (obs_id, z, R, u, timestamp_ns,
    x_est) with device tensors -- enough to replay the filters, which are open-loop in (u, z, t)."""
    import math

    import torch

    if n_sub % 2:
        raise ValueError("run_estimated: n_sub must be even (the velocity observation sits at mid-period)")
    sn = dict(SENSORS, **(sensors or {}))
    trk = solver.device_track(track)
    L = float(track["L"])
    x, u_prev = x0.clone(), u0.clone()
    B, dev = x.shape[1], x.device
    kw = dict(dtype=torch.float64, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    col = lambda v: torch.as_tensor(v, **kw)[:, None]  # noqa: E731
    sig_v, sig_p, sd0 = col(sn["sig_vel"]), col(sn["sig_pose"]), col(sn["sd0"])
    R_v = torch.diag(sig_v[:, 0] ** 2)[:, :, None].repeat(1, 1, B).contiguous()
    R_p = torch.diag(sig_p[:, 0] ** 2)[:, :, None].repeat(1, 1, B).contiguous()
    inf = math.inf
    cfg = {"x0": [0.0] * 6, "P0": torch.diag(sd0[:, 0] ** 2).cpu().numpy(), "Q": torch.diag(torch.as_tensor(sn["Q"], dtype=torch.float64)).numpy(),
           "x_min": [-inf] * 3 + [-float(c) for c in sn["clip"]], "x_max": [inf] * 3 + [float(c) for c in sn["clip"]]}
    solver.ekf_create(B, **cfg)
    o_vel, o_pose = solver.ekf_register_observation((3, 5)), solver.ekf_register_observation((0, 1, 2))
    pose = solver.frenet_to_global(spline, x)
    x_est = torch.cat([pose, x[3:6]]) + 0.5 * torch.randn((6, B), generator=gen, **kw) * sd0
    x_est[3].clamp_(min=0.5)
    x_est0 = x_est.clone()
    P0 = torch.diag(sd0[:, 0] ** 2)[:, :, None].repeat(1, 1, B).contiguous()
    solver.ekf_set_state(x_est, P0)
    solver.ekf_initialize(0)
    frenet, status = solver.global_to_frenet(spline, x_est[0:3].contiguous())
    track_status = status.clone()
    x_ic = torch.cat([frenet, x_est[3:6]]).contiguous()
    inp = solver.prepare(trk, x_ic, dt, speed_scale=speed_scale)
    out = solver.alloc_outputs(B)
    dist, worst_excess = torch.zeros(B, **kw), torch.zeros(B, **kw)
    n_fail = torch.zeros(B, dtype=torch.int64, device=dev)
    flags_or = torch.zeros(B, dtype=torch.int32, device=dev)
    sq_err = torch.zeros(6, **kw)
    half_b = float(solver.vehicle["b"]) / 2.0
    dt_ns = int(round(dt * 1e9))
    trace = []
    for k in range(steps):
        inp["x_ic"], inp["u_ic"] = x_ic, u_prev
        solver.solve(inp, out)
        ok = out["status"] == 0
        n_fail.add_((~ok).to(torch.int64))
        u_apply = torch.where(ok[None, :], out["U_optm"][:, 0, :], inp["U_ref"][:, 0, :]).contiguous()
        solver.ekf_update_control(u_apply)
        s_before = x[0].clone()
        solver.plant_step(trk, x, u_apply, dt / n_sub, n_sub // 2)
        z_v = (x[[3, 5]] + sig_v * torch.randn((2, B), generator=gen, **kw)).contiguous()
        ts = k * dt_ns + dt_ns // 2
        xe, _, _, fl = solver.ekf_update(o_vel, z_v, R_v, ts)
        flags_or |= fl
        if record_trace:
            trace.append((o_vel, z_v, R_v, u_apply, ts, xe))
        solver.plant_step(trk, x, u_apply, dt / n_sub, n_sub // 2)
        ds = x[0] - s_before
        dist.add_(torch.where(ds < -L / 2, ds + L, ds))
        exc = torch.maximum(x[1] + half_b - inp["bound_left"][0], inp["bound_right"][0] - (x[1] - half_b))
        torch.maximum(worst_excess, exc, out=worst_excess)
        pose = solver.frenet_to_global(spline, x)
        z_p = pose + sig_p * torch.randn((3, B), generator=gen, **kw)
        z_p[2] = torch.atan2(torch.sin(z_p[2]), torch.cos(z_p[2]))
        z_p[0] = torch.where(torch.rand((B,), generator=gen, **kw) < float(sn["dropout"]), torch.full((B,), math.nan, **kw), z_p[0])
        ts = (k + 1) * dt_ns
        x_est, _, _, fl = solver.ekf_update(o_pose, z_p, R_p, ts)
        flags_or |= fl
        if record_trace:
            trace.append((o_pose, z_p, R_p, u_apply, ts, x_est))
        err = x_est - torch.cat([pose, x[3:6]])
        err[2] = torch.atan2(torch.sin(err[2]), torch.cos(err[2]))
        sq_err += (err ** 2).mean(dim=1)
        # the next period's controller state: the new estimate in the Frenet frame, projected from its previous abscissa
        frenet, status = solver.global_to_frenet(spline, x_est[0:3].contiguous(), s0=x_ic[0].contiguous())
        torch.maximum(track_status, status, out=track_status)
        x_ic = torch.cat([frenet, x_est[3:6]]).contiguous()
        u_prev = u_apply
        nxt = solver.shift(trk, inp, out, dt, speed_scale=speed_scale)
        if restart_failed:
            solver.prepare_failed(trk, x_ic, out["status"], nxt, dt, speed_scale=speed_scale)
        inp = nxt
    res = {"x": x, "distance": dist, "worst_excess": worst_excess, "n_fail": n_fail, "track_status": track_status, "warm_hit_rate": None,
           "x_est": x_est, "rms_error": torch.sqrt(sq_err / max(steps, 1)), "ekf_flags": flags_or, "x_est0": x_est0, "P0": P0, "ekf_config": cfg}
    if record_trace:
        res["trace"] = trace
    return res


def run_estimated_fused(solver, track: dict, spline, x0, u0, steps: int, dt: float = 0.025, n_sub: int = 2, speed_scale: float = 0.9,
                        restart_failed: bool = True, sensors: dict | None = None, seed: int = 0, record_trace: bool = False, poll: int = 0):
    """`run_estimated` with everything between two solves in ONE launch, lmpc_loop_advance_estimated_batch
    (include/lmpc_hip_estimated.h): a period is the solve and that call, with no torch operation on the stream between them.  The same
    arguments and result keys.  The noise is drawn from the same torch.Generator in the same order -- randn(6, B) for the start, then
    per period randn(2, B), randn(3, B), rand(B) -- and a dropout is a NaN in noise_pose[0], so the two loops see identical sensors;
    the statistics differ from run_estimated's only by the rounding of the fused kernel's arithmetic and by "rms_error" summing the
    cars last (per-car sums of squares on the device, one mean at the end).
    poll: how many periods run between host reads.  The loop itself reads nothing back; every `poll` periods the host waits for the
    stream (which bounds the queue of launches and noise buffers ahead of the device), and poll = 0 waits once, at the end.
    record_trace=True adds "trace" as run_estimated does, from per-period output buffers of the call; the estimate after a velocity
    update is not an output of the fused call, so that entry's last member is None."""
    import math

    import torch

    if n_sub % 2:
        raise ValueError("run_estimated_fused: n_sub must be even (the velocity observation sits at mid-period)")
    sn = dict(SENSORS, **(sensors or {}))
    trk = solver.device_track(track)
    x, u_prev = x0.clone(), u0.clone()
    B, dev = x.shape[1], x.device
    kw = dict(dtype=torch.float64, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    col = lambda v: torch.as_tensor(v, **kw)[:, None]  # noqa: E731
    sig_v, sig_p, sd0 = col(sn["sig_vel"]), col(sn["sig_pose"]), col(sn["sd0"])
    R_v = torch.diag(sig_v[:, 0] ** 2)[:, :, None].repeat(1, 1, B).contiguous()
    R_p = torch.diag(sig_p[:, 0] ** 2)[:, :, None].repeat(1, 1, B).contiguous()
    inf = math.inf
    cfg = {"x0": [0.0] * 6, "P0": torch.diag(sd0[:, 0] ** 2).cpu().numpy(), "Q": torch.diag(torch.as_tensor(sn["Q"], dtype=torch.float64)).numpy(),
           "x_min": [-inf] * 3 + [-float(c) for c in sn["clip"]], "x_max": [inf] * 3 + [float(c) for c in sn["clip"]]}
    solver.ekf_create(B, **cfg)
    o_vel, o_pose = solver.ekf_register_observation((3, 5)), solver.ekf_register_observation((0, 1, 2))
    pose = solver.frenet_to_global(spline, x)
    x_est = torch.cat([pose, x[3:6]]) + 0.5 * torch.randn((6, B), generator=gen, **kw) * sd0
    x_est[3].clamp_(min=0.5)
    x_est0 = x_est.clone()
    P0 = torch.diag(sd0[:, 0] ** 2)[:, :, None].repeat(1, 1, B).contiguous()
    solver.ekf_set_state(x_est, P0)
    solver.ekf_initialize(0)
    frenet, status = solver.global_to_frenet(spline, x_est[0:3].contiguous())
    track_status = status.clone()
    x_ic = torch.cat([frenet, x_est[3:6]]).contiguous()
    inp = solver.prepare(trk, x_ic, dt, speed_scale=speed_scale)
    out = solver.alloc_outputs(B)
    dist, worst_excess = torch.zeros(B, **kw), torch.zeros(B, **kw)
    n_fail = torch.zeros(B, dtype=torch.int64, device=dev)
    flags_or = torch.zeros(B, dtype=torch.int32, device=dev)
    sq_err = torch.zeros((6, B), **kw)
    dt_ns = int(round(dt * 1e9))
    dropout = float(sn["dropout"])
    nan = torch.full((B,), math.nan, **kw)
    trace = []
    stream = torch.cuda.current_stream(dev)
    for k in range(steps):
        inp["x_ic"], inp["u_ic"] = x_ic, u_prev
        solver.solve(inp, out)
        # this period's sensors, in run_estimated's order of draws (fresh buffers: the launch that reads them is only queued)
        noise_v = (sig_v * torch.randn((2, B), generator=gen, **kw)).contiguous()
        noise_p = (sig_p * torch.randn((3, B), generator=gen, **kw)).contiguous()
        noise_p[0] = torch.where(torch.rand((B,), generator=gen, **kw) < dropout, nan, noise_p[0])
        ts_v, ts_p = k * dt_ns + dt_ns // 2, (k + 1) * dt_ns
        rec = dict(x_est=x_est)
        if record_trace:
            rec = dict(x_est=torch.empty((6, B), **kw), z_vel=torch.empty((2, B), **kw), z_pose=torch.empty((3, B), **kw))
            u_rec = torch.empty((2, B), **kw)
        solver.loop_advance_estimated(trk, spline, inp, out, x, u_rec if record_trace else u_prev, x_ic, dt, dt / n_sub, n_sub, o_vel, o_pose,
                                      ts_v, ts_p, noise_v, R_v, noise_p, R_p, speed_scale=speed_scale, restart_failed=restart_failed,
                                      ekf_flags=flags_or, track_status=track_status, distance=dist, worst_excess=worst_excess, n_fail=n_fail,
                                      sq_err=sq_err, **rec)
        if record_trace:
            u_prev = u_rec
            x_est = rec["x_est"]
            trace.append((o_vel, rec["z_vel"], R_v, u_rec, ts_v, None))
            trace.append((o_pose, rec["z_pose"], R_p, u_rec, ts_p, x_est))
        if poll and (k + 1) % poll == 0:
            stream.synchronize()
    stream.synchronize()
    res = {"x": x, "distance": dist, "worst_excess": worst_excess, "n_fail": n_fail, "track_status": track_status, "warm_hit_rate": None,
           "x_est": x_est, "rms_error": torch.sqrt(sq_err.mean(dim=1) / max(steps, 1)), "ekf_flags": flags_or, "x_est0": x_est0, "P0": P0,
           "ekf_config": cfg}
    if record_trace:
        res["trace"] = trace
    return res


def record_laps(solver, track: dict, speed_scales=(0.80, 0.85, 0.90, 0.95, 1.0), dt: float = 0.03, n_sub: int = 3):
    """The laps SURVEY.md 8d config 3 stores in the safe set: "running config 1's tracking loop for 5 laps with seed-indexed speed
    scales {0.80, 0.85, 0.90, 0.95, 1.0}", one sample per 0.03 s (the recorder's period upstream, racing_mpc_node.cpp:66).  One
    car per scale from the start line at the profile's speed, driven by `solver` (a tracking handle) until it has covered one lap;
    the samples of that lap are returned as host arrays [n][6], oldest (slowest) first -- what SafeSetRecorder would have written."""
    import numpy as np
    import torch

    L, M = float(track["L"]), int(track["M"])
    laps = []
    for sc in speed_scales:
        v0 = max(float(np.asarray(track["vel"])[0]) * sc, 0.5)
        x0 = torch.tensor([[0.0], [0.0], [0.0], [v0], [0.0], [0.0]], dtype=torch.float64, device=solver.device)
        u0 = torch.zeros((2, 1), dtype=torch.float64, device=solver.device)
        v_min = max(float(np.asarray(track["vel"]).min()) * sc * 0.8, 0.4)
        steps = int(1.25 * L / (v_min * dt)) + 8
        r = run(solver, track, x0, u0, steps=steps, dt=dt, n_sub=n_sub, speed_scale=sc, record_every=1)
        xs = np.stack([x0.cpu().numpy()[:, 0]] + [t.cpu().numpy()[:, 0] for t in r["trace"]])     # [steps + 1][6], abscissa wrapped
        ds = np.diff(xs[:, 0])
        ds = np.where(ds < -L / 2, ds + L, ds)
        travelled = np.concatenate([[0.0], np.cumsum(ds)])
        n = int(np.searchsorted(travelled, L))       # first sample past the line: the lap is samples 0 .. n-1
        if n >= xs.shape[0]:
            raise RuntimeError("record_laps: the car at speed scale %.2f did not complete a lap in %d periods" % (sc, steps))
        laps.append(xs[:n].copy())
    return laps


def run_lmpc(tracker, learner, track: dict, x0, u0, warm_laps: int = 2, learn_laps: int = 4, dt: float = 0.025,
             n_sub: int = 2, warm_speed_scale: float = 0.7, max_steps: int = 20000, debug: bool = False, warm: bool = False,
             advance: int = 1):
    """The LMPC experiment of the reference (sim_barc_lmpc): `warm_laps` laps under the tracking MPC fill the safe
    set, then the learning MPC drives and every completed lap of car 0 is added to the set (SafeSetRecorder ->
    SafeSetManager -> device store).  All B cars share car 0's safe set.  Returns car 0's lap times (tracking laps
    first) and per-car statistics.  x0 [6][B], u0 [2][B] on the device.

    warm=True (round 6): the learning solves go through lmpc_solve_batch_warm_ss -- the shifted previous plan and the previous
    solution's simplex weights (racing_mpc.cpp:281, 293-305), the safe set by reference, the weights carried onto the new period's
    points by lmpc_shift_lambda_batch (`advance` samples along the lap); the tracking laps through lmpc_solve_batch_warm.  Returns
    the share of the learning solves whose active-set attempt was accepted as "warm_hit_rate"."""
    import numpy as np
    import torch

    from . import safe_set as SS

    trk = tracker.device_track(track)
    L = float(track["L"])
    B = x0.shape[1]
    man = SS.SafeSetManager(int(learner.config["max_lap_stored"]))
    rec = SS.SafeSetRecorder(man)
    x, u_prev = x0.clone(), u0.clone()
    half_b = float(tracker.vehicle["b"]) / 2.0
    worst_excess = torch.zeros(B, dtype=torch.float64, device=x.device)
    n_fail = torch.zeros(B, dtype=torch.int64, device=x.device)
    lap_times, lap_kind, t_lap_start, t = [], [], None, 0.0
    debug_left = [12]
    solver, learning = tracker, False
    inp = solver.prepare(trk, x, dt, speed_scale=warm_speed_scale)
    out = solver.alloc_outputs(B)
    S = int(learner.config["num_ss_pts"])
    lam = torch.zeros((S, B), dtype=torch.float64, device=x.device)
    curv0 = np.asarray(track["curvature"], dtype=np.float64)
    # The state box also applies to knot 0 (racing_mpc.cpp:147,201), so a plant that lands a hair outside an active
    # bound (the QP rides vx = vx_max; the nonlinear plant overshoots by the linearisation error) would make every
    # following problem infeasible.  The harness hands the controller the measured state projected onto the box.
    x_lo = torch.as_tensor(learner.config["x_min"], dtype=torch.float64, device=x.device)[:, None]
    x_hi = torch.as_tensor(learner.config["x_max"], dtype=torch.float64, device=x.device)[:, None]
    idx_prev, have_prev, n_warm, n_hit = None, False, 0, 0
    acc = torch.zeros(B, dtype=torch.int32, device=x.device)
    for k in range(max_steps):
        inp["x_ic"], inp["u_ic"] = (torch.minimum(torch.maximum(x, x_lo), x_hi) if learning else x), u_prev
        # car 0 feeds the recorder (RacingMPC::solve, racing_mpc.cpp:246): state, applied input, curvature, time
        x_h = x[:, 0].cpu().numpy()
        k_h = float(np.interp(x_h[0] % L, np.arange(curv0.size) * L / curv0.size, curv0, period=L))
        if rec.step(x_h, u_prev[:, 0].cpu().numpy(), k_h, t, L):
            lap_times.append(t - t_lap_start)
            lap_kind.append("lmpc" if learning else "tracking")
            man.sync(learner)
            have_prev = False   # (the store was replaced: the previous period's codes no longer name its rows)
            if not learning and len(man.laps) >= warm_laps:
                solver, learning = learner, True
                out = solver.alloc_outputs(B)
                out["convex_combi_optm"] = lam
            if learning and lap_kind.count("lmpc") >= learn_laps:
                break
        if rec.initialized and (t_lap_start is None or rec.x and len(rec.x) == 1):
            t_lap_start = t
        if learning:
            # query = last knot of the abscissa-aligned reference (racing_mpc.cpp:219-223,249-254)
            s_last, s0 = inp["X_ref"][0, -1], x[0]
            kk = (s0 - s_last).abs() + L / 2
            q = torch.stack([s_last + (kk - torch.fmod(kk, L)) * torch.sign(s0 - s_last), inp["X_ref"][1, -1]]).contiguous()
            if warm:
                idx, _ = solver.ss_query_idx(q)
                idx = idx.clone()  # (kept for the next period's weight transfer)
                if have_prev:
                    lam_ref = solver.shift_lambda(idx_prev, lam, idx, advance)
                    solver.solve(inp, out, ss_idx=idx, warm={"X_optm_ref": inp["X_ref"], "U_optm_ref": inp["U_ref"], "convex_combi_optm_ref": lam_ref})
                    solver.warm_accepted(B, acc)
                    n_warm += B
                    n_hit += int(acc.sum())
                else:
                    solver.solve(inp, out, ss_idx=idx)
                idx_prev = idx
            else:
                ss_x, ss_j, _ = solver.ss_query(q)
                solver.solve(inp, out, ss_x=ss_x, ss_j=ss_j)
        else:
            solver.solve(inp, out, warm=True if (warm and k > 0) else None)
        ok = out["status"] == 0
        n_fail += (~ok).to(torch.int64)
        if learning and warm:
            have_prev = bool(ok.all()) or True   # (a failed car's weights are stale; its attempt is refused by the KKT test, nothing else)
        if debug and learning and not bool(ok[0]) and debug_left[0] > 0:
            debug_left[0] -= 1
            print("step", k, "t %.3f" % t, "car0 status", int(out["status"][0]), "iters", int(out["iters"][0]), "x", x[:, 0].cpu().numpy().round(3),
                  "u_prev", u_prev[:, 0].cpu().numpy().round(4), "Xref vx %.2f..%.2f" % (float(inp["X_ref"][3, :, 0].min()), float(inp["X_ref"][3, :, 0].max())))
        u_apply = torch.where(ok[None, :], out["U_optm"][:, 0, :], inp["U_ref"][:, 0, :]).contiguous()
        solver.plant_step(trk, x, u_apply, dt / n_sub, n_sub)
        exc = torch.maximum(x[1] + half_b - inp["bound_left"][0], inp["bound_right"][0] - (x[1] - half_b))
        worst_excess = torch.maximum(worst_excess, exc)
        u_prev = u_apply
        inp = solver.shift(trk, inp, out, dt, speed_scale=warm_speed_scale if not learning else 1.0)
        t += dt
    return {"lap_times": lap_times, "lap_kind": lap_kind, "worst_excess": worst_excess, "n_fail": n_fail, "steps": k + 1,
            "laps_in_set": len(man.laps), "x": x, "warm_hit_rate": (n_hit / n_warm) if n_warm else None}


def _check_plants(plant, plants, B: int, who: str, what: str = "plants"):
    if plants is not None and plant is not None:
        raise ValueError(who + ": " + what + "= (one vehicle per car) and plant= (one for all) are exclusive")
    if plants is not None and len(plants) != B:
        raise ValueError(who + ": " + what + "= holds %d vehicles for %d cars" % (len(plants), B))


class _CarsPlant:
    """run_lmpc_fleet's `plant` for plants=: plant_step is the solver's plant_step_cars (car b stepped by vehicle b of its car table)."""

    def __init__(self, solver):
        self.plant_step = solver.plant_step_cars


class _DtrackPlant:
    """run_lmpc_fleet's `plant` for plants_dt=: plant_step is the solver's plant_step_dtrack (car b stepped by the four-wheel vehicle
    b of its double-track table)."""

    def __init__(self, solver):
        self.plant_step = solver.plant_step_dtrack


def _with_dtrack_controllers(run, who, tracker, learner, B, controllers_dt, plants_dt, regression):
    """controllers_dt= of run_lmpc_fleet / run_lmpc_fleet_fused: the list is the double-track table of both handles and both solve on
    it (Solver.set_dtrack_controller_model) while `run` runs; switch and tables are off again on the way out, whatever happened."""
    if regression is not None:
        raise ValueError(who + ": controllers_dt= and regression= are exclusive (the regression corrects the single-track model)")
    if plants_dt is not None and plants_dt is not controllers_dt and list(plants_dt) != list(controllers_dt):
        raise ValueError(who + ": the plant reads the learner's double-track table, so plants_dt= and controllers_dt= must be the same list")
    _check_plants(None, controllers_dt, B, who, "controllers_dt")
    try:
        for sv in (tracker, learner):
            sv.set_dtrack_vehicles(controllers_dt)
            sv.set_dtrack_controller_model(True)
        return run()
    finally:
        for sv in (tracker, learner):
            sv.set_dtrack_controller_model(False)
            sv.set_dtrack_vehicles(None)


def _with_cars_controllers(run, who, tracker, learner, B, controllers, plant, plants, plants_dt, controllers_dt, regression):
    """controllers= of run_lmpc_fleet / run_lmpc_fleet_fused: the list is the car table of both handles and both solve on it
    (Solver.set_cars_controller_model) while `run(plants)` runs; switch and tables are off again on the way out, whatever happened."""
    if regression is not None:
        raise ValueError(who + ": controllers= and regression= are exclusive (the regression corrects the handle's vehicle)")
    if controllers_dt is not None or plants_dt is not None:
        raise ValueError(who + ": controllers= (single-track cars) is exclusive with controllers_dt= and plants_dt= (double-track cars)")
    if plant is not None:
        raise ValueError(who + ": controllers= and plant= are exclusive (a handle with a car table steps its plant with that table)")
    if plants is not None and plants is not controllers and list(plants) != list(controllers):
        raise ValueError(who + ": the plant reads the learner's car table, so plants= and controllers= must be the same list")
    _check_plants(None, controllers, B, who, "controllers")
    try:
        for sv in (tracker, learner):
            sv.set_car_vehicles(controllers)
            sv.set_cars_controller_model(True)
        return run(controllers)
    finally:
        for sv in (tracker, learner):
            sv.set_cars_controller_model(False)
            sv.set_car_vehicles(None)


def run_lmpc_fleet(tracker, learner, track: dict, x0, u0, warm_laps: int = 2, learn_laps: int = 4, dt: float = 0.025,
                   n_sub: int = 2, warm_speed_scale: float = 0.7, max_steps: int = 20000, max_pts_per_lap: int = 1024,
                   record_trace: bool = False, regression: dict | None = None, plant=None, plants=None, plants_dt=None,
                   warmup: dict | None = None, _warm_plant: str = "handle", controllers_dt=None, controllers=None):
    """run_lmpc with every car learning from ITS OWN laps: the fleet safe set on `learner` (lmpc_fleet_ss_*: one recorder and one
    ring of max_lap_stored laps per car, on the device) replaces the host recorder of car 0 and the shared store.  Per period, in
    run_lmpc's order: record (x, u_prev, curvature at s, t) for all cars, query every learning car's own ring, solve, plant step,
    shift.  Car b switches from the tracking to the learning controller when its own ring holds `warm_laps` laps; while the fleet is
    mixed both controllers solve the batch and results and shifted inputs are selected per car (the cars not learning yet pass
    through the learning kernel on the zero-filled set the query writes for an empty ring, and their status from it is ignored);
    when all cars are in one phase only that controller runs.  Stops when every car has `learn_laps` learning laps, or at max_steps.

    No state is copied to the host: lap times and kinds are kept on the device from lmpc_fleet_ss_stats (a lap's kind is the phase
    its car drove it in; the lap at whose close a car switches is still "tracking").  The host reads one small int32 tensor per
    period -- laps_in_ring [B] and, beside it, the per-car "has its learning laps" flag -- to decide which controllers to launch.

    Returns "lap_times" / "lap_kind": per car the list of its closed laps in order (at most warm_laps + learn_laps + 8 are kept),
    device tensors "worst_excess", "n_fail" (failures of the controller the car was driving with), "n_dropped", "laps_in_ring", and
    "steps", "x"; record_trace=True adds "trace", the (x, u, k, t) handed to the recorder each period.

    regression (a dict of Solver.fleet_ss_set_regression's keyword arguments): the learning controller also corrects each car's model
    by the error-dynamics regression on that car's own closed laps (it is switched on on `learner`, and stays on after the run).
    plant (a Solver): its plant_step drives the cars instead of the controllers' -- a plant whose vehicle differs from the
    controllers' gives the regression something to learn.
    plants (a list of B vehicle dicts, exclusive with plant=): car b drives on plants[b] -- the list becomes `learner`'s car table
    (Solver.set_car_vehicles) for the run, every period steps with its plant_step_cars, and the table is cleared at the end.
    plants_dt (a list of B double-track vehicle dicts, presets.barc_double_track's keys; exclusive with plant= and plants=): car b
    drives on the FOUR-WHEEL model with plants_dt[b] while the controllers stay single-track -- the list becomes `learner`'s
    double-track table (Solver.set_dtrack_vehicles) for the run, every period steps with its plant_step_dtrack, and the table is
    cleared at the end.
    warmup (a dict, _fleet_warm_up's): the warm laps are driven by the vanilla controller on the run's own plants in a few launches
    (warm_up_vanilla) instead of by the tracking controller; the loop starts where they end, with its clock at their end, and
    "lap_times" / "lap_kind" list only the laps closed after them, and "warmup" = {"periods", "t_end", "lap_count"} says where they
    ended.  None: the run as it always was.
    controllers_dt (a list of B double-track vehicle dicts, usually plants_dt's list): the CONTROLLERS' model -- the list is the
    double-track table of both handles and both solve on it, problem b linearised on controllers_dt[b]
    (Solver.set_dtrack_controller_model); switch and tables are off again on return.  The plant reads the learner's table, so with
    plants_dt= it must be the same list, and it is exclusive with regression=: ValueError otherwise.
    controllers (a list of B single-track vehicle dicts, usually plants=' list): the CONTROLLERS' model on single-track cars -- the
    list is the car table of both handles and both solve on it, problem b linearised on controllers[b]
    (Solver.set_cars_controller_model); switch and tables are off again on return.  The plant reads the learner's table: the cars
    drive on the same list (plants= may be left out; where it is given it must be the same list), and controllers= is exclusive with
    plant=, regression=, controllers_dt= and plants_dt=: ValueError otherwise.  Boxes, reference rollouts and worst_excess's body width
    stay on the handles' vehicle (include/lmpc_hip_cars_model.h)."""
    import numpy as np
    import torch

    B = x0.shape[1]
    if controllers is not None:
        return _with_cars_controllers(
            lambda same: run_lmpc_fleet(tracker, learner, track, x0, u0, warm_laps, learn_laps, dt, n_sub, warm_speed_scale, max_steps,
                                        max_pts_per_lap, record_trace, None, None, same, None, warmup, _warm_plant),
            "run_lmpc_fleet", tracker, learner, B, controllers, plant, plants, plants_dt, controllers_dt, regression)
    if controllers_dt is not None:
        return _with_dtrack_controllers(
            lambda: run_lmpc_fleet(tracker, learner, track, x0, u0, warm_laps, learn_laps, dt, n_sub, warm_speed_scale, max_steps, max_pts_per_lap,
                                   record_trace, regression, plant, plants, plants_dt, warmup, _warm_plant),
            "run_lmpc_fleet", tracker, learner, B, controllers_dt, plants_dt, regression)
    if warmup is not None and plant is not None and _warm_plant == "handle":
        raise ValueError("run_lmpc_fleet: warmup= drives the warm laps on the learner's vehicle, plants= or plants_dt=, not on plant=")
    if plants_dt is not None:
        if plants is not None:
            raise ValueError("run_lmpc_fleet: plants= (single-track cars) and plants_dt= (double-track cars) are exclusive")
        _check_plants(plant, plants_dt, B, "run_lmpc_fleet", "plants_dt")
        learner.set_dtrack_vehicles(plants_dt)
        try:
            return run_lmpc_fleet(tracker, learner, track, x0, u0, warm_laps, learn_laps, dt, n_sub, warm_speed_scale, max_steps, max_pts_per_lap,
                                  record_trace, regression, plant=_DtrackPlant(learner), warmup=warmup, _warm_plant="dtrack")
        finally:
            learner.set_dtrack_vehicles(None)
    _check_plants(plant, plants, B, "run_lmpc_fleet")
    if plants is not None:
        learner.set_car_vehicles(plants)
        try:
            return run_lmpc_fleet(tracker, learner, track, x0, u0, warm_laps, learn_laps, dt, n_sub, warm_speed_scale, max_steps, max_pts_per_lap,
                                  record_trace, regression, plant=_CarsPlant(learner), warmup=warmup, _warm_plant="cars")
        finally:
            learner.set_car_vehicles(None)
    trk = tracker.device_track(track)
    L = float(track["L"])
    dev = x0.device
    learner.fleet_ss_create(B, max_pts_per_lap)
    if regression is not None:
        learner.fleet_ss_set_regression(**regression)
    x, u_prev = x0.clone(), u0.clone()
    t_start, laps_before, warmed = 0.0, np.zeros(B, dtype=np.int64), {}
    if warmup is not None:
        x, u_prev, t_start, laps_before = _fleet_warm_up(learner, trk, x, u_prev, warm_laps, dt, n_sub, warmup, _warm_plant)
        warmed = {"warmup": {"periods": int(round(t_start / dt)), "t_end": t_start, "lap_count": laps_before}}
    half_b = float(tracker.vehicle["b"]) / 2.0
    worst_excess = torch.zeros(B, dtype=torch.float64, device=dev)
    n_fail = torch.zeros(B, dtype=torch.int64, device=dev)
    inp = tracker.prepare(trk, x, dt, speed_scale=warm_speed_scale)
    out_t, out_l = tracker.alloc_outputs(B), learner.alloc_outputs(B)
    S = int(learner.config["num_ss_pts"])
    out_l["convex_combi_optm"] = torch.zeros((S, B), dtype=torch.float64, device=dev)
    ss_buf = (torch.zeros((6, S, B), dtype=torch.float64, device=dev), torch.zeros((S, B), dtype=torch.float64, device=dev),
              torch.zeros((B,), dtype=torch.int32, device=dev))
    curv = trk["curvature"]
    M = int(curv.numel())
    x_lo = torch.as_tensor(learner.config["x_min"], dtype=torch.float64, device=dev)[:, None]
    x_hi = torch.as_tensor(learner.config["x_max"], dtype=torch.float64, device=dev)[:, None]
    keys = ("X_ref", "U_ref", "T_ref", "bound_left", "bound_right", "curvatures", "vel_ref")
    # device bookkeeping of the laps: slot i of car b is its i-th closed lap
    n_rec = warm_laps + learn_laps + 8 + int(laps_before.max())   # (the laps of a warm-up keep their slots: none after them is lost)
    lap_time = torch.zeros((n_rec, B), dtype=torch.float64, device=dev)
    lap_learn = torch.zeros((n_rec, B), dtype=torch.bool, device=dev)
    n_learn = torch.zeros(B, dtype=torch.int64, device=dev)
    learning_d = torch.zeros(B, dtype=torch.bool, device=dev)
    small = torch.zeros((2, B), dtype=torch.int32, device=dev)   # what the host reads: laps_in_ring, done
    stats = {"laps_in_ring": small[0], "lap_count": torch.zeros(B, dtype=torch.int32, device=dev),
             "n_dropped": torch.zeros(B, dtype=torch.int32, device=dev), "last_lap_time": torch.zeros(B, dtype=torch.float64, device=dev)}
    count_prev = torch.as_tensor(laps_before, dtype=torch.int32, device=dev)
    learning = np.zeros(B, dtype=bool)   # host mirror of learning_d
    trace, t, k = [], t_start, -1
    for k in range(max_steps):
        # x_ic by the phase the car was in BEFORE this period's sample (run_lmpc sets it before its recorder step): learning cars get
        # the measured state projected onto the state box
        if learning.all():
            x_ic = torch.minimum(torch.maximum(x, x_lo), x_hi)
        elif learning.any():
            x_ic = torch.where(learning_d[None, :], torch.minimum(torch.maximum(x, x_lo), x_hi), x)
        else:
            x_ic = x
        inp["x_ic"], inp["u_ic"] = x_ic, u_prev
        # every car feeds its recorder: state, applied input, curvature at its abscissa (periodic linear interpolation), time
        pos = torch.remainder(x[0], L) * (M / L)
        i0 = torch.clamp(pos.floor().long(), 0, M - 1)
        fr = pos - i0
        kap = curv[i0] * (1.0 - fr) + curv[(i0 + 1) % M] * fr
        if record_trace:
            trace.append((x.clone(), u_prev.clone(), kap.clone(), t))
        learner.fleet_ss_record(x, u_prev, kap, t, L)
        learner.fleet_ss_stats(B, out=stats)
        closed = (stats["lap_count"] != count_prev) & (count_prev >= 1)   # (the first crossing closes the discarded partial lap)
        slot = torch.clamp(count_prev.long() - 1, 0, n_rec - 1)[None, :]
        keep = (closed & (count_prev <= n_rec))[None, :]
        lap_time.scatter_(0, slot, torch.where(keep, stats["last_lap_time"][None, :], lap_time.gather(0, slot)))
        lap_learn.scatter_(0, slot, torch.where(keep, learning_d[None, :], lap_learn.gather(0, slot)))
        n_learn += (closed & learning_d).to(torch.int64)
        count_prev.copy_(stats["lap_count"])
        learning_d |= small[0] >= warm_laps   # after the lap's kind was noted
        small[1].copy_((n_learn >= learn_laps).to(torch.int32))
        host = small.cpu().numpy()            # the period's one read
        learning |= host[0] >= warm_laps
        if host[1].all():
            break
        some, every = bool(learning.any()), bool(learning.all())
        if some:
            # query = last knot of the abscissa-aligned reference (racing_mpc.cpp:219-223,249-254)
            s_last, s0 = inp["X_ref"][0, -1], x[0]
            kk = (s0 - s_last).abs() + L / 2
            q = torch.stack([s_last + (kk - torch.fmod(kk, L)) * torch.sign(s0 - s_last), inp["X_ref"][1, -1]]).contiguous()
            ss_x, ss_j, _ = learner.fleet_ss_query(q, out=ss_buf)
            learner.solve(inp, out_l, ss_x=ss_x, ss_j=ss_j)
        if not every:
            tracker.solve(inp, out_t)
        if every:
            out = out_l
        elif not some:
            out = out_t
        else:
            out = {"X_optm": torch.where(learning_d, out_l["X_optm"], out_t["X_optm"]),
                   "U_optm": torch.where(learning_d, out_l["U_optm"], out_t["U_optm"]),
                   "status": torch.where(learning_d, out_l["status"], out_t["status"])}
        ok = out["status"] == 0
        n_fail += (~ok).to(torch.int64)
        u_apply = torch.where(ok[None, :], out["U_optm"][:, 0, :], inp["U_ref"][:, 0, :]).contiguous()
        (plant if plant is not None else learner if every else tracker).plant_step(trk, x, u_apply, dt / n_sub, n_sub)
        exc = torch.maximum(x[1] + half_b - inp["bound_left"][0], inp["bound_right"][0] - (x[1] - half_b))
        worst_excess = torch.maximum(worst_excess, exc)
        u_prev = u_apply
        if every:
            inp = learner.shift(trk, inp, out, dt, speed_scale=1.0)
        elif not some:
            inp = tracker.shift(trk, inp, out, dt, speed_scale=warm_speed_scale)
        else:
            nl, nt = learner.shift(trk, inp, out, dt, speed_scale=1.0), tracker.shift(trk, inp, out, dt, speed_scale=warm_speed_scale)
            inp = {key: torch.where(learning_d, nl[key], nt[key]) for key in keys}
            inp["L"] = L
        t += dt
    learner.fleet_ss_stats(B, out=stats)
    n_closed = np.minimum(np.maximum(count_prev.cpu().numpy() - 1, 0), n_rec)
    skip = np.maximum(laps_before - 1, 0)   # the laps a warm-up closed
    lt, lk = lap_time.cpu().numpy(), lap_learn.cpu().numpy()
    return {"lap_times": [[float(v) for v in lt[skip[b]:n_closed[b], b]] for b in range(B)],
            "lap_kind": [["lmpc" if v else "tracking" for v in lk[skip[b]:n_closed[b], b]] for b in range(B)],
            "worst_excess": worst_excess, "n_fail": n_fail, "n_dropped": stats["n_dropped"].clone(),
            "laps_in_ring": stats["laps_in_ring"].clone(), "steps": k + 1, "x": x, "trace": trace, **warmed}


def run_lmpc_fleet_fused(tracker, learner, track: dict, x0, u0, warm_laps: int = 2, learn_laps: int = 4, dt: float = 0.025,
                         n_sub: int = 2, warm_speed_scale: float = 0.7, max_steps: int = 20000, max_pts_per_lap: int = 1024,
                         record_trace: bool = False, regression: dict | None = None, plant=None, poll: int = 1, plants=None,
                         warmup: dict | None = None, _warm_plant: str = "handle", plants_dt=None, controllers_dt=None, controllers=None):
    """run_lmpc_fleet with everything between two solves in one launch, lmpc_fleet_loop_advance_batch on `learner`: input selection
    between the two controllers' results, plant, shift, x_ic, every car's recorder and ring, the lap book, the per-car phase and the
    next query point.  Same arguments, same experiment, same return dictionary; per period the fleet query when any car learns, the
    solve of each controller that has cars, and that one call.

    The phase, the lap book and the query live on the device.  The host reads two int32 counters -- cars in the learning phase, cars
    that have their learning laps -- every `poll` periods, and only the call of such a period may switch a car's phase, so what the
    host knows about which controllers have cars stays true in between: with poll > 1 whole runs of periods are enqueued without a
    read, a car switches up to poll - 1 periods after its ring is full, and the run ends up to poll - 1 periods late.  poll = 1 is
    run_lmpc_fleet's schedule.

    plant (a Solver): its VEHICLE drives the cars (the call takes the plant's vehicle by value).  record_trace: the curvature in the
    (x, u, k, t) tuples is run_lmpc_fleet's torch interpolation; the ring holds the kernel's own lookup at the same abscissa.
    plants (a list of B vehicle dicts, exclusive with plant=): car b drives on plants[b] -- the list is `learner`'s car table
    (Solver.set_car_vehicles) for the run, which the fused call reads, and the table is cleared at the end.
    plants_dt (a list of B double-track vehicle dicts, exclusive with plant= and plants=): car b drives on the FOUR-WHEEL model with
    plants_dt[b] -- the list is `learner`'s double-track table (Solver.set_dtrack_vehicles) for the run, every period is
    lmpc_fleet_loop_advance_dtrack_batch (fleet_loop_advance(dtrack=True)), and the table is cleared at the end.
    warmup (a dict, _fleet_warm_up's): run_lmpc_fleet's -- the warm laps by the vanilla controller on the run's own plants; the
    head-only call then sends every car whose ring holds warm_laps laps straight to the learning controller.
    controllers_dt (a list of B double-track vehicle dicts, usually plants_dt's list): run_lmpc_fleet's -- both controllers solve on the
    four-wheel model, problem b on controllers_dt[b]; the same list as plants_dt= where both are given, exclusive with regression=.
    controllers (a list of B single-track vehicle dicts, usually plants=' list): run_lmpc_fleet's -- both controllers linearise problem b
    on controllers[b] and the cars drive on the same list; the same list as plants= where both are given, exclusive with plant=,
    regression=, controllers_dt= and plants_dt=.
    Raises ValueError when the two solvers differ in N or vehicle: one launch shifts both controllers' plans with one model."""
    import numpy as np
    import torch

    if int(tracker.N) != int(learner.N) or dict(tracker.vehicle) != dict(learner.vehicle):
        raise ValueError("run_lmpc_fleet_fused: tracker and learner must have the same N and the same vehicle")
    if poll < 1:
        raise ValueError("run_lmpc_fleet_fused: poll must be >= 1")
    B = x0.shape[1]
    if controllers is not None:
        return _with_cars_controllers(
            lambda same: run_lmpc_fleet_fused(tracker, learner, track, x0, u0, warm_laps, learn_laps, dt, n_sub, warm_speed_scale, max_steps,
                                              max_pts_per_lap, record_trace, None, None, poll, same, warmup, _warm_plant),
            "run_lmpc_fleet_fused", tracker, learner, B, controllers, plant, plants, plants_dt, controllers_dt, regression)
    if controllers_dt is not None:
        return _with_dtrack_controllers(
            lambda: run_lmpc_fleet_fused(tracker, learner, track, x0, u0, warm_laps, learn_laps, dt, n_sub, warm_speed_scale, max_steps,
                                         max_pts_per_lap, record_trace, regression, plant, poll, plants, warmup, _warm_plant, plants_dt),
            "run_lmpc_fleet_fused", tracker, learner, B, controllers_dt, plants_dt, regression)
    if plants_dt is not None:
        if plants is not None:
            raise ValueError("run_lmpc_fleet_fused: plants= (single-track cars) and plants_dt= (double-track cars) are exclusive")
        _check_plants(plant, plants_dt, B, "run_lmpc_fleet_fused", "plants_dt")
        learner.set_dtrack_vehicles(plants_dt)
        try:
            return run_lmpc_fleet_fused(tracker, learner, track, x0, u0, warm_laps, learn_laps, dt, n_sub, warm_speed_scale, max_steps,
                                        max_pts_per_lap, record_trace, regression, None, poll, warmup=warmup, _warm_plant="dtrack")
        finally:
            learner.set_dtrack_vehicles(None)
    _check_plants(plant, plants, B, "run_lmpc_fleet_fused")
    if warmup is not None and plant is not None:
        raise ValueError("run_lmpc_fleet_fused: warmup= drives the warm laps on the learner's vehicle, plants= or plants_dt=, not on plant=")
    if plants is not None:
        learner.set_car_vehicles(plants)
        try:
            return run_lmpc_fleet_fused(tracker, learner, track, x0, u0, warm_laps, learn_laps, dt, n_sub, warm_speed_scale, max_steps,
                                        max_pts_per_lap, record_trace, regression, None, poll, warmup=warmup, _warm_plant="cars")
        finally:
            learner.set_car_vehicles(None)
    trk = tracker.device_track(track)
    L = float(track["L"])
    dev = x0.device
    learner.fleet_ss_create(B, max_pts_per_lap)
    if regression is not None:
        learner.fleet_ss_set_regression(**regression)
    x, u_prev = x0.clone(), u0.clone()
    t_start, laps_before, warmed = 0.0, np.zeros(B, dtype=np.int64), {}
    if warmup is not None:
        x, u_prev, t_start, laps_before = _fleet_warm_up(learner, trk, x, u_prev, warm_laps, dt, n_sub, warmup, _warm_plant)
        warmed = {"warmup": {"periods": int(round(t_start / dt)), "t_end": t_start, "lap_count": laps_before}}
    worst_excess = torch.zeros(B, dtype=torch.float64, device=dev)
    n_fail = torch.zeros(B, dtype=torch.int64, device=dev)
    inp = tracker.prepare(trk, x, dt, speed_scale=warm_speed_scale)
    out_t, out_l = tracker.alloc_outputs(B), learner.alloc_outputs(B)
    S = int(learner.config["num_ss_pts"])
    out_l["convex_combi_optm"] = torch.zeros((S, B), dtype=torch.float64, device=dev)
    ss_buf = (torch.zeros((6, S, B), dtype=torch.float64, device=dev), torch.zeros((S, B), dtype=torch.float64, device=dev),
              torch.zeros((B,), dtype=torch.int32, device=dev))
    n_rec = warm_laps + learn_laps + 8 + int(laps_before.max())   # (the laps of a warm-up keep their slots: none after them is lost)
    state = learner.fleet_loop_state(B, n_rec)
    kw = dict(dt=dt, dt_sim=dt / n_sub, n_sub=n_sub, speed_scale=(warm_speed_scale, 1.0),
              speed_limit=(float(tracker.config["x_max"][3]), float(learner.config["x_max"][3])),
              max_vel_ref_diff=(float(tracker.config["max_vel_ref_diff"]), float(learner.config["max_vel_ref_diff"])),
              restart_failed=False, warm_laps=warm_laps, learn_laps=learn_laps, plant=None if plant is None else plant.vehicle,
              worst_excess=worst_excess, n_fail=n_fail, dtrack=_warm_plant == "dtrack")   # ("dtrack": the plants_dt= branch above)
    curv = trk["curvature"]
    M = int(curv.numel())
    trace, t, k = [], t_start, -1

    def note():
        pos = torch.remainder(x[0], L) * (M / L)
        i0 = torch.clamp(pos.floor().long(), 0, M - 1)
        fr = pos - i0
        trace.append((x.clone(), u_prev.clone(), curv[i0] * (1.0 - fr) + curv[(i0 + 1) % M] * fr, t))

    # period 0: nothing to apply yet -- the recorder's first sample, x_ic and the query on the prepared references
    learner.fleet_loop_advance(trk, inp, None, None, x, u_prev, state, t=t, switch_phase=True, **kw)
    if record_trace:
        note()
    n_lrn = n_done = 0
    for k in range(max_steps):
        if k % poll == 0:
            n_lrn, n_done = (int(v) for v in state["counters"].cpu())   # the only read, every `poll` periods
        if n_done == B:
            break
        some, every = n_lrn > 0, n_lrn == B
        inp["x_ic"], inp["u_ic"] = state["x_ic"], u_prev
        if some:
            ss_x, ss_j, _ = learner.fleet_ss_query(state["query"], out=ss_buf)
            learner.solve(inp, out_l, ss_x=ss_x, ss_j=ss_j)
        if not every:
            tracker.solve(inp, out_t)
        t += dt
        learner.fleet_loop_advance(trk, inp, None if every else out_t, out_l if some else None, x, u_prev, state, t=t,
                                   switch_phase=(k + 1) % poll == 0, **kw)
        if record_trace:
            note()
    stats = learner.fleet_ss_stats(B)
    n_closed = np.minimum(np.maximum(stats["lap_count"].cpu().numpy() - 1, 0), n_rec)
    skip = np.maximum(laps_before - 1, 0)   # the laps a warm-up closed
    lt, lk = state["lap_time"].cpu().numpy(), state["lap_kind"].cpu().numpy()
    return {"lap_times": [[float(v) for v in lt[skip[b]:n_closed[b], b]] for b in range(B)],
            "lap_kind": [["lmpc" if v else "tracking" for v in lk[skip[b]:n_closed[b], b]] for b in range(B)],
            "worst_excess": worst_excess, "n_fail": n_fail, "n_dropped": stats["n_dropped"], "laps_in_ring": stats["laps_in_ring"],
            "steps": k + 1, "x": x, "trace": trace, **warmed}


def run_lqr(solver, x0, X_traj, U_traj, steps: int):
    """Receding-horizon LQR tracking of a long reference, the loop of the reference's own test (test_racing_lqr.cpp): period t solves
    on the window t .. t+N-1 of the trajectory (N = the horizon of solver.lqr_create, which the caller has made for at least B cars)
    and the plan's second knot X_optm[:, 1] -- one RK4 step of the model under u = U_optm[:, 0] -- is the next state: the model is
    the plant.  x0 [6][B]; X_traj [B][6][M], U_traj [B][2][M-1] with M >= steps + N - 1.  The windows are slices of one device
    copy of the trajectory, batch axis last; nothing goes through the host inside the loop.
    Returns {"X" [6][steps+1][B] the states from x0 on, "U" [2][steps][B] the applied inputs, "flags" int32 [B] the OR of every
    solve's flags (LQR_NOT_FINITE)}."""
    import torch

    if getattr(solver, "_lqr_N", None) is None:
        raise ValueError("run_lqr: no controller (Solver.lqr_create)")
    N = int(solver._lqr_N)
    X_all = solver._t(X_traj).permute(1, 2, 0).contiguous()  # [6][M][B]
    U_all = solver._t(U_traj).permute(1, 2, 0).contiguous()  # [2][M-1][B]
    M = X_all.shape[1]
    if M < steps + N - 1 or U_all.shape[1] < steps + N - 2:
        raise ValueError(f"run_lqr: {steps} periods of horizon {N} need a reference of {steps + N - 1} knots, got {M}")
    x = solver._t(x0).clone()
    B = x.shape[1]
    kw = dict(dtype=torch.float64, device=x.device)
    X, U = torch.empty((6, steps + 1, B), **kw), torch.empty((2, steps, B), **kw)
    flags_or = torch.zeros(B, dtype=torch.int32, device=x.device)
    out = None
    X[:, 0] = x
    for t in range(steps):
        out = solver.lqr_solve(x, X_all[:, t:t + N].contiguous(), U_all[:, t:t + N - 1].contiguous(), out=out)
        flags_or |= out["flags"]
        U[:, t] = out["u"]
        x = out["X_optm"][:, 1].contiguous()
        X[:, t + 1] = x
    return {"X": X, "U": U, "flags": flags_or}


def _table_lookup(tab, M: int, L: float, s):
    """The periodic linear interpolation of an lmpc_track table at s [B], operation by operation as lmpc_vanilla_rollout_batch forms
    k_log and the bounds of worst_excess (no contraction there): the same bits."""
    import torch

    u = torch.fmod(s, L)
    u = torch.where(u < 0.0, u + L, u)
    u = u / torch.full_like(u, L / M)   # (a tensor divisor: torch divides by a Python scalar as a product with its reciprocal)
    fl = torch.floor(u)
    fr = u - fl
    i0 = torch.remainder(torch.nan_to_num(fl, nan=0.0, posinf=0.0, neginf=0.0).long(), M)
    i1 = torch.where(i0 + 1 == M, torch.zeros_like(i0), i0 + 1)
    return tab[i0] * (1.0 - fr) + tab[i1] * fr


def run_vanilla(solver, track: dict, spline, x0, steps: int, dt: float = 0.025, n_sub: int = 2, speed_scale: float = 1.0, chunk: int = 64,
                fused: bool = True, fleet_record: bool = False):
    """A fleet driven by the vanilla controller (pure pursuit + PID, lmpc_vanilla_*), one controller per car: what buys an LMPC
    experiment its first feasible laps without a QP.  The caller has made the controllers (solver.vanilla_create for B cars; their PID
    state is used as it stands and is left where the run ends); `track` holds the uniform tables the plant reads, `spline` is
    Solver.spline_track of the same track.  x0 [6][B]; `steps` control periods of n_sub plant sub-steps of dt / n_sub each.  (dt is the
    period the plant is stepped over; the PID integrates with the dt of its own config, as upstream.)

    fused=True: lmpc_vanilla_rollout_batch in chunks of `chunk` periods -- ceil(steps / chunk) launches in all.  fused=False: one
    vanilla_solve, one plant_step and the bookkeeping in torch per period, the same arithmetic (the plant is compiled into two
    translation units, so nothing guarantees the same contraction: tests/test_gpu_vanilla.py compares at the rollout's tolerance,
    demands the decision bit for bit, and finds the 700-period laps both paths record identical with this compiler).  A car whose decision or state turns non-finite is frozen at its last finite state in both; what the
    unfused path cannot do is take back the PID update of a period whose plant step went non-finite.

    fleet_record=True: every logged sample (x, u_model, curvature, t = period * dt) goes to the fleet safe set's recorder
    (solver.fleet_ss_record, one call per period; the caller has made the store with fleet_ss_create); frozen cars are skipped.

    Returns run's statistics -- "x" [6][B], "distance" [B], "worst_excess" [B] (from 0, as run keeps it), "n_fail" int64 [B] (the
    periods a car was not driven: frozen), "trace" [], "warm_hit_rate" None -- and "flags" int32 [B] (the OR over the run:
    VANILLA_NOT_FINITE), "X_log" [6][steps][B], "U_log" [2][steps][B], "k_log" [steps][B]."""
    import torch

    if getattr(solver, "_vanilla_B", None) is None:
        raise ValueError("run_vanilla: no controller (Solver.vanilla_create)")
    if chunk < 1:
        raise ValueError("run_vanilla: chunk must be at least 1")
    trk = solver.device_track(track)
    L, M = float(trk["L"]), int(trk["M"])
    x = solver._t(x0).clone()
    B, dev = x.shape[1], x.device
    kw = dict(dtype=torch.float64, device=dev)
    dist, worst = torch.zeros(B, **kw), torch.zeros(B, **kw)
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    X_log, U_log, k_log = torch.empty((6, steps, B), **kw), torch.empty((2, steps, B), **kw), torch.empty((steps, B), **kw)
    half_b = float(solver.vehicle["b"]) / 2.0

    def record(p0, p1):
        for p in range(p0, p1):
            solver.fleet_ss_record(X_log[:, p], U_log[:, p], k_log[p], p * dt, L, active=torch.isfinite(k_log[p]).to(torch.int32))

    if fused:
        for p0 in range(0, steps, chunk):
            n = min(chunk, steps - p0)
            out = solver.vanilla_rollout(spline, trk, x, n, dt / n_sub, n_sub, speed_scale=speed_scale, distance=dist, worst_excess=worst)
            # (a car frozen in an earlier chunk freezes again at once: the period that froze it was undone, so the kernel meets the
            # same state and the same PID state, and its logs are NaN again)
            X_log[:, p0:p0 + n], U_log[:, p0:p0 + n], k_log[p0:p0 + n] = out["X_log"], out["U_log"], out["k_log"]
            flags |= out["flags"]
            if fleet_record:
                record(p0, p0 + n)
    else:
        out = None
        nan = torch.full((), float("nan"), **kw)
        for p in range(steps):
            out = solver.vanilla_solve(spline, x, None, speed_scale=speed_scale, out=out)
            frozen = flags != 0
            live = (out["flags"] == 0) & ~frozen
            xs = torch.where(live, x, torch.zeros_like(x)).contiguous()
            u = torch.where(live, out["u_model"], torch.zeros_like(out["u_model"])).contiguous()
            solver.plant_step(trk, xs, u, dt / n_sub, n_sub)
            live = live & torch.isfinite(xs).all(dim=0)
            flags |= (~live).to(torch.int32)
            X_log[:, p] = torch.where(live, x, nan)
            U_log[:, p] = torch.where(live, out["u_model"], nan)
            k_log[p] = torch.where(live, _table_lookup(trk["curvature"], M, L, x[0]), nan)
            ds = xs[0] - x[0]
            dist += torch.where(live, torch.where(ds < -L / 2.0, ds + L, ds), torch.zeros_like(ds))
            bl, br = _table_lookup(trk["bound_left"], M, L, x[0]), _table_lookup(trk["bound_right"], M, L, x[0])
            exc = torch.maximum(xs[1] + half_b - bl, br - (xs[1] - half_b))
            worst = torch.where(live, torch.maximum(worst, exc), worst)
            x = torch.where(live, xs, x).contiguous()
            if fleet_record:
                record(p, p + 1)
    return {"x": x, "distance": dist, "worst_excess": worst, "n_fail": torch.isnan(k_log).sum(dim=0).to(torch.int64), "trace": [],
            "warm_hit_rate": None, "flags": flags, "X_log": X_log, "U_log": U_log, "k_log": k_log}


def _warm_up_chunks(solver, trk, spline, x, u_prev, laps: int, dt: float, n_sub: int, speed_scale: float, chunk: int, max_periods: int,
                    plant: str, record):
    """warm_up_vanilla's loop on tables that are already set: x and u_prev are updated in place."""
    import torch

    B, dev = x.shape[1], x.device
    kw = dict(dtype=torch.float64, device=dev)
    dist, worst = torch.zeros(B, **kw), torch.full((B,), -float("inf"), **kw)
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    out, stats, periods = None, None, 0
    while periods < max_periods:
        n = min(chunk, max_periods - periods)
        out = solver.vanilla_rollout_fleet(spline, trk, x, n, dt / n_sub, n_sub, plant=plant, record=record, period0=periods, dt=dt, u_prev=u_prev,
                                           speed_scale=speed_scale, distance=dist, worst_excess=worst, out=out if n == chunk else None)
        flags |= out["flags"]
        periods += n
        stats = solver.fleet_ss_stats(B, out=stats)
        if int(stats["laps_in_ring"].min()) >= laps:   # the chunk's one read
            break
    if stats is None:
        stats = solver.fleet_ss_stats(B)
    return {"x": x, "u_prev": u_prev, "periods": periods, "t_end": periods * dt, "flags": flags, "distance": dist, "worst_excess": worst,
            "laps_in_ring": stats["laps_in_ring"].clone(), "lap_count": stats["lap_count"].clone()}


def warm_up_vanilla(solver, track: dict, spline, x0, u0, laps: int, dt: float = 0.025, n_sub: int = 2, speed_scale: float = 1.0, chunk: int = 64,
                    max_periods: int = 4096, plants=None, plants_dt=None, record="arrived"):
    """The first laps of a fleet LMPC experiment without a QP: the vanilla controller (pure pursuit + PID) drives every car ON ITS OWN
    PLANT and every car's recorder takes its samples inside the same launch (Solver.vanilla_rollout_fleet), `chunk` periods per
    launch, until every car's ring holds `laps` laps or `max_periods` periods have been driven.  Every car drives the same number of
    periods -- the fleet shares one clock -- and the host reads one fleet_ss_stats per chunk.

    The caller has made the controllers (solver.vanilla_create for B cars; the PID state is used as it stands) and the fleet store
    (solver.fleet_ss_create).  `track` holds the uniform tables, `spline` is Solver.spline_track of the same track; x0 [6][B], u0
    [2][B] the input applied before the first period (the "arrived" convention records it with x0).  plants (B vehicle dicts) /
    plants_dt (B double-track vehicle dicts), exclusive: car b's plant; the list is the solver's car table / double-track table for
    the call and the table is cleared at the end, as run_lmpc_fleet does.  Neither: the solver's vehicle.  record: "arrived" (what the
    LMPC loop records: continue with fleet_loop_advance at t_end) or "applied" (run_vanilla's convention).

    Returns {"x" [6][B], "u_prev" [2][B] the last input applied, "periods", "t_end" = periods * dt (the time stamp of the next sample),
    "flags" int32 [B] (the OR over the chunks: VANILLA_NOT_FINITE), "distance" [B], "worst_excess" [B] (from -inf), "laps_in_ring" [B]}."""
    if getattr(solver, "_vanilla_B", None) is None:
        raise ValueError("warm_up_vanilla: no controller (Solver.vanilla_create)")
    if chunk < 1 or max_periods < 1:
        raise ValueError("warm_up_vanilla: chunk and max_periods must be at least 1")
    x, u_prev = solver._t(x0).clone(), solver._t(u0).clone()
    B = x.shape[1]
    if plants is not None and plants_dt is not None:
        raise ValueError("warm_up_vanilla: plants= (single-track cars) and plants_dt= (double-track cars) are exclusive")
    _check_plants(None, plants if plants is not None else plants_dt, B, "warm_up_vanilla", "plants" if plants is not None else "plants_dt")
    trk = solver.device_track(track)
    plant = "cars" if plants is not None else "dtrack" if plants_dt is not None else "handle"
    if plants is not None:
        solver.set_car_vehicles(plants)
    if plants_dt is not None:
        solver.set_dtrack_vehicles(plants_dt)
    try:
        res = _warm_up_chunks(solver, trk, spline, x, u_prev, laps, dt, n_sub, speed_scale, chunk, max_periods, plant, record)
    finally:
        if plants is not None:
            solver.set_car_vehicles(None)
        if plants_dt is not None:
            solver.set_dtrack_vehicles(None)
    res.pop("lap_count")
    return res


def _fleet_warm_up(learner, trk, x, u_prev, warm_laps: int, dt: float, n_sub: int, warmup: dict, plant: str):
    """warmup= of run_lmpc_fleet and run_lmpc_fleet_fused, after the store is made and the run's table is set: the vanilla controllers
    are made on `learner`, the warm laps are driven on the run's plants and recorded by the loop's convention.  warmup: "config" (the
    vanilla controller's, Solver.vanilla_create's dict) and "spline" (Solver.spline_track of the run's track on `learner`, or the
    dict it is made from), and optionally warm_up_vanilla's "laps" (default: warm_laps), "speed_scale", "chunk", "max_periods".
    -> (x, u_prev, t_end, the recorders' lap_count [B] as a host array)."""
    unknown = set(warmup) - {"config", "spline", "laps", "speed_scale", "chunk", "max_periods"}
    if unknown or "config" not in warmup or "spline" not in warmup:
        raise ValueError("warmup= takes config, spline and optionally laps, speed_scale, chunk, max_periods; got %s" % sorted(warmup))
    spline = warmup["spline"]
    if isinstance(spline, dict):
        spline = learner.spline_track(spline)
    learner.vanilla_create(warmup["config"], x.shape[1])
    res = _warm_up_chunks(learner, trk, spline, x, u_prev, int(warmup.get("laps", warm_laps)), dt, n_sub, float(warmup.get("speed_scale", 1.0)),
                          int(warmup.get("chunk", 64)), int(warmup.get("max_periods", 4096)), plant, "arrived")
    learner.vanilla_destroy()
    return res["x"], res["u_prev"], res["t_end"], res["lap_count"].cpu().numpy().astype("int64")
