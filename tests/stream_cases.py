"""Which stream every entry point of include/lmpc_hip.h works on: the classification table, the rows that exercise it and the gate
(tests/test_stream_table.py holds the table to the header without a GPU, tests/test_gpu_streams.py runs the rows on one).

TABLE has one entry per `lmpc_*` prototype, its class taken from the header's own words:
  async      enqueues on the handle's stream and returns;
  blocking   waits for the handle's stream, or allocates / frees device memory (which the runtime orders against the whole device);
  host-only  no device work.
`sync` marks the entries whose comment says that they synchronise (wait for) the handle's stream: behind a gated stream they must
not return before the gate opens.  `io` marks the entries with device inputs or outputs, or with handle-held device state they
change; every one of them appears in at least one row of ROWS.

A row is a Case: device input buffers with two valid fillings of the same shapes -- `real`, and `stale`, another draw of the same
generator -- the call, pure outputs (filled with a sentinel before every run), the handle-held state the call changes (read by
`state`, restored by `reset`).  reference() runs it on the default stream; gated() runs it on a fresh non-blocking stream behind a
finite delay, with `stale` in the buffers until the stream itself copies `real` in (and fills the outputs with the sentinel once
more) and puts `stale` back behind the call.  Work that left the stream runs during the delay: it sees `stale`, the state as it was
before the stream's earlier work, and what it writes is wiped by the stream's own sentinel fill; work that was forked and not joined
leaves the sentinel.  A row whose call reads only handle-held state makes the call behind a launch, on the same stream, that changes
that state.

The gate is torch.cuda._sleep, calibrated with two events; a chain of element-wise kernels where that is not usable.  Nothing here
waits on a host-written value, so a gate always ends and a blocking call behind it always returns."""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

ASYNC, BLOCKING, HOST = "async", "blocking", "host-only"

# name: (class, sync, io)
TABLE = {
    "lmpc_create": (BLOCKING, False, False),
    "lmpc_destroy": (BLOCKING, True, False),
    "lmpc_last_error": (HOST, False, False),
    "lmpc_set_stream": (HOST, False, False),
    "lmpc_synchronize": (BLOCKING, True, False),
    "lmpc_linearize_batch": (ASYNC, False, True),
    "lmpc_solve_batch": (ASYNC, False, True),
    "lmpc_solve_batch_warm": (ASYNC, False, True),
    "lmpc_solve_batch_warm_ss": (ASYNC, False, True),
    "lmpc_shift_lambda_batch": (ASYNC, False, True),
    "lmpc_get_warm_accepted": (ASYNC, False, True),
    "lmpc_solve_batch_mixed": (ASYNC, False, True),
    "lmpc_set_warm_rounds": (HOST, False, False),
    "lmpc_solve_batch_f32": (ASYNC, False, True),
    "lmpc_solve_host": (BLOCKING, True, True),
    "lmpc_solve_host_warm": (BLOCKING, True, True),
    "lmpc_solve_host_warm_ss": (BLOCKING, True, True),
    "lmpc_solve_full_dynamics_batch": (BLOCKING, True, True),
    "lmpc_solve_full_dynamics_host": (BLOCKING, True, True),
    "lmpc_set_safe_set": (BLOCKING, True, True),
    "lmpc_ss_query_host": (BLOCKING, True, True),
    "lmpc_set_regression_laps": (BLOCKING, True, True),
    "lmpc_regress_batch": (ASYNC, False, True),
    "lmpc_ss_query_batch": (ASYNC, False, True),
    "lmpc_ss_query_idx_batch": (ASYNC, False, True),
    "lmpc_solve_batch_ss_idx": (ASYNC, False, True),
    "lmpc_prepare_batch": (ASYNC, False, True),
    "lmpc_prepare_failed_batch": (ASYNC, False, True),
    "lmpc_shift_batch": (ASYNC, False, True),
    "lmpc_plant_step_batch": (ASYNC, False, True),
    "lmpc_loop_advance_batch": (ASYNC, False, True),
    "lmpc_set_output_layout": (HOST, False, False),
    "lmpc_reserve": (BLOCKING, False, False),
    "lmpc_set_launch_order": (HOST, False, False),
    "lmpc_launch_order_from_iters": (ASYNC, False, True),
    "lmpc_query_launch": (HOST, False, False),
    "lmpc_query_residency": (HOST, False, False),
    "lmpc_query_launch_for": (HOST, False, False),
    "lmpc_set_waves_per_problem": (HOST, False, False),
    "lmpc_last_solve_precision": (HOST, False, False),
    "lmpc_enable_timing": (HOST, False, False),
    "lmpc_last_kernel_ms": (BLOCKING, False, False),
    "lmpc_fleet_ss_create": (BLOCKING, False, True),
    "lmpc_fleet_ss_destroy": (BLOCKING, True, False),
    "lmpc_fleet_ss_reset": (ASYNC, False, True),
    "lmpc_fleet_ss_bytes": (HOST, False, False),
    "lmpc_fleet_ss_record_batch": (ASYNC, False, True),
    "lmpc_fleet_ss_query_batch": (ASYNC, False, True),
    "lmpc_fleet_ss_load": (BLOCKING, True, True),
    "lmpc_fleet_ss_get_laps": (BLOCKING, True, True),
    "lmpc_fleet_ss_stats": (ASYNC, False, True),
    "lmpc_fleet_loop_advance_batch": (ASYNC, False, True),
    "lmpc_fleet_ss_set_regression": (BLOCKING, True, True),   # (sync: when the table's size changes -- the row's case)
    "lmpc_fleet_ss_regress_batch": (ASYNC, False, True),
    "lmpc_spline_track_create": (BLOCKING, True, True),
    "lmpc_spline_track_destroy": (BLOCKING, True, False),
    "lmpc_track_sample_batch": (ASYNC, False, True),
    "lmpc_spline_track_tabulate": (ASYNC, False, True),
    "lmpc_global_to_frenet_batch": (ASYNC, False, True),
    "lmpc_frenet_to_global_batch": (ASYNC, False, True),
    "lmpc_ekf_create": (BLOCKING, False, True),
    "lmpc_ekf_destroy": (BLOCKING, True, False),
    "lmpc_ekf_register_observation": (BLOCKING, True, True),
    "lmpc_ekf_initialize": (HOST, False, False),
    "lmpc_ekf_set_state": (ASYNC, False, True),
    "lmpc_ekf_update_control": (ASYNC, False, True),
    "lmpc_ekf_update_batch": (ASYNC, False, True),
    "lmpc_ekf_get": (ASYNC, False, True),
    "lmpc_lqr_create": (BLOCKING, True, True),
    "lmpc_lqr_destroy": (BLOCKING, True, False),
    "lmpc_lqr_solve_batch": (ASYNC, False, True),
    "lmpc_vanilla_create": (BLOCKING, True, True),
    "lmpc_vanilla_destroy": (BLOCKING, True, False),
    "lmpc_vanilla_reset": (ASYNC, False, True),
    "lmpc_vanilla_get": (ASYNC, False, True),
    "lmpc_vanilla_solve_batch": (ASYNC, False, True),
    "lmpc_vanilla_rollout_batch": (ASYNC, False, True),
}

# row id: (group, the entry points the row's call makes on the gated stream)
ROWS = {
    "solve f64 N=20 cold": ("tracking", ("lmpc_solve_batch",)),
    "solve f64 N=20 warm": ("tracking", ("lmpc_solve_batch_warm", "lmpc_get_warm_accepted")),
    "solve f64 N=20 launch order": ("tracking", ("lmpc_solve_batch",)),
    "solve f64 N=20 timing events": ("tracking", ("lmpc_solve_batch",)),
    "solve f64 N=41 two waves": ("tracking", ("lmpc_solve_batch",)),
    "solve f32 N=20": ("tracking", ("lmpc_solve_batch_f32",)),
    "solve_host": ("tracking", ("lmpc_solve_host",)),
    "solve_host_warm": ("tracking", ("lmpc_solve_host_warm",)),
    "synchronize": ("tracking", ("lmpc_plant_step_batch", "lmpc_synchronize")),
    "ss_query": ("learning", ("lmpc_ss_query_batch",)),
    "ss_query_idx": ("learning", ("lmpc_ss_query_idx_batch",)),
    "learning solve by arrays": ("learning", ("lmpc_solve_batch",)),
    "learning solve by ss_idx": ("learning", ("lmpc_solve_batch_ss_idx",)),
    "learning solve by arrays, mixed": ("learning", ("lmpc_solve_batch_mixed",)),
    "learning solve by ss_idx, mixed": ("learning", ("lmpc_solve_batch_ss_idx",)),
    "warm_ss with shift_lambda": ("learning", ("lmpc_shift_lambda_batch", "lmpc_solve_batch_warm_ss", "lmpc_get_warm_accepted")),
    "set_safe_set": ("learning", ("lmpc_set_safe_set", "lmpc_ss_query_batch")),
    "ss_query_host": ("learning", ("lmpc_ss_query_host",)),
    "solve_host_warm_ss": ("learning", ("lmpc_solve_host_warm_ss",)),
    "linearize": ("regression", ("lmpc_linearize_batch",)),
    "regress": ("regression", ("lmpc_regress_batch",)),
    "solve with the shared regression": ("regression", ("lmpc_solve_batch",)),
    "set_regression_laps": ("regression", ("lmpc_set_regression_laps", "lmpc_regress_batch")),
    "fleet_ss_regress": ("regression", ("lmpc_fleet_ss_regress_batch",)),
    "solve with the fleet regression": ("regression", ("lmpc_solve_batch",)),
    "fleet_ss_set_regression refill": ("regression", ("lmpc_fleet_ss_set_regression", "lmpc_fleet_ss_regress_batch")),
    "prepare": ("prep", ("lmpc_prepare_batch",)),
    "prepare_failed": ("prep", ("lmpc_prepare_failed_batch",)),
    "shift": ("prep", ("lmpc_shift_batch",)),
    "plant_step": ("prep", ("lmpc_plant_step_batch",)),
    "loop_advance": ("prep", ("lmpc_loop_advance_batch",)),
    "launch_order_from_iters": ("prep", ("lmpc_launch_order_from_iters",)),
    "fleet_ss_create": ("fleet", ("lmpc_fleet_ss_create", "lmpc_fleet_ss_record_batch", "lmpc_fleet_ss_stats")),
    "fleet_ss_reset": ("fleet", ("lmpc_fleet_ss_record_batch", "lmpc_fleet_ss_reset")),
    "fleet_ss_record": ("fleet", ("lmpc_fleet_ss_record_batch",)),
    "fleet_ss_query": ("fleet", ("lmpc_fleet_ss_query_batch",)),
    "fleet_ss_stats": ("fleet", ("lmpc_fleet_ss_record_batch", "lmpc_fleet_ss_stats")),
    "fleet_loop_advance": ("fleet", ("lmpc_fleet_loop_advance_batch",)),
    "fleet_ss_load": ("fleet", ("lmpc_fleet_ss_record_batch", "lmpc_fleet_ss_load")),
    "fleet_ss_get_laps": ("fleet", ("lmpc_fleet_ss_record_batch", "lmpc_fleet_ss_get_laps")),
    "track_sample": ("track", ("lmpc_track_sample_batch",)),
    "tabulate": ("track", ("lmpc_spline_track_tabulate",)),
    "global_to_frenet": ("track", ("lmpc_global_to_frenet_batch",)),
    "frenet_to_global": ("track", ("lmpc_frenet_to_global_batch",)),
    "spline_track_create": ("track", ("lmpc_spline_track_create", "lmpc_track_sample_batch")),
    "ekf_create": ("ekf", ("lmpc_ekf_create", "lmpc_ekf_register_observation", "lmpc_ekf_set_state", "lmpc_ekf_update_control",
                           "lmpc_ekf_update_batch", "lmpc_ekf_get")),
    "ekf_set_state": ("ekf", ("lmpc_ekf_set_state",)),
    "ekf_update_control": ("ekf", ("lmpc_ekf_update_control",)),
    "ekf_update predict only": ("ekf", ("lmpc_ekf_update_batch",)),
    "ekf_update nz=1": ("ekf", ("lmpc_ekf_update_batch",)),
    "ekf_update nz=2": ("ekf", ("lmpc_ekf_update_batch",)),
    "ekf_update nz=3": ("ekf", ("lmpc_ekf_update_batch",)),
    "ekf_update nz=4": ("ekf", ("lmpc_ekf_update_batch",)),
    "ekf_update nz=5": ("ekf", ("lmpc_ekf_update_batch",)),
    "ekf_update nz=6": ("ekf", ("lmpc_ekf_update_batch",)),
    "ekf_get": ("ekf", ("lmpc_ekf_update_batch", "lmpc_ekf_get")),
    "ekf_register_observation": ("ekf", ("lmpc_ekf_register_observation",)),
    "lqr_solve with gains": ("lqr", ("lmpc_lqr_solve_batch",)),
    "lqr_solve without gains": ("lqr", ("lmpc_lqr_solve_batch",)),
    "lqr_create": ("lqr", ("lmpc_lqr_create", "lmpc_lqr_solve_batch")),
    "vanilla_reset": ("vanilla", ("lmpc_vanilla_solve_batch", "lmpc_vanilla_reset")),
    "vanilla_get": ("vanilla", ("lmpc_vanilla_solve_batch", "lmpc_vanilla_get")),
    "vanilla_solve": ("vanilla", ("lmpc_vanilla_solve_batch",)),
    "vanilla_rollout": ("vanilla", ("lmpc_vanilla_rollout_batch",)),
    "vanilla_create": ("vanilla", ("lmpc_vanilla_create", "lmpc_vanilla_solve_batch")),
    "solve_full_dynamics": ("sqp", ("lmpc_solve_full_dynamics_batch",)),
    "solve_full_dynamics_host": ("sqp", ("lmpc_solve_full_dynamics_host",)),
}


def row_class(row: str):
    """(class, sync) of a row: blocking when any of its entry points is, sync when any of them must wait for the stream."""
    fns = ROWS[row][1]
    blocking = any(TABLE[f][0] == BLOCKING for f in fns)
    return (BLOCKING if blocking else ASYNC), any(TABLE[f][1] for f in fns)


# ---- the gate -------------------------------------------------------------------------------------------------------------------------
GATE_FLOOR_MS = 20.0
GATE_FACTOR = 10.0


class Gate:
    """A finite delay on the current stream.  hold(ms) enqueues it; it ends by itself."""

    def __init__(self):
        import torch

        self.torch = torch
        self.kind, self.per_ms = "sleep", 0.0
        try:
            ms = self._time(lambda: torch.cuda._sleep(20_000_000))
            if ms >= 0.5:
                self.per_ms = 20_000_000 / ms
        except (AttributeError, RuntimeError):
            ms = 0.0
        if not self.per_ms:   # the sleep kernel is not usable here: element-wise kernels over 512 MB, timed the same way
            self.kind = "chain"
            self.buf = torch.ones(1 << 26, dtype=torch.float64, device="cuda")
            self.per_ms = 50 / self._time(lambda: [self.buf.mul_(1.0) for _ in range(50)])
        self.calibration_ms = ms

    def _time(self, fn):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def hold(self, ms: float):
        n = max(int(ms * self.per_ms), 1)
        if self.kind == "sleep":
            self.torch.cuda._sleep(n)
        else:
            for _ in range(n):
                self.buf.mul_(1.0)

    def measure(self, ms: float) -> float:
        return self._time(lambda: self.hold(ms))

    def tune(self, ms: float) -> float:
        """The calibration run is shorter than the gate and the delay is not linear in its count (the clocks ramp): measure the gate
        at the length it will have and rescale until it lasts at least what is asked.  -> its measured length."""
        for _ in range(6):
            got = self.measure(ms)
            if got >= ms:
                return got
            self.per_ms *= 1.1 * ms / max(got, 1e-3)
        return self.measure(ms)


# ---- a row ----------------------------------------------------------------------------------------------------------------------------
SENTINEL_F, SENTINEL_I = -6.0221e23, -77777


class Case:
    def __init__(self, row, call, bufs=None, real=None, stale=None, outs=None, inout=(), state=None, reset=None, keep=None, call_off=None):
        self.row, self.call = row, call
        self.call_off = call_off   # call_off(T): the row's call with the entry point under test alone issued under stream T (a control)
        self.bufs, self.real, self.stale = bufs or {}, real or {}, stale or {}
        self.outs, self.inout, self.state, self.reset = outs or {}, tuple(inout), state, reset
        self.keep = keep   # whatever must outlive the rows (solvers, tracks)
        self.cls, self.sync = row_class(row)
        assert set(self.bufs) == set(self.real) == set(self.stale), row
        for k, t in self.bufs.items():
            for src in (self.real[k], self.stale[k]):
                assert src.shape == t.shape and src.dtype == t.dtype and src.data_ptr() != t.data_ptr(), (row, k)
        assert set(self.inout) <= set(self.bufs), row


def like(d):
    """Fresh buffers of the shapes of d, holding a copy (never uninitialised memory: every buffer is valid data at all times)."""
    return {k: v.clone() for k, v in d.items()}


def _load(case, src):
    for k, t in case.bufs.items():
        t.copy_(src[k])


def _tensors(d):
    """(the binding hangs a list of the tensors it must keep alive on the result dictionary it is given)"""
    import torch

    return {k: v for k, v in d.items() if torch.is_tensor(v)}


def _sentinel(case):
    for t in _tensors(case.outs).values():
        t.fill_(SENTINEL_F if t.is_floating_point() else SENTINEL_I)


def _collect(case):
    import torch

    got = {"out " + k: v.clone() for k, v in _tensors(case.outs).items()}
    got.update({"in place " + k: case.bufs[k].clone() for k in case.inout})
    if case.state is not None:
        for k, v in case.state().items():
            got["state " + k] = v.clone() if torch.is_tensor(v) else torch.as_tensor(np.ascontiguousarray(v))
    return got


def reference(case, which: str = "real"):
    """Step a: on the default stream, once untimed (workspace growth, first launches), once timed.  -> (want, host seconds)."""
    import torch

    src = case.real if which == "real" else case.stale
    sec = 0.0
    for _ in range(2):
        if case.reset:
            case.reset()
        _load(case, src)
        _sentinel(case)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        case.call()
        sec = time.perf_counter() - t0
        torch.cuda.synchronize()
    want = _collect(case)
    torch.cuda.synchronize()
    return want, sec


def gated(case, gate: Gate, gate_ms: float, call_stream=None, wipe: bool = True):
    """Step b: `stale` in the buffers, a fresh stream S held by the gate, `real` copied in on S, the call, the outputs and the state
    cloned on S, `stale` put back on S.  call_stream: the detector control -- the call alone is made under that stream instead
    (wipe=False leaves out the stream's own sentinel fill, so that what such a call wrote during the gate can be looked at).
    -> (got, whether the gate was still closed when the call returned)."""
    import torch

    if case.reset:
        case.reset()
    _load(case, case.stale)
    _sentinel(case)
    real2 = like(case.real)
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        gate.hold(gate_ms)
        g = torch.cuda.Event()
        g.record()
        _load(case, real2)
        if wipe:
            _sentinel(case)   # on S, behind the gate: what work that left the stream wrote during the gate is wiped before the clone
        if call_stream is None:
            case.call()
        elif case.call_off is not None:
            case.call_off(call_stream)
            call_stream.synchronize()
        else:
            with torch.cuda.stream(call_stream):
                case.call()
            call_stream.synchronize()
        closed = not g.query()
        got = _collect(case)
        _load(case, case.stale)
    torch.cuda.synchronize()
    return got, closed


def bits_equal(a, b) -> bool:
    """Bit for bit (a failed solve may leave a NaN, which compares unequal to itself as a number)."""
    import torch

    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point():
        view = {8: torch.int64, 4: torch.int32}[a.element_size()]
        return torch.equal(a.contiguous().view(view), b.contiguous().view(view))
    return torch.equal(a, b)


def differences(got: dict, want: dict):
    assert set(got) == set(want), (sorted(got), sorted(want))
    return [k for k in want if not bits_equal(got[k].cpu(), want[k].cpu())]


# ---- builders ---------------------------------------------------------------------------------------------------------------------------
B, DT = 70, 0.025
KEYS9 = ("x_ic", "u_ic", "X_ref", "U_ref", "T_ref", "bound_left", "bound_right", "curvatures", "vel_ref")
REF7 = KEYS9[2:]


def dev(a, dtype=None):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda")


def _i32(a):
    import torch

    return dev(a, torch.int32)


def _empty(shape, dtype=None):
    import torch

    return torch.zeros(shape, dtype=dtype or torch.float64, device="cuda")


def _ctrack(s, trk):
    return s._ctrack(trk)


def query_point(X_ref, x_ic, L):
    """racing_mpc.cpp:219-223,249-254: the last knot of the reference, its abscissa aligned with the car's."""
    import torch

    s_last, s0 = X_ref[0, -1], x_ic[0]
    kk = (s0 - s_last).abs() + L / 2
    return torch.stack([s_last + (kk - torch.fmod(kk, L)) * torch.sign(s0 - s_last), X_ref[1, -1]]).contiguous()


def _solve_outs(s, n=B, lam=0, f32=False):
    import torch

    o = s.alloc_outputs(n, aos=False)
    if f32:
        o = {k: (v.float() if v.is_floating_point() else v) for k, v in o.items()}
    if lam:
        o["convex_combi_optm"] = _empty((lam, n))
    for v in o.values():
        v.zero_()
    return o


def _cold_inputs(pkg, s, trk, L, seed, n=B, near=None):
    """The nine input arrays of a solve: a cold start (lmpc_prepare_batch) at a draw of initial states."""
    if near is None:
        x, u = pkg.workloads.sample_initial_states("barc", n, L, [-0.01, -0.3], [0.01, 0.3], seed=seed)
    else:
        x, u = pkg.workloads.sample_states_near_laps(near, n, L, seed=seed)
    inp = s.prepare(trk, x.T.copy(), DT)
    inp["u_ic"] = dev(u.T.copy())
    return {k: inp[k].clone() for k in KEYS9}


def _one_period_on(s, trk, L, inp9, **solve_kw):
    """The inputs of the next period (the shifted plan as references: what a warm start is given) and the solution they come from."""
    inp = dict(like(inp9), L=L)
    out = _solve_outs(s, inp["x_ic"].shape[1], lam=solve_kw.pop("lam", 0))
    sol = s.solve(inp, out, **solve_kw)
    x, u = inp["x_ic"].clone(), inp["u_ic"].clone()
    s.loop_advance(trk, inp, sol, x, u, DT, DT / 2, 2)
    inp["x_ic"], inp["u_ic"] = x, u
    return {k: inp[k] for k in KEYS9}, sol


SETTLE = 6   # periods of the closed loop behind a cold start before a plan is taken as a warm start: most are then accepted


def _periods_on(s, trk, L, inp9, periods=SETTLE):
    for _ in range(periods):
        inp9, _ = _one_period_on(s, trk, L, inp9)
    return inp9


def _host_problem(inp9, b=0):
    """Problem b as the host entry points take it: column-major 6 x N, 2 x (N-1), plain per-knot rows."""
    a = {k: v.cpu().numpy() for k, v in inp9.items()}
    col = lambda t: np.ascontiguousarray(t, dtype=np.float64)   # noqa: E731
    return [col(a["x_ic"][:, b]), col(a["u_ic"][:, b]), col(a["X_ref"][:, :, b].T), col(a["U_ref"][:, :, b].T), col(a["T_ref"][:, b]),
            col(a["bound_left"][:, b]), col(a["bound_right"][:, b]), col(a["curvatures"][:, b]), col(a["vel_ref"][:, b])]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _solve_host(s, L, hx, warm=None, ss=None, lam_ref=None):
    """lmpc_solve_host / _warm / _warm_ss -> host results as one dict of arrays."""
    N = s.N
    S = 0 if ss is None else ss[1].size
    X, U, dU, lam = np.zeros((N, 6)), np.zeros((N - 1, 2)), np.zeros((N - 1, 2)), np.zeros(max(S, 1))
    st, it = C.c_int32(-1), C.c_int32(-1)
    s.use_current_stream()
    head = [s._h] + [_p(a) for a in hx] + [C.c_double(L)]
    tail = [C.byref(st), C.byref(it)]
    if warm is None:
        rc, who = s.lib.lmpc_solve_host(*head, None, None, _p(X), _p(U), _p(dU), None, *tail), "lmpc_solve_host"
    elif ss is None:
        rc, who = s.lib.lmpc_solve_host_warm(*head, _p(warm[0]), _p(warm[1]), _p(X), _p(U), _p(dU), *tail), "lmpc_solve_host_warm"
    else:
        rc = s.lib.lmpc_solve_host_warm_ss(*head, _p(ss[0]), _p(ss[1]), _p(warm[0]), _p(warm[1]), _p(lam_ref), _p(X), _p(U), _p(dU), _p(lam), *tail)
        who = "lmpc_solve_host_warm_ss"
    s._check(rc, who)
    return {"X": X, "U": U, "dU": dU, "lam": lam, "status": np.array([st.value, it.value], dtype=np.int32)}


def build_tracking(pkg):
    import torch

    tr = pkg.workloads.synthetic_track("barc")
    L = float(tr["L"])
    veh = pkg.presets.barc_vehicle()
    mk = lambda N=20: pkg.Solver(pkg.presets.barc_tracking_mpc(N), veh, device=0)   # noqa: E731
    s, s_ord, s_tim, s41 = mk(), mk(), mk(), mk(41)
    trk = s.device_track(tr)
    real, stale = _cold_inputs(pkg, s, trk, L, 1), _cold_inputs(pkg, s, trk, L, 2)
    cases = []

    def solve_case(row, sv, real, stale, extra=None, **kw):
        bufs, outs = like(stale), _solve_outs(sv)
        if extra:
            bufs.update(extra[0])
            real, stale = dict(real, **extra[1]), dict(stale, **extra[2])
        return Case(row, lambda: sv.solve(dict({k: bufs[k] for k in KEYS9}, L=L), outs, **kw), bufs, real, stale, outs, keep=sv)

    cases.append(solve_case("solve f64 N=20 cold", s, real, stale))
    # warm: the shifted plan of one period on; the flags are handle-held state (a cold solve clears them)
    wreal, wstale = _periods_on(s, trk, L, real), _periods_on(s, trk, L, stale)
    wb, wo, scratch = like(wstale), _solve_outs(s), _solve_outs(s)
    wo["accepted"] = _empty((B,), torch.int32)

    def warm_call():
        s.solve(dict(wb, L=L), wo, warm=True)
        s.warm_accepted(B, out=wo["accepted"])

    cases.append(Case("solve f64 N=20 warm", warm_call, wb, wreal, wstale, wo, reset=lambda: s.solve(dict(wb, L=L), scratch), keep=s))
    # launch order: the pointer is registered once, the permutation in it is an input
    perm = lambda inp9: s_ord.launch_order_from_iters(s_ord.solve(dict(like(inp9), L=L))["iters"]).clone()   # noqa: E731
    order = _i32(np.arange(B))
    s_ord.set_launch_order(order)
    assert s_ord._launch_order.data_ptr() == order.data_ptr()
    cases.append(solve_case("solve f64 N=20 launch order", s_ord, real, stale, extra=({"order": order}, {"order": perm(real)}, {"order": perm(stale)})))
    s_tim.enable_timing(True)
    cases.append(solve_case("solve f64 N=20 timing events", s_tim, real, stale))
    trk41 = s41.device_track(tr)
    cases.append(solve_case("solve f64 N=41 two waves", s41, _cold_inputs(pkg, s41, trk41, L, 3), _cold_inputs(pkg, s41, trk41, L, 4)))
    f32 = lambda d: {k: v.float() for k, v in d.items()}   # noqa: E731
    fb, fo = f32(stale), _solve_outs(s, f32=True)
    cases.append(Case("solve f32 N=20", lambda: s.solve_f32(fb, fo), fb, f32(real), f32(stale), fo, keep=s))
    # one problem through host pointers
    hold = {}
    hx, hw = _host_problem(real), _host_problem(wreal)
    plan = (hw[2].copy(), hw[3].copy())
    cases.append(Case("solve_host", lambda: hold.update(a=_solve_host(s, L, hx)), state=lambda: hold["a"], keep=s))
    cases.append(Case("solve_host_warm", lambda: hold.update(b=_solve_host(s, L, hw, warm=plan)), state=lambda: hold["b"], keep=s))
    # lmpc_synchronize behind a launch
    xb = {"x": real["x_ic"].clone(), "u": real["u_ic"].clone()}

    def sync_call():
        s.plant_step(trk, xb["x"], xb["u"], DT / 2, 2)
        s.synchronize()

    cases.append(Case("synchronize", sync_call, xb, {"x": real["x_ic"], "u": real["u_ic"]}, {"x": stale["x_ic"], "u": stale["u_ic"]},
                      inout=("x",), keep=(s, trk)))
    return cases


def build_learning(pkg):
    import torch

    tr = pkg.workloads.synthetic_track("barc")
    L = float(tr["L"])
    cfg = dict(pkg.presets.barc_lmpc(20, 2))
    S = int(cfg["num_ss_pts"])
    laps = pkg.workloads.synthetic_laps(tr, 2)
    s = pkg.Solver(cfg, pkg.presets.barc_vehicle(), device=0)
    s.set_safe_set(laps, L)
    trk = s.device_track(tr)
    cases = []

    def draw(seed):
        d = _cold_inputs(pkg, s, trk, L, seed, near=laps)
        d["query"] = query_point(d["X_ref"], d["x_ic"], L)
        d["ss_x"], d["ss_j"], _ = s.ss_query(d["query"])
        d["ss_idx"], _ = s.ss_query_idx(d["query"])
        return d

    real, stale = draw(5), draw(6)
    pick = lambda d, keys: {k: d[k] for k in keys}   # noqa: E731
    qb = like(pick(stale, ("query",)))
    qo = {"ss_x": _empty((6, S, B)), "ss_j": _empty((S, B)), "n_found": _empty((B,), torch.int32)}
    cases.append(Case("ss_query", lambda: s.ss_query(qb["query"], out=(qo["ss_x"], qo["ss_j"], qo["n_found"])), qb, pick(real, ("query",)),
                      pick(stale, ("query",)), qo, keep=s))
    ib = like(pick(stale, ("query",)))
    io = {"ss_idx": _empty((S, B), torch.int32), "n_found": _empty((B,), torch.int32)}
    cases.append(Case("ss_query_idx", lambda: s.ss_query_idx(ib["query"], out=(io["ss_idx"], io["n_found"])), ib, pick(real, ("query",)),
                      pick(stale, ("query",)), io, keep=s))

    def solve_case(row, keys, mixed):
        bufs, outs = like(pick(stale, KEYS9 + keys)), _solve_outs(s, lam=S)
        kw = (lambda: dict(ss_idx=bufs["ss_idx"])) if keys == ("ss_idx",) else (lambda: dict(ss_x=bufs["ss_x"], ss_j=bufs["ss_j"]))
        return Case(row, lambda: s.solve(dict({k: bufs[k] for k in KEYS9}, L=L), outs, mixed=mixed, **kw()), bufs, pick(real, KEYS9 + keys),
                    pick(stale, KEYS9 + keys), outs, keep=s)

    cases.append(solve_case("learning solve by arrays", ("ss_x", "ss_j"), False))
    cases.append(solve_case("learning solve by ss_idx", ("ss_idx",), False))
    cases.append(solve_case("learning solve by arrays, mixed", ("ss_x", "ss_j"), True))
    cases.append(solve_case("learning solve by ss_idx, mixed", ("ss_idx",), True))

    # the warm start of the learning problem: last period's weights carried onto this period's codes, the solve, its flags
    def next_period(d):
        nxt, sol = _one_period_on(s, trk, L, pick(d, KEYS9), ss_idx=d["ss_idx"], lam=S)
        nxt["idx_prev"], nxt["lam_prev"] = d["ss_idx"].clone(), sol["convex_combi_optm"].clone()
        nxt["query"] = query_point(nxt["X_ref"], nxt["x_ic"], L)
        nxt["idx"] = s.ss_query_idx(nxt["query"])[0].clone()
        return nxt

    def settled(d):
        for _ in range(SETTLE):
            d = next_period(d)
            d["ss_idx"] = d["idx"]
        return d

    def with_plan(d):
        """The plan of a warm start that is accepted: the problem's own optimum and its weights (the closed loop's shifted plan has
        the support right on a quarter of the periods at best, include/lmpc_hip.h; six periods in, on none of these 70)."""
        sol = s.solve(dict(pick(d, KEYS9), L=L), _solve_outs(s, lam=S), ss_idx=d["ss_idx"])
        w = dict(pick(d, KEYS9 + ("query",)), idx_prev=d["ss_idx"].clone(), idx=d["ss_idx"].clone(), lam_prev=sol["convex_combi_optm"].clone(),
                 X_plan=torch.nan_to_num(sol["X_optm"]).clone(), U_plan=torch.nan_to_num(sol["U_optm"]).clone())
        return w

    wreal, wstale = with_plan(settled(real)), with_plan(settled(stale))
    wkeys = KEYS9 + ("idx_prev", "lam_prev", "idx", "X_plan", "U_plan")
    wb, wo, scratch = like(pick(wstale, wkeys)), _solve_outs(s, lam=S), _solve_outs(s, lam=S)
    wo["lam_ref"], wo["accepted"] = _empty((S, B)), _empty((B,), torch.int32)

    def warm_call():
        s.shift_lambda(wb["idx_prev"], wb["lam_prev"], wb["idx"], 0, out=wo["lam_ref"])
        s.solve(dict({k: wb[k] for k in KEYS9}, L=L), wo, ss_idx=wb["idx"],
                warm={"X_optm_ref": wb["X_plan"], "U_optm_ref": wb["U_plan"], "convex_combi_optm_ref": wo["lam_ref"]})
        s.warm_accepted(B, out=wo["accepted"])

    cases.append(Case("warm_ss with shift_lambda", warm_call, wb, pick(wreal, wkeys), pick(wstale, wkeys), wo,
                      reset=lambda: s.solve(dict({k: wb[k] for k in KEYS9}, L=L), scratch, ss_idx=wb["idx"]), keep=s))

    # host pointers.  A store of its own for lmpc_set_safe_set, so that the codes of the rows above stay valid
    s2 = pkg.Solver(cfg, pkg.presets.barc_vehicle(), device=0)
    other = pkg.workloads.synthetic_laps(tr, 2, v0=1.2)
    sb = like(pick(stale, ("query",)))
    so = {"ss_x": _empty((6, S, B)), "ss_j": _empty((S, B)), "n_found": _empty((B,), torch.int32)}

    def store_call():
        s2.use_current_stream()
        s2.set_safe_set(laps, L)
        s2.ss_query(sb["query"], out=(so["ss_x"], so["ss_j"], so["n_found"]))

    cases.append(Case("set_safe_set", store_call, sb, pick(real, ("query",)), pick(stale, ("query",)), so,
                      reset=lambda: s2.set_safe_set(other, L), keep=s2))
    hold = {}
    q0 = np.ascontiguousarray(real["query"][:, 0].cpu().numpy())

    def query_host():
        sx, sj, nf, j0 = np.zeros((S, 6)), np.zeros(S), C.c_int32(-1), C.c_double(0.0)
        s.use_current_stream()
        s._check(s.lib.lmpc_ss_query_host(s._h, _p(q0), _p(sx), _p(sj), C.byref(nf), C.byref(j0)), "lmpc_ss_query_host")
        hold["q"] = {"ss_x": sx, "ss_j": sj, "n_found": np.array([nf.value]), "j0": np.array([j0.value])}

    cases.append(Case("ss_query_host", query_host, state=lambda: hold["q"], keep=s))
    hw = _host_problem(pick(wreal, KEYS9))
    plan = (np.ascontiguousarray(wreal["X_plan"][:, :, 0].cpu().numpy().T), np.ascontiguousarray(wreal["U_plan"][:, :, 0].cpu().numpy().T))
    sx1, sj1, _ = s.ss_query(wreal["query"])
    lam1 = s.shift_lambda(wreal["idx_prev"], wreal["lam_prev"], wreal["idx"], 0)
    ss_host = (np.ascontiguousarray(sx1[:, :, 0].cpu().numpy().T), np.ascontiguousarray(sj1[:, 0].cpu().numpy()))
    lam_host = np.ascontiguousarray(lam1[:, 0].cpu().numpy())
    cases.append(Case("solve_host_warm_ss", lambda: hold.update(w=_solve_host(s, L, hw, warm=plan, ss=ss_host, lam_ref=lam_host)),
                      state=lambda: hold["w"], keep=s))
    return cases


def _lap_near(tr, inp9, seed, n=60):
    """One recorded lap of n samples near the references of a batch (states and inputs within the regression's bandwidth of some
    query), abscissa rising, time stamps 0.02 .. 0.04 s apart: (x [n, 6], u [n, 2], k [n], t [n])."""
    rng = np.random.default_rng(seed)
    X, U = inp9["X_ref"].cpu().numpy(), inp9["U_ref"].cpu().numpy()
    i, b = rng.integers(0, U.shape[1], n), rng.integers(0, U.shape[2], n)
    x = X[:, i, b].T + rng.normal(0, 1, (n, 6)) * 0.1
    u = U[:, i, b].T + rng.normal(0, 1, (n, 2)) * np.array([0.002, 0.05])
    x[:, 0] = np.linspace(0.1, float(tr["L"]) - 0.1, n)
    k = np.interp(x[:, 0], np.arange(tr["M"]) * tr["L"] / tr["M"], tr["curvature"], period=tr["L"])
    return x, u, k, np.cumsum(rng.uniform(0.02, 0.04, n))


def build_regression(pkg):
    tr = pkg.workloads.synthetic_track("barc")
    L = float(tr["L"])
    mk = lambda: pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)   # noqa: E731
    s, s_reg, s_set, s_fr, s_fr2 = mk(), mk(), mk(), mk(), mk()
    trk = s.device_track(tr)
    real, stale = _cold_inputs(pkg, s, trk, L, 7), _cold_inputs(pkg, s, trk, L, 8)
    lap, lap2 = _lap_near(tr, real, 41), _lap_near(tr, stale, 42)
    cases = []
    N = s.N
    lin_keys = ("X_ref", "U_ref", "T_ref", "curvatures")
    pick = lambda d, keys: {k: d[k] for k in keys}   # noqa: E731

    def linearize(sv, d, out):
        sv.use_current_stream()
        sv._check(sv.lib.lmpc_linearize_batch(sv._h, C.c_int32(B), *[C.c_void_p(d[k].data_ptr()) for k in lin_keys],
                                              *[C.c_void_p(out[k].data_ptr()) for k in ("A", "Bm", "g")]), "lmpc_linearize_batch")

    lb = like(pick(stale, lin_keys))
    lo = {"A": _empty((6, 6, N - 1, B)), "Bm": _empty((6, 2, N - 1, B)), "g": _empty((6, N - 1, B))}
    cases.append(Case("linearize", lambda: linearize(s, lb, lo), lb, pick(real, lin_keys), pick(stale, lin_keys), lo, keep=s))

    def with_model(d):
        out = {"A": _empty((6, 6, N - 1, B)), "Bm": _empty((6, 2, N - 1, B)), "g": _empty((6, N - 1, B))}
        linearize(s, d, out)
        return dict(pick(d, ("X_ref", "U_ref")), **out)

    mreal, mstale = with_model(real), with_model(stale)
    abg = ("A", "Bm", "g")

    def regress_case(row, sv, fleet, reset=None):
        bufs = like(mstale)
        fn = sv.fleet_ss_regress if fleet else sv.regress
        return Case(row, lambda: fn(bufs, bufs["A"], bufs["Bm"], bufs["g"]), bufs, mreal, mstale, inout=abg, reset=reset, keep=sv)

    def solve_case(row, sv, reset=None):
        bufs, outs = like(stale), _solve_outs(sv)
        return Case(row, lambda: sv.solve(dict(bufs, L=L), outs), bufs, real, stale, outs, reset=reset, keep=sv)

    s_reg.set_regression_laps([lap], dist_max=1.0)
    cases.append(regress_case("regress", s_reg, False))
    cases.append(solve_case("solve with the shared regression", s_reg))
    # lmpc_set_regression_laps under the stream, the regression that reads the new store behind it
    sb = like(mstale)

    def set_call():
        s_set.use_current_stream()
        s_set.set_regression_laps([lap], dist_max=1.0)
        s_set.regress(sb, sb["A"], sb["Bm"], sb["g"])

    cases.append(Case("set_regression_laps", set_call, sb, mreal, mstale, inout=abg, reset=lambda: s_set.set_regression_laps([lap2], dist_max=1.0),
                      keep=s_set))
    # per car: every ring holds the lap; the packed tables are handle-held state, refilled on the device in front of a use
    for sv in (s_fr, s_fr2):
        sv.fleet_ss_create(B, 64)
        sv.fleet_ss_load([lap], L, car=-1)
    s_fr.fleet_ss_set_regression(dist_max=1.0)
    again = lambda: s_fr.fleet_ss_set_regression(dist_max=1.0)   # noqa: E731  (every stamp stale: the next use packs every car again)
    cases.append(regress_case("fleet_ss_regress", s_fr, True, reset=again))
    cases.append(solve_case("solve with the fleet regression", s_fr, reset=again))
    fb = like(mstale)
    six = (0, 1, 2, 3, 4, 5)

    def refill_call():   # (5, 3) -> (8, 6): the table's size changes, which is when the call waits for the stream
        s_fr2.fleet_ss_set_regression(in_state=six, in_ctrl=(0, 1), out_rows=six, dist_max=1.0)
        s_fr2.fleet_ss_regress(fb, fb["A"], fb["Bm"], fb["g"])

    cases.append(Case("fleet_ss_set_regression refill", refill_call, fb, mreal, mstale, inout=abg,
                      reset=lambda: s_fr2.fleet_ss_set_regression(dist_max=1.0), keep=s_fr2))
    return cases


def build_prep(pkg):
    import torch

    tr = pkg.workloads.synthetic_track("barc")
    L = float(tr["L"])
    s = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    trk = s.device_track(tr)
    N = s.N
    cases = []
    pick = lambda d, keys: {k: d[k] for k in keys}   # noqa: E731
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    limit = float(s.config["x_max"][3])

    def draw(seed, fail_every):
        d = _cold_inputs(pkg, s, trk, L, seed)
        sol = s.solve(dict(like(d), L=L), _solve_outs(s))
        d["X_optm"], d["U_optm"] = torch.nan_to_num(sol["X_optm"]).clone(), torch.nan_to_num(sol["U_optm"]).clone()
        d["status"], d["iters"] = sol["status"].clone(), sol["iters"].clone()
        d["status"][::fail_every] = 1
        d["warm"] = _periods_on(s, trk, L, pick(d, KEYS9))
        rng = np.random.default_rng(seed)
        d["distance"], d["worst_excess"] = dev(rng.uniform(0, 3, B)), dev(rng.uniform(-0.2, 0.1, B))
        d["n_fail"] = dev(rng.integers(0, 4, B), torch.int64)
        d["n_accepted"] = dev(np.array(rng.integers(1, 100)), torch.int64)
        return d

    real, stale = draw(9, 7), draw(10, 5)
    refs = lambda: {k: _empty(stale[k].shape) for k in REF7}   # noqa: E731

    pb, po = like(pick(stale, ("x_ic",))), refs()

    def prepare():
        s.use_current_stream()
        ct = _ctrack(s, trk)
        s._check(s.lib.lmpc_prepare_batch(s._h, C.c_int32(B), C.byref(ct), ptr(pb["x_ic"]), C.c_double(DT), C.c_double(0.9), C.c_double(limit),
                                          *[ptr(po[k]) for k in REF7]), "lmpc_prepare_batch")

    cases.append(Case("prepare", prepare, pb, pick(real, ("x_ic",)), pick(stale, ("x_ic",)), po, keep=(s, trk)))
    fkeys = ("x_ic", "status") + REF7
    fb = like(pick(stale, fkeys))
    cases.append(Case("prepare_failed", lambda: s.prepare_failed(trk, fb["x_ic"], fb["status"], fb, DT, speed_scale=0.9), fb, pick(real, fkeys),
                      pick(stale, fkeys), inout=REF7, keep=s))
    skeys = ("X_optm", "U_optm", "X_ref", "U_ref", "status")
    hb, ho = like(pick(stale, skeys)), refs()

    def shift():
        s.use_current_stream()
        ct = _ctrack(s, trk)
        s._check(s.lib.lmpc_shift_batch(s._h, C.c_int32(B), C.byref(ct), ptr(hb["X_optm"]), ptr(hb["U_optm"]), ptr(hb["X_ref"]), ptr(hb["U_ref"]),
                                        ptr(hb["status"]), C.c_double(DT), C.c_double(0.9), C.c_double(limit), *[ptr(ho[k]) for k in REF7]),
                 "lmpc_shift_batch")

    cases.append(Case("shift", shift, hb, pick(real, skeys), pick(stale, skeys), ho, keep=s))
    xb = like(pick(stale, ("x_ic", "u_ic")))
    cases.append(Case("plant_step", lambda: s.plant_step(trk, xb["x_ic"], xb["u_ic"], DT / 2, 2), xb, pick(real, ("x_ic", "u_ic")),
                      pick(stale, ("x_ic", "u_ic")), inout=("x_ic",), keep=s))
    akeys = ("status", "iters", "X_optm", "U_optm", "x_ic", "u_ic") + REF7 + ("distance", "worst_excess", "n_fail", "n_accepted")
    ab, scratch = like(pick(stale, akeys)), _solve_outs(s)
    warm_inp = dict(like(real["warm"]), L=L)

    def advance():
        s.loop_advance(trk, ab, ab, ab["x_ic"], ab["u_ic"], DT, DT / 2, 2, speed_scale=0.9, restart_failed=True, distance=ab["distance"],
                       worst_excess=ab["worst_excess"], n_fail=ab["n_fail"], n_accepted=ab["n_accepted"])

    # the call reads the warm kernel's own flags: a warm solve of this batch is the handle's last solve when it runs
    cases.append(Case("loop_advance", advance, ab, pick(real, akeys), pick(stale, akeys), inout=akeys[4:],
                      reset=lambda: s.solve(warm_inp, scratch, warm=True), keep=s))
    ib, io = like(pick(stale, ("iters",))), {"order": _empty((B,), torch.int32)}
    cases.append(Case("launch_order_from_iters", lambda: s.launch_order_from_iters(ib["iters"], io["order"]), ib, pick(real, ("iters",)),
                      pick(stale, ("iters",)), io, keep=s))
    return cases


def build_fleet(pkg):
    import torch

    import test_gpu_fleet_loop as FL

    sc = FL.scene(pkg, 20)
    learner, trk, L = sc["learner"], sc["trk"], sc["L"]
    S = int(learner.config["num_ss_pts"])
    roll = lambda d: {k: torch.roll(v, 1, dims=-1).contiguous() for k, v in d.items()}   # noqa: E731  (the neighbour's data: valid, different)
    # every car's recorder in its case's state (test_gpu_fleet_loop.py CASES), through the recorder itself
    FL.prefeed(learner, sc["s0"], L)
    rng = np.random.default_rng(11)
    feed = []
    for j in range(max(len(c[1]) for c in FL.CASES)):
        act = np.array([j < len(FL.CASES[c][1]) for c in FL.CASE], dtype=np.int32)
        s_j = np.array([(sc["s0"][b] if FL.CASES[c][1][j] == "s0" else FL.CASES[c][1][j] * L) if act[b] else 0.0 for b, c in enumerate(FL.CASE)])
        feed.append((dev(np.concatenate([s_j[None, :], rng.normal(size=(5, B))])), dev(rng.normal(size=(2, B))), dev(rng.normal(size=B)),
                     0.025 * j, _i32(act)))

    def restore():
        learner.fleet_ss_reset()
        for x, u, k, t, act in feed:
            learner.fleet_ss_record(x, u, k, t, L, active=act)

    def stats():
        return dict(learner.fleet_ss_stats(B))

    def laps():
        """Every car's closed laps as flat arrays (fleet_ss_get_laps waits for the stream)."""
        learner.use_current_stream()
        per_car = [learner.fleet_ss_get_laps(b) for b in range(B)]
        out = {"n_pts": np.array([l[0].shape[0] for car in per_car for l in car] + [-1], dtype=np.int64),
               "n_laps": np.array([len(car) for car in per_car], dtype=np.int64)}
        for i, name in enumerate("xukt"):
            out[name] = np.concatenate([np.asarray(l[i], dtype=np.float64).reshape(-1) for car in per_car for l in car] + [np.zeros(1)])
        return out

    def ring():
        out = stats()
        FL.close_open_laps(learner, L)   # what went into open laps becomes visible
        out.update(laps())
        return out

    cases = []
    sample = {"x": sc["x"].clone(), "u": sc["u_prev"].clone(), "k": FL.torch_curvature(trk, sc["x"][0]).contiguous(),
              "active": _i32((np.arange(B) % 11 != 0).astype(np.int32))}
    record = lambda b: learner.fleet_ss_record(b["x"], b["u"], b["k"], FL.T_CALL, L, active=b["active"])   # noqa: E731
    rb = like(roll(sample))
    cases.append(Case("fleet_ss_record", lambda: record(rb), rb, sample, roll(sample), state=ring, reset=restore, keep=sc))
    zb = like(roll(sample))

    def reset_call():   # behind a record on the stream: memsets that left the stream would run first and the sample would survive
        record(zb)
        learner.fleet_ss_reset()

    def reset_off(T):
        record(zb)
        with torch.cuda.stream(T):
            learner.fleet_ss_reset()

    def after_reset():
        """One more sample just behind the line, then the counters.  An emptied recorder is only seeded by it; one in which the
        sample recorded before the reset survived (its abscissa and its VALID flag) sees a drop of more than L / 2 from there and
        counts a crossing."""
        FL.close_open_laps(learner, L)
        return stats()

    cases.append(Case("fleet_ss_reset", reset_call, zb, sample, roll(sample), state=after_reset, reset=restore, keep=sc, call_off=reset_off))
    # a store made under the stream (its zero-fill is enqueued there), and the recorder and the counters that read it behind it
    maker = pkg.Solver(learner.config, learner.vehicle, device=0)
    maker.fleet_ss_create(B, 4)
    mo = {k: _empty((B,), torch.int32) for k in ("laps_in_ring", "lap_count", "n_dropped")}
    mo["last_lap_time"] = _empty((B,))

    def create_call():
        maker.fleet_ss_create(B, FL.CAP)
        for x, u, k, t_j, act in feed:
            maker.fleet_ss_record(x, u, k, t_j, L, active=act)
        maker.fleet_ss_stats(B, out=mo)

    cases.append(Case("fleet_ss_create", create_call, outs=mo, reset=lambda: maker.fleet_ss_create(B, 4), keep=maker))
    # the query against rings that hold more samples per lap than a query takes (the scene's laps are a few samples long: every point
    # is a neighbour of every query there): a store of its own, two laps of 60 samples in every car's ring
    asker = pkg.Solver(learner.config, learner.vehicle, device=0)
    asker.fleet_ss_create(B, 64)
    lap_rng = np.random.default_rng(13)
    long_lap = lambda: (np.concatenate([np.sort(lap_rng.uniform(0.1, L - 0.1, 60))[:, None], lap_rng.normal(0, 0.2, (60, 5))], axis=1),   # noqa: E731
                        lap_rng.normal(size=(60, 2)), lap_rng.normal(size=60), np.cumsum(lap_rng.uniform(0.02, 0.04, 60)))
    asker.fleet_ss_load([long_lap(), long_lap()], L, car=-1)
    q = {"query": FL.query_formula(sc["inp"]["X_ref"], sc["x"], L).contiguous()}
    qb = like(roll(q))
    qo = {"ss_x": _empty((6, S, B)), "ss_j": _empty((S, B)), "n_found": _empty((B,), torch.int32)}
    cases.append(Case("fleet_ss_query", lambda: asker.fleet_ss_query(qb["query"], out=(qo["ss_x"], qo["ss_j"], qo["n_found"])), qb, q, roll(q), qo,
                      keep=(sc, asker)))
    to = {k: _empty((B,), torch.int32) for k in ("laps_in_ring", "lap_count", "n_dropped")}
    to["last_lap_time"] = _empty((B,))
    tb = like(roll(sample))

    def stats_call():   # behind a sample on the stream: the counters it reads are the ones that sample moves
        record(tb)
        learner.fleet_ss_stats(B, out=to)

    cases.append(Case("fleet_ss_stats", stats_call, tb, sample, roll(sample), to, reset=restore, keep=sc))
    # the fused period
    st = FL.fresh_state(learner)
    full = {("trk " + k): sc["out_t"][k].clone() for k in ("X_optm", "U_optm", "status")}
    full.update({("lrn " + k): sc["out_l"][k].clone() for k in ("X_optm", "U_optm", "status")})
    full.update(x=sc["x"].clone(), u_prev=sc["u_prev"].clone(), **{k: sc["inp"][k].clone() for k in FL.KEYS}, **{k: v.clone() for k, v in st.items()})
    full.update(distance=_empty((B,)), worst_excess=_empty((B,)), n_fail=_empty((B,), torch.int64))
    ab = like(roll(full))

    def advance():
        sol = lambda p: {k: ab[p + " " + k] for k in ("X_optm", "U_optm", "status")}   # noqa: E731
        learner.fleet_loop_advance(trk, ab, sol("trk"), sol("lrn"), ab["x"], ab["u_prev"], ab, dt=DT, dt_sim=DT / 2, n_sub=2, t=FL.T_CALL,
                                   speed_scale=FL.SPEED, speed_limit=(6.0, 3.0), restart_failed=True, warm_laps=FL.WARM, learn_laps=FL.LEARN,
                                   switch_phase=True, distance=ab["distance"], worst_excess=ab["worst_excess"], n_fail=ab["n_fail"])

    cases.append(Case("fleet_loop_advance", advance, ab, full, roll(full), inout=tuple(k for k in full if k[:4] not in ("trk ", "lrn ")),
                      state=ring, reset=restore, keep=sc))
    # host pointers
    lap_rng = np.random.default_rng(12)
    n = FL.CAP - 1
    lap = (np.concatenate([np.linspace(0.1, L - 0.1, n)[:, None], lap_rng.normal(size=(n, 5))], axis=1), lap_rng.normal(size=(n, 2)),
           lap_rng.normal(size=n), np.cumsum(lap_rng.uniform(0.02, 0.04, n)))
    lb = like(roll(sample))

    def load_call():
        record(lb)
        learner.fleet_ss_load([lap], L, car=-1)

    cases.append(Case("fleet_ss_load", load_call, lb, sample, roll(sample), state=ring, reset=restore, keep=sc))
    gb, hold = like(roll(sample)), {}

    def get_call():   # the sample, the sample that closes the lap it went into, and the read that has to wait for both
        record(gb)
        FL.close_open_laps(learner, L)
        hold["laps"] = laps()

    cases.append(Case("fleet_ss_get_laps", get_call, gb, sample, roll(sample), state=lambda: hold["laps"], reset=restore, keep=sc))
    return cases


def build_track(pkg):
    import torch

    import track_cases as TC
    import vanilla_cases as VC

    t = VC.track("barc")
    L = float(t["L"])
    s = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    spline = s.spline_track(t["spline"])
    cases, n_knots, M = [], 5, 256
    ptr = lambda a: C.c_void_p(a.data_ptr())   # noqa: E731

    def draw(seed):
        rng = np.random.default_rng(seed)
        fr, pose, _ = TC.poses(t["tr"], B * n_knots, seed)
        X = np.concatenate([fr, rng.normal(size=(3, B * n_knots))]).reshape(6, n_knots, B)
        return {"s": dev(rng.uniform(-L, 2 * L, B)), "pose": dev(pose[:, :B]), "s0": dev(fr[0, :B] + rng.normal(0, 0.05, B)),
                "seeded": _i32(rng.integers(0, 2, B)), "X": dev(X)}

    real, stale = draw(21), draw(22)
    pick = lambda d, keys: {k: d[k] for k in keys}   # noqa: E731
    sb, so = like(pick(stale, ("s",))), {"out": _empty((7, B))}
    cases.append(Case("track_sample", lambda: s.track_sample(spline, sb["s"], out=so["out"]), sb, pick(real, ("s",)), pick(stale, ("s",)), so,
                      keep=(s, spline)))
    to = {k: _empty((M,)) for k in ("curvature", "bound_left", "bound_right", "vel")}

    def tabulate():
        s.use_current_stream()
        s._check(s.lib.lmpc_spline_track_tabulate(s._h, spline._p, C.c_int32(M), *[ptr(to[k]) for k in ("curvature", "bound_left", "bound_right", "vel")]),
                 "lmpc_spline_track_tabulate")

    cases.append(Case("tabulate", tabulate, outs=to, keep=s))
    gk = ("pose", "s0", "seeded")
    gb, go = like(pick(stale, gk)), {"frenet": _empty((3, B)), "status": _empty((B,), torch.int32)}
    cases.append(Case("global_to_frenet", lambda: s.global_to_frenet(spline, gb["pose"], gb["s0"], gb["seeded"], out=(go["frenet"], go["status"])), gb,
                      pick(real, gk), pick(stale, gk), go, keep=s))
    fb, fo = like(pick(stale, ("X",))), {"pose": _empty((3, n_knots, B))}
    cases.append(Case("frenet_to_global", lambda: s.frenet_to_global(spline, fb["X"], out=fo["pose"]), fb, pick(real, ("X",)), pick(stale, ("X",)), fo,
                      keep=s))
    # a track made under the stream, and the first launch that reads its tables
    cb, co, made = like(pick(stale, ("s",))), {"out": _empty((7, B))}, []

    def create():
        made.append(s.spline_track(t["spline"]))
        s.track_sample(made[-1], cb["s"], out=co["out"])

    def drop():
        while made:
            made.pop().close()

    cases.append(Case("spline_track_create", create, cb, pick(real, ("s",)), pick(stale, ("s",)), co, reset=drop, keep=(s, made)))
    return cases


def build_ekf(pkg):
    import torch

    import ekf_cases as EC

    n = 64
    sc = EC.scenario(n, periods=2)
    s = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    observations = ((0,), (3, 5), (5, 2, 0), (0, 1, 2, 3), (1, 2, 3, 4, 5), (0, 1, 2, 3, 4, 5))
    to_dev = lambda a: dev(np.moveaxis(np.asarray(a, dtype=np.float64), 0, -1))   # noqa: E731  [B, ...] -> [...][B]
    cfg = sc["cfg"]
    sig = np.array([0.02, 0.02, 0.01, 0.05, 0.05, 0.05])
    truth = sc["x0"].copy()
    truth[:, 3] = np.maximum(truth[:, 3], 1.5)
    x0, P0, u0 = to_dev(sc["x0"]), to_dev(sc["P0"]), to_dev(sc["updates"][0][3])
    z0 = to_dev(truth + np.random.default_rng(30).normal(0, 1, (n, 6)) * sig)
    R0 = to_dev(EC.spd(np.random.default_rng(31), n, 6))
    NS0, NS1 = 5_000_000, 10_000_000

    def make(register=True):
        """The filter anew (its gain has no setter): every observation, a start per car, and one full-width update behind it, so that
        the gain is not zero and P not diagonal.  The time of the last update is host state and starts again at NS0."""
        s.ekf_create(n, cfg["x0"], cfg["P0"], cfg["Q"], cfg["x_min"], cfg["x_max"])
        if not register:
            s.ekf_set_state(x0, P0)
            return
        for rows in observations:
            s.ekf_register_observation(rows)
        s.ekf_set_state(x0, P0)
        s.ekf_update_control(u0)
        s.ekf_initialize(0)
        s.ekf_update(5, z0, R0, NS0)

    def get():
        g = s.ekf_get()
        return {k: g[k] for k in ("x", "P", "K")}

    def draw(seed):
        rng = np.random.default_rng(seed)
        d = {"x": to_dev(sc["x0"] + rng.normal(0, 0.05, (n, 6))), "P": to_dev(EC.spd(rng, n, 6, scale=0.5).reshape(n, 36)),
             "u": to_dev(sc["updates"][0][3] * rng.uniform(0.5, 1.5, (n, 1)))}
        for i, rows in enumerate(observations):
            z = truth[:, list(rows)] + rng.normal(0, 1, (n, len(rows))) * sig[list(rows)]
            d["z%d" % i], d["R%d" % i] = to_dev(z), to_dev(EC.spd(rng, n, len(rows)))
        return d

    real, stale = draw(32), draw(33)
    pick = lambda d, keys: {k: d[k] for k in keys}   # noqa: E731
    cases = []
    make()
    sb = like(pick(stale, ("x", "P")))
    cases.append(Case("ekf_set_state", lambda: s.ekf_set_state(sb["x"], sb["P"]), sb, pick(real, ("x", "P")), pick(stale, ("x", "P")), state=get,
                      reset=make, keep=s))

    def outs(nz):
        o = {"x": _empty((6, n)), "P": _empty((6, 6, n)), "flags": _empty((n,), torch.int32)}
        if nz:
            o["Kz"] = _empty((6, nz, n))
        return o

    ub, uo = like(pick(stale, ("u",))), outs(0)

    def control():   # the control is read by the next prediction
        s.ekf_update_control(ub["u"])
        s.ekf_update(-1, None, None, NS1, out=(uo["x"], uo["P"], None, uo["flags"]))

    cases.append(Case("ekf_update_control", control, ub, pick(real, ("u",)), pick(stale, ("u",)), uo, state=get, reset=make, keep=s))
    po = outs(0)
    cases.append(Case("ekf_update predict only", lambda: s.ekf_update(-1, None, None, NS1, out=(po["x"], po["P"], None, po["flags"])), outs=po,
                      state=get, reset=make, keep=s))
    for i, rows in enumerate(observations):
        keys = ("z%d" % i, "R%d" % i)
        bufs, o = like(pick(stale, keys)), outs(len(rows))
        cases.append(Case("ekf_update nz=%d" % len(rows),
                          lambda i=i, bufs=bufs, o=o, keys=keys: s.ekf_update(i, bufs[keys[0]], bufs[keys[1]], NS1, out=(o["x"], o["P"], o["Kz"], o["flags"])),
                          bufs, pick(real, keys), pick(stale, keys), o, state=get, reset=make, keep=s))
    go = {"x": _empty((6, n)), "P": _empty((36, n)), "K": _empty((6, sum(len(r) for r in observations), n))}

    gb = like(pick(stale, ("z5", "R5")))

    def get_call():   # behind an update on the stream: the store it copies is the one that update writes
        s.ekf_update(5, gb["z5"], gb["R5"], NS1)
        s._check(s.lib.lmpc_ekf_get(s._h, C.c_int32(n), *[C.c_void_p(go[k].data_ptr()) for k in ("x", "P", "K")], None, None), "lmpc_ekf_get")

    cases.append(Case("ekf_get", get_call, gb, pick(real, ("z5", "R5")), pick(stale, ("z5", "R5")), go, reset=make, keep=s))
    # the whole filter made under the stream: the zero-fill and the seed of lmpc_ekf_create are enqueued there, and everything behind
    # them reads what they wrote
    co = {"x": _empty((6, n)), "P": _empty((36, n)), "K": _empty((6, sum(len(r) for r in observations), n))}

    def create_call():
        make()
        s._check(s.lib.lmpc_ekf_get(s._h, C.c_int32(n), *[C.c_void_p(co[k].data_ptr()) for k in ("x", "P", "K")], None, None), "lmpc_ekf_get")

    cases.append(Case("ekf_create", create_call, outs=co, reset=make, keep=s))
    # registration under the stream (it waits for it), then the first update on the new gain
    rb, ro = like(pick(stale, ("z2", "R2"))), outs(3)

    def register():
        oid = s.ekf_register_observation(observations[2])
        s.ekf_initialize(0)
        s.ekf_update(oid, rb["z2"], rb["R2"], NS0, out=(ro["x"], ro["P"], ro["Kz"], ro["flags"]))

    cases.append(Case("ekf_register_observation", register, rb, pick(real, ("z2", "R2")), pick(stale, ("z2", "R2")), ro, state=get,
                      reset=lambda: make(register=False), keep=s))
    return cases


def build_lqr(pkg):
    import torch

    import lqr_cases as LC

    s = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    N, dt = 21, 0.01
    cfg, other = LC.config(N, dt), LC.general_config(N, dt)
    s.lqr_create(cfg, B)

    def draw(seed):
        sc = LC.scenario("barc", N, dt, seed, B=B)
        return {k: dev(np.moveaxis(sc[k], 0, -1)) for k in ("x_ic", "X_ref", "U_ref")}

    real, stale = draw(13), draw(14)

    def outs(gains):
        o = {"X_optm": _empty((6, N, B)), "U_optm": _empty((2, N - 1, B)), "flags": _empty((B,), torch.int32)}
        if gains:
            o["K"], o["P0"] = _empty((2, 6, N - 1, B)), _empty((6, 6, B))
        return o

    cases = []
    for row, gains in (("lqr_solve with gains", True), ("lqr_solve without gains", False)):
        bufs, o = like(stale), outs(gains)
        cases.append(Case(row, lambda bufs=bufs, o=o: s.lqr_solve(bufs["x_ic"], bufs["X_ref"], bufs["U_ref"], out=o), bufs, real, stale,
                          {k: v for k, v in o.items()}, reset=lambda: s.lqr_create(cfg, B), keep=s))
    cb, co = like(stale), outs(True)

    def create():
        s.lqr_create(cfg, B)
        s.lqr_solve(cb["x_ic"], cb["X_ref"], cb["U_ref"], out=co)

    cases.append(Case("lqr_create", create, cb, real, stale, {k: v for k, v in co.items()}, reset=lambda: s.lqr_create(other, B), keep=s))
    return cases


def build_vanilla(pkg):
    import torch

    import vanilla_cases as VC

    sc = VC.scenario("barc", B=B)
    s = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    spline = s.spline_track(sc["trk"]["spline"])
    table = s.device_track(sc["trk"]["table"])
    periods = 3
    s.vanilla_create(sc["cfg"], B)
    to_dev = lambda a: dev(np.moveaxis(np.asarray(a, dtype=np.float64), 0, -1))   # noqa: E731
    x_fix, integ_fix = to_dev(sc["x0"]), dev(np.random.default_rng(50).uniform(-1, 1, B))

    def nonzero():   # a PID state with every entry set: the integral given, error and last_error from one decision
        s.vanilla_reset(B, integ_fix)
        s.vanilla_solve(spline, x_fix, None, speed_scale=sc["speed_scale"])
        s.vanilla_solve(spline, x_fix, None, speed_scale=1.0)

    def get():
        o = _empty((3, B))
        s.use_current_stream()
        s._check(s.lib.lmpc_vanilla_get(s._h, C.c_int32(B), *[C.c_void_p(o[i].data_ptr()) for i in range(3)]), "lmpc_vanilla_get")
        return {"pid": o}

    def draw(seed):
        rng = np.random.default_rng(seed)
        other = VC.scenario("barc", B=B)
        x = other["x0"].copy()
        x[:, 0] = np.mod(x[:, 0] + rng.uniform(0, 1, B), sc["trk"]["L"])
        x[:, 3] = rng.uniform(1.0, 2.0, B)
        return {"x": to_dev(x), "vel_ref": dev(rng.uniform(0.5, 2.5, B)), "integral": dev(rng.uniform(-1, 1, B)),
                "distance": dev(rng.uniform(0, 2, B)), "worst_excess": dev(rng.uniform(-0.3, 0.0, B))}

    real, stale = draw(51), draw(52)
    pick = lambda d, keys: {k: d[k] for k in keys}   # noqa: E731
    cases = []
    ib = like(pick(stale, ("integral",)))

    def reset_call():   # behind a decision on the stream: a memset that left the stream would run first and the errors would survive
        s.vanilla_solve(spline, x_fix, None, speed_scale=0.8)
        s.vanilla_reset(B, ib["integral"])

    def reset_off(T):
        s.vanilla_solve(spline, x_fix, None, speed_scale=0.8)
        with torch.cuda.stream(T):
            s.vanilla_reset(B, ib["integral"])

    cases.append(Case("vanilla_reset", reset_call, ib, pick(real, ("integral",)), pick(stale, ("integral",)), state=get, reset=nonzero, keep=s,
                      call_off=reset_off))
    go = {"pid": _empty((3, B))}

    gb = like(pick(stale, ("x", "vel_ref")))

    def get_call():   # behind a decision on the stream: the PID state it copies is the one that decision leaves
        s.vanilla_solve(spline, gb["x"], gb["vel_ref"], speed_scale=sc["speed_scale"])
        s._check(s.lib.lmpc_vanilla_get(s._h, C.c_int32(B), *[C.c_void_p(go["pid"][i].data_ptr()) for i in range(3)]), "lmpc_vanilla_get")

    cases.append(Case("vanilla_get", get_call, gb, pick(real, ("x", "vel_ref")), pick(stale, ("x", "vel_ref")), go, reset=nonzero, keep=s))
    sb = like(pick(stale, ("x", "vel_ref")))
    so = {"u_out": _empty((3, B)), "u_model": _empty((2, B)), "flags": _empty((B,), torch.int32)}
    cases.append(Case("vanilla_solve", lambda: s.vanilla_solve(spline, sb["x"], sb["vel_ref"], speed_scale=sc["speed_scale"], out=so), sb,
                      pick(real, ("x", "vel_ref")), pick(stale, ("x", "vel_ref")), so, state=get, reset=nonzero, keep=(s, spline, table)))
    rk = ("x", "distance", "worst_excess")
    rb = like(pick(stale, rk))
    ro = {"X_log": _empty((6, periods, B)), "U_log": _empty((2, periods, B)), "k_log": _empty((periods, B)), "flags": _empty((B,), torch.int32)}
    cases.append(Case("vanilla_rollout", lambda: s.vanilla_rollout(spline, table, rb["x"], periods, sc["dt_sim"], sc["n_sub"], speed_scale=sc["speed_scale"],
                                                                   distance=rb["distance"], worst_excess=rb["worst_excess"], out=ro),
                      rb, pick(real, rk), pick(stale, rk), ro, inout=rk, state=get, reset=nonzero, keep=s))
    cb = like(pick(stale, ("x", "vel_ref")))
    co = {"u_out": _empty((3, B)), "u_model": _empty((2, B)), "flags": _empty((B,), torch.int32)}

    def create():   # replaces the store: the PID state starts at zero, whatever the old one held
        s.vanilla_create(sc["cfg"], B)
        s.vanilla_solve(spline, cb["x"], cb["vel_ref"], speed_scale=sc["speed_scale"], out=co)

    cases.append(Case("vanilla_create", create, cb, pick(real, ("x", "vel_ref")), pick(stale, ("x", "vel_ref")), co, state=get, reset=nonzero, keep=s))
    return cases


def build_sqp(pkg):
    import sqp_cases as SC

    sm = SC.sample(pkg, "tracking N = 8")
    s = pkg.Solver(*sm["preset"], device=0)
    n = 16
    cut = lambda lo: {k: dev(np.asarray(sm["inp"][k], dtype=np.float64)[..., lo:lo + n]) for k in KEYS9}   # noqa: E731
    real, stale = cut(0), cut(n)
    L = float(sm["inp"].get("L", 0.0))
    bufs, hold = like(stale), {}
    keys = ("X_optm", "U_optm", "dU_optm", "status", "iters", "sqp_iters", "sqp_move", "defect")

    def call():
        r = s.solve_full_dynamics(dict(bufs, L=L), max_sqp=4)
        hold["a"] = {k: r[k] for k in keys}

    host_inp = {k: np.asarray(sm["inp"][k], dtype=np.float64) for k in KEYS9}

    def host_call():
        s.use_current_stream()
        hold["b"] = s.solve_full_dynamics_host(dict(host_inp, L=L), b=3, max_sqp=4)

    return [Case("solve_full_dynamics", call, bufs, real, stale, state=lambda: hold["a"], keep=s),
            Case("solve_full_dynamics_host", host_call, state=lambda: hold["b"], keep=s)]


BUILDERS = {"tracking": build_tracking, "learning": build_learning, "regression": build_regression, "prep": build_prep, "fleet": build_fleet,
            "track": build_track, "ekf": build_ekf, "lqr": build_lqr, "vanilla": build_vanilla, "sqp": build_sqp}


def build(pkg, group: str) -> dict:
    cases = {c.row: c for c in BUILDERS[group](pkg)}
    assert set(cases) == {r for r, (g, _) in ROWS.items() if g == group}, (group, sorted(cases))
    return cases
