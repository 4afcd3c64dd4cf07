"""Which stream the entry points of include/lmpc_hip_cars_model.h work on: stream_cases.py's classification and rows for the per-car
single-track controller model -- the linearisation is asynchronous, the two switch functions are host-only
(tests/test_stream_table_cars_model.py holds the table to that header without a GPU, tests/test_gpu_streams_cars_model.py runs the
rows on one).  Classes, reference(), gated() and the gate are stream_cases.py's, Case is stream_cases_cars.py's with this module's
rows."""
from __future__ import annotations

import cars_model_cases as MC
import stream_cases as SC

# name: (class, sync, io), as stream_cases.TABLE
TABLE = {
    "lmpc_linearize_cars_batch": (SC.ASYNC, False, True),
    "lmpc_cars_set_controller_model": (SC.HOST, False, False),
    "lmpc_cars_get_controller_model": (SC.HOST, False, False),
}

# row id: (group, the entry points the row's call makes on the gated stream)
ROWS = {
    "linearize_cars": ("cars_model", ("lmpc_linearize_cars_batch",)),
    "cars controller model on, then solve": ("cars_model", ("lmpc_cars_set_controller_model", "lmpc_solve_batch")),
    "cars controller model on, then solve_f32": ("cars_model", ("lmpc_cars_set_controller_model", "lmpc_solve_batch_f32")),
}


def entry(name: str):
    return TABLE[name] if name in TABLE else SC.TABLE[name]


def row_class(row: str):
    """(class, sync) of a row, by stream_cases.row_class's rule (a host-only entry point makes no row blocking)."""
    fns = ROWS[row][1]
    blocking = any(entry(f)[0] == SC.BLOCKING for f in fns)
    return (SC.BLOCKING if blocking else SC.ASYNC), any(entry(f)[1] for f in fns)


class Case(SC.Case):
    """stream_cases.Case for a row of ROWS above (that class looks its row up in its own module's table)."""

    def __init__(self, row, call, bufs=None, real=None, stale=None, outs=None, inout=(), state=None, reset=None, keep=None):
        self.row, self.call, self.call_off = row, call, None
        self.bufs, self.real, self.stale = bufs or {}, real or {}, stale or {}
        self.outs, self.inout, self.state, self.reset, self.keep = outs or {}, tuple(inout), state, reset, keep
        self.cls, self.sync = row_class(row)
        assert set(self.bufs) == set(self.real) == set(self.stale), row
        for k, t in self.bufs.items():
            for src in (self.real[k], self.stale[k]):
                assert src.shape == t.shape and src.dtype == t.dtype and src.data_ptr() != t.data_ptr(), (row, k)
        assert set(self.inout) <= set(self.bufs), row


def build(pkg):
    """The three rows: the linearisation of a cold start's references on three kinds of car, and an fp64 and a single-precision solve
    of the same cold start behind the switch -- before every run of those rows the switch is off, so a solve that ran on the handle's
    vehicle shows."""
    B, like, KEYS9 = SC.B, SC.like, SC.KEYS9
    tr = pkg.workloads.synthetic_track("barc")
    L = float(tr["L"])
    mk = lambda: pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)   # noqa: E731
    s_lin, s_sol, s_f32 = mk(), mk(), mk()
    trk = s_lin.device_track(tr)
    real, stale = SC._cold_inputs(pkg, s_lin, trk, L, 11), SC._cold_inputs(pkg, s_lin, trk, L, 12)
    veh = MC.fleet(pkg.presets.barc_vehicle(), B)
    cases = []
    s_lin.set_car_vehicles(veh)
    keys = MC.KEYS
    lb = like({k: stale[k] for k in keys})
    N = s_lin.N
    lo = {"A": SC._empty((6, 6, N - 1, B)), "Bm": SC._empty((6, 2, N - 1, B)), "g": SC._empty((6, N - 1, B))}
    cases.append(Case("linearize_cars", lambda: s_lin.linearize_cars(lb, out=(lo["A"], lo["Bm"], lo["g"])), lb,
                      {k: real[k] for k in keys}, {k: stale[k] for k in keys}, outs=lo, keep=(s_lin, trk)))
    s_sol.set_car_vehicles(veh)
    sb, so = like(stale), SC._solve_outs(s_sol)

    def on_then_solve():
        s_sol.set_cars_controller_model(True)
        s_sol.solve(dict({k: sb[k] for k in KEYS9}, L=L), so)

    cases.append(Case("cars controller model on, then solve", on_then_solve, sb, real, stale, outs=so,
                      reset=lambda: s_sol.set_cars_controller_model(False), keep=s_sol))
    # the single-precision entry: float arrays in, float arrays out (the buffers are the fp64 draws, rounded once)
    s_f32.set_car_vehicles(veh)
    f32 = lambda d: {k: v.float() for k, v in d.items()}   # noqa: E731
    fb, fo = f32(stale), SC._solve_outs(s_f32, f32=True)

    def on_then_solve_f32():
        s_f32.set_cars_controller_model(True)
        s_f32.solve_f32(fb, fo)

    cases.append(Case("cars controller model on, then solve_f32", on_then_solve_f32, fb, f32(real), f32(stale), outs=fo,
                      reset=lambda: s_f32.set_cars_controller_model(False), keep=s_f32))
    assert {c.row for c in cases} == set(ROWS)
    return {c.row: c for c in cases}
