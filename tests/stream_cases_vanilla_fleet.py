"""Which stream the entry point of include/lmpc_hip_vanilla_fleet.h works on: stream_cases.py's classification and row for the vanilla
rollout of a fleet (tests/test_stream_table_vanilla_fleet.py holds the table to that header without a GPU,
tests/test_gpu_streams_vanilla_fleet.py runs the row on one).  Classes, reference(), gated() and the gate are stream_cases.py's, Case
is stream_cases_dtrack.py's with this module's rows."""
from __future__ import annotations

import stream_cases as SC

# name: (class, sync, io), as stream_cases.TABLE
TABLE = {
    "lmpc_vanilla_rollout_fleet_batch": (SC.ASYNC, False, True),
}

# row id: (group, the entry points the row's call makes on the gated stream)
ROWS = {
    "vanilla_rollout_fleet": ("vanilla_fleet", ("lmpc_vanilla_rollout_fleet_batch",)),
}


def entry(name: str):
    return TABLE[name] if name in TABLE else SC.TABLE[name]


def row_class(row: str):
    """(class, sync) of a row, by stream_cases.row_class's rule."""
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


PERIODS, PERIOD0 = 3, 40


def build(pkg):
    """One row: three periods of the BARC scenario on the mixed car table, recording by the "arrived" convention.  Inputs on the
    stream: x, u_prev and the accumulators; outputs: the logs and flags; state: the PID state and the recorders' counters.  Half the
    cars of a draw start within a period's travel of the start line, so that their recorders count a crossing."""
    import numpy as np
    import torch

    import vanilla_cases as VC
    import vanilla_fleet_cases as FC

    B, like, dev = SC.B, SC.like, SC.dev
    sc = VC.scenario("barc", B=B)
    L = float(sc["trk"]["L"])
    s = pkg.Solver(pkg.presets.barc_lmpc(20, FC.RING), pkg.presets.barc_vehicle(), device=0)
    spline = s.spline_track(sc["trk"]["spline"])
    table = s.device_track(sc["trk"]["table"])
    s.vanilla_create(sc["cfg"], B)
    s.fleet_ss_create(B, 64)
    s.set_car_vehicles(FC.car_vehicle_dicts(pkg, sc, B))
    to_dev = lambda a: dev(np.moveaxis(np.asarray(a, dtype=np.float64), 0, -1))   # noqa: E731
    x_fix, integ_fix = to_dev(sc["x0"]), dev(np.random.default_rng(60).uniform(-1, 1, B))

    def reset():   # a PID state with every entry set, and empty recorders
        s.vanilla_reset(B, integ_fix)
        s.vanilla_solve(spline, x_fix, None, speed_scale=sc["speed_scale"])
        s.vanilla_solve(spline, x_fix, None, speed_scale=1.0)
        s.fleet_ss_reset()

    def state():
        got = {"pid " + k: v for k, v in s.vanilla_get(B).items()}
        got.update({"ring " + k: v for k, v in s.fleet_ss_stats(B).items()})
        return got

    def draw(seed):
        rng = np.random.default_rng(seed)
        x = sc["x0"].copy()
        x[:, 0] = np.mod(x[:, 0] + rng.uniform(0, 1, B), L)
        x[:, 3] = rng.uniform(1.0, 2.0, B)
        near = rng.permutation(B)[: B // 2]
        x[near, 0] = L - rng.uniform(0.2, 0.8, near.size) * x[near, 3] * sc["dt"] * PERIODS
        return {"x": to_dev(x), "u_prev": to_dev(rng.uniform(-0.2, 0.2, (B, 2))), "distance": dev(rng.uniform(0, 2, B)),
                "worst_excess": dev(rng.uniform(-0.3, 0.0, B))}

    real, stale = draw(61), draw(62)
    bufs = like(stale)
    outs = {"X_log": SC._empty((6, PERIODS, B)), "U_log": SC._empty((2, PERIODS, B)), "k_log": SC._empty((PERIODS, B)),
            "flags": SC._empty((B,), torch.int32)}

    def call():
        s.vanilla_rollout_fleet(spline, table, bufs["x"], PERIODS, sc["dt_sim"], sc["n_sub"], plant="cars", record="arrived", period0=PERIOD0,
                                dt=sc["dt"], u_prev=bufs["u_prev"], speed_scale=sc["speed_scale"], distance=bufs["distance"],
                                worst_excess=bufs["worst_excess"], out=outs)

    cases = [Case("vanilla_rollout_fleet", call, bufs, real, stale, outs, inout=tuple(bufs), state=state, reset=reset, keep=(s, spline, table))]
    assert {c.row for c in cases} == set(ROWS)
    return {c.row: c for c in cases}
