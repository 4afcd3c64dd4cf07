"""Which stream the entry points of include/lmpc_hip_dtrack.h work on: stream_cases.py's classification and rows for the double-track
table (one four-wheel plant vehicle per car) and the plant step that reads it (tests/test_stream_table_dtrack.py holds the table to
that header without a GPU, tests/test_gpu_streams_dtrack.py runs the rows on one).  Classes, reference(), gated() and the gate are
stream_cases.py's, Case is stream_cases_cars.py's with this module's rows."""
from __future__ import annotations

import stream_cases as SC

# name: (class, sync, io), as stream_cases.TABLE
TABLE = {
    "lmpc_dtrack_set_vehicles": (SC.BLOCKING, True, True),
    "lmpc_dtrack_get_vehicles": (SC.BLOCKING, True, True),
    "lmpc_plant_step_dtrack_batch": (SC.ASYNC, False, True),
}

# row id: (group, the entry points the row's call makes on the gated stream)
ROWS = {
    "plant_step_dtrack": ("dtrack", ("lmpc_plant_step_dtrack_batch",)),
    "set_dtrack_vehicles, then plant_step_dtrack": ("dtrack", ("lmpc_dtrack_set_vehicles", "lmpc_plant_step_dtrack_batch")),
    "plant_step_dtrack, then get_dtrack_vehicles": ("dtrack", ("lmpc_plant_step_dtrack_batch", "lmpc_dtrack_get_vehicles")),
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


def fleet(pkg, n, other=False):
    """n double-track vehicles by b % 3: the BARC preset, mu = 0.7, kroll_f = 0.35 with Ef = Er = 0.6; `other`: shifted by one car."""
    base = pkg.presets.barc_double_track()
    kinds = (base, dict(base, mu=0.7), dict(base, kroll_f=0.35, Ef=0.6, Er=0.6))
    return [kinds[(b + (1 if other else 0)) % 3] for b in range(n)]


def build(pkg):
    """stream_cases_cars.build's three rows on the double-track table: the same states, inputs and sub-steps; the plant step also
    writes gamma_y, an output of the row."""
    import numpy as np
    import torch

    B, like, DT = SC.B, SC.like, SC.DT
    tr = pkg.workloads.synthetic_track("barc")
    L = float(tr["L"])
    mk = lambda: pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)   # noqa: E731
    s, s_set, s_get = mk(), mk(), mk()
    trk = s.device_track(tr)

    def draw(seed):
        x, u = pkg.workloads.sample_initial_states("barc", B, L, [-0.01, -0.3], [0.01, 0.3], seed=seed)
        return {"x": SC.dev(x.T.copy()), "u": SC.dev(u.T.copy())}

    real, stale = draw(7), draw(8)
    gam = lambda: {"gamma_y": torch.zeros(B, dtype=torch.float64, device="cuda")}   # noqa: E731
    cases = []
    s.set_dtrack_vehicles(fleet(pkg, B))
    xb, xo = like(stale), gam()
    cases.append(Case("plant_step_dtrack", lambda: s.plant_step_dtrack(trk, xb["x"], xb["u"], DT / 2, 2, xo["gamma_y"]), xb, real, stale,
                      outs=xo, inout=("x",), keep=(s, trk)))
    # the setter under the stream, the plant step that reads the new table behind it; before every run the handle holds the other table
    sb, so = like(stale), gam()

    def set_then_step():
        s_set.set_dtrack_vehicles(fleet(pkg, B))
        s_set.plant_step_dtrack(trk, sb["x"], sb["u"], DT / 2, 2, so["gamma_y"])

    cases.append(Case("set_dtrack_vehicles, then plant_step_dtrack", set_then_step, sb, real, stale, outs=so, inout=("x",),
                      reset=lambda: s_set.set_dtrack_vehicles(fleet(pkg, B, other=True)), keep=s_set))
    # the getter behind a plant step on the same stream: it waits for the stream, and what it returns is the table (the row's state)
    s_get.set_dtrack_vehicles(fleet(pkg, B))
    gb, go, got = like(stale), gam(), {}

    def step_then_get():
        s_get.plant_step_dtrack(trk, gb["x"], gb["u"], DT / 2, 2, go["gamma_y"])
        got["veh"] = s_get.get_dtrack_vehicles()

    def table():
        return {"mu kroll_f Ef integrator": np.array([[v["mu"], v["kroll_f"], v["Ef"], v["integrator"]] for v in got["veh"]])}

    cases.append(Case("plant_step_dtrack, then get_dtrack_vehicles", step_then_get, gb, real, stale, outs=go, inout=("x",), state=table,
                      keep=s_get))
    assert {c.row for c in cases} == set(ROWS)
    return {c.row: c for c in cases}
