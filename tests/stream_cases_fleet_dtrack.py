"""Which stream the entry point of include/lmpc_hip_fleet_dtrack.h works on: stream_cases.py's classification and row for the fused
fleet LMPC period on the double-track table (tests/test_stream_table_fleet_dtrack.py holds the table to that header without a GPU,
tests/test_gpu_streams_fleet_dtrack.py runs the row on one).  Classes, reference(), gated() and the gate are stream_cases.py's, Case
is stream_cases_vanilla_fleet.py's with this module's rows."""
from __future__ import annotations

import stream_cases as SC
import stream_cases_vanilla_fleet as SF

# name: (class, sync, io), as stream_cases.TABLE
TABLE = {
    "lmpc_fleet_loop_advance_dtrack_batch": (SC.ASYNC, False, True),
}

# row id: (group, the entry points the row's call makes on the gated stream)
ROWS = {
    "fleet_loop_advance_dtrack": ("fleet_dtrack", ("lmpc_fleet_loop_advance_dtrack_batch",)),
}


def entry(name: str):
    return TABLE[name] if name in TABLE else SC.TABLE[name]


def row_class(row: str):
    """(class, sync) of a row, by stream_cases.row_class's rule."""
    fns = ROWS[row][1]
    blocking = any(entry(f)[0] == SC.BLOCKING for f in fns)
    return (SC.BLOCKING if blocking else SC.ASYNC), any(entry(f)[1] for f in fns)


class Case(SF.Case):
    """stream_cases_vanilla_fleet.Case for a row of ROWS above (that class looks its row up in its own module's table)."""

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
    """One row: stream_cases.build_fleet's fused period (the scene, the recorders' pre-feed and the buffers of
    tests/test_gpu_fleet_loop.py) through the double-track entry point, on a three-kind table, with gamma_y as the pure output.
    Inputs on the stream: both solutions, x, u_prev, the references, the loop's state and the accumulators; state: the recorders'
    counters and the rings.  The scene is test_gpu_fleet_loop's cache: the module that builds the row closes it."""
    import numpy as np
    import torch

    import test_gpu_fleet_loop as FL
    import vanilla_fleet_cases as FC

    B, like, dev = SC.B, SC.like, SC.dev
    assert B == FL.B
    sc = FL.scene(pkg, 20)
    learner, trk, L = sc["learner"], sc["trk"], sc["L"]
    learner.set_dtrack_vehicles(FC.dtrack_vehicles(pkg, B))
    roll = lambda d: {k: torch.roll(v, 1, dims=-1).contiguous() for k, v in d.items()}   # noqa: E731  (the neighbour's data: valid, different)
    FL.prefeed(learner, sc["s0"], L)
    rng = np.random.default_rng(11)
    feed = []
    for j in range(max(len(c[1]) for c in FL.CASES)):
        act = np.array([j < len(FL.CASES[c][1]) for c in FL.CASE], dtype=np.int32)
        s_j = np.array([(sc["s0"][b] if FL.CASES[c][1][j] == "s0" else FL.CASES[c][1][j] * L) if act[b] else 0.0 for b, c in enumerate(FL.CASE)])
        feed.append((dev(np.concatenate([s_j[None, :], rng.normal(size=(5, B))])), dev(rng.normal(size=(2, B))), dev(rng.normal(size=B)),
                     0.025 * j, SC._i32(act)))

    def restore():
        learner.fleet_ss_reset()
        for x, u, k, t, act in feed:
            learner.fleet_ss_record(x, u, k, t, L, active=act)

    def ring():
        out = dict(learner.fleet_ss_stats(B))
        FL.close_open_laps(learner, L)   # what went into open laps becomes visible
        learner.use_current_stream()
        per_car = [learner.fleet_ss_get_laps(b) for b in range(B)]
        out["n_pts"] = np.array([lap[0].shape[0] for car in per_car for lap in car] + [-1], dtype=np.int64)
        out["n_laps"] = np.array([len(car) for car in per_car], dtype=np.int64)
        for i, name in enumerate("xukt"):
            out[name] = np.concatenate([np.asarray(lap[i], dtype=np.float64).reshape(-1) for car in per_car for lap in car] + [np.zeros(1)])
        return out

    st = FL.fresh_state(learner)
    full = {("trk " + k): sc["out_t"][k].clone() for k in ("X_optm", "U_optm", "status")}
    full.update({("lrn " + k): sc["out_l"][k].clone() for k in ("X_optm", "U_optm", "status")})
    full.update(x=sc["x"].clone(), u_prev=sc["u_prev"].clone(), **{k: sc["inp"][k].clone() for k in FL.KEYS}, **{k: v.clone() for k, v in st.items()})
    full.update(distance=SC._empty((B,)), worst_excess=SC._empty((B,)), n_fail=SC._empty((B,), torch.int64))
    ab = like(roll(full))
    outs = {"gamma_y": SC._empty((B,))}

    def advance():
        sol = lambda p: {k: ab[p + " " + k] for k in ("X_optm", "U_optm", "status")}   # noqa: E731
        learner.fleet_loop_advance(trk, ab, sol("trk"), sol("lrn"), ab["x"], ab["u_prev"], ab, dt=SC.DT, dt_sim=SC.DT / 2, n_sub=2, t=FL.T_CALL,
                                   speed_scale=FL.SPEED, speed_limit=(6.0, 3.0), restart_failed=True, warm_laps=FL.WARM, learn_laps=FL.LEARN,
                                   switch_phase=True, distance=ab["distance"], worst_excess=ab["worst_excess"], n_fail=ab["n_fail"],
                                   dtrack=True, gamma_y=outs["gamma_y"])

    cases = [Case("fleet_loop_advance_dtrack", advance, ab, full, roll(full), outs,
                  inout=tuple(k for k in full if k[:4] not in ("trk ", "lrn ")), state=ring, reset=restore, keep=())]
    assert {c.row for c in cases} == set(ROWS)
    return {c.row: c for c in cases}
