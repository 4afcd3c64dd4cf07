"""Which stream the entry points of include/lmpc_hip_rows.h work on: stream_cases.py's classification and rows for the regression
with one feature list per regressed row (tests/test_stream_table_rows.py holds the table to that header without a GPU,
tests/test_gpu_streams_rows.py runs the rows on one).  Classes, Case, reference(), gated() and the gate are stream_cases.py's; a row
here may also name an entry point of stream_cases.TABLE (the regression and the solve that apply the per-row spec)."""
from __future__ import annotations

import ctypes as C

import stream_cases as SC

# name: (class, sync, io), as stream_cases.TABLE
TABLE = {
    "lmpc_set_regression_laps_rows": (SC.BLOCKING, True, True),
    "lmpc_fleet_ss_set_regression_rows": (SC.BLOCKING, True, True),   # (sync: when the table's size changes -- the row's case)
}

# row id: (group, the entry points the row's call makes on the gated stream)
ROWS = {
    "regress, per-row lists": ("regression rows", ("lmpc_regress_batch",)),
    "solve with the shared per-row regression": ("regression rows", ("lmpc_solve_batch",)),
    "set_regression_laps, per-row lists": ("regression rows", ("lmpc_set_regression_laps_rows", "lmpc_regress_batch")),
    "fleet_ss_regress, per-row lists": ("regression rows", ("lmpc_fleet_ss_regress_batch",)),
    "solve with the fleet per-row regression": ("regression rows", ("lmpc_solve_batch",)),
    "fleet_ss_set_regression refill, per-row lists": ("regression rows", ("lmpc_fleet_ss_set_regression_rows", "lmpc_fleet_ss_regress_batch")),
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


PER_ROW = {3: ((3, 4, 5), (0,)), 4: ((3, 4, 5), (1,)), 5: ((2, 3, 4, 5), (1,))}


def build(pkg):
    """The rows of stream_cases.build_regression that involve a regression spec, with PER_ROW in its place: same inputs, same laps."""
    B, like = SC.B, SC.like
    tr = pkg.workloads.synthetic_track("barc")
    L = float(tr["L"])
    mk = lambda: pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)   # noqa: E731
    s, r_reg, r_set, r_fr, r_fr2 = mk(), mk(), mk(), mk(), mk()
    trk = s.device_track(tr)
    real, stale = SC._cold_inputs(pkg, s, trk, L, 7), SC._cold_inputs(pkg, s, trk, L, 8)
    lap, lap2 = SC._lap_near(tr, real, 41), SC._lap_near(tr, stale, 42)
    N = s.N
    lin_keys = ("X_ref", "U_ref", "T_ref", "curvatures")

    def with_model(d):
        out = {"A": SC._empty((6, 6, N - 1, B)), "Bm": SC._empty((6, 2, N - 1, B)), "g": SC._empty((6, N - 1, B))}
        s.use_current_stream()
        s._check(s.lib.lmpc_linearize_batch(s._h, C.c_int32(B), *[C.c_void_p(d[k].data_ptr()) for k in lin_keys],
                                            *[C.c_void_p(out[k].data_ptr()) for k in ("A", "Bm", "g")]), "lmpc_linearize_batch")
        return dict({k: d[k] for k in ("X_ref", "U_ref")}, **out)

    mreal, mstale = with_model(real), with_model(stale)
    abg = ("A", "Bm", "g")
    cases = []

    def regress_case(row, sv, fleet, reset=None):
        bufs = like(mstale)
        fn = sv.fleet_ss_regress if fleet else sv.regress
        return Case(row, lambda: fn(bufs, bufs["A"], bufs["Bm"], bufs["g"]), bufs, mreal, mstale, inout=abg, reset=reset, keep=(sv, s))

    def solve_case(row, sv, reset=None):
        bufs, outs = like(stale), SC._solve_outs(sv)
        return Case(row, lambda: sv.solve(dict(bufs, L=L), outs), bufs, real, stale, outs, reset=reset, keep=sv)

    r_reg.set_regression_laps([lap], rows=PER_ROW, dist_max=1.0)
    cases.append(regress_case("regress, per-row lists", r_reg, False))
    cases.append(solve_case("solve with the shared per-row regression", r_reg))
    # lmpc_set_regression_laps_rows under the stream, the regression that reads the new store behind it
    rb = like(mstale)

    def set_rows_call():
        r_set.use_current_stream()
        r_set.set_regression_laps([lap], rows=PER_ROW, dist_max=1.0)
        r_set.regress(rb, rb["A"], rb["Bm"], rb["g"])

    cases.append(Case("set_regression_laps, per-row lists", set_rows_call, rb, mreal, mstale, inout=abg,
                      reset=lambda: r_set.set_regression_laps([lap2], rows=PER_ROW, dist_max=1.0), keep=r_set))
    # per car: every ring holds the lap; the packed tables are handle-held state, refilled on the device in front of a use
    for sv in (r_fr, r_fr2):
        sv.fleet_ss_create(B, 64)
        sv.fleet_ss_load([lap], L, car=-1)
    r_fr.fleet_ss_set_regression(rows=PER_ROW, dist_max=1.0)
    again = lambda: r_fr.fleet_ss_set_regression(rows=PER_ROW, dist_max=1.0)   # noqa: E731  (every stamp stale: the next use packs every car again)
    cases.append(regress_case("fleet_ss_regress, per-row lists", r_fr, True, reset=again))
    cases.append(solve_case("solve with the fleet per-row regression", r_fr, reset=again))
    rfb = like(mstale)

    def refill_rows_call():   # one list (5, 3) -> per-row lists: the table's size changes, which is when the call waits for the stream
        r_fr2.fleet_ss_set_regression(rows=PER_ROW, dist_max=1.0)
        r_fr2.fleet_ss_regress(rfb, rfb["A"], rfb["Bm"], rfb["g"])

    cases.append(Case("fleet_ss_set_regression refill, per-row lists", refill_rows_call, rfb, mreal, mstale, inout=abg,
                      reset=lambda: r_fr2.fleet_ss_set_regression(dist_max=1.0), keep=r_fr2))
    assert {c.row for c in cases} == set(ROWS)
    return {c.row: c for c in cases}
