"""Which stream the entry point of include/lmpc_hip_estimated.h works on: stream_cases.py's classification and row for the fused
estimated period -- lmpc_loop_advance_estimated_batch is asynchronous (tests/test_stream_table_estimated.py holds the table to that
header without a GPU, tests/test_gpu_streams_estimated.py runs the row on one).  Classes, reference(), gated() and the gate are
stream_cases.py's, Case is that module's with this module's row."""
from __future__ import annotations

import numpy as np

import stream_cases as SC

# name: (class, sync, io), as stream_cases.TABLE
TABLE = {
    "lmpc_loop_advance_estimated_batch": (SC.ASYNC, False, True),
}

# row id: (group, the entry points the row's call makes on the gated stream)
ROWS = {
    "loop_advance_estimated": ("estimated", ("lmpc_loop_advance_estimated_batch",)),
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


IN = ("X_optm", "U_optm", "status", "noise_vel", "noise_pose", "R_vel", "R_pose")
INOUT = ("x", "u_prev", "x_ic") + SC.REF7 + ("ekf_flags", "track_status", "distance", "worst_excess", "n_fail", "sq_err")
OUT = ("x_est", "z_vel", "z_pose")


def build(pkg):
    """The one row: a period behind a real solve of a cold start with some cars declared failed, every optional array given.  The
    filter's store and clock are the handle's: before every run the filter is made anew at the same start, and the store is part of
    what the runs are compared on."""
    import torch

    import ekf_cases as EC
    import track_cases as TC

    B, DT, like = SC.B, SC.DT, SC.like
    s = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    tr = pkg.racing_trajectory.RacingTrajectory(TC.BARC)
    spline = s.spline_track(tr)
    trk = s.device_track(tr.to_track_table(1024))
    L = float(trk["L"])
    cfg = EC.config()
    dt_ns = int(round(DT * 1e9))

    def draw(seed, fail_every):
        rng = np.random.default_rng(seed)
        x = np.stack([rng.uniform(0, L, B), rng.uniform(-0.05, 0.05, B), rng.normal(0, 0.02, B), rng.uniform(1.5, 2.5, B), rng.normal(0, 0.02, B),
                      rng.normal(0, 0.1, B)])
        d = {"x": SC.dev(x)}
        pose = s.frenet_to_global(spline, d["x"])
        d["est0"] = torch.cat([pose, d["x"][3:6]]) + SC.dev(0.1 * rng.normal(0, 1, (6, B)) * EC.SD0[:, None])
        frenet, _ = s.global_to_frenet(spline, d["est0"][0:3].contiguous())
        d["x_ic"] = torch.cat([frenet, d["est0"][3:6]]).contiguous()
        d["u_prev"] = SC.dev(rng.normal(0, 1e-3, (2, B)))
        inp = s.prepare(trk, d["x_ic"], DT, speed_scale=0.9)
        inp["u_ic"] = d["u_prev"]
        sol = s.solve(dict(inp, L=L), SC._solve_outs(s))
        d["X_optm"], d["U_optm"] = torch.nan_to_num(sol["X_optm"]).clone(), torch.nan_to_num(sol["U_optm"]).clone()
        d["status"] = sol["status"].clone()
        d["status"][::fail_every] = 1
        for k in SC.REF7:
            d[k] = inp[k].clone()
        d["noise_vel"] = SC.dev(rng.normal(0, 1, (2, B)) * EC.SIG_VEL[:, None])
        noise = rng.normal(0, 1, (3, B)) * EC.SIG_POSE[:, None]
        noise[0, rng.random(B) < 0.1] = np.nan
        d["noise_pose"] = SC.dev(noise)
        d["R_vel"] = SC.dev(np.moveaxis(EC.spd(rng, B, 2), 0, -1))
        d["R_pose"] = SC.dev(np.moveaxis(EC.spd(rng, B, 3, scale=0.02), 0, -1))
        d["ekf_flags"], d["track_status"] = SC.dev(rng.integers(0, 2, B) * 2, torch.int32), SC.dev(np.zeros(B), torch.int32)
        d["distance"], d["worst_excess"] = SC.dev(rng.uniform(0, 3, B)), SC.dev(rng.uniform(-0.2, 0.1, B))
        d["n_fail"], d["sq_err"] = SC.dev(rng.integers(0, 4, B), torch.int64), SC.dev(rng.uniform(0, 1, (6, B)))
        return d

    real, stale = draw(41, 7), draw(42, 5)
    pick = lambda d, keys: {k: d[k] for k in keys}   # noqa: E731
    P0 = SC.dev(np.moveaxis(np.tile(np.diag(EC.SD0 ** 2), (B, 1, 1)), 0, -1))
    # the filter's start is the REAL draw's in every run: the store is state of the handle, not one of the row's buffers
    est0 = real["est0"].clone()
    ids = {}

    def make():
        s.ekf_create(B, cfg["x0"], cfg["P0"], cfg["Q"], cfg["x_min"], cfg["x_max"])
        ids["vel"], ids["pose"] = s.ekf_register_observation(EC.ROWS_VEL), s.ekf_register_observation(EC.ROWS_POSE)
        s.ekf_set_state(est0, P0)
        s.ekf_initialize(0)

    def get():
        g = s.ekf_get()
        return {k: g[k] for k in ("x", "P", "K")}

    keys = IN + INOUT
    bufs = like(pick(stale, keys))
    outs = {"x_est": SC._empty((6, B)), "z_vel": SC._empty((2, B)), "z_pose": SC._empty((3, B))}

    def advance():
        s.loop_advance_estimated(trk, spline, bufs, bufs, bufs["x"], bufs["u_prev"], bufs["x_ic"], DT, DT / 2, 2, ids["vel"], ids["pose"], dt_ns // 2,
                                 dt_ns, bufs["noise_vel"], bufs["R_vel"], bufs["noise_pose"], bufs["R_pose"], speed_scale=0.9, restart_failed=True,
                                 ekf_flags=bufs["ekf_flags"], track_status=bufs["track_status"], distance=bufs["distance"],
                                 worst_excess=bufs["worst_excess"], n_fail=bufs["n_fail"], sq_err=bufs["sq_err"], **outs)

    cases = [Case("loop_advance_estimated", advance, bufs, pick(real, keys), pick(stale, keys), outs=outs, inout=INOUT, state=get, reset=make,
                  keep=(spline, s, trk))]
    assert {c.row for c in cases} == set(ROWS)
    return {c.row: c for c in cases}
