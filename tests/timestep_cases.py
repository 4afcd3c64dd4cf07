"""The problem sets behind tests/golden/dense_dt_*.npz: the problems of tests/dense_cases.py -- same seeds, same generators, the
first problems of the 4096-batch bench.py draws -- with a time step T_ref [N-1][B] that differs from stage to stage and from problem
to problem.  Every other input set of the suite has T_ref == 0.025 everywhere, so a kernel that read t_{i+1} for t_i, [b][i] for
[i][b], a stage clamped one too early or a neighbour's column would pass it.

  * T_ref[i][b] = 0.025 exp(U(ln 0.5, ln 2)), drawn independently per stage and problem from default_rng(the case's constant);
  * problem 0 of every case: T_ref[i] = 0.0125 (1 + 3 i / (N - 2)) -- strictly increasing from 0.0125 to 0.05, so that a shift by
    any number of stages changes every entry;
  * X_ref, U_ref and the track samples stay as the cold start made them at 0.025 (the QP linearises about whatever it is given; the
    reference need not be a rollout at the new steps), except that U_ref gets the small noise test_linearize_matches_complex_step
    adds, so that B and g are not taken at u = 1e-9.

A fixture stores the dense, polished, KKT-certified optimum of every problem, the optimum of the SAME problem with T_ref rolled by
one stage, and their distance: the measure of how far a one-stage index slip moves the answer (tests/golden/make_timestep_fixtures.py
asserts >= 1e3 TOL_XU on every problem).  A problem the dense solver cannot certify is replaced by the next one of the draw: `build`
returns a pool of count + count // 10 problems, the fixture's `draw_index` names the `count` that are used, `select` takes them."""
from __future__ import annotations

import numpy as np

import dense_cases as DC
from oracle import cbind, params as P, qp as Q, scenario as S
from tolerances import TOL_DU, TOL_XU

DT = 0.025
GOLD = DC.__file__.rsplit("/", 1)[0] + "/golden"
SENSITIVITY_MIN = 1e3 * TOL_XU        # the rolled-T_ref optimum is at least this far (scaled) from the true one, every problem
ACTIVE_RATE_SHARE_MIN = 0.25          # share of a case's problems with a rate row (dU at its box) active at some stage
REPLACED_SHARE_MAX = 0.10

# name: (family, N, count, rng constant, what it reaches)
CASES = {
    "dt_trk_n3": ("trk", 3, 32, 9103, "shortest horizon, NS = 2"),
    "dt_trk_n12": ("trk", 12, 32, 9112, "below the N = 23 / 24 row-layout boundary"),
    "dt_trk_n20": ("trk", 20, 32, 9120, "the headline instance"),
    "dt_trk_n24": ("trk", 24, 32, 9124, "first horizon past the row-layout boundary"),
    "dt_iac_n40": ("iac", 40, 32, 9140, "IAC scale; the shape fp32 and mixed are quoted on"),
    "dt_trk_n41": ("trk", 41, 16, 9141, "first lean-record horizon (LN_DT); two-wave kernel by the library's own choice"),
    "dt_trk_n65": ("trk", 65, 12, 9165, "NS = 64: every thread of a wave owns a stage, none is left to the loader's tail loop"),
    "dt_trk_n81": ("trk", 81, 8, 9181, "longest horizon; with one wave forced, NS = 80 > 64: the loader's tail loop"),
    "dt_iac_n66": ("iac", 66, 8, 9166, "the shortest horizon with a stage in the tail loop (NS = 65), at the scale the float kernels serve"),
    "dt_lrn_n20_s160": ("spc", 20, 32, 9220, "terminal block behind non-uniform stages"),
    "dt_lrn_n40_s160": ("spc", 40, 16, 9240, "terminal block, longest horizon on full records (ST_DT)"),
    "dt_lrn_n41_s160": ("spc", 41, 8, 9241, "terminal block on lean records: the one-wave lean kernel as the library itself picks it"),
}
BATCH_KEYS = DC.INPUT_KEYS


def pool_size(name: str) -> int:
    count = CASES[name][2]
    return count + max(1, count // 10)


def oracle_model(name: str):
    family, N = CASES[name][0], CASES[name][1]
    if family == "trk":
        return P.barc_tracking_mpc(N), P.barc_vehicle()
    if family == "iac":
        return P.iac_tracking_mpc(N), P.iac_vehicle()
    return P.barc_lmpc(N, 5), P.barc_vehicle()


def presets(pkg, name: str):
    family, N = CASES[name][0], CASES[name][1]
    if family == "trk":
        return pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle()
    if family == "iac":
        return pkg.presets.iac_tracking_mpc(N), pkg.presets.iac_vehicle()
    return pkg.presets.barc_lmpc(N, 5), pkg.presets.barc_vehicle()


def draw_t_ref(N: int, B: int, constant: int) -> np.ndarray:
    rng = np.random.default_rng(constant)
    T = DT * np.exp(rng.uniform(np.log(0.5), np.log(2.0), (N - 1, B)))
    T[:, 0] = 0.5 * DT * (1.0 + 3.0 * np.arange(N - 1) / max(N - 2, 1))
    return T


def build(pkg, name: str):
    """-> cfg, veh, inp (batch axis last, pool_size(name) problems in the order of the draw), ss_x, ss_j (None for tracking)"""
    family, N, count, constant, _ = CASES[name]
    n = pool_size(name)
    wl = pkg.workloads
    cfg, veh = oracle_model(name)
    kind = "putnam" if family == "iac" else "barc"
    tr = wl.synthetic_track(kind)
    if family == "iac":
        x, u = wl.sample_initial_states(kind, DC.BATCH, tr["L"], [-10.0, -0.314159], [5.0, 0.314159], seed=1)
    else:
        x, u = wl.sample_initial_states(kind, DC.BATCH, tr["L"], [-0.01, -0.314159], [0.01, 0.314159], seed=0)
    inp = S.cold_start_inputs(cfg, veh, tr, x[:n], u[:n], DT)
    ss_x = ss_j = None
    if family == "spc":
        q = DC.ss_query_point(inp, tr["L"])
        ss_x, ss_j, _ = cbind.ss_query_batch(DC.spec_laps(), tr["L"], cfg.num_ss_pts, cfg.num_ss_pts_per_lap, q)
    inp["T_ref"] = draw_t_ref(N, n, constant)
    rng = np.random.default_rng(constant + 1)
    inp["U_ref"] = inp["U_ref"] + rng.normal(0, 1.0, inp["U_ref"].shape) * np.array([0.004, 0.1])[:, None, None]
    return cfg, veh, inp, ss_x, ss_j


def select(inp: dict, ss_x, ss_j, idx):
    """The problems `idx` of a pool, batch axis last and contiguous."""
    idx = np.asarray(idx)
    out = {k: (np.ascontiguousarray(np.asarray(v)[..., idx]) if k in BATCH_KEYS else v) for k, v in inp.items()}
    return out, (None if ss_x is None else np.ascontiguousarray(ss_x[..., idx])), (None if ss_j is None else np.ascontiguousarray(ss_j[..., idx]))


def rolled(inp: dict) -> dict:
    """The same problems with every T_ref column rolled by one stage (t_i := t_{i-1}, t_0 := t_{N-2}): what an index slip reads."""
    return dict(inp, T_ref=np.ascontiguousarray(np.roll(inp["T_ref"], 1, axis=0)))


def load(name: str) -> dict:
    with np.load(f"{GOLD}/dense_{name}.npz") as z:
        return {k: z[k] for k in z.files}


def fixture_problems(pkg, name: str):
    """-> fx, cfg, veh, inp, ss_x, ss_j: the fixture and the inputs of ITS problems, rebuilt from the seeds and held to its digest."""
    fx = load(name)
    cfg, veh, pool, px, pj = build(pkg, name)
    inp, ss_x, ss_j = select(pool, px, pj, fx["draw_index"])
    np.testing.assert_allclose(DC.digest(inp, ss_x, ss_j), fx["digest"], rtol=1e-11, atol=0)
    assert np.array_equal(inp["T_ref"], fx["T_ref"])
    return fx, cfg, veh, inp, ss_x, ss_j


def rate_row_active(qp, lam: np.ndarray, tol: float = 1e-9) -> bool:
    """From the dense multipliers: a row that bounds a dU alone carries a multiplier."""
    N = qp.N
    lo, hi = Q.NX * N + Q.NU * (N - 1), Q.NX * N + 2 * Q.NU * (N - 1)
    nz = qp.C != 0.0
    rate = nz[:, lo:hi].any(axis=1) & (nz.sum(axis=1) == 1)
    return bool((lam[rate] > tol).any())


# ---- the comparison every entry point is held to ---------------------------------------------------------------------------------------
def errors(out: dict, fx: dict):
    """Per problem: max scaled |X - X*| and |U - U*|, max scaled |dU - dU*|, and for the learning problem max |lambda - lambda*|
    folded into the first (the weights are O(1) and unscaled)."""
    SX, SU = P.SCALE_X[:, None, None], P.SCALE_U[:, None, None]
    ex = np.abs((np.asarray(out["X_optm"], dtype=np.float64) - fx["X_optm"]) / SX).max(axis=(0, 1))
    eu = np.abs((np.asarray(out["U_optm"], dtype=np.float64) - fx["U_optm"]) / SU).max(axis=(0, 1))
    ed = np.abs((np.asarray(out["dU_optm"], dtype=np.float64) - fx["dU_optm"]) / SU).max(axis=(0, 1))
    exu = np.maximum(ex, eu)
    if "convex_combi_optm" in fx and out.get("convex_combi_optm") is not None:
        exu = np.maximum(exu, np.abs(np.asarray(out["convex_combi_optm"], dtype=np.float64) - fx["convex_combi_optm"]).max(axis=0))
    return exu, ed


def accepted(out: dict, fx: dict, tol_xu: float = TOL_XU, tol_du: float = TOL_DU) -> np.ndarray:
    """bool [B]: the problems whose answer passes -- status 0 and within tol_xu / tol_du (scaled) of the fixture's optimum.  NaN fails."""
    exu, ed = errors(out, fx)
    return (np.asarray(out["status"]) == 0) & (exu < tol_xu) & (ed < tol_du)


def assert_matches(out: dict, fx: dict, who: str, tol_xu: float = TOL_XU, tol_du: float = TOL_DU, allow=()):
    """Every problem accepted, except those named in `allow` (reduced precision only: the named problem's error is printed)."""
    exu, ed = errors(out, fx)
    ok = accepted(out, fx, tol_xu, tol_du)
    print("%s: %d problems, X/U(/lambda) max %.1e, dU max %.1e, statuses %s" % (who, ok.size, np.nanmax(exu), np.nanmax(ed), np.bincount(np.asarray(out["status"])).tolist()))
    for b in allow:
        print("   named exception: problem %d, X/U %.2e dU %.2e status %d" % (b, exu[b], ed[b], int(np.asarray(out["status"])[b])))
        ok[b] = True
    bad = np.nonzero(~ok)[0]
    assert bad.size == 0, (who, bad.tolist(), exu[bad].tolist(), ed[bad].tolist(), np.asarray(out["status"])[bad].tolist())
    return float(np.nanmax(exu)), float(np.nanmax(ed))


def rate_identity_error(out: dict, inp: dict) -> float:
    """max scaled |dU_i t_i - (u_i - u_{i-1})|, u_{-1} = u_ic, on an entry point's OWN outputs (racing_mpc.cpp:190-196)."""
    U, dU = np.asarray(out["U_optm"]), np.asarray(out["dU_optm"])
    prev = np.concatenate([inp["u_ic"][:, None, :], U[:, :-1, :]], axis=1)
    return float(np.abs((dU * inp["T_ref"][None] - (U - prev)) / P.SCALE_U[:, None, None]).max())
