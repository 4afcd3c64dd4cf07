"""GPU: the small kernels either side of the solve (csrc/lmpc_prep_kernels.hip) against plain references of their own
(tests/glue_cases.py, pinned without a GPU by tests/test_glue_reference.py) -- the carry-over of simplex weights by the identity of
the safe-set points, the launch order, a whole period between two solves against the oracle's node and simulator, the warm flag
through every solve entry, and an infeasible initial state through the two-wave kernel.  Integer results and the weights are
compared exactly; floating-point arrays at the bounds the project already states (1e-11 relative, 1e-8 scaled, TOL_TWIN)."""
import numpy as np
import pytest
import torch

import glue_cases as G
from oracle import cbind, params as P, scenario as S
from parity import per_problem_err
from tolerances import TOL_TWIN

pytestmark = pytest.mark.gpu
REL = 1e-11          # the bound of test_shift_and_plant_match_node_and_simulator: |a - r| <= REL max(1, max |r|)


def _np(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items() if not k.startswith("_")}


def _close(a, r):
    return float(np.abs(np.asarray(a) - np.asarray(r)).max()) <= REL * max(1.0, float(np.abs(r).max()))


# ---- weights carried by identity (lmpc_shift_lambda_batch) ------------------------------------------------------------------------------
NPTS = (37, 64, 101)          # three laps of awkward lengths: rows 0 .. 36, 37 .. 100, 101 .. 201
TOTAL = sum(NPTS)


def _learner_with_store(pkg, laps, L, B):
    sv = pkg.Solver(pkg.presets.barc_lmpc(20, 3), pkg.presets.barc_vehicle(), device=0)
    sv.set_safe_set(laps, L)
    rng = np.random.default_rng(2)
    q = torch.as_tensor(np.stack([rng.uniform(0, L, B), rng.uniform(-0.1, 0.1, B)]), dtype=torch.float64, device="cuda")
    sv.ss_query_idx(q)                       # the handle has seen a query against this store
    return sv, int(sv.config["num_ss_pts"])


def _synthetic_laps(L=17.0):
    rng = np.random.default_rng(1)
    laps = []
    for n in NPTS:
        x = rng.normal(0, 0.05, (n, 6))
        x[:, 0] = np.arange(n) * L / n
        x[:, 3] += 1.5
        laps.append(x)
    return laps, L


def _e(lap, sample, rep=0):
    return G.encode(NPTS, lap, sample, rep)


# name -> (previous set [(code, weight)], new set [codes]); each occupies one problem, entries at ascending seeded positions
CASES = {
    # the last sample of a lap moves into the next copy (advance 1), is reached as "two on" (advance 0), or leaves (advance 2)
    "last sample rep 0 and 1": ([(_e(0, 36, 0), 0.5), (_e(1, 63, 1), 0.5)], [_e(1, 0, 2), _e(0, 0, 1), _e(0, 2, 1)]),
    "last sample rep 2, itself present": ([(_e(0, 36, 2), 0.6), (_e(1, 63, 2), 0.4)], [_e(0, 0, 2), _e(0, 36, 2), _e(1, 0, 0)]),
    "last sample rep 2, dropped": ([(_e(2, 100, 2), 1.0)], [_e(2, 0, 2), _e(2, 0, 0), _e(2, 99, 2)]),
    # the lap lookup at off[t] and off[t] - 1
    "first row of lap 1, last row of lap 0": ([(_e(1, 0, 0), 0.3), (_e(0, 36, 0), 0.7)],
                                              [_e(1, 2, 0), _e(1, 1, 0), _e(0, 0, 1), _e(0, 36, 0), _e(1, 0, 0), _e(0, 1, 1), _e(1, 0, 1)]),
    "first row of lap 2, last row of lap 1": ([(_e(2, 0, 0), 0.5), (_e(1, 63, 0), 0.5)],
                                              [_e(2, 1, 0), _e(1, 0, 1), _e(2, 2, 0), _e(1, 1, 1), _e(2, 0, 1), _e(1, 63, 0)]),
    "padding": ([(-1, 0.5), (_e(1, 5), 0.25), (-1, 0.25)], [-1, -1, _e(1, 6), -1, _e(1, 5)]),
    "repeated code": ([(_e(1, 5), 1.0)], [_e(1, 8), _e(1, 6), _e(1, 6), _e(1, 5), _e(1, 6), _e(1, 5), _e(1, 7), _e(1, 7)]),
    # 5 -> 6; 6 -> 7 absent, itself; 4 -> 5 absent, 4 absent, two on = 6: (0.1 + 0.2) + 0.3 with advance 1
    "two and three on one cell": ([(_e(1, 5), 0.1), (_e(1, 6), 0.2), (_e(1, 4), 0.3)], [_e(1, 6)]),
    "seven distinct": ([(_e(1, 10 + 3 * i), 0.1 + 0.01 * i) for i in range(7)], [_e(1, 10 + i) for i in range(24)]),
    "eight distinct": ([(_e(2, 10 + 3 * i), 0.1 + 0.01 * i) for i in range(8)], [_e(2, 10 + i) for i in range(27)]),
    # a seventh entry whose first candidate is a cell that holds a weight already (the second entry's: 13 + advance) ...
    "seven, the last on a taken cell": ([(_e(1, 10 + 3 * i), 0.1) for i in range(6)] + [(_e(1, 13), 0.05)], [_e(1, 10 + i) for i in range(24)]),
    # ... and one that is refused on new cells first: advance 0: 12 new, 12 again, 13 taken; 1: 13 new, 12 new, 14 taken; 2: 14 new, 12 taken
    "seven, refused then taken": ([(_e(1, 10 + 3 * i), 0.1) for i in range(6)] + [(_e(1, 12), 0.05)], [_e(1, 10 + i) for i in range(24)]),
    # ten: the ninth and tenth carry the codes of the first and second, so every candidate of theirs is a cell that holds a weight
    # already -- the cap of six would let them add; only "the first eight count" keeps them out
    "ten": ([(_e(0, 3 * i), 0.05 + 0.01 * i) for i in range(8)] + [(_e(0, 0), 0.13), (_e(0, 3), 0.14)], [_e(0, i) for i in range(32)]),
    "threshold": ([(_e(1, 20), 1e-9), (_e(1, 24), 2e-9), (_e(1, 28), 0.5)], [_e(1, 20 + i) for i in range(12)]),
    # rows at and past the store's total name no point.  (A lookup that lets them through reads row 202 as lap 2 sample 101 + adv
    # -> sample adv of the next copy, and row 207 rep 1 as sample 5 + adv of copy 2: those cells are in the new set, so they show.)
    "past the store": ([((TOTAL << 2) | 0, 0.4), (((TOTAL + 5) << 2) | 1, 0.3), (_e(2, 100, 0), 0.3)],
                       [_e(2, 0, 1), _e(2, 1, 1), _e(2, 2, 1), _e(2, 3, 1), (TOTAL << 2) | 0, _e(2, 5, 2), _e(2, 6, 2), _e(2, 7, 2), _e(2, 8, 2),
                        ((TOTAL + 5) << 2) | 1, _e(2, 100, 0), (TOTAL << 2) | 1]),
}


def _lambda_batch(S_pts, B, names=None):
    """idx_prev, lam_prev, idx [S][B]: the named cases on problems 0, 1, ... and -- with names = None -- every case, then seeded
    problems whose codes crowd a few rows around the lap boundaries (collisions, repeats, padding, every route)."""
    rng = np.random.default_rng(7)
    idx_prev = np.full((S_pts, B), -1, dtype=np.int32)
    lam_prev = np.zeros((S_pts, B))
    idx = np.full((S_pts, B), -1, dtype=np.int32)
    where = {}
    names = list(CASES if names is None else names)
    for b, name in enumerate(names):
        prev, new = CASES[name]
        idx_prev[:, b] = [_e(2, 40 + int(r), 1) for r in rng.integers(0, 50, S_pts)]          # weightless fillers, far from every case
        pp = np.sort(rng.choice(S_pts, len(prev), replace=False))
        idx_prev[pp, b] = [c for c, _ in prev]
        lam_prev[pp, b] = [w for _, w in prev]
        idx[np.sort(rng.choice(S_pts, len(new), replace=False)), b] = new
        where[name] = b
    centres = (0, 36, 37, 100, 101, 201, 60, 150)
    for b in range(len(names), B):
        c = centres[b % len(centres)]
        rows = np.clip(c + rng.integers(-12, 13, S_pts), 0, TOTAL - 1)
        idx_prev[:, b] = (rows << 2) | rng.integers(0, 3, S_pts)
        idx_prev[rng.random(S_pts) < 0.05, b] = -1
        k = int(rng.integers(1, 11))
        pp = rng.choice(S_pts, k, replace=False)
        lam_prev[pp, b] = rng.dirichlet(np.ones(k))
        moved = [G.advance_code(NPTS, int(cd), int(a)) for cd, a in zip(idx_prev[:, b], rng.integers(0, 4, S_pts))]
        fresh = (np.clip(c + rng.integers(-12, 13, S_pts), 0, TOTAL - 1) << 2) | rng.integers(0, 3, S_pts)
        idx[:, b] = rng.permutation(np.where(rng.random(S_pts) < 0.5, moved, fresh))
    return idx_prev, lam_prev, idx, where


def _kernel_shift(sv, idx_prev, lam_prev, idx, advance):
    out = torch.full(idx.shape, 7.0, dtype=torch.float64, device="cuda")          # (every entry is to be written)
    sv.shift_lambda(torch.as_tensor(idx_prev, device="cuda"), torch.as_tensor(lam_prev, device="cuda"), torch.as_tensor(idx, device="cuda"), advance, out=out)
    return out.cpu().numpy()


def test_weights_are_carried_by_the_identity_of_the_points(pkg):
    B = 130
    laps, L = _synthetic_laps()
    sv, S_pts = _learner_with_store(pkg, laps, L, B)
    idx_prev, lam_prev, idx, where = _lambda_batch(S_pts, B)
    seen = set()
    for advance in (0, 1, 2):
        routes = []
        want = G.shift_lambda(NPTS, idx_prev, lam_prev, idx, advance, routes)
        seen |= {t for _, t in routes}
        # the cases do what their names say (on the reference; the hand-worked values are in tests/test_glue_reference.py)
        col = lambda name: want[:, where[name]]
        assert (col("seven distinct") > 0).sum() == 6 and (col("eight distinct") > 0).sum() == 6 and (col("ten") > 0).sum() == 6
        for name in ("seven, the last on a taken cell", "seven, refused then taken"):
            assert (col(name) > 0).sum() == 6 and col(name).max() == 0.1 + 0.05
        ten = col("ten")
        assert sorted(ten[ten > 0]) == [0.05 + 0.01 * i for i in range(6)]          # the ninth and tenth added nothing to the first two
        assert col("threshold").sum() == 2e-9 + 0.5 and col("past the store").sum() == 0.3 and col("padding").sum() == 0.25
        assert col("last sample rep 2, dropped").sum() == 0.0 and col("last sample rep 2, itself present").sum() == 0.6
        if advance == 1:
            assert col("last sample rep 0 and 1").sum() == 1.0 and col("two and three on one cell").sum() == (0.1 + 0.2) + 0.3
        got = _kernel_shift(sv, idx_prev, lam_prev, idx, advance)
        bad = np.nonzero((got != want).any(axis=0))[0]
        assert np.array_equal(got, want), (advance, bad, [n for n, b in where.items() if b in bad])
    assert seen == {0, 1, 2, None}
    sv.close()


def test_codes_past_the_store_carry_nothing(pkg):
    """Row = total and row = total + 5: no point, whatever the advance -- not a sample of the last lap.  (Larger rows are left out on
    purpose: before the store's total was handed to the kernel, the lap walk took O(row / n) turns.)"""
    B = 3
    laps, L = _synthetic_laps()
    sv, S_pts = _learner_with_store(pkg, laps, L, B)
    idx_prev, lam_prev, idx, _ = _lambda_batch(S_pts, B, names=["past the store"] * B)
    for advance in (0, 1, 2):
        want = G.shift_lambda(NPTS, idx_prev, lam_prev, idx, advance)
        got = _kernel_shift(sv, idx_prev, lam_prev, idx, advance)
        assert (want.sum(axis=0) == 0.3).all() and np.array_equal(got, want), (advance, got.sum(axis=0))
    sv.close()


def test_weights_carried_on_the_recorded_laps(pkg):
    """Codes of real queries: the reference's recorded laps in the store, 130 queries along lap 3 and the same queries zero, one or
    two samples further on (one on average: a control period), weights on six found points of the first set."""
    import lmpc_scenario as LS

    B, advance = 130, 1
    laps = LS.load_laps()
    npts = [lap.shape[0] for lap in laps]
    sv, S_pts = _learner_with_store(pkg, laps, LS.L_BARC_SS, B)
    at = np.linspace(0, npts[2] - 1, B).astype(int)
    on = (at + np.arange(B) % 3) % npts[2]
    q0 = torch.as_tensor(laps[2][at][:, :2].T.copy(), device="cuda")
    q1 = torch.as_tensor(laps[2][on][:, :2].T.copy(), device="cuda")
    (i0, n0), (i1, _) = sv.ss_query_idx(q0), sv.ss_query_idx(q1)
    idx_prev, idx, n0 = i0.cpu().numpy(), i1.cpu().numpy(), n0.cpu().numpy()
    assert (n0 >= 6).all()
    rng = np.random.default_rng(9)
    lam_prev = np.zeros((S_pts, B))
    for b in range(B):
        pp = rng.choice(int(n0[b]), 6, replace=False)
        lam_prev[pp, b] = rng.dirichlet(np.ones(6))
    routes = []
    want = G.shift_lambda(npts, idx_prev, lam_prev, idx, advance, routes)
    share = [sum(w for w, t in routes if t == r) / B for r in (0, 1, 2)]
    print("recorded laps, %d queries, advance %d: share of the weight carried %.3f (%.3f one sample on, %.3f on the point itself, %.3f two on)"
          % (B, advance, want.sum() / B, *share))
    assert want.sum() > 0 and all(s > 0 for s in share)
    assert np.array_equal(_kernel_shift(sv, idx_prev, lam_prev, idx, advance), want)
    sv.close()


def test_permuted_set_takes_the_permuted_weights_and_solves_alike(pkg):
    """End to end on the kernel's own codes and weights (fixture barc_lmpc_n20_s160, 256 problems, solved cold by reference): with
    the rows of the set permuted per problem, advance = 0 must hand every support weight to the same point at its new position, and
    a warm solve on the permuted set with the carried weights is the warm solve on the set as it was."""
    import dense_cases as DC

    n = 256
    cfg, veh, inp, _, _ = DC.build(pkg, "barc_lmpc_n20_s160")
    inp = {k: (np.ascontiguousarray(v[..., :n]) if hasattr(v, "shape") and np.ndim(v) >= 1 else v) for k, v in inp.items()}
    tr = pkg.workloads.synthetic_track("barc")
    laps = pkg.workloads.synthetic_laps(tr, 5)
    npts = [lap.shape[0] for lap in laps]
    S_pts = int(cfg.num_ss_pts)
    sv = pkg.Solver(pkg.presets.barc_lmpc(20, 5), pkg.presets.barc_vehicle(), device=0)
    sv.set_safe_set(laps, tr["L"])
    idx_t, _ = sv.ss_query_idx(torch.as_tensor(DC.ss_query_point(inp, tr["L"]), device="cuda"))

    def solve(codes, warm=None):
        out = sv.alloc_outputs(n)
        out["convex_combi_optm"] = torch.zeros((S_pts, n), dtype=torch.float64, device="cuda")
        o = _np(sv.solve(inp, out, ss_idx=codes, warm=warm))
        o["accepted"] = sv.warm_accepted(n).cpu().numpy()
        return o

    cold = solve(idx_t)
    ok = cold["status"] == 0
    assert ok.mean() > 0.99 and not cold["accepted"].any()
    idx, lam = idx_t.cpu().numpy(), cold["convex_combi_optm"]
    rng = np.random.default_rng(4)
    perm = np.stack([rng.permutation(S_pts) for _ in range(n)], axis=1)
    idx_perm, lam_perm = np.take_along_axis(idx, perm, 0), np.take_along_axis(lam, perm, 0)
    want = G.shift_lambda(npts, idx, lam, idx_perm, 0)
    # the support (weights > 1e-9) moves whole where it has at most six entries and the codes of the set are distinct
    exact = ((lam > G.SUPPORT_MIN).sum(axis=0) <= G.FREE_MAX) & np.array([np.unique(idx[:, b]).size == S_pts for b in range(n)])
    assert np.array_equal(want[:, exact], np.where(lam_perm > G.SUPPORT_MIN, lam_perm, 0.0)[:, exact])
    print("permuted set: the support moves whole on %d of %d problems (support sizes %s)" % (exact.sum(), n, np.bincount((lam > G.SUPPORT_MIN).sum(axis=0)).tolist()))
    assert exact.mean() > 0.5
    idx_perm_t = torch.as_tensor(idx_perm, device="cuda")
    got = sv.shift_lambda(idx_t, torch.as_tensor(lam, device="cuda"), idx_perm_t, 0)
    assert np.array_equal(got.cpu().numpy(), want)
    plan = {"X_optm_ref": torch.as_tensor(cold["X_optm"], device="cuda"), "U_optm_ref": torch.as_tensor(cold["U_optm"], device="cuda")}
    wa = solve(idx_t, dict(plan, convex_combi_optm_ref=torch.as_tensor(lam, device="cuda")))
    wb = solve(idx_perm_t, dict(plan, convex_combi_optm_ref=got))
    both = (wa["status"] == 0) & (wb["status"] == 0)
    err = max(np.abs((wa[k] - wb[k]) / sc[:, None, None])[..., both].max() for k, sc in (("X_optm", P.SCALE_X), ("U_optm", P.SCALE_U), ("dU_optm", P.SCALE_U)))
    differ = np.nonzero(wa["accepted"] != wb["accepted"])[0]
    print("warm on the permuted set: accepted %d / %d (as it was: %d), differing on %s (support moved whole there: %s); answers %.1e apart"
          % (wb["accepted"].sum(), n, wa["accepted"].sum(), differ.tolist(), exact[differ].tolist(), err))
    assert wa["accepted"].sum() > 0 and np.array_equal(wa["status"], wb["status"])
    assert np.array_equal(wa["accepted"], wb["accepted"]) and err < 1e-8
    sv.close()


# ---- launch order (lmpc_launch_order_from_iters) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 63, 64, 1023, 1024, 1025, 2049, 4099])
def test_launch_order_is_the_stable_sort_at_every_chunk_count(pkg, B):
    """One workgroup walks the batch in chunks of 1024: one partial chunk, exactly one, one and a bit, two and a bit, four and a bit
    -- the rank carried from chunk to chunk -- with counts below 0 and above 63 (both clips), all equal, and strictly increasing."""
    sv = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    rng = np.random.default_rng(B)
    for iters in (rng.integers(-3, 71, B), np.full(B, 7), np.arange(B), rng.integers(5, 9, B)):
        it = np.asarray(iters, dtype=np.int32)
        got = sv.launch_order_from_iters(torch.as_tensor(it, device="cuda"), torch.full((B,), -5, dtype=torch.int32, device="cuda")).cpu().numpy()
        assert np.array_equal(got, G.launch_order(it)), (B, np.nonzero(got != G.launch_order(it))[0][:8])
    sv.close()


# ---- a period between two solves (lmpc_loop_advance_batch) against the oracle's node and simulator -------------------------------------------
def _period_inputs(pkg, N, B, dt):
    """Inputs of a period without a solve: the cold start's rollout (prepare) with seeded noise as the old plan, the same rollout
    with other noise as the "solution", a status with zeros, ones and twos in every wave's worth of lanes, and eight cars so close
    to the end of the lap that the plant step takes them across it."""
    tr = pkg.workloads.synthetic_track("barc")
    sv = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
    rng = np.random.default_rng(100 + N)
    L = tr["L"]
    s0 = rng.uniform(0, 0.95 * L, B)
    near_end = np.array([2, 3, 40, 63, 64, 100, 127, 129])
    s0[near_end] = L - rng.uniform(1e-3, 4e-3, near_end.size)         # (1 m/s x 25 ms = 25 mm per period)
    x = np.stack([s0, rng.uniform(-0.1, 0.1, B), rng.normal(0, 0.03, B), 0.7 * S.track_lookup(tr["vel"], s0, L), rng.normal(0, 0.02, B), rng.normal(0, 0.1, B)])
    assert (x[3] > 0.5).all()
    inp = _np(sv.prepare(tr, x.copy(), dt, speed_scale=0.9))
    sx, su = np.array([0.01, 0.005, 0.005, 0.02, 0.005, 0.02])[:, None, None], np.array([0.05, 0.02])[:, None, None]
    roll = inp["X_ref"].copy()
    sol = {"X_optm": roll + sx * rng.normal(0, 1, roll.shape), "U_optm": su * rng.normal(0, 1, (2, N - 1, B))}
    inp["X_ref"] = roll + sx * rng.normal(0, 1, roll.shape)
    inp["U_ref"] = su * rng.normal(0, 1, (2, N - 1, B))
    inp["bound_left"] = inp["bound_left"] + rng.normal(0, 0.01, (N, B))        # (which knot's bounds the excursion is taken against shows)
    inp["bound_right"] = inp["bound_right"] + rng.normal(0, 0.01, (N, B))
    status = np.zeros(B, dtype=np.int32)
    status[1::5] = 1
    status[3::7] = 2
    status[[128, 129]] = [0, 2]
    for lo, hi in ((0, 64), (64, 128), (128, B)):
        assert set(status[lo:hi]) >= ({0, 1, 2} if hi - lo > 2 else {0, 2})
    sol["status"] = status
    sol["iters"] = np.full(B, 5, dtype=np.int32)
    return tr, sv, x, inp, sol


@pytest.mark.parametrize("restart", [True, False])
@pytest.mark.parametrize("N", [3, 9, 17, 20])
def test_loop_advance_against_the_oracle(pkg, N, restart):
    """B = 130 (a partial wave) at horizons below, at and across the eight waves a workgroup deals the knots to."""
    B, dt = 130, 0.025
    cfg, veh = P.barc_tracking_mpc(N), P.barc_vehicle()
    tr, sv, x, inp, sol = _period_inputs(pkg, N, B, dt)
    ref = G.loop_advance(cfg, veh, tr, inp, sol, x, dt, dt / 2, 2, 0.9, restart)
    wrapped = ref["x"][0] < x[0]
    assert wrapped.sum() >= 4 and (~wrapped).sum() >= 4 and (ref["distance"] > 0).all()
    trk = sv.device_track(tr)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    sol_t = {k: dev(v) for k, v in sol.items()}
    rng = np.random.default_rng(5)
    dist0, exc0, nf0 = rng.uniform(0, 3, B), rng.uniform(-0.3, 0.1, B), rng.integers(0, 4, B)

    def call(acc_on, dist, exc, nf, acc):
        cur = {k: dev(inp[k]) for k in G.REF_KEYS}
        xt, ut = dev(x), torch.full((2, B), 9.0, dtype=torch.float64, device="cuda")
        kw = dict(distance=dist, worst_excess=exc, n_fail=nf, n_accepted=acc) if acc_on else {}
        sv.loop_advance(trk, cur, sol_t, xt, ut, dt, dt / 2, 2, speed_scale=0.9, restart_failed=restart, **kw)
        got = _np(cur)
        got["x"], got["u"] = xt.cpu().numpy(), ut.cpu().numpy()
        return got

    def check(got):
        assert np.array_equal(got["u"], ref["u"])                              # a selection: exact
        assert _close(got["x"], ref["x"]) and (got["x"][0] >= 0).all() and (got["x"][0] < tr["L"]).all()
        keep = ~ref["restarted"]
        for k in G.REF_KEYS:
            assert _close(got[k][..., keep], ref[k][..., keep]), k
        if ref["restarted"].any():
            cars = np.nonzero(ref["restarted"])[0]
            assert _close(got["X_ref"][:, 0, cars], ref["x"][:, cars]) and np.array_equal(got["X_ref"][:, 0, cars], got["x"][:, cars])
            assert (got["U_ref"][:, :, cars] == 1e-9).all() and (got["T_ref"][:, cars] == dt).all()
            err = G.cold_rollout_errors(cfg, veh, tr, got, cars, dt, 0.9)
            assert all(e <= REL for e in err.values()), err

    dist, exc, nf = dev(dist0), dev(exc0), dev(nf0.astype(np.int64))
    acc = torch.zeros((), dtype=torch.int64, device="cuda")
    check(call(True, dist, exc, nf, acc))
    assert _close(dist.cpu().numpy(), dist0 + ref["distance"]) and _close(exc.cpu().numpy(), np.maximum(exc0, ref["excess"]))
    assert np.array_equal(nf.cpu().numpy(), nf0 + ref["fail"]) and int(acc) == 0          # (no warm solve ran on this handle)
    # the accumulators accumulate: the same period once more on top
    check(call(True, dist, exc, nf, acc))
    assert _close(dist.cpu().numpy(), dist0 + ref["distance"] + ref["distance"]) and _close(exc.cpu().numpy(), np.maximum(exc0, ref["excess"]))
    assert np.array_equal(nf.cpu().numpy(), nf0 + 2 * ref["fail"]) and int(acc) == 0
    # every accumulator NULL
    check(call(False, None, None, None, None))
    sv.close()


# ---- the warm flag through every solve entry ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["f32", "mixed", "full_dynamics", "f64"])
def test_a_cold_solve_through_any_entry_clears_the_warm_flags(pkg, entry):
    """After a warm solve of B problems the flags say which attempts were accepted and lmpc_loop_advance_batch counts them; a cold
    solve of the same B through ANY entry -- the fp32 one has a launch path of its own -- leaves nothing to report or to count."""
    from test_gpu_warm import _periods, _start

    B, dt = 200, 0.025
    tr, sv, inp = _start(pkg, 20, B)
    trk = sv.device_track(tr)
    nxt = _periods(sv, tr, inp, 6)
    out = sv.solve(nxt, warm=True)
    flags = sv.warm_accepted(B).cpu().numpy()
    status = out["status"].cpu().numpy()
    assert set(np.unique(flags)) <= {0, 1} and flags.sum() > 0
    assert not sv.warm_accepted(B // 2).cpu().numpy().any()            # a smaller batch gets zeros, not a prefix (include/lmpc_hip.h)
    assert np.array_equal(sv.warm_accepted(B).cpu().numpy(), flags)
    acc = torch.zeros((), dtype=torch.int64, device="cuda")

    def advance():
        cur = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in nxt.items()}
        sv.loop_advance(trk, cur, out, nxt["x_ic"].clone(), nxt["u_ic"].clone(), dt, dt / 2, 2, speed_scale=0.9, n_accepted=acc)
        return int(acc)

    counted = int(((flags != 0) & (status == 0)).sum())
    assert advance() == counted and counted > 0
    if entry == "f32":
        sv.solve_f32(nxt)
    elif entry == "mixed":
        sv.solve(nxt, mixed=True)
    elif entry == "full_dynamics":
        sv.solve_full_dynamics(nxt, max_sqp=2)
    else:
        sv.solve(nxt)
    assert not sv.warm_accepted(B).cpu().numpy().any()
    assert advance() == counted                                            # (nothing added)
    sv.close()


# ---- an infeasible initial state through the two-wave kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [41, 65, 81])
def test_infeasible_initial_state_through_the_two_wave_kernel(pkg, N):
    """test_infeasible_initial_state_and_determinism's construction (one car's vx below x_min[3]) at horizons the library gives to
    the two-wave kernel: the early exit is where two waves with separate barrier sites could part ways.  The serial twin says what
    is to come out; the neighbours' answers are the twin's, the one-wave kernel's, and the same bits from run to run."""
    from oracle import qp as Q

    B, car = 64, 5
    cfg, veh = P.barc_tracking_mpc(N), P.barc_vehicle()
    tr = pkg.workloads.synthetic_track("barc")
    u_lo, u_hi, _, _ = Q.effective_bounds(cfg, veh)
    x, u = pkg.workloads.sample_initial_states("barc", B, tr["L"], u_lo, u_hi, 4)
    x[car, 3] = 0.05
    assert x[car, 3] < cfg.x_min[3]
    inp = S.cold_start_inputs(cfg, veh, tr, x, u, 0.025)
    tw = cbind.solve_batch(cfg, veh, inp)
    others = np.arange(B) != car
    assert tw["status"][car] == 2 and (tw["status"][others] == 0).all()
    sv = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
    assert sv.launch_info("f64")["threads_per_problem"] == 128

    def solve():
        out = sv.alloc_outputs(B)
        for k in ("X_optm", "U_optm", "dU_optm"):
            out[k].zero_()                     # (whatever the kernel leaves unwritten for the infeasible car is the same in every run)
        return _np(sv.solve(inp, out))

    o2, o2b = solve(), solve()
    sv.set_waves_per_problem(1)
    o1 = solve()
    sv.close()
    assert np.array_equal(o2["status"], tw["status"]) and np.array_equal(o1["status"], tw["status"])
    keys = ("X_optm", "U_optm", "dU_optm")
    exu, ed = per_problem_err({k: o2[k][..., others] for k in keys}, {k: tw[k][..., others] for k in keys})
    e12 = np.abs((o2["X_optm"] - o1["X_optm"]) / P.SCALE_X[:, None, None])[..., others].max()
    print("N = %d, one infeasible start among %d: two waves vs twin X/U %.1e dU %.1e, vs one wave %.1e" % (N, B, exu.max(), ed.max(), e12))
    assert exu.max() < TOL_TWIN and ed.max() < TOL_TWIN
    assert e12 < 1e-8                      # (what test_two_wave_kernel_against_the_twin_and_the_one_wave_kernel asks of the two kernels)
    for k in keys + ("status", "iters"):
        assert np.array_equal(o2[k], o2b[k]), k
