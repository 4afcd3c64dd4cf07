"""Per-car error-dynamics regression with one feature list per regressed row (lmpc_fleet_ss_set_regression_rows,
csrc/lmpc_fleet_reg_rows_kernel.hip) against the CPU restatement.  Needs an MI355X.

The fixtures and sizes are tests/test_gpu_fleet_regression.py's (37 or fewer cars, a ring of 3 laps of at most 64 samples); the
reference for car b is regression_rows_cases.rows_reference -- oracle.regression.regress_batch once per row -- on
fleet_ss_get_laps(b), what the device holds for that car at that moment, at 1e-9 (1 + max|ref|) on A, B and g of every (car, stage);
a row of a query the oracle finds no candidate for comes back bit-identical."""
import numpy as np
import pytest
import torch

from oracle import params as P
from regression_rows_cases import ROWS_245, ROWS_444, ROWS_555, rel_err, row_masks, rows_reference
from test_gpu_fleet_regression import (CAP, RING, SPEC_ALL, _feed, _flat, _fleet_of_37, _fleet_run, _monotone, _near_lap, _plant_laps,
                                       _rec_seq, _regress, _setup)
from test_regression_oracle import synthetic_lap
from tolerances import TOL_TWIN

pytestmark = pytest.mark.gpu

H = 0.6


def _check_rows_against_oracle(sv, veh, inp, rows, h, as_written, lin, res, what):
    """Every car against the reference on ITS laps as the device holds them.  Returns (touched [B, rows, N-1], per-car laps)."""
    N, B = inp["X_ref"].shape[1:]
    (A0, B0, g0), (A, Bm, g) = lin, res
    got, nominal = [_flat(a) for a in (A, Bm, g)], [_flat(a) for a in (A0, B0, g0)]
    masks = row_masks(rows)
    worst, touched_all, held = 0.0, [], []
    for b in range(B):
        laps = sv.fleet_ss_get_laps(b)
        held.append(laps)
        laps = [l for l in laps if l[0].shape[0] >= 2]      # a lap of one sample holds no sample with a successor
        touched = np.zeros((len(rows), N - 1), bool)
        ref = [a[b] for a in nominal]
        if laps:
            qx, qu = inp["X_ref"][:, :N - 1, b].T.copy(), inp["U_ref"][:, :, b].T.copy()
            *ref, touched = rows_reference(veh, laps, rows, h, qx, qu, *ref, as_written=as_written)
        for k, (a, r, a0) in enumerate(zip(got, ref, nominal)):
            e = rel_err(a[b], r)
            worst = max(worst, float(e.max()))
            assert e.max() < 1e-9, (what, b, int(np.argmax(e)), float(e.max()))
            may = np.zeros(a[b].shape, bool)
            for o in range(len(rows)):
                may |= touched[o].reshape((-1,) + (1,) * masks[o][k].ndim) & masks[o][k]
            assert np.array_equal(a[b][~may], a0[b][~may]), (what, b)      # outside the lists of a touched row: the same bits
        touched_all.append(touched)
    touched_all = np.stack(touched_all)
    print("%s: %d (query, row) pairs, %d touched, worst %.1e relative to 1 + max|ref|" % (what, touched_all.size, touched_all.sum(), worst))
    return touched_all, held


# ---- 1. every car against its own laps ----------------------------------------------------------------------------------------------
ONE_BY_ONE = [("444_n20", 20, ROWS_444, False), ("245_n3_as_written", 3, ROWS_245, True), ("245_n81", 81, ROWS_245, False)]


@pytest.mark.parametrize("case", ONE_BY_ONE, ids=[c[0] for c in ONE_BY_ONE])
def test_every_car_is_regressed_row_by_row_on_its_own_laps(pkg, case):
    """37 cars loaded one by one (test_gpu_fleet_regression._fleet_of_37): a car with no lap, one whose only lap has two samples, full
    rings, every table padding.  N = 3, 20 and 81 (two waves per car), both instances (4 and 5 features per row), both signs."""
    name, N, rows, as_written = case
    rng = np.random.default_rng(sum(map(ord, name)))
    veh, tr, inp, sv = _setup(pkg, "barc", N, 37)
    _fleet_of_37(sv, veh, tr, inp, False, rng)
    sv.fleet_ss_set_regression(rows=rows, dist_max=H, as_written=as_written)
    lin, res = _regress(sv, inp)
    touched, held = _check_rows_against_oracle(sv, veh, inp, rows, H, as_written, lin, res, name)
    sv.close()
    assert held[0] == [] and [l[0].shape[0] for l in held[1]] == [2] and len(held[2]) == RING and len(held[11]) == RING
    assert not touched[0].any()
    for o in range(len(rows)):
        assert touched[:, o].sum() >= touched[:, o].size // 10, (o, touched[:, o].sum())      # >= 10 % of the queries, every row


# ---- 2. the ring moves on -----------------------------------------------------------------------------------------------------------
def test_the_ring_moving_on_repacks_only_the_car_that_crossed(pkg):
    B, N = 12, 20
    veh, tr, inp, sv = _setup(pkg, "barc", N, B)
    L = float(tr["L"])
    n_laps = [1 + b % RING for b in range(B)]
    for b in range(B):
        sv.fleet_ss_load([synthetic_lap(veh, 20 + 3 * l + b, 100 * b + l) for l in range(n_laps[b])], L, car=b)
    sv.fleet_ss_set_regression(rows=ROWS_444, dist_max=H)
    lin = sv.linearize(inp)
    lin_np, res1 = _regress(sv, inp, lin)
    t1, _ = _check_rows_against_oracle(sv, veh, inp, ROWS_444, H, False, lin_np, res1, "loaded")
    # one more full lap for every other car, through the recorder: it closes a lap and, where the ring is full, evicts one
    _feed(sv, B, L, {b: _rec_seq(_monotone(synthetic_lap(veh, 40, 500 + b), L), L, seed=True, close=True) for b in range(0, B, 2)})
    _, res2 = _regress(sv, inp, lin)
    t2, held2 = _check_rows_against_oracle(sv, veh, inp, ROWS_444, H, False, lin_np, res2, "one more lap for the even cars")
    for b in range(B):
        if b % 2:    # saw nothing: the same bits
            assert all(np.array_equal(r1[..., b], r2[..., b]) for r1, r2 in zip(res1, res2)), b
        else:
            assert len(held2[b]) == min(n_laps[b] + 1, RING) and held2[b][-1][0].shape[0] == 40
            assert not np.array_equal(res1[0][..., b], res2[0][..., b]), b
    # reset, and the same NUMBER of laps with other contents: lap_count is what it was, the table must not be
    sv.fleet_ss_reset()
    for b in range(B):
        sv.fleet_ss_load([synthetic_lap(veh, 25 + 2 * l + b, 7000 + 100 * b + l) for l in range(n_laps[b])], L, car=b)
    _, res3 = _regress(sv, inp, lin)
    t3, _ = _check_rows_against_oracle(sv, veh, inp, ROWS_444, H, False, lin_np, res3, "reset and reloaded")
    sv.close()
    for t in (t1, t2, t3):
        assert t.sum() >= t.size // 10


# ---- 3. a new spec invalidates ------------------------------------------------------------------------------------------------------
def test_a_new_rows_spec_or_sign_repacks_every_car(pkg):
    """... and so does the other form on the same store: the (8, 6) one-list table and the 4-feature per-row table have the same
    size, so the allocation is kept and only the stamps stand between one layout and the other."""
    B, N = 9, 10
    veh, tr, inp, sv = _setup(pkg, "barc", N, B)
    rng = np.random.default_rng(3)
    for b in range(B):
        sv.fleet_ss_load([_near_lap(inp, tr, b, 12 + 5 * l + b, rng) for l in range(1 + b % RING)], float(tr["L"]), car=b)
    lin = sv.linearize(inp)
    sizes = {}
    for rows, as_written in ((ROWS_444, False), (ROWS_444, True), (None, False), (ROWS_245, True), (ROWS_245, False), (ROWS_555, False),
                             (ROWS_444, False)):
        if rows is None:
            sv.fleet_ss_set_regression(in_state=SPEC_ALL[0], in_ctrl=SPEC_ALL[1], out_rows=SPEC_ALL[2], dist_max=H)
            sizes["one-list (8, 6)"] = sv.fleet_ss_bytes()
            _regress(sv, inp, lin)                     # packs every car in the one-list layout
            continue
        sv.fleet_ss_set_regression(rows=rows, dist_max=H, as_written=as_written)
        sizes[max(len(s) + len(c) for s, c in rows.values())] = sv.fleet_ss_bytes()
        lin_np, res = _regress(sv, inp, lin)
        touched, _ = _check_rows_against_oracle(sv, veh, inp, rows, H, as_written, lin_np, res, "rows %s as_written %s" % (rows, as_written))
        assert touched.sum() >= touched.size // 10
    sv.close()
    assert sizes[4] == sizes["one-list (8, 6)"] and sizes[5] > sizes[4]


# ---- 4. equal stores, equal answers -------------------------------------------------------------------------------------------------
def test_equal_stores_give_the_shared_rows_regression_and_the_same_solves(pkg):
    B, N = 16, 20
    veh = P.barc_vehicle()
    tr = pkg.workloads.synthetic_track("barc")
    laps = _plant_laps(veh, tr)
    fleet = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
    shared = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
    x0 = np.stack([laps[b % RING][0][3 * b] for b in range(B)], axis=1)       # on the laps: every problem has samples in reach
    inp = fleet.prepare(tr, x0, 0.025)
    inp["u_ic"] = torch.zeros((2, B), dtype=torch.float64, device="cuda")
    base = fleet.solve(inp)
    base = {k: base[k].cpu().numpy() for k in ("X_optm", "U_optm", "dU_optm", "status")}
    fleet.fleet_ss_create(B, CAP)
    fleet.fleet_ss_load(laps, float(tr["L"]), car=-1)
    fleet.fleet_ss_set_regression(rows=ROWS_245, dist_max=H)
    shared.set_regression_laps(laps, rows=ROWS_245, dist_max=H)
    A0, B0, g0 = fleet.linearize(inp)
    got = [t.cpu().numpy() for t in fleet.fleet_ss_regress(inp, A0.clone(), B0.clone(), g0.clone())]
    ref = [t.cpu().numpy() for t in shared.regress(inp, A0.clone(), B0.clone(), g0.clone())]
    for a, r, a0 in zip(got, ref, (A0, B0, g0)):
        assert np.abs(a - r).max() <= 1e-9 * (1 + np.abs(r).max())
        assert np.abs(r - a0.cpu().numpy()).max() > 1e-6       # the correction is there
    out_f, out_s = fleet.solve(inp), shared.solve(inp)
    assert (out_f["status"].cpu().numpy() == out_s["status"].cpu().numpy()).all() and (out_s["status"].cpu().numpy() == 0).all()
    for key, scale in (("X_optm", P.SCALE_X), ("U_optm", P.SCALE_U), ("dU_optm", P.SCALE_U)):
        err = np.abs((out_f[key].cpu().numpy() - out_s[key].cpu().numpy()) / scale[:, None, None]).max()
        assert err < TOL_TWIN, (key, err)
    assert np.abs(out_f["X_optm"].cpu().numpy() - base["X_optm"]).max() > 1e-6      # the corrected model reaches the QP
    fleet.fleet_ss_set_regression(off=True)
    again = fleet.solve(inp)
    for key in ("X_optm", "U_optm", "dU_optm", "status"):
        assert np.array_equal(again[key].cpu().numpy(), base[key]), key
    fleet.close()
    shared.close()


# ---- 5. closed loop -----------------------------------------------------------------------------------------------------------------
def test_closed_loop_with_an_empty_bandwidth_is_the_loop_without_regression(pkg):
    """dist_max = 1e-12: the kernels run every learning period and no sample is ever inside a row's bandwidth -- the same bits."""
    ref = _fleet_run(pkg)
    got = _fleet_run(pkg, regression={"rows": ROWS_444, "dist_max": 1e-12})
    assert all("lmpc" in kinds for kinds in ref["lap_kind"])            # the learning controller (and with it the regression) ran
    assert got["steps"] == ref["steps"] and got["lap_times"] == ref["lap_times"]
    assert np.array_equal(got["x"], ref["x"]) and np.array_equal(got["n_fail"], ref["n_fail"])


def test_closed_loop_correction_reaches_the_qp_on_a_plant_with_less_grip(pkg):
    veh = dict(pkg.presets.barc_vehicle())
    veh["mu"] = 0.9 * veh["mu"]
    plant = pkg.Solver(pkg.presets.barc_tracking_mpc(20), veh, device=0)
    ref = _fleet_run(pkg, plant=plant)
    got = _fleet_run(pkg, plant=plant, regression={"rows": ROWS_444, "dist_max": 0.6})
    plant.close()
    assert all("lmpc" in kinds for kinds in ref["lap_kind"])
    assert np.isfinite(got["x"]).all()
    assert np.abs(got["x"] - ref["x"]).max() > 1e-6
