"""The plain references of tests/glue_cases.py on hand-worked cases (no GPU): the references the GPU tests hold the kernels to get
an anchor of their own.  Store of the code examples: three laps of 5, 7 and 4 samples, so off = (0, 5, 12) and 16 rows in all."""
import numpy as np

import glue_cases as G
from oracle import params as P

NPTS = (5, 7, 4)


def test_codes_hand_worked():
    assert G.offsets(NPTS) == [0, 5, 12]
    assert G.encode(NPTS, 1, 6, 1) == 45 and G.decode(NPTS, 45) == (1, 6, 1)
    assert G.encode(NPTS, 1, 6, 2) == 46 and G.encode(NPTS, 0, 4, 0) == 16
    assert G.decode(NPTS, 22) == (1, 0, 2) and G.decode(NPTS, 5) == (0, 1, 1)
    # lap 1 sample 6 is the lap's last: one sample on is the first sample of the next copy
    assert G.advance_code(NPTS, 45, 1) == 22
    assert G.advance_code(NPTS, 46, 1) == G.NONE          # there is no fourth copy
    assert G.advance_code(NPTS, 16, 2) == 5
    assert G.advance_code(NPTS, 16, 0) == 16 and G.advance_code(NPTS, 45, 0) == 45
    # the lap lookup at its edges: row 4 is lap 0's last, row 5 lap 1's first, row 11 lap 1's last, row 12 lap 2's first
    assert G.decode(NPTS, 4 << 2) == (0, 4, 0) and G.decode(NPTS, 5 << 2) == (1, 0, 0)
    assert G.decode(NPTS, 11 << 2) == (1, 6, 0) and G.decode(NPTS, 12 << 2) == (2, 0, 0)
    assert G.advance_code(NPTS, 4 << 2, 1) == (0 << 2) | 1 and G.advance_code(NPTS, 5 << 2, 1) == 6 << 2
    # more than one copy in one go: lap 2 has four samples, nine on from sample 1 of copy 0 is sample 2 of copy 2; thirteen on is past it
    assert G.advance_code(NPTS, G.encode(NPTS, 2, 1, 0), 9) == G.encode(NPTS, 2, 2, 2)
    assert G.advance_code(NPTS, G.encode(NPTS, 2, 1, 0), 11) == G.NONE


def test_codes_that_name_no_point():
    for adv in (0, 1, 2, 7):
        assert G.advance_code(NPTS, -1, adv) == G.NONE
        for rep in (0, 1, 2):
            assert G.advance_code(NPTS, (16 << 2) | rep, adv) == G.NONE      # row 16 = total: the first row past the store
            assert G.advance_code(NPTS, (21 << 2) | rep, adv) == G.NONE
        assert G.advance_code(NPTS, (3 << 2) | 3, adv) == G.NONE             # rep 3 is no copy
    assert G.decode(NPTS, 15 << 2) == (2, 3, 0) and G.decode(NPTS, 16 << 2) is None


def _sl(idx_prev, lam_prev, idx, advance, routes=None):
    return G.shift_lambda_one(NPTS, np.array(idx_prev), np.array(lam_prev, dtype=np.float64), np.array(idx), advance, routes).tolist()


def test_shift_lambda_candidates_in_order():
    # 45 one sample on is 22: taken.  16 one sample on is code 1 (lap 0 sample 0 rep 1): absent; the point itself, position 2.
    r = []
    assert _sl([45, 16, -1, 8], [0.6, 0.4, 0.0, 0.0], [22, 5, 16, 45], 1, r) == [0.6, 0.0, 0.4, 0.0]
    assert r == [(0.6, 0), (0.4, 1)]
    # advance = 2: 16 -> 5 at position 1; 45 -> lap 1 sample 1 rep 2 = code 26: absent, itself at position 3
    assert _sl([45, 16, -1, 8], [0.6, 0.4, 0.0, 0.0], [22, 5, 16, 45], 2) == [0.0, 0.4, 0.0, 0.6]
    # advance = 0: candidates 0, 0, 1 -- the point itself first, then one sample on
    assert _sl([45, 16, -1, 8], [0.6, 0.4, 0.0, 0.0], [22, 5, 16, 45], 0) == [0.0, 0.0, 0.4, 0.6]
    assert _sl([45], [1.0], [22], 0) == [1.0]
    # the third candidate: 8 (lap 0 sample 2) with advance 1 -> 12 absent, 8 absent, 16 (two on) present
    r = []
    assert _sl([8], [1.0], [16, 0], 1, r) == [1.0, 0.0] and r == [(1.0, 2)]
    # nothing there: dropped
    r = []
    assert _sl([8, 46], [0.5, 0.5], [0, 4], 1, r) == [0.0, 0.0] and r == [(0.5, None), (0.5, None)]
    # rep 2 on a lap's last sample: no next copy, falls back to the point itself when that is there
    assert _sl([46], [1.0], [22, 46], 1) == [0.0, 1.0]


def test_shift_lambda_padding_first_occurrence_and_sums():
    # -1 with a weight in the previous set names no point; -1 in the new set is never a target
    assert _sl([-1, 16], [0.7, 0.3], [-1, -1, 16], 0) == [0.0, 0.0, 0.3]
    # a repeated code: the first occurrence takes the weight
    assert _sl([16], [1.0], [0, 16, 16, 16], 0) == [0.0, 1.0, 0.0, 0.0]
    # two support points on one cell add up, in support order: (0.1 + 0.2) + 0.3 in floating point
    got = _sl([12, 16, 16 + 0], [0.1, 0.2, 0.3], [16], 1)      # 12 one on is 16; 16 one on is absent, itself
    assert got == [(0.1 + 0.2) + 0.3] and got != [0.1 + (0.2 + 0.3)]
    # the threshold is strict
    assert _sl([0, 4, 8], [1e-9, 2e-9, 0.5], [8, 4, 0], 0) == [0.5, 2e-9, 0.0]


def test_shift_lambda_six_out_of_the_first_eight():
    codes = [4 * r for r in range(10)]               # rows 0 .. 9, copy 0; advance 0 keeps each where it is
    idx = codes[::-1]
    lam = [0.01 * (i + 1) for i in range(10)]
    # seven: the seventh would be a seventh positive entry, and so would its other candidate (one on = row 7): dropped
    r = []
    got = _sl(codes[:7], lam[:7], idx, 0, r)
    assert [got[9 - i] for i in range(10)] == lam[:6] + [0.0] * 4 and r[6] == (lam[6], None)
    # ... unless its candidate falls on a cell that is positive already: a seventh entry with the code of the third
    got = _sl(codes[:6] + [codes[2]], lam[:7], idx, 0)
    assert got[9 - 2] == lam[2] + lam[6] and sum(1 for v in got if v > 0) == 6
    # ten: entries nine and ten are not looked at, seven and eight are refused
    r = []
    got = _sl(codes, lam, idx, 0, r)
    assert [got[9 - i] for i in range(10)] == lam[:6] + [0.0] * 4 and len(r) == 8
    # ... even where the cap of six would let them in: a ninth and a tenth with the codes of the first and second would land on
    # cells that are positive already (as the seventh above did), and must add nothing
    r = []
    got = _sl(codes[:8] + [codes[0], codes[1]], lam, idx, 0, r)
    assert [got[9 - i] for i in range(10)] == lam[:6] + [0.0] * 4 and len(r) == 8
    # a refused first candidate leaves the next one its chance: support rows 5 .. 10 of lap 1 fill six cells, then row 4 of lap 0
    # (code 16) with advance 1: one on is code 1 -- present but new (refused); itself: new (refused); two on is code 5 -- make that
    # cell positive beforehand through a support point that lands on it
    idx2 = [4 * r for r in (5, 6, 7, 8, 9)] + [5, 1, 16]
    prev = [4 * r for r in (5, 6, 7, 8, 9)] + [5, 16]
    r = []
    got = G.shift_lambda_one(NPTS, np.array(prev), np.full(7, 0.125), np.array(idx2), 0, r)
    assert got.tolist() == [0.125] * 6 + [0.0, 0.0] and r[-1] == (0.125, None)        # advance 0: 16, 16, then code 1: all new
    r = []
    got = G.shift_lambda_one(NPTS, np.array(prev), np.full(7, 0.125), np.array(idx2), 1, r)
    # advance 1: rows 5 .. 8 move on to 6 .. 9 (row 5 itself is left empty), row 9 -> 10 absent -> itself (taken: adds);
    # code 5 -> lap 0 sample 2 rep 1 absent -> itself; code 16 -> code 1: the sixth cell
    assert got.tolist() == [0.0, 0.125, 0.125, 0.125, 0.25, 0.125, 0.125, 0.0]
    assert [t for _, t in r] == [0, 0, 0, 0, 1, 1, 0]


def test_launch_order_hand_worked():
    assert G.launch_order([3, 9, 3, 70, -2, 0, 63, 9]).tolist() == [3, 6, 1, 7, 0, 2, 4, 5]     # 70 and 63 tie at 63, -2 and 0 at 0
    assert G.launch_order([5, 5, 5]).tolist() == [0, 1, 2]
    assert G.launch_order([1, 2, 3]).tolist() == [2, 1, 0]
    assert G.launch_order([]).tolist() == []


def test_loop_advance_reference_on_a_straight_track():
    """Selection, shift and bookkeeping by hand on three cars (solved / failed / failed near the end of the lap); the model steps
    themselves are the oracle's (tests/test_oracle_dynamics.py)."""
    N, dt, L = 4, 0.025, 10.0
    cfg, veh = P.barc_tracking_mpc(N), P.barc_vehicle()
    M = 8
    tr = {"L": L, "M": M, "curvature": np.zeros(M), "bound_left": np.full(M, 0.5), "bound_right": np.full(M, -0.5), "vel": np.full(M, 2.0)}
    x = np.zeros((6, 3))
    x[0] = [1.0, 2.0, L - 0.01]
    x[1] = [0.0, 0.45, -0.48]
    x[3] = 1.0
    rng = np.random.default_rng(0)
    inp = {"X_ref": rng.normal(0, 0.1, (6, N, 3)) + np.array([0, 0, 0, 1.0, 0, 0])[:, None, None], "U_ref": rng.normal(0, 0.01, (2, N - 1, 3)),
           "bound_left": np.array([[0.5, 0.4, 0.6]] * N) + np.arange(N)[:, None], "bound_right": -np.array([[0.5, 0.6, 0.45]] * N) - np.arange(N)[:, None]}
    sol = {"X_optm": rng.normal(0, 0.1, (6, N, 3)) + np.array([0, 0, 0, 1.0, 0, 0])[:, None, None], "U_optm": rng.normal(0, 0.01, (2, N - 1, 3)),
           "status": np.array([0, 2, 1])}
    for restart in (False, True):
        r = G.loop_advance(cfg, veh, tr, inp, sol, x, dt, dt / 2, 2, 0.9, restart)
        assert np.array_equal(r["u"][:, 0], sol["U_optm"][:, 0, 0]) and np.array_equal(r["u"][:, 1:], inp["U_ref"][:, 0, 1:])
        assert r["fail"].tolist() == [0, 1, 1] and r["restarted"].tolist() == [False, restart, restart]
        # one metre per second for 25 ms on a straight, the random inputs pulling a little either way: 25 mm further give or take
        # 5 mm, the third car across the line -- and the distance is the difference of the abscissae, unwrapped
        assert np.allclose(r["distance"], 0.025, atol=5e-3) and 0.0 <= r["x"][0, 2] < 0.02
        assert np.array_equal(r["distance"][:2], r["x"][0, :2] - x[0, :2]) and r["distance"][2] == r["x"][0, 2] - x[0, 2] + L
        hb = veh.b / 2
        want = [max(r["x"][1, 0] + hb - 0.5, -0.5 - (r["x"][1, 0] - hb)), max(r["x"][1, 1] + hb - 0.4, -0.6 - (r["x"][1, 1] - hb)),
                max(r["x"][1, 2] + hb - 0.6, -0.45 - (r["x"][1, 2] - hb))]
        assert np.allclose(r["excess"], want, rtol=0, atol=1e-15)
        # the shift: knot i is knot i + 1 of the solution (car 0) or of the old plan (cars 1, 2 without a restart), the last input repeated
        assert np.array_equal(r["X_ref"][:, :N - 1, 0], sol["X_optm"][:, 1:, 0]) and np.array_equal(r["U_ref"][:, :, 0], sol["U_optm"][:, [1, 2, 2], 0])
        if restart:
            assert np.array_equal(r["X_ref"][:, 0, 1:], r["x"][:, 1:]) and (r["U_ref"][:, :, 1:] == 1e-9).all()
        else:
            assert np.array_equal(r["X_ref"][:, :N - 1, 1:], inp["X_ref"][:, 1:, 1:]) and np.array_equal(r["U_ref"][:, :, 1:], inp["U_ref"][:, [1, 2, 2], 1:])
        assert (r["T_ref"] == dt).all() and (r["curvatures"] == 0).all()
