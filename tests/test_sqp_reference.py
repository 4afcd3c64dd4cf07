"""The restated pass of tests/sqp_cases.py pinned without a GPU: its merit terms against an independent assembly (the dense QP of
oracle/qp.py through oracle.nlp.merit_cost), its line search and its pass on hand-worked cases, and the samples the GPU tests run
on: four passes of the chain with the serial C twin's QPs must shorten steps, back off and leave few steps to rounding -- what makes
tests/test_gpu_sqp.py worth running."""
import numpy as np
import pytest

import sqp_cases as C
from oracle import nlp as NLP, params as P, qp as Q, scenario as S


# ---- merit_terms against the dense assembly --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tracking N = 8", "tracking N = 8, Euler", "learning (3, 32)", "learning (10, 32)"])
def test_merit_terms_against_the_dense_objective(pkg, name):
    """merit(y1) - merit(y0) (the dense objective carries the constant of the tracking cost): two sums of about 100 fp64 terms in
    different orders, so 1e-12 relative to the size of what is summed, |merit(y0)| + |merit(y1)|.  The points leave the track (the
    boundary slack is at work) and, for the learning problem, the hull."""
    sm = C.sample(pkg, name)
    cfg, veh, inp, n_lam = sm["cfg"], sm["veh"], sm["inp"], sm["S"]
    rng = np.random.default_rng(3)
    B = inp["X_ref"].shape[2]
    pts = []
    for _ in range(2):
        X = inp["X_ref"] + rng.normal(0, 1, inp["X_ref"].shape) * np.array([0.05, 0.4, 0.1, 0.3, 0.1, 0.3])[:, None, None]
        U = rng.normal(0, 1, inp["U_ref"].shape) * np.array([0.005, 0.1])[:, None, None]
        dU = rng.normal(0, 1, inp["U_ref"].shape) * np.array([0.05, 1.0])[:, None, None]
        lam = rng.dirichlet(np.ones(n_lam), B).T * rng.uniform(0.5, 1.5, B) if n_lam else np.zeros((0, B))
        pts.append((X, U, dU, lam))
    terms = C.terms_of(sm)
    (J0, c0, i0), (J1, c1, i1) = terms(*pts[0]), terms(*pts[1])
    outside = 0
    for b in (0, 7, 63, 64):
        qp = Q.build_qp(cfg, veh, S.problem(inp, b), *((sm["ss_x"][:, :, b], sm["ss_j"][:, b]) if n_lam else ()))
        m = []
        for X, U, dU, lam in pts:
            y = Q.pack(qp, X[:, :, b], U[:, :, b], dU[:, :, b], sigma=0.0, lam=lam[:, b], eps=np.zeros(6))
            m.append(NLP.merit_cost(qp, y))
        assert abs((J1[b] - J0[b]) - (m[1] - m[0])) <= 1e-12 * (abs(m[0]) + abs(m[1])), (b, J1[b] - J0[b], m[1] - m[0])
        marg = cfg.margin + veh.b / 2
        outside += int((pts[0][0][1, :, b] > inp["bound_left"][:, b] - marg).any())
        # the defect norms against the oracle's own defect of the same point
        d = np.abs(NLP.defect(veh, S.problem(inp, b), pts[0][0][:, :, b], pts[0][1][:, :, b]))
        assert abs(c0[b] - d.sum()) <= 1e-13 * d.sum() and abs(i0[b] - d.max()) <= 1e-13 * d.max()
    assert outside >= 1 and (c0 > 0).all()


def test_merit_terms_at_a_rollout_have_no_defect(pkg):
    sm = C.sample(pkg, "tracking N = 8")
    inp = sm["inp"]
    _, c1, cinf = C.terms_of(sm)(inp["X_ref"], inp["U_ref"], np.zeros_like(inp["U_ref"]), np.zeros((0, C.B_SAMPLE)))
    assert c1.max() < 1e-13 and (cinf <= c1).all()          # (the cold start is a rollout with the same step map)


# ---- line_search, hand-worked ----------------------------------------------------------------------------------------------------------
def test_line_search_penalty_weight():
    flat = [0.0] * 8
    # c0 > 0 and dJ > 0: nu = dJ / (0.9 c0) = 0.9 / 0.45 = 2; phi0 = 1 + 2 * 0.5 = 2, slope = 0.9 - 1 = -0.1; phi(1) = 1.9 <= 2 - 1e-5
    a, nu, margin = C.line_search(1.0, 0.5, [1.9] * 8, flat, 0.0)
    assert a == 1.0 and abs(nu - 2.0) < 1e-14 and abs(margin - (0.1 - 1e-5) / 3.0) < 1e-12
    # a larger weight from an earlier pass stays
    assert C.line_search(1.0, 0.5, [1.9] * 8, flat, 5.0)[:2] == (1.0, 5.0)
    # dJ < 0: not raised, whatever c0; never below 1e-3
    assert C.line_search(1.0, 0.5, [0.5] * 8, flat, 0.0)[:2] == (1.0, 1e-3)
    assert C.line_search(1.0, 0.5, [0.5] * 8, flat, 0.25)[:2] == (1.0, 0.25)
    # c0 = 0 and dJ > 0: not raised (no division by zero), and no step length passes: phi(a) = 2 > 1 + 1e-4 a
    a, nu, _ = C.line_search(1.0, 0.0, [2.0] * 8, flat, 0.0)
    assert (a, nu) == (2.0 ** -7, 1e-3)


def test_line_search_step_lengths():
    # phi0 = 1 (c0 = 0, nu = 1e-3), dJ = 9: the rhs is 1 + 9e-4 a; cost 10, 5, 0.5 at a = 1, 1/2, 1/4: the third passes
    a, nu, margin = C.line_search(1.0, 0.0, [10.0, 5.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0], [0.0] * 8, 0.0)
    assert (a, nu) == (0.25, 1e-3) and abs(margin - (1 + 9e-4 * 0.25 - 0.5) / 2.0) < 1e-12
    # the defect of the trial point counts with the weight: J passes at a = 1 but J + nu c does not (nu = 5), at a = 1/2 it does
    a, nu, _ = C.line_search(1.0, 0.1, [0.9] * 8, [0.2, 0.05, 0, 0, 0, 0, 0, 0], 5.0)
    assert (a, nu) == (0.5, 5.0)          # phi0 = 1.5; phi(1) = 1.9, phi(1/2) = 1.15 <= 1.5 + 1e-4 / 2 * (-0.1 - 0.5)
    # a stops at 2^-7 and is taken whatever the test says
    assert C.line_search(1.0, 0.0, [3.0] * 8, [0.0] * 8, 0.0)[0] == 2.0 ** -7
    # the margin: far from the rule's edge, and on it (nothing to gain, nothing to lose: the 1e-14 slack alone lets the step pass)
    a, _, margin = C.line_search(1.0, 0.0, [1.0 - 1e-4] * 8, [0.0] * 8, 0.0)          # dJ = -1e-4: rhs(1) = 1 - 1e-8 + 2e-14
    assert a == 1.0 and margin > 1e-5
    a, _, margin = C.line_search(0.0, 0.0, [0.0] * 8, [0.0] * 8, 0.0)
    assert a == 1.0 and margin == 1e-14


# ---- expected_pass, hand-worked --------------------------------------------------------------------------------------------------------
def _toy_terms(X, U, dU, lam):
    """A made-up merit: cost |X|^2 + |U|^2 + sum lambda, "defect" the gap between the two knots' e_y."""
    c = np.abs(X[1, 1] - X[1, 0])
    return (X ** 2).sum(axis=(0, 1)) + (U ** 2).sum(axis=(0, 1)) + lam.sum(axis=0), c, c


def _toy_qp(B, value, status=0, iters=5):
    return {"X": np.full((6, 2, B), float(value)), "U": np.full((2, 1, B), float(value)), "dU": np.full((2, 1, B), float(value)),
            "lam": np.full((2, B), float(value)), "status": np.full(B, status), "iters": np.full(B, iters)}


def _toy_start(B=2):
    return C.initial_state(np.full((6, 2, B), 8.0), np.full((2, 1, B), 8.0), 2)


def test_first_pass_takes_the_full_step():
    st0 = _toy_start()
    qp = _toy_qp(2, 4.0, iters=7)
    st, log = C.expected_pass(_toy_terms, st0, qp, True, 1e-9)          # (the cost falls from 8 to 4 anyway; on a first pass nobody asks)
    assert (log["branch"] == "step").all() and (log["a"] == 1.0).all()
    for k in C.ITERATE:
        assert np.array_equal(st[k], qp[k]) and np.array_equal(st[k + "_saved"], st0[k])
    assert (st["move"] == 4.0 / 0.1).all()          # the largest scaled change is e_psi's: 4 / 0.1
    assert (st["sqp_iters"] == 1).all() and (st["iters"] == 7).all() and (st["status"] == 0).all() and st["active"].all()
    assert (st["nu"] == 0).all() and st0["X"][0, 0, 0] == 8.0          # (the state handed in is not modified)
    # a cost that RISES is taken in full on the first pass too
    st, log = C.expected_pass(_toy_terms, st0, _toy_qp(2, 16.0), True, 1e-9)
    assert (log["a"] == 1.0).all() and (st["X"] == 16.0).all()


def test_a_later_pass_searches_and_a_small_step_ends_the_problem():
    st1, _ = C.expected_pass(_toy_terms, _toy_start(), _toy_qp(2, 4.0), True, 1e-9)
    qp = _toy_qp(2, 16.0)          # cost up: no step length passes
    qp["X"][..., 1] = 4.0 + 1e-12          # problem 1: the QP proposes (almost) no step
    qp["U"][..., 1] = qp["dU"][..., 1] = qp["lam"][..., 1] = 4.0
    st2, log = C.expected_pass(_toy_terms, st1, qp, False, 1e-9)
    assert log["a"][0] == 2.0 ** -7 and st2["X"][0, 0, 0] == 4.0 + 12.0 / 128 and st2["lam"][0, 0] == 4.0 + 12.0 / 128
    assert st2["move"][0] == 12.0 / 0.1 and st2["active"][0] and st2["nu"][0] == 1e-3
    assert not st2["active"][1] and st2["move"][1] <= 1e-9 and st2["sqp_iters"][1] == 2          # move = the QP's step, 1e-12 / 0.1
    assert np.array_equal(st2["X_saved"], st1["X"])
    # the ended problem is left alone from now on, counters included
    st3, log = C.expected_pass(_toy_terms, st2, _toy_qp(2, 1.0, status=2), False, 1e-9)
    assert log["branch"][1] == "idle"
    for k, v in st3.items():
        assert np.array_equal(v[..., 1], st2[k][..., 1]), k
    # a step length handed in replaces the search's
    st2b, logb = C.expected_pass(_toy_terms, st1, qp, False, 1e-9, a_given=np.array([0.5, np.nan]))
    assert logb["a"][0] == 0.5 and st2b["X"][0, 0, 0] == 10.0 and st2b["move"][0] == st2["move"][0]


def test_back_off_goes_to_the_midpoint_with_the_saved_iterate_not_the_start():
    st1, _ = C.expected_pass(_toy_terms, _toy_start(), _toy_qp(2, 4.0), True, 1e-9)          # 8 -> 4, saved 8
    st2, _ = C.expected_pass(_toy_terms, st1, _toy_qp(2, 2.0), False, 1e-9)                   # 4 -> 2 (cost down: a = 1), saved 4
    assert (st2["X"] == 2.0).all() and (st2["X_saved"] == 4.0).all()
    bad = _toy_qp(2, -77.0, status=2, iters=3)
    bad["status"][1] = 0          # problem 1 carries on
    st3, log = C.expected_pass(_toy_terms, st2, bad, False, 1e-9)
    assert log["branch"][0] == "backoff" and log["branch"][1] == "step"
    for k in C.ITERATE:
        assert (st3[k][..., 0] == 3.0).all(), k          # (2 + 4) / 2 -- not (2 + 8) / 2, and nothing of the failed QP's arrays
        assert (st3[k + "_saved"][..., 0] == 4.0).all(), k
    assert st3["backoffs"][0] == 1 and st3["nu"][0] == st2["nu"][0] and st3["move"][0] == st2["move"][0]
    assert st3["status"][0] == 2 and st3["sqp_iters"][0] == 3 and st3["iters"][0] == 5 + 5 + 3 and st3["active"][0]
    # a second failure in a row: the midpoint of the new iterate and the SAME saved iterate
    st4, _ = C.expected_pass(_toy_terms, st3, bad, False, 1e-9)
    assert (st4["X"][..., 0] == 3.5).all() and st4["backoffs"][0] == 2
    # a QP that succeeds resets the count
    st5, _ = C.expected_pass(_toy_terms, st4, _toy_qp(2, 1.0), False, 1e-9)
    assert st5["backoffs"][0] == 0 and (st5["X_saved"][..., 0] == 3.5).all() and st5["status"][0] == 0


def test_the_seventh_failure_in_a_row_stops_the_problem():
    st, _ = C.expected_pass(_toy_terms, _toy_start(1), _toy_qp(1, 4.0), True, 1e-9)
    bad = _toy_qp(1, 0.0, status=2, iters=2)
    x = 4.0
    for n in range(1, 7):
        st, log = C.expected_pass(_toy_terms, st, bad, False, 1e-9)
        x = 0.5 * (x + 8.0)
        assert log["branch"][0] == "backoff" and st["backoffs"][0] == n and (st["X"] == x).all() and st["active"][0]
    last, log = C.expected_pass(_toy_terms, st, bad, False, 1e-9)
    assert log["branch"][0] == "stop" and not last["active"][0] and last["status"][0] == 2
    assert last["sqp_iters"][0] == 8 and last["iters"][0] == 5 + 7 * 2
    for k in C.ITERATE + ("move", "defect", "nu"):
        assert np.array_equal(last[k], st[k]), k


def test_a_failed_first_qp_stops_at_once():
    st0 = _toy_start()
    bad = _toy_qp(2, 0.0, status=2, iters=4)
    bad["status"][1] = 0
    st, log = C.expected_pass(_toy_terms, st0, bad, True, 1e-9)
    assert list(log["branch"]) == ["stop", "step"]
    for k in C.ITERATE:
        assert np.array_equal(st[k][..., 0], st0[k][..., 0]), k
    assert (st["dU"][..., 0] == 0).all() and (st["lam"][..., 0] == 0).all()
    assert st["sqp_iters"][0] == 1 and st["status"][0] == 2 and st["iters"][0] == 4 and not st["active"][0]
    assert st["defect"][0] == 0.0 and np.isinf(st["move"][0]) and not st["move"][0] <= 1e-9


# ---- the dense SQP on a learning problem -----------------------------------------------------------------------------------------------
def test_dense_sqp_solves_a_learning_problem(pkg):
    sm = C.sample(pkg, "learning (3, 32)")
    b = 0
    pr, sx, sj = S.problem(sm["inp"], b), sm["ss_x"][:, :, b], sm["ss_j"][:, b]
    X, U, dU, sigma, info = NLP.solve_nlp_dense(sm["cfg"], sm["veh"], pr, tol=1e-8, ss_x=sx, ss_j=sj)
    lam = info["lam"]
    assert info["status"] == 0 and abs(lam.sum() - 1.0) < 1e-9 and lam.min() > -1e-10
    c = NLP.nlp_kkt_certificate(sm["cfg"], sm["veh"], dict(pr, ss_x=sx, ss_j=sj), X, U, dU, lam=lam, eps=X[:, -1] - sx @ lam)
    assert c["defect"] < 1e-7 and c["ineq"] < 1e-7 and c["stat"] < 1e-6 and c["comp"] < 1e-6, c


# ---- the chain on the CPU: the samples are worth running -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.SAMPLES)
def test_four_passes_with_the_twin_exercise_the_rule(pkg, name):
    """Four passes (past the fourth the margin reaches the Armijo test's own 1e-14 slack and rounding decides the step length).
    Over passes 2 to 4: at most 10 % of the (problem, pass) pairs undecided (margin < 1e-9), at least 20 shortened steps, and at
    least one back-off in the N = 8 and N = 20 tracking samples."""
    sm = C.sample(pkg, name)
    st, logs = C.run_chain(sm, C.twin_qp(sm), 4)
    n = C.chain_counts(logs)
    print(name, n, "nu raised on", int((st["nu"] > C.NU_MIN).sum()), "problems; active after four passes", int(st["active"].sum()))
    assert len(logs) == 4 and (logs[0]["branch"] == "step").all()
    assert n["pairs"] >= 190 and n["undecided"] <= 0.10 * n["pairs"]
    assert n["short"] >= 20
    if name in ("tracking N = 8", "tracking N = 20"):
        assert n["backoffs"] >= 1
    assert (st["nu"] > C.NU_MIN).sum() >= 5          # the weight is raised somewhere, or a kernel that never raises it would pass
    if sm["S"]:
        assert np.abs(st["lam"]).max() > 0.1          # the weights move with the step
