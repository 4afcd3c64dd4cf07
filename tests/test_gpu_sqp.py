"""GPU: lmpc_solve_full_dynamics_batch against the plain restatement of one pass (tests/sqp_cases.py, pinned without a GPU by
tests/test_sqp_reference.py), pass by pass: the end of the chain is where an SQP with a line search arrives under many defects; what
goes wrong shows on the way, in the iterate of a problem that stops early and in sqp_iters, iters, sqp_move and defect.

How the passes are obtained: max_sqp = k for k = 1 .. 4 gives the iterate w_k after each pass (every run starts again from X_ref,
U_ref), and the QP the entry solved inside pass k is recomputed with Solver.solve about w_{k-1}.  The premise is that the kernels
give the same bits from run to run (asserted first).  The reference is fed the device's own iterates and QPs, so it never forks
from the device; nu, the saved iterate, the back-off count and the counters are carried by the reference."""
import numpy as np
import pytest
import torch

import sqp_cases as C
from oracle import nlp as NLP, params as P, scenario as S

pytestmark = pytest.mark.gpu
TOL = 1e-9          # step_tol of every run here
PASSES = 4          # (past the fourth the Armijo test is decided by rounding: tests/test_sqp_reference.py)
TOL_ITERATE = 1e-12          # rounding of the blend is three decades below, the 1e-9 the entry works to three decades above
TOL_DEFECT = 1e-9            # |d_gpu - d_ref| / max(1, d_ref): the suite's own bound (test_full_dynamics_sqp_reaches_kkt_points_of_the_nlp)
OUT = ("X_optm", "U_optm", "dU_optm", "convex_combi_optm", "status", "iters", "sqp_iters", "sqp_move", "defect")
_solvers, _traces, _refs = {}, {}, {}


def _np(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items() if not k.startswith("_")}


def _lam_out(n_lam, B):
    return torch.zeros((n_lam, B), dtype=torch.float64, device="cuda")


def _solver(pkg, name):
    if name not in _solvers:
        _solvers[name] = pkg.Solver(*C.sample(pkg, name)["preset"], device=0)
    return _solvers[name]


def _entry(sv, sm, inp, max_sqp, tol=TOL):
    kw = dict(ss_x=sm["ss_x"], ss_j=sm["ss_j"]) if sm["S"] else {}
    if sm["S"] and inp["x_ic"].shape[1] != sm["ss_x"].shape[2]:
        raise ValueError("slice the safe set with the batch")
    return _np(sv.solve_full_dynamics(inp, max_sqp=max_sqp, tol=tol, **kw))


def _qp(sv, sm, inp, X, U):
    """The QP about (X, U) as lmpc_solve_batch solves it"""
    B = X.shape[2]
    out = sv.alloc_outputs(B)
    kw = {}
    if sm["S"]:
        out["convex_combi_optm"] = _lam_out(sm["S"], B)
        kw = dict(ss_x=sm["ss_x"], ss_j=sm["ss_j"])
    return _np(sv.solve(dict(inp, X_ref=X, U_ref=U), out, **kw))


def _iterate(o, n_lam):
    B = o["X_optm"].shape[2]
    return {"X": o["X_optm"], "U": o["U_optm"], "dU": o["dU_optm"], "lam": o["convex_combi_optm"] if n_lam else np.zeros((0, B))}


def _same_bits(a, b, keys=OUT):
    return [k for k in keys if a.get(k) is not None and not np.array_equal(a[k], b[k], equal_nan=True)]


def _trace(pkg, name):
    """W[k] the entry's outputs at max_sqp = k (W[0]: the start), QP[k] the QP about w_{k-1}; computed once per sample."""
    if name not in _traces:
        sm, sv = C.sample(pkg, name), _solver(pkg, name)
        inp = sm["inp"]
        W = [None] + [_entry(sv, sm, inp, k) for k in range(1, PASSES + 1)]
        start = C.initial_state(inp["X_ref"], inp["U_ref"], sm["S"])
        its = [{f: start[f] for f in C.ITERATE}] + [_iterate(w, sm["S"]) for w in W[1:]]
        QP = [None] + [C.qp_of(_qp(sv, sm, inp, its[k - 1]["X"], its[k - 1]["U"]), sm["S"]) for k in range(1, PASSES + 1)]
        _traces[name] = (W, its, QP)
    return _traces[name]


def _step_length(prev, new, qp, b):
    """The step length the device took, from the element of X that the QP moves most (scaled)"""
    d = (qp["X"][..., b] - prev["X"][..., b]) / P.SCALE_X[:, None]
    e = np.unravel_index(np.abs(d).argmax(), d.shape)
    return float((new["X"][..., b][e] - prev["X"][..., b][e]) / (qp["X"][..., b][e] - prev["X"][..., b][e]))


def _reference(pkg, name):
    """expected_pass along the device's own iterates.  -> per pass k = 1 .. 4: (state after the pass, log, a_dev [B], follows [B]):
    a_dev the step length read off the device's iterate (nan where none can be read), follows = the pairs in which the rule leaves
    the choice to rounding (margin < 1e-9) and the reference was handed the device's step length -- one of the rule's own or its
    two neighbours, asserted here."""
    if name in _refs:
        return _refs[name]
    sm = C.sample(pkg, name)
    W, its, QP = _trace(pkg, name)
    terms = C.terms_of(sm)
    st = C.initial_state(sm["inp"]["X_ref"], sm["inp"]["U_ref"], sm["S"])
    B = C.B_SAMPLE
    out = [None]
    for k in range(1, PASSES + 1):
        st = dict(st, **{f: its[k - 1][f] for f in C.ITERATE})          # the device's iterate; everything else is the reference's
        new, log = C.expected_pass(terms, st, QP[k], k == 1, TOL)
        a_dev, follows = np.full(B, np.nan), np.zeros(B, dtype=bool)
        given = np.full(B, np.nan)
        for b in np.nonzero(log["branch"] == "step")[0]:
            if new["move"][b] > 1e-6:          # (a wrong a moves the iterate by at least 2^-7 * 1e-6: readable)
                a_dev[b] = _step_length(its[k - 1], its[k], QP[k], b)
            if k > 1 and log["margin"][b] < C.UNDECIDED:
                follows[b] = True
                if np.isfinite(a_dev[b]):
                    t = int(np.clip(round(-np.log2(max(a_dev[b], 1e-9))), 0, 7))
                    t_ref = C.STEPS.index(log["a"][b])
                    assert abs(t - t_ref) <= 1 and abs(a_dev[b] - C.STEPS[t]) <= 1e-6 * C.STEPS[t], (name, k, b, a_dev[b], log["a"][b])
                    given[b] = C.STEPS[t]
        if np.isfinite(given).any():
            new, log2 = C.expected_pass(terms, st, QP[k], k == 1, TOL, a_given=given)
            log = dict(log2, margin=log["margin"], a_rule=log["a"])
        out.append((new, log, a_dev, follows))
        st = new
    _refs[name] = out
    return out


# ---- the premise ------------------------------------------------------------------------------------------------------------------------
def test_solves_and_passes_are_bitwise_reproducible(pkg):
    """Two solves of the same inputs give the same bits (test_solves_are_bitwise_reproducible), and so do two runs of the entry:
    without this, w_{k-1} of one run is not the iterate pass k of the next run starts from."""
    for name in ("tracking N = 8", "learning (10, 32)"):
        sm, sv = C.sample(pkg, name), _solver(pkg, name)
        inp = sm["inp"]
        a, b = _qp(sv, sm, inp, inp["X_ref"], inp["U_ref"]), _qp(sv, sm, inp, inp["X_ref"], inp["U_ref"])
        assert _same_bits(a, b) == []
        a, b = _entry(sv, sm, inp, 3), _entry(sv, sm, inp, 3)
        assert _same_bits(a, b) == []
        # and the first pass is the full step onto that QP: the recomputed QP is the QP the entry solved
        one, qp = _entry(sv, sm, inp, 1), _qp(sv, sm, inp, inp["X_ref"], inp["U_ref"])
        assert (qp["status"] == 0).all()
        assert _same_bits(one, qp, ("status", "iters")) == [], name
        for k, sc in (("X_optm", P.SCALE_X), ("U_optm", P.SCALE_U), ("dU_optm", P.SCALE_U)):          # (w + 1 (w_QP - w) rounds)
            assert np.abs((one[k] - qp[k]) / sc[:, None, None]).max() <= TOL_ITERATE, (name, k)


# ---- every pass of every problem --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.SAMPLES)
def test_every_pass_of_every_problem(pkg, name):
    sm = C.sample(pkg, name)
    W, its, QP = _trace(pkg, name)
    ref = _reference(pkg, name)
    pairs = undecided = short = 0
    worst = {f: 0.0 for f in C.ITERATE}
    scale = {"X": P.SCALE_X[:, None, None], "U": P.SCALE_U[:, None, None], "dU": P.SCALE_U[:, None, None], "lam": 1.0}
    for k in range(1, PASSES + 1):
        new, log, a_dev, follows = ref[k]
        moved = log["branch"] != "idle"
        if k > 1:
            pairs += int(moved.sum())
            undecided += int(follows.sum())
            short += int(((log["branch"] == "step") & (log["a"] < 1.0)).sum())
        # the step length, wherever the rule decides it and it can be read
        decided = (log["branch"] == "step") & ~follows & np.isfinite(a_dev)
        bad = decided & ~(np.abs(a_dev - log["a"]) <= 1e-6 * log["a"])
        assert not bad.any(), (name, k, np.nonzero(bad)[0], a_dev[bad], log["a"][bad], log["margin"][bad])
        # the iterate
        for f in C.ITERATE:
            if its[k][f].size:
                err = np.abs((its[k][f] - new[f]) / scale[f]).reshape(-1, C.B_SAMPLE).max(axis=0)
                worst[f] = max(worst[f], err.max())
                assert err.max() <= TOL_ITERATE, (name, k, f, np.nonzero(err > TOL_ITERATE)[0], err.max(), log["branch"][err > TOL_ITERATE])
        # the book-keeping
        assert np.array_equal(W[k]["sqp_iters"], new["sqp_iters"]), (name, k)
        assert np.array_equal(W[k]["status"], new["status"]), (name, k)
        assert np.array_equal(W[k]["iters"], new["iters"]), (name, k)
        fin = np.isfinite(new["move"])
        assert np.array_equal(np.isfinite(W[k]["sqp_move"]), fin)
        assert (np.abs(W[k]["sqp_move"][fin] - new["move"][fin]) <= 1e-14 * new["move"][fin]).all(), (name, k)
    print("%s: %d pairs over passes 2 to %d, %d left to rounding (%.1f %%), %d shortened steps; worst scaled error %s"
          % (name, pairs, PASSES, undecided, 100.0 * undecided / pairs, short, {f: "%.1e" % v for f, v in worst.items()}))
    assert pairs >= 190 and undecided <= 0.10 * pairs and short >= 20
    if sm["S"]:
        assert np.abs(its[PASSES]["lam"]).max() > 0.1


@pytest.mark.parametrize("name", C.SAMPLES)
def test_defect_is_that_of_the_iterate_returned(pkg, name):
    """Every problem at every k: stepped, backed off, stopped and unconverged ones alike.  A problem that never moved reports 0."""
    sm = C.sample(pkg, name)
    W, its, QP = _trace(pkg, name)
    terms = C.terms_of(sm)
    worst = 0.0
    for k in range(1, PASSES + 1):
        want = terms(*[its[k][f] for f in C.ITERATE])[2]
        want = np.where((W[k]["sqp_iters"] == 1) & (W[k]["status"] != 0), 0.0, want)
        err = np.abs(W[k]["defect"] - want) / np.maximum(1.0, want)
        worst = max(worst, err.max())
        assert err.max() <= TOL_DEFECT, (name, k, np.nonzero(err > TOL_DEFECT)[0], W[k]["defect"][err > TOL_DEFECT], want[err > TOL_DEFECT])
    print("%s: reported defect against the recomputation, worst %.1e (largest defect %.1e)" % (name, worst, want.max()))


@pytest.mark.parametrize("name", ["tracking N = 8", "tracking N = 20"])
def test_back_offs_occur_and_go_half_way_to_the_saved_iterate(pkg, name):
    W, its, QP = _trace(pkg, name)
    ref = _reference(pkg, name)
    n = 0
    for k in range(2, PASSES + 1):
        new, log, _, _ = ref[k]
        for b in np.nonzero(log["branch"] == "backoff")[0]:
            n += 1
            assert QP[k]["status"][b] != 0 and W[k]["status"][b] == QP[k]["status"][b]
            assert W[k]["sqp_iters"][b] == W[k - 1]["sqp_iters"][b] + 1 and W[k]["sqp_move"][b] == W[k - 1]["sqp_move"][b]
            # half way between w_{k-1} and the iterate its step started from -- NOT the start of the chain where that is another point
            mid = 0.5 * (its[k - 1]["X"][..., b] + new["X_saved"][..., b])
            assert np.abs((its[k]["X"][..., b] - mid) / P.SCALE_X[:, None]).max() <= TOL_ITERATE
            assert np.abs((its[k]["X"][..., b] - its[k - 1]["X"][..., b]) / P.SCALE_X[:, None]).max() > 1e-6
    assert n >= 1, "no problem backs off in passes 2 to %d: the test is vacuous, choose the sample again (on the CPU)" % PASSES
    # a back-off of a later pass distinguishes the saved iterate from the start
    later = sum(int((ref[k][1]["branch"] == "backoff").sum()) for k in range(3, PASSES + 1))
    print("%s: %d back-offs, %d of them after the second pass" % (name, n, later))


# ---- a converged problem is left alone --------------------------------------------------------------------------------------------------
def test_a_converged_problem_is_left_alone(pkg):
    name = "tracking N = 8"
    sm, sv = C.sample(pkg, name), _solver(pkg, name)
    a, b = _entry(sv, sm, sm["inp"], 30), _entry(sv, sm, sm["inp"], 31)
    done = a["sqp_move"] <= TOL
    print("converged after 30 passes: %d of %d; still moving at 31: %d" % (done.sum(), done.size, (b["sqp_iters"] == 31).sum()))
    assert done.sum() >= 5
    for k in OUT:
        if k in a:
            assert np.array_equal(a[k][..., done], b[k][..., done]), k


# ---- a failed first QP ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tracking N = 8", "learning (10, 32)"])
def test_a_failed_first_qp_returns_the_start(pkg, name):
    sm, sv = C.sample(pkg, name), _solver(pkg, name)
    cars = np.array([0, 31, 63, 64])
    inp = dict(sm["inp"], x_ic=sm["inp"]["x_ic"].copy())
    inp["x_ic"][3, cars] = sm["cfg"].x_max[3] + 0.5
    clean, o = _trace(pkg, name)[0][PASSES], _entry(sv, sm, inp, PASSES)
    assert (o["status"][cars] == 2).all() and (o["sqp_iters"][cars] == 1).all()
    assert np.array_equal(o["X_optm"][..., cars], inp["X_ref"][..., cars]) and np.array_equal(o["U_optm"][..., cars], inp["U_ref"][..., cars])
    assert (o["dU_optm"][..., cars] == 0).all() and (o["defect"][cars] == 0).all()
    assert not (o["sqp_move"][cars] <= TOL).any() and np.isinf(o["sqp_move"][cars]).all()
    if sm["S"]:
        assert (o["convex_combi_optm"][..., cars] == 0).all()
    others = np.setdiff1d(np.arange(C.B_SAMPLE), cars)
    for k in OUT:
        if k in o:
            assert np.array_equal(o[k][..., others], clean[k][..., others]), k


# ---- independence of the batch, and the host entry --------------------------------------------------------------------------------------
def _one(sm, b):
    cut = lambda a: np.ascontiguousarray(a[..., b:b + 1])
    inp = {k: (cut(v) if isinstance(v, np.ndarray) else v) for k, v in sm["inp"].items()}
    return dict(sm, inp=inp, ss_x=cut(sm["ss_x"]) if sm["S"] else None, ss_j=cut(sm["ss_j"]) if sm["S"] else None)


@pytest.mark.parametrize("name", ["tracking N = 8", "learning (10, 32)"])
def test_a_problem_solved_alone_is_its_row_of_the_batch(pkg, name):
    sm, sv = C.sample(pkg, name), _solver(pkg, name)
    whole = _trace(pkg, name)[0][PASSES]
    for b in (0, 63, 64):
        one = _one(sm, b)
        alone = _entry(sv, one, one["inp"], PASSES)
        for k in OUT:
            if k in whole:
                assert np.array_equal(alone[k][..., 0], whole[k][..., b]), (b, k)


@pytest.mark.parametrize("name", ["tracking N = 8", "learning (10, 32)"])
def test_the_host_entry_is_the_batch_entrys_row(pkg, name):
    sm, sv = C.sample(pkg, name), _solver(pkg, name)
    whole = _trace(pkg, name)[0][PASSES]
    b = 64
    kw = dict(ss_x=sm["ss_x"], ss_j=sm["ss_j"]) if sm["S"] else {}
    host = sv.solve_full_dynamics_host(sm["inp"], b, max_sqp=PASSES, tol=TOL, **kw)
    assert whole["sqp_iters"][b] == PASSES and whole["defect"][b] > 0
    for k in OUT:
        if k in whole:
            assert np.array_equal(host[k][..., 0], whole[k][..., b]), k


# ---- arguments --------------------------------------------------------------------------------------------------------------------------
def test_a_learning_handle_without_a_safe_set_is_refused_before_anything_runs(pkg):
    """The check is the library's (LMPC_ERR_ARGUMENT, before anything is launched or written); the same handle solves afterwards."""
    name = "learning (3, 32)"
    sm, sv = C.sample(pkg, name), _solver(pkg, name)
    for kw in (dict(ss_x=None, ss_j=sm["ss_j"]), dict(ss_x=sm["ss_x"], ss_j=None), dict()):
        with pytest.raises(Exception, match="needs ss_x and ss_j"):
            sv.solve_full_dynamics(sm["inp"], max_sqp=2, **kw)
    assert _same_bits(_entry(sv, sm, sm["inp"], PASSES), _trace(pkg, name)[0][PASSES]) == []


# ---- the learning chain's end -----------------------------------------------------------------------------------------------------------
def test_the_learning_chain_ends_at_first_order_points(pkg):
    """max_sqp = 60 on (10, 32).  Share converging: the twin chain (tests/sqp_cases.py run_chain with the serial twin's QPs) brings
    53 of the 65 problems to sqp_move <= 1e-8 within 60 passes; the device is held to that count less one problem."""
    name = "learning (10, 32)"
    sm, sv = C.sample(pkg, name), _solver(pkg, name)
    cfg, veh, inp = sm["cfg"], sm["veh"], sm["inp"]
    o = _entry(sv, sm, inp, 60)
    conv = (o["status"] == 0) & (o["sqp_move"] <= 1e-8)
    twin, _ = C.run_chain(sm, C.twin_qp(sm), 60)
    twin_conv = (twin["status"] == 0) & (twin["move"] <= 1e-8)
    print("learning (10, 32), 60 passes: %d of %d converge on the device, %d with the twin's QPs; QPs per converged problem: median %d, most %d"
          % (conv.sum(), conv.size, twin_conv.sum(), np.median(o["sqp_iters"][conv]), o["sqp_iters"][conv].max()))
    assert twin_conv.sum() >= 40 and conv.sum() >= twin_conv.sum() - 1
    lam = o["convex_combi_optm"]
    assert np.abs(lam.sum(axis=0) - 1.0)[conv].max() <= 1e-9 and lam[:, conv].min() >= -1e-10
    assert o["defect"][conv].max() < 1e-7
    for b in np.nonzero(conv)[0]:
        pr = dict(S.problem(inp, b), ss_x=sm["ss_x"][:, :, b], ss_j=sm["ss_j"][:, b])
        X = o["X_optm"][:, :, b]
        c = NLP.nlp_kkt_certificate(cfg, veh, pr, X, o["U_optm"][:, :, b], o["dU_optm"][:, :, b], lam=lam[:, b], eps=X[:, -1] - pr["ss_x"] @ lam[:, b])
        assert c["defect"] < 1e-7 and c["ineq"] < 1e-7 and c["stat"] < 1e-6 and c["comp"] < 1e-6, (b, c)
    # the oracle's dense SQP from the same start: three problems the twin chain brings home in 10, 20 and 9 passes
    for b in (5, 63, 64):
        assert conv[b] and twin_conv[b]
        Xo, Uo, dUo, sg, info = NLP.solve_nlp_dense(cfg, veh, S.problem(inp, b), tol=1e-8, ss_x=sm["ss_x"][:, :, b], ss_j=sm["ss_j"][:, b])
        assert info["status"] == 0, (b, info)
        assert np.abs((o["X_optm"][:, :, b] - Xo) / P.SCALE_X[:, None]).max() < 1e-5, b
        assert np.abs((o["U_optm"][:, :, b] - Uo) / P.SCALE_U[:, None]).max() < 1e-5, b
