"""Every entry point held to its stream contract (include/lmpc_hip.h) on a stream that is not the null stream and is held by a gate.

Every other GPU test runs on torch's default stream, which is the device's null stream: a launch, memset or copy issued on stream 0
instead of the handle's, a hidden synchronisation, a helper that drops its stream argument are all invisible there.  Here each row
of tests/stream_cases.py runs twice: on the default stream (the reference), and on a fresh non-blocking stream behind a finite delay,
with another valid draw in the input buffers until the stream itself copies the real inputs in.  The results must be the
reference's bit for bit; an asynchronous entry point must have returned while the gate still held the stream; one whose comment says
that it synchronises the handle's stream must not have.

The gate: 10 times the slowest ungated host-side duration of an asynchronous row's call, 20 ms at least (the factor is for the
host's scheduling jitter).  Both numbers are printed by test_rows_are_built_and_the_gate_is_measured.  MEASURED on an MI355X, six
runs: the slowest ungated host time of an asynchronous call is 0.04 .. 0.29 ms (a solve through the ctypes binding: two to five
launches), ten times that is 3 ms at most, so the 20 ms floor is the gate -- torch.cuda._sleep at 2.6e6 counts per ms once
tuned at that length (the 10 ms calibration run alone gave 2.0e6 and a gate of 16.7 ms), 22.0 ms measured alone on a stream.  The
slowest blocking calls, for scale: fleet_ss_get_laps of 70 cars 8 ms, solve_full_dynamics 1.6 ms, solve_host 0.3 ms.

Then the benchmark's own configuration (three handles on three streams, rounds enqueued without a host synchronisation), one handle
moved between two streams by a caller who orders them, and one period of the fused fleet loop captured as a graph and replayed.
Needs an MI355X."""
import traceback

import numpy as np
import pytest
import torch

import stream_cases as SC

pytestmark = pytest.mark.gpu

GROUPS = tuple(SC.BUILDERS)
_built = {}       # group -> {row: Case}
_refs = {}        # row -> (want, host seconds of the ungated call)
_shared = {}
_errors = {}      # group -> traceback of a builder or reference run that raised


@pytest.fixture(scope="module")
def fleet_scene(pkg):
    """test_gpu_fleet_loop.py's scene at N = 20 for this module: the fleet rows and the graph test work on it, and its Solvers are
    closed when the module is done (that module's own fixture does the same for its tests)."""
    import test_gpu_fleet_loop as FL

    yield FL.scene(pkg, 20)
    for sc in FL._scenes.values():
        for sv in (sc["tracker"], sc["learner"], sc["ref"], *sc["plants"].values()):
            sv.close()
    FL._scenes.clear()


@pytest.fixture(scope="module")
def rows(pkg, fleet_scene):
    """Every row built and its reference run made (step a), so that the gate can be sized by the slowest asynchronous call."""
    for group in GROUPS:
        try:   # (a group that cannot be built fails its own rows, with its own traceback, and the others still run)
            _built[group] = SC.build(pkg, group)
            for row, case in _built[group].items():
                _refs[row] = SC.reference(case)
        except Exception:
            _errors[group] = traceback.format_exc()
    gate = SC.Gate()
    slow_row, slow = max(((r, sec) for r, (_, sec) in _refs.items() if SC.row_class(r)[0] == SC.ASYNC), key=lambda p: p[1])
    gate_ms = max(SC.GATE_FACTOR * slow * 1e3, SC.GATE_FLOOR_MS)
    _shared.update(gate=gate, gate_ms=gate_ms, slow_row=slow_row, slow_ms=slow * 1e3, measured_ms=gate.tune(gate_ms))
    yield _shared
    _built.clear()
    _refs.clear()


def test_rows_are_built_and_the_gate_is_measured(rows):
    g = rows["gate"]
    print("gate: %s, %.3g units per ms (calibration run %.2f ms); slowest ungated host time of an asynchronous call %.3f ms (%s); "
          "gate %.1f ms asked, %.1f ms measured alone" % (g.kind, g.per_ms, g.calibration_ms, rows["slow_ms"], rows["slow_row"], rows["gate_ms"],
                                                           rows["measured_ms"]))
    for r, (_, sec) in sorted(_refs.items(), key=lambda p: -p[1][1])[:8]:
        print("    %-40s %-9s %.3f ms" % (r, SC.row_class(r)[0], sec * 1e3))
    assert not _errors, "\n".join(_errors.values())
    assert {r for grp in _built.values() for r in grp} == set(SC.ROWS)
    # the gate is a gate: alone on a stream it lasts what was asked of it, give or take the calibration
    assert rows["measured_ms"] >= rows["gate_ms"] >= SC.GATE_FLOOR_MS, (rows["measured_ms"], rows["gate_ms"])


SAME_ON_STALE = {"fleet_ss_reset"}


@pytest.mark.parametrize("row", list(SC.ROWS))
def test_row_on_a_gated_stream(rows, row):
    if SC.ROWS[row][0] in _errors:
        pytest.fail(_errors[SC.ROWS[row][0]], pytrace=False)
    case = _built[SC.ROWS[row][0]][row]
    want, _ = _refs[row]
    got, closed = SC.gated(case, rows["gate"], rows["gate_ms"])
    diff = SC.differences(got, want)
    assert not diff, (row, "differs from the default-stream run in", diff)
    if case.cls == SC.ASYNC:
        assert closed, (row, "returned after the gate had opened: a synchronisation the header denies (or a host call slower than the gate)")
    elif case.sync:
        assert not closed, (row, "returned while the gate still held the stream it says it waits for")
    if "accepted" in case.outs:
        print(" [%d of %d warm starts accepted]" % (int(want["out accepted"].sum()), want["out accepted"].numel()), end="")
        assert int(want["out accepted"].sum()) > 0, (row, "no warm start was accepted: the short route did not run")
    # the equality is not vacuous: the other filling of the buffers gives another result (a row listed in SAME_ON_STALE checks an
    # ORDER on the stream -- its end state does not depend on the data)
    if case.bufs and row not in SAME_ON_STALE:
        assert SC.differences(SC.reference(case, "stale")[0], want), (row, "`stale` gives the result of `real`: the row would prove nothing")


def test_detector_control_sees_a_call_on_the_wrong_stream(rows):
    """The same run with the call made under a second stream T while S is gated: the handle really is on the wrong stream.  The
    sample then reads `stale` (S has not copied `real` in yet): the result is not the reference's, and is the reference on `stale`;
    with the stream's own sentinel fill behind the gate, as every row runs, it is wiped and the sentinel is what is left."""
    case = _built["track"]["track_sample"]
    want, _ = _refs["track_sample"]
    want_stale, _ = SC.reference(case, "stale")
    assert SC.differences(want_stale, want), "the two draws give the same result: the control would prove nothing"
    got, _ = SC.gated(case, rows["gate"], rows["gate_ms"], call_stream=torch.cuda.Stream(), wipe=False)
    assert SC.differences(got, want) == ["out out"], "a call on the wrong stream went unnoticed"
    assert not SC.differences(got, want_stale)
    got, _ = SC.gated(case, rows["gate"], rows["gate_ms"], call_stream=torch.cuda.Stream())
    assert SC.differences(got, want) == ["out out"] and bool((got["out out"] == SC.SENTINEL_F).all())


@pytest.mark.parametrize("row", ["fleet_ss_reset", "vanilla_reset"])
def test_a_reset_issued_from_another_stream_is_seen(rows, row):
    """The rows whose end state does not depend on the data check an ORDER: the reset behind a launch on the same stream.  With the
    reset alone issued under a second stream -- its memsets then run while the gate holds the launch -- the state read back is not
    the reference's: the sample, or the decision, that should have been wiped has survived."""
    case = _built[SC.ROWS[row][0]][row]
    got, _ = SC.gated(case, rows["gate"], rows["gate_ms"], call_stream=torch.cuda.Stream())
    diff = SC.differences(got, _refs[row][0])
    print(" [differs in %s]" % diff, end="")
    assert diff, (row, "a reset that left the stream went unnoticed")


# ---- several handles, several streams: the benchmark's configuration -------------------------------------------------------------------
B_MULTI, ROUNDS = 256, 6
OUT_KEYS = ("X_optm", "U_optm", "dU_optm", "status", "iters", "kkt")


def _multi_setup(pkg, kind):
    tr = pkg.workloads.synthetic_track("barc")
    L = float(tr["L"])
    learning = kind != "tracking"
    cfg = dict(pkg.presets.barc_lmpc(20, 2)) if learning else pkg.presets.barc_tracking_mpc(20)
    laps = pkg.workloads.synthetic_laps(tr, 2) if learning else None
    solvers, jobs = [], []
    for i in range(3):
        s = pkg.Solver(cfg, pkg.presets.barc_vehicle(), device=0)
        s.reserve(B_MULTI)
        if learning:
            s.set_safe_set(laps, L)
        base = SC._cold_inputs(pkg, s, s.device_track(tr), L, 60 + i, n=B_MULTI, near=laps)
        rng = np.random.default_rng(70 + i)
        per_round = []
        for _ in range(ROUNDS):   # its own inputs per (stream, round): x_ic perturbed, everything else the handle's cold start
            inp = dict(SC.like(base), L=L)
            inp["x_ic"] += SC.dev(rng.normal(0, 1, (6, B_MULTI)) * np.array([0.0, 0.01, 0.01, 0.03, 0.01, 0.03])[:, None])
            kw = {}
            if learning:
                kw["ss_idx"] = s.ss_query_idx(SC.query_point(inp["X_ref"], inp["x_ic"], L))[0]
                kw["mixed"] = kind == "mixed"
            per_round.append((inp, kw))
        solvers.append(s)
        jobs.append(per_round)
    return solvers, jobs, (int(cfg["num_ss_pts"]) if learning else 0)


@pytest.mark.parametrize("kind", ["tracking", "learning by ss_idx", "mixed"])
def test_three_handles_on_three_streams_give_each_solve_its_own_answer(pkg, kind):
    """bench.py's configuration: three Solvers on three non-blocking streams, six rounds enqueued round-robin with no host
    synchronisation in between, every (stream, round) with its own inputs and outputs.  Every output equals, bit for bit, what the
    same solver returns for those inputs alone and synchronised."""
    solvers, jobs, S = _multi_setup(pkg, kind)
    outs = lambda s: SC._solve_outs(s, B_MULTI, lam=S)   # noqa: E731
    alone = [[None] * ROUNDS for _ in solvers]
    for i, s in enumerate(solvers):
        for r, (inp, kw) in enumerate(jobs[i]):
            alone[i][r] = s.solve(inp, outs(s), **kw)
            torch.cuda.synchronize()
    together = [[outs(s) for _ in range(ROUNDS)] for s in solvers]
    for grid in together:
        for o in grid:
            for k in OUT_KEYS + (("convex_combi_optm",) if S else ()):
                o[k].fill_(SC.SENTINEL_F if o[k].is_floating_point() else SC.SENTINEL_I)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in solvers]
    assert len({st.cuda_stream for st in streams}) == 3 and 0 not in {st.cuda_stream for st in streams}
    for r in range(ROUNDS):
        for i, s in enumerate(solvers):
            with torch.cuda.stream(streams[i]):
                inp, kw = jobs[i][r]
                s.solve(inp, together[i][r], **kw)
    torch.cuda.synchronize()
    solved = 0
    for i in range(3):
        for r in range(ROUNDS):
            for k in OUT_KEYS + (("convex_combi_optm",) if S else ()):
                assert SC.bits_equal(together[i][r][k], alone[i][r][k]), (kind, "handle", i, "round", r, k)
            solved += int((alone[i][r]["status"] == 0).sum())
    assert solved > 0.5 * 3 * ROUNDS * B_MULTI, solved      # most problems solve: the comparison is of answers, not of failures
    assert not SC.bits_equal(alone[0][0]["X_optm"], alone[0][1]["X_optm"])   # the rounds differ
    for s in solvers:
        s.close()


def test_one_handle_moves_between_two_streams_when_the_caller_orders_them(pkg):
    """prepare on A, solve on B behind A, shift and plant step on A behind B: the single-stream result.  The handle holds no state
    tied to a stream; ordering two streams is the caller's (include/lmpc_hip.h, lmpc_set_stream)."""
    tr = pkg.workloads.synthetic_track("barc")
    L = float(tr["L"])
    s = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    trk = s.device_track(tr)
    x, u = pkg.workloads.sample_initial_states("barc", SC.B, L, [-0.01, -0.3], [0.01, 0.3], seed=80)
    x0, u0 = SC.dev(x.T.copy()), SC.dev(u.T.copy())
    torch.cuda.synchronize()

    def period(on_prepare, on_solve, between):
        with torch.cuda.stream(on_prepare):
            inp = s.prepare(trk, x0, SC.DT, speed_scale=0.9)
            inp["u_ic"] = u0
        between(on_solve, on_prepare)
        with torch.cuda.stream(on_solve):
            out = s.solve(inp)
        between(on_prepare, on_solve)
        with torch.cuda.stream(on_prepare):
            nxt = s.shift(trk, inp, out, SC.DT, speed_scale=0.9)
            xn = s.plant_step(trk, x0.clone(), out["U_optm"][:, 0, :].contiguous(), SC.DT / 2, 2)
        torch.cuda.synchronize()
        res = {k: out[k] for k in OUT_KEYS}
        res.update({"next " + k: nxt[k] for k in SC.REF7}, x=xn)
        return res

    one = torch.cuda.Stream()
    want = period(one, one, lambda later, earlier: None)
    got = period(torch.cuda.Stream(), torch.cuda.Stream(), lambda later, earlier: later.wait_stream(earlier))
    for k in want:
        assert SC.bits_equal(got[k], want[k]), k
    s.close()


# ---- "legal inside a captured control period": the fused fleet period -------------------------------------------------------------------
def test_fleet_period_replays_from_a_graph(pkg, fleet_scene):
    """One period of closed_loop.run_lmpc_fleet_fused between two polls -- the fleet query, both controllers' solves,
    lmpc_fleet_loop_advance_batch -- captured on one stream after a warm-up period on a side stream (closed_loop.run's pattern: nothing
    allocates inside the capture) and replayed three times: states, references, rings and lap book are those of the same four periods
    run eagerly.  The time stamp of the recorded sample is a launch argument, so a replay records the captured one; the eager twin
    is given the same."""
    import test_gpu_fleet_loop as FL

    sc = fleet_scene
    tracker, learner, trk, L, n = sc["tracker"], sc["learner"], sc["trk"], sc["L"], FL.B
    S = int(learner.config["num_ss_pts"])

    def fresh():
        FL.prefeed(learner, sc["s0"], L)
        w = dict(x=sc["x"].clone(), u_prev=sc["u_prev"].clone(), inp=dict(FL.clone(sc["inp"])), st=FL.fresh_state(learner),
                 out_t=tracker.alloc_outputs(n), out_l=learner.alloc_outputs(n),
                 ss=(torch.zeros((6, S, n), **FL.F64), torch.zeros((S, n), **FL.F64), torch.zeros(n, dtype=torch.int32, device="cuda")),
                 worst=torch.zeros(n, **FL.F64), n_fail=torch.zeros(n, dtype=torch.int64, device="cuda"))
        w["out_l"]["convex_combi_optm"] = torch.zeros((S, n), **FL.F64)
        w["kw"] = dict(dt=FL.DT, dt_sim=FL.DT / 2, n_sub=2, speed_scale=FL.SPEED, speed_limit=(6.0, 3.0), restart_failed=False, warm_laps=FL.WARM,
                       learn_laps=FL.LEARN, worst_excess=w["worst"], n_fail=w["n_fail"])
        # period 0: the head-only call -- x_ic and the query on the prepared references
        learner.fleet_loop_advance(trk, w["inp"], None, None, w["x"], w["u_prev"], w["st"], t=0.0, switch_phase=False, **w["kw"])
        torch.cuda.synchronize()
        return w

    def period(w):   # both phases have cars (test_gpu_fleet_loop.py PHASE0) and no phase switches between two polls
        w["inp"]["x_ic"], w["inp"]["u_ic"] = w["st"]["x_ic"], w["u_prev"]
        ss_x, ss_j, _ = learner.fleet_ss_query(w["st"]["query"], out=w["ss"])
        learner.solve(w["inp"], w["out_l"], ss_x=ss_x, ss_j=ss_j)
        tracker.solve(w["inp"], w["out_t"])
        learner.fleet_loop_advance(trk, w["inp"], w["out_t"], w["out_l"], w["x"], w["u_prev"], w["st"], t=FL.T_CALL, switch_phase=False, **w["kw"])

    def result(w):
        torch.cuda.synchronize()
        r = {k: w[k].clone() for k in ("x", "u_prev", "worst", "n_fail")}
        r.update({"ref " + k: w["inp"][k].clone() for k in FL.KEYS}, **{"book " + k: v.clone() for k, v in w["st"].items()})
        return r, FL.ring_state(learner)

    eager = fresh()
    for _ in range(4):
        period(eager)
    want, want_ring = result(eager)

    w = fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        period(w)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        period(w)
    for _ in range(3):
        g.replay()
    got, got_ring = result(w)
    assert int((want["book phase"] == 1).sum()) not in (0, n) and float((want["x"] - sc["x"]).abs().max()) > 0
    for k in want:
        assert SC.bits_equal(got[k], want[k]), k
    FL.assert_rings(got_ring, want_ring, "graph replay")
