"""lmpc_fleet_loop_advance_dtrack_batch (include/lmpc_hip_fleet_dtrack.h): the fused fleet LMPC period with step 2's plant the
double-track step on vehicle b of the handle's double-track table, everything else lmpc_fleet_loop_advance_batch's.  The scene, the
reference and compare() are tests/test_gpu_fleet_loop.py's.  One call is held in two parts: the plant to lmpc_plant_step_dtrack_batch
within that entry point's own bound (the out-of-line step of the fused kernel and the stand-alone kernel are compiled apart and need
not contract alike), and everything else bit for bit, by the reference run with a plant hook that hands back the state the fused
call produced.  Then: gamma_y does not perturb, the head-only call, the plain entry point still ignores the table, refusals, whole
runs fused against unfused with a replay of every period, and the warm-up into the fused loop.  Needs an MI355X."""
import numpy as np
import pytest
import torch

import test_gpu_fleet_loop as FL
import vanilla_fleet_cases as FC
from test_gpu_fleet_loop import B, DT, F64, KEYS, LEARN, SPEED, T_CALL, WARM

pytestmark = pytest.mark.gpu

EULER = (7, 12)             # the two cars of the table that integrate with Euler (the cars of vanilla_fleet_cases' car fleet)
STATE = ("phase", "n_learn", "lap_time", "lap_kind", "counters", "x_ic", "query")


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    """The scenes are test_gpu_fleet_loop's cache: whatever this module added to it is closed here."""
    yield
    for sc in FL._scenes.values():
        for sv in (sc["tracker"], sc["learner"], sc["ref"], *sc["plants"].values()):
            sv.close()
    FL._scenes.clear()


def table(pkg, n):
    """Car b's four-wheel vehicle by b % 3 (vanilla_fleet_cases.dtrack_vehicles), cars 7 and 12 on Euler."""
    veh = FC.dtrack_vehicles(pkg, n)
    return [dict(v, integrator="euler") if b in EULER else v for b, v in enumerate(veh)]


def plant_bound(want):
    """tests/test_gpu_plant_dtrack.py's bound for this plant step."""
    return 1e-11 * max(1.0, float(want.abs().max()))


class GivenPlant:
    """What reference() steps the plant with: the state the fused call produced (close(): nothing to close)."""

    def __init__(self, x):
        self.x = x

    def plant_step(self, trk, x, u, dt_sim, n_sub):
        return self.x.clone()

    def close(self):
        pass


def one_call_dt(sc, switch, restart, out_t, out_l, head_only=False, gamma=None):
    """test_gpu_fleet_loop.one_call through the double-track entry point."""
    FL.prefeed(sc["learner"], sc["s0"], sc["L"])
    st = FL.fresh_state(sc["learner"])
    inp2, x2, u2 = FL.clone(sc["inp"]), sc["x"].clone(), sc["u_prev"].clone()
    dist, exc, nf = torch.zeros(B, **F64), torch.zeros(B, **F64), torch.zeros(B, dtype=torch.int64, device="cuda")
    if head_only:
        FL.advance(sc, st, x2, u2, inp2, None, None, switch_phase=switch, restart_failed=restart, dtrack=True, gamma_y=gamma)
    else:
        FL.advance(sc, st, x2, u2, inp2, out_t, out_l, switch_phase=switch, restart_failed=restart, distance=dist, worst_excess=exc, n_fail=nf,
                   dtrack=True, gamma_y=gamma)
    torch.cuda.synchronize()
    return (x2, u2, inp2, dist, exc, nf), st


def assert_same_bits(a, b, what):
    """Two (one_call result, state, ring_state) triples: every output torch.equal, the rings array_equal."""
    (got, st_g, ring_g), (want, st_w, ring_w) = a, b
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), what
    for k in KEYS:
        assert torch.equal(got[2][k], want[2][k]), (what, k)
    for g, w in zip(got[3:], want[3:]):
        assert torch.equal(g, w), what
    for k in STATE:
        assert torch.equal(st_g[k], st_w[k]), (what, k)
    for key in ("laps_in_ring", "lap_count", "n_dropped", "last_lap_time"):
        assert np.array_equal(ring_g[key], ring_w[key]), (what, key)
    for b_ in range(B):
        assert len(ring_g["laps"][b_]) == len(ring_w["laps"][b_]), (what, b_)
        for la, lw in zip(ring_g["laps"][b_], ring_w["laps"][b_]):
            assert all(np.array_equal(p, q) for p, q in zip(la, lw)), (what, b_)


def with_ring(sc, result):
    got, st = result
    return got, st, FL.ring_state(sc["learner"])


# ---------------------------------------------------------------- 1. one call is the composition of what it replaces
@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("N", [20, 3])
def test_one_call_is_the_composition_with_plant_step_dtrack(pkg, N, restart):
    sc = FL.scene(pkg, N)
    learner = sc["learner"]
    learner.set_dtrack_vehicles(table(pkg, B))
    kept = sc["plants"].pop("sv", None)
    try:
        gamma = torch.full((B,), float("nan"), **F64)
        first, _ = one_call_dt(sc, True, restart, sc["out_t"], sc["out_l"], gamma=gamma)
        x_fused = first[0].clone()
        # (b) everything else, bit for bit: the reference with the plant handing back the fused call's state
        sc["plants"]["sv"] = GivenPlant(x_fused)
        r = FL.reference(pkg, sc, restart, "the double-track table", sc["out_t"], sc["out_l"])
        ok = r["ok"].cpu().numpy()
        assert 0 < (~ok).sum() < B
        # (a) the plant: lmpc_plant_step_dtrack_batch on the input the composition applies
        gamma_want = torch.zeros(B, **F64)
        want = learner.plant_step_dtrack(sc["trk"], sc["x"].clone(), r["u_prev"], DT / 2, 2, gamma_y=gamma_want)
        torch.cuda.synchronize()
        err, bound = float((x_fused - want).abs().max()), plant_bound(want)
        gerr = float(((gamma - gamma_want).abs() / torch.clamp(gamma_want.abs(), min=1.0)).max())
        print("N = %d restart = %s: max |fused x - plant_step_dtrack| = %.3e (bound %.3e), %d of %d values bit-identical; gamma_y: "
              "max |d| / max(1, |gamma_y|) = %.3e, %d of %d bit-identical, max |gamma_y| = %.3e"
              % (N, restart, err, bound, int((x_fused == want).sum()), want.numel(), gerr, int((gamma == gamma_want).sum()), B,
                 float(gamma_want.abs().max())))
        assert bool(torch.isfinite(x_fused).all()) and bool(torch.isfinite(gamma).all())
        assert bool(((x_fused - want).abs() <= bound).all())
        assert bool(((gamma - gamma_want).abs() <= 1e-11 * torch.clamp(gamma_want.abs(), min=1.0)).all())
        # the table is in effect: the plain call moves every car elsewhere
        plain, _ = FL.one_call(sc, True, restart, None, sc["out_t"], sc["out_l"])
        assert bool((plain[0] != x_fused).any(dim=0).all())
        for switch in (False, True):
            got, st = one_call_dt(sc, switch, restart, sc["out_t"], sc["out_l"])
            FL.compare(sc, r, got, st, switch, (N, restart, "dtrack", switch))
    finally:
        sc["plants"].pop("sv", None)
        if kept is not None:
            sc["plants"]["sv"] = kept
        learner.set_dtrack_vehicles(None)


# ---------------------------------------------------------------- 2. gamma_y does not perturb
def test_gamma_y_does_not_perturb(pkg):
    sc = FL.scene(pkg, 20)
    learner = sc["learner"]
    learner.set_dtrack_vehicles(table(pkg, B))
    try:
        gamma = torch.full((B,), float("nan"), **F64)
        with_g = with_ring(sc, one_call_dt(sc, True, True, sc["out_t"], sc["out_l"], gamma=gamma))
        without = with_ring(sc, one_call_dt(sc, True, True, sc["out_t"], sc["out_l"]))
        assert bool(torch.isfinite(gamma).all()) and float(gamma.abs().max()) > 0
        assert_same_bits(with_g, without, "gamma_y")
    finally:
        learner.set_dtrack_vehicles(None)


# ---------------------------------------------------------------- 3. head-only
def test_head_only_is_the_plain_head_only_call(pkg):
    sc = FL.scene(pkg, 20)
    learner = sc["learner"]
    want = with_ring(sc, FL.one_call(sc, True, False, None, None, None, head_only=True))
    learner.set_dtrack_vehicles(table(pkg, B))
    try:
        gamma = torch.full((B,), -7.0, **F64)
        got = with_ring(sc, one_call_dt(sc, True, False, None, None, head_only=True, gamma=gamma))
        assert_same_bits(got, want, "head only")
        assert bool((gamma == -7.0).all())                  # no plant: gamma_y is not written
        assert torch.equal(got[0][0], sc["x"])
    finally:
        learner.set_dtrack_vehicles(None)


# ---------------------------------------------------------------- 4. the plain entry point still ignores the table
def test_the_plain_entry_point_ignores_the_table(pkg):
    sc = FL.scene(pkg, 20)
    learner = sc["learner"]
    want = with_ring(sc, FL.one_call(sc, True, True, None, sc["out_t"], sc["out_l"]))
    learner.set_dtrack_vehicles(table(pkg, B))
    try:
        got = with_ring(sc, FL.one_call(sc, True, True, None, sc["out_t"], sc["out_l"]))
        assert_same_bits(got, want, "plain call, table set")
        low = with_ring(sc, FL.one_call(sc, True, True, FL.low_mu(pkg), sc["out_t"], sc["out_l"]))     # plant= is still its own source
    finally:
        learner.set_dtrack_vehicles(None)
    assert_same_bits(low, with_ring(sc, FL.one_call(sc, True, True, FL.low_mu(pkg), sc["out_t"], sc["out_l"])), "plain call with plant=, table set")


# ---------------------------------------------------------------- 5. refusals
def test_refusals_write_nothing(pkg):
    sc = FL.scene(pkg, 20)
    learner = sc["learner"]
    FL.prefeed(learner, sc["s0"], sc["L"])
    st = FL.fresh_state(learner)
    inp2, x2, u2 = FL.clone(sc["inp"]), sc["x"].clone(), sc["u_prev"].clone()
    nf = torch.zeros(B, dtype=torch.int64, device="cuda")
    gamma = torch.full((B,), -7.0, **F64)
    keep = (FL.clone(inp2), x2.clone(), u2.clone(), FL.clone(st), nf.clone(), gamma.clone())
    ring0 = FL.ring_state(learner)
    args = dict(dt=DT, dt_sim=DT / 2, n_sub=2, t=T_CALL, speed_scale=SPEED, speed_limit=(6.0, 3.0), warm_laps=WARM, learn_laps=LEARN, n_fail=nf,
                dtrack=True, gamma_y=gamma)

    def refused(**kw):
        with pytest.raises(pkg.LmpcError, match="-> -1:") as e:
            learner.fleet_loop_advance(sc["trk"], inp2, sc["out_t"], sc["out_l"], x2, u2, st, **args, **kw)
        assert "lmpc_fleet_loop_advance_dtrack_batch" in str(e.value)
        assert len(str(e.value).split(":", 1)[1].strip()) > 0
        torch.cuda.synchronize()

    try:
        refused()                                               # no table
        learner.set_dtrack_vehicles(table(pkg, B - 6))          # tables of another batch than the store's
        refused()
        learner.set_dtrack_vehicles(table(pkg, B + 186))
        refused()
        learner.set_dtrack_vehicles(table(pkg, B))
        refused(plant=FL.low_mu(pkg))                           # io->plant: a second source for the plant
        refused(plant=pkg.presets.barc_vehicle())
        learner.set_car_vehicles([pkg.presets.barc_vehicle()] * B)
        try:
            refused()                                           # a car table set as well
        finally:
            learner.set_car_vehicles(None)
        for a, w in zip((inp2, x2, u2, st, nf, gamma), keep):
            if isinstance(a, dict):
                assert all(torch.equal(a[k], w[k]) for k in a if torch.is_tensor(a[k]))
            else:
                assert torch.equal(a, w)
        ring1 = FL.ring_state(learner)
        for key in ("laps_in_ring", "lap_count", "n_dropped", "last_lap_time"):
            assert np.array_equal(ring0[key], ring1[key]), key
        assert all(len(a) == len(w) and all(all(np.array_equal(p, q) for p, q in zip(la, lw)) for la, lw in zip(a, w))
                   for a, w in zip(ring1["laps"], ring0["laps"]))
        # and the same arguments with a table of the store's batch go through
        learner.fleet_loop_advance(sc["trk"], inp2, sc["out_t"], sc["out_l"], x2, u2, st, **args)
        torch.cuda.synchronize()
        assert bool((x2 != keep[1]).any(dim=0).all()) and bool((gamma != -7.0).all())
    finally:
        learner.set_car_vehicles(None)
        learner.set_dtrack_vehicles(None)


# ---------------------------------------------------------------- 6. whole runs, fused against unfused
def _sixty_periods(pkg):
    n, periods = 9, 60
    tr = pkg.workloads.synthetic_track("barc")
    x0 = FL.experiment_x0(n)
    x0[:, 3:9] = x0[:, :1]                       # cars 0 and 3 .. 8 start from one state: two (kind 0: three) of each kind
    x0 = torch.as_tensor(x0, device="cuda")
    u0 = torch.zeros((2, n), **F64)
    plants_dt = FC.dtrack_vehicles(pkg, n)
    res = {}
    for fused in (True, False):
        tracker, learner = FL.solvers(pkg)
        fn = pkg.closed_loop.run_lmpc_fleet_fused if fused else pkg.closed_loop.run_lmpc_fleet
        res[fused] = fn(tracker, learner, tr, x0, u0, max_steps=periods, plants_dt=plants_dt, record_trace=True, **({"poll": 1} if fused else {}))
        torch.cuda.synchronize()
        with pytest.raises(pkg.LmpcError):       # the run cleared the table it set
            learner.get_dtrack_vehicles()
        if fused:
            with pytest.raises(ValueError):
                fn(tracker, learner, tr, x0, u0, max_steps=1, plants_dt=plants_dt, plants=[pkg.presets.barc_vehicle()] * n)
            with pytest.raises(ValueError):
                fn(tracker, learner, tr, x0, u0, max_steps=1, plants_dt=plants_dt, plant=tracker)
            with pytest.raises(ValueError):
                fn(tracker, learner, tr, x0, u0, max_steps=1, plants_dt=plants_dt[:-1])
            with pytest.raises(pkg.LmpcError):   # (a refused run set no table either)
                learner.get_dtrack_vehicles()
        tracker.close(), learner.close()
    return tr, plants_dt, res


def test_sixty_periods_equal_run_lmpc_fleet(pkg):
    """9 four-wheel cars, 60 periods, poll = 1: run_lmpc_fleet_fused(plants_dt=) against run_lmpc_fleet(plants_dt=).  The final states
    are held to the bound tests/test_gpu_fleet_loop_cars.py::test_sixty_periods_equal_run_lmpc_fleet holds the car-table runs to,
    1e-9 in its scaling; here the two plants differ by rounding each period where the car-table ones do not.  The measured value
    is printed, and recorded in profiles/fleet_dtrack_fused.md beside the car-table test's."""
    n, periods = 9, 60
    tr, plants_dt, res = _sixty_periods(pkg)
    a, b = res[True], res[False]
    assert a["steps"] == b["steps"] == periods
    assert torch.equal(a["n_fail"], b["n_fail"])
    # the replay: the cars the fused period moved are the four-wheel cars of the table, period after period
    replay = pkg.Solver(pkg.presets.barc_lmpc(20, 3), pkg.presets.barc_vehicle(), device=0)
    replay.set_dtrack_vehicles(plants_dt)
    trk = replay.device_track(tr)
    trace = a["trace"]
    assert len(trace) == periods + 1
    worst = 0.0
    for p in range(periods):
        want = replay.plant_step_dtrack(trk, trace[p][0].clone(), trace[p + 1][1].contiguous(), DT / 2, 2)
        d = (trace[p + 1][0] - want).abs()
        worst = max(worst, float(d.max()) / plant_bound(want))
        assert bool((d <= plant_bound(want)).all()), (p, float(d.max()), plant_bound(want))
    replay.close()
    x = a["x"]
    assert torch.equal(x[:, 0], x[:, 3]) and torch.equal(x[:, 0], x[:, 6])      # same vehicle, same x0: the same car
    assert torch.equal(x[:, 4], x[:, 7]) and torch.equal(x[:, 5], x[:, 8])
    assert not torch.equal(x[:, 3], x[:, 4]) and not torch.equal(x[:, 3], x[:, 5]) and not torch.equal(x[:, 4], x[:, 5])
    sx = torch.tensor([2000.0, 10.0, 0.1, 80.0, 2.0, 2.0], **F64)[:, None]
    same = (a["n_fail"] == 0) & (b["n_fail"] == 0)
    err = float((((a["x"] - b["x"]) / sx).abs()[:, same]).max())
    print("fused vs run_lmpc_fleet on four-wheel cars, 60 periods: final states %.1e (scaled), cars without a failed solve %d of %d; "
          "replay of the fused run's periods: worst |d| / bound %.2e" % (err, int(same.sum()), n, worst))
    assert int(same.sum()) > 0 and err < 1e-9


# ---------------------------------------------------------------- 7. the warm-up into the fused loop
def test_warm_up_into_the_fused_loop(pkg):
    """8 four-wheel cars: the warm laps by the vanilla controller on the double-track table, the head-only call, 40 fused periods."""
    import test_gpu_vanilla_fleet as VF
    n = 8
    sc, tracker, learner, asked, warmup = VF.experiment(pkg, n)
    x0 = torch.as_tensor(np.ascontiguousarray(sc["x0"].T), device="cuda")
    u0 = torch.zeros((2, n), **F64)
    res = pkg.closed_loop.run_lmpc_fleet_fused(tracker, learner, sc["trk"]["table"], x0, u0, warm_laps=2, learn_laps=1, dt=sc["dt"], n_sub=sc["n_sub"],
                                               max_steps=40, plants_dt=FC.dtrack_vehicles(pkg, n), warmup=warmup)
    torch.cuda.synchronize()
    assert "warmup" in res
    w = res["warmup"]
    count = learner.fleet_ss_stats(n)["lap_count"].cpu().numpy()
    print("warm-up %d periods on four-wheel cars; %d fused periods: lap_count %s (after the warm-up %s), n_fail %s, worst_excess %.4f"
          % (w["periods"], res["steps"], count.tolist(), w["lap_count"].tolist(), res["n_fail"].cpu().numpy().tolist(), float(res["worst_excess"].max())))
    assert res["steps"] <= 40 and w["periods"] > 0
    assert np.isfinite(res["x"].cpu().numpy()).all() and np.isfinite(res["worst_excess"].cpu().numpy()).all()
    assert (count >= w["lap_count"]).all()
    with pytest.raises(pkg.LmpcError):           # the run cleared the table it set
        learner.get_dtrack_vehicles()
    tracker.close(), learner.close()
