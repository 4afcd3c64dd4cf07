"""lmpc_fleet_loop_advance_batch with a car table (include/lmpc_hip_cars.h): step 2 of the call steps car b's plant with vehicle b,
everything else keeps the handle's vehicle.  The scene, the reference and compare() are tests/test_gpu_fleet_loop.py's: one call with
a three-vehicle table is the composition it replaces with lmpc_plant_step_cars_batch in place of lmpc_plant_step_batch, held to
exactly what that file holds the call without a table to; a table with every car on one vehicle is the call with plant= that vehicle,
bit for bit; whole runs, fused against unfused; and the experiment the table is for -- half a fleet on a plant with less grip and more
mass, every car's regression learning its own car.  Needs an MI355X."""
import numpy as np
import pytest
import torch

import test_gpu_fleet_loop as FL
from test_gpu_fleet_loop import B, DT, F64, KEYS, LEARN, SPEED, T_CALL, WARM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    """The scenes are test_gpu_fleet_loop's cache: whatever this module added to it is closed here."""
    yield
    for sc in FL._scenes.values():
        for sv in (sc["tracker"], sc["learner"], sc["ref"], *sc["plants"].values()):
            sv.close()
    FL._scenes.clear()


def perturbed(pkg):
    """20 % less grip, 10 % more mass (tests/test_regression_oracle.py's perturbed plant)"""
    base = pkg.presets.barc_vehicle()
    return dict(base, mu=0.8 * base["mu"], m=1.1 * base["m"])


def three_kinds(pkg, n):
    kinds = (pkg.presets.barc_vehicle(), FL.low_mu(pkg), perturbed(pkg))
    return [kinds[b % 3] for b in range(n)]


class CarsPlant:
    """What reference() steps the plant with: the solver's plant_step_cars (close(): the scene's solvers are closed by the fixture)."""

    def __init__(self, solver):
        self.plant_step = solver.plant_step_cars

    def close(self):
        pass


# ---------------------------------------------------------------- 1. one call is the composition of what it replaces
@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("N", [20, 3])
def test_one_call_with_a_table_is_the_composition_with_plant_step_cars(pkg, N, restart):
    sc = FL.scene(pkg, N)
    learner = sc["learner"]
    learner.set_car_vehicles(three_kinds(pkg, B))
    kept = sc["plants"].pop("sv", None)
    try:
        sc["plants"]["sv"] = CarsPlant(learner)
        r = FL.reference(pkg, sc, restart, "the car table", sc["out_t"], sc["out_l"])
        # the table is in effect: the handle's vehicle moves the cars of the two other kinds elsewhere
        one = learner.plant_step(sc["trk"], sc["x"].clone(), r["u_prev"], DT / 2, 2)
        same = (one == r["x"]).all(dim=0).cpu().numpy()
        assert not same[1::3].any() and not same[2::3].any()
        ok = r["ok"].cpu().numpy()
        assert 0 < (~ok).sum() < B
        for switch in (False, True):
            got, st = FL.one_call(sc, switch, restart, None, sc["out_t"], sc["out_l"])
            FL.compare(sc, r, got, st, switch, (N, restart, "cars", switch))
    finally:
        sc["plants"].pop("sv")
        if kept is not None:
            sc["plants"]["sv"] = kept
        learner.set_car_vehicles(None)


# ---------------------------------------------------------------- 2. a table of one vehicle is plant= that vehicle
@pytest.mark.parametrize("restart", [False, True])
def test_every_car_on_low_mu_is_the_call_with_that_plant(pkg, restart):
    """Both calls run the same out-of-line plant function on the same vehicle: every output has the same bits."""
    sc = FL.scene(pkg, 20)
    learner = sc["learner"]
    want, st_w = FL.one_call(sc, True, restart, FL.low_mu(pkg), sc["out_t"], sc["out_l"])
    ring_w = FL.ring_state(learner)
    learner.set_car_vehicles([FL.low_mu(pkg)] * B)
    try:
        got, st_g = FL.one_call(sc, True, restart, None, sc["out_t"], sc["out_l"])
        ring_g = FL.ring_state(learner)
    finally:
        learner.set_car_vehicles(None)
    base, _ = FL.one_call(sc, True, restart, None, sc["out_t"], sc["out_l"])
    assert not torch.equal(base[0], want[0])          # the plant matters
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for k in KEYS:
        assert torch.equal(got[2][k], want[2][k]), k
    for a, w in zip(got[3:], want[3:]):
        assert torch.equal(a, w)
    for k in ("phase", "n_learn", "lap_time", "lap_kind", "counters", "x_ic", "query"):
        assert torch.equal(st_g[k], st_w[k]), k
    for key in ("laps_in_ring", "lap_count", "n_dropped", "last_lap_time"):
        assert np.array_equal(ring_g[key], ring_w[key]), key
    for b in range(B):
        assert len(ring_g["laps"][b]) == len(ring_w["laps"][b])
        for la, lw in zip(ring_g["laps"][b], ring_w["laps"][b]):
            assert all(np.array_equal(p, q) for p, q in zip(la, lw)), b


# ---------------------------------------------------------------- 3. refusals
def test_refusals_write_nothing(pkg):
    sc = FL.scene(pkg, 20)
    learner = sc["learner"]
    FL.prefeed(learner, sc["s0"], sc["L"])
    st = FL.fresh_state(learner)
    inp2, x2, u2 = FL.clone(sc["inp"]), sc["x"].clone(), sc["u_prev"].clone()
    nf = torch.zeros(B, dtype=torch.int64, device="cuda")
    keep = (FL.clone(inp2), x2.clone(), u2.clone(), FL.clone(st), nf.clone())
    ring0 = FL.ring_state(learner)
    args = dict(dt=DT, dt_sim=DT / 2, n_sub=2, t=T_CALL, speed_scale=SPEED, speed_limit=(6.0, 3.0), warm_laps=WARM, learn_laps=LEARN, n_fail=nf)

    def refused(**kw):
        with pytest.raises(pkg.LmpcError, match="-> -1:") as e:
            learner.fleet_loop_advance(sc["trk"], inp2, sc["out_t"], sc["out_l"], x2, u2, st, **args, **kw)
        assert len(str(e.value).split(":", 1)[1].strip()) > 0
        torch.cuda.synchronize()

    try:
        learner.set_car_vehicles(three_kinds(pkg, B))
        refused(plant=FL.low_mu(pkg))                       # a table and io->plant: two sources for the plant
        refused(plant=pkg.presets.barc_vehicle())           # (the handle's own vehicle is still a second source)
        learner.set_car_vehicles(three_kinds(pkg, B - 6))   # a table of another batch than the store's
        refused()
        learner.set_car_vehicles(three_kinds(pkg, B + 186))
        refused()
        for a, w in zip((inp2, x2, u2, st, nf), keep):
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
        learner.set_car_vehicles(three_kinds(pkg, B))
        learner.fleet_loop_advance(sc["trk"], inp2, sc["out_t"], sc["out_l"], x2, u2, st, **args)
        torch.cuda.synchronize()
        assert not torch.equal(x2, keep[1])
    finally:
        learner.set_car_vehicles(None)


# ---------------------------------------------------------------- 4. whole runs
def test_sixty_periods_equal_run_lmpc_fleet(pkg):
    tr = pkg.workloads.synthetic_track("barc")
    x0 = FL.experiment_x0(B)
    x0[:, 3:9] = x0[:, :1]                       # cars 0 and 3 .. 8 start from one state: two of each kind
    x0 = torch.as_tensor(x0, device="cuda")
    u0 = torch.zeros((2, B), **F64)
    plants = three_kinds(pkg, B)
    res = {}
    for fused in (True, False):
        tracker, learner = FL.solvers(pkg)
        fn = pkg.closed_loop.run_lmpc_fleet_fused if fused else pkg.closed_loop.run_lmpc_fleet
        res[fused] = fn(tracker, learner, tr, x0, u0, max_steps=60, plants=plants, **({"poll": 1} if fused else {}))
        torch.cuda.synchronize()
        with pytest.raises(pkg.LmpcError):       # the run cleared the table it set
            learner.car_vehicles()
        with pytest.raises(ValueError):
            fn(tracker, learner, tr, x0, u0, max_steps=1, plants=plants, plant=tracker)
        with pytest.raises(ValueError):
            fn(tracker, learner, tr, x0, u0, max_steps=1, plants=plants[:-1])
        tracker.close(), learner.close()
    a, b = res[True], res[False]
    assert a["steps"] == b["steps"] == 60
    assert torch.equal(a["n_fail"], b["n_fail"])
    sx = torch.tensor([2000.0, 10.0, 0.1, 80.0, 2.0, 2.0], **F64)[:, None]
    same = (a["n_fail"] == 0) & (b["n_fail"] == 0)
    err = float((((a["x"] - b["x"]) / sx).abs()[:, same]).max())
    print("fused vs run_lmpc_fleet with a car table, 60 periods: final states %.1e (scaled), cars without a failed solve %d of %d"
          % (err, int(same.sum()), B))
    assert int(same.sum()) > 0 and err < 1e-9
    x = a["x"]
    assert torch.equal(x[:, 0], x[:, 3]) and torch.equal(x[:, 0], x[:, 6])      # same vehicle, same x0: the same car
    assert torch.equal(x[:, 4], x[:, 7]) and torch.equal(x[:, 5], x[:, 8])
    assert not torch.equal(x[:, 3], x[:, 4]) and not torch.equal(x[:, 3], x[:, 5]) and not torch.equal(x[:, 4], x[:, 5])


# ---------------------------------------------------------------- 5. the experiment
H_REG = 0.6                 # the bandwidth of tests/test_regression_oracle.py's inequality
POINTS = 19                 # linearisation points per car: the N - 1 knots of one query


def regression_points(lap, n=POINTS):
    """n recorded samples of a lap, evenly spread, clear of its two ends (the start line): the linearisation point IS a recorded
    sample, as in tests/test_regression_oracle.py, so its own one-step residual is inside the bandwidth."""
    m = len(lap[0])
    return np.linspace(0.15 * m, 0.85 * m, n).astype(int)


def test_the_experiment_every_car_learns_its_own_car(pkg):
    """64 cars from one x0, half on the nominal plant and half on the perturbed one, each with its own safe set and regression.
    The corrections are a car's own: identical within a vehicle group, different between the groups; and for the perturbed group the
    corrected one-step prediction is closer to that car's plant than the nominal linearisation (median over cars and points).
    The same inequality is first checked on the host with oracle/regression.py on one car's recorded lap."""
    from oracle import params as P, regression as R
    from oracle.dynamics import rk4_jacobian_cs
    n = 64
    tr = pkg.workloads.synthetic_track("barc")
    x0 = torch.as_tensor(np.repeat(FL.experiment_x0(n)[:, :1], n, axis=1), device="cuda")
    u0 = torch.zeros((2, n), **F64)
    plants = [pkg.presets.barc_vehicle() if b < n // 2 else perturbed(pkg) for b in range(n)]
    tracker, learner = FL.solvers(pkg)
    res = pkg.closed_loop.run_lmpc_fleet_fused(tracker, learner, tr, x0, u0, warm_laps=1, learn_laps=1, warm_speed_scale=0.7, poll=1,
                                               regression={"dist_max": H_REG}, plants=plants)
    torch.cuda.synchronize()
    for b in range(n):
        assert res["lap_kind"][b].count("lmpc") >= 1, (b, res["lap_kind"][b])      # every car closed its learning lap
    assert int(res["n_dropped"].sum()) == 0
    laps = [learner.fleet_ss_get_laps(b) for b in (0, n - 1)]
    N = learner.N
    assert N - 1 == POINTS
    # linearisation points from each car's own last closed lap
    X, U, K, truth = np.zeros((6, N, n)), np.zeros((2, N - 1, n)), np.zeros((N, n)), np.zeros((6, N - 1, n))
    for b in range(n):
        x, u, k, _ = learner.fleet_ss_get_laps(b)[-1]
        idx = regression_points((x, u, k))
        X[:, :N - 1, b], U[:, :, b], K[:N - 1, b] = x[idx].T, u[idx].T, k[idx]
        X[:, N - 1, b], K[N - 1, b] = x[idx[-1] + 1], k[idx[-1] + 1]
        truth[:, :, b] = x[idx + 1].T                                               # what that car's plant did next
    inp = {"X_ref": torch.as_tensor(X, **F64), "U_ref": torch.as_tensor(U, **F64), "curvatures": torch.as_tensor(K, **F64),
           "T_ref": torch.full((N - 1, n), DT, **F64)}
    zero = lambda *s: torch.zeros(s, **F64)   # noqa: E731
    dA, dB, dg = learner.fleet_ss_regress(inp, zero(6, 6, N - 1, n), zero(6, 2, N - 1, n), zero(6, N - 1, n))
    A0, B0, g0 = learner.linearize(inp)
    torch.cuda.synchronize()
    half = n // 2
    for t in (dA, dB, dg):
        assert float(t.abs().max()) > 0
        for group in (slice(0, half), slice(half, n)):
            first = t[..., group][..., :1]
            assert torch.equal(t[..., group], first.expand_as(t[..., group]))       # bit-identical within a vehicle group
        assert not torch.equal(t[..., 0], t[..., n - 1])                            # and a group's own
    # the one-step prediction of the perturbed group, nominal against corrected
    Xk, Uk, Tk = inp["X_ref"][:, :N - 1], inp["U_ref"], torch.as_tensor(truth, **F64)

    def miss(A, Bm, g):
        pred = torch.einsum("rcib,cib->rib", A, Xk) + torch.einsum("rcib,cib->rib", Bm, Uk) + g
        return (pred - Tk)[3:].abs().amax(dim=0)[:, half:]                          # [points][perturbed cars]

    e0, e1 = float(miss(A0, B0, g0).median()), float(miss(A0 + dA, B0 + dB, g0 + dg).median())
    # the same on the host, first: oracle/regression.py on the last perturbed car's recorded laps, oracle linearisation
    veh = P.barc_vehicle()
    olaps = [tuple(np.asarray(a) for a in lap) for lap in laps[1]]
    x, u, k, _ = olaps[-1]
    h0, h1 = [], []
    for j in regression_points((x, u, k)):
        A, Bm, g = (a[0] for a in rk4_jacobian_cs(x[j][None], u[j][None], k[j:j + 1], np.array([DT]), veh))
        A1, B1, g1 = R.regress(veh, olaps, (3, 4, 5), (0, 1), (3, 4, 5), H_REG, x[j], u[j], A, Bm, g)
        h0.append(np.abs((A @ x[j] + Bm @ u[j] + g - x[j + 1])[3:]).max())
        h1.append(np.abs((A1 @ x[j] + B1 @ u[j] + g1 - x[j + 1])[3:]).max())
    print("one-step error of the perturbed cars, median: nominal %.3e, corrected %.3e (device, %d cars x %d points); "
          "oracle on car %d: nominal %.3e, corrected %.3e" % (e0, e1, n - half, POINTS, n - 1, np.median(h0), np.median(h1)))
    assert np.median(h1) < np.median(h0)
    assert e1 < e0
    tracker.close(), learner.close()
