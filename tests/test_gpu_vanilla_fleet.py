"""lmpc_vanilla_rollout_fleet_batch on the device (include/lmpc_hip_vanilla_fleet.h): the vanilla rollout with a plant per car and the
fleet recorder inside the period loop, against lmpc_vanilla_rollout_batch (bit for bit on the handle's plant), the numpy restatement
of tests/vanilla_fleet_cases.py, the unfused device composition (one decision and one plant step per period), and a replay of its
own logs through lmpc_fleet_ss_record_batch (bit for bit, both recording conventions); and closed_loop's warm-up of the fleet LMPC
experiment.  On the rigs of tests/test_gpu_vanilla.py; every scenario is one tests/test_vanilla_fleet_reference.py has qualified.

Tolerances, elementwise |d| / max(1, |reference|): vanilla_cases.TOL_ROLLOUT = 1e-8 for the single-track plants and
vanilla_fleet_cases.TOL_DTRACK = 1e-9 for the four-wheel plant, each 1e4 times a drift measured on the CPU over the same 64 periods
and 67 cars."""
import numpy as np
import pytest

import test_gpu_vanilla as TV
import vanilla_cases as VC
import vanilla_fleet_cases as FC

pytestmark = pytest.mark.gpu

B = VC.B_TEST
dev, host, pid_of, Rig = TV.dev, TV.host, TV.pid_of, TV.Rig
STATS = ("laps_in_ring", "lap_count", "n_dropped", "last_lap_time")


@pytest.fixture(scope="module")
def rigs(pkg):
    made = {}

    def get(name, n=B, which=0):
        if (name, n, which) not in made:
            made[(name, n, which)] = Rig(pkg, VC.scenario(name, n))
        return made[(name, n, which)]

    return get


def set_table(rig, plant, mixed=True):
    s, n = rig.solver, rig.sc["x0"].shape[0]
    s.set_car_vehicles(FC.car_vehicle_dicts(rig.pkg, rig.sc, n, mixed) if plant == "cars" else None)
    s.set_dtrack_vehicles(FC.dtrack_vehicles(rig.pkg, n) if plant == "dtrack" else None)


def fleet_rollout(rig, x0, periods, plant="handle", record=None, chunk=None, u_prev=None, period0=0, logs=True, cap=None, integral=None):
    """The scenario's fleet rollout from a zero PID state (or `integral`), in launches of `chunk` periods: numpy arrays [B, ...] like
    the restatement's, "u_prev", and with a recorder "ring" = the store read back."""
    import torch
    s, sc = rig.solver, rig.sc
    n = x0.shape[0]
    s.vanilla_create(sc["cfg"], n)
    if integral is not None:
        s.vanilla_reset(n, dev(s, integral))
    if record is not None:
        s.fleet_ss_create(n, cap)
    x = dev(s, x0)
    kw = dict(dtype=torch.float64, device=s.device)
    dist, wst = torch.zeros(n, **kw), torch.full((n,), -np.inf, **kw)
    up = None if u_prev is None else dev(s, u_prev)
    parts, flags = [], np.zeros(n, dtype=np.int32)
    for p0 in range(0, periods, chunk or periods):
        m = min(chunk or periods, periods - p0)
        out = s.vanilla_rollout_fleet(rig.spline, rig.table, x, m, sc["dt_sim"], sc["n_sub"], plant=plant, record=record, period0=period0 + p0,
                                      dt=sc["dt"], u_prev=up, speed_scale=sc["speed_scale"], logs=logs, distance=dist, worst_excess=wst)
        parts.append(out)
        flags |= out["flags"].cpu().numpy()
    s.synchronize()
    got = {"x": host(x), "distance": dist.cpu().numpy(), "worst_excess": wst.cpu().numpy(), "flags": flags, "pid": pid_of(s, n),
           "u_prev": None if up is None else host(up)}
    if logs:
        for k in ("X_log", "U_log", "k_log"):
            got[k] = host(torch.cat([p[k] for p in parts], dim=-2))
    if record is not None:
        got["ring"] = ring_of(s, n)
    return got


def ring_of(s, n):
    st = s.fleet_ss_stats(n)
    s.synchronize()
    return {"stats": {k: st[k].cpu().numpy() for k in STATS}, "laps": [s.fleet_ss_get_laps(b) for b in range(n)]}


def assert_rings_equal(got, want, cars=None):
    cars = range(len(want["laps"])) if cars is None else cars
    for k in STATS:
        assert np.array_equal(got["stats"][k][list(cars)], want["stats"][k][list(cars)]), k
    for b in cars:
        assert len(got["laps"][b]) == len(want["laps"][b]), b
        for lg, lw in zip(got["laps"][b], want["laps"][b]):
            for name, a, c in zip("xukt", lg, lw):
                assert np.array_equal(a, c), (b, name)


def assert_bits(got, want, keys=VC.ROLLOUT_KEYS + ("flags",)):
    for k in keys:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert all(np.array_equal(got["pid"][k], want["pid"][k]) for k in VC.PID_KEYS)


def worst_of(got, ref, keys=VC.ROLLOUT_KEYS):
    worst = {k: VC.err(got[k], ref[k]) for k in keys}
    worst["pid"] = max(VC.err(got["pid"][k], ref["pid"][k]) for k in VC.PID_KEYS)
    return worst


def unfused(rig, x0, periods, plant):
    """The only way to do a period's work without the fused kernel: vanilla_solve, then plant_step_cars / plant_step_dtrack."""
    import torch
    s, sc = rig.solver, rig.sc
    n = x0.shape[0]
    s.vanilla_create(sc["cfg"], n)
    x = dev(s, x0)
    step = s.plant_step_cars if plant == "cars" else s.plant_step_dtrack
    X_log, U_log, out = [], [], None
    for _ in range(periods):
        out = s.vanilla_solve(rig.spline, x, None, speed_scale=sc["speed_scale"], out=out)
        X_log.append(x.clone())
        U_log.append(out["u_model"].clone())
        step(rig.table, x, out["u_model"], sc["dt_sim"], sc["n_sub"])
    s.synchronize()
    assert not out["flags"].cpu().numpy().any()
    return {"x": host(x), "X_log": host(torch.stack(X_log, dim=1)), "U_log": host(torch.stack(U_log, dim=1)), "pid": pid_of(s, n)}


# ---- 1. the handle's plant, no recorder: lmpc_vanilla_rollout_batch's bits ----
@pytest.mark.parametrize("periods", (1, 2, VC.PERIODS))
@pytest.mark.parametrize("name", ("barc", "synthetic"))
def test_handle_plant_is_the_vanilla_rollout_bit_for_bit(rigs, name, periods):
    rig = rigs(name)
    want = TV.device_rollout(rig, rig.sc["x0"], periods)
    got = fleet_rollout(rig, rig.sc["x0"], periods)
    assert_bits(got, want)
    assert not got["flags"].any()


# ---- 2. the car table ----
def test_car_table_of_the_handles_vehicle_is_the_handle_plant(rigs):
    rig = rigs("barc")
    want = fleet_rollout(rig, rig.sc["x0"], VC.PERIODS)
    set_table(rig, "cars", mixed=False)
    got = fleet_rollout(rig, rig.sc["x0"], VC.PERIODS, plant="cars")
    set_table(rig, None)
    assert_bits(got, want)


@pytest.mark.parametrize("plant,tol", (("cars", VC.TOL_ROLLOUT), ("dtrack", FC.TOL_DTRACK)))
def test_table_plants_against_restatement_and_unfused_composition(pkg, rigs, plant, tol):
    """2. and 3.: 64 periods of 67 cars on the mixed car table / the four-wheel fleet."""
    rig = rigs("barc")
    set_table(rig, plant)
    got = fleet_rollout(rig, rig.sc["x0"], VC.PERIODS, plant=plant)
    loose = unfused(rig, rig.sc["x0"], VC.PERIODS, plant)
    set_table(rig, None)
    assert not got["flags"].any()
    ref = FC.reference(pkg, plant)
    worst = worst_of(got, ref)
    print(plant, "against the restatement", {k: "%.1e" % v for k, v in worst.items()})
    apart = worst_of(got, loose, ("x", "X_log", "U_log"))
    print(plant, "against vanilla_solve + plant_step_%s per period" % plant, {k: "%.1e" % v for k, v in apart.items()},
          "bit for bit" if max(apart.values()) == 0.0 else "NOT bit for bit")
    assert max(worst.values()) <= tol, worst
    assert np.array_equal(got["U_log"][:, :, 0], loose["U_log"][:, :, 0]), "the first decision, taken at the same state"
    assert max(apart.values()) <= tol, apart
    # the table is in effect: another plant than the handle's
    assert VC.err(got["x"], VC.reference("barc", "rollout", VC.PERIODS)["x"]) > 1e-6


# ---- 4. the recorder against a replay of the run's own logs ----
def replay(pkg, sc, got, record, cap, u_prev0, period0=0):
    """The run's logs through lmpc_fleet_ss_record_batch on a solver of its own, sample by sample."""
    import torch
    n, P = got["k_log"].shape
    other = Rig(pkg, sc)
    s = other.solver
    s.fleet_ss_create(n, cap)
    X, U, K = dev(s, got["X_log"]), dev(s, got["U_log"]), dev(s, got["k_log"])       # [6][P][n], [2][P][n], [P][n]
    first = dev(s, u_prev0) if record == "arrived" else None
    L = float(sc["trk"]["L"])
    for p in range(P):
        u = U[:, p] if record == "applied" else (U[:, p - 1] if p else first)
        s.fleet_ss_record(X[:, p], u, K[p], (period0 + p) * sc["dt"], L, active=torch.isfinite(K[p]).to(torch.int32))
    ring = ring_of(s, n)
    s.close()
    return ring


@pytest.mark.parametrize("record", ("applied", "arrived"))
@pytest.mark.parametrize("plant", FC.PLANTS)
def test_recorder_is_the_replay_of_its_own_logs(pkg, rigs, plant, record):
    """The handle's plant: 67 cars, 700 periods in chunks of 64, slots of 1024, at least one lap per car.  The tables: 16 cars, 1000
    periods, slots of 512, at least two laps per car."""
    n, periods, cap, laps = (B, 700, 1024, 1) if plant == "handle" else (16, 1000, 512, 2)
    rig = rigs("barc", n)
    sc = rig.sc
    u0 = np.random.default_rng(5).uniform(-0.1, 0.1, (n, 2))
    set_table(rig, plant)
    got = fleet_rollout(rig, sc["x0"], periods, plant=plant, record=record, chunk=64, u_prev=u0, period0=3, cap=cap)
    set_table(rig, None)
    assert not got["flags"].any() and (got["worst_excess"] <= 0.0).all()
    assert (got["ring"]["stats"]["laps_in_ring"] >= laps).all(), got["ring"]["stats"]["laps_in_ring"].min()
    assert not got["ring"]["stats"]["n_dropped"].any()
    assert np.array_equal(got["u_prev"], got["U_log"][:, :, -1])
    assert_rings_equal(got["ring"], replay(pkg, sc, got, record, cap, u0, period0=3))
    rig.solver.fleet_ss_destroy()


def test_short_slots_drop_every_lap(pkg, rigs):
    rig = rigs("barc", 16)
    sc = rig.sc
    u0 = np.zeros((16, 2))
    set_table(rig, "cars")
    got = fleet_rollout(rig, sc["x0"], 1000, plant="cars", record="arrived", chunk=64, u_prev=u0, cap=256)
    set_table(rig, None)
    st = got["ring"]["stats"]
    assert not st["laps_in_ring"].any() and (st["n_dropped"] >= 2).all() and np.array_equal(st["n_dropped"], st["lap_count"] - 1)
    assert_rings_equal(got["ring"], replay(pkg, sc, got, "arrived", 256, u0))
    rig.solver.fleet_ss_destroy()


def test_applied_on_the_handle_plant_is_run_vanilla(pkg, rigs):
    """closed_loop.run_vanilla(fused=True, fleet_record=True): one launch and 64 recorder launches per chunk, the same rings."""
    rig = rigs("barc")
    sc = rig.sc
    got = fleet_rollout(rig, sc["x0"], 700, record="applied", chunk=64, cap=1024)
    other = rigs("barc", B, 1)
    s = other.solver
    s.vanilla_create(sc["cfg"], B)
    s.fleet_ss_create(B, 1024)
    res = pkg.closed_loop.run_vanilla(s, other.table, other.spline, dev(s, sc["x0"]), 700, dt=sc["dt"], n_sub=sc["n_sub"], speed_scale=sc["speed_scale"],
                                      chunk=64, fused=True, fleet_record=True)
    s.synchronize()
    assert np.array_equal(host(res["x"]), got["x"]) and np.array_equal(host(res["X_log"]), got["X_log"])
    assert_rings_equal(got["ring"], ring_of(s, B))
    assert (got["ring"]["stats"]["laps_in_ring"] >= 1).all()
    s.fleet_ss_destroy()
    rig.solver.fleet_ss_destroy()


# ---- 5. chunks ----
def test_two_launches_of_32_leave_the_bits_of_one_of_64(rigs):
    rig = rigs("barc")
    sc = rig.sc
    x0 = sc["x0"].copy()
    x0[::2, 0] = sc["trk"]["L"] - 0.02 * (1 + np.arange(x0[::2].shape[0]))   # half the cars cross the start line within the run
    u0 = np.random.default_rng(6).uniform(-0.1, 0.1, (B, 2))
    set_table(rig, "cars")
    whole = fleet_rollout(rig, x0, 64, plant="cars", record="arrived", u_prev=u0, period0=10, cap=128)
    halves = fleet_rollout(rig, x0, 64, plant="cars", record="arrived", chunk=32, u_prev=u0, period0=10, cap=128)
    set_table(rig, None)
    assert_bits(halves, whole, VC.ROLLOUT_KEYS + ("flags", "u_prev"))
    assert_rings_equal(halves["ring"], whole["ring"])
    assert (whole["ring"]["stats"]["lap_count"] == 1).sum() >= B // 2
    rig.solver.fleet_ss_destroy()


# ---- 6. poison ----
def test_a_poisoned_car_is_frozen_and_never_recorded(pkg, rigs):
    rig = rigs("barc")
    sc = rig.sc
    integral, u0 = np.full(B, 0.25), np.random.default_rng(7).uniform(-0.1, 0.1, (B, 2))
    set_table(rig, "cars")
    clean = fleet_rollout(rig, sc["x0"], 700, plant="cars", record="arrived", u_prev=u0, logs=False, cap=1024, integral=integral)
    x0 = sc["x0"].copy()
    x0[5, 1], x0[40, 0] = np.nan, 1e300
    got = fleet_rollout(rig, x0, 700, plant="cars", record="arrived", u_prev=u0, logs=False, cap=1024, integral=integral)
    set_table(rig, None)
    planted = np.zeros(B, dtype=bool)
    planted[[5, 40]] = True
    rest = np.flatnonzero(~planted)
    assert (got["flags"][planted] == pkg.VANILLA_NOT_FINITE).all() and not got["flags"][~planted].any()
    assert np.array_equal(got["x"][planted], x0[planted], equal_nan=True)
    assert np.array_equal(got["u_prev"][planted], u0[planted])
    for k in VC.PID_KEYS:
        assert (got["pid"][k][planted] == (0.25 if k == "integral" else 0.0)).all(), k
        assert np.array_equal(got["pid"][k][~planted], clean["pid"][k][~planted]), k
    for b in np.flatnonzero(planted):
        assert got["ring"]["laps"][b] == [] and all(got["ring"]["stats"][k][b] == 0 for k in STATS)
    for k in ("x", "distance", "worst_excess", "u_prev"):
        assert np.array_equal(got[k][~planted], clean[k][~planted]), k
    assert_rings_equal(got["ring"], clean["ring"], cars=rest)
    assert (clean["ring"]["stats"]["laps_in_ring"] >= 1).all()
    rig.solver.fleet_ss_destroy()


# ---- 7. arguments ----
def test_argument_errors(pkg, rigs):
    import torch
    rig = rigs("barc", 4)
    s, sc = rig.solver, rig.sc
    bad = pytest.raises(pkg.LmpcError, match="-> -1")
    x = dev(s, sc["x0"])
    up = torch.full((2, 4), 0.125, dtype=torch.float64, device=s.device)
    kw = dict(dtype=torch.float64, device=s.device)
    logs = {"X_log": torch.full((6, 2, 4), -7.0, **kw), "U_log": torch.full((2, 2, 4), -7.0, **kw), "k_log": torch.full((2, 4), -7.0, **kw),
            "flags": torch.full((4,), -7, dtype=torch.int32, device=s.device)}

    def call(xx=x, periods=2, dt_sim=0.0125, n_sub=2, spline=rig.spline, table=rig.table, **over):
        args = dict(plant="handle", record=None, period0=0, dt=0.025, u_prev=up, out=logs)
        args.update(over)
        s.vanilla_rollout_fleet(spline, table, xx, periods, dt_sim, n_sub, **args)

    s.vanilla_destroy()
    s.fleet_ss_destroy()
    set_table(rig, None)
    with bad:
        call()                                                    # no vanilla store
    s.vanilla_create(sc["cfg"], 4)
    s.vanilla_reset(4, torch.full((4,), 0.25, **kw))
    s.fleet_ss_create(4, 64)
    s.fleet_ss_record(x, up, torch.zeros(4, **kw), 0.0, float(sc["trk"]["L"]))       # every recorder holds its first sample
    s.fleet_ss_record(torch.zeros_like(x), up, torch.zeros(4, **kw), 0.025, float(sc["trk"]["L"]))
    before_x, before_ring = x.clone(), ring_of(s, 4)
    five = dev(s, VC.scenario("barc", 5)["x0"])
    with bad:
        call(xx=five, u_prev=None)                                 # another batch than the store's
    for args in ((0, 0.01, 1), (-1, 0.01, 1), (2, 0.01, 0), (2, 0.0, 1), (2, -0.01, 1), (2, float("nan"), 1), (2, float("inf"), 1)):
        with bad:
            call(periods=args[0], dt_sim=args[1], n_sub=args[2])
    with bad:
        call(spline=None)                                         # null track
    with bad:
        call(table=dict(rig.table, L=0.0))                        # a table of no length
    io = pkg.capi.CVanillaFleetRollout()
    ct = s._ctrack(rig.table)
    import ctypes as C
    assert s.lib.lmpc_vanilla_rollout_fleet_batch(s._h, C.c_int32(4), rig.spline._p, C.byref(ct), None) == -1       # NULL io
    io.periods, io.n_sub, io.dt_sim, io.speed_scale = 2, 2, 0.0125, 1.0
    assert s.lib.lmpc_vanilla_rollout_fleet_batch(s._h, C.c_int32(4), rig.spline._p, C.byref(ct), C.byref(io)) == -1    # NULL io->x
    for plant, record in ((3, 0), (-1, 0), (0, 3), (0, -1)):                                                              # unknown values
        io.x, io.u_prev, io.plant, io.record, io.dt = x.data_ptr(), up.data_ptr(), plant, record, 0.025
        assert s.lib.lmpc_vanilla_rollout_fleet_batch(s._h, C.c_int32(4), rig.spline._p, C.byref(ct), C.byref(io)) == -1
    with bad:
        call(plant="cars")                                        # no car table
    with bad:
        call(plant="dtrack")                                      # no double-track table
    s.set_car_vehicles(FC.car_vehicle_dicts(pkg, VC.scenario("barc", 5), 5))
    s.set_dtrack_vehicles(FC.dtrack_vehicles(pkg, 5))
    with bad:
        call(plant="cars")                                        # a table of another batch
    with bad:
        call(plant="dtrack")
    set_table(rig, None)
    for dt in (0.0, -0.025, float("nan"), float("inf"), None):
        with bad:
            call(record="applied", dt=dt)                         # recording needs a time step
    with bad:
        call(record="arrived", u_prev=None)                       # ARRIVED reads u_prev
    with bad:
        call(period0=-1)
    with bad:
        call(record="applied", period0=-1)
    s.fleet_ss_destroy()
    with bad:
        call(record="applied")                                    # no fleet store
    s.fleet_ss_create(5, 64)
    with bad:
        call(record="arrived")                                    # a store of another batch
    assert "lmpc_vanilla_rollout_fleet_batch" in s.lib.lmpc_last_error(s._h).decode()
    s.synchronize()
    # nothing was written: outputs, state, u_prev, the PID state, and (before it was replaced) the store
    assert all((t == -7).all().item() for t in logs.values())
    assert torch.equal(x, before_x) and (up == 0.125).all().item()
    p = pid_of(s, 4)
    assert (p["integral"] == 0.25).all() and (p["error"] == 0).all() and (p["last_error"] == 0).all()
    s.fleet_ss_create(4, 64)
    s.fleet_ss_record(x, up, torch.zeros(4, **kw), 0.0, float(sc["trk"]["L"]))
    s.fleet_ss_record(torch.zeros_like(x), up, torch.zeros(4, **kw), 0.025, float(sc["trk"]["L"]))
    with bad:
        call(record="arrived", dt=0.0)
    assert_rings_equal(ring_of(s, 4), before_ring)
    call(record="arrived")                                        # the same call with a time step: accepted
    s.synchronize()
    assert not logs["flags"].cpu().numpy().any() and not torch.equal(x, before_x)
    s.fleet_ss_destroy()
    s.vanilla_destroy()


# ---- 8. the warm-up of the fleet LMPC experiment ----
def seam_stamps(laps, t_end):
    """The time stamps of the closed lap that holds samples of the warm-up and of the loop, or None."""
    for lap in laps:
        t = lap[3]
        if t[0] < t_end - 1e-9 and t[-1] > t_end - 1e-9:
            return t
    return None


def check_seam(learner, res, sc, n):
    """In every car's ring the lap that spans the seam between warm-up and loop has time stamps dt apart throughout.  A car whose seam
    lap was still open when the run ended gets two synthetic samples behind the run -- at 0.9 L, then at 0 -- which close it; the
    synthetic sample that lap then ends with is left out of the check."""
    import torch
    L, dt, t_end = float(sc["trk"]["L"]), sc["dt"], res["warmup"]["t_end"]
    t_run = t_end + res["steps"] * dt
    if any(seam_stamps(learner.fleet_ss_get_laps(b), t_end) is None for b in range(n)):
        x = res["x"].clone()
        zero = torch.zeros((2, n), dtype=torch.float64, device=x.device)
        for s_fake, tt in ((0.9 * L, t_run + dt), (0.0, t_run + 2 * dt)):
            x[0] = s_fake
            learner.fleet_ss_record(x, zero, zero[0], tt, L)
        learner.synchronize()
    for b in range(n):
        t = seam_stamps(learner.fleet_ss_get_laps(b), t_end)
        assert t is not None, b
        t = t[t < t_run + 0.5 * dt]
        assert t[0] < t_end - 1e-9 and t[-1] > t_end - 1e-9, b
        assert np.abs(np.diff(t) - dt).max() <= 1e-12, (b, np.abs(np.diff(t) - dt).max())


def experiment(pkg, n=8):
    sc = VC.scenario("barc", n)
    tracker = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    learner = pkg.Solver(pkg.presets.barc_lmpc(20, 3), pkg.presets.barc_vehicle(), device=0)
    asked = []
    solve = tracker.solve
    tracker.solve = lambda *a, **k: (asked.append(1), solve(*a, **k))[1]
    warmup = dict(config=sc["cfg"], spline=sc["trk"]["spline"], speed_scale=sc["speed_scale"], chunk=64, max_periods=2048)
    return sc, tracker, learner, asked, warmup


def test_fused_fleet_experiment_from_a_vanilla_warm_up(pkg):
    """8 cars on the mixed car table, warm_laps 2, learn_laps 1.  Asserted: the tracking controller never solves, every listed lap is
    "lmpc", the lap that spans the seam between warm-up and loop has time stamps dt apart throughout, no lap was dropped (slots of the
    experiment's default size, 1024 samples = 25.6 s: the warm-up's laps are 304 to 322 samples).  Whether the learning laps complete
    from pure-pursuit laps is reported (profiles/vanilla_fleet.md), not asserted: without the regression the three cars with 30 % less
    grip than the controllers' model fail most of their learning solves and leave the track (laps of 7.7, 12.05 and 17.05 s), the
    five others drive theirs in 5.3 to 7.3 s without a failure, and the run ends on its own after 653 periods."""
    import torch
    n = 8
    sc, tracker, learner, asked, warmup = experiment(pkg, n)
    x0 = torch.as_tensor(np.ascontiguousarray(sc["x0"].T), device="cuda")
    u0 = torch.zeros((2, n), dtype=torch.float64, device="cuda")
    res = pkg.closed_loop.run_lmpc_fleet_fused(tracker, learner, sc["trk"]["table"], x0, u0, warm_laps=2, learn_laps=1, dt=sc["dt"], n_sub=sc["n_sub"],
                                               max_steps=1500, plants=FC.car_vehicle_dicts(pkg, sc, n), warmup=warmup)
    torch.cuda.synchronize()
    w = res["warmup"]
    print("warm-up %d periods; the loop ran %d periods (%s), laps %s, n_fail %s, worst_excess %.4f"
          % (w["periods"], res["steps"], "ended on its own" if res["steps"] < 1500 else "stopped at max_steps", [len(v) for v in res["lap_times"]],
             res["n_fail"].cpu().numpy().tolist(), float(res["worst_excess"].max())))
    assert not asked, "the tracking controller was asked to solve"
    assert all(k == "lmpc" for kinds in res["lap_kind"] for k in kinds)
    assert not res["n_dropped"].cpu().numpy().any()
    assert (w["lap_count"] >= 3).all()
    with pytest.raises(pkg.LmpcError):
        learner.car_vehicles()                                     # the run cleared the table it set
    check_seam(learner, res, sc, n)
    tracker.close(), learner.close()


def test_unfused_fleet_experiment_on_four_wheel_cars_from_a_vanilla_warm_up(pkg):
    """run_lmpc_fleet(plants_dt=..., warmup=...), 40 periods past the warm-up: the same seam check."""
    import torch
    n = 8
    sc, tracker, learner, asked, warmup = experiment(pkg, n)
    x0 = torch.as_tensor(np.ascontiguousarray(sc["x0"].T), device="cuda")
    u0 = torch.zeros((2, n), dtype=torch.float64, device="cuda")
    res = pkg.closed_loop.run_lmpc_fleet(tracker, learner, sc["trk"]["table"], x0, u0, warm_laps=2, learn_laps=1, dt=sc["dt"], n_sub=sc["n_sub"],
                                         max_steps=40, plants_dt=FC.dtrack_vehicles(pkg, n), warmup=warmup)
    torch.cuda.synchronize()
    w = res["warmup"]
    print("warm-up %d periods on four-wheel cars; 40 periods of the loop: n_fail %s, worst_excess %.4f"
          % (w["periods"], res["n_fail"].cpu().numpy().tolist(), float(res["worst_excess"].max())))
    assert res["steps"] == 40 and not asked
    assert np.isfinite(res["x"].cpu().numpy()).all()
    with pytest.raises(pkg.LmpcError):
        learner.get_dtrack_vehicles()
    check_seam(learner, res, sc, n)
    tracker.close(), learner.close()
