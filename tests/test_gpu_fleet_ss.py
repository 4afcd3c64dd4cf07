"""The fleet safe set on the device -- one recorder and one ring of laps per car (lmpc_fleet_ss_*) -- against the host classes
(safe_set.py), the shared-store query kernel, the C oracle, and run_lmpc.  Every equality is np.array_equal: the feature moves and
selects doubles, it does not round them.  Needs an MI355X."""
from pathlib import Path

import numpy as np
import pytest

from oracle import cbind

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).parent / "golden" / "barc_ss"


# ---------------------------------------------------------------- recorder and ring against the host classes
L_REC, B_REC, T_REC, CAP, RING = 10.0, 257, 3000, 1024, 3


def recorder_inputs():
    rng = np.random.default_rng(21)
    ds = rng.uniform(0.004, 0.12, B_REC)
    s0 = rng.uniform(0, L_REC, B_REC)
    jit = rng.normal(0, 0.01, (T_REC, B_REC))
    ds[0], ds[1], s0[0] = 0.008, 4.0, 5.0
    s = np.mod(s0 + np.cumsum(np.broadcast_to(ds, (T_REC, B_REC)), axis=0) + jit, L_REC)
    r2 = np.random.default_rng(22)
    x = np.concatenate([s[:, None, :], r2.normal(size=(T_REC, 5, B_REC))], axis=1)   # [T][6][B]
    u = r2.normal(size=(T_REC, 2, B_REC))
    k = r2.normal(size=(T_REC, B_REC))
    t = 0.025 * np.arange(T_REC)
    return x, u, k, t


def host_fleet(pkg, x, u, k, t, L, cap, ring, active=None):
    """One SafeSetRecorder / SafeSetManager(ring) per car fed the same samples; the capacity rule -- a lap longer than `cap` is not
    added -- is applied here.  Returns per car: laps, lap_count, n_dropped, last_lap_time, longest open lap seen."""
    SS = pkg.safe_set

    class Capped(SS.SafeSetManager):
        def __init__(self):
            super().__init__(ring)
            self.n_dropped, self.t_first = 0, None

        def add_lap(self, lx, lu, lk, lt, total_length):
            self.t_first = float(np.asarray(lt).reshape(-1)[0])
            if np.asarray(lx).reshape(-1, 6).shape[0] > cap:
                self.n_dropped += 1
                return
            super().add_lap(lx, lu, lk, lt, total_length)

    T, _, B = x.shape
    res = []
    for b in range(B):
        man = Capped()
        rec = SS.SafeSetRecorder(man)
        last, longest = 0.0, 0
        if active is None or active[b]:
            for i in range(T):
                if rec.step(x[i, :, b], u[i, :, b], k[i, b], t[i], L):
                    last = t[i] - man.t_first
                if rec.initialized:
                    longest = max(longest, len(rec.x))
        res.append({"laps": list(man.laps), "lap_count": rec.lap_count, "n_dropped": man.n_dropped, "last_lap_time": last,
                    "longest_open": longest, "open_end": len(rec.x) if rec.initialized else 0})
    return res


def device_fleet(solver, x, u, k, t, L, active=None):
    import torch
    xd, ud, kd = (torch.as_tensor(a, device="cuda") for a in (x, u, k))
    act = None if active is None else torch.as_tensor(active.astype(np.int32), device="cuda")
    for i in range(x.shape[0]):
        solver.fleet_ss_record(xd[i], ud[i], kd[i], float(t[i]), L, active=act)
    solver.synchronize()


def assert_laps_equal(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for j, (g, w) in enumerate(zip(got, want)):
        for name, a, c in zip("xukt", g, w):
            assert np.array_equal(a, c), (what, "lap", j, name)


@pytest.fixture(scope="module")
def recorded(pkg):
    cfg = pkg.presets.barc_lmpc(20, RING)
    cfg.update(num_ss_pts=96, num_ss_pts_per_lap=32, max_lap_stored=RING)
    solver = pkg.Solver(cfg, pkg.presets.barc_vehicle(), device=0)
    nbytes = solver.fleet_ss_create(B_REC, CAP)
    x, u, k, t = recorder_inputs()
    host = host_fleet(pkg, x, u, k, t, L_REC, CAP, RING)
    device_fleet(solver, x, u, k, t, L_REC)
    return {"solver": solver, "host": host, "inputs": (x, u, k, t), "bytes": nbytes}


def test_recorder_inputs_cover_the_cases(recorded, pkg):
    """What the issue states about these inputs, from the host recorder alone (no capacity rule: the reference's unbounded store)."""
    x, u, k, t = recorded["inputs"]
    host = recorded["host"]
    n_closed = np.array([max(h["lap_count"] - 1, 0) for h in host])     # closed laps = crossings - the discarded partial lap
    assert (n_closed == 0).sum() == 1
    assert ((n_closed >= 1) & (n_closed <= 3)).sum() == 24
    assert (n_closed > 3).sum() == 232
    assert sum(h["n_dropped"] > 0 for h in host) == 19
    assert sum(h["open_end"] > CAP for h in host) == 7                  # the lap open at the end has passed the capacity
    assert min(lap[0].shape[0] for h in host for lap in h["laps"]) == 2
    assert 1100 <= n_closed[1] <= 1300


def test_recorder_and_ring_match_host_classes(recorded):
    solver, host = recorded["solver"], recorded["host"]
    assert recorded["bytes"] >= B_REC * (RING + 1) * CAP * 80 and recorded["bytes"] == solver.fleet_ss_bytes()
    st = {key: v.cpu().numpy() for key, v in solver.fleet_ss_stats(B_REC).items()}
    for b in range(B_REC):
        h = host[b]
        assert st["laps_in_ring"][b] == len(h["laps"]), b
        assert st["lap_count"][b] == h["lap_count"], b
        assert st["n_dropped"][b] == h["n_dropped"], b
        assert st["last_lap_time"][b] == h["last_lap_time"], b
        assert_laps_equal(solver.fleet_ss_get_laps(b), h["laps"], b)
    assert sum(h["n_dropped"] for h in host) > 0 and any(len(h["laps"]) == 0 for h in host)


def test_a_car_is_untouched_by_its_neighbours(recorded, pkg):
    """Canary: with only every second car recording (active), those cars' rings are what they were with everybody recording -- the
    over-capacity cars sit between ordinary ones -- and the others stay empty.  On a second store, which also exercises reset."""
    x, u, k, t = recorded["inputs"]
    host = recorded["host"]
    cfg = pkg.presets.barc_lmpc(20, RING)
    cfg.update(max_lap_stored=RING)
    solver = pkg.Solver(cfg, pkg.presets.barc_vehicle(), device=0)
    solver.fleet_ss_create(B_REC, CAP)
    for parity in (0, 1):
        solver.fleet_ss_reset()
        active = (np.arange(B_REC) % 2) == parity
        device_fleet(solver, x, u, k, t, L_REC, active=active)
        st = {key: v.cpu().numpy() for key, v in solver.fleet_ss_stats(B_REC).items()}
        for b in range(B_REC):
            if active[b]:
                assert_laps_equal(solver.fleet_ss_get_laps(b), host[b]["laps"], (parity, b))
                assert st["lap_count"][b] == host[b]["lap_count"] and st["n_dropped"][b] == host[b]["n_dropped"]
            else:
                assert solver.fleet_ss_get_laps(b) == [] and st["lap_count"][b] == 0 and st["last_lap_time"][b] == 0.0


# ---------------------------------------------------------------- the query against the oracle, per car
def test_query_matches_oracle_per_car(recorded):
    import torch
    solver, host = recorded["solver"], recorded["host"]
    rng = np.random.default_rng(4)
    q = np.stack([rng.uniform(-1.0, L_REC + 1.0, B_REC), rng.uniform(-0.3, 0.3, B_REC)])
    ss_x, ss_j, nf = (a.cpu().numpy() for a in solver.fleet_ss_query(q))
    empty = [b for b in range(B_REC) if not host[b]["laps"]]
    assert empty                      # (the car without a closed lap, and cars whose only closed laps were over capacity)
    for b in range(B_REC):
        rx, rj, rn = cbind.ss_query_batch([lap[0] for lap in host[b]["laps"]], L_REC, 96, 32, q[:, b:b + 1])
        assert nf[b] == rn[0], b
        assert np.array_equal(ss_x[:, :, b], rx[:, :, 0]), b
        assert np.array_equal(ss_j[:, b], rj[:, 0]), b
    for b in empty:
        assert nf[b] == 0 and not ss_x[:, :, b].any() and not ss_j[:, b].any()
    # a NaN query on one car: nothing found for it, the other cars' columns untouched.  The buffers are reused, poisoned first.
    bad = 100
    assert host[bad]["laps"]
    q2 = q.copy()
    q2[0, bad] = np.nan
    buf = (torch.full((6, 96, B_REC), 7.0, dtype=torch.float64, device="cuda"), torch.full((96, B_REC), 7.0, dtype=torch.float64, device="cuda"),
           torch.full((B_REC,), 7, dtype=torch.int32, device="cuda"))
    x2, j2, n2 = (a.cpu().numpy() for a in solver.fleet_ss_query(q2, out=buf))
    assert n2[bad] == 0 and not x2[:, :, bad].any() and not j2[:, bad].any()
    keep = np.arange(B_REC) != bad
    assert np.array_equal(n2[keep], nf[keep]) and np.array_equal(x2[:, :, keep], ss_x[:, :, keep]) and np.array_equal(j2[:, keep], ss_j[:, keep])


# ---------------------------------------------------------------- the query against the shared-store kernel
def golden_laps():
    return [tuple(np.loadtxt(GOLD / f"ss_lap_{i}_{s}.txt", ndmin=2) for s in "xukt") for i in (1, 2, 3)]


def both_queries(pkg, cfg, laps, L, q, cap):
    """(shared-store result, fleet result) of the same queries on equal stores: set_safe_set(laps) against the laps loaded into
    every car of a fleet of q.shape[1] cars."""
    B = q.shape[1]
    shared = pkg.Solver(cfg, pkg.presets.barc_vehicle(), device=0)
    shared.set_safe_set([lap[0] for lap in laps], L)
    want = tuple(a.cpu().numpy() for a in shared.ss_query(q))
    fleet = pkg.Solver(cfg, pkg.presets.barc_vehicle(), device=0)
    fleet.fleet_ss_create(B, cap)
    fleet.fleet_ss_load(laps, L, car=-1)
    got = tuple(a.cpu().numpy() for a in fleet.fleet_ss_query(q))
    return want, got, fleet


@pytest.mark.parametrize("n_laps", [3, 1])
def test_query_equals_shared_store_kernel_on_recorded_laps(pkg, n_laps):
    from test_safe_set_oracle import load_laps
    laps = golden_laps()
    for a, c in zip(load_laps(), laps):
        assert np.array_equal(a, c[0])
    L = 17.05
    rng = np.random.default_rng(3)
    q = np.stack([rng.uniform(-1.0, L + 1.0, 777), rng.uniform(-0.3, 0.3, 777)])
    cfg = pkg.presets.barc_lmpc(20, n_laps)
    assert cfg["num_ss_pts"] == 32 * n_laps and cfg["num_ss_pts_per_lap"] == 32 and cfg["max_lap_stored"] == n_laps
    cap = max(lap[0].shape[0] for lap in laps)
    want, got, fleet = both_queries(pkg, cfg, laps, L, q, cap)
    for w, g, name in zip(want, got, ("ss_x", "ss_j", "n_found")):
        assert np.array_equal(w, g), name
    # what went in comes out: the ring of any car holds the last n_laps laps, x, u, k and t
    for car in (0, 776):
        assert_laps_equal(fleet.fleet_ss_get_laps(car), [tuple(a if a.shape[1] > 1 else a[:, 0] for a in lap) for lap in laps[-n_laps:]], car)
    st = fleet.fleet_ss_stats(777)
    assert (st["laps_in_ring"].cpu().numpy() == n_laps).all() and (st["lap_count"].cpu().numpy() == 3).all()


def awkward_cases():
    """The nine cases of test_gpu_path.test_ss_query_awkward_laps_match_oracle, generator re-stated: laps that defeat the fast
    path (a lap passing the same place every 64 samples), K = 64, a lap shorter than K, exact distance ties, truncated / padded S."""
    rng = np.random.default_rng(12)
    L = 10.0

    def lap(n, s):
        x = np.zeros((n, 6))
        x[:, 0] = s
        x[:, 1] = 0.05 * np.sin(np.arange(n) * 0.7)
        x[:, 2:] = rng.normal(size=(n, 4))
        return x
    n = 448
    looping = lap(n, 0.5 + 0.01 * (np.arange(n) % 64) + 1e-4 * (np.arange(n) // 64))
    tied = lap(200, np.repeat(np.linspace(0.0, 9.9, 100), 2))
    tied[:, 1] = 0.0
    short = lap(20, np.linspace(0.0, 9.0, 20))
    normal = lap(400, np.linspace(0.0, 9.99, 400))
    q = np.stack([rng.uniform(-1.0, L + 1.0, 300), rng.uniform(-0.2, 0.2, 300)])
    q[:, :40] = np.stack([tied[::5, 0], np.zeros(40)])
    cases = (([normal, looping], 32, 64), ([looping, normal, looping], 32, 96), ([normal, tied], 32, 64),
             ([normal, short, looping], 32, 96), ([looping, normal], 64, 128), ([short], 32, 32),
             ([normal, looping], 32, 50), ([tied, normal], 32, 80), ([normal], 32, 96))
    return L, q, cases


@pytest.mark.parametrize("case", range(9))
def test_query_equals_shared_store_kernel_on_awkward_laps(pkg, case):
    L, q, cases = awkward_cases()
    laps_x, K, S = cases[case]
    r = np.random.default_rng(100 + case)
    laps = [(x, r.normal(size=(x.shape[0], 2)), r.normal(size=x.shape[0]), np.arange(x.shape[0]) * 0.025) for x in laps_x]
    cfg = pkg.presets.barc_lmpc(20, 3)
    cfg.update(num_ss_pts=S, num_ss_pts_per_lap=K, max_lap_stored=len(laps))
    want, got, _ = both_queries(pkg, cfg, laps, L, q, 448)
    rx, rj, rn = cbind.ss_query_batch(laps_x, L, S, K, q)
    for w, g, o, name in zip(want, got, (rx, rj, rn), ("ss_x", "ss_j", "n_found")):
        assert np.array_equal(w, g), (name, K, S)
        assert np.array_equal(o, g), (name, K, S, "oracle")


def test_argument_errors(pkg):
    import torch
    cfg = pkg.presets.barc_lmpc(20, 3)
    solver = pkg.Solver(cfg, pkg.presets.barc_vehicle(), device=0)
    q = torch.zeros((2, 8), dtype=torch.float64, device="cuda")
    with pytest.raises(pkg.LmpcError, match="-> -1"):      # no fleet store
        solver.fleet_ss_query(q)
    with pytest.raises(pkg.LmpcError, match="-> -1"):      # sizes that would overflow
        solver.fleet_ss_create(2 ** 31 - 1, 2 ** 31 - 1)
    assert solver.fleet_ss_bytes() == 0
    solver.fleet_ss_create(16, 8)
    with pytest.raises(pkg.LmpcError, match="-> -1"):      # a batch other than the store's
        solver.fleet_ss_query(q)
    with pytest.raises(pkg.LmpcError, match="-> -1"):
        solver.fleet_ss_record(torch.zeros((6, 8), dtype=torch.float64, device="cuda"), torch.zeros((2, 8), dtype=torch.float64, device="cuda"),
                               torch.zeros(8, dtype=torch.float64, device="cuda"), 0.0, 10.0)
    lap = (np.zeros((9, 6)), np.zeros((9, 2)), np.zeros(9), np.zeros(9))
    with pytest.raises(pkg.LmpcError, match="-> -1"):      # a lap over the capacity
        solver.fleet_ss_load([lap], 10.0, car=3)
    assert solver.fleet_ss_get_laps(3) == []
    solver.fleet_ss_destroy()
    assert solver.fleet_ss_bytes() == 0
    cfg2 = dict(cfg, num_ss_pts_per_lap=65, num_ss_pts=130)
    wide = pkg.Solver(cfg2, pkg.presets.barc_vehicle(), device=0)
    wide.fleet_ss_create(8, 8)
    with pytest.raises(pkg.LmpcError, match="-> -1"):      # num_ss_pts_per_lap > 64
        wide.fleet_ss_query(q)


# ---------------------------------------------------------------- the experiment
def experiment(pkg, x0, fleet, **kw):
    import torch
    N, B = 20, x0.shape[1]
    tracker = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
    learner = pkg.Solver(pkg.presets.barc_lmpc(N, 3), pkg.presets.barc_vehicle(), device=0)
    tr = pkg.workloads.synthetic_track("barc")
    fn = pkg.closed_loop.run_lmpc_fleet if fleet else pkg.closed_loop.run_lmpc
    res = fn(tracker, learner, tr, torch.as_tensor(x0, device="cuda"), torch.zeros((2, B), dtype=torch.float64, device="cuda"),
             warm_laps=2, learn_laps=4, warm_speed_scale=0.7, **kw)
    return res, learner, tr


def experiment_x0():
    """x0 of test_gpu_path.test_lmpc_experiment_lap_times_improve."""
    B = 64
    rng = np.random.default_rng(0)
    x0 = np.stack([np.full(B, 0.5), rng.uniform(-0.05, 0.05, B), np.zeros(B), np.full(B, 2.0), np.zeros(B), np.zeros(B)])
    x0[:, 0] = [0.5, 0.0, 0.0, 2.0, 0.0, 0.0]
    return x0


def periods(times, dt=0.025):
    return [int(round(v / dt)) for v in times]


def test_experiment_identical_cars(pkg):
    """64 copies of car 0: run_lmpc_fleet and run_lmpc do the same solves, so car 0's laps are run_lmpc's, lap for lap in whole
    control periods, and every other car equals car 0."""
    x0 = np.repeat(experiment_x0()[:, :1], 64, axis=1)
    ref, _, _ = experiment(pkg, x0, fleet=False)
    res, _, _ = experiment(pkg, x0, fleet=True)
    print("run_lmpc", periods(ref["lap_times"]), ref["lap_kind"], "fleet car 0", periods(res["lap_times"][0]), res["lap_kind"][0])
    assert ref["lap_kind"] == ["tracking", "tracking", "lmpc", "lmpc", "lmpc", "lmpc"]
    assert periods(res["lap_times"][0]) == periods(ref["lap_times"]) and res["lap_kind"][0] == ref["lap_kind"]
    for b in range(1, 64):
        assert res["lap_times"][b] == res["lap_times"][0] and res["lap_kind"][b] == res["lap_kind"][0], b
    assert (res["laps_in_ring"].cpu().numpy() == 3).all()
    assert (res["n_dropped"].cpu().numpy() == 0).all()
    assert res["steps"] == ref["steps"]


def test_experiment_different_cars(pkg):
    """The experiment's own x0 (e_y +-0.05): one workgroup solves one problem, so car 0's problem is the same in both runs whatever
    its neighbours do, and its lap period counts equal run_lmpc's car 0 -- which pins the per-car phase switch while other cars
    switch at other times.  Every car's ring equals what a host SafeSetRecorder builds from the samples the car's recorder was
    handed.  No improvement factor is asserted for cars other than car 0: how they drive on their own sets is reported
    (profiles/fleet_lmpc_experiment.md), not gated."""
    x0 = experiment_x0()
    ref, _, _ = experiment(pkg, x0, fleet=False)
    res, learner, tr = experiment(pkg, x0, fleet=True, record_trace=True)
    n = len(ref["lap_times"])
    print("run_lmpc", periods(ref["lap_times"]), "fleet car 0", periods(res["lap_times"][0]), "steps", ref["steps"], res["steps"])
    assert n == 6
    assert periods(res["lap_times"][0][:n]) == periods(ref["lap_times"]) and res["lap_kind"][0][:n] == ref["lap_kind"]
    x = np.stack([s[0].cpu().numpy() for s in res["trace"]])
    u = np.stack([s[1].cpu().numpy() for s in res["trace"]])
    k = np.stack([s[2].cpu().numpy() for s in res["trace"]])
    t = np.array([s[3] for s in res["trace"]])
    host = host_fleet(pkg, x, u, k, t, float(tr["L"]), 1024, 3)
    lir, nd = res["laps_in_ring"].cpu().numpy(), res["n_dropped"].cpu().numpy()
    for b in range(64):
        assert_laps_equal(learner.fleet_ss_get_laps(b), host[b]["laps"], b)
        assert lir[b] == len(host[b]["laps"]) and nd[b] == host[b]["n_dropped"], b
        closed = max(host[b]["lap_count"] - 1, 0)
        assert len(res["lap_times"][b]) == min(closed, 14), b
