"""lmpc_fleet_loop_advance_batch: everything between two solves of a fleet LMPC period in one launch.  It must be the composition of
what it replaces in closed_loop.run_lmpc_fleet -- result selection between the two controllers, lmpc_plant_step_batch,
lmpc_shift_batch per controller, lmpc_prepare_failed_batch, lmpc_fleet_ss_record_batch, lmpc_fleet_ss_stats and the torch
bookkeeping -- compared here bit for bit on one call (the project's allowance for the last knot's one-step rollout, the recorded
curvature and the lap time: rtol 1e-14, atol 1e-15, tests/test_gpu_loop.py), and over whole runs of the experiment.
Needs an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("X_ref", "U_ref", "T_ref", "bound_left", "bound_right", "curvatures", "vel_ref")
B, CAP, RING, DT, T_CALL = 70, 8, 2, 0.025, 0.5
WARM, LEARN, N_REC = 2, 2, 3
SPEED = (0.7, 1.0)
F64 = dict(dtype=torch.float64, device="cuda")

# What each car's recorder has seen before the call, as abscissae in units of L ("s0": the car's own abscissa), and what the call's
# sample then does.  A crossing is a drop of more than L / 2.
CASES = (
    ("seeds", (), "far"),                                                              # a fresh recorder: the sample only seeds it
    ("first crossing", ("s0",), "line"),                                               # the partial lap is discarded
    ("close fills ring", (0.9, 0.1, 0.5, 0.9, 0.1, 0.5, "s0"), "line"),                # 1 -> 2 laps = warm_laps
    ("close below warm", (0.9, 0.1, 0.5, "s0"), "line"),                               # 0 -> 1 lap
    ("learning close", (0.9, 0.1, 0.5, 0.9, 0.1, 0.5, "s0"), "line"),                  # phase 1, n_learn reaches learn_laps
    ("close evicts", (0.9, 0.1, 0.5, 0.9, 0.1, 0.5, 0.9, 0.1, 0.5, "s0"), "line"),     # ring full before
    ("overflow dropped", (0.9, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.85, "s0"), "line"),   # 10 samples into a slot of 8
    ("no crossing", (0.9, 0.1, "s0"), "far"),                                          # an open lap gets one more sample
)
CASE = np.arange(B) % len(CASES)
PHASE0 = np.where(np.isin(CASE, (4, 5)) | (np.isin(CASE, (0, 7)) & ((np.arange(B) // len(CASES)) % 2 == 1)), 1, 0).astype(np.int32)
N_LEARN0 = np.where(CASE == 4, LEARN - 1, 0).astype(np.int32)


def low_mu(pkg):
    return dict(pkg.presets.barc_vehicle(), mu=0.7)


def clone(d):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}


def prefeed(solver, s0, L):
    """Puts every car's recorder into its case's state through lmpc_fleet_ss_record_batch (the recorder does not check physics)."""
    solver.fleet_ss_create(B, CAP)
    rng = np.random.default_rng(11)
    steps = max(len(c[1]) for c in CASES)
    for j in range(steps):
        act = np.array([j < len(CASES[c][1]) for c in CASE], dtype=np.int32)
        s = np.array([(s0[b] if CASES[c][1][j] == "s0" else CASES[c][1][j] * L) if act[b] else 0.0 for b, c in enumerate(CASE)])
        x = np.concatenate([s[None, :], rng.normal(size=(5, B))])
        solver.fleet_ss_record(torch.as_tensor(x, **F64), torch.as_tensor(rng.normal(size=(2, B)), **F64),
                               torch.as_tensor(rng.normal(size=B), **F64), 0.025 * j, L, active=torch.as_tensor(act, device="cuda"))


def ring_state(solver):
    st = {k: v.cpu().numpy() for k, v in solver.fleet_ss_stats(B).items()}
    st["laps"] = [solver.fleet_ss_get_laps(b) for b in range(B)]
    return st


def close_open_laps(solver, L):
    """One more sample just behind the line for every car: what the call recorded into OPEN laps becomes visible to get_laps."""
    x = torch.zeros((6, B), **F64)
    x[0] = 1e-4
    solver.fleet_ss_record(x, torch.zeros((2, B), **F64), torch.zeros(B, **F64), 9.0, L)


def assert_rings(got, want, what):
    for key in ("laps_in_ring", "lap_count", "n_dropped"):
        assert np.array_equal(got[key], want[key]), (what, key)
    np.testing.assert_allclose(got["last_lap_time"], want["last_lap_time"], rtol=1e-14, atol=1e-15, err_msg=str(what))
    for b in range(B):
        assert len(got["laps"][b]) == len(want["laps"][b]), (what, b)
        for j, (g, w) in enumerate(zip(got["laps"][b], want["laps"][b])):
            for name, a, c in zip("xukt", g, w):
                if name == "k":   # the curvature: the kernel's own table lookup against the harness's torch interpolation
                    np.testing.assert_allclose(a, c, rtol=1e-14, atol=1e-15, err_msg=str((what, b, j)))
                else:
                    assert np.array_equal(a, c), (what, b, "lap", j, name)


def torch_curvature(trk, s):
    """run_lmpc_fleet's periodic linear interpolation of the curvature table."""
    curv, L = trk["curvature"], trk["L"]
    M = int(curv.numel())
    pos = torch.remainder(s, L) * (M / L)
    i0 = torch.clamp(pos.floor().long(), 0, M - 1)
    fr = pos - i0
    return curv[i0] * (1.0 - fr) + curv[(i0 + 1) % M] * fr


def query_formula(X_ref, x, L):
    s_last, s0 = X_ref[0, -1], x[0]
    kk = (s0 - s_last).abs() + L / 2
    return torch.stack([s_last + (kk - torch.fmod(kk, L)) * torch.sign(s0 - s_last), X_ref[1, -1]])


_scenes = {}


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    """The scenes' Solvers (and the plant Solver reference() adds) live for this module only."""
    yield
    for sc in _scenes.values():
        for sv in (sc["tracker"], sc["learner"], sc["ref"], *sc["plants"].values()):
            sv.close()
    _scenes.clear()


def scene(pkg, N):
    """Tracker and learner solve one prepared batch; shared by the tests of a horizon and left unchanged (they work on clones)."""
    if N in _scenes:
        return _scenes[N]
    tr = pkg.workloads.synthetic_track("barc")
    L = float(tr["L"])
    veh = pkg.presets.barc_vehicle()
    cfg_l = pkg.presets.barc_lmpc(N, RING)
    tracker = pkg.Solver(pkg.presets.barc_tracking_mpc(N), veh, device=0)
    learner = pkg.Solver(cfg_l, veh, device=0)
    ref = pkg.Solver(cfg_l, veh, device=0)      # owns the second store, the reference's
    trk = tracker.device_track(tr)
    rng = np.random.default_rng(5)
    place = np.array([CASES[c][2] == "line" for c in CASE])
    s0 = np.where(place, L - 1e-3, rng.uniform(0.15 * L, 0.8 * L, B))     # half a plant step is ~0.01 m: these cars cross in the call
    vel = np.interp(s0, np.arange(tr["M"]) * L / tr["M"], tr["vel"], period=L)
    x = np.stack([s0, rng.uniform(-0.1, 0.1, B), rng.normal(0, 0.03, B), 0.9 * vel, rng.normal(0, 0.02, B), rng.normal(0, 0.1, B)])
    x[3, ::9] = 3.4                                  # outside the learner's state box (vx <= 3; braking takes < 0.25 m/s off in a period): x_ic must be projected
    x = torch.as_tensor(x, **F64)
    u_prev = torch.as_tensor(rng.normal(0, 1e-3, (2, B)), **F64)
    inp = tracker.prepare(trk, x, DT, speed_scale=SPEED[0])
    inp["x_ic"], inp["u_ic"] = x, u_prev
    out_t = tracker.solve(inp)
    learner.set_safe_set(pkg.workloads.synthetic_laps(tr, RING), L)
    ss_x, ss_j, _ = learner.ss_query(query_formula(inp["X_ref"], x, L).contiguous())
    out_l = learner.alloc_outputs(B)
    out_l["convex_combi_optm"] = torch.zeros((ss_x.shape[1], B), **F64)
    learner.solve(inp, out_l, ss_x=ss_x, ss_j=ss_j)
    for o in (out_t, out_l):                          # (a failed solve may leave anything: the bit comparisons need numbers)
        o["X_optm"], o["U_optm"] = torch.nan_to_num(o["X_optm"]), torch.nan_to_num(o["U_optm"])
    # some are declared failed, as test_gpu_loop.py does, and every fifth learning solve that failed is declared solved with the
    # tracker's plan as its result (the call moves plans, it does not judge them), so that both branches of both phases are populated
    fill = (out_l["status"] != 0) & (out_t["status"] == 0) & (torch.arange(B, device="cuda") % 5 == 1)
    out_l["X_optm"][..., fill], out_l["U_optm"][..., fill] = out_t["X_optm"][..., fill], out_t["U_optm"][..., fill]
    out_l["status"][fill] = 0
    out_t["status"][::7] = 1
    out_l["status"][::5] = 1
    torch.cuda.synchronize()
    sc = dict(tr=tr, trk=trk, L=L, tracker=tracker, learner=learner, ref=ref, x=x, u_prev=u_prev, inp=inp, out_t=out_t, out_l=out_l,
              s0=s0, plants={})
    _scenes[N] = sc
    return sc


def fresh_state(learner, phase=PHASE0, n_learn=N_LEARN0):
    st = learner.fleet_loop_state(B, N_REC)
    st["phase"].copy_(torch.as_tensor(phase))
    st["n_learn"].copy_(torch.as_tensor(n_learn))
    st["counters"].copy_(torch.tensor([int(phase.sum()), 0], dtype=torch.int32))
    return st


def advance(sc, st, x, u, inp, out_t, out_l, **kw):
    args = dict(dt=DT, dt_sim=DT / 2, n_sub=2, t=T_CALL, speed_scale=SPEED, speed_limit=(6.0, 3.0), restart_failed=False, warm_laps=WARM,
                learn_laps=LEARN, switch_phase=True)
    args.update(kw)
    sc["learner"].fleet_loop_advance(sc["trk"], inp, out_t, out_l, x, u, st, **args)


def reference(pkg, sc, restart, plant, out_t, out_l, phase=PHASE0, n_learn=N_LEARN0, head_only=False):
    """run_lmpc_fleet's own sequence on copies, with the second store."""
    tracker, learner, ref, trk, L = sc["tracker"], sc["learner"], sc["ref"], sc["trk"], sc["L"]
    sel = torch.as_tensor(phase.astype(bool), device="cuda")
    inp, x, u_prev = sc["inp"], sc["x"], sc["u_prev"]
    r = {}
    if head_only:
        r["x"], r["u_prev"], r["nxt"] = x.clone(), u_prev.clone(), clone(inp)
        r["n_fail"] = torch.zeros(B, dtype=torch.int64, device="cuda")
        r["distance"], r["worst_excess"] = torch.zeros(B, **F64), torch.zeros(B, **F64)
        ok = torch.ones(B, dtype=torch.bool, device="cuda")
    else:
        bad = torch.ones(B, dtype=torch.int32, device="cuda")
        zt = dict(X_optm=torch.zeros_like(inp["X_ref"]), U_optm=torch.zeros_like(inp["U_ref"]), status=bad)
        ot, ol = (out_t or zt), (out_l or zt)
        out = {k: torch.where(sel, ol[k], ot[k]).contiguous() for k in ("X_optm", "U_optm", "status")}
        ok = out["status"] == 0
        u_apply = torch.where(ok[None, :], out["U_optm"][:, 0, :], inp["U_ref"][:, 0, :]).contiguous()
        if plant is not None and "sv" not in sc["plants"]:
            sc["plants"]["sv"] = pkg.Solver(pkg.presets.barc_tracking_mpc(tracker.N), plant, device=0)
        r["x"] = (sc["plants"]["sv"] if plant is not None else learner).plant_step(trk, x.clone(), u_apply, DT / 2, 2)
        r["u_prev"] = u_apply
        ds = r["x"][0] - x[0]
        r["distance"] = torch.where(ds < -L / 2, ds + L, ds)
        hb = float(learner.vehicle["b"]) / 2
        r["worst_excess"] = torch.maximum(torch.zeros(B, **F64),
                                          torch.maximum(r["x"][1] + hb - inp["bound_left"][0], inp["bound_right"][0] - (r["x"][1] - hb)))
        r["n_fail"] = (~ok).to(torch.int64)
        nl = learner.shift(trk, inp, out, DT, speed_scale=SPEED[1])
        nt = tracker.shift(trk, inp, out, DT, speed_scale=SPEED[0])
        if restart:
            learner.prepare_failed(trk, r["x"], out["status"], nl, DT, speed_scale=SPEED[1])
            tracker.prepare_failed(trk, r["x"], out["status"], nt, DT, speed_scale=SPEED[0])
        r["nxt"] = {k: torch.where(sel, nl[k], nt[k]) for k in KEYS}
    r["ok"] = ok
    x_lo = torch.as_tensor(learner.config["x_min"], **F64)[:, None]
    x_hi = torch.as_tensor(learner.config["x_max"], **F64)[:, None]
    r["x_ic"] = torch.where(sel[None, :], torch.minimum(torch.maximum(r["x"], x_lo), x_hi), r["x"])
    prefeed(ref, sc["s0"], L)
    before = ref.fleet_ss_stats(B)
    count_prev = before["lap_count"].clone()
    ref.fleet_ss_record(r["x"], r["u_prev"], torch_curvature(trk, r["x"][0]), T_CALL, L)
    stats = ref.fleet_ss_stats(B)
    closed = (stats["lap_count"] != count_prev) & (count_prev >= 1)
    slot = torch.clamp(count_prev.long() - 1, 0, N_REC - 1)[None, :]
    keep = (closed & (count_prev <= N_REC))[None, :]
    lap_time, lap_kind = torch.zeros((N_REC, B), **F64), torch.zeros((N_REC, B), dtype=torch.int32, device="cuda")
    lap_time.scatter_(0, slot, torch.where(keep, stats["last_lap_time"][None, :], lap_time.gather(0, slot)))
    lap_kind.scatter_(0, slot, torch.where(keep, sel[None, :].to(torch.int32), lap_kind.gather(0, slot)))
    r["lap_time"], r["lap_kind"], r["closed"] = lap_time, lap_kind, closed
    r["n_learn"] = torch.as_tensor(n_learn, device="cuda") + (closed & sel).to(torch.int32)
    r["done_now"] = int((closed & sel & (r["n_learn"] == LEARN)).sum())
    r["switch"] = (~sel) & (stats["laps_in_ring"] >= WARM)
    r["ring"] = ring_state(ref)
    close_open_laps(ref, L)
    r["ring_closed"] = ring_state(ref)
    return r


def compare(sc, r, got, st, switch, what):
    x2, u2, inp2, dist, exc, nf = got
    ok = r["ok"]
    assert torch.equal(x2, r["x"]) and torch.equal(u2, r["u_prev"]), what
    assert torch.equal(dist, r["distance"]) and torch.equal(exc, r["worst_excess"]) and torch.equal(nf, r["n_fail"]), what
    for k in KEYS:
        a, w = inp2[k], r["nxt"][k]
        if k in ("U_ref", "T_ref"):
            assert torch.equal(a, w), (what, k)
            continue
        assert torch.equal(a[..., :-1, :], w[..., :-1, :]), (what, k)
        assert torch.equal(a[..., -1, :][..., ~ok], w[..., -1, :][..., ~ok]), (what, k)
        assert torch.allclose(a[..., -1, :], w[..., -1, :], rtol=1e-14, atol=1e-15), (what, k, float((a[..., -1, :] - w[..., -1, :]).abs().max()))
    assert torch.equal(st["x_ic"], r["x_ic"]), what
    assert torch.equal(st["query"], query_formula(inp2["X_ref"], x2, sc["L"])), what      # on the X_ref this call wrote
    assert torch.equal(st["lap_kind"], r["lap_kind"]) and torch.equal(st["n_learn"], r["n_learn"]), what
    assert torch.allclose(st["lap_time"], r["lap_time"], rtol=1e-14, atol=1e-15), what
    phase0 = torch.as_tensor(PHASE0, device="cuda")
    want_phase = torch.where(r["switch"], torch.ones_like(phase0), phase0) if switch else phase0
    assert torch.equal(st["phase"], want_phase), what
    c = st["counters"].cpu().numpy()
    assert c[0] == int(phase0.sum()) + (int(r["switch"].sum()) if switch else 0) and c[1] == r["done_now"], (what, c)
    assert_rings(ring_state(sc["learner"]), r["ring"], what)
    close_open_laps(sc["learner"], sc["L"])
    assert_rings(ring_state(sc["learner"]), r["ring_closed"], (what, "closed"))


def one_call(sc, switch, restart, plant, out_t, out_l, head_only=False):
    prefeed(sc["learner"], sc["s0"], sc["L"])
    st = fresh_state(sc["learner"])
    inp2, x2, u2 = clone(sc["inp"]), sc["x"].clone(), sc["u_prev"].clone()
    dist, exc, nf = torch.zeros(B, **F64), torch.zeros(B, **F64), torch.zeros(B, dtype=torch.int64, device="cuda")
    if head_only:
        advance(sc, st, x2, u2, inp2, None, None, switch_phase=switch, restart_failed=restart, plant=plant)
    else:
        advance(sc, st, x2, u2, inp2, out_t, out_l, switch_phase=switch, restart_failed=restart, plant=plant, distance=dist, worst_excess=exc,
                n_fail=nf)
    torch.cuda.synchronize()
    return (x2, u2, inp2, dist, exc, nf), st


# ---------------------------------------------------------------- 1. one call is the composition of what it replaces
@pytest.mark.parametrize("plant", [False, True])
@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("N", [20, 3])
def test_one_call_is_the_composition_of_what_it_replaces(pkg, N, restart, plant):
    sc = scene(pkg, N)
    pv = low_mu(pkg) if plant else None
    r = reference(pkg, sc, restart, pv, sc["out_t"], sc["out_l"])
    ok, closed, cnt = r["ok"].cpu().numpy(), r["closed"].cpu().numpy(), r["ring"]["laps_in_ring"]
    # the batch covers what the issue lists
    assert 0 < (~ok).sum() < B and (ok & (PHASE0 == 1)).any() and (ok & (PHASE0 == 0)).any()
    assert r["ring"]["lap_count"][CASE == 0].max() == 0 and (r["ring"]["lap_count"][CASE == 1] == 1).all() and not closed[CASE == 1].any()
    assert (cnt[CASE == 2] == WARM).all() and (cnt[CASE == 3] == 1).all() and closed[np.isin(CASE, (2, 3, 4, 5, 6))].all()
    assert r["done_now"] == int((CASE == 4).sum()) > 0
    assert (cnt[CASE == 5] == RING).all() and (r["ring"]["n_dropped"][CASE == 6] == 1).all() and (cnt[CASE == 6] == 0).all()
    assert not closed[CASE == 7].any() and (r["ring"]["lap_count"][CASE == 7] == 1).all()
    assert int(r["switch"].sum()) == int((CASE == 2).sum()) > 0
    assert not torch.equal(r["x_ic"], r["x"])          # the projection did something
    if plant:
        assert not torch.equal(r["x"], sc["learner"].plant_step(sc["trk"], sc["x"].clone(), r["u_prev"], DT / 2, 2))
    for switch in (False, True):
        got, st = one_call(sc, switch, restart, pv, sc["out_t"], sc["out_l"])
        compare(sc, r, got, st, switch, (N, restart, plant, switch))


# ---------------------------------------------------------------- 2. variants of the call
def test_head_only_call(pkg):
    sc = scene(pkg, 20)
    r = reference(pkg, sc, False, None, None, None, head_only=True)
    got, st = one_call(sc, True, False, None, None, None, head_only=True)
    compare(sc, r, got, st, True, "head only")
    for k in KEYS:
        assert torch.equal(got[2][k], sc["inp"][k]), k


@pytest.mark.parametrize("absent", ["learner", "tracker"])
def test_one_controller_absent(pkg, absent):
    sc = scene(pkg, 20)
    out_t = None if absent == "tracker" else sc["out_t"]
    out_l = None if absent == "learner" else sc["out_l"]
    r = reference(pkg, sc, False, None, out_t, out_l)
    missing = torch.as_tensor(PHASE0 == (1 if absent == "learner" else 0), device="cuda")
    assert bool((r["n_fail"][missing] == 1).all()) and 0 < int(missing.sum()) < B
    got, st = one_call(sc, True, False, None, out_t, out_l)
    compare(sc, r, got, st, True, absent)


# ---------------------------------------------------------------- 3. a car is nobody's neighbour
def test_a_car_is_nobodys_neighbour(pkg):
    sc = scene(pkg, 20)
    L = sc["L"]
    got, st = one_call(sc, True, True, None, sc["out_t"], sc["out_l"])
    ring = ring_state(sc["learner"])
    perm = np.random.default_rng(5).permutation(B)          # new car j is old car perm[j]
    pt = torch.as_tensor(perm, device="cuda")
    # the permuted batch, recorders included: the same pre-feed with the cars' columns permuted
    learner = sc["learner"]
    learner.fleet_ss_create(B, CAP)
    rng = np.random.default_rng(11)
    for j in range(max(len(c[1]) for c in CASES)):
        act = np.array([j < len(CASES[c][1]) for c in CASE], dtype=np.int32)
        s = np.array([(sc["s0"][b] if CASES[c][1][j] == "s0" else CASES[c][1][j] * L) if act[b] else 0.0 for b, c in enumerate(CASE)])
        x = np.concatenate([s[None, :], rng.normal(size=(5, B))])
        u, k = rng.normal(size=(2, B)), rng.normal(size=B)
        learner.fleet_ss_record(torch.as_tensor(x[:, perm].copy(), **F64), torch.as_tensor(u[:, perm].copy(), **F64),
                                torch.as_tensor(k[perm].copy(), **F64), 0.025 * j, L, active=torch.as_tensor(act[perm].copy(), device="cuda"))
    stp = fresh_state(learner, PHASE0[perm], N_LEARN0[perm])
    take = lambda d: {k: (v[..., pt].contiguous() if torch.is_tensor(v) else v) for k, v in d.items()}
    inp2, x2, u2 = take(sc["inp"]), sc["x"][:, pt].contiguous(), sc["u_prev"][:, pt].contiguous()
    dist, exc, nf = torch.zeros(B, **F64), torch.zeros(B, **F64), torch.zeros(B, dtype=torch.int64, device="cuda")
    advance(sc, stp, x2, u2, inp2, take(sc["out_t"]), take(sc["out_l"]), restart_failed=True, distance=dist, worst_excess=exc, n_fail=nf)
    torch.cuda.synchronize()
    assert torch.equal(x2, got[0][:, pt]) and torch.equal(u2, got[1][:, pt])
    for k in KEYS:
        assert torch.equal(inp2[k], got[2][k][..., pt]), k
    assert torch.equal(dist, got[3][pt]) and torch.equal(exc, got[4][pt]) and torch.equal(nf, got[5][pt])
    for k in ("phase", "n_learn", "lap_time", "lap_kind", "x_ic", "query"):
        assert torch.equal(stp[k], st[k][..., pt]), k
    assert torch.equal(stp["counters"], st["counters"])
    ringp = ring_state(learner)
    for key in ("laps_in_ring", "lap_count", "n_dropped", "last_lap_time"):
        assert np.array_equal(ringp[key], ring[key][perm]), key
    for j in range(B):
        a, w = ringp["laps"][j], ring["laps"][perm[j]]
        assert len(a) == len(w), j
        for la, lw in zip(a, w):
            assert all(np.array_equal(p, q) for p, q in zip(la, lw)), j


# ---------------------------------------------------------------- 4. refusals
def test_refusals_write_nothing(pkg):
    sc = scene(pkg, 20)
    learner, tracker = sc["learner"], sc["tracker"]
    prefeed(learner, sc["s0"], sc["L"])
    st = fresh_state(learner)
    inp2, x2, u2 = clone(sc["inp"]), sc["x"].clone(), sc["u_prev"].clone()
    nf = torch.zeros(B, dtype=torch.int64, device="cuda")
    keep = (clone(inp2), x2.clone(), u2.clone(), clone(st), nf.clone())
    ring0 = ring_state(learner)
    ot, ol = sc["out_t"], sc["out_l"]

    def refused(code, inp=inp2, out_t=ot, out_l=ol, state=st, x=x2, solver=learner, trk=None, **kw):
        args = dict(dt=DT, dt_sim=DT / 2, n_sub=2, t=T_CALL, speed_scale=SPEED, speed_limit=(6.0, 3.0), warm_laps=WARM, learn_laps=LEARN, n_fail=nf)
        args.update(kw)
        with pytest.raises(pkg.LmpcError, match="-> %d:" % code) as e:
            solver.fleet_loop_advance(trk or sc["trk"], inp, out_t, out_l, x, u2, state, **args)
        assert len(str(e.value).split(":", 1)[1].strip()) > 0      # a message in lmpc_last_error
        torch.cuda.synchronize()

    refused(-1, solver=tracker)                                             # no fleet store
    refused(-1, x=x2[:, :64].contiguous())                                  # a batch other than the store's
    for key in ("X_ref", "vel_ref"):
        refused(-1, inp={k: v for k, v in inp2.items() if k != key})        # a null required pointer
    for key in ("phase", "counters", "query", "lap_time"):
        refused(-1, state={k: v for k, v in st.items() if k != key})
    refused(-1, trk=dict(sc["trk"], L=0.0))                                 # a bad track
    refused(-1, out_t={k: v for k, v in ot.items() if k != "status"})       # two members of a triple
    refused(-1, out_l={"X_optm": ol["X_optm"]})                             # one member of a triple
    refused(-1, dt=0.0)
    refused(-1, dt_sim=-1.0)
    refused(-1, n_sub=0)
    refused(-1, warm_laps=0)
    refused(-1, learn_laps=0)
    refused(-1, n_rec=0)                                                    # (the lap book itself is valid)
    refused(-1, plant=dict(pkg.presets.barc_vehicle(), model_id=1))
    refused(-1, plant=dict(pkg.presets.barc_vehicle(), integrator=7))
    refused(-1, inp=dict(inp2, X_ref=ot["X_optm"]))                         # references aliasing a solution
    refused(-1, inp=dict(inp2, U_ref=ol["U_optm"]))
    learner.set_output_layout("aos")
    try:
        refused(-3)
    finally:
        learner.set_output_layout("soa")
    for a, w in zip((inp2, x2, u2, st, nf), keep):
        if isinstance(a, dict):
            assert all(torch.equal(a[k], w[k]) for k in a if torch.is_tensor(a[k]))
        else:
            assert torch.equal(a, w)
    ring1 = ring_state(learner)
    for key in ("laps_in_ring", "lap_count", "n_dropped", "last_lap_time"):
        assert np.array_equal(ring0[key], ring1[key]), key
    assert all(len(a) == len(w) and all(all(np.array_equal(p, q) for p, q in zip(la, lw)) for la, lw in zip(a, w))
               for a, w in zip(ring1["laps"], ring0["laps"]))
    # and the same arguments unrefused go through
    learner.fleet_loop_advance(sc["trk"], inp2, ot, ol, x2, u2, st, dt=DT, dt_sim=DT / 2, n_sub=2, t=T_CALL, speed_scale=SPEED,
                               speed_limit=(6.0, 3.0), warm_laps=WARM, learn_laps=LEARN, n_fail=nf)
    torch.cuda.synchronize()
    assert not torch.equal(x2, keep[1])


# ---------------------------------------------------------------- 5, 6. whole runs
def experiment_x0(B_):
    """x0 of test_gpu_fleet_ss.experiment_x0, for B_ cars."""
    rng = np.random.default_rng(0)
    x0 = np.stack([np.full(B_, 0.5), rng.uniform(-0.05, 0.05, B_), np.zeros(B_), np.full(B_, 2.0), np.zeros(B_), np.zeros(B_)])
    x0[:, 0] = [0.5, 0.0, 0.0, 2.0, 0.0, 0.0]
    return x0


def solvers(pkg, N=20, ring=3):
    return (pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0),
            pkg.Solver(pkg.presets.barc_lmpc(N, ring), pkg.presets.barc_vehicle(), device=0))


def test_sixty_periods_equal_run_lmpc_fleet(pkg):
    tr = pkg.workloads.synthetic_track("barc")
    x0 = torch.as_tensor(experiment_x0(B), device="cuda")
    u0 = torch.zeros((2, B), **F64)
    res = {}
    for fused in (True, False):
        tracker, learner = solvers(pkg)
        fn = pkg.closed_loop.run_lmpc_fleet_fused if fused else pkg.closed_loop.run_lmpc_fleet
        res[fused] = fn(tracker, learner, tr, x0, u0, max_steps=60, **({"poll": 1} if fused else {}))
        torch.cuda.synchronize()
        tracker.close(), learner.close()
    a, b = res[True], res[False]
    assert a["steps"] == b["steps"] == 60
    assert torch.equal(a["n_fail"], b["n_fail"])
    # (the last knot's ulp reaches the plant through the next solves: the runs agree to rounding, as test_closed_loop_fused_equals_unfused)
    sx = torch.tensor([2000.0, 10.0, 0.1, 80.0, 2.0, 2.0], **F64)[:, None]
    same = (a["n_fail"] == 0) & (b["n_fail"] == 0)
    err = float((((a["x"] - b["x"]) / sx).abs()[:, same]).max())
    print("fused vs run_lmpc_fleet, 60 periods: final states %.1e (scaled), cars without a failed solve %d of %d" % (err, int(same.sum()), B))
    assert int(same.sum()) > 0 and err < 1e-9
    tracker, learner = solvers(pkg)
    other_n = pkg.Solver(pkg.presets.barc_lmpc(12, 3), pkg.presets.barc_vehicle(), device=0)
    other_v = pkg.Solver(pkg.presets.barc_lmpc(20, 3), low_mu(pkg), device=0)
    for bad in (other_n, other_v):
        with pytest.raises(ValueError):
            pkg.closed_loop.run_lmpc_fleet_fused(tracker, bad, tr, x0, u0, max_steps=1)
    for sv in (tracker, learner, other_n, other_v):
        sv.close()


def periods(times):
    return [int(round(v / DT)) for v in times]


def test_the_experiment(pkg):
    tr = pkg.workloads.synthetic_track("barc")
    x0 = torch.as_tensor(np.repeat(experiment_x0(64)[:, :1], 64, axis=1), device="cuda")
    u0 = torch.zeros((2, 64), **F64)
    kw = dict(warm_laps=1, learn_laps=1, warm_speed_scale=0.7)
    def run(fn, **more):
        tracker, learner = solvers(pkg)
        out = fn(tracker, learner, tr, x0, u0, **kw, **more)
        torch.cuda.synchronize()
        tracker.close(), learner.close()
        return out

    ref = run(pkg.closed_loop.run_lmpc_fleet)
    res = run(pkg.closed_loop.run_lmpc_fleet_fused, poll=1, record_trace=True)
    print("run_lmpc_fleet car 0", periods(ref["lap_times"][0]), ref["lap_kind"][0], "steps", ref["steps"],
          "| fused car 0", periods(res["lap_times"][0]), res["lap_kind"][0], "steps", res["steps"])
    assert ref["lap_kind"][0] == ["tracking", "lmpc"]
    differ = 0
    for b in range(64):
        assert res["lap_kind"][b] == ref["lap_kind"][b] and len(res["lap_times"][b]) == len(ref["lap_times"][b]), b
        assert res["lap_times"][b] == res["lap_times"][0] and res["lap_kind"][b] == res["lap_kind"][0], b
        for j, (p, q) in enumerate(zip(periods(res["lap_times"][b]), periods(ref["lap_times"][b]))):
            if p != q:
                differ += b == 0      # (counted once: every car of the fused run is asserted equal to car 0 just above)
                print("car", b, "lap", j, "fused", p, "run_lmpc_fleet", q)
            assert abs(p - q) <= 1, (b, j, p, q)
    assert differ < 2
    assert torch.equal(res["laps_in_ring"], ref["laps_in_ring"]) and int(res["n_dropped"].sum()) == 0
    assert len(res["trace"]) == res["steps"] and res["trace"][1][3] == DT
    # poll = 16: every car still gets its learning lap, none before its ring held warm_laps, and the run ends at most 16 periods late
    slow = run(pkg.closed_loop.run_lmpc_fleet_fused, poll=16)
    print("poll 16 car 0", periods(slow["lap_times"][0]), slow["lap_kind"][0], "steps", slow["steps"])
    for b in range(64):
        kinds = slow["lap_kind"][b]
        assert kinds.count("lmpc") >= 1, b
        assert kinds[:kw["warm_laps"]] == ["tracking"] * kw["warm_laps"], (b, kinds)
    assert slow["steps"] <= res["steps"] + 16
