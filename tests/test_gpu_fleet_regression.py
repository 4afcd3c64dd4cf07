"""Per-car error-dynamics regression on the fleet safe set (lmpc_fleet_ss_set_regression / lmpc_fleet_ss_regress_batch,
csrc/lmpc_fleet_reg_kernel.hip) against the CPU restatement.  Needs an MI355X.

The reference for car b is always oracle.regression.regress_batch on fleet_ss_get_laps(b) -- what the device holds for that car at
that moment -- at the bound tests/test_gpu_regression.py holds the shared kernel to: 1e-9 (1 + max|ref|) on A, B and g of every
(car, stage); a query the oracle finds no candidate for comes back bit-identical.  Stores are small (R = 3 laps of at most C = 64
samples per car).  Laps are test_regression_oracle's synthetic_lap / planted_pairs where the features are the bench's (speeds, yaw
rate, inputs); where the abscissa is among the features ((8, 6), the IAC-scale case) no query comes within reach of those, and the
laps are noisy copies of the car's own reference, as test_gpu_regression._long_laps builds them for its IAC cases.

How wide that noise and the bandwidth are was chosen on the CPU from the ORACLE'S OWN reproducibility, before any kernel ran: the
ridge system carries the abscissa next to the intercept, and where all samples inside the bandwidth sit within centimetres of each
other at s ~ 10^3 m its condition number is 10^8 and more -- oracle.regression.regress and regress_batch, the same arithmetic summed
in another order, then differ by up to 4e-8 of 1 + max|ref| on the BARC (8, 6) cases and 6e-9 on the IAC case (measured with the
noise test_gpu_regression._long_laps uses, centimetres, and dist_max 0.6), which no comparison at 1e-9 can resolve.  With the samples spread over the bandwidth (NEAR_NOISE; on the
IAC track metres and m/s at 60 m/s, dist_max 4) the two differ by 7e-12 (BARC) and 2e-11 (IAC); every case asserts that on a few
of its own queries at 1e-10, an order below the kernel's bound."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import params as P, qp as Q, regression as R, scenario as S
from oracle.dynamics import rk4
from test_regression_oracle import planted_pairs, synthetic_lap
from tolerances import TOL_TWIN

pytestmark = pytest.mark.gpu

RING, CAP = 3, 64
BENCH_SPEC = ((3, 4, 5), (0, 1), (3, 4, 5))
SPEC_1234 = ((1, 2, 3, 4), (1,), (3, 4, 5))
SPEC_01234 = ((0, 1, 2, 3, 4), (), (2, 4, 5))
SPEC_ALL = ((0, 1, 2, 3, 4, 5), (0, 1), (0, 1, 2, 3, 4, 5))
# standard deviations of the samples around the car's reference, state and input (see the module's note)
NEAR_NOISE = {"barc": ([0.15] * 6, [0.15, 0.15]), "iac": ([1.0, 0.5, 0.05, 1.0, 0.5, 0.05], [0.5, 0.02])}
GAIN = np.array([[0.02, 0.0, 0.01, 0.5, 0.0, 0.001], [0.0, -0.03, 0.0, 0.0, 0.02, 0.0], [0.01, 0.0, 0.0, 0.0, 0.1, -0.002]])


def _setup(pkg, kind, N, B, seed=31):
    """Cold-start inputs (oracle) of B problems on the BARC or the IAC (putnam) track -- the linearisation points -- and a solver with a
    fleet store for them."""
    if kind == "barc":
        veh, cfg, tr = P.barc_vehicle(), P.barc_tracking_mpc(N), pkg.workloads.synthetic_track("barc")
        u_lo, u_hi, _, _ = Q.effective_bounds(cfg, veh)
        x, u = pkg.workloads.sample_initial_states("barc", B, tr["L"], u_lo, u_hi, seed)
        sv = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
    else:
        veh, cfg, tr = P.iac_vehicle(), P.iac_tracking_mpc(N), pkg.workloads.synthetic_track("putnam")
        x, u = pkg.workloads.sample_initial_states("putnam", B, tr["L"], [-10.0, -0.314159], [5.0, 0.314159], seed=seed)
        sv = pkg.Solver(pkg.presets.iac_tracking_mpc(N), pkg.presets.iac_vehicle(), device=0)
    inp = S.cold_start_inputs(cfg, veh, tr, x, u, 0.025)
    assert int(sv.config["max_lap_stored"]) == RING
    sv.fleet_ss_create(B, CAP)
    return veh, tr, inp, sv


def _monotone(lap, L):
    """The lap with an abscissa the recorder can follow: rising from 0.1 to L - 0.1."""
    x, u, k, t = lap
    x = x.copy()
    x[:, 0] = np.linspace(0.1, L - 0.1, x.shape[0])
    return x, u, k, t


def _near_lap(inp, tr, b, n, rng, kind="barc"):
    """n noisy samples of car b's own reference, non-uniform time stamps."""
    NS = inp["U_ref"].shape[1]
    idx = rng.integers(0, NS, n)
    x = inp["X_ref"][:, idx, b].T + rng.normal(0, 1, (n, 6)) * np.array(NEAR_NOISE[kind][0])
    u = inp["U_ref"][:, idx, b].T + rng.normal(0, 1, (n, 2)) * np.array(NEAR_NOISE[kind][1])
    return x, u, S.track_lookup(tr["curvature"], x[:, 0], tr["L"]), np.cumsum(rng.uniform(0.02, 0.04, n))


def _feed(sv, B, L, seqs, t0=0.0):
    """seqs: {car: (x [n, 6], u [n, 2], k [n])}.  Call i hands sample i of every car that still has one to the recorder."""
    for i in range(max(s[0].shape[0] for s in seqs.values())):
        x, u, k, act = np.zeros((6, B)), np.zeros((2, B)), np.zeros(B), np.zeros(B, dtype=np.int32)
        for b, (sx, su, sk) in seqs.items():
            if i < sx.shape[0]:
                x[:, b], u[:, b], k[b], act[b] = sx[i], su[i], sk[i], 1
        sv.fleet_ss_record(x, u, k, t0 + 0.03 * i, L, active=act)


def _rec_seq(lap, L, seed, close):
    """What the recorder is handed for one lap (abscissa rising): in front a sample just before the line (`seed`: a car whose
    recorder has seen nothing -- it only seeds the abscissa, and the lap's first sample is then the crossing that starts recording);
    behind it (`close`) a sample just past the line, which closes the lap and opens the next."""
    x, u, k, _ = lap
    xs, us, ks = [x], [u], [k]
    if seed:
        first = x[:1].copy()
        first[0, 0] = L - 0.05
        xs, us, ks = [first] + xs, [u[:1]] + us, [k[:1]] + ks
    if close:
        last = x[-1:].copy()
        last[0, 0] = 0.05
        xs, us, ks = xs + [last], us + [u[-1:]], ks + [k[-1:]]
    return np.concatenate(xs), np.concatenate(us), np.concatenate(ks)


def _flat(a):
    """[..., N-1, B] -> [B, N-1, ...]"""
    return np.ascontiguousarray(np.moveaxis(a, (-1, -2), (0, 1)))


def _oracle(veh, laps, spec, h, as_written, inp, b, A0, B0, g0):
    """oracle.regression on car b's queries against `laps`: (A, B, g [N-1, ...], touched [N-1]); laps of one sample hold no sample
    with a successor and are left out, no lap at all touches nothing."""
    N = inp["X_ref"].shape[1]
    laps = [l for l in laps if l[0].shape[0] >= 2]
    a0, b0, c0 = _flat(A0)[b], _flat(B0)[b], _flat(g0)[b]
    if not laps:
        return a0, b0, c0, np.zeros(N - 1, dtype=bool)
    qx, qu = inp["X_ref"][:, :N - 1, b].T.copy(), inp["U_ref"][:, :, b].T.copy()
    return R.regress_batch(veh, laps, spec[0], spec[1], spec[2], h, qx, qu, a0, b0, c0, as_written=as_written)


def _rel(got, ref):
    n = ref.shape[0]
    return np.abs(got - ref).reshape(n, -1).max(axis=1) / (1 + np.abs(ref).reshape(n, -1).max(axis=1))


def _regress(sv, inp, lin=None):
    A0, B0, g0 = lin if lin is not None else sv.linearize(inp)
    A, Bm, g = sv.fleet_ss_regress(inp, A0.clone(), B0.clone(), g0.clone())
    return tuple(t.cpu().numpy() for t in (A0, B0, g0)), tuple(t.cpu().numpy() for t in (A, Bm, g))


def _check_against_oracle(sv, veh, inp, spec, h, as_written, lin, res, what, laps_of=None):
    """Every car against the oracle on ITS laps as the device holds them.  Returns (touched [B, N-1], per-car laps)."""
    B = inp["X_ref"].shape[2]
    (A0, B0, g0), (A, Bm, g) = lin, res
    fa, fb, fg = _flat(A), _flat(Bm), _flat(g)
    worst, touched_all, held = 0.0, [], []
    for b in range(B):
        laps = sv.fleet_ss_get_laps(b) if laps_of is None else laps_of[b]
        held.append(laps)
        Ar, Br, gr, touched = _oracle(veh, laps, spec, h, as_written, inp, b, A0, B0, g0)
        for got, ref in ((fa[b], Ar), (fb[b], Br), (fg[b], gr)):
            e = _rel(got, ref)
            worst = max(worst, float(e.max()))
            assert e.max() < 1e-9, (what, b, int(np.argmax(e)), float(e.max()))
            assert np.array_equal(got[~touched], ref[~touched]), (what, b)     # untouched: the same bits
        touched_all.append(touched)
    touched_all = np.stack(touched_all)
    # the reference reproduces itself an order below the bound on this data: the per-query oracle against the vectorised one
    tq = np.argwhere(touched_all)
    for b, i in tq[np.linspace(0, len(tq) - 1, 4).astype(int)] if len(tq) else []:
        a1, b1, c1 = R.regress(veh, [l for l in held[b] if l[0].shape[0] >= 2], spec[0], spec[1], spec[2], h, inp["X_ref"][:, i, b],
                               inp["U_ref"][:, i, b], A0[:, :, i, b], B0[:, :, i, b], g0[:, i, b], as_written=as_written)
        Ar, Br, gr, _ = _oracle(veh, held[b], spec, h, as_written, inp, b, A0, B0, g0)
        for ref, other in ((a1, Ar[i]), (b1, Br[i]), (c1, gr[i])):
            assert np.abs(ref - other).max() <= 1e-10 * (1 + np.abs(ref).max()), (what, int(b), int(i))
    print("%s: %d queries, %d touched, worst %.1e relative to 1 + max|ref|" % (what, touched_all.size, touched_all.sum(), worst))
    return touched_all, held


# ---- 1. every car against its own laps ----------------------------------------------------------------------------------------------
def _fleet_of_37(sv, veh, tr, inp, near, rng, kind="barc"):
    """Loads 37 cars one by one with different laps and returns {role: car}.  Cars 0-4 are the special ones, 5-8 are trimmed to the
    four table paddings, the rest hold one to three laps of 8 to 64 samples."""
    B, L = 37, float(tr["L"])
    lap = (lambda b, n: _near_lap(inp, tr, b, n, rng, kind)) if near else (lambda b, n: synthetic_lap(veh, n, int(rng.integers(1 << 30))))
    pairs = planted_pairs(veh, 12, 5, GAIN)
    for b in range(B):
        if b == 0:
            continue                                           # no lap
        if b == 1:
            laps = [lap(b, 2)] if near else pairs[:1]          # its only lap has two samples
        elif b == 2:
            laps = [lap(b, int(rng.integers(8, CAP + 1))) for _ in range(RING + 2)]     # the two oldest are evicted
        elif 5 <= b <= 8:
            laps = [lap(b, 20), lap(b, 17), lap(b, 30)]
            nvalid = sum(l[0].shape[0] - 1 for l in laps)
            cut = (nvalid - (4 - (b - 5)) % 4) % 4             # npad - nvalid = b - 5
            laps[-1] = tuple(a[:a.shape[0] - cut] for a in laps[-1])
        elif b in (9, 10) and not near:
            laps = pairs[3 * (b - 9) + 1:3 * (b - 9) + 4]      # three two-sample laps: three rows
        elif b == 11:
            laps = [lap(b, CAP) for _ in range(RING)]          # a full ring of full slots: the table's last row is in use
        else:
            laps = [lap(b, int(rng.integers(8, CAP + 1))) for _ in range(1 + b % RING)]
        sv.fleet_ss_load(laps, L, car=b)
    # car 3: an open lap of several samples on top of its closed ones; car 4: one lap longer than a slot, dropped at its close
    open_lap, long_lap = _monotone(synthetic_lap(veh, 9, 900), L), _monotone(synthetic_lap(veh, CAP + 5, 901), L)
    _feed(sv, B, L, {3: _rec_seq(open_lap, L, seed=True, close=False), 4: _rec_seq(long_lap, L, seed=True, close=True)})
    return B


ONE_BY_ONE = [
    # id, track, N, spec, laps near the car's reference, as_written, dist_max
    ("bench_n20", "barc", 20, BENCH_SPEC, False, False, 0.6),
    ("bench_n3_as_written", "barc", 3, BENCH_SPEC, False, True, 0.6),
    ("bench_n81", "barc", 81, BENCH_SPEC, False, False, 0.6),
    ("s1234_n20_as_written", "barc", 20, SPEC_1234, False, True, 0.6),
    ("s1234_n3", "barc", 3, SPEC_1234, False, False, 0.6),
    ("all_n20", "barc", 20, SPEC_ALL, True, False, 0.6),
    ("all_n81_as_written", "barc", 81, SPEC_ALL, True, True, 0.6),
    ("all_n3", "barc", 3, SPEC_ALL, True, False, 0.6),
    ("s01234_iac_n20", "iac", 20, SPEC_01234, True, False, 4.0),     # the abscissa of a 2.8 km lap among the features
]


@pytest.mark.parametrize("case", ONE_BY_ONE, ids=[c[0] for c in ONE_BY_ONE])
def test_every_car_is_regressed_on_its_own_laps(pkg, case):
    """37 cars loaded one by one: every table padding, a car with no lap, one whose only lap has two samples, one loaded with R + 2
    laps, one with an open lap on top (recorder), one whose over-long lap was dropped (recorder), a full ring of full slots.  N = 3,
    20 and 81 (two waves per car, the second with 16 live lanes), both instances, both signs, one IAC-scale case."""
    name, kind, N, spec, near, as_written, h = case
    rng = np.random.default_rng(sum(map(ord, name)))
    veh, tr, inp, sv = _setup(pkg, kind, N, 37)
    B = _fleet_of_37(sv, veh, tr, inp, near, rng, kind)
    sv.fleet_ss_set_regression(in_state=spec[0], in_ctrl=spec[1], out_rows=spec[2], dist_max=h, as_written=as_written)
    lin, res = _regress(sv, inp)
    touched, held = _check_against_oracle(sv, veh, inp, spec, h, as_written, lin, res, name)
    stats = {k: v.cpu().numpy() for k, v in sv.fleet_ss_stats(B).items()}
    sv.close()
    # the fixture is what it says
    rows = [sum(max(l[0].shape[0] - 1, 0) for l in laps) for laps in held]
    assert {(-r) % 4 for r in rows if r} == {0, 1, 2, 3}
    assert [(-rows[b]) % 4 for b in range(5, 9)] == [0, 1, 2, 3]
    assert held[0] == [] and [l[0].shape[0] for l in held[1]] == [2] and len(held[2]) == RING
    assert stats["lap_count"][2] == RING + 2 and rows[11] == RING * (CAP - 1)
    assert stats["n_dropped"][4] == 1 and stats["n_dropped"].sum() == 1 and len(held[4]) == 1 + 4 % RING
    assert not touched[0].any()
    assert touched.sum() >= touched.size // 10, (touched.sum(), touched.size)      # >= 10 % of the queries
    # car b's answer is not car b + 1's: the result on the neighbour's laps differs (an indexing slip a symmetric fixture would hide)
    (A0, B0, g0), (A, Bm, g) = lin, res
    with_data = [b for b in range(B - 1) if rows[b] and rows[b + 1]]
    differs = 0
    for b in with_data:
        Ar, _, gr, _ = _oracle(veh, held[b + 1], spec, h, as_written, inp, b, A0, B0, g0)
        differs += int(max(_rel(_flat(A)[b], Ar).max(), _rel(_flat(g)[b], gr).max()) > 1e-6)
    assert 3 * differs >= len(with_data), (differs, len(with_data))


# ---- 2. the ring moves on -----------------------------------------------------------------------------------------------------------
def test_the_ring_moves_on_and_a_reset_leaves_no_stamp(pkg):
    B, N, h, spec = 12, 20, 0.6, BENCH_SPEC
    veh, tr, inp, sv = _setup(pkg, "barc", N, B)
    L = float(tr["L"])
    n_laps = [1 + b % RING for b in range(B)]
    for b in range(B):
        sv.fleet_ss_load([synthetic_lap(veh, 20 + 3 * l + b, 100 * b + l) for l in range(n_laps[b])], L, car=b)
    sv.fleet_ss_set_regression(dist_max=h)
    lin = sv.linearize(inp)
    lin_np, res1 = _regress(sv, inp, lin)
    t1, held1 = _check_against_oracle(sv, veh, inp, spec, h, False, lin_np, res1, "loaded")
    # one more full lap for every other car, through the recorder: it closes a lap and, where the ring is full, evicts one
    _feed(sv, B, L, {b: _rec_seq(_monotone(synthetic_lap(veh, 40, 500 + b), L), L, seed=True, close=True) for b in range(0, B, 2)})
    _, res2 = _regress(sv, inp, lin)
    t2, held2 = _check_against_oracle(sv, veh, inp, spec, h, False, lin_np, res2, "one more lap for the even cars")
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
    t3, _ = _check_against_oracle(sv, veh, inp, spec, h, False, lin_np, res3, "reset and reloaded")
    for b in range(1, B, 2):
        assert not np.array_equal(res1[0][..., b], res3[0][..., b]), b
    sv.close()
    for t in (t1, t2, t3):
        assert t.sum() >= t.size // 10


# ---- 3. a new spec invalidates ------------------------------------------------------------------------------------------------------
def test_a_new_spec_or_sign_repacks_every_car(pkg):
    B, N, h = 9, 10, 0.6
    veh, tr, inp, sv = _setup(pkg, "barc", N, B)
    rng = np.random.default_rng(3)
    for b in range(B):
        sv.fleet_ss_load([_near_lap(inp, tr, b, 12 + 5 * l + b, rng) for l in range(1 + b % RING)], float(tr["L"]), car=b)
    lin = sv.linearize(inp)
    for spec, as_written in ((BENCH_SPEC, False), (BENCH_SPEC, True), (SPEC_ALL, True), (SPEC_ALL, False), (SPEC_1234, False)):
        sv.fleet_ss_set_regression(in_state=spec[0], in_ctrl=spec[1], out_rows=spec[2], dist_max=h, as_written=as_written)
        lin_np, res = _regress(sv, inp, lin)
        touched, _ = _check_against_oracle(sv, veh, inp, spec, h, as_written, lin_np, res, "spec %s as_written %s" % (spec[0], as_written))
        assert touched.sum() >= touched.size // 10
    sv.close()


# ---- 4. equal stores, equal answers -------------------------------------------------------------------------------------------------
def _plant_laps(veh, tr, n_laps=RING, n=60):
    """Laps driven by a plant with less grip and more mass than the model (rollouts, 30 ms steps, small random inputs)."""
    plant = dataclasses.replace(veh, mu=0.8 * veh.mu, m=1.1 * veh.m)
    laps = []
    for l in range(n_laps):
        rng = np.random.default_rng(40 + l)
        x = np.zeros((n, 6))
        x[0] = [1.0 + 3.0 * l, 0.0, 0.0, 1.5 + 0.2 * l, 0.0, 0.0]
        u = np.stack([rng.uniform(-0.005, 0.005, n), rng.uniform(-0.1, 0.1, n)], axis=1)
        k = np.zeros(n)
        for j in range(n):
            k[j] = S.track_lookup(tr["curvature"], x[j:j + 1, 0], tr["L"])[0]
            if j + 1 < n:
                x[j + 1] = rk4(x[j], u[j], float(k[j]), 0.03, plant)
        laps.append((x, u, k, np.arange(n) * 0.03))
    return laps


def test_equal_stores_give_the_shared_regression_and_the_same_solves(pkg):
    B, N, h = 16, 20, 0.6
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
    fleet.fleet_ss_set_regression(dist_max=h)
    shared.set_regression_laps(laps, dist_max=h)
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


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def _refused(pkg, code, call):
    with pytest.raises(pkg.capi.LmpcError, match=r"-> %d:" % code):
        call()


def test_refusals_leave_the_outputs_untouched(pkg):
    B, N = 8, 10
    veh, tr, inp, sv = _setup(pkg, "barc", N, B)
    small = {k: (np.ascontiguousarray(v[..., :B - 2]) if isinstance(v, np.ndarray) and v.ndim and v.shape[-1] == B else v) for k, v in inp.items()}
    laps = [synthetic_lap(veh, 30, 1)]
    sv.fleet_ss_load(laps, float(tr["L"]), car=-1)
    sv.fleet_ss_set_regression(dist_max=0.6)
    bytes_on = sv.fleet_ss_bytes()
    A0, B0, g0 = sv.linearize(small)
    marks = [t.clone() for t in (A0, B0, g0)]
    _refused(pkg, -1, lambda: sv.fleet_ss_regress(small, A0, B0, g0))                     # a batch other than the store's
    assert all(torch.equal(a, m) for a, m in zip((A0, B0, g0), marks))
    out = sv.alloc_outputs(B - 2)
    for key in ("X_optm", "U_optm", "dU_optm", "status", "iters"):
        out[key].fill_(7)
    _refused(pkg, -1, lambda: sv.solve(small, out))
    assert all(bool((out[key] == 7).all()) for key in ("X_optm", "U_optm", "dU_optm", "status", "iters"))
    kw = dict(dtype=torch.float32, device="cuda")
    out32 = {"X_optm": torch.full((6, N, B), 7.0, **kw), "U_optm": torch.full((2, N - 1, B), 7.0, **kw), "dU_optm": torch.full((2, N - 1, B), 7.0, **kw),
             "kkt": torch.full((4, B), 7.0, **kw), "status": torch.full((B,), 7, dtype=torch.int32, device="cuda"),
             "iters": torch.full((B,), 7, dtype=torch.int32, device="cuda")}
    _refused(pkg, -3, lambda: sv.solve_f32(inp, out32))                                   # the fp32 entry
    assert all(bool((out32[key] == 7).all()) for key in ("X_optm", "U_optm", "dU_optm", "status", "iters"))
    _refused(pkg, -1, lambda: sv.set_regression_laps(laps, dist_max=0.6))                 # both at once: shared on top of per-car
    _refused(pkg, -3, lambda: sv.fleet_ss_set_regression(in_state=(3, 4), in_ctrl=(0, 1)))   # (4, 3) is not built
    _refused(pkg, -1, lambda: sv.fleet_ss_set_regression(in_state=(3, 4, 6)))             # index out of range
    _refused(pkg, -1, lambda: sv.fleet_ss_set_regression(dist_max=0.0))
    assert sv.fleet_ss_bytes() == bytes_on                                                # a refused spec changes nothing
    full = sv.linearize(inp)
    sv.fleet_ss_regress(inp, *[t.clone() for t in full])                                  # ... and it is still on
    sv.fleet_ss_set_regression(off=True)
    assert sv.fleet_ss_bytes() < bytes_on
    _refused(pkg, -1, lambda: sv.fleet_ss_regress(inp, *full))                            # switched off
    sv.set_regression_laps(laps, dist_max=0.6)
    _refused(pkg, -1, lambda: sv.fleet_ss_set_regression(dist_max=0.6))                   # both at once: per-car on top of shared
    sv.set_regression_laps([])
    sv.fleet_ss_set_regression(dist_max=0.6)
    sv.fleet_ss_create(B, CAP)                                                            # replacing the store switches it off
    _refused(pkg, -1, lambda: sv.fleet_ss_regress(inp, *full))
    sv.fleet_ss_set_regression(dist_max=0.6)
    sv.fleet_ss_destroy()                                                                 # and so does destroying it
    _refused(pkg, -1, lambda: sv.fleet_ss_set_regression(dist_max=0.6))                   # no store
    _refused(pkg, -1, lambda: sv.fleet_ss_regress(inp, *full))
    assert all(torch.equal(a, m) for a, m in zip(full, sv.linearize(inp)))
    sv.solve(small)                                                                       # off: any batch solves again
    sv.close()


# ---- 6. closed loop -----------------------------------------------------------------------------------------------------------------
def _fleet_run(pkg, **kw):
    N, B = 20, 8
    tracker = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
    learner = pkg.Solver(pkg.presets.barc_lmpc(N, 3), pkg.presets.barc_vehicle(), device=0)
    tr = pkg.workloads.synthetic_track("barc")
    rng = np.random.default_rng(0)
    x0 = np.stack([np.full(B, 0.5), rng.uniform(-0.05, 0.05, B), np.zeros(B), np.full(B, 2.0), np.zeros(B), np.zeros(B)])
    res = pkg.closed_loop.run_lmpc_fleet(tracker, learner, tr, torch.as_tensor(x0, device="cuda"), torch.zeros((2, B), dtype=torch.float64, device="cuda"),
                                         warm_laps=1, learn_laps=1, warm_speed_scale=0.7, **kw)
    out = {"x": res["x"].cpu().numpy(), "lap_times": res["lap_times"], "n_fail": res["n_fail"].cpu().numpy(), "steps": res["steps"],
           "lap_kind": res["lap_kind"]}
    tracker.close()
    learner.close()
    return out


def test_closed_loop_with_an_empty_bandwidth_is_the_loop_without_regression(pkg):
    """dist_max = 1e-12: the kernels run every learning period and no sample is ever inside the bandwidth -- the same bits."""
    ref = _fleet_run(pkg)
    got = _fleet_run(pkg, regression={"dist_max": 1e-12})
    assert all("lmpc" in kinds for kinds in ref["lap_kind"])            # the learning controller (and with it the regression) ran
    assert got["steps"] == ref["steps"] and got["lap_times"] == ref["lap_times"]
    assert np.array_equal(got["x"], ref["x"]) and np.array_equal(got["n_fail"], ref["n_fail"])


def test_closed_loop_correction_reaches_the_qp_on_a_plant_with_less_grip(pkg):
    veh = dict(pkg.presets.barc_vehicle())
    veh["mu"] = 0.9 * veh["mu"]
    plant = pkg.Solver(pkg.presets.barc_tracking_mpc(20), veh, device=0)
    ref = _fleet_run(pkg, plant=plant)
    got = _fleet_run(pkg, plant=plant, regression={"dist_max": 0.6})
    plant.close()
    assert all("lmpc" in kinds for kinds in ref["lap_kind"])
    assert np.isfinite(got["x"]).all()
    assert np.abs(got["x"] - ref["x"]).max() > 1e-6
