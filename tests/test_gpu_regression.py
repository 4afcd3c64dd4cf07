"""Error-dynamics regression kernel (BASELINE config 5) against the CPU restatement.  Needs an MI355X."""
import dataclasses

import numpy as np
import pytest
import torch

import dense_cases as DC
from oracle import params as P, qp as Q, regression as R, scenario as S
from oracle.dynamics import rk4
from test_regression_oracle import perturbed_plant_laps, planted_pairs, synthetic_lap

pytestmark = pytest.mark.gpu


def recorded_laps(veh, n_laps=3, n=150):
    """Pseudo-laps with the statistics the feature space needs (speeds, yaw rates, inputs around a driving point)."""
    return [synthetic_lap(veh, n, 20 + l) for l in range(n_laps)]


@pytest.mark.parametrize("as_written", [False, True])
def test_regression_matches_the_restatement_on_A_B_g(pkg, as_written):
    veh, cfg = P.barc_vehicle(), P.barc_tracking_mpc(10)
    solver = pkg.Solver(pkg.presets.barc_tracking_mpc(10), pkg.presets.barc_vehicle(), device=0)
    tr = pkg.workloads.synthetic_track("barc")
    u_lo, u_hi, _, _ = Q.effective_bounds(cfg, veh)
    B = 24
    x, u = pkg.workloads.sample_initial_states("barc", B, tr["L"], u_lo, u_hi, 31)
    inp = S.cold_start_inputs(cfg, veh, tr, x, u, 0.025)
    laps = recorded_laps(veh)
    h = 0.6
    solver.set_regression_laps(laps, in_state=(3, 4, 5), in_ctrl=(0, 1), out_rows=(3, 4, 5), dist_max=h, as_written=as_written)
    A0, B0, g0 = solver.linearize(inp)
    A, Bm, g = solver.regress(inp, A0.clone(), B0.clone(), g0.clone())
    A0, B0, g0, A, Bm, g = (t.cpu().numpy() for t in (A0, B0, g0, A, Bm, g))
    n_touched = 0
    for b in range(0, B, 3):
        for i in range(cfg.N - 1):
            Ar, Br, gr = R.regress(veh, laps, (3, 4, 5), (0, 1), (3, 4, 5), h, inp["X_ref"][:, i, b], inp["U_ref"][:, i, b],
                                   A0[:, :, i, b], B0[:, :, i, b], g0[:, i, b], as_written=as_written)
            n_touched += int(np.abs(Ar - A0[:, :, i, b]).max() > 0)
            sc = 1.0 + np.abs(Ar).max()
            assert np.abs(A[:, :, i, b] - Ar).max() < 1e-9 * sc
            assert np.abs(Bm[:, :, i, b] - Br).max() < 1e-9 * (1.0 + np.abs(Br).max())
            assert np.abs(g[:, i, b] - gr).max() < 1e-9 * (1.0 + np.abs(gr).max())
    assert n_touched > 10  # the bandwidth actually catches lap samples on this workload


def test_regression_recovers_a_planted_error_model_and_enters_the_solve(pkg):
    veh = P.barc_vehicle()
    solver = pkg.Solver(pkg.presets.barc_tracking_mpc(10), pkg.presets.barc_vehicle(), device=0)
    tr = pkg.workloads.synthetic_track("barc")
    gain = np.array([[0.02, 0.0, 0.01, 0.5, 0.0, 0.001], [0.0, -0.03, 0.0, 0.0, 0.02, 0.0], [0.01, 0.0, 0.0, 0.0, 0.1, -0.002]])
    laps = planted_pairs(veh, 400, 5, gain)
    x = np.tile(np.array([1.0, 0.0, 0.0, 1.6, 0.0, 0.0]), (8, 1))
    inp = solver.prepare(tr, x.T.copy(), 0.025)
    inp["u_ic"] = torch.zeros((2, 8), dtype=torch.float64, device="cuda")
    base = solver.solve(inp)["X_optm"].cpu().numpy()
    solver.set_regression_laps(laps, dist_max=3.0)
    A0, B0, g0 = solver.linearize(inp)
    A, Bm, g = solver.regress(inp, A0.clone(), B0.clone(), g0.clone())
    dA = (A - A0).cpu().numpy()[3:, 3:6, 0, 0]
    assert np.allclose(dA, gain[:, :3], atol=2e-2)           # the planted error model, with its sign
    with_reg = solver.solve(inp)
    assert (with_reg["status"].cpu().numpy() == 0).all()
    assert np.abs(with_reg["X_optm"].cpu().numpy() - base).max() > 1e-6   # the corrected model reaches the QP
    solver.set_regression_laps([])
    assert np.abs(solver.solve(inp)["X_optm"].cpu().numpy() - base).max() == 0.0


def test_regression_reduces_the_one_step_error_of_a_perturbed_plant_on_the_device(pkg):
    """The default regression in front of the solve does what it is for: laps recorded on a plant with less
    grip and more mass, linearisation about recorded samples -- the corrected (A, B, g) predicts the plant's next state
    better than the nominal linearisation; the reference's literal signs (as_written) predict it worse."""
    veh = P.barc_vehicle()
    laps, plant = perturbed_plant_laps(veh)
    idx = list(range(0, 600, 25))
    B, N = len(idx), 3
    solver = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
    X = np.zeros((6, N, B)); U = np.zeros((2, N - 1, B)); K = np.zeros((N, B))
    for b, j in enumerate(idx):
        X[:, :, b] = laps[j][0][0][:, None]
        U[:, :, b] = laps[j][1][0][:, None]
        K[:, b] = laps[j][2][0]
    inp = {"X_ref": X, "U_ref": U, "T_ref": np.full((N - 1, B), 0.03), "curvatures": K}
    truth = np.stack([laps[j][0][1] for j in idx], axis=1)        # [6][B]

    def one_step_error(A, Bm, g):
        A, Bm, g = (t.cpu().numpy() for t in (A, Bm, g))
        pred = np.einsum("rcb,cb->rb", A[:, :, 0], X[:, 0]) + np.einsum("rcb,cb->rb", Bm[:, :, 0], U[:, 0]) + g[:, 0]
        return np.median(np.abs(pred - truth)[3:].max(axis=0))

    A0, B0, g0 = solver.linearize(inp)
    e0 = one_step_error(A0, B0, g0)
    solver.set_regression_laps(laps, dist_max=0.6)
    e1 = one_step_error(*solver.regress(inp, A0.clone(), B0.clone(), g0.clone()))
    solver.set_regression_laps(laps, dist_max=0.6, as_written=True)
    ew = one_step_error(*solver.regress(inp, A0.clone(), B0.clone(), g0.clone()))
    assert e1 < 0.4 * e0 and ew > 5 * e0, (e0, e1, ew)


# ---- lmpc_regress_kernel against oracle.regression on every (problem, stage) pair -------------------------------------------------
# feature specs: (in_state, in_ctrl, out_rows).  (5, 3) is the bench's and two others (one without controls, one with the abscissa);
# ALL is the (8, 6) instance.
BENCH_SPEC = ((3, 4, 5), (0, 1), (3, 4, 5))
SPEC_1234 = ((1, 2, 3, 4), (1,), (3, 4, 5))
SPEC_01234 = ((0, 1, 2, 3, 4), (), (2, 4, 5))
SPEC_ALL = ((0, 1, 2, 3, 4, 5), (0, 1), (0, 1, 2, 3, 4, 5))
REG_H = 0.6


def _queries(pkg, kind, N, B, seed):
    """Cold-start inputs (oracle) of B problems on the BARC or the IAC (putnam) track: the linearisation points."""
    if kind == "barc":
        veh, cfg, tr = P.barc_vehicle(), P.barc_tracking_mpc(N), pkg.workloads.synthetic_track("barc")
        x, u = pkg.workloads.sample_states_near_laps(DC.spec_laps(), B, tr["L"], seed=seed)
    else:
        veh, cfg, tr = P.iac_vehicle(), P.iac_tracking_mpc(N), pkg.workloads.synthetic_track("putnam")
        x, u = pkg.workloads.sample_initial_states("putnam", B, tr["L"], [-10.0, -0.314159], [5.0, 0.314159], seed=seed)
    return veh, cfg, tr, S.cold_start_inputs(cfg, veh, tr, x, u, 0.025)


def _trim_to_pad(laps, pad):
    """Shorten the last lap so that the kernel's sample table is padded by `pad` rows: npad - nvalid = pad (nvalid = samples that
    have a successor, npad = nvalid rounded up to a multiple of four)."""
    nvalid = sum(l[0].shape[0] - 1 for l in laps)
    cut = (nvalid - (4 - pad) % 4) % 4
    if cut and laps[-1][0].shape[0] == 2:    # two-sample laps: one valid sample each
        laps = laps[:-cut]
    elif cut:
        x, u, k, t = laps[-1]
        assert x.shape[0] - cut >= 2
        laps[-1] = (x[:-cut], u[:-cut], k[:-cut], t[:-cut])
    nvalid = sum(l[0].shape[0] - 1 for l in laps)
    assert (-nvalid) % 4 == pad
    return laps


def _long_laps(kind, inp, tr, N, rng):
    """Long laps with non-uniform time stamps.  BARC: the committed spec laps' states with small random inputs.  IAC: the reference
    rollouts of the first half of the batch's problems (the first one as it is -- its queries sit ON samples, where the expanded
    distance cancels worst at s ~ 10^3 m -- the others with noise); the second half of the batch has no sample in the bandwidth."""
    laps = []
    if kind == "barc":
        for x in DC.spec_laps():
            n = x.shape[0]
            u = np.stack([rng.uniform(-0.005, 0.005, n), rng.uniform(-0.1, 0.1, n)], axis=1)
            k = S.track_lookup(tr["curvature"], x[:, 0], tr["L"])
            laps.append((x.copy(), u, k, np.cumsum(rng.uniform(0.02, 0.04, n))))
        return laps
    B = inp["x_ic"].shape[1]
    for b in range(max(1, B // 2)):
        n = N if B > 1 else N // 2
        x = inp["X_ref"][:, :n, b].T.copy()
        u = np.concatenate([inp["U_ref"][:, :, b].T, inp["U_ref"][:, -1:, b].T])[:n].copy()
        if b > 0:
            x += rng.normal(0, 1, x.shape) * np.array([0.05, 0.03, 0.005, 0.05, 0.03, 0.01])
            u += rng.normal(0, 1, u.shape) * np.array([0.05, 0.005])
        k = S.track_lookup(tr["curvature"], x[:, 0], tr["L"])
        laps.append((x, u, k, np.cumsum(rng.uniform(0.018, 0.032, n))))
    if B == 1:   # a second, noisy pass over the same knots
        x, u, k, t = laps[0]
        laps.append((x + rng.normal(0, 0.02, x.shape), u + rng.normal(0, 0.002, u.shape), k, t))
    return laps


def _pair_laps(pkg, tr, veh, rng):
    """The bench's two-sample laps (workloads.regression_sample_pairs) around the stored spec laps, successors from a CPU plant: the
    oracle's RK4 with 15 % less grip."""
    plant = dataclasses.replace(veh, mu=0.85 * veh.mu)

    def step(xa, ua):
        return rk4(xa, ua, S.track_lookup(tr["curvature"], xa[:, 0], tr["L"]), 0.03, plant)

    return pkg.workloads.regression_sample_pairs(tr, DC.spec_laps()[:3], step, seed=int(rng.integers(1 << 30)))


REG_OP_CASES = [
    # id, track, N, B, spec, data, npad - nvalid, as_written, dist_max, the instance's EXACT flag (DC.reg_exact)
    ("bench_barc_n10_b1_long", "barc", 10, 1, BENCH_SPEC, "long", 0, False, REG_H, False),
    ("bench_barc_n41_b37_pairs", "barc", 41, 37, BENCH_SPEC, "pairs", 1, True, REG_H, False),
    ("s1234_barc_n20_b29_long", "barc", 20, 29, SPEC_1234, "long", 2, False, REG_H, False),
    ("s01234_iac_n81_b1_long", "iac", 81, 1, SPEC_01234, "long", 3, True, REG_H, True),
    ("s01234_iac_n10_b40_long", "iac", 10, 40, SPEC_01234, "long", 1, False, REG_H, True),
    ("all_iac_n20_b45_long", "iac", 20, 45, SPEC_ALL, "long", 0, False, REG_H, True),
    ("all_iac_n41_b1_long", "iac", 41, 1, SPEC_ALL, "long", 2, True, REG_H, True),
    ("all_barc_n3_b100_pairs", "barc", 3, 100, SPEC_ALL, "pairs", 3, False, REG_H, True),
    ("all_barc_n81_b5_long", "barc", 81, 5, SPEC_ALL, "long", 1, True, REG_H, True),
    # the (8, 6) instance with screened weights: BARC features (s <= 15.6) within 16 dist_max
    ("all_barc_n20_b37_pairs_h15", "barc", 20, 37, SPEC_ALL, "pairs", 0, False, 1.5, False),
    ("all_barc_n41_b3_long_h15", "barc", 41, 3, SPEC_ALL, "long", 2, True, 1.5, False),
]


@pytest.mark.parametrize("case", REG_OP_CASES, ids=[c[0] for c in REG_OP_CASES])
def test_regression_kernel_matches_the_oracle_on_every_problem_and_stage(pkg, case):
    """Solver.regress (lmpc_regress_kernel<NF, NOUT, false>) against oracle.regression on EVERY (problem, stage) pair, A, B and g, at
    1e-9 (1 + max|ref|); a query the oracle finds no candidate for comes back bit-identical.  The matrix: both instances ((5, 3) with
    three feature lists, (8, 6)) with screened and with exact weights, BARC and IAC scales, N = 3 .. 81, one problem and batches whose B (N - 1) queries are not a multiple
    of the 64-lane workgroup, long laps with non-uniform time stamps and the bench's two-sample laps, every table padding, both signs."""
    name, kind, N, B, (ins, inc, outs), data, pad, as_written, h, exact = case
    rng = np.random.default_rng(sum(map(ord, name)))
    veh, cfg, tr, inp = _queries(pkg, kind, N, B, seed=3)
    laps = _long_laps(kind, inp, tr, N, rng) if data == "long" else _pair_laps(pkg, tr, veh, rng)
    laps = _trim_to_pad(laps, pad)
    assert DC.reg_exact(laps, (ins, inc, outs), h) == exact   # the instance lmpc_set_regression_laps selects for this data
    pv = pkg.presets.barc_vehicle() if kind == "barc" else pkg.presets.iac_vehicle()
    pc = pkg.presets.barc_tracking_mpc(N) if kind == "barc" else pkg.presets.iac_tracking_mpc(N)
    sv = pkg.Solver(pc, pv, device=0)
    sv.set_regression_laps(laps, in_state=ins, in_ctrl=inc, out_rows=outs, dist_max=h, as_written=as_written)
    A0, B0, g0 = sv.linearize(inp)
    A, Bm, g = sv.regress(inp, A0.clone(), B0.clone(), g0.clone())
    sv.close()
    # [6, 6, N-1, B] -> [(b, i), 6, 6]
    A0, B0, g0, A, Bm, g = (t.cpu().numpy() for t in (A0, B0, g0, A, Bm, g))
    flat = lambda a: np.ascontiguousarray(np.moveaxis(a, (-1, -2), (0, 1)).reshape(B * (N - 1), *a.shape[:-2]))
    qx = flat(inp["X_ref"][:, : N - 1, :])
    qu = flat(inp["U_ref"])
    Ar, Br, gr, touched = R.regress_batch(veh, laps, ins, inc, outs, h, qx, qu, flat(A0), flat(B0), flat(g0), as_written=as_written)
    A, Bm, g, A0 = flat(A), flat(Bm), flat(g), flat(A0)
    # the vectorised oracle is the per-query one on touched queries: only the summation order differs, which the ridge system's
    # conditioning amplifies to 3e-10 on the IAC queries that sit on samples -- held to the bound the kernel is held to
    tq = np.nonzero(touched)[0]
    for o in tq[np.linspace(0, tq.size - 1, 4).astype(int)]:
        a1, b1, c1 = R.regress(veh, laps, ins, inc, outs, h, qx[o], qu[o], A0[o], flat(B0)[o], flat(g0)[o], as_written=as_written)
        for ref, got in ((a1, Ar[o]), (b1, Br[o]), (c1, gr[o])):
            assert np.abs(ref - got).max() <= 1e-9 * (1 + np.abs(ref).max()), (name, int(o))
    eA = np.abs(A - Ar).max(axis=(1, 2)) / (1 + np.abs(Ar).max(axis=(1, 2)))
    eB = np.abs(Bm - Br).max(axis=(1, 2)) / (1 + np.abs(Br).max(axis=(1, 2)))
    eg = np.abs(g - gr).max(axis=1) / (1 + np.abs(gr).max(axis=1))
    e = np.maximum(np.maximum(eA, eB), eg)
    worst = int(np.argmax(e))
    print("%s: %d queries, %d touched, %d samples; kernel vs oracle (relative to 1 + max|ref|) worst %.1e at (problem %d, stage %d)"
          % (name, touched.size, touched.sum(), sum(l[0].shape[0] - 1 for l in laps), e.max(), worst // (N - 1), worst % (N - 1)))
    assert touched.sum() >= max(min(10, N - 1), touched.size // 10), touched.sum()   # >= 10 % of the queries
    assert e.max() < 1e-9, (name, worst // (N - 1), worst % (N - 1), eA[worst], eB[worst], eg[worst])
    far = ~touched
    assert np.array_equal(A[far], A0[far]) and np.array_equal(Bm[far], flat(B0)[far]) and np.array_equal(g[far], flat(g0)[far])
    if kind == "iac" and B > 1:
        assert far.sum() >= B * (N - 1) // 4, far.sum()    # the second half of the batch has no sample in the bandwidth
