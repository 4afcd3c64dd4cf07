"""The problem sets behind tests/golden/dense_*.npz (>= 512 dense optima per BASELINE config, compared with
the KERNEL directly).  Shared by the generator (tests/golden/make_dense_fixtures.py), the CPU test (twin against the fixtures,
tests/test_dense_fixtures.py) and the GPU test (kernel against the fixtures, tests/test_gpu_dense_fixtures.py).

A fixture stores what is expensive -- the dense, polished, KKT-certified optimum of every problem (oracle/qp.py) -- and a digest
of the inputs; the inputs themselves are rebuilt here, on the CPU, from a seed: the product's synthetic workload generator
(numpy) + the oracle's restatement of the node's cold start (oracle/scenario.py) + the oracle's safe-set query.  They are the
FIRST `count` problems of the 4096-batch bench.py draws for the same configuration, so the fixtures pin the distribution the
headline is measured on."""
from __future__ import annotations

import numpy as np

from oracle import cbind, params as P, scenario as S

BATCH = 4096   # the draw the first `count` problems are taken from (bench.py's batch)
INPUT_KEYS = ("x_ic", "u_ic", "X_ref", "U_ref", "T_ref", "bound_left", "bound_right", "curvatures", "vel_ref")

# name: (family, N, count, BASELINE config it pins)
CASES = {
    "barc_tracking_n20": ("trk", 20, 512, "configs[1]"),
    "iac_tracking_n40": ("iac", 40, 512, "configs[3]"),
    "barc_lmpc_n20_s160": ("lrn", 20, 512, "configs[2] / configs[4] (5 laps, 160 points)"),
    "barc_lmpc_n20_s96": ("rec", 20, 512, "configs[2] on the reference's recorded laps (3 laps, 96 points)"),
    "barc_lmpc_spec_n20_s160": ("spc", 20, 512, "configs[2] / configs[4] AS bench.py QUOTES THEM since round 5 (--lmpc-data spec): laps recorded by the "
                                               "tracking loop at five speed scales, configs[1]'s random x0 (SURVEY.md 8d config 3)"),
    "barc_tracking_n40": ("trk", 40, 128, "shipped horizon"),
    "barc_tracking_n60": ("trk", 60, 96, "shipped horizon (barc_tracking_mpc.param.yaml)"),
    "barc_tracking_n80": ("trk", 80, 64, "shipped horizon"),
    "iac_tracking_n80": ("iac", 80, 64, "shipped horizon (iac_car_tracking_mpc.param.yaml)"),
    "barc_lmpc_n40_s160": ("lrn", 40, 96, "shipped horizon (barc_lmpc.param.yaml)"),
    "barc_lmpc_n60_s160": ("lrn", 60, 64, "shipped horizon (iac_car_lmpc.param.yaml's N)"),
}


def spec_laps():
    """The committed recording of SURVEY.md 8(d) config 3's laps: [n][6] each, oldest (slowest) first."""
    from pathlib import Path

    with np.load(Path(__file__).resolve().parent / "golden" / "spec_laps.npz") as z:
        return [z["lap%d" % i] for i in range(5)]


def ss_query_point(inp: dict, L: float) -> np.ndarray:
    """(s, e_y) of the last reference knot, abscissa aligned to x_ic (racing_mpc.cpp:219-223, 249-254; lmpc_utils/utils.hpp:35-41) --
    as bench.py forms the safe-set query."""
    s_last, s0 = inp["X_ref"][0, -1], inp["x_ic"][0]
    kk = np.abs(s0 - s_last) + L / 2
    return np.stack([s_last + (kk - np.fmod(kk, L)) * np.sign(s0 - s_last), inp["X_ref"][1, -1]])


def build(pkg, name: str):
    """-> cfg, veh, inp (batch axis last, `count` problems), ss_x, ss_j (None for tracking)"""
    family, N, count, _ = CASES[name]
    wl = pkg.workloads
    if family == "trk":
        tr = wl.synthetic_track("barc")
        cfg, veh = P.barc_tracking_mpc(N), P.barc_vehicle()
        x, u = wl.sample_initial_states("barc", BATCH, tr["L"], [-0.01, -0.314159], [0.01, 0.314159], seed=0)
        return cfg, veh, S.cold_start_inputs(cfg, veh, tr, x[:count], u[:count], 0.025), None, None
    if family == "iac":
        tr = wl.synthetic_track("putnam")
        cfg, veh = P.iac_tracking_mpc(N), P.iac_vehicle()
        x, u = wl.sample_initial_states("putnam", BATCH, tr["L"], [-10.0, -0.314159], [5.0, 0.314159], seed=1)
        return cfg, veh, S.cold_start_inputs(cfg, veh, tr, x[:count], u[:count], 0.025), None, None
    if family == "lrn":
        tr = wl.synthetic_track("barc")
        cfg, veh = P.barc_lmpc(N, 5), P.barc_vehicle()
        laps = wl.synthetic_laps(tr, 5)
        x, u = wl.sample_states_near_laps(laps, BATCH, tr["L"], seed=0)
        inp = S.cold_start_inputs(cfg, veh, tr, x[:count], u[:count], 0.025)
        s_last, s0, L = inp["X_ref"][0, -1], inp["x_ic"][0], tr["L"]
        kk = np.abs(s0 - s_last) + L / 2      # lmpc_utils/utils.hpp:35-41, as bench.py forms the query
        q = np.stack([s_last + (kk - np.fmod(kk, L)) * np.sign(s0 - s_last), inp["X_ref"][1, -1]])
        ss_x, ss_j, _ = cbind.ss_query_batch(laps, L, cfg.num_ss_pts, cfg.num_ss_pts_per_lap, q)
        return cfg, veh, inp, ss_x, ss_j
    if family == "spc":
        # SURVEY.md 8(d) config 3 as written, = bench.py --workload lmpc --lmpc-data spec on rank 0: the five laps the tracking loop
        # records at speed scales 0.80 .. 1.0 (closed_loop.record_laps on the GPU; committed as DATA, tests/golden/spec_laps.npz, by
        # tests/golden/make_spec_laps.py -- tests/test_gpu_spec_workload.py holds a fresh recording to the file) and configs[1]'s x0
        tr = wl.synthetic_track("barc")
        cfg, veh = P.barc_lmpc(N, 5), P.barc_vehicle()
        laps = spec_laps()
        x, u = wl.sample_initial_states("barc", BATCH, tr["L"], [-0.01, -0.314159], [0.01, 0.314159], seed=0)
        inp = S.cold_start_inputs(cfg, veh, tr, x[:count], u[:count], 0.025)
        q = ss_query_point(inp, tr["L"])
        ss_x, ss_j, _ = cbind.ss_query_batch(laps, tr["L"], cfg.num_ss_pts, cfg.num_ss_pts_per_lap, q)
        return cfg, veh, inp, ss_x, ss_j
    if family == "rec":
        import lmpc_scenario as LS

        veh, cfg, tr, laps, inp, q = LS.make(count, 21, N=N)
        ss_x, ss_j, _ = LS.oracle_safe_set(cfg, laps, q)
        return cfg, veh, inp, ss_x, ss_j
    raise KeyError(name)


def digest(inp: dict, ss_x=None, ss_j=None) -> np.ndarray:
    """One number per problem: the sum of |.| over every input array of the problem (drift of the regenerated inputs against the
    ones the fixture was solved on shows up here at the 1e-12 level, long before it shows in the comparison)."""
    d = sum(np.abs(np.asarray(inp[k], dtype=np.float64)).reshape(-1, np.asarray(inp[k]).shape[-1]).sum(axis=0) for k in INPUT_KEYS)
    if ss_x is not None:
        d = d + np.abs(ss_x).sum(axis=(0, 1)) + np.abs(ss_j).sum(axis=0)
    return d


# ---- regressed solves (BASELINE configs[4]: the error-dynamics regression in front of every stage) -----------------------------------
# A table of its own: tests/test_dense_fixtures.py runs the serial twin over CASES, and the twin has no regression.  The reference model
# comes from the oracle alone -- oracle.qp.linearise, corrected by oracle.regression, handed to build_qp(lin=...) -- never from the
# product's regress().  The regression samples are the bench's two-sample laps (workloads.regression_sample_pairs) with successors from
# a CPU plant: the oracle's RK4 with 15 % less grip.
BENCH_REG = ((3, 4, 5), (0, 1), (3, 4, 5))
S01234_REG = ((0, 1, 2, 3, 4), (), (2, 4, 5))
ALL_REG = ((0, 1, 2, 3, 4, 5), (0, 1), (0, 1, 2, 3, 4, 5))
REG_DIST_MAX = 0.6

# name: (family, N, count, feature spec, dist_max, what it pins).  Which kernel instance runs follows from the spec (5 features / 3 rows
# or 8 / 6) and from the scale of the features against dist_max (lmpc_set_regression_laps: EXACT weights where max |z| > 16 dist_max).
REG_CASES = {
    "reg_barc_lmpc_spec_n20_s160": ("spc", 20, 512, BENCH_REG, REG_DIST_MAX, "configs[4] as benched: spec laps, configs[1]'s random x0 (rank 0)"),
    "reg_barc_lmpc_near_n20_s160": ("near", 20, 512, BENCH_REG, REG_DIST_MAX, "configs[4] on states drawn near the stored laps (bench.py --lmpc-data near)"),
    "reg_barc_tracking_n20": ("trk", 20, 96, BENCH_REG, REG_DIST_MAX, "tracking, one-wave kernel; <5, 3> screened weights"),
    "reg_barc_tracking_n60": ("trk", 60, 64, BENCH_REG, REG_DIST_MAX, "tracking, two-wave kernel (reads the regressed records through its own loader)"),
    "reg_barc_tracking_all_n20": ("trk", 20, 64, ALL_REG, 1.5, "<8, 6> with screened weights inside a solve (BARC: max |z| ~ 17 < 16 x 1.5)"),
    "reg_iac_tracking_n40": ("iac", 40, 64, ALL_REG, REG_DIST_MAX, "<8, 6> with exact weights inside a solve, IAC scale"),
    "reg_iac_tracking_s01234_n40": ("iac", 40, 64, S01234_REG, REG_DIST_MAX, "<5, 3> with exact weights inside a solve (the abscissa at IAC scale)"),
}


def reg_exact(samples, spec, dist_max) -> bool:
    """The rule lmpc_set_regression_laps applies (csrc/lmpc_capi.hip): exact weights where the largest squared feature norm over the
    samples exceeds 256 dist_max^2."""
    ins, inc = list(spec[0]), list(spec[1])
    z2 = max(float(((np.asarray(x)[:, ins] ** 2).sum(axis=1) + (np.asarray(u)[:, inc] ** 2).sum(axis=1)).max()) for (x, u, k, t) in samples)
    return not (z2 <= 256.0 * dist_max * dist_max)


def regression_samples(pkg, tr, veh, stored):
    """Two-sample laps around `stored` state laps, successors one 30 ms step of the CPU plant (mu x 0.85)."""
    import dataclasses

    from oracle import scenario as S2
    from oracle.dynamics import rk4

    plant = dataclasses.replace(veh, mu=0.85 * veh.mu)
    return pkg.workloads.regression_sample_pairs(
        tr, stored, lambda xa, ua: rk4(xa, ua, S2.track_lookup(tr["curvature"], xa[:, 0], tr["L"]), 0.03, plant))


def oracle_regressed_model(cfg, veh, inp, samples, spec, dist_max=REG_DIST_MAX):
    """Per problem (A [N-1,6,6], B [N-1,6,2], g [N-1,6]) as build_qp(lin=...) takes them, stacked on a leading batch axis: the oracle's
    linearisation about (X_ref, U_ref) plus the oracle's regression at every stage."""
    from oracle import qp as Q, regression as R

    N, Bn = cfg.N, inp["x_ic"].shape[1]
    lin = [Q.linearise(cfg, veh, S.problem(inp, b)) for b in range(Bn)]
    A0 = np.stack([l[0] for l in lin]).reshape(Bn * (N - 1), 6, 6)
    B0 = np.stack([l[1] for l in lin]).reshape(Bn * (N - 1), 6, 2)
    g0 = np.stack([l[2] for l in lin]).reshape(Bn * (N - 1), 6)
    qx = inp["X_ref"][:, : N - 1, :].transpose(2, 1, 0).reshape(-1, 6)
    qu = inp["U_ref"].transpose(2, 1, 0).reshape(-1, 2)
    A, B, g, touched = R.regress_batch(veh, samples, *spec, dist_max, qx, qu, A0, B0, g0)
    return A.reshape(Bn, N - 1, 6, 6), B.reshape(Bn, N - 1, 6, 2), g.reshape(Bn, N - 1, 6), touched.reshape(Bn, N - 1)


def build_reg(pkg, name: str):
    """-> cfg, veh, inp, ss_x, ss_j (None for tracking), samples (the regression's laps), spec, (A, B, g, touched) of the oracle"""
    family, N, count, spec, dist_max, _ = REG_CASES[name]
    wl = pkg.workloads
    if family in ("spc", "near"):
        tr = wl.synthetic_track("barc")
        cfg, veh = P.barc_lmpc(N, 5), P.barc_vehicle()
        # (a) the spec laps and configs[1]'s x0 (the problems of dense_barc_lmpc_spec_n20_s160); (b) bench.py --lmpc-data near: the
        # synthetic laps and states drawn near them (the problems of dense_barc_lmpc_n20_s160)
        stored = spec_laps() if family == "spc" else wl.synthetic_laps(tr, 5)
        _, _, inp, ss_x, ss_j = build(pkg, "barc_lmpc_spec_n20_s160" if family == "spc" else "barc_lmpc_n20_s160")
    elif family == "trk":
        cfg, veh, inp, ss_x, ss_j = build(pkg, "barc_tracking_n%d" % N)
        inp = {k: (v[..., :count] if isinstance(v, np.ndarray) else v) for k, v in inp.items()}
        tr = wl.synthetic_track("barc")
        stored = spec_laps()
    elif family == "iac":
        cfg, veh, inp, ss_x, ss_j = build(pkg, "iac_tracking_n%d" % N)
        inp = {k: (v[..., :count] if isinstance(v, np.ndarray) else v) for k, v in inp.items()}
        tr = wl.synthetic_track("putnam")
        stored = [inp["X_ref"][:, :, b].T.copy() for b in range(0, count, 2)]   # samples around every other problem's cold start
    else:
        raise KeyError(name)
    samples = regression_samples(pkg, tr, veh, stored)
    return cfg, veh, inp, ss_x, ss_j, samples, spec, oracle_regressed_model(cfg, veh, inp, samples, spec, dist_max)


def reg_digests(samples, model):
    """(per-problem sum |.| of the oracle's corrected A, B, g; one number for the regression samples)"""
    A, B, g = model[:3]
    return (np.abs(A).sum(axis=(1, 2, 3)) + np.abs(B).sum(axis=(1, 2, 3)) + np.abs(g).sum(axis=(1, 2)),
            float(sum(np.abs(np.asarray(a)).sum() for lap in samples for a in lap)))
