"""CPU: the fixtures on a non-uniform time step (tests/golden/dense_dt_*.npz, tests/timestep_cases.py).

  * the conditions tests/golden/make_timestep_fixtures.py asserts hold on the committed files: every problem dense status 0 with a KKT
    certificate, at most 10 % of a case replaced, a rate row active on at least a quarter of a case, the rolled-T_ref optimum at least
    1e3 TOL_XU away on every problem; the inputs rebuilt from the seeds match the digests; T_ref is what the module says it is;
  * a fresh dense solve of a few problems reproduces the stored optimum (the fixture is this oracle's output);
  * the serial C twin against the dense optimum, every problem, TOL_XU / TOL_DU, statuses equal;
  * the comparison the GPU tests apply (timestep_cases.accepted) REJECTS the optimum of the rolled problem on every problem of every
    case, and so does the rate identity: an entry point that read T_ref one stage off cannot pass tests/test_gpu_timestep.py."""
import numpy as np
import pytest

import timestep_cases as TC
from oracle import cbind, qp as Q, scenario as S
from tolerances import TOL_DU, TOL_F32_SWEEP, TOL_MEDIAN, TOL_XU

KEYS = ("X_optm", "U_optm", "dU_optm")


@pytest.mark.parametrize("name", list(TC.CASES))
def test_fixture_conditions(pkg, name):
    fx, cfg, veh, inp, ss_x, ss_j = TC.fixture_problems(pkg, name)
    family, N, count = TC.CASES[name][:3]
    B = fx["status"].size
    assert B == count and cfg.N == N and fx["T_ref"].shape == (N - 1, B)
    assert (fx["status"] == 0).all()
    cert = fx["kkt_cert"]
    assert cert[0].max() < 1e-9 and cert[1].max() < 1e-9 and cert[2].max() < 1e-9 and cert[3].max() < 1e-8, (name, cert.max(axis=1))
    idx = fx["draw_index"]
    assert idx[0] == 0 and (np.diff(idx) > 0).all() and idx.max() < TC.pool_size(name)
    assert (idx >= count).sum() <= TC.REPLACED_SHARE_MAX * count
    assert fx["rate_row_active"].mean() >= TC.ACTIVE_RATE_SHARE_MIN, (name, fx["rate_row_active"].mean())
    assert fx["rolled_distance"].min() >= TC.SENSITIVITY_MIN, (name, fx["rolled_distance"].min())
    # the time step: inside [0.0125, 0.05], different from stage to stage and from problem to problem; problem 0 strictly increasing
    T = fx["T_ref"]
    assert T.min() >= 0.0125 and T.max() <= 0.05
    np.testing.assert_allclose(T[:, 0], 0.0125 * (1.0 + 3.0 * np.arange(N - 1) / (N - 2)), rtol=1e-15)
    assert (np.diff(T[:, 0]) > 0).all()
    assert np.unique(T).size == T.size
    # the stored rolled optimum is the stored distance away
    d = np.maximum(*TC.errors({k: fx[k + "_rolled"] for k in KEYS}, fx))
    np.testing.assert_allclose(d, fx["rolled_distance"], rtol=1e-12)
    if ss_x is not None:
        lam = fx["convex_combi_optm"]
        assert lam.shape == (cfg.num_ss_pts, B) and np.abs(lam.sum(axis=0) - 1.0).max() < 1e-9 and lam.min() > -1e-9


@pytest.mark.parametrize("name", ["dt_trk_n3", "dt_trk_n20", "dt_lrn_n20_s160"])
def test_fixture_is_this_oracles_output(pkg, name):
    fx, cfg, veh, inp, ss_x, ss_j = TC.fixture_problems(pkg, name)
    for b in (0, 1, fx["status"].size - 1):
        kw = {} if ss_x is None else {"ss_x": ss_x[:, :, b], "ss_j": ss_j[:, b]}
        qp = Q.build_qp(cfg, veh, S.problem(inp, b), **kw)
        y, info = Q.solve_dense(qp)
        o = qp.split(y)
        assert info["status"] == 0 and TC.rate_row_active(qp, info["lam"]) == bool(fx["rate_row_active"][b])
        exu, ed = TC.errors({k: o[k][..., None] for k in o if k in KEYS + ("convex_combi_optm",)} | {"status": np.zeros(1, dtype=int)},
                            {k: fx[k][..., b:b + 1] for k in KEYS + (("convex_combi_optm",) if ss_x is not None else ())})
        assert exu.max() < 1e-9 and ed.max() < 1e-8, (name, b, exu, ed)


@pytest.mark.parametrize("name", list(TC.CASES))
def test_twin_against_dense_fixture_every_problem(pkg, name):
    fx, cfg, veh, inp, ss_x, ss_j = TC.fixture_problems(pkg, name)
    tw = cbind.solve_batch(cfg, veh, inp, ss_x, ss_j)
    assert np.array_equal(tw["status"], fx["status"]), (name, np.nonzero(tw["status"])[0], tw["status"][tw["status"] != 0])
    exu, ed = TC.assert_matches(tw, fx, "%s, twin vs dense" % name)
    assert np.median(TC.errors(tw, fx)[0]) < TOL_MEDIAN
    assert TC.rate_identity_error(tw, inp) < 1e-12


@pytest.mark.parametrize("name", list(TC.CASES))
def test_the_comparison_rejects_the_rolled_optimum_on_every_problem(name):
    """What tests/test_gpu_timestep.py would see from an entry point that read t_{i-1} for t_i and was otherwise perfect: the optimum
    of the rolled problem, status 0.  The fp64 comparison and the reduced-precision one (TOL_F32_SWEEP) both refuse every problem; so
    does the rate identity, which holds dU t_i to the differences of U with the TRUE t_i."""
    fx = TC.load(name)
    B = fx["status"].size
    slipped = {k: fx[k + "_rolled"] for k in KEYS}
    slipped["status"] = np.zeros(B, dtype=np.int32)
    assert not TC.accepted(slipped, fx).any()
    assert not TC.accepted(slipped, fx, TOL_F32_SWEEP, TOL_F32_SWEEP / 0.025).any(), np.nonzero(TC.accepted(slipped, fx, TOL_F32_SWEEP, TOL_F32_SWEEP / 0.025))[0]
    with pytest.raises(AssertionError):
        TC.assert_matches(slipped, fx, "%s, rolled" % name)
    # and the true optimum passes it
    assert TC.accepted(dict({k: fx[k] for k in KEYS}, status=fx["status"]), fx).all()
    assert fx["rolled_distance"].min() >= 1e3 * max(TOL_XU, TOL_DU)
