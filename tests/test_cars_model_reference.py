"""The reference of the per-car controller model (tests/cars_model_cases.py) held to an independent one, without a GPU: the analytic
Jacobian of the oracle on every kind of car -- the perturbed vehicles and the two on Euler -- agrees with the complex-step Jacobian of
the oracle's integrator; the committed fixtures (tests/golden/dense_cars_*.npz) were solved on the inputs and the per-car model that are
rebuilt today, every stored certificate and every stored distance to the optimum on the handle's vehicle holds its bound, and their
first problems re-solve to the stored optimum with a KKT certificate."""
import numpy as np
import pytest

import cars_model_cases as MC
from oracle import dynamics as D, qp as Q, scenario as S
from parity import per_problem_err
from tolerances import TOL_LINEARIZE_REL, TOL_XU

GOLD = MC.__file__.rsplit("/", 1)[0] + "/golden"


@pytest.fixture(scope="module")
def built(pkg):
    """every fixture's problems and reference model, rebuilt once"""
    out = {}
    for name in MC.FIXTURES:
        cfg, veh, inp, ss_x, ss_j, table = MC.build(pkg, name)
        out[name] = dict(cfg=cfg, veh=veh, inp=inp, ss_x=ss_x, ss_j=ss_j, table=table, model=MC.qp_model(MC.reference(inp, table)))
    return out


def test_the_kinds_differ_from_the_preset_in_fields_the_dynamics_read(pkg):
    ignored = {"b", "Fd_max", "Fb_max", "Td", "Tb", "max_steer", "max_steer_rate"}
    for base in (pkg.presets.barc_vehicle(), pkg.presets.iac_vehicle()):
        kinds = MC.kinds(base)
        assert len(kinds) == 3
        for k in kinds:
            changed = {f for f in base if k[f] != base[f]}
            assert changed and not changed & (ignored | {"model_id", "integrator"}), changed
        assert len({tuple(sorted(k.items())) for k in kinds}) == 3
    veh = MC.fleet(pkg.presets.barc_vehicle(), 16)
    assert [b for b, v in enumerate(veh) if v["integrator"] == "euler"] == list(MC.EULER_PROBLEMS) and len(MC.groups(veh)) == 5
    assert MC.oracle_vehicle(veh[4]).integrator == "euler" and MC.oracle_vehicle(dict(veh[4], integrator=1)).integrator == "euler"


@pytest.mark.parametrize("B,N", [(70, 3), (40, 20)])
def test_the_analytic_reference_agrees_with_complex_step_on_every_kind_of_car(pkg, B, N):
    """On independent draws per stage, TOL_LINEARIZE_REL as tests/test_gpu_timestep.py applies it, stage by stage.  The complex step
    goes through oracle.dynamics.rk4, which knows both integrators; the analytic side takes the Euler weights in cars_model_cases."""
    inp, veh = MC.lin_draws(pkg, B, N)
    assert sum(v["integrator"] == "euler" for v in veh) == 2 and len(MC.groups(veh)) == 5
    want = MC.reference(inp, veh, jac=lambda x, u, k, dt, v: D.rk4_jacobian_cs(x, u, k, dt, v))
    got = MC.reference(inp, veh)
    worst = [0.0, 0.0, 0.0]
    for i in range(N - 1):
        for j, (g, w, tol) in enumerate(zip(got, want, (TOL_LINEARIZE_REL, TOL_LINEARIZE_REL, 10 * TOL_LINEARIZE_REL))):
            g, w = (g[:, :, i], w[:, :, i]) if j < 2 else (g[:, i], w[:, i])
            scale = np.abs(w).max() if j < 2 else max(1.0, np.abs(w).max())
            worst[j] = max(worst[j], float(np.abs(g - w).max() / scale))
            assert np.abs(g - w).max() <= tol * scale, (i, j)
    print("B = %d N = %d: analytic against complex step, relative to the stage's largest entry: A %.1e Bm %.1e g %.1e" % (B, N, *worst))
    # an Euler car is not an RK4 car: the two differ by far more than the bound (the reference would notice a wrong integrator)
    e = MC.EULER[0]
    rk = MC.reference({k: v[..., e:e + 1] for k, v in inp.items()}, [dict(veh[e], integrator="rk4")])
    assert np.abs(rk[0][..., 0] - got[0][..., e]).max() > 1e3 * TOL_LINEARIZE_REL * np.abs(rk[0]).max()


@pytest.mark.parametrize("name", list(MC.FIXTURES))
def test_fixture_digests_match_the_regenerated_inputs(built, name):
    d = built[name]
    with np.load(f"{GOLD}/dense_{name}.npz") as z:
        fx = {k: z[k] for k in z.files}
    count = MC.FIXTURES[name][2]
    assert fx["status"].shape == (count,) and (fx["status"] == 0).all(), "no problem is dropped"
    d_in, d_model = MC.digest(d["inp"], d["ss_x"], d["ss_j"], d["model"])
    np.testing.assert_allclose(d_in, fx["digest"], rtol=1e-11, atol=0)
    np.testing.assert_allclose(d_model, fx["model_digest"], rtol=1e-9, atol=0)
    assert fx["kkt_cert"].max() <= MC.MAX_CERTIFICATE
    assert fx["single_vehicle_distance"].shape == (count,) and fx["single_vehicle_distance"].min() > MC.MIN_DISTANCE
    assert MC.MIN_DISTANCE == 1e-4 and round(MC.MIN_DISTANCE / TOL_XU) == 100
    veh = d["table"]
    assert [b for b, v in enumerate(veh) if v["integrator"] == "euler"] == list(MC.EULER_PROBLEMS)
    assert len(MC.groups(veh)) == 5


@pytest.mark.parametrize("name", list(MC.FIXTURES))
def test_first_problems_resolve_to_the_fixture_with_a_certificate(built, name):
    d = built[name]
    with np.load(f"{GOLD}/dense_{name}.npz") as z:
        fx = {k: z[k][..., :4] for k in ("X_optm", "U_optm", "dU_optm")}
    got = {k: [] for k in fx}
    for b in range(4):
        kw = {} if d["ss_x"] is None else {"ss_x": d["ss_x"][:, :, b], "ss_j": d["ss_j"][:, b]}
        qp = Q.build_qp(d["cfg"], d["veh"], S.problem(d["inp"], b), lin=tuple(m[b] for m in d["model"]), **kw)
        y, info = Q.solve_dense(qp)
        assert info["status"] == 0
        c = Q.kkt_certificate(qp, y)
        gs = max(1.0, float(np.abs(qp.H @ y + qp.h).max()))
        assert max(c["stat"] / gs, c["eq"], c["ineq"], c["comp"]) <= MC.MAX_CERTIFICATE
        o = qp.split(y)
        for k in got:
            got[k].append(o[k])
    exu, ed = per_problem_err({k: np.stack(v, -1) for k, v in got.items()}, fx)
    assert exu.max() < 1e-9 and ed.max() < 1e-9, (exu, ed)
