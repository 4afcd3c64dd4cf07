"""The reference of the double-track controller model (tests/dtrack_model_cases.py) held to what it restates, without a GPU: the torch
step equals tests/dtrack_cases.py's numpy step, its autograd Jacobians agree with Richardson differences of the numpy step, the
committed fixtures (tests/golden/dense_dtrack_*.npz) were solved on the inputs and the model that are rebuilt today, and their first
problems re-solve to the stored optimum with a KKT certificate."""
import numpy as np
import pytest
import torch

import dtrack_cases as DT
import dtrack_model_cases as MC
from oracle import qp as Q, scenario as S
from parity import per_problem_err

GOLD = MC.__file__.rsplit("/", 1)[0] + "/golden"


@pytest.fixture(scope="module")
def built(pkg):
    """every fixture's problems and reference model, rebuilt once"""
    out = {}
    for name in MC.FIXTURES:
        cfg, veh, inp, ss_x, ss_j, table = MC.build(pkg, name)
        out[name] = dict(cfg=cfg, veh=veh, inp=inp, ss_x=ss_x, ss_j=ss_j, table=table, model=MC.qp_model(MC.reference(inp, table)))
    return out


def stage_points(d, problems):
    """(x, u, k, dt, vehicle) per distinct vehicle among the listed problems: every stage of each"""
    inp, NS = d["inp"], d["cfg"].N - 1
    for cars in MC.groups([d["table"][b] for b in problems]):
        cars = [problems[c] for c in cars]
        x = inp["X_ref"][:, :NS, cars].transpose(2, 1, 0).reshape(-1, 6)
        u = inp["U_ref"][:, :, cars].transpose(2, 1, 0).reshape(-1, 2)
        yield x, u, inp["curvatures"][:NS, cars].T.reshape(-1), inp["T_ref"][:, cars].T.reshape(-1), d["table"][cars[0]]


@pytest.mark.parametrize("name", ["dtrack_trk_n20", "dtrack_iac_n40"])
def test_the_torch_step_is_the_numpy_step(built, name):
    worst = 0.0
    for x, u, k, dt, p in stage_points(built[name], list(range(8))):
        z = DT.to_native(x)
        want = DT.from_native(DT.step_native(z, u, k, dt[:, None], p))
        got = MC.phi(torch.tensor(x), torch.tensor(u), torch.tensor(k), torch.tensor(dt), p).numpy()
        worst = max(worst, float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()))
        f_np = DT.f_continuous(z, u, k, p)[0]
        f_t = MC.f_continuous(torch.tensor(z), torch.tensor(u), torch.tensor(k), p).numpy()
        worst = max(worst, float((np.abs(f_t - f_np) / np.maximum(1.0, np.abs(f_np))).max()))
    print("%s: max |torch - numpy| / max(1, |.|) over step and dynamics = %.2e" % (name, worst))
    assert worst <= 1e-14


@pytest.mark.parametrize("name", ["dtrack_trk_n20", "dtrack_iac_n40"])
def test_autograd_agrees_with_richardson_differences(built, name):
    """Scaled by max(1, |J|); the finite difference is the weaker side (h = 1e-4, error O(h^4) and rounding / h)."""
    worst = 0.0
    for x, u, k, dt, p in stage_points(built[name], list(range(8))):
        A, Bm, g = MC.jacobians(x, u, k, dt, p)
        fA, fB = MC.richardson(x, u, k, dt, p)
        for got, want in ((fA, A), (fB, Bm)):
            worst = max(worst, float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()))
        # g closes the affine model at the point
        y = MC.numpy_step(x, u, k, dt, p)
        aff = np.einsum("mrc,mc->mr", A, x) + np.einsum("mrc,mc->mr", Bm, u) + g
        assert (np.abs(aff - y) <= 1e-12 * np.maximum(1.0, np.abs(y))).all()
    print("%s: max |Richardson - autograd| / max(1, |J|) = %.2e" % (name, worst))
    assert worst <= 1e-4


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
    assert fx["single_track_distance"].min() > MC.MIN_DISTANCE
    veh = d["table"]
    assert veh[MC.EULER_PROBLEM]["integrator"] == "euler" and sum(v["integrator"] == "euler" for v in veh) == 1
    assert len(MC.groups(veh)) == 4


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
