"""The inputs and references of tests/test_gpu_envelope.py held to their own conditions, without a GPU (tests/envelope_cases.py): the
audit -- every field the vehicle model reads moves the reference on the envelope draws -- the oracle's two Jacobians against each
other in the per-problem measure, the double-track autograd reference against Richardson differences, and the C twin's linearisation
(the solve tests' reference, which has run on the same two vehicles as the kernels) on the envelope vehicle."""
import numpy as np
import pytest

import cars_model_cases as CM
import dtrack_model_cases as DM
import envelope_cases as E
from oracle import cbind, params as P
from tolerances import TOL_LINEARIZE_REL

B, N = E.B_TEST, E.N_TEST


@pytest.mark.parametrize("track", ["single", "double"])
@pytest.mark.parametrize("kind", E.KINDS)
def test_every_field_the_model_reads_moves_the_reference(kind, track):
    moved = E.audit(kind, track)
    fields = E.FIELDS if track == "single" else E.DTRACK_FIELDS
    assert tuple(moved) == fields and not set(fields) & set(E.NOT_READ)
    print("%s, %s track: + 10 %% moves the Jacobian / the one-step state by more than %.0e on (of %d points):" % (kind, track, E.AUDIT_MOVE, (N - 1) * B))
    print("  " + "  ".join("%s %d/%d" % (f, a, s) for f, (a, s, _) in moved.items()))
    for f, (a, s, n) in moved.items():
        assert n == (N - 1) * B and min(a, s) >= E.AUDIT_SHARE * n, (f, a, s)


@pytest.mark.parametrize("kind", E.KINDS)
def test_the_envelope_vehicles_are_off_the_presets_and_the_draws_reach_the_branches(kind):
    for track, fields in (("single", E.FIELDS), ("double", E.DTRACK_FIELDS)):
        base = E.base_vehicle(kind, track)
        veh = E.table(kind, B, track)
        assert len(CM.groups(veh)) == 3 and [v["kd"] for v in veh[:3]] == [0.35, 1.0, 0.35] and veh[2]["integrator"] == "euler"
        for v in veh[:3]:
            assert not E.off_preset(v, base, fields) and v["Af"] != 1.0 and v["rho"] != v["Af"]
        if track == "double":
            assert veh[0]["tw_f"] != veh[0]["tw_r"]
        inp = E.envelope_draws(kind, B, N, track=track)   # (asserts its own conditions)
        th = np.tanh(inp["U_ref"][0])
        assert (th > E.SATURATED).mean() > 0.3 and (th < -E.SATURATED).mean() > 0.3 and (np.abs(th) < E.MIDPOINT).mean() > 0.3
    one = E.envelope_draws(kind, 1, N)
    assert one["X_ref"].shape == (6, N, 1) and sorted(np.sign(np.round(np.tanh(one["U_ref"][0, :, 0]))).tolist()) == [-1.0, 0.0, 1.0]


@pytest.mark.parametrize("kind", E.KINDS)
def test_the_oracles_two_jacobians_agree_per_problem_on_the_envelope(kind):
    """rk4_jacobian_analytic (f_and_partials for the Euler car) against rk4_jacobian_cs on the three-car table, within
    TOL_LINEARIZE_REL in the per-problem measure -- the spread that sets the device's allowance (envelope_cases.bounds)."""
    inp, veh = E.envelope_draws(kind, B, N), E.table(kind, B)
    cs, an = E.complex_step(inp, veh), CM.reference(inp, veh)
    assert all(np.isfinite(a).all() for a in cs + an)
    eA, eB, eg = E.errors(an, cs)
    print("%s: analytic against complex step, per problem: A %.1e Bm %.1e g %.1e; Euler cars A %.1e; max |A| %.1e, smallest per-problem max |A| %.2f"
          % (kind, eA.max(), eB.max(), eg.max(), eA[:, 2::3].max(), np.abs(cs[0]).max(), np.abs(cs[0]).max(axis=(0, 1)).min()))
    assert eA.max() <= TOL_LINEARIZE_REL and eB.max() <= TOL_LINEARIZE_REL and eg.max() <= 10 * TOL_LINEARIZE_REL
    bA, bB, bg = E.bounds(an, cs)
    assert bA.max() == TOL_LINEARIZE_REL and bB.max() == TOL_LINEARIZE_REL and bg.max() == 10 * TOL_LINEARIZE_REL


@pytest.mark.parametrize("kind", E.KINDS)
def test_dtrack_autograd_agrees_with_richardson_on_the_envelope(kind):
    """tests/test_dtrack_model_reference.py's check and bound (1e-4 on max(1, |J|); the difference quotient is the weaker side), on
    the double-track envelope table and draws; g closes the affine model."""
    inp, veh = E.envelope_draws(kind, B, N, track="double"), E.table(kind, B, "double")
    NS, worst = N - 1, 0.0
    for cars in DM.groups(veh):
        x = inp["X_ref"][:, :NS, cars].transpose(2, 1, 0).reshape(-1, 6)
        u = inp["U_ref"][:, :, cars].transpose(2, 1, 0).reshape(-1, 2)
        k, dt, p = inp["curvatures"][:NS, cars].T.reshape(-1), inp["T_ref"][:, cars].T.reshape(-1), veh[cars[0]]
        A, Bm, g = DM.jacobians(x, u, k, dt, p)
        fA, fB = DM.richardson(x, u, k, dt, p)
        for got, want in ((fA, A), (fB, Bm)):
            worst = max(worst, float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()))
        y = DM.numpy_step(x, u, k, dt, p)
        aff = np.einsum("mrc,mc->mr", A, x) + np.einsum("mrc,mc->mr", Bm, u) + g
        assert (np.abs(aff - y) <= 1e-12 * np.maximum(1.0, np.abs(y))).all()
    print("%s: max |Richardson - autograd| / max(1, |J|) = %.2e" % (kind, worst))
    assert worst <= 1e-4


@pytest.mark.parametrize("integrator", ["rk4", "euler"])
@pytest.mark.parametrize("kind", E.KINDS)
def test_the_c_twin_linearises_the_envelope_vehicle(kind, integrator):
    """oracle.cbind.linearize_batch against the complex step, per problem, under envelope_cases.bounds."""
    inp = E.envelope_draws(kind, B, N)
    v = dict(E.envelope_vehicle(E.base_vehicle(kind)), integrator=integrator)
    cs, an = E.complex_step(inp, [v] * B), CM.reference(inp, [v] * B)
    got = cbind.linearize_batch(P.barc_tracking_mpc(N), CM.oracle_vehicle(v), inp)
    err, bnd = E.errors(got, cs), E.bounds(an, cs)
    print("%s %s: C twin against complex step, per problem: A %.1e Bm %.1e g %.1e" % (kind, integrator, *(e.max() for e in err)))
    for name, e, b in zip(("A", "Bm", "g"), err, bnd):
        assert (e <= b).all(), (name, float((e / b).max()))
