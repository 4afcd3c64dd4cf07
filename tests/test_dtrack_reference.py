"""tests/dtrack_cases.py, the plain reference the double-track plant (include/lmpc_hip_dtrack.h) is held to on the GPU, checked on
its own: mirror symmetry (left / right and sign slips among the four tyres), its closed-form gamma_y against the residual equation,
the limit without load transfer, and that the model really differs from the single-track one.  No GPU."""
import numpy as np
import pytest

import dtrack_cases as DC
from oracle import dynamics as D, params as P, scenario as S

B = 300


@pytest.fixture(scope="module")
def sets(pkg):
    """name -> (track, x, u, vehicles): the BARC draws of the GPU test and the IAC-scale set"""
    tb = pkg.workloads.synthetic_track("barc")
    xb, ub, vb = DC.barc_draws(pkg, B, tb["L"])
    ti = DC.iac_track(pkg)
    xi, ui = DC.iac_draws(B, ti["L"])
    assert np.abs(ti["curvature"]).max() <= 0.01
    return {"barc": (tb, xb, ub, vb), "iac": (ti, xi, ui, [pkg.presets.iac_double_track()] * B)}


def mirrored(track):
    return dict(track, curvature=-track["curvature"])


@pytest.mark.parametrize("name", ["barc", "iac"])
def test_the_restatement_is_mirror_symmetric_and_finite(sets, name):
    tr, x, u, veh = sets[name]
    want, gam = DC.reference(tr, x, u, veh)
    assert np.isfinite(want).all() and np.isfinite(gam).all()
    got, gam_m = DC.reference(mirrored(tr), x * DC.MIRROR_X, u * DC.MIRROR_U, veh)
    err = np.abs(got * DC.MIRROR_X - want).max(axis=0)
    print(name, "mirror: max |difference| per component", err, " max |gamma_y| %.3e" % np.abs(gam).max())
    assert (err <= 1e-13).all()
    assert np.abs(gam_m + gam).max() <= 1e-13 * max(1.0, np.abs(gam).max())
    assert (got[:, 0] >= 0).all() and (got[:, 0] < tr["L"]).all()


@pytest.mark.parametrize("name", ["barc", "iac"])
def test_gamma_y_is_a_root_of_the_residual(sets, name):
    tr, x, u, veh = sets[name]
    z = DC.to_native(x)
    k = S.track_lookup(tr["curvature"], z[:, 0], float(tr["L"]))
    worst = 0.0
    for kind in {id(v): v for v in veh}.values():
        cars = [b for b, v in enumerate(veh) if v is kind]
        gam = DC.f_continuous(z[cars], u[cars], k[cars], kind)[1]
        res = DC.residual(gam, z[cars], u[cars], kind)
        worst = max(worst, (np.abs(res) / np.maximum(1.0, np.abs(gam))).max())
        assert (np.abs(res) <= 1e-12 * np.maximum(1.0, np.abs(gam))).all()
    print(name, "max |g(gamma_y)| / max(1, |gamma_y|) = %.3e" % worst)


@pytest.mark.parametrize("name", ["barc", "iac"])
def test_without_cg_height_there_is_no_load_transfer(sets, name):
    tr, x, u, veh = sets[name]
    z = DC.to_native(x)
    k = S.track_lookup(tr["curvature"], z[:, 0], float(tr["L"]))
    _, gam, Fz = DC.f_continuous(z, u, k, dict(veh[0], h=0.0))
    assert (gam == 0.0).all()
    assert (Fz[0] == Fz[1]).all() and (Fz[2] == Fz[3]).all()


def test_the_model_differs_from_the_single_track_model(sets, pkg):
    """One RK4 step of each model on the same draws: more than 1e-6 apart."""
    for name, single in (("barc", P.barc_vehicle()), ("iac", P.iac_vehicle())):
        tr, x, u, veh = sets[name]
        k = S.track_lookup(tr["curvature"], x[:, 0], float(tr["L"]))
        one = D.rk4(x, u, k, DC.DT_SIM, single)
        rk4_car = dict(veh[0], integrator="rk4")
        four = DC.from_native(DC.step_native(DC.to_native(x), u, k, DC.DT_SIM, rk4_car))
        moved = np.abs(four - one).max(axis=1)
        ordinary = np.ones(B, dtype=bool)
        if name == "barc":
            ordinary[DC.SLOW] = False   # (pulling away from a standstill in a straight line the models agree)
        print(name, "min / max |double track - single track| after one step: %.3e / %.3e" % (moved[ordinary].min(), moved.max()))
        assert moved.max() > 1e-6 and (moved[ordinary] > 1e-6).mean() > 0.9


def test_newton_from_zero_reaches_the_closed_form_root(sets):
    """What the kernel does -- LMPC_DTRACK_NEWTON iterations from gamma = 0 with the analytic derivative -- restated on the residual
    of this module, at IAC scale: three iterations are not enough for 1e-11, five are (the count in include/lmpc_hip_dtrack.h)."""
    import re
    from pathlib import Path
    header = (Path(__file__).resolve().parents[1] / "include" / "lmpc_hip_dtrack.h").read_text()
    count = int(re.search(r"#define LMPC_DTRACK_NEWTON (\d+)", header).group(1))
    tr, x, u, veh = sets["iac"]
    p = veh[0]
    z = DC.to_native(x)
    k = S.track_lookup(tr["curvature"], z[:, 0], float(tr["L"]))
    root = DC.f_continuous(z, u, k, p)[1]
    Fx_f, _, Fz_f, Fz_r, S_ij = DC.tyre_terms(z, u, p)
    cg = p["h"] / (0.5 * (p["tw_f"] + p["tw_r"]))
    ef, er, kf, kr = p["eps_f"] / p["Fz0_f"], p["eps_r"] / p["Fz0_r"], p["kroll_f"], 1.0 - p["kroll_f"]
    gam, rel = np.zeros(B), {}
    for it in range(1, count + 1):
        Fz = DC.loads(Fz_f, Fz_r, gam, p)
        dF = p["mu"] * kf * ((1.0 + 2.0 * ef * Fz[1]) * S_ij[1] - (1.0 + 2.0 * ef * Fz[0]) * S_ij[0])
        dR = p["mu"] * kr * ((1.0 + 2.0 * er * Fz[3]) * S_ij[3] - (1.0 + 2.0 * er * Fz[2]) * S_ij[2])
        gam = gam - DC.residual(gam, z, u, p) / (1.0 - cg * (dR + dF * np.cos(u[:, 1])))
        rel[it] = (np.abs(gam - root) / np.maximum(1.0, np.abs(root))).max()
    print("Newton from 0, max relative distance to the closed-form root by iteration:", {i: "%.1e" % r for i, r in rel.items()},
          " max |gamma_y| %.3e" % np.abs(root).max())
    assert count >= 4 and rel[count] <= 1e-13 and rel[count - 1] <= 1e-11
