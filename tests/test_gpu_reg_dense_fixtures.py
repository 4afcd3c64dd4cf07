"""GPU: solves with the error-dynamics regression switched on, against the DENSE optimum of the oracle's regressed QP (tests/dense_cases.py
REG_CASES, tests/golden/dense_reg_*.npz).  The reference model never comes from the product: oracle linearisation + oracle regression +
build_qp(lin=...).  What this pins that the operation-level test (tests/test_gpu_regression.py, lmpc_regress_batch's separate A/B/g
arrays) cannot: the regression's write into the solve's linearisation records (lmpc_regress_kernel<., ., true>), read by the one-wave
kernel (N = 20) and by the two-wave kernel's own loader (N = 60), and the (8, 6) instance inside a solve at IAC scale."""
import numpy as np
import pytest
import torch

import dense_cases as DC
from oracle import params as P
from parity import per_problem_err
from tolerances import TOL_DU, TOL_F32, TOL_XU

pytestmark = pytest.mark.gpu
GOLD = DC.__file__.rsplit("/", 1)[0] + "/golden"
SCALES = {"X_optm": P.SCALE_X[:, None, None], "U_optm": P.SCALE_U[:, None, None], "dU_optm": P.SCALE_U[:, None, None]}


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items() if hasattr(v, "cpu")}


def _setup(pkg, name):
    d = np.load(f"{GOLD}/dense_{name}.npz")
    fx = {k: d[k] for k in d.files}
    cfg, veh, inp, ss_x, ss_j, samples, spec, model = DC.build_reg(pkg, name)
    md, sd = DC.reg_digests(samples, model)
    np.testing.assert_allclose(DC.digest(inp, ss_x, ss_j), fx["digest"], rtol=1e-11, atol=0)
    np.testing.assert_allclose(md, fx["model_digest"], rtol=1e-11, atol=0)
    np.testing.assert_allclose(sd, fx["samples_digest"], rtol=1e-11, atol=0)
    family, N, _, _, dist_max, _ = DC.REG_CASES[name]
    if family in ("spc", "near"):
        pc, pv = pkg.presets.barc_lmpc(N, 5), pkg.presets.barc_vehicle()
    elif family == "trk":
        pc, pv = pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle()
    else:
        pc, pv = pkg.presets.iac_tracking_mpc(N), pkg.presets.iac_vehicle()
    sv = pkg.Solver(pc, pv, device=0)
    reg = lambda: sv.set_regression_laps(samples, in_state=spec[0], in_ctrl=spec[1], out_rows=spec[2], dist_max=dist_max)
    reg()
    ss = None if ss_x is None else (torch.as_tensor(ss_x, device="cuda"), torch.as_tensor(ss_j, device="cuda"))
    return fx, inp, sv, ss, reg


def _solve(sv, inp, ss, mixed=False, warm=None):
    B = inp["x_ic"].shape[-1]
    if ss is None:
        return _np(sv.solve(inp, mixed=mixed, warm=warm))
    o = sv.alloc_outputs(B)
    o["convex_combi_optm"] = torch.zeros((ss[0].shape[1], B), dtype=torch.float64, device="cuda")
    return _np(sv.solve(inp, o, ss_x=ss[0], ss_j=ss[1], mixed=mixed, warm=warm))


def _warm(sv, inp, ss, cold):
    ok = cold["status"] == 0
    w = {"X_optm_ref": torch.as_tensor(cold["X_optm"], device="cuda"), "U_optm_ref": torch.as_tensor(cold["U_optm"], device="cuda")}
    if ss is not None:
        w["convex_combi_optm_ref"] = torch.as_tensor(cold["convex_combi_optm"], device="cuda")
    out = _solve(sv, inp, ss, warm=w)
    err = max(float(np.abs((out[k] - cold[k]) / s)[..., ok].max()) for k, s in SCALES.items())
    return out, (out["status"] == 0).mean(), (out["iters"][ok] <= 2).mean(), err


@pytest.mark.parametrize("name,waves", [(n, 0) for n in DC.REG_CASES] + [("reg_barc_tracking_n60", 1)])
def test_regressed_solve_against_the_dense_optimum_of_the_oracles_model(pkg, name, waves):
    """Every problem: the dense solver's status, and X / U / dU within TOL_XU / TOL_DU (scaled) of its optimum.  Then the warm start
    (lmpc_solve_batch_warm, or _warm_ss with the simplex weights on the learning handle) from each regressed cold optimum: >= 99 %
    solved, within 1e-8 of the cold answer, and accepted within two rounds as often as on the same inputs with the regression off
    (98 % or the unregressed rate, whichever is lower, less one problem in 50)."""
    fx, inp, sv, ss, reg = _setup(pkg, name)
    sv.set_waves_per_problem(waves)
    cold = _solve(sv, inp, ss)
    B = fx["status"].size
    assert fx["touched"].sum() >= B * 10, fx["touched"].sum()
    assert np.array_equal(cold["status"] == 0, fx["status"] == 0), (np.nonzero(cold["status"] != fx["status"])[0], cold["status"][cold["status"] != 0])
    ok = fx["status"] == 0
    exu, ed = per_problem_err({k: cold[k][..., ok] for k in SCALES}, {k: fx[k][..., ok] for k in SCALES})
    worst = np.argsort(np.maximum(exu, ed))[-3:]
    _, solved, acc, ew = _warm(sv, inp, ss, cold)
    sv.set_regression_laps([])
    cold0 = _solve(sv, inp, ss)
    _, solved0, acc0, ew0 = _warm(sv, inp, ss, cold0)
    sv.close()
    print("%s (waves %d): %d problems (%d dense-optimal), %d stages regressed; kernel vs dense X/U max %.1e median %.1e, dU max %.1e; "
          "warm: solved %.3f, within two rounds %.3f (regression off: %.3f), vs cold %.1e"
          % (name, waves, B, ok.sum(), fx["touched"].sum(), exu.max(), np.median(exu), ed.max(), solved, acc, acc0, ew))
    assert exu.max() < TOL_XU and ed.max() < TOL_DU, (name, worst, exu[worst], ed[worst], fx["margin"][ok][worst])
    assert solved >= 0.99 and ew < 1e-8, (solved, ew)
    assert acc >= min(0.98, acc0) - 0.02, (acc, acc0)


def test_mixed_entry_and_safe_set_by_reference_on_the_regressed_learning_problem(pkg):
    """configs[4] on states near the laps: lmpc_solve_batch_mixed (fp32 iteration, fp64 arrays, the regression applied in fp64 in front)
    within TOL_F32 of the dense optimum on every problem (include/lmpc_hip.h's bound for this workload) and reported as "mixed"; and the
    safe set by reference (lmpc_ss_query_idx_batch + lmpc_solve_batch_ss_idx) gives the array solve's answer bit for bit with the
    regression on."""
    name = "reg_barc_lmpc_near_n20_s160"
    fx, inp, sv, ss, reg = _setup(pkg, name)
    om = _solve(sv, inp, ss, mixed=True)
    assert sv.last_solve_precision() == "mixed"
    assert (om["status"] == 0).all(), np.nonzero(om["status"])[0]
    exu, ed = per_problem_err(om, fx)
    print("%s mixed: X/U max %.1e median %.1e, dU max %.1e" % (name, exu.max(), np.median(exu), ed.max()))
    assert exu.max() < TOL_F32 and ed.max() < TOL_F32 / 0.025, (exu.max(), ed.max())
    tr = pkg.workloads.synthetic_track("barc")
    sv.set_safe_set(pkg.workloads.synthetic_laps(tr, 5), tr["L"])
    q = torch.as_tensor(DC.ss_query_point(inp, tr["L"]), device="cuda").contiguous()
    ss_x, ss_j, _ = sv.ss_query(q)
    idx, _ = sv.ss_query_idx(q)
    B = fx["status"].size
    outs = []
    for kw in ({"ss_x": ss_x, "ss_j": ss_j}, {"ss_idx": idx}):
        o = sv.alloc_outputs(B)
        o["convex_combi_optm"] = torch.zeros((ss_x.shape[1], B), dtype=torch.float64, device="cuda")
        outs.append(_np(sv.solve(inp, o, **kw)))
    sv.close()
    a, b = outs
    assert (a["status"] == 0).all()
    for k in ("X_optm", "U_optm", "dU_optm", "convex_combi_optm", "status", "iters"):
        assert np.array_equal(a[k], b[k]), k


def test_single_precision_entry_refuses_a_regressed_handle_and_solves_once_it_is_off(pkg):
    """lmpc_solve_batch_f32 has no regression: LMPC_ERR_UNSUPPORTED (-3) while the handle holds regression laps, a solve again after
    set_regression_laps([])."""
    name = "reg_barc_tracking_n20"
    fx, inp, sv, ss, reg = _setup(pkg, name)
    with pytest.raises(pkg.LmpcError, match=r"lmpc_solve_batch_f32 -> -3:"):
        sv.solve_f32(inp)
    sv.set_regression_laps([])
    out = sv.solve_f32(inp)
    st = out["status"].cpu().numpy()
    assert sv.last_solve_precision() == "f32"
    assert (st == 0).mean() > 0.95, np.bincount(st)
    sv.close()
