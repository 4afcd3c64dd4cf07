"""Error-dynamics regression with one feature list per regressed row on the shared store (lmpc_set_regression_laps_rows,
csrc/lmpc_reg_rows_kernel.hip) against the CPU restatement.  Needs an MI355X.

The reference is regression_rows_cases.rows_reference: oracle.regression.regress_batch once per row, with that row's lists and
out_rows = (r,).  The bound is the kernel family's, |got - ref| <= 1e-9 (1 + max|ref|) per array and query
(tests/test_gpu_regression.py); a row the oracle finds no candidate for comes back with the nominal linearisation's bits."""
import numpy as np
import pytest
import torch

from oracle import params as P, regression as R
from regression_rows_cases import ROWS_245, ROWS_444, ROWS_555, flat, queries_on_samples, rel_err, row_masks, rows_reference
from test_gpu_regression import recorded_laps
from test_regression_oracle import perturbed_plant_laps, planted_pairs
from tolerances import TOL_TWIN

pytestmark = pytest.mark.gpu

H = 0.6
BOUND = 1e-9


def _solver(pkg, N):
    return pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)


def _refused(pkg, code, call):
    with pytest.raises(pkg.capi.LmpcError, match=r"-> %d:" % code):
        call()


def _lin_and_regress(sv, inp):
    A0, B0, g0 = sv.linearize(inp)
    A, Bm, g = sv.regress(inp, A0.clone(), B0.clone(), g0.clone())
    return tuple(t.cpu().numpy() for t in (A0, B0, g0)), tuple(t.cpu().numpy() for t in (A, Bm, g))


def _reference(veh, laps, rows, h, inp, lin, as_written=False):
    N = inp["X_ref"].shape[1]
    return rows_reference(veh, laps, rows, h, flat(inp["X_ref"][:, :N - 1, :]), flat(inp["U_ref"]), *(flat(a) for a in lin),
                          as_written=as_written)


def _hold_to_reference(got, ref, lin, touched, rows, what):
    """A, B, g of every query within the bound; every entry outside a touched row's lists with the nominal bits.  Returns the worst
    relative error."""
    worst = 0.0
    for a, r in zip(got, ref[:3]):
        e = rel_err(flat(a), r)
        print("%s: worst %.1e relative to 1 + max|ref| at query %d" % (what, e.max(), int(np.argmax(e))))
        worst = max(worst, float(e.max()))
    assert worst < BOUND, (what, worst)
    may = [np.zeros(flat(a).shape, bool) for a in lin]
    for o, masks in enumerate(row_masks(rows)):
        for m, mask in zip(may, masks):
            m |= touched[o].reshape((-1,) + (1,) * mask.ndim) & mask
    for a, a0, m in zip(got, lin, may):
        assert np.array_equal(flat(a)[~m], flat(a0)[~m]), what
    return worst


# ---- 1. every row on its own lists --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_written", [False, True])
@pytest.mark.parametrize("B,N", [(7, 12), (1, 3)])
def test_every_row_is_regressed_on_its_own_lists(pkg, B, N, as_written):
    veh = P.barc_vehicle()
    laps = recorded_laps(veh)
    assert sum(l[0].shape[0] - 1 for l in laps) % 4 != 0 and (B * (N - 1)) % 64 != 0
    inp = queries_on_samples(laps, N, B, seed=11 + B)
    sv = _solver(pkg, N)
    sv.set_regression_laps(laps, rows=ROWS_444, dist_max=H, as_written=as_written)
    lin, got = _lin_and_regress(sv, inp)
    sv.set_regression_laps(laps, dist_max=H, as_written=as_written)       # the one-list (5, 3) kernel on the same laps
    _, one_list = _lin_and_regress(sv, inp)
    sv.close()
    ref = _reference(veh, laps, ROWS_444, H, inp, lin, as_written)
    touched = ref[3]
    assert touched.all()                                                  # the queries sit next to samples
    _hold_to_reference(got, ref, lin, touched, ROWS_444, "rows 4/4/4 B %d N %d as_written %s" % (B, N, as_written))
    # not the one-list answer: a kernel that ignored the per-row lists would not pass
    assert max(rel_err(flat(a), flat(o)).max() for a, o in zip(got, one_list)) > 1e3 * BOUND


# ---- 2. different lengths per row ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [ROWS_245, {4: ((3, 4, 5), (1,)), 3: ((3,), (0,))}, {5: ((2, 3, 4, 5), (1,))}, {3: ((4, 3), ())}],
                         ids=["2_4_5", "two_rows", "one_row", "no_control"])
def test_rows_of_different_lengths(pkg, rows):
    B, N = 7, 12
    veh = P.barc_vehicle()
    laps = recorded_laps(veh)
    inp = queries_on_samples(laps, N, B, seed=5)
    sv = _solver(pkg, N)
    sv.set_regression_laps(laps, rows=rows, dist_max=H)
    lin, got = _lin_and_regress(sv, inp)
    sv.close()
    ref = _reference(veh, laps, rows, H, inp, lin)
    assert ref[3].all()
    _hold_to_reference(got, ref, lin, ref[3], rows, "rows %s" % (rows,))   # ... which holds every column outside a row's lists to the nominal bits
    assert np.abs(flat(got[0]) - flat(lin[0])).max() > 1e-6


# ---- 3. a row without candidates ----------------------------------------------------------------------------------------------------
def test_a_row_without_candidates_is_left_alone_while_the_others_are_corrected(pkg):
    B, N = 7, 12
    veh = P.barc_vehicle()
    laps = recorded_laps(veh)
    inp = queries_on_samples(laps, N, B, seed=6)
    far = np.zeros((N, B), bool)
    far[::2, ::2] = True
    inp["X_ref"][2][far] += 10.0        # the heading error: only the yaw-rate row of ROWS_245 lists it
    sv = _solver(pkg, N)
    sv.set_regression_laps(laps, rows=ROWS_245, dist_max=H)
    lin, got = _lin_and_regress(sv, inp)
    sv.close()
    ref = _reference(veh, laps, ROWS_245, H, inp, lin)
    touched, farq = ref[3], flat(far[None, :N - 1, :])[:, 0]
    assert touched[0].all() and touched[1].all() and not touched[2][farq].any() and touched[2][~farq].all()    # the oracle agrees
    _hold_to_reference(got, ref, lin, touched, ROWS_245, "yaw-rate row out of reach")
    A, Bm, g = (torch.from_numpy(flat(a)) for a in got)
    A0, B0, g0 = (torch.from_numpy(flat(a)) for a in lin)
    fq = torch.from_numpy(farq)
    assert torch.equal(A[fq][:, 5], A0[fq][:, 5]) and torch.equal(Bm[fq][:, 5], B0[fq][:, 5]) and torch.equal(g[fq][:, 5], g0[fq][:, 5])
    assert not torch.equal(A[fq][:, 3], A0[fq][:, 3]) and not torch.equal(A[fq][:, 4], A0[fq][:, 4])


# ---- 4. equal lists reduce to the one-list kernel -----------------------------------------------------------------------------------
def test_equal_lists_give_the_one_list_answer(pkg):
    B, N = 7, 12
    veh = P.barc_vehicle()
    laps = recorded_laps(veh)
    inp = queries_on_samples(laps, N, B, seed=7)
    sv = _solver(pkg, N)
    sv.set_regression_laps(laps, rows=ROWS_555, dist_max=H)
    lin, got = _lin_and_regress(sv, inp)
    sv.set_regression_laps(laps, in_state=(3, 4, 5), in_ctrl=(0, 1), dist_max=H)
    _, one_list = _lin_and_regress(sv, inp)
    sv.close()
    for a, o, a0 in zip(got, one_list, lin):
        assert rel_err(flat(a), flat(o)).max() < BOUND
        assert np.abs(o - a0).max() > 1e-6


# ---- 5. it reaches the QP -----------------------------------------------------------------------------------------------------------
# throttle only in the vx row, steering only in the vy and yaw-rate rows: columns (vx, vy, w, u0, u1, 1)
GAIN = np.array([[0.02, 0.0, 0.01, 0.5, 0.0, 0.001], [0.0, -0.03, 0.0, 0.0, 0.02, 0.0], [0.01, 0.0, 0.0, 0.0, 0.1, -0.002]])


def test_per_row_fit_recovers_a_planted_error_model_and_enters_the_solve(pkg):
    """The solve entry points take no prepared linearisation, so the solve itself is held to two things: the stage matrices of
    lmpc_linearize_batch + lmpc_regress_batch against the oracle (stage matrices only), and, with equal lists on every row, the
    solve through the workspace-layout rows kernel against the solve through the one-list kernel."""
    veh = P.barc_vehicle()
    sv = _solver(pkg, 10)
    tr = pkg.workloads.synthetic_track("barc")
    laps = planted_pairs(veh, 400, 5, GAIN)
    x = np.tile(np.array([1.0, 0.0, 0.0, 1.6, 0.0, 0.0]), (8, 1))
    inp = sv.prepare(tr, x.T.copy(), 0.025)
    inp["u_ic"] = torch.zeros((2, 8), dtype=torch.float64, device="cuda")
    base = sv.solve(inp)["X_optm"].cpu().numpy()
    sv.set_regression_laps(laps, rows=ROWS_444, dist_max=3.0)
    lin, got = _lin_and_regress(sv, inp)
    dA, dB = (got[0] - lin[0])[3:, 3:6, 0, 0], (got[1] - lin[1])[3:, :, 0, 0]
    assert np.allclose(dA, GAIN[:, :3], atol=2e-2)                   # the planted error model, with its sign
    assert np.allclose(dB[1:, 1], GAIN[1:, 4], atol=2e-2)            # steering where the row lists it
    assert dB[0, 1] == 0.0 and dB[1, 0] == 0.0 and dB[2, 0] == 0.0   # and nothing where it does not
    inp_np = {k: inp[k].cpu().numpy() for k in ("X_ref", "U_ref")}
    ref = _reference(veh, laps, ROWS_444, 3.0, inp_np, lin)
    _hold_to_reference(got, ref, lin, ref[3], ROWS_444, "planted pairs, stage matrices")
    results = lambda out: {k: out[k].cpu().numpy() for k in ("X_optm", "U_optm", "dU_optm", "status")}     # noqa: E731
    with_rows = sv.solve(inp)
    assert (with_rows["status"].cpu().numpy() == 0).all()
    assert np.abs(with_rows["X_optm"].cpu().numpy() - base).max() > 1e-6      # the corrected model reaches the QP
    sv.set_regression_laps(laps, rows=ROWS_555, dist_max=3.0)
    equal_rows = results(sv.solve(inp))
    sv.set_regression_laps(laps, dist_max=3.0)
    one_list = results(sv.solve(inp))
    assert (equal_rows["status"] == 0).all() and (one_list["status"] == 0).all()
    for key, scale in (("X_optm", P.SCALE_X), ("U_optm", P.SCALE_U), ("dU_optm", P.SCALE_U)):
        assert np.abs((equal_rows[key] - one_list[key]) / scale[:, None, None]).max() < TOL_TWIN, key
    assert np.abs(one_list["X_optm"] - with_rows["X_optm"].cpu().numpy()).max() > 1e-9   # per-row lists: another model, another plan
    sv.set_regression_laps([], rows=ROWS_444)
    assert np.abs(sv.solve(inp)["X_optm"].cpu().numpy() - base).max() == 0.0
    sv.close()


# ---- 6. it does its job -------------------------------------------------------------------------------------------------------------
def test_per_row_regression_reduces_the_one_step_error_of_a_perturbed_plant(pkg):
    """Laps recorded on a plant with less grip and more mass, linearisation about recorded samples: the corrected (A, B, g) predicts
    the plant's next state better than the nominal linearisation (the oracle's value for these lists: 0.36 of the nominal error)."""
    veh = P.barc_vehicle()
    laps, _ = perturbed_plant_laps(veh)
    idx = list(range(0, 600, 25))
    B, N = len(idx), 3
    sv = _solver(pkg, N)
    X = np.zeros((6, N, B)); U = np.zeros((2, N - 1, B)); K = np.zeros((N, B))
    for b, j in enumerate(idx):
        X[:, :, b] = laps[j][0][0][:, None]
        U[:, :, b] = laps[j][1][0][:, None]
        K[:, b] = laps[j][2][0]
    inp = {"X_ref": X, "U_ref": U, "T_ref": np.full((N - 1, B), 0.03), "curvatures": K}
    truth = np.stack([laps[j][0][1] for j in idx], axis=1)        # [6][B]

    def one_step_error(A, Bm, g):
        pred = np.einsum("rcb,cb->rb", A[:, :, 0], X[:, 0]) + np.einsum("rcb,cb->rb", Bm[:, :, 0], U[:, 0]) + g[:, 0]
        return np.median(np.abs(pred - truth)[3:].max(axis=0))

    sv.set_regression_laps(laps, rows=ROWS_444, dist_max=H)
    lin, got = _lin_and_regress(sv, inp)
    sv.close()
    e0, e1 = one_step_error(*lin), one_step_error(*got)
    print("median one-step error: nominal %.4f, per-row regression %.4f (%.2f)" % (e0, e1, e1 / e0))
    assert e1 < 0.4 * e0, (e0, e1)


# ---- 7. refusals and state ----------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_the_two_forms_replace_each_other(pkg):
    B, N = 6, 8
    veh = P.barc_vehicle()
    laps = recorded_laps(veh, n_laps=2, n=40)
    inp = queries_on_samples(laps, N, B, seed=8)
    sv = _solver(pkg, N)
    lin = sv.linearize(inp)

    def answer():
        return [t.cpu().numpy() for t in sv.regress(inp, *[t.clone() for t in lin])]

    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    _refused(pkg, -1, lambda: sv.regress(inp, *[t.clone() for t in lin]))                      # nothing set yet
    sv.set_regression_laps(laps, rows=ROWS_444, dist_max=H)
    rows_answer = answer()
    assert not same(rows_answer, [t.cpu().numpy() for t in lin])
    s345 = (3, 4, 5)
    refusals = [
        (-3, dict(rows={2: (s345, (0,)), 3: (s345, (0,)), 4: (s345, (1,)), 5: (s345, (1,))})),   # 4 rows
        (-3, dict(rows={3: ((0, 1, 2, 3, 4, 5), ()), 4: (s345, (1,))})),                        # 6 features in a row
        (-3, dict(rows={3: ((1, 2, 3, 4), (0, 1))})),                                           # 6 features in a row, with controls
        (-3, dict(rows={3: ((), (0,)), 4: (s345, (1,))})),                                      # zero state features
        (-1, dict(rows={3: ((3, 4, 3), (0,))})),                                                # duplicate feature state
        (-1, dict(rows={3: (s345, (1, 1))})),                                                   # duplicate feature control
        (-1, dict(rows=[(3, (s345, (0,))), (3, (s345, (1,)))])),                                # the same row twice (see below)
        (-1, dict(rows={3: ((3, 4, 6), (0,))})),                                                # index 6
        (-1, dict(rows={6: (s345, (0,))})),                                                     # regressed row 6
        (-1, dict(rows={3: (s345, (2,))})),                                                     # control 2
        (-1, dict(rows=ROWS_444, dist_max=0.0)),
    ]
    for code, kw in refusals:
        kw.setdefault("dist_max", H)
        rows = kw.pop("rows")
        if isinstance(rows, list):       # a duplicate row cannot be written as a dict: hand the struct over directly
            import ctypes as C
            spec = pkg.capi._rows_spec({}, kw["dist_max"], False)
            spec.n_out = len(rows)
            for o, (r, (ins, inc)) in enumerate(rows):
                spec.out[o], spec.n_in_state[o], spec.n_in_ctrl[o] = r, len(ins), len(inc)
                spec.in_state[o][:len(ins)] = list(ins)
                spec.in_ctrl[o][:len(inc)] = list(inc)
            n_pts = np.array([l[0].shape[0] for l in laps], dtype=np.int32)
            cat = [np.ascontiguousarray(np.concatenate([np.asarray(l[i], dtype=np.float64).reshape(n, -1) for l, n in zip(laps, n_pts)], 0))
                   for i in range(4)]
            rc = sv.lib.lmpc_set_regression_laps_rows(sv._h, C.c_int32(len(laps)), n_pts.ctypes.data_as(C.c_void_p),
                                                      *[a.ctypes.data_as(C.c_void_p) for a in cat], C.byref(spec))
            assert rc == code, (rc, rows)
        else:
            _refused(pkg, code, lambda: sv.set_regression_laps(laps, rows=rows, **kw))
        assert same(answer(), rows_answer), (code, rows)                                        # the spec in effect before is still in effect
    with pytest.raises(ValueError):
        sv.set_regression_laps(laps, rows=ROWS_444, in_state=(3, 4), dist_max=H)                # rows= excludes the one-list keywords
    # the fp32 entry while on
    kw32 = dict(dtype=torch.float32, device="cuda")
    out32 = {"X_optm": torch.full((6, N, B), 7.0, **kw32), "U_optm": torch.full((2, N - 1, B), 7.0, **kw32),
             "dU_optm": torch.full((2, N - 1, B), 7.0, **kw32), "kkt": torch.full((4, B), 7.0, **kw32),
             "status": torch.full((B,), 7, dtype=torch.int32, device="cuda"), "iters": torch.full((B,), 7, dtype=torch.int32, device="cuda")}
    tr = pkg.workloads.synthetic_track("barc")
    full = sv.prepare(tr, np.tile(np.array([1.0, 0.0, 0.0, 1.6, 0.0, 0.0]), (B, 1)).T.copy(), 0.025)
    full["u_ic"] = torch.zeros((2, B), dtype=torch.float64, device="cuda")
    _refused(pkg, -3, lambda: sv.solve_f32(full, out32))
    assert all(bool((out32[key] == 7).all()) for key in ("X_optm", "U_optm", "dU_optm", "status", "iters"))
    # the per-car regression on top of the shared rows-spec, in either form; and the reverse
    sv.fleet_ss_create(B, 16)
    bytes_off = sv.fleet_ss_bytes()
    _refused(pkg, -1, lambda: sv.fleet_ss_set_regression(rows=ROWS_444, dist_max=H))
    _refused(pkg, -1, lambda: sv.fleet_ss_set_regression(dist_max=H))
    assert sv.fleet_ss_bytes() == bytes_off and same(answer(), rows_answer)
    sv.set_regression_laps([])                                                                   # off ...
    _refused(pkg, -1, lambda: sv.regress(inp, *[t.clone() for t in lin]))
    sv.fleet_ss_set_regression(rows=ROWS_444, dist_max=H)
    bytes_on = sv.fleet_ss_bytes()
    assert bytes_on > bytes_off
    _refused(pkg, -1, lambda: sv.set_regression_laps(laps, rows=ROWS_444, dist_max=H))
    _refused(pkg, -1, lambda: sv.set_regression_laps(laps, dist_max=H))
    _refused(pkg, -3, lambda: sv.fleet_ss_set_regression(rows={3: ((), (0,))}, dist_max=H))
    _refused(pkg, -1, lambda: sv.fleet_ss_set_regression(rows={3: ((3, 3), (0,))}, dist_max=H))
    assert sv.fleet_ss_bytes() == bytes_on
    sv.fleet_ss_regress(inp, *[t.clone() for t in lin])                                          # ... and it is still on
    sv.fleet_ss_set_regression(off=True)
    assert sv.fleet_ss_bytes() == bytes_off
    sv.fleet_ss_destroy()
    sv.set_regression_laps(laps, rows=ROWS_444, dist_max=H)                                      # ... and on again: the same bits
    assert same(answer(), rows_answer)
    # either form replaces the other
    sv.set_regression_laps(laps, dist_max=H)
    one_list_answer = answer()
    assert not same(one_list_answer, rows_answer)
    sv.set_regression_laps(laps, rows=ROWS_444, dist_max=H)
    assert same(answer(), rows_answer)
    sv.set_regression_laps(laps, dist_max=H)
    assert same(answer(), one_list_answer)
    sv.close()
