"""The spline track on the device (csrc/lmpc_track_kernel.hip): the interpolants, the lmpc_track tables, batched global -> Frenet
projection and Frenet -> global.  The projection is held to an independent oracle (scipy splines + brentq, tests/track_cases.py),
not to the host class, whose own accuracy in s is about 5e-7."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import track_cases as TC
from oracle import params as OP
from oracle.trajectory import TrackOracle
from tolerances import TOL_XU

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "racing-lmpc-ros2_amd" / "lib"

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver(pkg):
    return pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)


@pytest.fixture(scope="module", params=["barc", "synthetic"])
def case(request, pkg, solver):
    """Per track: the host class, the oracle, the device track, 20 000 poses with their generating Frenet states and the oracle's
    projection of every one of them."""
    tab = TC.table(request.param)
    tr, orc = pkg.racing_trajectory.RacingTrajectory(tab), TrackOracle(tab)
    dev = solver.spline_track(tr)
    frenet, pose, min_jac = TC.poses(tr)
    ref = TC.oracle_projection(orc, pose, frenet[0], dev.h_bar)
    return {"name": request.param, "tr": tr, "orc": orc, "dev": dev, "frenet": frenet, "pose": pose, "min_jac": min_jac, "ref": ref}


@pytest.fixture(scope="module")
def barc(pkg, solver):
    tr = pkg.racing_trajectory.RacingTrajectory(TC.BARC)
    return tr, solver.spline_track(tr)


def _errors(got, ref, L):
    return (np.abs(TC.wrap_diff(got[0], ref[0], L)).max(), np.abs(got[1] - ref[1]).max(), np.abs(got[2] - ref[2]).max())


def test_sample_and_tabulate(solver, case):
    tr, orc, dev = case["tr"], case["orc"], case["dev"]
    s = np.linspace(-3.0, 2.5 * tr.total_length, 2001)
    ref = orc.eval(s)
    got = solver.track_sample(dev, s).cpu().numpy()
    for row, k in enumerate(("x", "y", "yaw", "curvature", "left", "right", "vel")):
        err = np.abs(got[row] - ref[k]).max()
        print(case["name"], k, "%.2e" % err)
        assert err < TC.TOL_EVAL[k], (k, err)
    tab, host = solver.tabulate_track(dev, 512), tr.to_track_table(512)
    assert tab["M"] == 512 and tab["L"] == tr.total_length
    for k in ("curvature", "bound_left", "bound_right", "vel"):
        err = np.abs(tab[k].cpu().numpy() - host[k]).max()
        print(case["name"], "table", k, "%.2e" % err)
        assert err < TC.TOL_TABLE, (k, err)


def test_projection_against_the_oracle_root(solver, case):
    assert case["min_jac"] >= 0.6, case["min_jac"]       # 1 - kappa t: the poses stay clear of the evolute
    fr, st = solver.global_to_frenet(case["dev"], case["pose"])
    fr, st = fr.cpu().numpy(), st.cpu().numpy()
    es, et, exi = _errors(fr, case["ref"], case["tr"].total_length)
    print(case["name"], "min 1 - kappa t %.3f" % case["min_jac"], "status counts", np.bincount(st), "s %.2e t %.2e xi %.2e" % (es, et, exi))
    assert (st == 0).all(), np.bincount(st)
    assert es < TC.TOL_S and et < TC.TOL_T and exi < TC.TOL_XI, (es, et, exi)
    # and the abscissa the pose was generated from (the host class made the poses: its frenet_to_global is exact to rounding)
    es, et, exi = _errors(fr, case["frenet"], case["tr"].total_length)
    assert es < TC.TOL_S and et < TC.TOL_T and exi < TC.TOL_XI, (es, et, exi)


def test_seeded_projection_and_mixed_mask(solver, case):
    dev, pose, L = case["dev"], case["pose"], case["tr"].total_length
    n = pose.shape[1]
    rng = np.random.default_rng(5)
    s0 = case["frenet"][0] + rng.uniform(-3.0, 3.0, n) * dev.h_bar
    plain, st_p = solver.global_to_frenet(dev, pose)
    seeded, st_s = solver.global_to_frenet(dev, pose, s0=s0)
    assert (st_p.cpu().numpy() == 0).all() and (st_s.cpu().numpy() == 0).all()
    es, et, exi = _errors(seeded.cpu().numpy(), plain.cpu().numpy(), L)
    print(case["name"], "seeded vs unseeded: s %.2e t %.2e xi %.2e" % (es, et, exi))
    assert es < 1e-9 and et < 1e-9 and exi < 1e-8
    mask = (rng.uniform(size=n) < 0.5).astype(np.int32)
    mixed, st_m = solver.global_to_frenet(dev, pose, s0=s0, seeded=mask)
    want = np.where(mask[None, :] != 0, seeded.cpu().numpy(), plain.cpu().numpy())
    assert np.array_equal(mixed.cpu().numpy(), want) and (st_m.cpu().numpy() == 0).all()


def test_projection_against_the_host_class(solver, case):
    tr, pose = case["tr"], case["pose"][:, :512]
    fr = solver.global_to_frenet(case["dev"], pose)[0].cpu().numpy()
    host = np.array([tr.global_to_frenet(*[float(v) for v in pose[:, b]]) for b in range(512)]).T
    es, et, exi = _errors(fr, host, tr.total_length)
    print(case["name"], "vs host global_to_frenet: s %.2e t %.2e xi %.2e" % (es, et, exi))
    assert es < 1e-6 and et < 1e-6 and exi < 1e-6


def test_frenet_to_global_of_a_plan_and_the_round_trip(solver, case):
    import torch
    tr, dev, L = case["tr"], case["dev"], case["tr"].total_length
    rng = np.random.default_rng(7)
    n, B = 20, 4096
    X = np.zeros((6, n, B))
    X[0] = rng.uniform(-0.5 * L, 1.5 * L, (n, B))          # a plan's abscissa runs past the start line
    u = rng.uniform(-0.9, 0.9, (n, B))
    X[1] = np.where(u >= 0, u * tr.left_boundary(X[0]), -u * tr.right_boundary(X[0]))
    X[2] = rng.uniform(-0.5, 0.5, (n, B))
    X[3:] = rng.normal(size=(3, n, B))
    got = solver.frenet_to_global(dev, X).cpu().numpy()
    hx, hy, hyaw = tr.frenet_to_global(X[0], X[1], X[2])
    ex, ey = np.abs(got[0] - hx).max(), np.abs(got[1] - hy).max()
    eyaw = np.abs(np.arctan2(np.sin(got[2] - hyaw), np.cos(got[2] - hyaw))).max()
    print(case["name"], "frenet_to_global vs host: x %.2e y %.2e yaw %.2e" % (ex, ey, eyaw))
    assert got.shape == (3, n, B) and ex < 1e-10 and ey < 1e-10 and eyaw < 1e-8
    # car states [6][B] take the same path, and the projection brings every element back
    x6 = torch.as_tensor(X[:, 3, :], device=solver.device).contiguous()
    pose = solver.frenet_to_global(dev, x6)
    assert np.array_equal(pose.cpu().numpy(), got[:, 3, :])
    back, st = solver.global_to_frenet(dev, torch.as_tensor(got.reshape(3, n * B), device=solver.device), s0=X[0].reshape(-1))
    es, et, exi = _errors(back.cpu().numpy(), X[:3].reshape(3, -1), L)
    print(case["name"], "round trip: s %.2e t %.2e xi %.2e" % (es, et, exi))
    assert (st.cpu().numpy() == 0).all() and es < 1e-9 and et < 1e-9 and exi < 1e-8


def test_bad_input_is_flagged_and_leaves_its_neighbours_alone(solver, case, pkg):
    dev, tr = case["dev"], case["tr"]
    pose = case["pose"][:, :256].copy()
    clean, st0 = solver.global_to_frenet(dev, pose)
    clean, st0 = clean.cpu().numpy(), st0.cpu().numpy()
    dirty = pose.copy()
    bad = {3: (0, np.nan), 17: (1, np.inf), 64: (2, -np.inf), 65: (0, -np.inf), 130: (2, np.nan), 255: (1, np.nan)}
    for b, (row, v) in bad.items():
        dirty[row, b] = v
    got, st = solver.global_to_frenet(dev, dirty)
    got, st = got.cpu().numpy(), st.cpu().numpy()
    keep = np.ones(256, dtype=bool)
    keep[list(bad)] = False
    assert (st[~keep] == pkg.TRACK_BAD_INPUT).all() and np.isnan(got[:, ~keep]).all()
    assert np.array_equal(got[:, keep], clean[:, keep]) and np.array_equal(st[keep], st0[keep]) and (st0 == 0).all()
    # a pose at three times the boundary offset is still projected
    s = case["frenet"][0, :256]
    far = np.stack(tr.frenet_to_global(s, 3.0 * tr.left_boundary(s), np.zeros(256)))
    _, st_far = solver.global_to_frenet(dev, far)
    assert (st_far.cpu().numpy() == 0).all()


def test_two_calls_are_bit_identical(solver, case):
    a = solver.global_to_frenet(case["dev"], case["pose"])
    b = solver.global_to_frenet(case["dev"], case["pose"])
    assert np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy()) and np.array_equal(a[1].cpu().numpy(), b[1].cpu().numpy())
    X = np.concatenate([case["frenet"], np.zeros_like(case["frenet"])])
    assert np.array_equal(solver.frenet_to_global(case["dev"], X).cpu().numpy(), solver.frenet_to_global(case["dev"], X).cpu().numpy())


def test_argument_errors(solver, barc, pkg):
    import torch
    _, dev = barc
    d = barc[0].to_spline_track()
    with pytest.raises(pkg.LmpcError):
        solver.spline_track(dict(d, breaks=d["breaks"][::-1].copy()))
    with pytest.raises(pkg.LmpcError):
        solver.spline_track(dict(d, L=-1.0))
    pose = torch.zeros((3, 4), dtype=torch.float64, device=solver.device)
    rc = solver.lib.lmpc_global_to_frenet_batch(solver._h, dev._p, C.c_int32(4), C.c_void_p(pose.data_ptr()), None, None, None, None)
    assert rc == -1 and b"lmpc_global_to_frenet_batch" in solver.lib.lmpc_last_error(solver._h)


def test_closed_loop_through_the_global_frame(pkg, solver, barc):
    """run_global against run from the same x0: 4096 cars, 200 periods on the BARC track.  The two conversions are the identity on
    (s, e_y, e_psi) up to rounding, so the loops stay within the project's 1e-6 scaled contract of each other."""
    import torch
    tr, dev = barc
    tab = tr.to_track_table(1024)
    B = 4096
    rng = np.random.default_rng(1)
    s0 = rng.uniform(0, tab["L"], B)
    x0 = np.stack([s0, rng.uniform(-0.05, 0.05, B), np.zeros(B), 0.8 * np.interp(s0, np.arange(1024) * tab["L"] / 1024, tab["vel"]),
                   np.zeros(B), np.zeros(B)])
    x0 = torch.as_tensor(x0, device=solver.device)
    u0 = torch.zeros((2, B), dtype=torch.float64, device=solver.device)
    a = pkg.closed_loop.run(solver, tab, x0, u0, steps=200)
    b = pkg.closed_loop.run_global(solver, tab, dev, x0, u0, steps=200)
    assert (b["track_status"].cpu().numpy() == 0).all()
    fa, fb = a["n_fail"].cpu().numpy(), b["n_fail"].cpu().numpy()
    xa, xb = a["x"].cpu().numpy(), b["x"].cpu().numpy()
    d = xb - xa
    d[0] = TC.wrap_diff(xb[0], xa[0], tab["L"])
    err = np.abs(d / OP.SCALE_X[:, None]).max(axis=1)
    print("n_fail", fa.sum(), fb.sum(), "scaled final-state difference per component", err)
    assert np.array_equal(fa, fb)
    assert err.max() < TOL_XU, err


def test_cpp_facade_driver():
    exe = LIB / "test_device_track"
    assert exe.exists(), "run __graft_entry__.build() first"
    r = subprocess.run([str(exe), str(TC.BARC), "4096"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), (r.stdout[-2000:], r.stderr[-2000:])
