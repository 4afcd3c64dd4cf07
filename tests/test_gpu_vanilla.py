"""The batched vanilla controller on the device (lmpc_vanilla_*) against the plain numpy restatement of tests/vanilla_cases.py.

Tolerances, elementwise |d| / max(1, |reference|): vanilla_cases.TOL = 1e-9 for one decision and TOL_ROLLOUT = 1e-8 for a rollout of
up to 64 periods -- 1e4 times the restatement's measured distance from its extended-precision twin on the same scenarios at the same
batch sizes (tests/test_vanilla_reference.py): room for the device's atan2 / sin / hypot / tanh and for FMA contraction in the plant,
each carried through the closed loop; a wrong term shows at 1e-3 or more.  Every scenario is one the CPU gate has qualified."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import vanilla_cases as VC

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "racing-lmpc-ros2_amd" / "lib"

pytestmark = pytest.mark.gpu


class Rig:
    """A solver over a scenario's vehicle with the scenario's track on the device."""

    def __init__(self, pkg, sc):
        veh = dict(pkg.presets.barc_vehicle() if sc["vehicle"] == "barc" else pkg.presets.iac_vehicle(), **sc["veh_over"])
        self.pkg, self.sc = pkg, sc
        self.solver = pkg.Solver(pkg.presets.barc_tracking_mpc(20), veh, device=0)
        self.spline = self.solver.spline_track(sc["trk"]["spline"])
        self.table = self.solver.device_track(sc["trk"]["table"])


@pytest.fixture(scope="module")
def rigs(pkg):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Rig(pkg, VC.scenario(name))
        return made[name]

    return get


def dev(solver, a):
    """[B, ...] on the host -> [...][B] on the device."""
    import torch
    return torch.as_tensor(np.ascontiguousarray(np.moveaxis(np.asarray(a, dtype=np.float64), 0, -1)), device=solver.device)


def host(t):
    return np.moveaxis(t.cpu().numpy(), -1, 0)


def pid_of(solver, B):
    g = solver.vanilla_get(B)
    return {k: g[k].cpu().numpy() for k in VC.PID_KEYS}


def device_decide(rig, x, vel_ref=None, speed_scale=None, cfg=None, integral=None, **kw):
    s, sc = rig.solver, rig.sc
    B = x.shape[0]
    s.vanilla_create(sc["cfg"] if cfg is None else cfg, B)
    if integral is not None:
        s.vanilla_reset(B, dev(s, integral))
    out = s.vanilla_solve(rig.spline, dev(s, x), None if vel_ref is None else dev(s, vel_ref),
                          speed_scale=sc["speed_scale"] if speed_scale is None else speed_scale, **kw)
    s.synchronize()
    got = {k: host(v) for k, v in out.items() if v is not None}
    got["pid"] = pid_of(s, B)
    return got


def device_rollout(rig, x0, periods, chunks=1, distance=None, worst=None, logs=True):
    """The scenario's rollout from a zero PID state: numpy arrays [B, ...] like the restatement's."""
    import torch
    s, sc = rig.solver, rig.sc
    B = x0.shape[0]
    s.vanilla_create(sc["cfg"], B)
    x = dev(s, x0)
    kw = dict(dtype=torch.float64, device=s.device)
    dist = torch.zeros(B, **kw) if distance is None else dev(s, distance)
    wst = torch.full((B,), -np.inf, **kw) if worst is None else dev(s, worst)
    parts, flags = [], np.zeros(B, dtype=np.int32)
    for _ in range(chunks):
        out = s.vanilla_rollout(rig.spline, rig.table, x, periods // chunks, sc["dt_sim"], sc["n_sub"], speed_scale=sc["speed_scale"],
                                logs=logs, distance=dist, worst_excess=wst)
        parts.append(out)
        flags |= out["flags"].cpu().numpy()
    s.synchronize()
    got = {"x": host(x), "distance": dist.cpu().numpy(), "worst_excess": wst.cpu().numpy(), "flags": flags, "pid": pid_of(s, B)}
    if logs:
        import torch as _t
        for k in ("X_log", "U_log", "k_log"):
            got[k] = host(_t.cat([p[k] for p in parts], dim=-2))
    return got


def check_decision(got, ref):
    worst = VC.decision_err(got, ref)
    print("decision %.1e" % worst)
    assert got["u_out"].shape == ref["u_out"].shape and got["u_model"].shape == ref["u_model"].shape
    assert worst <= VC.TOL, worst
    assert not got["flags"].any()


def check_rollout(got, ref):
    worst = {k: VC.err(got[k], ref[k]) for k in VC.ROLLOUT_KEYS}
    worst["pid"] = max(VC.err(got["pid"][k], ref["pid"][k]) for k in VC.PID_KEYS)
    print({k: "%.1e" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= VC.TOL_ROLLOUT, (k, v)
    assert not got["flags"].any()


# ---- solve ----
@pytest.mark.parametrize("given", (False, True), ids=("spline_vel", "vel_ref"))
@pytest.mark.parametrize("name", VC.SCENARIOS)
def test_solve_parity(rigs, name, given):
    """B = 67: one full wave and a partial one; u_out, u_model and the PID state of every car."""
    rig = rigs(name)
    sc = rig.sc
    check_decision(device_decide(rig, sc["x0"], sc["vel_ref"] if given else None), VC.reference(name, "decide_ref" if given else "decide"))


def test_solve_one_car(rigs):
    rig = rigs("barc")
    ref = VC.reference("barc", "decide")
    got = device_decide(rig, rig.sc["x0"][:1])
    one = {"u_out": ref["u_out"][:1], "u_model": ref["u_model"][:1], "pid": {k: v[:1] for k, v in ref["pid"].items()}}
    check_decision(got, one)


def test_solve_optional_outputs_and_repeatability(rigs):
    import torch
    rig = rigs("preset2")
    s, sc = rig.solver, rig.sc
    full = device_decide(rig, sc["x0"])
    bare = device_decide(rig, sc["x0"], out={"u_out": torch.empty((3, VC.B_TEST), dtype=torch.float64, device=s.device)})
    assert set(bare) == {"u_out", "pid"} and np.array_equal(bare["u_out"], full["u_out"])
    assert all(np.array_equal(bare["pid"][k], full["pid"][k]) for k in VC.PID_KEYS)
    # a second decision on the same store moves the PID state on; from a reset store the first one repeats bit for bit
    x = dev(s, sc["x0"])
    second = s.vanilla_solve(rig.spline, x, None, speed_scale=sc["speed_scale"])
    assert not np.array_equal(host(second["u_out"]), full["u_out"])          # (k_d = 0.1: the first call's derivative kick is gone)
    assert np.array_equal(pid_of(s, VC.B_TEST)["last_error"], full["pid"]["error"])
    s.vanilla_reset(VC.B_TEST)
    again = s.vanilla_solve(rig.spline, x, None, speed_scale=sc["speed_scale"])
    s.synchronize()
    for k in ("u_out", "u_model", "flags"):
        assert np.array_equal(host(again[k]), full[k]), k
    assert all(np.array_equal(pid_of(s, VC.B_TEST)[k], full["pid"][k]) for k in VC.PID_KEYS)
    # reset with an integral: error and last_error zero, the integral as given
    s.vanilla_reset(VC.B_TEST, torch.full((VC.B_TEST,), 0.25, dtype=torch.float64, device=s.device))
    p = pid_of(s, VC.B_TEST)
    assert (p["integral"] == 0.25).all() and (p["error"] == 0).all() and (p["last_error"] == 0).all()


# ---- rollout ----
@pytest.mark.parametrize("periods", (1, 2, VC.PERIODS))
@pytest.mark.parametrize("name", VC.SCENARIOS)
def test_rollout_parity(rigs, name, periods):
    rig = rigs(name)
    check_rollout(device_rollout(rig, rig.sc["x0"], periods), VC.reference(name, "rollout", periods))


def test_rollout_chunks_and_optional_outputs(rigs):
    """Two launches of 32 periods leave the bits of one of 64 -- state, logs, accumulators, PID state; without logs, the same state."""
    rig = rigs("barc")
    whole = device_rollout(rig, rig.sc["x0"], 64)
    halves = device_rollout(rig, rig.sc["x0"], 64, chunks=2)
    for k in VC.ROLLOUT_KEYS + ("flags",):
        assert np.array_equal(whole[k], halves[k]), k
    assert all(np.array_equal(whole["pid"][k], halves["pid"][k]) for k in VC.PID_KEYS)
    s, sc = rig.solver, rig.sc
    s.vanilla_create(sc["cfg"], VC.B_TEST)
    x = dev(s, sc["x0"])
    out = s.vanilla_rollout(rig.spline, rig.table, x, 64, sc["dt_sim"], sc["n_sub"], speed_scale=sc["speed_scale"], out={})
    s.synchronize()
    assert out == {} and np.array_equal(host(x), whole["x"])


def test_run_vanilla_fused_against_unfused(pkg, rigs):
    """closed_loop.run_vanilla: one launch per chunk against one solve and one plant step per period.  The plant is compiled into two
    translation units and nothing guarantees the same contraction in both (lmpc_loop_advance_batch documents 1 - 2 ulp for the same
    reason), so the runs are compared at the rollout's tolerance; the first decision, taken at the same state, is bit for bit.
    (Measured: 0 -- the out-of-line plant of lmpc_vanilla_kernel.hip meets lmpc_plant_kernel's bits with this compiler.)"""
    rig = rigs("barc")
    s, sc = rig.solver, rig.sc
    runs = {}
    for fused in (True, False):
        s.vanilla_create(sc["cfg"], VC.B_TEST)
        r = pkg.closed_loop.run_vanilla(s, rig.table, rig.spline, dev(s, sc["x0"]), 64, dt=sc["dt"], n_sub=sc["n_sub"], speed_scale=sc["speed_scale"],
                                        chunk=24, fused=fused)
        s.synchronize()
        runs[fused] = {k: host(r[k]) for k in ("x", "X_log", "U_log", "k_log", "distance", "worst_excess", "flags", "n_fail")}
        runs[fused]["pid"] = pid_of(s, VC.B_TEST)
    f, u = runs[True], runs[False]
    assert not f["flags"].any() and not u["flags"].any() and not f["n_fail"].any()
    assert np.array_equal(f["U_log"][:, :, 0], u["U_log"][:, :, 0]) and np.array_equal(f["k_log"][:, 0], u["k_log"][:, 0])
    worst = {k: VC.err(f[k], u[k]) for k in VC.ROLLOUT_KEYS}
    print({k: "%.1e" % v for k, v in worst.items()})
    assert max(worst.values()) <= VC.TOL_ROLLOUT, worst
    ref = VC.reference("barc", "rollout", 64)
    for k in ("x", "X_log", "U_log", "k_log", "distance"):
        assert VC.err(f[k], ref[k]) <= VC.TOL_ROLLOUT, k
    assert VC.err(f["worst_excess"], np.maximum(ref["worst_excess"], 0.0)) <= VC.TOL_ROLLOUT   # (run_vanilla keeps it from 0, as run does)


def test_long_run_fills_the_fleet_safe_set(pkg, rigs):
    """700 periods of the BARC scenario in chunks of 64 with fleet_record=True: every car closes at least one full lap into its ring,
    and the ring's laps are np.array_equal to what the unfused path (one solve, one plant step, one record per period, on a solver of
    its own) records.  This needs the fused kernel's plant to have lmpc_plant_kernel's bits for 47 000 car-steps: it had not while
    the plant was inlined into the period loop (a quarter of the cars an ulp off after one period), and has since the plant is an
    out-of-line function in the form of the plant kernel's body (csrc/lmpc_vanilla_kernel.hip, vanilla_plant)."""
    rig = rigs("barc")
    sc = rig.sc
    other = Rig(pkg, sc)
    laps = {}
    for fused, r in ((True, rig), (False, other)):
        s = r.solver
        s.vanilla_create(sc["cfg"], VC.B_TEST)
        s.fleet_ss_create(VC.B_TEST, 1024)
        res = pkg.closed_loop.run_vanilla(s, r.table, r.spline, dev(s, sc["x0"]), 700, dt=sc["dt"], n_sub=sc["n_sub"], speed_scale=sc["speed_scale"],
                                          chunk=64, fused=fused, fleet_record=True)
        s.synchronize()
        assert not res["flags"].cpu().numpy().any()
        assert (res["worst_excess"].cpu().numpy() <= 0.0).all()
        stats = s.fleet_ss_stats(VC.B_TEST)
        assert (stats["laps_in_ring"].cpu().numpy() >= 1).all(), stats["laps_in_ring"].cpu().numpy().min()
        laps[fused] = [s.fleet_ss_get_laps(b) for b in range(VC.B_TEST)]
        s.fleet_ss_destroy()
    for b in range(VC.B_TEST):
        assert len(laps[True][b]) == len(laps[False][b]) >= 1, b
        for lf, lu in zip(laps[True][b], laps[False][b]):
            for a, c in zip(lf, lu):
                assert np.array_equal(a, c), b


# ---- poison ----
def test_one_cars_nan_stays_its_own(pkg, rigs):
    """A NaN start, a 1e300 abscissa and a NaN vel_ref, planted in a batch of 67: those cars are flagged, their PID state is left as
    it was, the call succeeds, and every other car has the clean batch's bits."""
    rig = rigs("barc")
    sc = rig.sc
    integral = np.full(VC.B_TEST, 0.25)
    clean = device_decide(rig, sc["x0"], sc["vel_ref"], integral=integral)
    x, vr = sc["x0"].copy(), sc["vel_ref"].copy()
    x[5, 1], x[40, 0], vr[66] = np.nan, 1e300, np.nan
    got = device_decide(rig, x, vr, integral=integral)
    planted = np.zeros(VC.B_TEST, dtype=bool)
    planted[[5, 40, 66]] = True
    assert (got["flags"][planted] == pkg.VANILLA_NOT_FINITE).all() and not got["flags"][~planted].any()
    assert not np.isfinite(got["u_out"][planted]).all(axis=1).any()
    for k in ("u_out", "u_model"):
        assert np.array_equal(got[k][~planted], clean[k][~planted]), k
    for k in VC.PID_KEYS:
        assert np.array_equal(got["pid"][k][~planted], clean["pid"][k][~planted]), k
        assert (got["pid"][k][planted] == (0.25 if k == "integral" else 0.0)).all(), k


def test_rollout_freezes_a_poisoned_car(pkg, rigs):
    """The rollout has no vel_ref: its third poisoned car has a NaN yaw rate, which the decision does not read and the plant does.
    All three are flagged and frozen -- state and PID state as they were, logs NaN, nothing accumulated -- and every other car has the
    clean batch's bits."""
    rig = rigs("barc")
    sc = rig.sc
    clean = device_rollout(rig, sc["x0"], 8)
    x0 = sc["x0"].copy()
    x0[5, 1], x0[40, 0], x0[66, 5] = np.nan, 1e300, np.nan
    got = device_rollout(rig, x0, 8)
    planted = np.zeros(VC.B_TEST, dtype=bool)
    planted[[5, 40, 66]] = True
    assert (got["flags"][planted] == pkg.VANILLA_NOT_FINITE).all() and not got["flags"][~planted].any()
    for k in ("X_log", "U_log", "k_log"):
        assert np.isnan(got[k][planted]).all(), k
    assert np.array_equal(got["x"][planted], x0[planted], equal_nan=True)
    assert (got["distance"][planted] == 0).all() and (got["worst_excess"][planted] == -np.inf).all()
    for k in VC.PID_KEYS:
        assert (got["pid"][k][planted] == 0).all(), k
        assert np.array_equal(got["pid"][k][~planted], clean["pid"][k][~planted]), k
    for k in VC.ROLLOUT_KEYS:
        assert np.array_equal(got[k][~planted], clean[k][~planted]), k
    check_rollout({k: (v[~planted] if k != "pid" else {n: a[~planted] for n, a in v.items()}) for k, v in got.items()},
                  {k: (v[~planted] if k != "pid" else {n: a[~planted] for n, a in v.items()}) for k, v in VC.reference("barc", "rollout", 8).items()})


# ---- arguments ----
def test_argument_errors(pkg, rigs):
    import torch
    rig = rigs("barc")
    s, sc = rig.solver, rig.sc
    cfg = sc["cfg"]
    bad = pytest.raises(pkg.LmpcError, match="-> -1")
    for wrong in (dict(cfg, dt=0.0), dict(cfg, dt=-0.1), dict(cfg, dt=float("nan")), dict(cfg, dt=float("inf")),
                  dict(cfg, min_lookahead_distance=0.0), dict(cfg, min_lookahead_distance=-1.0), dict(cfg, min_lookahead_distance=11.0),
                  dict(cfg, min_i=1.0, max_i=0.5), dict(cfg, min_cmd=1.0, max_cmd=0.5)):
        with bad:
            s.vanilla_create(wrong, 4)
    with bad:
        s.vanilla_create(cfg, 0)
    s.vanilla_destroy()
    x = dev(s, sc["x0"][:4])
    kw = dict(dtype=torch.float64, device=s.device)
    sentinel = lambda *shape: torch.full(shape, -7.0, **kw)   # noqa: E731
    with bad:
        s.vanilla_solve(rig.spline, x)                              # no store
    with bad:
        s.vanilla_rollout(rig.spline, rig.table, x, 1, 0.01, 1)
    with bad:
        s.vanilla_get(4)
    with bad:
        s.vanilla_reset(4)
    s.vanilla_create(cfg, 4)
    five = dev(s, sc["x0"][:5])
    out = {"u_out": sentinel(3, 5), "u_model": sentinel(2, 5)}
    with bad:
        s.vanilla_solve(rig.spline, five, out=out)                   # another batch than the store's
    with bad:
        s.vanilla_rollout(rig.spline, rig.table, five, 1, 0.01, 1)
    with bad:
        s.vanilla_get(5)
    with bad:
        s.vanilla_reset(5)
    out4 = {"u_out": sentinel(3, 4), "u_model": sentinel(2, 4)}
    with bad:
        s.vanilla_solve(None, x, out=out4)                           # null track
    with bad:
        s.vanilla_solve(rig.spline, x, out={"u_out": None, "u_model": out4["u_model"]})   # null required pointer
    x_before = x.clone()
    logs = {"X_log": sentinel(6, 2, 4), "U_log": sentinel(2, 2, 4), "k_log": sentinel(2, 4), "flags": torch.full((4,), -7, dtype=torch.int32, device=s.device)}
    for args in ((0, 0.01, 1), (-1, 0.01, 1), (2, 0.01, 0), (2, 0.0, 1), (2, -0.01, 1), (2, float("nan"), 1), (2, float("inf"), 1)):
        with bad:
            s.vanilla_rollout(rig.spline, rig.table, x, args[0], args[1], args[2], out=logs)
    with bad:
        s.vanilla_rollout(None, rig.table, x, 2, 0.01, 1, out=logs)
    s.synchronize()
    # nothing was written: outputs, state and PID state
    assert all((t == -7).all().item() for t in list(out.values()) + list(out4.values()) + list(logs.values()))
    assert torch.equal(x, x_before)
    p = pid_of(s, 4)
    assert all((p[k] == 0).all() for k in VC.PID_KEYS)
    assert "lmpc_vanilla" in s.lib.lmpc_last_error(s._h).decode()
    s.vanilla_rollout(rig.spline, rig.table, x, 2, 0.01, 1, out=logs)   # the same call with a track: accepted
    s.vanilla_destroy()
    s.vanilla_destroy()                                              # nothing to destroy: LMPC_OK


# ---- the C++ class ----
def test_cpp_class_driver(rigs, tmp_path, golden):
    """VanillaController (host/vanilla_controller.hpp), one car, 64 decisions on tests/golden/vanilla_one_car.npz with the PID state
    carried: the C ABI's bits at B = 1, the fixture's numbers."""
    exe = LIB / "test_vanilla_controller"
    assert exe.exists(), "run __graft_entry__.build() first"
    g = golden("vanilla_one_car")
    rig = rigs("barc")
    s = rig.solver
    cfg = dict(zip((str(n) for n in g["cfg_names"]), (float(v) for v in g["cfg_values"])))
    order = ("lookahead_speed_ratio", "min_lookahead_distance", "max_lookahead_distance", "k_p", "k_i", "k_d", "min_cmd", "max_cmd", "min_i",
             "max_i", "dt", "force_to_lon")
    P = g["vel_ref"].shape[0]
    fmt = lambda a: " ".join(repr(float(v)) for v in np.asarray(a).reshape(-1))   # noqa: E731
    case, out = tmp_path / "case.txt", tmp_path / "out.txt"
    case.write_text("\n".join([fmt([cfg[k] for k in order]), str(P)] + [fmt(list(g["X_log"][:, p]) + [g["vel_ref"][p]]) for p in range(P)]) + "\n")
    r = subprocess.run([str(exe), str(VC.TC.BARC), str(case), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), (r.stdout[-2000:], r.stderr[-2000:])
    rows = np.array([[float(v) for v in ln.split()] for ln in out.read_text().splitlines()])
    assert rows.shape == (P, 9) and not rows[:, 5].any()
    # the same sequence through the C ABI at B = 1, on the splines the C++ track class exports (its banded solve and numpy's dense one
    # round the polynomials differently: tests/test_track_spline.py), so that the two sides evaluate the same numbers
    host_dir = ROOT / "racing-lmpc-ros2_amd" / "host"
    export = tmp_path / "test_spline_export"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{host_dir}", "-o", str(export), str(ROOT / "tests" / "cpp" / "test_spline_export.cpp"),
                    str(host_dir / "racing_trajectory.cpp")], check=True, timeout=300)
    lines = subprocess.run([str(export), str(VC.TC.BARC)], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    head = lines[0].split()
    arr = [np.array([float(v) for v in ln.split()]) for ln in lines[1:6]]
    cpp_track = s.spline_track({"L": float(head[0]), "breaks": arr[0], "coef": arr[1].reshape(5, int(head[2]), 4), "wp_x": arr[2], "wp_y": arr[3],
                                "wp_s": arr[4]})
    s.vanilla_create(cfg, 1)
    abi = np.empty((P, 8))
    for p in range(P):
        o = s.vanilla_solve(cpp_track, dev(s, g["X_log"][None, :, p]), dev(s, g["vel_ref"][p:p + 1]))
        pid = pid_of(s, 1)
        abi[p] = np.concatenate([host(o["u_out"])[0], host(o["u_model"])[0], [pid[k][0] for k in VC.PID_KEYS]])
    assert np.array_equal(rows[:, :5], abi[:, :5]) and np.array_equal(rows[:, 6:], abi[:, 5:])
    assert VC.err(rows[:, :3], g["u_out"]) <= VC.TOL and VC.err(rows[:, 3:5], g["U_log"].T) <= VC.TOL
    assert VC.err(rows[-1, 6:], g["pid"]) <= VC.TOL
