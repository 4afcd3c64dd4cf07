"""GPU: every consumer of T_ref on a time step that differs per stage and per problem (tests/timestep_cases.py; every other input set
of the suite has T_ref == 0.025 everywhere).  The arbiter is the dense, KKT-certified optimum of tests/golden/dense_dt_*.npz, not the
serial twin; tests/test_timestep_fixtures.py shows on the CPU that the comparison used here refuses the optimum of the problem with
T_ref read one stage off, on every problem of every case.

Which case reaches which reader of T_ref (csrc/lmpc_capi.hip `kernel_table` / `choose_kernel`, csrc/lmpc_solve_setup.hip.h):
  full records (ST_DT)   fp64 up to N = 40 -- dt_trk_n3 / n12 / n20 / n24, dt_iac_n40, dt_lrn_n20 / n40 -- and every float kernel
  lean records (LN_DT)   fp64 from N = 41 on: the two-wave kernels the library picks for tracking (dt_trk_n41 / n65 / n81, dt_iac_n66),
                         the one-wave kernels with one wave forced on the same cases, under the warm start, and under the learning
                         problem (dt_lrn_n41_s160)
  the loader's tail loop a stage index past the loading threads: 64 threads and NS > 64, i.e. the ONE-wave kernels from N = 66 on
                         (one wave forced on dt_trk_n81 and dt_iac_n66; the float kernels on dt_iac_n66).  The two-wave kernels load
                         with 128 threads and never run it; at N = 65 (NS = 64) every thread owns exactly one stage
  two waves at N = 24    lmpc_set_waves_per_problem(2) accepts the horizon (the W2(7) row): dt_trk_n24 with two waves forced."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import timestep_cases as TC
import timestep_check as K
from oracle import dynamics as D, params as P, qp as Q, scenario as S
from tolerances import TOL_F32_SWEEP, TOL_LINEARIZE_REL, TOL_XU

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "racing-lmpc-ros2_amd" / "lib"
LEARNING = [n for n in TC.CASES if TC.CASES[n][0] == "spc"]
LEAN_TRACKING = ["dt_trk_n41", "dt_trk_n65", "dt_trk_n81", "dt_iac_n66"]
# Reduced precision: a problem that misses TOL_F32_SWEEP with status OPTIMAL while fp64 is right is the known tail of the reduced-
# precision entries (tests/tolerances.py), not a time-step defect; it is NAMED here, at most one per (entry, case), and printed.
# lmpc_solve_batch_f32 on dt_trk_n20, problem 21: X/U 3.0e-3, dU 1.6e-2 from the dense optimum, status OPTIMAL; fp64 8e-13 and mixed 1.2e-6 on
# the same problem, the other 31 problems of the case within 2e-3 (a stage read one off moves every problem of this case by 0.6 or
# more).  include/lmpc_hip.h: the single-precision entry is "NOT for the BARC tracking problem at low speed".
NAMED_REDUCED_PRECISION_TAIL: dict = {("f32", "dt_trk_n20"): (21,)}


# ---- linearisation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", ["rk4", "euler"])
@pytest.mark.parametrize("N", [3, 20, 41])
def test_linearize_matches_complex_step_on_nonuniform_steps(pkg, N, integrator):
    """lmpc_linearize_batch against the complex-step Jacobian of the oracle's integrator with dt = T_ref[i][b]; 300 problems (a second,
    partly filled 256-thread block).  TOL_LINEARIZE_REL as test_linearize_matches_complex_step applies it, and stage by stage: the error
    of stage i against max |A_i| (|B_i|, |g_i|) of that stage, so that a wrong step on one short stage -- B_i and g_i scale with t_i
    -- is not measured against the longest one."""
    import dataclasses

    B = 300
    veh, cfg = dataclasses.replace(P.barc_vehicle(), integrator=integrator), P.barc_tracking_mpc(N)
    sv = pkg.Solver(pkg.presets.barc_tracking_mpc(N), dict(pkg.presets.barc_vehicle(), integrator=integrator), device=0)
    tr = pkg.workloads.synthetic_track("barc")
    u_lo, u_hi, _, _ = Q.effective_bounds(cfg, veh)
    x, u = pkg.workloads.sample_initial_states("barc", B, tr["L"], u_lo, u_hi, 11)
    inp = S.cold_start_inputs(cfg, veh, tr, x, u, 0.025)
    inp["T_ref"] = TC.draw_t_ref(N, B, 9400 + N)
    rng = np.random.default_rng(5)
    inp["U_ref"] = inp["U_ref"] + rng.normal(0, 1.0, inp["U_ref"].shape) * np.array([0.004, 0.1])[:, None, None]
    A, Bm, g = (t.cpu().numpy() for t in sv.linearize(inp))
    sv.close()
    Ar, Br, gr = D.rk4_jacobian_cs(inp["X_ref"][:, :N - 1].transpose(1, 2, 0), inp["U_ref"].transpose(1, 2, 0), inp["curvatures"][:N - 1], inp["T_ref"], veh)
    eA, eB, eg = np.abs(A.transpose(2, 3, 0, 1) - Ar), np.abs(Bm.transpose(2, 3, 0, 1) - Br), np.abs(g.transpose(1, 2, 0) - gr)
    print("N = %d %s: A %.1e B %.1e g %.1e (relative to the largest entry)" % (N, integrator, eA.max() / np.abs(Ar).max(), eB.max() / np.abs(Br).max(), eg.max() / max(1.0, np.abs(gr).max())))
    assert eA.max() <= TOL_LINEARIZE_REL * np.abs(Ar).max()
    assert eB.max() <= TOL_LINEARIZE_REL * np.abs(Br).max()
    assert eg.max() <= 10 * TOL_LINEARIZE_REL * max(1.0, np.abs(gr).max())
    for i in range(N - 1):
        assert eA[i].max() <= TOL_LINEARIZE_REL * np.abs(Ar[i]).max(), i
        assert eB[i].max() <= TOL_LINEARIZE_REL * np.abs(Br[i]).max(), i
        assert eg[i].max() <= 10 * TOL_LINEARIZE_REL * max(1.0, np.abs(gr[i]).max()), i
    # and per problem: a stage's largest entry belongs to its slowest car and hides an error in a fast one (tests/envelope_cases.py)
    import envelope_cases as E
    E.held_per_problem("N = %d %s" % (N, integrator), (A, Bm, g), inp, veh)


# ---- fp64, every case --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.CASES))
def test_fp64_solve_against_the_dense_fixture_in_both_layouts(pkg, name):
    """lmpc_solve_batch: X, U, dU (and the simplex weights) of every problem within TOL_XU / TOL_DU of the dense optimum, status 0;
    dU_optm t_i equal to the differences of U_optm and u_ic to 1e-12 (scaled) on the kernel's own outputs -- the division of the
    result write-out, pinned separately from the optimum; the AOS layout holds the same bits."""
    rec = K.check_fp64(pkg, name)
    N = TC.CASES[name][1]
    assert rec["threads"] == (128 if (N >= 41 and name not in LEARNING) else 64), rec      # the kernel the module text says this case reaches


def test_fp64_solve_in_the_debug_hook_build():
    """The same check of every case in liblmpc_hip_dbg.so (a second register allocation of every kernel), in a process of its own so
    that LMPC_HIP_LIBRARY selects the build, as tests/test_gpu_dispatch.py does."""
    lib = LIB / "liblmpc_hip_dbg.so"
    assert lib.exists(), "%s not built: __graft_entry__.build()" % lib.name
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "timestep_check.py")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, LMPC_HIP_LIBRARY=str(lib)))
    lines = r.stdout.strip().splitlines()
    assert lines and lines[-1].startswith("{"), (r.stdout[-2000:], r.stderr[-3000:])
    s = json.loads(lines[-1])
    print("\n".join(lines[:-1]))
    assert r.returncode == 0 and not s["failures"], (s["failures"], r.stderr[-2000:])
    assert s["library"] == lib.name and s["cases"] == len(TC.CASES)


# ---- the other fp64 entries on the same inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.CASES))
def test_warm_start_from_the_optimum_returns_the_optimum(pkg, name):
    """lmpc_solve_batch_warm (tracking) / lmpc_solve_batch_warm_ss on the arrays (learning), the plan the fixture's optimum shifted by
    zero stages.  The answers are held to the fixture like a cold solve's.  The plan's active set is the optimum's, so the active-set
    attempt -- the warm kernel's own reading of T_ref -- is what answers wherever the library has a warm kernel; at least half of the
    case must have taken that route (lmpc_get_warm_accepted) for the comparison to be about it and not about the cold fallback."""
    c = K.case(pkg, name)
    o = K.solve(pkg, name, "warm")
    print("%s: warm attempt accepted on %d of %d, iterations mean %.2f" % (name, int(o["accepted"].sum()), o["accepted"].size, o["iters"].mean()))
    TC.assert_matches(o, c["fx"], "%s, warm start" % name)
    assert TC.rate_identity_error(o, c["inp"]) < K.RATE_IDENTITY_TOL
    assert o["accepted"].mean() >= 0.5, (name, o["accepted"])          # (every case has a warm kernel: tracking any N, learning N <= 60)


@pytest.mark.parametrize("name", LEARNING)
def test_safe_set_by_reference_cold_and_warm(pkg, name):
    """lmpc_solve_batch_ss_idx and lmpc_solve_batch_warm_ss with ss_idx: the spec laps stored on the handle, the codes from
    lmpc_ss_query_idx_batch; same fixtures, same tolerances."""
    c = K.case(pkg, name)
    for entry in ("ss_idx", "warm_idx"):
        o = K.solve(pkg, name, entry)
        TC.assert_matches(o, c["fx"], "%s, %s" % (name, entry))
        assert TC.rate_identity_error(o, c["inp"]) < K.RATE_IDENTITY_TOL


@pytest.mark.parametrize("name", LEAN_TRACKING)
def test_one_wave_forced_on_the_lean_horizons(pkg, name):
    """lmpc_set_waves_per_problem(1) from N = 41 on: the one-wave kernel on lean records, which the library itself only picks for the
    learning problem and the warm start; at N = 66 and 81 its 64 loading threads leave stages 64 .. NS - 1 to the loader's tail loop."""
    c = K.case(pkg, name)
    o = K.solve(pkg, name, waves=1)
    assert o["threads"] == 64
    TC.assert_matches(o, c["fx"], "%s, one wave forced" % name)
    assert TC.rate_identity_error(o, c["inp"]) < K.RATE_IDENTITY_TOL


def test_two_waves_forced_at_n24(pkg):
    """lmpc_set_waves_per_problem(2) takes N = 24 (the shortest horizon with a two-wave kernel): full records behind the 128-thread loader."""
    c = K.case(pkg, "dt_trk_n24")
    o = K.solve(pkg, "dt_trk_n24", waves=2)
    assert o["threads"] == 128
    TC.assert_matches(o, c["fx"], "dt_trk_n24, two waves forced")
    assert TC.rate_identity_error(o, c["inp"]) < K.RATE_IDENTITY_TOL


@pytest.mark.parametrize("name", ["dt_trk_n20", "dt_trk_n65"])
def test_host_entries_on_single_problems(pkg, name):
    """lmpc_solve_host (column-major host arrays, T_ref repacked by the library) on problems 0 and 1: bit for bit the batch call's
    columns, as test_aos_layout_does_not_reach_the_solves_the_library_runs_for_itself asserts on uniform steps, and therefore within
    TOL_XU of the fixture; lmpc_solve_host_warm from the fixture's optimum: within TOL_XU / TOL_DU of the fixture."""
    c = K.case(pkg, name)
    fx, inp, N = c["fx"], c["inp"], TC.CASES[name][1]
    batch = K.solve(pkg, name)
    sv = pkg.Solver(*TC.presets(pkg, name), device=0)
    lib, h = pkg.load_library(), sv._h
    col = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64))  # noqa: E731
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        for b in (0, 1):
            hx = [col(inp["x_ic"][:, b]), col(inp["u_ic"][:, b]), col(inp["X_ref"][:, :, b].T), col(inp["U_ref"][:, :, b].T), col(inp["T_ref"][:, b]),
                  col(inp["bound_left"][:, b]), col(inp["bound_right"][:, b]), col(inp["curvatures"][:, b]), col(inp["vel_ref"][:, b])]
            one = {k: fx[k][..., b:b + 1] for k in ("X_optm", "U_optm", "dU_optm")}
            X, U, dU = np.zeros((N, 6)), np.zeros((N - 1, 2)), np.zeros((N - 1, 2))
            st, it = C.c_int32(-1), C.c_int32(-1)
            rc = lib.lmpc_solve_host(h, *[p(a) for a in hx], C.c_double(float(inp["L"])), None, None, p(X), p(U), p(dU), None, C.byref(st), C.byref(it))
            assert rc == 0 and st.value == 0
            assert np.array_equal(X.T, batch["X_optm"][:, :, b]) and np.array_equal(U.T, batch["U_optm"][:, :, b]) and np.array_equal(dU.T, batch["dU_optm"][:, :, b]), (name, b)
            TC.assert_matches({"X_optm": X.T[..., None], "U_optm": U.T[..., None], "dU_optm": dU.T[..., None], "status": np.array([st.value])}, one,
                              "%s problem %d, lmpc_solve_host" % (name, b))
            Xw, Uw = col(fx["X_optm"][:, :, b].T), col(fx["U_optm"][:, :, b].T)
            X, U, dU = np.zeros((N, 6)), np.zeros((N - 1, 2)), np.zeros((N - 1, 2))
            st, it = C.c_int32(-1), C.c_int32(-1)
            rc = lib.lmpc_solve_host_warm(h, *[p(a) for a in hx], C.c_double(float(inp["L"])), p(Xw), p(Uw), p(X), p(U), p(dU), C.byref(st), C.byref(it))
            assert rc == 0
            TC.assert_matches({"X_optm": X.T[..., None], "U_optm": U.T[..., None], "dU_optm": dU.T[..., None], "status": np.array([st.value])}, one,
                              "%s problem %d, lmpc_solve_host_warm (%d iterations)" % (name, b, it.value))
    finally:
        sv.close()


# ---- reduced precision ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,name", [("f32", "dt_iac_n40"), ("f32", "dt_trk_n20"), ("f32", "dt_iac_n66"),
                                        ("mixed", "dt_iac_n40"), ("mixed", "dt_trk_n20"), ("mixed", "dt_lrn_n20_s160"), ("mixed", "dt_iac_n66")])
def test_reduced_precision_against_the_dense_fixture(pkg, entry, name):
    """lmpc_solve_batch_f32 / lmpc_solve_batch_mixed against the dense optimum at TOL_F32_SWEEP, the project's stated tolerance away
    from the BASELINE draws (dU: TOL_F32_SWEEP / 0.025, as tests/dispatch_sweep.py applies it); a slipped stage is three decades above."""
    c = K.case(pkg, name)
    o = K.solve(pkg, name, entry)
    assert o["precision"] == entry
    allow = NAMED_REDUCED_PRECISION_TAIL.get((entry, name), ())
    assert len(allow) <= 1
    TC.assert_matches(o, c["fx"], "%s, %s" % (name, entry), TOL_F32_SWEEP, TOL_F32_SWEEP / 0.025, allow=allow)


# ---- per-problem independence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dt_trk_n20", "dt_trk_n65", "dt_lrn_n20_s160"])
def test_batch_order_reversed_gives_the_same_bits(pkg, name):
    """The batch reversed, inputs, safe sets and T_ref together: the results reversed back are bit for bit the first run's.  T_ref is
    drawn per problem, so a step read from a neighbour's column changes the answer of that problem."""
    B = TC.CASES[name][2]
    a, b = K.solve(pkg, name), K.solve(pkg, name, order=np.arange(B)[::-1])
    for k in ("X_optm", "U_optm", "dU_optm", "convex_combi_optm", "status", "iters"):
        if k in a:
            assert np.array_equal(a[k], b[k][..., ::-1]), (name, k)


# ---- facade ------------------------------------------------------------------------------------------------------------------------------------
def _dm(f, a):
    a = np.atleast_2d(np.asarray(a, dtype=np.float64))
    f.write(f"{a.shape[0]} {a.shape[1]}\n")
    f.write(" ".join(repr(float(v)) for v in a.T.reshape(-1)) + "\n")  # column-major


@pytest.mark.parametrize("b", [0, 1])
def test_facade_takes_the_time_step_vector_of_each_call(pkg, tmp_path, b):
    """tests/cpp/test_facade_timestep.cpp: RacingMPC::solve with a non-uniform T_ref, then with the first plan as the warm start and
    ANOTHER non-uniform T_optm_ref (the column rolled by one stage), each against lmpc_solve_batch on the same arrays -- which in turn
    is within TOL_XU of the fixture's optimum and of its rolled optimum."""
    name = "dt_trk_n20"
    exe = LIB / "test_facade_timestep"
    assert exe.exists(), "run __graft_entry__.build() first"
    c = K.case(pkg, name)
    fx, inp = c["fx"], c["inp"]
    first = K.solve(pkg, name)
    sv = pkg.Solver(*TC.presets(pkg, name), device=0)
    second = {k: v.cpu().numpy() for k, v in sv.solve(TC.rolled(inp)).items() if hasattr(v, "cpu")}
    sv.close()
    TC.assert_matches(second, {k: fx[k + "_rolled"] for k in ("X_optm", "U_optm", "dU_optm")}, "%s with T_ref rolled, lmpc_solve_batch" % name)
    path = tmp_path / "problem.txt"
    with open(path, "w") as f:
        f.write("20 %r %r\n" % (float(inp["L"]), TOL_XU))
        _dm(f, inp["x_ic"][:, b:b + 1])
        _dm(f, inp["u_ic"][:, b:b + 1])
        _dm(f, inp["X_ref"][:, :, b])
        _dm(f, inp["U_ref"][:, :, b])
        for k in ("T_ref", "bound_left", "bound_right", "curvatures", "vel_ref"):
            _dm(f, inp[k][:, b][None, :])
        _dm(f, np.roll(inp["T_ref"][:, b], 1)[None, :])
        for o in (first, second):
            for k in ("X_optm", "U_optm", "dU_optm"):
                _dm(f, o[k][:, :, b])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    print(r.stdout.strip())
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), (r.stdout, r.stderr)
