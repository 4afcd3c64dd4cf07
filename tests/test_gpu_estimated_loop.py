"""lmpc_loop_advance_estimated_batch (include/lmpc_hip_estimated.h): everything between two solves of the ESTIMATED closed loop in one
launch.  It must be the composition of the entry points it replaces, in closed_loop.run_estimated's order -- held here stage by stage,
each unfused stage run on the fused call's own recorded intermediate so that no tolerance has to absorb an upstream difference --
over consecutive calls, against the numpy filter on a whole run, on its refusals and optional pointers, and loop against loop.

Shapes: the BARC track and vehicle, N = 20 and N = 3, B = one workgroup of the kernel plus one lane (65) and B = 1, start vx in
[1.5, 2.5] (tests/estimated_cases.py; tests/test_estimated_reference.py is the scenario's gate without a GPU).
Tolerances: bit for bit wherever the text is shared and contraction is off or the code is out of line; the filter, inlined into another
kernel, at ekf_cases.TOL; the last knot of a shifted solution at the project's rtol = 1e-14, atol = 1e-15, the exception
tests/test_gpu_loop.py has.  Needs an MI355X."""
import ctypes as C
import math

import numpy as np
import pytest

import ekf_cases as EC
import estimated_cases as XC
import stream_cases as SC
import track_cases as TC
from oracle import params as OP

pytestmark = pytest.mark.gpu
KEYS = XC.REF_KEYS
DT, DT_NS = XC.DT, XC.DT_NS
OPTIONAL = ("x_est", "z_vel", "z_pose", "ekf_flags", "track_status", "distance", "worst_excess", "n_fail", "sq_err")


@pytest.fixture(scope="module")
def world(pkg):
    """Per horizon N: two solvers (the fused call's handle and the handle of the unfused chain with its own filter), each with the
    BARC spline track and tables."""
    import torch  # noqa: F401
    tr = pkg.racing_trajectory.RacingTrajectory(TC.BARC)
    tab = tr.to_track_table(1024)
    made = {}

    def get(N):
        if N not in made:
            pair = []
            for _ in range(2):
                sv = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
                pair.append(dict(sv=sv, spline=sv.spline_track(tr), trk=sv.device_track(tab)))
            made[N] = pair
        return made[N]

    yield dict(get=get, tr=tr, tab=tab, L=float(tab["L"]))
    for pair in made.values():
        for w in pair:
            w["spline"].close()
            w["sv"].close()


def _dev(a, dtype=None):
    return SC.dev(a, dtype)


def _filter(w, est0, P0, rows_vel=EC.ROWS_VEL, rows_pose=EC.ROWS_POSE):
    """The handle's filter made anew: ekf_cases' config, the two observations, a start per car, the clock at 0.  -> (obs_vel, obs_pose)"""
    cfg = EC.config()
    sv = w["sv"]
    sv.ekf_create(est0.shape[1], cfg["x0"], cfg["P0"], cfg["Q"], cfg["x_min"], cfg["x_max"])
    ids = sv.ekf_register_observation(rows_vel), sv.ekf_register_observation(rows_pose)
    sv.ekf_set_state(est0, P0)
    sv.ekf_initialize(0)
    return ids


def _scene(world, N, B, seed=5, rows_vel=EC.ROWS_VEL, rows_pose=EC.ROWS_POSE, solve=True):
    """One period's inputs on the device: the scenario's truth and filter start, x_ic the start's projection, the cold start's plan
    at x_ic and -- N = 20 -- a real solve from it, every seventh car declared failed.  N = 3: the plan with seeded noise on it as the
    solution (tests/test_gpu_glue.py's way for short horizons)."""
    import torch
    A, Bh = world["get"](N)
    sv = A["sv"]
    sc = XC.scenario(world["L"], B, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    d = {"x": _dev(sc["x"]), "u_prev": _dev(sc["u_prev"]), "P0": _dev(sc["P0"])}
    pose = sv.frenet_to_global(A["spline"], d["x"])
    d["est0"] = (torch.cat([pose, d["x"][3:6]]) + _dev(sc["est_noise"])).contiguous()
    frenet, st = sv.global_to_frenet(A["spline"], d["est0"][0:3].contiguous())
    assert int(st.max()) == 0
    d["x_ic"] = torch.cat([frenet, d["est0"][3:6]]).contiguous()
    inp = sv.prepare(A["trk"], d["x_ic"].clone(), DT, speed_scale=XC.SPEED_SCALE)
    inp["u_ic"] = d["u_prev"]
    if solve:
        out = sv.solve(inp)
        sol = {"X_optm": torch.nan_to_num(out["X_optm"]).clone(), "U_optm": torch.nan_to_num(out["U_optm"]).clone(), "status": out["status"].clone()}
    else:
        sx, su = np.array([0.01, 0.005, 0.005, 0.02, 0.005, 0.02])[:, None, None], np.array([0.0005, 0.02])[:, None, None]
        sol = {"X_optm": inp["X_ref"] + _dev(sx * rng.normal(0, 1, (6, N, B))), "U_optm": _dev(su * rng.normal(0, 1, (2, N - 1, B))),
               "status": torch.zeros(B, dtype=torch.int32, device="cuda")}
    sol["status"][_dev(sc["failed"], torch.bool)] = 1
    d["inp"] = {k: inp[k].clone() for k in KEYS}
    d["sol"] = sol
    nz_v, nz_p = len(rows_vel), len(rows_pose)
    d["noise_vel"] = _dev(np.concatenate([sc["noise_vel"], 0.5 * sc["noise_vel"][:1]])[:nz_v])
    d["noise_pose"] = _dev(sc["noise_pose"][:nz_p])
    d["R_vel"] = _dev(np.moveaxis(EC.spd(rng, B, nz_v), 0, -1))
    d["R_pose"] = _dev(np.moveaxis(EC.spd(rng, B, nz_p, scale=0.02), 0, -1))
    d["sc"], d["rows"] = sc, (tuple(rows_vel), tuple(rows_pose))
    return d


def _buffers(d, optional=True):
    """Fresh copies of everything the call updates in place, and the optional arrays (accumulators at zero)."""
    import torch
    B = d["x"].shape[1]
    kw = dict(dtype=torch.float64, device="cuda")
    b = {"x": d["x"].clone(), "u_prev": d["u_prev"].clone(), "x_ic": d["x_ic"].clone(), "inp": {k: v.clone() for k, v in d["inp"].items()}}
    nz_v, nz_p = len(d["rows"][0]), len(d["rows"][1])
    b["opt"] = {k: None for k in OPTIONAL}
    if optional:
        b["opt"] = {"x_est": torch.full((6, B), -7.0, **kw), "z_vel": torch.full((nz_v, B), -7.0, **kw), "z_pose": torch.full((nz_p, B), -7.0, **kw),
                    "ekf_flags": torch.zeros(B, dtype=torch.int32, device="cuda"), "track_status": torch.zeros(B, dtype=torch.int32, device="cuda"),
                    "distance": torch.zeros(B, **kw), "worst_excess": torch.zeros(B, **kw), "n_fail": torch.zeros(B, dtype=torch.int64, device="cuda"),
                    "sq_err": torch.zeros((6, B), **kw)}
    return b


def _advance(w, d, b, ids, restart, t_vel=DT_NS // 2, t_pose=DT_NS, sol=None, **over):
    kw = dict(speed_scale=XC.SPEED_SCALE, restart_failed=restart, **b["opt"])
    kw.update(over)
    w["sv"].loop_advance_estimated(w["trk"], w["spline"], b["inp"], sol or d["sol"], b["x"], b["u_prev"], b["x_ic"], DT, DT / XC.N_SUB, XC.N_SUB,
                                   ids[0], ids[1], t_vel, t_pose, d["noise_vel"], d["R_vel"], d["noise_pose"], d["R_pose"], **kw)


def _bits(a, b):
    return SC.bits_equal(a, b)


def _store(w):
    g = w["sv"].ekf_get()
    return {k: g[k].cpu().numpy() for k in ("x", "P", "K")}, g["timestamp_ns"]


def _compose(world, N, B, restart, rows_vel=EC.ROWS_VEL, rows_pose=EC.ROWS_POSE, nan_seed=True):
    """One fused call against the unfused chain on the second handle, stage by stage.  Prints what was measured; asserts what the
    issue sets."""
    import torch
    A, U = world["get"](N)
    d = _scene(world, N, B, rows_vel=rows_vel, rows_pose=rows_pose, solve=N == 20)
    sol, inp, st = d["sol"], d["inp"], d["sol"]["status"]
    ok = st == 0
    if B > 1:
        assert 0 < int((~ok).sum()) < B
        if nan_seed:   # behind the solve: one car's seed of the projection is not finite -- the nearest waypoint starts it, in both chains
            d["x_ic"][0, 5] = math.nan
    ids = _filter(A, d["est0"], d["P0"], rows_vel, rows_pose)
    b = _buffers(d)
    _advance(A, d, b, ids, restart)
    torch.cuda.synchronize()
    o = b["opt"]
    sv2, trk2, sp2 = U["sv"], U["trk"], U["spline"]
    # 1 the input applied, the failures counted
    u_apply = torch.where(ok[None, :], sol["U_optm"][:, 0, :], inp["U_ref"][:, 0, :]).contiguous()
    assert torch.equal(b["u_prev"], u_apply) and torch.equal(o["n_fail"], (~ok).to(torch.int64))
    # 2 - 4 the truth against two plant_step calls, the velocity observation between them: bit for bit
    x_half = sv2.plant_step(trk2, d["x"].clone(), u_apply, DT / XC.N_SUB, XC.N_SUB // 2)
    z_vel_ref = (x_half[list(rows_vel)] + d["noise_vel"]).contiguous()
    x_ref = sv2.plant_step(trk2, x_half.clone(), u_apply, DT / XC.N_SUB, XC.N_SUB // 2)
    assert torch.equal(o["z_vel"], z_vel_ref)
    assert torch.equal(b["x"], x_ref), int((b["x"] != x_ref).sum())
    ds = x_ref[0] - d["x"][0]
    hb = float(sv2.vehicle["b"]) / 2
    exc_ref = torch.maximum(torch.zeros_like(ds), torch.maximum(x_ref[1] + hb - inp["bound_left"][0], inp["bound_right"][0] - (x_ref[1] - hb)))
    assert torch.equal(o["distance"], torch.where(ds < -world["L"] / 2, ds + world["L"], ds)) and torch.equal(o["worst_excess"], exc_ref)
    # 5 the pose observation: frenet_to_global of the fused truth, plus the noise, the yaw wrapped as run_estimated wraps it
    pose = sv2.frenet_to_global(sp2, b["x"])
    zp = pose[list(rows_pose)] + d["noise_pose"]
    for a, r in enumerate(rows_pose):
        if r == 2:
            zp[a] = torch.atan2(torch.sin(zp[a]), torch.cos(zp[a]))
    # (bit for bit where a number stands; a dropped-out car's NaN is a NaN in both, whatever its payload)
    assert torch.equal(torch.isnan(o["z_pose"]), torch.isnan(zp)) and torch.equal(o["z_pose"].nan_to_num(), zp.nan_to_num()), \
        float((o["z_pose"] - zp).abs().nan_to_num().max())
    if B > 1:   # the dropout is the NaN of noise_pose[0]
        assert 0 < int(torch.isnan(o["z_pose"][0]).sum()) < B and not bool(torch.isnan(o["z_pose"][1:]).any())
    # the filter: a second handle's, fed the fused (u, z_vel, z_pose, t) through lmpc_ekf_update_batch
    ids2 = _filter(U, d["est0"], d["P0"], rows_vel, rows_pose)
    sv2.ekf_update_control(b["u_prev"])
    _, _, _, f1 = sv2.ekf_update(ids2[0], o["z_vel"], d["R_vel"], DT_NS // 2)
    xe, _, _, f2 = sv2.ekf_update(ids2[1], o["z_pose"], d["R_pose"], DT_NS)
    (ga, ta), (gu, tu) = _store(A), _store(U)
    worst = {k: float(np.abs(ga[k] - gu[k]).max()) for k in ga}
    worst["x_est"] = float((o["x_est"] - xe).abs().max())
    assert ta == tu == DT_NS
    assert torch.equal(o["ekf_flags"], f1 | f2) and not bool((o["ekf_flags"] & EC.NOT_FINITE).any())
    assert torch.equal(o["x_est"], _dev(ga["x"]))
    # 6 the squared error (contraction off in the kernel; torch's atan2 / sin / cos are not the kernel's calls: a few ulp on the yaw row)
    err = o["x_est"] - torch.cat([pose, b["x"][3:6]])
    err[2] = torch.atan2(torch.sin(err[2]), torch.cos(err[2]))
    assert torch.allclose(o["sq_err"], err ** 2, rtol=1e-13, atol=0.0)
    # 7 the projection of the fused estimate, seeded with the old x_ic[0]: bit for bit, status equal
    fr, ts = sv2.global_to_frenet(sp2, o["x_est"][0:3].contiguous(), s0=d["x_ic"][0].contiguous())
    assert torch.equal(b["x_ic"][0:3], fr) and torch.equal(o["track_status"], ts) and torch.equal(b["x_ic"][3:6], o["x_est"][3:6])
    assert int(ts.max()) == 0
    # 8 shift + prepare_failed AT THE FUSED x_ic
    nxt = sv2.shift(trk2, inp, sol, DT, speed_scale=XC.SPEED_SCALE)
    if restart:
        sv2.prepare_failed(trk2, b["x_ic"], st, nxt, DT, speed_scale=XC.SPEED_SCALE)
    torch.cuda.synchronize()
    n_last = 0
    for k in KEYS:
        a, r = b["inp"][k], nxt[k]
        if k in ("U_ref", "T_ref"):
            assert torch.equal(a, r), k
            continue
        assert torch.equal(a[..., :-1, :], r[..., :-1, :]), k
        assert torch.equal(a[..., -1, :][..., ~ok], r[..., -1, :][..., ~ok]), k
        n_last += int((a[..., -1, :] != r[..., -1, :]).sum())
        assert torch.allclose(a[..., -1, :], r[..., -1, :], rtol=1e-14, atol=1e-15), (k, float((a[..., -1, :] - r[..., -1, :]).abs().max()))
    if restart and B > 1:   # the cold start is at the ESTIMATE, not at the truth
        assert torch.equal(b["inp"]["X_ref"][:, 0, ~ok], b["x_ic"][:, ~ok]) and not torch.equal(b["inp"]["X_ref"][:, 0, ~ok], b["x"][:, ~ok])
    print("N %d B %d restart %s rows %s %s: filter |dx| %.1e |dP| %.1e |dK| %.1e |dx_est| %.1e (TOL %.0e); last-knot numbers that differ: %d"
          % (N, B, restart, rows_vel, rows_pose, worst["x"], worst["P"], worst["K"], worst["x_est"], EC.TOL, n_last))
    assert max(worst.values()) <= EC.TOL, worst
    return d, b


@pytest.mark.parametrize("restart", [True, False])
@pytest.mark.parametrize("N,B", [(20, XC.WG + 1), (3, XC.WG + 1), (20, 1)])
def test_one_call_is_the_composition_stage_by_stage(world, N, B, restart):
    """Measured on the MI355X (N 20, B 65): the truth, distance, worst_excess, both observations and the projection bit for bit -- no
    relaxation for contraction was needed; the filter's figures are printed."""
    _compose(world, N, B, restart)


def test_other_observation_rows_agree_with_the_unfused_chain_and_a_mixed_one_is_refused(world, pkg):
    """(3, 4, 5) + (0, 1): three velocity rows and a pose without its yaw.  (0, 3) belongs to neither family."""
    import torch
    _compose(world, 20, XC.WG + 1, True, rows_vel=(3, 4, 5), rows_pose=(0, 1))
    _compose(world, 20, XC.WG + 1, True, rows_vel=(5,), rows_pose=(2, 0, 1), nan_seed=False)
    A, _ = world["get"](20)
    d = _scene(world, 20, XC.WG + 1, rows_vel=(0, 3), rows_pose=(0, 1, 2))
    ids = _filter(A, d["est0"], d["P0"], (0, 3), (0, 1, 2))
    b = _buffers(d)
    before = {k: v.clone() for k, v in _flat(b).items()}
    g0 = _store(A)
    for pair in (ids, (ids[1], ids[0]), (ids[1], ids[1])):
        with pytest.raises(pkg.LmpcError, match=r"-> -3: "):
            _advance(A, d, b, pair, True)
    torch.cuda.synchronize()
    _untouched(before, _flat(b), g0, _store(A))


def _flat(b):
    out = {k: b[k] for k in ("x", "u_prev", "x_ic")}
    out.update(b["inp"])
    out.update({k: v for k, v in b["opt"].items() if v is not None})
    return out


def _untouched(before, after, g0, g1):
    for k in before:
        assert _bits(before[k], after[k]), k
    assert g0[1] == g1[1]
    for k in g0[0]:
        assert np.array_equal(g0[0][k], g1[0][k], equal_nan=True), k


def test_three_consecutive_calls_continue_the_clock_and_the_control(world):
    """Three periods of the real loop -- solve, fused call -- with the unfused filter of the second handle fed the fused (u, z, t) after
    each: the stores agree after the third, so the clock and the u store carried over from call to call."""
    import torch
    N, B = 20, XC.WG + 1
    A, U = world["get"](N)
    d = _scene(world, N, B, seed=9)
    ids, ids2 = _filter(A, d["est0"], d["P0"]), _filter(U, d["est0"], d["P0"])
    b = _buffers(d)
    inp = dict(b["inp"], L=world["L"])
    rng = np.random.default_rng(77)
    for k in range(3):
        inp["x_ic"], inp["u_ic"] = b["x_ic"], b["u_prev"]
        sol = A["sv"].solve(inp)
        d["noise_vel"] = _dev(rng.normal(0, 1, (2, B)) * EC.SIG_VEL[:, None])
        noise = rng.normal(0, 1, (3, B)) * EC.SIG_POSE[:, None]
        noise[0, rng.random(B) < 0.1] = np.nan
        d["noise_pose"] = _dev(noise)
        b["inp"] = {key: inp[key] for key in KEYS}
        tv, tp = k * DT_NS + DT_NS // 2, (k + 1) * DT_NS
        _advance(A, d, b, ids, True, t_vel=tv, t_pose=tp, sol=sol)
        U["sv"].ekf_update_control(b["u_prev"])
        U["sv"].ekf_update(ids2[0], b["opt"]["z_vel"], d["R_vel"], tv)
        xe, _, _, _ = U["sv"].ekf_update(ids2[1], b["opt"]["z_pose"], d["R_pose"], tp)
        torch.cuda.synchronize()
    (ga, ta), (gu, tu) = _store(A), _store(U)
    worst = {k: float(np.abs(ga[k] - gu[k]).max()) for k in ga}
    print("three calls: |dx| %.1e |dP| %.1e |dK| %.1e, clock %d ns, failed solves %d" % (worst["x"], worst["P"], worst["K"], ta, int(b["opt"]["n_fail"].sum())))
    assert ta == tu == 3 * DT_NS and max(worst.values()) <= EC.TOL, worst
    assert np.isfinite(ga["x"]).all() and bool(torch.isfinite(b["x"]).all())
    assert torch.equal(b["opt"]["x_est"], xe) or float((b["opt"]["x_est"] - xe).abs().max()) <= EC.TOL
    assert float(b["opt"]["distance"].min()) > 3 * DT * 1.0   # (the cars moved three periods at more than 1 m/s)


def test_every_optional_pointer_null_and_a_repeat_gives_the_same_bits(world):
    import torch
    N, B = 20, XC.WG + 1
    A, _ = world["get"](N)
    d = _scene(world, N, B, seed=6)
    runs = []
    for optional in (True, False, False):
        ids = _filter(A, d["est0"], d["P0"])
        b = _buffers(d, optional=optional)
        _advance(A, d, b, ids, True)
        torch.cuda.synchronize()
        runs.append((_flat(b), _store(A)))
    full, bare, again = runs
    for k in bare[0]:   # what is always written does not depend on the optional arrays, and a repeat is the same bits
        assert _bits(bare[0][k], full[0][k]) and _bits(bare[0][k], again[0][k]), k
    for k in bare[1][0]:
        assert np.array_equal(bare[1][0][k], full[1][0][k]) and np.array_equal(bare[1][0][k], again[1][0][k]), k
    assert bare[1][1] == full[1][1] == DT_NS
    # one optional array at a time: the others' absence does not move it
    for name in OPTIONAL:
        ids = _filter(A, d["est0"], d["P0"])
        b = _buffers(d)
        b["opt"] = {k: (v if k == name else None) for k, v in b["opt"].items()}
        _advance(A, d, b, ids, True)
        torch.cuda.synchronize()
        assert _bits(b["opt"][name], full[0][name]), name


def test_every_refusal_returns_its_code_and_touches_nothing(world, pkg):
    import torch
    N, B = 20, XC.WG + 1
    A, _ = world["get"](N)
    sv = A["sv"]
    d = _scene(world, N, B, seed=7)
    b = _buffers(d)
    before = {k: v.clone() for k, v in _flat(b).items()}

    def refused(code, call):
        with pytest.raises(pkg.LmpcError, match=r"-> %d: " % code):
            call()

    # no filter, a filter that is not initialised, another batch
    sv.ekf_destroy()
    refused(-1, lambda: _advance(A, d, b, (0, 1), True))
    cfg = EC.config()
    sv.ekf_create(B, cfg["x0"], cfg["P0"], cfg["Q"], cfg["x_min"], cfg["x_max"])
    ids = sv.ekf_register_observation(EC.ROWS_VEL), sv.ekf_register_observation(EC.ROWS_POSE)
    sv.ekf_set_state(d["est0"], d["P0"])
    refused(-1, lambda: _advance(A, d, b, ids, True))
    ids = _filter(A, d["est0"][:, :B - 1].contiguous(), d["P0"][..., :B - 1].contiguous())
    refused(-1, lambda: _advance(A, d, b, ids, True))
    ids = _filter(A, d["est0"], d["P0"])
    sv.ekf_update(-1, None, None, 1000)   # (the clock off zero, so that a refused call that moved it would show)
    torch.cuda.synchronize()
    g0 = _store(A)
    assert g0[1] == 1000
    # unknown observation ids
    for pair in ((ids[0], 2), (-1, ids[1]), (7, 7)):
        refused(-1, lambda pair=pair: _advance(A, d, b, pair, True))
    # dt, dt_sim, n_sub
    call = lambda **kw: sv.loop_advance_estimated(**dict(dict(   # noqa: E731
        track=A["trk"], spline=A["spline"], inp=b["inp"], sol=d["sol"], x=b["x"], u_prev=b["u_prev"], x_ic=b["x_ic"], dt=DT, dt_sim=DT / 2, n_sub=2,
        obs_vel=ids[0], obs_pose=ids[1], t_vel_ns=DT_NS // 2, t_pose_ns=DT_NS, noise_vel=d["noise_vel"], R_vel=d["R_vel"], noise_pose=d["noise_pose"],
        R_pose=d["R_pose"], **b["opt"]), **kw))
    for kw in (dict(dt=0.0), dict(dt=-DT), dict(dt=math.nan), dict(dt_sim=0.0), dict(dt_sim=math.nan), dict(n_sub=3), dict(n_sub=1), dict(n_sub=0),
               dict(n_sub=-2)):
        refused(-1, lambda kw=kw: call(**kw))
    # references aliasing the solution
    refused(-1, lambda: call(inp=dict(b["inp"], X_ref=d["sol"]["X_optm"])))
    refused(-1, lambda: call(inp=dict(b["inp"], U_ref=d["sol"]["U_optm"])))
    # a NULL required pointer, one at a time; a NULL io, track or spline
    io = pkg.capi.CEstimatedLoop()
    ptrs = dict(X_optm=d["sol"]["X_optm"], U_optm=d["sol"]["U_optm"], status=d["sol"]["status"], x=b["x"], u_prev=b["u_prev"], x_ic=b["x_ic"],
                noise_vel=d["noise_vel"], R_vel=d["R_vel"], noise_pose=d["noise_pose"], R_pose=d["R_pose"], **b["inp"], **b["opt"])
    for name, t in ptrs.items():
        setattr(io, name, t.data_ptr())
    io.dt, io.dt_sim, io.speed_scale, io.speed_limit = DT, DT / 2, XC.SPEED_SCALE, float(sv.config["x_max"][3])
    io.n_sub, io.restart_failed, io.obs_vel, io.obs_pose, io.t_vel_ns, io.t_pose_ns = 2, 1, ids[0], ids[1], DT_NS // 2, DT_NS
    ct = sv._ctrack(A["trk"])
    fn = sv.lib.lmpc_loop_advance_estimated_batch
    required = [n for n in ptrs if n not in OPTIONAL]
    assert len(required) == 17
    for name in required:
        setattr(io, name, None)
        assert fn(sv._h, C.c_int32(B), C.byref(ct), A["spline"]._p, C.byref(io)) == -1, name
        setattr(io, name, ptrs[name].data_ptr())
    assert fn(sv._h, C.c_int32(B), C.byref(ct), A["spline"]._p, None) == -1
    assert fn(sv._h, C.c_int32(B), None, A["spline"]._p, C.byref(io)) == -1
    assert fn(sv._h, C.c_int32(B), C.byref(ct), None, C.byref(io)) == -1
    # unsupported: the AOS layout, either controller-model switch
    sv.set_output_layout("aos")
    refused(-3, call)
    sv.set_output_layout("soa")
    sv.set_car_vehicles([pkg.presets.barc_vehicle()] * B)
    sv.set_cars_controller_model(True)
    refused(-3, call)
    sv.set_cars_controller_model(False)
    sv.set_car_vehicles(None)
    sv.set_dtrack_vehicles([pkg.presets.barc_double_track()] * B)
    sv.set_dtrack_controller_model(True)
    refused(-3, call)
    sv.set_dtrack_controller_model(False)
    sv.set_dtrack_vehicles(None)
    torch.cuda.synchronize()
    _untouched(before, _flat(b), g0, _store(A))
    # and the same arguments, unrefused, go through (the struct built by hand here is the one the binding builds)
    assert fn(sv._h, C.c_int32(B), C.byref(ct), A["spline"]._p, C.byref(io)) == 0
    torch.cuda.synchronize()
    assert _store(A)[1] == DT_NS and not _bits(before["x"], b["x"])


def test_a_nan_truth_and_a_nan_estimate_stay_in_their_cars(world):
    """Car 3's truth and car 9's estimate are NaN (one a successful solve's car, one in the tail workgroup would be car 64: it gets a NaN
    seed): every other car's outputs are the bits of the clean run."""
    import torch
    N, B = 20, XC.WG + 1
    A, _ = world["get"](N)
    d = _scene(world, N, B, seed=8)
    runs = []
    for dirty in (False, True):
        x, est0, x_ic = d["x"].clone(), d["est0"].clone(), d["x_ic"].clone()
        if dirty:
            x[:, 3], est0[:, 9], x_ic[0, 64] = math.nan, math.nan, math.nan
        ids = _filter(A, est0, d["P0"])
        b = _buffers(dict(d, x=x, x_ic=x_ic))
        _advance(A, d, b, ids, True)
        torch.cuda.synchronize()
        got = _flat(b)
        got.update({"store " + k: _dev(v) for k, v in _store(A)[0].items()})
        runs.append(got)
    clean, dirty = runs
    others = torch.ones(B, dtype=torch.bool, device="cuda")
    others[[3, 9]] = False
    for k in clean:
        sel = others.clone()
        if k in ("x_ic", "track_status") or k in KEYS:
            sel[64] = k in KEYS and bool(d["sol"]["status"][64] == 0)   # (car 64's projection started elsewhere; its plan is untouched if its solve held)
        assert _bits(clean[k][..., sel].contiguous(), dirty[k][..., sel].contiguous()), k
    assert bool(torch.isnan(dirty["x"][:, 3]).all()) and bool(torch.isnan(dirty["x_est"][:, 9]).any())
    assert int(dirty["track_status"][9]) == 2 and int(dirty["ekf_flags"][9]) & EC.NOT_FINITE
    # car 64 started from the nearest waypoint and arrived where the seeded run did
    assert int(dirty["track_status"][64]) == 0 and float((dirty["x_ic"][:, 64] - clean["x_ic"][:, 64]).abs().max()) < 1e-9


def _x0(world, B, seed=2):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, world["L"], B), rng.uniform(-0.05, 0.05, B), np.zeros(B), rng.uniform(1.5, 2.5, B), np.zeros(B), np.zeros(B)])


def test_replay_of_a_fused_run_through_the_numpy_filter(world, pkg):
    """64 cars x 100 periods of run_estimated_fused with the optional outputs recorded; the recorded (u, z, t) of 8 cars replayed
    through ekf_cases.Filter gives the recorded estimates -- the filter is open-loop in them."""
    import torch
    A, _ = world["get"](20)
    B, steps, nb = 64, 100, 8
    x0 = torch.as_tensor(_x0(world, B), device="cuda")
    u0 = torch.zeros((2, B), dtype=torch.float64, device="cuda")
    res = pkg.closed_loop.run_estimated_fused(A["sv"], world["tab"], A["spline"], x0, u0, steps, seed=4, record_trace=True, poll=25)
    for key in ("x", "x_est", "rms_error", "distance", "worst_excess"):
        assert bool(torch.isfinite(res[key]).all()), key
    assert int(res["track_status"].max()) == 0 and not bool((res["ekf_flags"] & EC.NOT_FINITE).any())
    assert len(res["trace"]) == 2 * steps
    host = lambda t: np.moveaxis(t.cpu().numpy(), -1, 0)   # noqa: E731
    cfg = {k: np.asarray(v, dtype=np.float64) for k, v in res["ekf_config"].items()}
    ref = EC.Filter(OP.barc_vehicle(), cfg, nb)
    ref.register_observation(EC.ROWS_VEL)
    ref.register_observation(EC.ROWS_POSE)
    ref.set_state(host(res["x_est0"])[:nb], host(res["P0"])[:nb])
    ref.initialize(0)
    worst, n_drop, n_cmp = 0.0, 0, 0
    for obs, z, R, u, ns, x_est in res["trace"]:
        ref.update_control(host(u)[:nb])
        x, _, _, fl = ref.update(obs, host(z)[:nb], host(R)[:nb], ns)
        n_drop += int((fl & EC.FALLBACK).sum())
        if x_est is not None:
            worst = max(worst, float(np.abs(x - host(x_est)[:nb]).max()))
            n_cmp += 1
    print("replay of %d cars: |dx| %.2e over %d updates (%d compared), %d dropouts; rms error %s; failed solves %d of %d"
          % (nb, worst, len(res["trace"]), n_cmp, n_drop, res["rms_error"].cpu().numpy().round(4), int(res["n_fail"].sum()), B * steps))
    assert n_cmp == steps and n_drop > 0 and worst <= EC.TOL, worst


def test_fused_loop_against_the_unfused_loop(world, pkg):
    """64 cars x 40 periods, run_estimated_fused against run_estimated under identical sensors, on the cars with no failed solve in any
    run (at least 90 % must remain).  The bound is measured, not chosen: S, the largest scaled difference of the final states between
    run_estimated from x0 and from x0 moved one ulp, is what rounding ONCE does to this loop; the fused kernel may round differently in
    each of 40 periods, hence 100 S, and never below the 1e-9 tests/test_gpu_loop.py asks of the tracking loop.
    Measured on the MI355X: see profiles/estimated_fused.md."""
    import torch
    A, U = world["get"](20)
    B, steps = 64, 40
    x0 = torch.as_tensor(_x0(world, B, seed=12), device="cuda")
    u0 = torch.zeros((2, B), dtype=torch.float64, device="cuda")
    x0_ulp = torch.nextafter(x0, torch.full_like(x0, math.inf))
    kw = dict(steps=steps, seed=11)
    base = pkg.closed_loop.run_estimated(U["sv"], world["tab"], U["spline"], x0, u0, **kw)
    moved = pkg.closed_loop.run_estimated(U["sv"], world["tab"], U["spline"], x0_ulp, u0, **kw)
    fused = pkg.closed_loop.run_estimated_fused(A["sv"], world["tab"], A["spline"], x0, u0, **kw)
    torch.cuda.synchronize()
    same = (base["n_fail"] == 0) & (moved["n_fail"] == 0) & (fused["n_fail"] == 0)
    sx = torch.tensor([2000.0, 10.0, 0.1, 80.0, 2.0, 2.0], dtype=torch.float64, device="cuda")[:, None]

    def dist(a, b):
        dx = a["x"] - b["x"]
        de = a["x_est"] - b["x_est"]
        de[2] = torch.atan2(torch.sin(de[2]), torch.cos(de[2]))
        return max(float((dx / sx).abs()[:, same].max()), float((de / sx).abs()[:, same].max()))

    S, got = dist(moved, base), dist(fused, base)
    bound = max(100.0 * S, 1e-9)
    print("loop against loop, %d periods: cars without a failed solve %d of %d (failed solves: %d / %d / %d); S = %.2e, fused - unfused = %.2e, "
          "bound %.2e; rms error fused %s unfused %s" % (steps, int(same.sum()), B, int(base["n_fail"].sum()), int(moved["n_fail"].sum()),
                                                         int(fused["n_fail"].sum()), S, got, bound, fused["rms_error"].cpu().numpy().round(4),
                                                         base["rms_error"].cpu().numpy().round(4)))
    assert int(same.sum()) >= 0.9 * B
    assert got <= bound, (got, S)
    assert torch.equal(fused["n_fail"][same], base["n_fail"][same]) and torch.equal(fused["ekf_flags"][same], base["ekf_flags"][same])
    assert float((fused["distance"] - base["distance"]).abs()[same].max()) <= bound * 2000.0
    assert float(fused["distance"].median()) > 0.5 * steps * DT * 1.0      # (the cars do move)
