"""Vehicles, draws and an audit that take the vehicle-model kernels off the preset vehicles (tests/test_envelope_reference.py,
tests/test_gpu_envelope.py).

Every preset, every test vehicle and every fixture of the suite has kd = 0, Af = 1 and rho = 1.2, the per-car tables never vary the
powertrain split, the aero or the rolling resistance, and every BARC-scale draw keeps |u_lon| <= 0.01, where tanh(u_lon) is 0 and the
drive / brake blend sits at its midpoint.  Here:

  * envelope_vehicle / dtrack_envelope_vehicle: every field the dynamics read off its preset value, kd strictly inside (0, 1),
    Af != 1, rho != Af (upstream's ax carries Af without rho, drag and downforce carry both: only Af != 1 tells them apart);
  * table: three distinct cars by b % 3 -- the envelope vehicle, one with kd = 1 (kb and cd moved again), one on Euler;
  * envelope_draws: linearisation points that are no trajectory, a third saturated on the drive side of the tanh blend, a third on
    the brake side, a third at its midpoint; steer to the actuator limit, slip past the Pacejka peak, e_y k up to about 0.3;
  * audit: for every field the model reads, + 10 % must move the reference's Jacobian and its one-step state on at least a
    quarter of the problems -- a condition on the INPUTS, which keeps a test on them from being blind to a field;
  * per_problem: the error of one (problem, stage) against the largest entry of that same (problem, stage), so that a slow car's
    |A| of hundreds does not hide an error in a fast car's |A| of one.

The references are the oracle's (oracle.dynamics) and tests/dtrack_cases.py / tests/dtrack_model_cases.py; nothing here is derived from
a kernel."""
from __future__ import annotations

import numpy as np

import cars_model_cases as CM
import dtrack_cases as DT
from oracle import dynamics as D, params as P
from tolerances import TOL_LINEARIZE_REL

KEYS = ("X_ref", "U_ref", "T_ref", "curvatures")
KINDS = ("barc", "iac")
B_TEST, N_TEST = 130, 4          # two waves and two lanes; three stages, one per band of u_lon for every problem
DT_SIM, N_SUB = 0.0125, 2        # the plant steps

# what the single-track dynamics read (oracle.dynamics.f_continuous), and what the double track reads on top (dtrack_cases)
FIELDS = ("m", "Jzz", "l", "cg_ratio", "h", "fr", "kd", "kb", "cd", "Af", "rho", "cl_f", "cl_r", "mu", "Bf", "Cf", "Br", "Cr")
DTRACK_FIELDS = FIELDS + ("tw_f", "tw_r", "kroll_f", "Ef", "Er", "eps_f", "eps_r", "Fz0_f", "Fz0_r")
# fields of the vehicle the dynamics provably do not read: none occurs in f_continuous of either model
NOT_READ = {
    "b": "the body width: only the QP's boundary rows read it (oracle.qp)",
    "Fd_max": "actuator limit: the QP's input box (oracle.qp.effective_bounds)",
    "Fb_max": "actuator limit: the QP's input box",
    "Td": "actuator time constant: the QP's rate box",
    "Tb": "actuator time constant: the QP's rate box",
    "max_steer": "actuator limit: the QP's input box",
    "max_steer_rate": "actuator limit: the QP's rate box",
    "model_id": "selects the model, no term of it",
    "integrator": "selects the integrator (the Euler car of the table covers it)",
}
AUDIT_MOVE, AUDIT_SHARE = 1e-6, 0.25


def presets():
    from __graft_entry__ import load_package
    return load_package().presets


def base_vehicle(kind, track="single"):
    p = presets()
    return {("barc", "single"): p.barc_vehicle, ("iac", "single"): p.iac_vehicle,
            ("barc", "double"): p.barc_double_track, ("iac", "double"): p.iac_double_track}[kind, track]()


# ---- vehicles ----------------------------------------------------------------------------------------------------------------------
def envelope_vehicle(base):
    """`base` (presets.barc_vehicle() or iac_vehicle(), or a double-track dict) with every field of FIELDS off its value."""
    return dict(base, m=1.07 * base["m"], Jzz=1.12 * base["Jzz"], l=1.05 * base["l"], cg_ratio=0.56, h=1.3 * base["h"], fr=0.02,
                kd=0.35, kb=0.37, cd=0.45, Af=1.7, rho=1.05, cl_f=0.6, cl_r=0.9, mu=0.93 * base["mu"],
                Bf=0.9 * base["Bf"], Cf=0.95 * base["Cf"], Br=0.85 * base["Br"], Cr=0.92 * base["Cr"])


def dtrack_envelope_vehicle(base):
    """presets.barc_double_track() / iac_double_track() with every field of DTRACK_FIELDS off its value, tw_f != tw_r."""
    return dict(envelope_vehicle(base), tw_f=0.95 * base["tw_f"], tw_r=1.08 * base["tw_r"], kroll_f=0.42, Ef=0.7, Er=0.55,
                eps_f=0.8 * base["eps_f"], eps_r=1.15 * base["eps_r"], Fz0_f=1.1 * base["Fz0_f"], Fz0_r=0.9 * base["Fz0_r"])


def kinds(env):
    """the three cars of a table: the envelope vehicle; all of the drive force on the front axle (kd = 1) and another brake split and
    drag; the envelope vehicle on Euler"""
    return (dict(env), dict(env, kd=1.0, kb=0.63, cd=0.8 * env["cd"]), dict(env, integrator="euler"))


def table(kind, B, track="single"):
    """by b % 3"""
    base = base_vehicle(kind, track)
    k = kinds(envelope_vehicle(base) if track == "single" else dtrack_envelope_vehicle(base))
    return [k[b % 3] for b in range(B)]


def off_preset(env, base, fields):
    """the fields of `fields` that the envelope vehicle leaves on the preset's value (must be none)"""
    return [f for f in fields if env[f] == base[f]]


# ---- the measure -------------------------------------------------------------------------------------------------------------------
def per_problem(got, want, floor=0.0):
    """[N-1, B] of arrays whose two trailing axes are (stage, problem): max over the entries of one (problem, stage) of |got - want|,
    over the max over the same entries of |want|; floor = 1.0 gives g's max(1, |want|) scale."""
    got, want = np.asarray(got), np.asarray(want)
    lead = tuple(range(want.ndim - 2))
    return np.abs(got - want).max(axis=lead) / np.maximum(floor, np.abs(want).max(axis=lead))


def bounds(analytic, cs):
    """Per (problem, stage) the bound of A, Bm and g of a device linearisation held to the complex-step Jacobian `cs`:
    max(TOL_LINEARIZE_REL, 8 x per_problem(analytic, complex step)) on that same problem -- the reference's own rounding sets the
    allowance, the 8 covers the other summation order of the device's forward-mode chain -- and 10 x that for g on max(1, |g|)."""
    bA = np.maximum(TOL_LINEARIZE_REL, 8.0 * per_problem(analytic[0], cs[0]))
    bB = np.maximum(TOL_LINEARIZE_REL, 8.0 * per_problem(analytic[1], cs[1]))
    return bA, bB, 10.0 * np.maximum(bA, bB)


def errors(got, cs):
    """per (problem, stage): the device's (A, Bm, g) against the complex step's in the per-problem measure"""
    return per_problem(got[0], cs[0]), per_problem(got[1], cs[1]), per_problem(got[2], cs[2], floor=1.0)


def complex_step(inp, veh):
    return CM.reference(inp, veh, jac=lambda x, u, k, dt, v: D.rk4_jacobian_cs(x, u, k, dt, v))


def held_per_problem(label, got, inp, v: P.Vehicle):
    """A device linearisation `got` = (A [6, 6, N-1, B], Bm [6, 2, N-1, B], g [6, N-1, B]) of the inputs `inp` on ONE vehicle, held
    per (problem, stage) to the complex step under bounds(); prints the worst figures."""
    NS = inp["U_ref"].shape[1]
    x, u = np.asarray(inp["X_ref"])[:, :NS].transpose(1, 2, 0), np.asarray(inp["U_ref"]).transpose(1, 2, 0)
    k, dt = np.asarray(inp["curvatures"])[:NS], np.asarray(inp["T_ref"])

    def layout(a, b, c):
        return a.transpose(2, 3, 0, 1), b.transpose(2, 3, 0, 1), c.transpose(2, 0, 1)
    cs, an = layout(*D.rk4_jacobian_cs(x, u, k, dt, v)), layout(*CM.stage_jacobian(x, u, k, dt, v))
    err, bnd = errors(got, cs), bounds(an, cs)
    print("%s, per problem: A %.2e Bm %.2e g %.2e (analytic against complex step: A %.2e Bm %.2e); worst error / bound %.2f"
          % (label, *(e.max() for e in err), per_problem(an[0], cs[0]).max(), per_problem(an[1], cs[1]).max(),
             max(float((e / b).max()) for e, b in zip(err, bnd))))
    for name, e, b in zip(("A", "Bm", "g"), err, bnd):
        assert (e <= b).all(), (label, name, float((e / b).max()), np.unravel_index(np.argmax(e / b), e.shape))


# ---- draws -------------------------------------------------------------------------------------------------------------------------
SATURATED, MIDPOINT = 0.99, 0.05
# (range of vy / vx, |omega|, |e_y|, |k|, drive band of u_lon, brake band of u_lon)
RANGES = {"barc": (0.35, 1.5, 0.4, 0.8, (2.7, 3.2), (-3.2, -2.7)),
          "iac": (0.35, 1.5, 6.0, 0.05, (2.7, 8.0), (-15.0, -2.7))}
VX_MIN = {"barc": 0.3, "iac": 5.0}
# vx per band (drive, brake, midpoint).  The double track divides by the native speed v, its slip rate carries 1 / (m v), and its
# plant holds v at 1e-6 from below between sub-steps.  A BARC-scale car under a saturated input (1000 N per unit of u_lon on 2.4 kg)
# gains or loses some 30 m/s in 25 ms and turns its slip angle by tens of radians per step below a few m/s, where no two
# implementations reproduce each other; so on the double track its two saturated bands are drawn fast enough to stay clear of the
# guard through the plant's two sub-steps, and its midpoint band from 1 m/s.  Every other band keeps the single track's speeds.
VX = {("barc", "single"): ((0.3, 4.0),) * 3, ("iac", "single"): ((5.0, 90.0),) * 3,
      ("barc", "double"): ((60.0, 75.0), (60.0, 75.0), (1.0, 4.0)), ("iac", "double"): ((5.0, 90.0),) * 3}
BRAKE_BAND = {"barc": (-2.9, -2.7), "iac": (-15.0, -2.7)}   # the double track's
MIN_DEN = 0.02   # |vx + 1e-3| (single track) / |v| (double track) at every evaluation of the dynamics inside a step


def band(i, b):
    """0: drive side saturated, 1: brake side saturated, 2: midpoint -- every problem sees each band on one stage in three"""
    return (np.asarray(i) + np.asarray(b)) % 3


def envelope_draws(kind, B, N, seed=7, track="single"):
    """Independent linearisation points per stage, as cars_model_cases.lin_draws returns them (batch axis last): X_ref [6, N, B],
    U_ref [2, N-1, B], T_ref [N-1, B] in [0.5, 1.5] x 0.025, curvatures [N, B]."""
    rng = np.random.default_rng(seed + 1000 * N + B)
    ratio, om, ey, kmax, drive, brake = RANGES[kind]
    steer = base_vehicle(kind)["max_steer"]
    sh = (N, B)
    bd = band(*np.meshgrid(np.arange(N), np.arange(B), indexing="ij"))
    vx = np.choose(bd, [rng.uniform(*r, sh) for r in VX[kind, track]])
    if track == "double":
        brake = BRAKE_BAND[kind]
    X = np.stack([rng.uniform(0.0, 10.0, sh), rng.uniform(-ey, ey, sh), rng.uniform(-0.6, 0.6, sh), vx, rng.uniform(-ratio, ratio, sh) * vx,
                  rng.uniform(-om, om, sh)])
    ul = np.where(bd == 0, rng.uniform(*drive, sh), np.where(bd == 1, rng.uniform(*brake, sh), rng.uniform(-0.04, 0.04, sh)))
    U = np.stack([ul, rng.uniform(-steer, steer, sh)])[:, : N - 1]
    inp = {"X_ref": np.ascontiguousarray(X), "U_ref": np.ascontiguousarray(U), "T_ref": 0.025 * rng.uniform(0.5, 1.5, (N - 1, B)),
           "curvatures": rng.uniform(-kmax, kmax, sh)}
    check_draws(kind, inp, track)
    return inp


def peak_slip(inp, v):
    """[N-1, B] bool: C atan(B alpha) beyond pi / 2 on the front or the rear axle of the single-track vehicle dict v"""
    NS = inp["U_ref"].shape[1]
    vx, vy, om = (inp["X_ref"][r, :NS] for r in (3, 4, 5))
    lr = v["cg_ratio"] * v["l"]
    lf = v["l"] - lr
    af = inp["U_ref"][1] - np.arctan((lf * om + vy) / (vx + 1e-3))
    ar = np.arctan((lr * om - vy) / (vx + 1e-3))
    return (np.abs(v["Cf"] * np.arctan(v["Bf"] * af)) > np.pi / 2) | (np.abs(v["Cr"] * np.arctan(v["Br"] * ar)) > np.pi / 2)


def discriminant(z, u, p):
    """b^2 - 4 a c of dtrack_cases.gamma_closed_form at the native states z (..., 6)"""
    Fx_f, _, Fz_f, Fz_r, S = DT.tyre_terms(z, u, p)
    delta = u[..., 1]
    cg = p["h"] / (0.5 * (p["tw_f"] + p["tw_r"]))
    F, sigma = (Fz_f, Fz_f, Fz_r, Fz_r), (-1.0, 1.0, -1.0, 1.0)
    kappa = (p["kroll_f"], p["kroll_f"], 1.0 - p["kroll_f"], 1.0 - p["kroll_f"])
    e = (p["eps_f"] / p["Fz0_f"],) * 2 + (p["eps_r"] / p["Fz0_r"],) * 2
    w = (np.cos(delta), np.cos(delta), 1.0, 1.0)
    a = sum(-cg * w[i] * p["mu"] * S[i] * e[i] * kappa[i] ** 2 for i in range(4))
    b = 1.0 + sum(-cg * w[i] * p["mu"] * S[i] * sigma[i] * kappa[i] * (1.0 + 2.0 * e[i] * F[i]) for i in range(4))
    c = -cg * (sum(w[i] * p["mu"] * S[i] * (F[i] + e[i] * F[i] ** 2) for i in range(4)) + 2.0 * Fx_f * np.sin(delta))
    return b * b - 4.0 * a * c


def stage_points(x, u, k, dt, f, euler=False):
    """the states at which one RK4 (or Euler) step from x evaluates the dynamics f(x, u, k)"""
    pts = [x]
    if not euler:
        for c in (0.5, 0.5, 1.0):
            pts.append(x + c * dt[..., None] * f(pts[-1], u, k))
    return pts


def check_draws(kind, inp, track="single"):
    """the conditions the module states, asserted on the draws themselves"""
    NS, B = inp["U_ref"].shape[1:]
    th = np.tanh(inp["U_ref"][0])
    i, b = np.meshgrid(np.arange(NS), np.arange(B), indexing="ij")
    bd = band(i, b)
    assert (th[bd == 0] > SATURATED).all() and (th[bd == 1] < -SATURATED).all() and (np.abs(th[bd == 2]) < MIDPOINT).all()
    if NS * B >= 30:
        assert min((bd == j).mean() for j in range(3)) > 0.3
    assert (inp["X_ref"][3] >= VX_MIN[kind]).all() and (inp["T_ref"] >= 0.0125).all() and (inp["T_ref"] <= 0.0375).all()
    assert np.abs(inp["U_ref"][1]).max() <= base_vehicle(kind)["max_steer"]
    assert np.abs(inp["X_ref"][1] * inp["curvatures"]).max() < 0.35
    env = envelope_vehicle(base_vehicle(kind))
    if NS * B >= 30:
        assert peak_slip(inp, env).mean() >= 0.25, peak_slip(inp, env).mean()
        assert np.abs(inp["X_ref"][1] * inp["curvatures"]).max() > 0.2 and np.abs(inp["U_ref"][1]).max() > 0.95 * env["max_steer"]
    x, u = inp["X_ref"][:, :NS].transpose(1, 2, 0), inp["U_ref"].transpose(1, 2, 0)
    kap = inp["curvatures"][:NS]
    if track == "single":
        for v in kinds(env)[:2]:
            ov = CM.oracle_vehicle(v)
            for p in stage_points(x, u, kap, inp["T_ref"], lambda a, c, d: D.f_continuous(a, c, d, ov)):
                assert np.abs(p[..., 3] + 1e-3).min() > MIN_DEN
    else:
        for p_ in kinds(dtrack_envelope_vehicle(base_vehicle(kind, "double")))[:2]:
            z = DT.to_native(x)
            assert z[..., 5].min() > 0.25   # clear of the 1e-6 guard
            for p in stage_points(z, u, kap, inp["T_ref"], lambda a, c, d: DT.f_continuous(a, c, d, p_)[0]):
                assert np.abs(p[..., 5]).min() > MIN_DEN and (discriminant(p, u, p_) > 0).all()


# ---- plant draws -------------------------------------------------------------------------------------------------------------------
def plant_draws(kind, B, L, seed=7, track="single"):
    """Stage 0 of envelope_draws (states), the inputs of its stage 0, and s spread over the track: x (B, 6), u (B, 2)."""
    inp = envelope_draws(kind, B, N_TEST, seed, track)
    x, u = inp["X_ref"][:, 0].T.copy(), inp["U_ref"][:, 0].T.copy()
    x[:, 0] = np.random.default_rng(seed + B).uniform(0.0, L, B)
    return x, u


def check_single_plant(tr, x, u, veh):
    """vx + 1e-3 clear of zero at every evaluation of the dynamics in both sub-steps"""
    from oracle import scenario as S
    for cars in CM.groups(veh):
        ov, xx = CM.oracle_vehicle(veh[cars[0]]), np.array(x[cars], dtype=np.float64)
        for _ in range(N_SUB):
            k = S.track_lookup(tr["curvature"], xx[:, 0], float(tr["L"]))
            for q in stage_points(xx, u[cars], k, np.full(len(cars), DT_SIM), lambda a, c, d: D.f_continuous(a, c, d, ov), euler=ov.integrator == "euler"):
                assert np.abs(q[:, 3] + 1e-3).min() > MIN_DEN
            xx = D.rk4(xx, u[cars], k, DT_SIM, ov)


def check_dtrack_plant(tr, x, u, veh):
    """v clear of the guard at the start of both sub-steps and after the last one, the discriminant positive at every evaluation"""
    from oracle import scenario as S
    groups = {}
    for b, v in enumerate(veh):
        groups.setdefault(tuple(sorted(v.items())), []).append(b)
    for cars in groups.values():
        p = veh[cars[0]]
        z = DT.to_native(np.array(x[cars], dtype=np.float64))
        for _ in range(N_SUB + 1):
            assert z[:, 5].min() > 0.25, z[:, 5].min()
            k = S.track_lookup(tr["curvature"], z[:, 0], float(tr["L"]))
            for q in stage_points(z, u[cars], k, np.full(len(cars), DT_SIM), lambda a, c, d: DT.f_continuous(a, c, d, p)[0],
                                  euler=p["integrator"] == "euler"):
                assert np.abs(q[:, 5]).min() > MIN_DEN and (discriminant(q, u[cars], p) > 0).all()
            z = DT.step_native(z, u[cars], k, DT_SIM, p)


# ---- the audit ---------------------------------------------------------------------------------------------------------------------
def _single(kind, B, N, seed):
    inp = envelope_draws(kind, B, N, seed)
    env = envelope_vehicle(base_vehicle(kind))
    NS = N - 1
    x, u = inp["X_ref"][:, :NS].transpose(1, 2, 0), inp["U_ref"].transpose(1, 2, 0)

    def model(v):
        A, Bm, _ = complex_step(inp, [v] * B)
        return A, Bm, D.rk4(x, u, inp["curvatures"][:NS], inp["T_ref"], CM.oracle_vehicle(v))
    return env, FIELDS, model


def _double(kind, B, N, seed):
    import dtrack_model_cases as DM
    inp = envelope_draws(kind, B, N, seed, "double")
    env = dtrack_envelope_vehicle(base_vehicle(kind, "double"))
    NS = N - 1
    x, u = inp["X_ref"][:, :NS].transpose(1, 2, 0), inp["U_ref"].transpose(1, 2, 0)

    def model(v):
        A, Bm, _ = DM.reference(inp, [v] * B)
        return A, Bm, DM.numpy_step(x, u, inp["curvatures"][:NS], inp["T_ref"], v)
    return env, DTRACK_FIELDS, model


def audit(kind, track="single", B=B_TEST, N=N_TEST, seed=7):
    """{field: (problems whose A or Bm moved, problems whose one-step state moved, problems)}: the field raised by 10 % on the
    envelope vehicle, `moved` = by more than AUDIT_MOVE in the per-problem measure (the state on max(1, |state|)).  Raises unless
    every field the model reads moves both on at least AUDIT_SHARE of the (problem, stage) points, and unless the fields of the
    vehicle are exactly the audited ones and NOT_READ."""
    env, fields, model = (_single if track == "single" else _double)(kind, B, N, seed)
    assert set(env) == set(fields) | set(NOT_READ), set(env) ^ (set(fields) | set(NOT_READ))
    assert not off_preset(env, base_vehicle(kind, track), fields)
    assert 0.0 < env["kd"] < 1.0 and env["Af"] != 1.0 and env["rho"] != env["Af"]
    A, Bm, xp = model(env)
    assert np.isfinite(A).all() and np.isfinite(Bm).all() and np.isfinite(xp).all()
    out = {}
    for f in fields:
        Aw, Bw, xw = model(dict(env, **{f: 1.1 * env[f]}))
        jac = np.maximum(per_problem(Aw, A), per_problem(Bw, Bm))
        step = np.abs(xw - xp).max(axis=-1) / np.maximum(1.0, np.abs(xp).max(axis=-1))
        out[f] = (int((jac > AUDIT_MOVE).sum()), int((step > AUDIT_MOVE).sum()), jac.size)
    blind = {f: v for f, v in out.items() if min(v[0], v[1]) < AUDIT_SHARE * v[2]}
    assert not blind, blind
    return out


def oracle_envelope(kind, **over) -> P.Vehicle:
    """the single-track envelope vehicle as the oracle's Vehicle"""
    return CM.oracle_vehicle(dict(envelope_vehicle(base_vehicle(kind)), **over))
