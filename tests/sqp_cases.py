"""One pass of the sequential-QP solve of the nonlinear-dynamics problem (lmpc_solve_full_dynamics_batch), restated in plain numpy
from its contract: the header comment of lmpc_solve_full_dynamics_batch (include/lmpc_hip.h), the comment block on top of
csrc/lmpc_sqp_kernel.hip and the cost of racing_mpc.cpp:442-543.  No GPU here; tests/test_sqp_reference.py pins these functions on
an independent assembly and on hand-worked cases, tests/test_gpu_sqp.py holds the device to them pass by pass.

Arrays are [field][knot][batch] (X [6][N][B], U and dU [2][N-1][B], lambda [S][B]); the decisions are taken one problem at a time in
loops that can be checked by eye."""
from __future__ import annotations

import dataclasses

import numpy as np

from oracle import dynamics as D, params as P, qp as Q, scenario as S

BACKOFF_MAX = 6          # back-offs in a row before the problem stops with the QP's status
NU_MIN = 1e-3
ARMIJO = 1e-4
STEPS = tuple(2.0 ** -t for t in range(8))          # a = 1, 1/2, .., 2^-7
UNDECIDED = 1e-9         # a (problem, pass) whose margin is below this is decided by rounding, not by the rule


# ---- the merit function's terms --------------------------------------------------------------------------------------------------------
def merit_terms(cfg, veh, inp, X, U, dU, lam=None, ss_x=None, ss_j=None):
    """-> (J [B], c1 [B], cinf [B]).  J: the QP's cost with the boundary slack eliminated -- tracking terms (none for the learning
    problem, which has ss_j' lambda + sum_k convex_hull_slack[k] eps_k^2, eps = x_T - SS lambda), input and input-rate effort,
    q_boundary sigma*^2 with sigma* the largest boundary violation over all N knots (>= 0).  The constant q_vel vref^2 of the
    tracking cost is left out: only differences of J are used (and the 1e-14 (1 + |phi0|) slack of the Armijo test).
    c1, cinf: the l1 and inf norms of (x_{i+1} - f_d(x_i, u_i, k_i, t_i)) / SCALE_X, f_d following veh.integrator."""
    N = cfg.N
    B = X.shape[2]
    J = np.zeros(B)
    if not cfg.learning:
        q = np.array([0.0, cfg.q_contour, cfg.q_heading, cfg.q_vel, cfg.q_vy, cfg.q_vyaw])
        qT = 10.0 * np.array([0.0, cfg.q_contour, cfg.q_heading, cfg.q_vel, 0.0, 0.0])
        for i in range(N):
            w, wv = (q, cfg.q_vel) if i < N - 1 else (qT, 10.0 * cfg.q_vel)
            for k in range(6):
                J += w[k] * X[k, i] ** 2
            J += -2.0 * wv * inp["vel_ref"][i] * X[3, i]
    for i in range(N - 1):
        for a in range(2):
            for c in range(2):
                J += cfg.R[a, c] * U[a, i] * U[c, i] + cfg.R_d[a, c] * dU[a, i] * dU[c, i]
    if cfg.q_boundary > 0.0:
        marg = cfg.margin + veh.b / 2.0
        sigma = np.zeros(B)
        for i in range(N):
            sigma = np.maximum(sigma, np.maximum(X[1, i] - (inp["bound_left"][i] - marg), (inp["bound_right"][i] + marg) - X[1, i]))
        J += cfg.q_boundary * sigma ** 2
    if cfg.learning:
        for b in range(B):
            eps = X[:, N - 1, b] - ss_x[:, :, b] @ lam[:, b]
            J[b] += ss_j[:, b] @ lam[:, b] + (cfg.convex_hull_slack * eps ** 2).sum()
    nxt = D.rk4(X[:, :-1].transpose(1, 2, 0), U.transpose(1, 2, 0), inp["curvatures"][:-1], inp["T_ref"], veh)      # [N-1][B][6]
    c = np.abs((X[:, 1:].transpose(1, 2, 0) - nxt) / P.SCALE_X)
    return J, c.sum(axis=(0, 2)), c.max(axis=(0, 2))


# ---- the line search of one problem ----------------------------------------------------------------------------------------------------
def line_search(J0: float, c0: float, Ja, ca, nu_prev: float):
    """J0, c0: cost and l1 defect of the iterate; Ja[t], ca[t]: of w + a (w_QP - w) at a = STEPS[t].  -> (a, nu, margin)
    nu = max(nu_prev, [c0 > 0 and dJ > 0] dJ / (0.9 c0), 1e-3), dJ = J(w_QP) - J(w);
    Armijo: phi(a) <= phi0 + 1e-4 a (dJ - nu c0) + 1e-14 (1 + |phi0|), phi = J + nu c1; the last a is taken whatever the test says;
    margin: the smallest |phi(a) - rhs| / (1 + |phi0|) over the step lengths tried -- how far the choice was from falling otherwise."""
    dJ = Ja[0] - J0
    nu = nu_prev
    if c0 > 0.0 and dJ > 0.0:
        nu = max(nu, dJ / (0.9 * c0))
    nu = max(nu, NU_MIN)
    phi0 = J0 + nu * c0
    slope = dJ - nu * c0
    margin = np.inf
    for t, a in enumerate(STEPS):
        rhs = phi0 + ARMIJO * a * slope + 1e-14 * (1.0 + abs(phi0))
        phi = Ja[t] + nu * ca[t]
        margin = min(margin, abs(phi - rhs) / (1.0 + abs(phi0)))
        if phi <= rhs or t == len(STEPS) - 1:
            return a, nu, margin


# ---- one pass --------------------------------------------------------------------------------------------------------------------------
ITERATE = ("X", "U", "dU", "lam")


def initial_state(X_ref, U_ref, n_lam: int = 0) -> dict:
    """The state lmpc_solve_full_dynamics_batch starts from: the iterate (X_ref, U_ref), dU = 0, lambda = 0; nu = 0, no back-offs,
    every problem active, sqp_move = inf, defect = 0, the counters 0."""
    B = X_ref.shape[2]
    st = {"X": np.array(X_ref, dtype=float), "U": np.array(U_ref, dtype=float), "dU": np.zeros_like(U_ref, dtype=float),
          "lam": np.zeros((n_lam, B))}
    for k in ITERATE:
        st[k + "_saved"] = st[k].copy()
    st.update(nu=np.zeros(B), backoffs=np.zeros(B, dtype=int), active=np.ones(B, dtype=bool), status=np.zeros(B, dtype=int),
              sqp_iters=np.zeros(B, dtype=int), iters=np.zeros(B, dtype=int), move=np.full(B, np.inf), defect=np.zeros(B))
    return st


def expected_pass(terms, st: dict, qp: dict, first: bool, step_tol: float, a_given=None):
    """What one pass does to every problem.  terms(X, U, dU, lam) -> (J, c1, cinf) per problem; st: initial_state's dict (not
    modified); qp: this pass's QP solution X, U, dU, lam (same layouts), status [B], iters [B].  a_given [B]: where finite, the step
    length to take instead of the line search's (the GPU test follows the device through a choice that rounding decides).
    -> (the new state, log) with log["branch"] [B] one of "idle", "step", "backoff", "stop", and for a step log["a"], log["margin"].

      first pass                                                the full step
      QP status != 0 on a later pass, < 6 back-offs in a row    the midpoint of the iterate and the iterate before the last step
                                                                taken (X, U, dU, lambda); nu, move and the saved iterate stay
      QP status != 0 on the first pass or after six back-offs   the problem stops, keeps its iterate and that status
      otherwise                                                 w + a (w_QP - w); move = max |X_QP - X| / SCALE_X; inactive once
                                                                move <= step_tol
      every pass in which the problem is active                 sqp_iters += 1, iters += this QP's, status = this QP's
    defect is that of the iterate the pass leaves (a stopped problem keeps what it had: 0 where it never moved)."""
    B = st["X"].shape[2]
    new = {k: np.array(v) for k, v in st.items()}
    log = {"branch": np.array(["idle"] * B, dtype=object), "a": np.full(B, np.nan), "margin": np.full(B, np.nan)}
    # the merit terms at the iterate, at every trial point and at the midpoint, for the whole batch at once (the choices are below)
    at = lambda a: terms(*[st[k] + a * (qp[k] - st[k]) for k in ITERATE])
    J0, c0, _ = terms(*[st[k] for k in ITERATE])
    with np.errstate(all="ignore"):          # (the arrays of a QP that failed hold anything; nothing below reads their trial points)
        trial = [at(a) for a in STEPS]
    mid = [0.5 * (st[k] + st[k + "_saved"]) for k in ITERATE]
    mid_defect = terms(*mid)[2]
    for b in range(B):
        if not st["active"][b]:
            continue
        new["sqp_iters"][b] += 1
        new["iters"][b] += qp["iters"][b]
        new["status"][b] = qp["status"][b]
        if qp["status"][b] != 0:
            if not first and st["backoffs"][b] < BACKOFF_MAX:
                log["branch"][b] = "backoff"
                new["backoffs"][b] += 1
                for k, m in zip(ITERATE, mid):
                    new[k][..., b] = m[..., b]
                new["defect"][b] = mid_defect[b]
            else:
                log["branch"][b] = "stop"
                new["active"][b] = False
            continue
        log["branch"][b] = "step"
        new["backoffs"][b] = 0
        a, margin = 1.0, np.inf
        if not first:
            a, new["nu"][b], margin = line_search(J0[b], c0[b], [t[0][b] for t in trial], [t[1][b] for t in trial], st["nu"][b])
        if a_given is not None and np.isfinite(a_given[b]):
            a = float(a_given[b])
        log["a"][b], log["margin"][b] = a, margin
        for k in ITERATE:
            new[k + "_saved"][..., b] = st[k][..., b]
            new[k][..., b] = st[k][..., b] + a * (qp[k][..., b] - st[k][..., b])
        new["move"][b] = np.abs((qp["X"][..., b] - st["X"][..., b]) / P.SCALE_X[:, None]).max()
        new["defect"][b] = trial[STEPS.index(a)][2][b]
        new["active"][b] = new["move"][b] > step_tol
    return new, log


def run_chain(sample: dict, solve_qp, passes: int, step_tol: float = 1e-9):
    """`passes` passes from the sample's start, the QP about the iterate from solve_qp(inp with X_ref, U_ref := the iterate) ->
    dict with X_optm, U_optm, dU_optm, convex_combi_optm, status, iters.  -> (the final state, [log of each pass])."""
    terms = terms_of(sample)
    st = initial_state(sample["inp"]["X_ref"], sample["inp"]["U_ref"], sample["S"])
    logs = []
    for k in range(passes):
        if not st["active"].any():
            break
        q = solve_qp(dict(sample["inp"], X_ref=st["X"], U_ref=st["U"]))
        st, log = expected_pass(terms, st, qp_of(q, sample["S"]), k == 0, step_tol)
        logs.append(log)
    return st, logs


def qp_of(q: dict, n_lam: int) -> dict:
    B = q["X_optm"].shape[2]
    lam = q.get("convex_combi_optm")
    return {"X": np.asarray(q["X_optm"]), "U": np.asarray(q["U_optm"]), "dU": np.asarray(q["dU_optm"]),
            "lam": np.asarray(lam) if n_lam else np.zeros((0, B)), "status": np.asarray(q["status"]), "iters": np.asarray(q["iters"])}


def terms_of(sample: dict):
    cfg, veh, inp = sample["cfg"], sample["veh"], sample["inp"]
    return lambda X, U, dU, lam: merit_terms(cfg, veh, inp, X, U, dU, lam, sample["ss_x"], sample["ss_j"])


def chain_counts(logs) -> dict:
    """Over passes 2 onwards: (problem, pass) pairs in which a problem was active, those whose step the rule leaves undecided, steps
    with a < 1, back-offs."""
    pairs = undecided = short = backoffs = 0
    for log in logs[1:]:
        step = log["branch"] == "step"
        pairs += int((log["branch"] != "idle").sum())
        undecided += int((step & (log["margin"] < UNDECIDED)).sum())
        short += int((step & (log["a"] < 1.0)).sum())
        backoffs += int((log["branch"] == "backoff").sum())
    return {"pairs": pairs, "undecided": undecided, "short": short, "backoffs": backoffs}


# ---- the samples -----------------------------------------------------------------------------------------------------------------------
# 65 problems: one problem in a second 64-thread block of the line-search kernel.  N = 3 is the smallest horizon the ABI takes, 32
# points the smallest safe set that is instantiated.
B_SAMPLE = 65
TRACKING = {"tracking N = 3": (3, "rk4"), "tracking N = 8": (8, "rk4"), "tracking N = 20": (20, "rk4"), "tracking N = 8, Euler": (8, "euler")}
LEARNING = {"learning (3, 32)": (3, 1, 81), "learning (10, 32)": (10, 1, 80), "learning (10, 96)": (10, 3, 80)}
# The N = 20 tracking sample on a time step that differs per stage and per problem (tests/timestep_cases.py draw_t_ref: 0.0125 .. 0.05,
# problem 0 strictly increasing): t_i is the step of the line search's rollout, of the linearisation and of the rate rows.  The start
# (X_ref, U_ref) stays the rollout at 0.025, so the first iterate has a defect at the steps it is now held to.
NONUNIFORM_T = {"tracking N = 20, non-uniform T_ref": 9320}
TRACKING.update({name: (20, "rk4") for name in NONUNIFORM_T})
SAMPLES = tuple(TRACKING) + tuple(LEARNING)
_cache: dict = {}


def sample(pkg, name: str) -> dict:
    """cfg, veh (oracle side), preset (config, vehicle) for the product's Solver, inp, ss_x [6][S][B], ss_j [S][B], S; built once."""
    if name in _cache:
        return _cache[name]
    if name in TRACKING:
        N, integrator = TRACKING[name]
        cfg, veh = P.barc_tracking_mpc(N), dataclasses.replace(P.barc_vehicle(), integrator=integrator)
        tr = pkg.workloads.synthetic_track("barc")
        u_lo, u_hi, _, _ = Q.effective_bounds(cfg, veh)
        x, u = pkg.workloads.sample_initial_states("barc", B_SAMPLE, tr["L"], u_lo, u_hi, 8)
        inp = S.cold_start_inputs(cfg, veh, tr, x, u, 0.025)
        if name in NONUNIFORM_T:
            from timestep_cases import draw_t_ref

            inp["T_ref"] = draw_t_ref(N, B_SAMPLE, NONUNIFORM_T[name])
        out = dict(cfg=cfg, veh=veh, inp=inp, ss_x=None, ss_j=None, S=0, laps=None,
                   preset=(pkg.presets.barc_tracking_mpc(N), dict(pkg.presets.barc_vehicle(), integrator=integrator)))
    else:
        import lmpc_scenario as LS

        N, n_laps, seed = LEARNING[name]
        veh, cfg, tr, laps, inp, q = LS.make(B_SAMPLE, seed, N=N, n_laps=n_laps)
        ss_x, ss_j, nf = LS.oracle_safe_set(cfg, laps, q)
        assert (nf == cfg.num_ss_pts).all()
        out = dict(cfg=cfg, veh=veh, inp=inp, ss_x=ss_x, ss_j=ss_j, S=int(cfg.num_ss_pts), laps=laps,
                   preset=(pkg.presets.barc_lmpc(N, n_laps), pkg.presets.barc_vehicle()))
    _cache[name] = out
    return out


def twin_qp(sample: dict):
    """The QP about an iterate from the serial C twin (oracle/c)."""
    from oracle import cbind

    return lambda inp: cbind.solve_batch(sample["cfg"], sample["veh"], inp, ss_x=sample["ss_x"], ss_j=sample["ss_j"])
