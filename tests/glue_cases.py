"""Plain references for the small kernels either side of the solve (csrc/lmpc_prep_kernels.hip): the safe-set code arithmetic and
the carry-over of simplex weights (lmpc_shift_lambda_batch), the launch order (lmpc_launch_order_from_iters) and one whole period
between two solves (lmpc_loop_advance_batch).  Written from the contracts in include/lmpc_hip.h, one problem at a time, in loops
that can be checked by eye; tests/test_glue_reference.py pins them on hand-worked cases (no GPU), tests/test_gpu_glue.py holds the
kernels to them.

Codes (csrc/lmpc_ss_kernel.hip): code = (row << 2) | rep, row an index into the laps laid end to end (lap l starts at row off[l],
off = prefix sums of npts), rep 0, 1, 2 the copy of the lap the point is taken from; -1 is "no point"."""
from __future__ import annotations

import numpy as np

from oracle import dynamics as D, scenario as S

NONE = -1
SUPPORT_MIN = 1e-9   # a weight belongs to the support when it is strictly larger
SUPPORT_MAX = 8      # the first eight support entries count
FREE_MAX = 6         # at most six positive entries come out
REF_KEYS = ("X_ref", "U_ref", "T_ref", "bound_left", "bound_right", "curvatures", "vel_ref")


def offsets(npts):
    off, acc = [], 0
    for n in npts:
        off.append(acc)
        acc += int(n)
    return off


def encode(npts, lap: int, sample: int, rep: int) -> int:
    assert 0 <= sample < npts[lap] and 0 <= rep <= 3
    return ((offsets(npts)[lap] + sample) << 2) | rep


def decode(npts, code: int):
    """-> (lap, sample, rep), or None for a code that names no row of the store"""
    if code < 0:
        return None
    row, rep = code >> 2, code & 3
    for lap, (o, n) in enumerate(zip(offsets(npts), npts)):
        if o <= row < o + n:
            return lap, row - o, rep
    return None


def advance_code(npts, code: int, adv: int) -> int:
    """The point `adv` samples further along the same lap; running off the end of a copy continues at the start of the next one."""
    where = decode(npts, int(code))
    if where is None:
        return NONE
    lap, sample, rep = where
    copies, sample = divmod(sample + adv, int(npts[lap]))
    rep += copies
    if rep > 2:
        return NONE
    return encode(npts, lap, sample, rep)


def shift_lambda_one(npts, idx_prev, lam_prev, idx, advance: int, routes=None) -> np.ndarray:
    """One problem: idx_prev [S], lam_prev [S], idx [S] -> lam_ref [S].  `routes` (a list) receives one (weight, t) per support
    entry: t = 0, 1, 2 the candidate that took it (`advance`, 0, `advance` + 1), None where the weight was dropped."""
    support = [(int(idx_prev[i]), lam_prev[i]) for i in range(len(idx_prev)) if lam_prev[i] > SUPPORT_MIN][:SUPPORT_MAX]
    first = {}
    for j, c in enumerate(idx):
        first.setdefault(int(c), j)
    out = np.zeros(len(idx), dtype=np.float64)
    taken = []                              # positions that hold a weight, in the order they got their first one
    for code, lam in support:
        route = None
        for t, adv in enumerate((advance, 0, advance + 1)):
            want = advance_code(npts, code, adv)
            if want == NONE or want not in first:
                continue
            j = first[want]
            if j not in taken:
                if len(taken) == FREE_MAX:
                    continue
                taken.append(j)
            out[j] = out[j] + lam
            route = t
            break
        if routes is not None:
            routes.append((float(lam), route))
    return out


def shift_lambda(npts, idx_prev, lam_prev, idx, advance: int, routes=None) -> np.ndarray:
    """[S][B] arrays, batch axis last"""
    out = np.zeros(idx.shape, dtype=np.float64)
    for b in range(idx.shape[1]):
        out[:, b] = shift_lambda_one(npts, idx_prev[:, b], lam_prev[:, b], idx[:, b], advance, routes)
    return out


def launch_order(iters) -> np.ndarray:
    """Longest job first over iteration counts clipped to 0 .. 63, ties by problem index"""
    return np.argsort(-np.clip(np.asarray(iters, dtype=np.int64), 0, 63), kind="stable").astype(np.int32)


def loop_advance(cfg, veh, track, inp: dict, sol: dict, x, dt: float, dt_sim: float, n_sub: int, speed_scale: float,
                 restart_failed: bool) -> dict:
    """One period between two solves, from the oracle's restatements of the node and the simulator (oracle/scenario.py).
    inp: the period's inputs (REF_KEYS, batch axis last), sol: X_optm [6][N][B], U_optm [2][N-1][B], status [B]; x [6][B].
    -> "u" [2][B] the input applied, "x" [6][B] the new state, REF_KEYS the next period's inputs, "distance" [B] the abscissa
    travelled, "excess" [B] the excursion beyond the track edge, "fail" [B] 0 / 1, and "restarted" [B] the cars whose inputs are a
    cold start (their rollouts are to be compared knot by knot: tests/test_gpu_path.py test_prepare_matches_node_cold_start)."""
    L = float(track["L"])
    ok = np.asarray(sol["status"]) == 0
    u = np.where(ok[None, :], sol["U_optm"][:, 0, :], inp["U_ref"][:, 0, :])
    x_new = S.plant_step(veh, track, np.asarray(x).T, u.T, dt_sim, n_sub).T
    plan_X = np.where(ok[None, None, :], sol["X_optm"], inp["X_ref"])
    plan_U = np.where(ok[None, None, :], sol["U_optm"], inp["U_ref"])
    nxt = S.shift_inputs(cfg, veh, track, plan_X, plan_U, dt, speed_scale=speed_scale)
    restarted = ~ok if restart_failed else np.zeros_like(ok)
    if restarted.any():
        B = ok.size
        cold = S.cold_start_inputs(cfg, veh, track, x_new.T, np.zeros((B, 2)), dt, speed_scale=speed_scale)
        for k in REF_KEYS:
            nxt[k][..., restarted] = cold[k][..., restarted]
    ds = x_new[0] - np.asarray(x)[0]
    half_b = float(veh.b) / 2.0
    out = {k: nxt[k] for k in REF_KEYS}
    out.update(u=u, x=x_new, restarted=restarted, fail=(~ok).astype(np.int64),
               distance=np.where(ds < -L / 2.0, ds + L, ds),
               excess=np.maximum(x_new[1] + half_b - inp["bound_left"][0], inp["bound_right"][0] - (x_new[1] - half_b)))
    return out


def cold_rollout_errors(cfg, veh, track, got: dict, cars, dt: float, speed_scale: float) -> dict:
    """A cold start's arrays for the cars `cars`, each knot from the knot before it AS GIVEN (the model's step is unstable at low
    speed: two correctly rounded rollouts part over a horizon) and each sampled reference at the knot's own abscissa.
    -> the largest |difference| per array, relative to max(1, largest reference magnitude)."""
    L, N = float(track["L"]), cfg.N
    X = got["X_ref"][:, :, cars]
    n = X.shape[2]
    err = {"X_ref": 0.0}
    for i in range(N - 1):
        k = S.track_lookup(track["curvature"], X[0, i], L)
        step = D.rk4(X[:, i].T, np.full((n, 2), 1e-9), k, dt, veh).T
        err["X_ref"] = max(err["X_ref"], np.abs(step - X[:, i + 1]).max() / max(1.0, np.abs(step).max()))
    want = dict(zip(("bound_left", "bound_right", "curvatures", "vel_ref"),
                    S._sample_refs(cfg, track, X.transpose(1, 2, 0), speed_scale, float(cfg.x_max[3]))))
    for k, w in want.items():
        err[k] = np.abs(got[k][:, cars] - w).max() / max(1.0, np.abs(w).max())
    return err
