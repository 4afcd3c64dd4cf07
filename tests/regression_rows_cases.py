"""What the tests of the per-row error-dynamics regression (lmpc_set_regression_laps_rows / lmpc_fleet_ss_set_regression_rows) share:
their reference and their queries.  No GPU is needed to import or call any of it.

THE REFERENCE.  The rows of the ridge regression are independent, so the answer for a spec {r: (S_r, C_r), ...} is the one-list oracle
applied row after row: oracle.regression.regress_batch(..., S_r, C_r, out_rows=(r,), ...) onto the running (A, B, g).  Each call
touches only A[r, S_r], B[r, C_r] and g[r], so the order of the rows does not matter and nothing is added twice
(tests/test_regression_rows_reference.py holds this composition to a direct solve of each row's normal equations)."""
import numpy as np

from oracle import regression as R

# the lists of the LMPC racing literature: the longitudinal row on the speeds and the longitudinal input, the lateral and yaw rows on
# the speeds and the steering angle
ROWS_444 = {3: ((3, 4, 5), (0,)), 4: ((3, 4, 5), (1,)), 5: ((3, 4, 5), (1,))}
# 2, 4 and 5 features; only the yaw-rate row lists the heading error (state 2)
ROWS_245 = {3: ((3,), (0,)), 4: ((3, 4, 5), (1,)), 5: ((2, 3, 4, 5), (1,))}
# the one-list bench spec, row by row
ROWS_555 = {3: ((3, 4, 5), (0, 1)), 4: ((3, 4, 5), (0, 1)), 5: ((3, 4, 5), (0, 1))}


def rows_reference(veh, laps, rows, dist_max, qx, qu, A, B, g, as_written=False):
    """qx [n, 6], qu [n, 2], A [n, 6, 6], B [n, 6, 2], g [n, 6] -> updated copies and touched [len(rows), n] (row o of the spec had a
    candidate at query n; where it had none the row's entries are returned bit-identical)."""
    touched = []
    for r, (ins, inc) in rows.items():
        A, B, g, t = R.regress_batch(veh, laps, ins, inc, (r,), dist_max, qx, qu, A, B, g, as_written=as_written)
        touched.append(t)
    return A, B, g, np.stack(touched)


def flat(a):
    """[..., N-1, B] -> [B (N-1), ...], query (b, i) at b (N-1) + i"""
    a = np.asarray(a)
    return np.ascontiguousarray(np.moveaxis(a, (-1, -2), (0, 1)).reshape(a.shape[-1] * a.shape[-2], *a.shape[:-2]))


def queries_on_samples(laps, N, B, seed, noise=0.05):
    """Linearisation points for B problems of N knots, each stage next to a recorded sample that has a successor (its state, input
    and curvature plus noise of `noise` standard deviations of the synthetic laps' spread), so that every bandwidth of a few tenths
    holds samples.  Returns what Solver.linearize / Solver.regress take: X_ref [6, N, B], U_ref [2, N-1, B], T_ref, curvatures."""
    rng = np.random.default_rng(seed)
    xs = np.concatenate([l[0][:-1] for l in laps])
    us = np.concatenate([l[1][:-1] for l in laps])
    ks = np.concatenate([l[2][:-1] for l in laps])
    j = rng.integers(0, xs.shape[0], (N, B))
    X = xs[j] + noise * rng.normal(0, 1, (N, B, 6)) * np.array([0.5, 0.05, 0.05, 0.3, 0.05, 0.3])
    U = us[j[:N - 1]] + noise * rng.normal(0, 1, (N - 1, B, 2)) * np.array([0.005, 0.1])
    return {"X_ref": np.ascontiguousarray(X.transpose(2, 0, 1)), "U_ref": np.ascontiguousarray(U.transpose(2, 0, 1)),
            "T_ref": np.full((N - 1, B), 0.03), "curvatures": np.ascontiguousarray(ks[j])}


def rel_err(got, ref):
    """per query: max |got - ref| / (1 + max |ref|)"""
    n = ref.shape[0]
    return np.abs(got - ref).reshape(n, -1).max(axis=1) / (1 + np.abs(ref).reshape(n, -1).max(axis=1))


def row_masks(rows):
    """Per row of the spec: boolean masks of the entries of A [6, 6], B [6, 2] and g [6] that row may change."""
    out = []
    for r, (ins, inc) in rows.items():
        mA, mB, mg = np.zeros((6, 6), bool), np.zeros((6, 2), bool), np.zeros(6, bool)
        mA[r, list(ins)] = True
        mB[r, list(inc)] = True
        mg[r] = True
        out.append((mA, mB, mg))
    return out
