"""Tracks, poses and the independent projection oracle of tests/test_track_spline.py and tests/test_gpu_track.py.

Two tracks: the reference's BARC track (tests/golden/barc_track/15_barc_optm.txt, 153 waypoints, L = 15.63 m) and a synthetic
2.4 km one with 1400 unevenly spaced waypoints, built here from a seed.  The oracle of the projection is independent of the code
under test: scipy's splines (oracle.trajectory.TrackOracle) and scipy's brentq on the first-order condition (r(s) - p) . r'(s) = 0
within half a median waypoint spacing of the abscissa the pose was generated from."""
from pathlib import Path

import numpy as np

BARC = Path(__file__).resolve().parent / "golden" / "barc_track" / "15_barc_optm.txt"

# the project's tolerances for the C++ track class (tests/test_racing_trajectory.py), against the scipy restatement
TOL_EVAL = {"x": 1e-10, "y": 1e-10, "vel": 1e-9, "left": 1e-10, "right": 1e-10, "yaw": 1e-8, "curvature": 1e-7}
TOL_TABLE = 1e-8
TOL_S, TOL_T, TOL_XI = 1e-9, 1e-9, 1e-8   # projection: a position error of 1e-10 over 1 - kappa t >= 0.6 stays below 1e-9


def synthetic_table() -> np.ndarray:
    """R(th) = 400 + 120 cos 2 th + 35 sin 3 th, x = R cos th, y = 0.6 R sin th at 1400 sorted th ~ U(0, 2 pi) (default_rng(3), th_0 = 0);
    abscissa along a 400 001-point polyline (L ~ 2416.09); left edge 7 + 2 sin 5 th along the left normal, right edge 0.8 of that."""
    def curve(th):
        R = 400.0 + 120.0 * np.cos(2 * th) + 35.0 * np.sin(3 * th)
        return R * np.cos(th), 0.6 * R * np.sin(th)

    th = np.sort(np.random.default_rng(3).uniform(0.0, 2 * np.pi, 1400))
    th[0] = 0.0
    fine = np.linspace(0.0, 2 * np.pi, 400001)
    fx, fy = curve(fine)
    arc = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(fx), np.diff(fy)))])
    x, y = curve(th)
    R = 400.0 + 120.0 * np.cos(2 * th) + 35.0 * np.sin(3 * th)
    dR = -240.0 * np.sin(2 * th) + 105.0 * np.cos(3 * th)
    tx, ty = dR * np.cos(th) - R * np.sin(th), 0.6 * (dR * np.sin(th) + R * np.cos(th))
    nrm = np.hypot(tx, ty)
    nx, ny = -ty / nrm, tx / nrm                       # left normal (the curve runs counter-clockwise)
    w = 7.0 + 2.0 * np.sin(5 * th)
    tab = np.zeros((1400, 17))
    tab[:, 0], tab[:, 1] = x, y
    tab[:, 4] = 40.0 + 10.0 * np.cos(3 * th)           # SPEED
    tab[:, 6] = np.interp(th, fine, arc)               # DIST_TO_SF_BWD
    tab[:, 7] = arc[-1]                                # DIST_TO_SF_FWD (row 0: the lap length)
    tab[:, 9], tab[:, 10] = x + w * nx, y + w * ny
    tab[:, 11], tab[:, 12] = x - 0.8 * w * nx, y - 0.8 * w * ny
    return tab


def table(name: str) -> np.ndarray:
    return np.loadtxt(BARC) if name == "barc" else synthetic_table()


def eval_spline_track(d: dict, s) -> dict:
    """to_spline_track()'s arrays evaluated in numpy as the device evaluates them: wrapped abscissa, last piece whose left break is
    <= it, Horner."""
    L = d["L"]
    s = np.asarray(s, dtype=np.float64)
    k = np.abs(L / 2.0 - s) + L / 2.0
    sm = s + (k - np.fmod(k, L)) * np.sign(L / 2.0 - s)
    P = d["breaks"].size - 1
    i = np.clip(np.searchsorted(d["breaks"], sm, side="right") - 1, 0, P - 1)
    h = sm - d["breaks"][i]
    a, b, c, e = (d["coef"][:, i, j] for j in range(4))
    val = a + h * (b + h * (c + h * e))
    d1 = b + h * (2.0 * c + 3.0 * h * e)
    d2 = 2.0 * c + 6.0 * h * e
    dx, dy, d2x, d2y = d1[0], d1[1], d2[0], d2[1]
    return {"x": val[0], "y": val[1], "vel": val[2], "left": val[3], "right": val[4], "yaw": np.arctan2(dy, dx),
            "curvature": dx * d2y - dy * d2x / np.sqrt((dx ** 2 + dy ** 2) ** 3)}


def poses(tr, n: int = 20000, seed: int = 11):
    """s ~ U(0, L), t = u bound(s) with u ~ U(-0.9, 0.9), xi ~ U(-0.5, 0.5), taken to the global frame by the host class.
    Returns (frenet [3][n], pose [3][n], min over the poses of 1 - kappa t)."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.0, tr.total_length, n)
    u = rng.uniform(-0.9, 0.9, n)
    xi = rng.uniform(-0.5, 0.5, n)
    t = np.where(u >= 0.0, u * tr.left_boundary(s), -u * tr.right_boundary(s))
    x, y, phi = tr.frenet_to_global(s, t, xi)
    return np.stack([s, t, xi]), np.stack([x, y, phi]), float((1.0 - tr.curvature(s) * t).min())


def oracle_projection(orc, pose, s_gen, h_bar: float):
    """(s, t, xi) of every pose by the independent route: brentq root of (r - p) . r' within +- h_bar / 2 of s_gen on the oracle's own
    splines (evaluated at the wrapped abscissa, as every interpolant is), then t and xi from the definitions."""
    from scipy.optimize import brentq

    out = np.empty((3, pose.shape[1]))
    for b in range(pose.shape[1]):
        px, py, phi = pose[:, b]

        def g(sv):
            sm = float(orc.mod(sv))
            return (orc.sx(sm) - px) * orc.sx(sm, 1) + (orc.sy(sm) - py) * orc.sy(sm, 1)

        root = brentq(g, s_gen[b] - h_bar / 2.0, s_gen[b] + h_bar / 2.0, xtol=1e-13, rtol=1e-15, maxiter=200)
        sm = float(orc.mod(root))
        xo, yo, yaw = float(orc.sx(sm)), float(orc.sy(sm)), float(np.arctan2(orc.sy(sm, 1), orc.sx(sm, 1)))
        sign = np.sign(np.cos(yaw) * (py - yo) - np.sin(yaw) * (px - xo))
        d = phi - yaw
        out[:, b] = sm, np.hypot(px - xo, py - yo) * sign, np.arctan2(np.sin(d), np.cos(d))
    return out


def wrap_diff(a, b, L: float):
    """a - b on the circle of length L (the projection returns its abscissa in [0, L])."""
    return (np.asarray(a) - np.asarray(b) + L / 2.0) % L - L / 2.0
