"""The per-row error-dynamics regression's surface and its tests' reference, checked without a GPU: capi.py's struct is the
header's, the library exports the two entry points and include/lmpc_hip_rows.h declares them (tests/test_abi.py holds
include/lmpc_hip.h, which includes it, to pedantic C11), Solver takes rows=, and regression_rows_cases.rows_reference -- what the GPU tests hold the kernels to -- is a direct solve of
each row's own normal equations."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import params as P, regression as R
from regression_rows_cases import ROWS_245, ROWS_444, ROWS_555, rows_reference
from test_regression_oracle import synthetic_lap

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = ("lmpc_set_regression_laps_rows", "lmpc_fleet_ss_set_regression_rows")


def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "lmpc_hip_rows.h").read_text(), flags=re.S)


def test_rows_spec_struct_has_the_headers_fields_in_order_and_its_size(pkg):
    body = re.search(r"typedef struct lmpc_regression_rows_spec \{(.*?)\} lmpc_regression_rows_spec;", _header(), flags=re.S).group(1)
    fields = re.findall(r"(int32_t|double)\s+(\w+)((?:\[\d+\])*)\s*;", body)
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    declared = []
    for typ, name, dims in fields:
        t = ctype[typ]
        for d in reversed(re.findall(r"\[(\d+)\]", dims)):
            t = t * int(d)
        declared.append((name, C.sizeof(t)))
    spec = pkg.capi.CRegressionRowsSpec
    assert [(n, C.sizeof(t)) for n, t in spec._fields_] == declared
    assert [n for n, _ in declared] == ["n_out", "out", "n_in_state", "in_state", "n_in_ctrl", "in_ctrl", "as_written", "dist_max"]
    # 1 + 6 + 6 + 36 + 6 + 12 + 1 = 68 int32, then the double on its 8-byte boundary
    assert C.sizeof(spec) == 68 * 4 + 8 and spec.dist_max.offset == 68 * 4 and spec.in_state.offset == 13 * 4 and spec.in_ctrl.offset == 55 * 4
    s = pkg.capi._rows_spec({5: ((2, 3), (1,)), 3: ((4,), ())}, 0.5, True)       # insertion order, row-major lists
    assert (s.n_out, list(s.out)[:2], list(s.n_in_state)[:2], list(s.n_in_ctrl)[:2]) == (2, [5, 3], [2, 1], [1, 0])
    assert list(s.in_state[0])[:2] == [2, 3] and s.in_state[1][0] == 4 and s.in_ctrl[0][0] == 1 and s.as_written == 1 and s.dist_max == 0.5


def test_rows_entry_points_are_exported_declared_and_mirrored(pkg):
    lib = pkg.load_library()
    declared = set(re.findall(r"\b(lmpc_[a-z_0-9]+)\s*\(", _header()))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in declared, name
    assert lib.lmpc_set_regression_laps_rows(None, C.c_int32(0), None, None, None, None, None, None) == -1      # a null handle
    assert lib.lmpc_fleet_ss_set_regression_rows(None, None) == -1
    for method in (pkg.Solver.set_regression_laps, pkg.Solver.fleet_ss_set_regression):
        assert inspect.signature(method).parameters["rows"].default is None


@pytest.mark.parametrize("as_written", [False, True])
@pytest.mark.parametrize("rows", [ROWS_444, ROWS_245, ROWS_555], ids=["444", "245", "555"])
def test_the_row_composition_solves_each_rows_own_normal_equations(rows, as_written):
    veh = P.barc_vehicle()
    laps = [synthetic_lap(veh, 40, 70 + l) for l in range(2)]
    rng = np.random.default_rng(1)
    h, n = 0.6, 5
    xs, us = np.concatenate([l[0][:-1] for l in laps]), np.concatenate([l[1][:-1] for l in laps])
    pick = rng.integers(0, xs.shape[0], n)
    qx, qu = xs[pick] + 0.01 * rng.normal(size=(n, 6)), us[pick].copy()
    qx[-1, 2] += 10.0       # out of reach for the one row that lists the heading error, and only for it
    A0, B0, g0 = rng.normal(size=(n, 6, 6)), rng.normal(size=(n, 6, 2)), rng.normal(size=(n, 6))
    A, B, g, touched = rows_reference(veh, laps, rows, h, qx, qu, A0, B0, g0, as_written=as_written)
    Y = np.concatenate([R.lap_residuals(veh, *l, as_written=as_written) for l in laps])
    may_A, may_B, may_g = np.zeros(A.shape, bool), np.zeros(B.shape, bool), np.zeros(g.shape, bool)
    for o, (r, (ins, inc)) in enumerate(rows.items()):
        ins, inc = list(ins), list(inc)
        Z = np.concatenate([xs[:, ins], us[:, inc]], axis=1)
        for i in range(n):
            d = np.linalg.norm(Z - np.concatenate([qx[i, ins], qu[i, inc]]), axis=1)
            m = d < h
            assert touched[o, i] == m.any()
            if not m.any():
                continue
            K = 0.75 / h * (1 - (d[m] / h) ** 2) ** 2
            M = np.concatenate([Z[m], np.ones((m.sum(), 1))], axis=1)
            Rr = np.linalg.solve((M.T * K) @ M + 1e-3 * np.eye(M.shape[1]), (-1.0 if as_written else 1.0) * (M.T * K) @ Y[m, r])
            ns = len(ins)
            assert np.allclose(A[i, r, ins] - A0[i, r, ins], Rr[:ns], rtol=1e-9, atol=1e-12)
            assert np.allclose(B[i, r, inc] - B0[i, r, inc], Rr[ns:-1], rtol=1e-9, atol=1e-12)
            assert np.isclose(g[i, r] - g0[i, r], Rr[-1], rtol=1e-9, atol=1e-12)
            may_A[i, r, ins], may_B[i, r, inc], may_g[i, r] = True, True, True
    assert touched[:, :-1].all() and touched[:, -1].sum() == len(rows) - (1 if rows is ROWS_245 else 0)
    # everything else has the bits it came with
    assert np.array_equal(A[~may_A], A0[~may_A]) and np.array_equal(B[~may_B], B0[~may_B]) and np.array_equal(g[~may_g], g0[~may_g])
