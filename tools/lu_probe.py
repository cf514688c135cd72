#!/usr/bin/env python3
"""
LU factor against the symmetric one on the C3 matrix (1 M dofs, BucklingColumn(706, 706)): device time of the numeric
phase (refactor_device from values already on the device: no host work, no upload), host time of the symmetrised
pattern an LU factor is given, device bytes, sweep time at 4 and 32 columns, and the residual of a refined LU solve.  The LU factor is made on K itself (symmetric=
False) and on an unsymmetric perturbation of K on the same pattern (K + 0.3 (tril(K, -1) - triu(K, 1))).
Then, per LU factor, the transposed solve: its first call (which allocates and fills the U side's forward copies)
against a later one, device bytes after it, transposed and forward sweeps alternating at 4 and 32 columns, the numeric
phase with the copies to fill, and the residual of a refined transposed solve.
    python tools/lu_probe.py          (REPS = numeric phases timed per factor, default 3; ROWS = comma list of
                                       cholesky, luK, unsym: the factors to run, default all)
"""
import os
import sys
import time

import numpy as np
from scipy import sparse

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eigd_amd.device import CSRMatrix, Factor, default_context, symmetrised_pattern  # noqa: E402
from eigd_amd.problems import BucklingColumn  # noqa: E402

ctx = default_context()
col = BucklingColumn(706, 706, seed=0)
K = col.stiffness().tocsr()
K.sort_indices()
U = (K + 0.3 * (sparse.tril(K, -1) - sparse.triu(K, 1))).tocsr()
U.sort_indices()
reps = int(os.environ.get("REPS", "3"))
n = K.shape[0]
rng = np.random.default_rng(0)


def timed(fn, count):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    ctx.sync()
    return 1e3 * (time.perf_counter() - t0) / count


base = Factor(ctx, K, coords=col.dof_coords())
sym = base.symbolic
rows = []
wanted = os.environ.get("ROWS", "cholesky,luK,unsym").split(",")
for key, name, mat, lu in (("cholesky", "cholesky K", K, False), ("luK", "lu K", K, True), ("unsym", "lu unsym", U, True)):
    if key not in wanted:
        continue
    F = base if not lu else Factor(ctx, mat, symbolic=sym, lu=True)
    t0 = time.perf_counter()
    vals = symmetrised_pattern(mat) if lu else mat
    t_host = 1e3 * (time.perf_counter() - t0)
    dvals = ctx.from_host(np.ascontiguousarray(vals.data).reshape(-1, 1))
    F.refactor_device(dvals)  # (warm-up)
    t_num = timed(lambda: F.refactor_device(dvals), reps)
    st = F.stats()
    sweeps = {}
    for k in (4, 32):
        B = ctx.from_host(rng.normal(size=(n, k)))
        X = ctx.empty(n, k)
        for _ in range(3):
            F.solve_to(B, X)
        sweeps[k] = timed(lambda: F.solve_to(B, X), 20)
    B = ctx.from_host(rng.normal(size=(n, 1)))
    X = F.solve_to(B, ctx.empty(n, 1))
    if lu:
        F.refine(CSRMatrix(ctx, mat), B, X, steps=1)
    r = np.linalg.norm(mat @ X.get() - B.get()) / np.linalg.norm(B.get())
    rows.append(name)
    print(f"{name:12s} numeric (device) {t_num:8.1f} ms  host symmetrise {t_host:7.1f} ms  bytes {st['device_bytes'] / 2**30:6.2f} GiB  sweep k=4 {sweeps[4]:7.3f} ms  "
          f"k=32 {sweeps[32]:7.3f} ms  interchanges {st['row_interchanges']}  static {st['static_pivots']}  "
          f"resid {r:.1e}", flush=True)
    if lu:
        B4, X4 = ctx.from_host(rng.normal(size=(n, 4))), ctx.empty(n, 4)
        t_first = timed(lambda: F.solve_to(B4, X4, trans=True), 1)
        st_t = F.stats()
        fwd_t, trn_t = {}, {}
        for k in (4, 32):
            B, X = ctx.from_host(rng.normal(size=(n, k))), ctx.empty(n, k)
            for _ in range(3):
                F.solve_to(B, X, trans=True)
            f_runs, t_runs = [], []
            for _ in range(3):  # alternating
                t_runs.append(timed(lambda: F.solve_to(B, X, trans=True), 20))
                f_runs.append(timed(lambda: F.solve_to(B, X), 20))
            fwd_t[k], trn_t[k] = sorted(f_runs)[1], sorted(t_runs)[1]
        t_num_t = timed(lambda: F.refactor_device(dvals), reps)
        B = ctx.from_host(rng.normal(size=(n, 1)))
        X = F.solve_to(B, ctx.empty(n, 1), trans=True)
        F.refine(CSRMatrix(ctx, mat), B, X, steps=1, trans=True)
        rt = np.linalg.norm(mat.T @ X.get() - B.get()) / np.linalg.norm(B.get())
        print(f"{name:12s} transposed: first solve {t_first:8.1f} ms  bytes {st_t['device_bytes'] / 2**30:6.2f} GiB  "
              f"sweep k=4 {trn_t[4]:7.3f} ms (forward after {fwd_t[4]:7.3f})  k=32 {trn_t[32]:7.3f} ms (forward after "
              f"{fwd_t[32]:7.3f})  numeric with the copies {t_num_t:8.1f} ms  resid {rt:.1e}", flush=True)
    if F is not base:
        del F
