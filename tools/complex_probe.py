#!/usr/bin/env python3
"""
The real-equivalent factors of a complex matrix against the real LU factor, on the C3 pattern (1 M dofs,
BucklingColumn(706, 706)) with damped-dynamic-stiffness values K - w^2 M + i w C (M = the diagonal of K scaled, C = a K +
b M: complex symmetric): device time of the numeric phase (refactor_device from values on the device), device bytes and
sweep times at 4 and 32 columns of the LU form, the symmetric form and the real LU factor of Re(mat); then the complex
product on split-layout blocks against the real SpMM on the real-equivalent matrix of order 2n, at 4 and 32 columns.
    python tools/complex_probe.py     (SIDE = elements per side, default 706; REPS = numeric phases timed, default 3)
"""
import os
import sys
import time

import numpy as np
from scipy import sparse

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eigd_amd.device import (ComplexCSRMatrix, CSRMatrix, Factor, default_context, real_equivalent)  # noqa: E402
from eigd_amd.problems import BucklingColumn  # noqa: E402

ctx = default_context()
side = int(os.environ.get("SIDE", "706"))
reps = int(os.environ.get("REPS", "3"))
col = BucklingColumn(side, side, seed=0)
K = col.stiffness().tocsr()
K.sort_indices()
n = K.shape[0]
Md = sparse.diags(K.diagonal() / K.diagonal().max()).tocsr()
w2 = 0.37 * K.diagonal().min()
mat = (K - w2 * Md + 1j * np.sqrt(w2) * (0.05 * K + 0.02 * Md)).tocsr()
mat.sort_indices()
rng = np.random.default_rng(0)
coords = col.dof_coords()


def timed(fn, count):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    ctx.sync()
    return 1e3 * (time.perf_counter() - t0) / count


print(f"n = {n}  nnz = {mat.nnz}", flush=True)
for name, A, lu, xy in (("real lu", mat.real.tocsr(), True, coords),
                        ("complex, lu form", real_equivalent(mat, "lu"), True, np.repeat(coords, 2, axis=0)),
                        ("complex, symmetric form", real_equivalent(mat, "symmetric"), False, np.repeat(coords, 2, axis=0))):
    t0 = time.perf_counter()
    F = Factor(ctx, A, coords=xy, lu=lu)
    ctx.sync()
    t_first = 1e3 * (time.perf_counter() - t0)
    dvals = ctx.from_host(np.ascontiguousarray(A.data).reshape(-1, 1))
    F.refactor_device(dvals)
    t_num = timed(lambda: F.refactor_device(dvals), reps)
    st = F.stats()
    sweeps = {}
    for k in (4, 32):
        B, X = ctx.from_host(rng.normal(size=(A.shape[0], k))), ctx.empty(A.shape[0], k)
        for _ in range(3):
            F.solve_to(B, X)
        sweeps[k] = timed(lambda: F.solve_to(B, X), 10)
    print(f"{name:24s} order {A.shape[0]:8d}  analysis + first numeric {t_first:9.1f} ms  numeric (device) {t_num:8.1f} ms  "
          f"bytes {st['device_bytes'] / 2**30:6.2f} GiB  sweep k=4 {sweeps[4]:8.3f} ms  k=32 {sweeps[32]:8.3f} ms  "
          f"kind {st['kind']}  static {st['static_pivots']}  interchanges {st['row_interchanges']}", flush=True)
    del F

Ad, Rd = ComplexCSRMatrix(ctx, mat), CSRMatrix(ctx, real_equivalent(mat, "lu"))
for k in (4, 32):
    Z, Y = ctx.from_host(rng.normal(size=(n, 2 * k))), ctx.empty(n, 2 * k)
    V, W = ctx.from_host(rng.normal(size=(2 * n, k))), ctx.empty(2 * n, k)
    for _ in range(3):
        Ad.apply(Z, Y)
        Rd.apply(V, W)
    tc, tr = timed(lambda: Ad.apply(Z, Y), 20), timed(lambda: Rd.apply(V, W), 20)
    print(f"product k={k:2d}: complex on split layout {tc:7.3f} ms ({Ad.spmm_bytes(k) / tc / 1e6:7.1f} GB/s algorithmic)  "
          f"real SpMM on the order-2n matrix {tr:7.3f} ms", flush=True)
