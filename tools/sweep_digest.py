#!/usr/bin/env python3
"""
SHA-256 of sweep results over grid matrices, widths 1..32, Cholesky, Bunch-Kaufman and LU factors, before and after a
numeric refactorisation, on the factor's own stream and through a sweep lane (a block on a second context) -- bitwise
comparison of two builds of the library (EIGD_LIB selects the shared object):
    python tools/sweep_digest.py ; EIGD_LIB=build/r3/libeigd_hip.so python tools/sweep_digest.py
"""
import hashlib
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_symbolic_cpu import grid_matrix  # noqa: E402
from eigd_amd.device import Factor, default_context  # noqa: E402


def unsymmetric(nx, ny, dof, seed):
    """a grid matrix made numerically unsymmetric, plus one-directional couplings (structurally unsymmetric)"""
    rng = np.random.default_rng(seed)
    A = grid_matrix(nx, ny, dof, seed)
    A = A + 0.3 * (sp.tril(A, -1) - sp.triu(A, 1))
    n = A.shape[0]
    r = rng.integers(0, n - 3 * nx * dof, size=n // 4)
    c = r + rng.integers(nx * dof, 3 * nx * dof, size=r.size)
    return (A + sp.csr_matrix((rng.uniform(-0.5, 0.5, size=r.size), (r, c)), shape=(n, n))).tocsr()


ctx = default_context()
other = ctx.fork(1)
rng = np.random.default_rng(0)
h = hashlib.sha256()
for (nx, ny, dof, seed, leaf, shift, lu) in ((150, 140, 2, 4, 0, 0.0, False), (90, 95, 3, 5, 50, 0.0, False),
                                             (201, 77, 1, 6, 37, 0.0, False), (120, 110, 2, 7, 0, 8.0, False),
                                             (130, 120, 2, 8, 0, 0.0, True)):
    A = unsymmetric(nx, ny, dof, seed) if lu else grid_matrix(nx, ny, dof, seed)
    if shift:  # interior shift: the Bunch-Kaufman path
        A = (A - shift * sp.identity(A.shape[0])).tocsr()
    F = Factor(ctx, A, leaf_size=leaf, lu=lu)
    tol = 1e-7 if (shift or lu) else 1e-11
    for rep in range(2):
        for k in (1, 4, 7, 9, 16, 21, 32):
            B = rng.normal(size=(A.shape[0], k))
            X = F.solve_inplace(ctx.from_host(B)).get()
            r = np.linalg.norm(A @ X - B) / np.linalg.norm(B)
            assert r < tol, (nx, k, r)
            h.update(X.tobytes())
        for k in (4, 32):  # through a lane: the sweep workspace of another stream
            B = rng.normal(size=(A.shape[0], k))
            Xo = other.empty(A.shape[0], k)
            F.solve_to(other.from_host(B), Xo)
            other.sync()
            X = Xo.get()
            r = np.linalg.norm(A @ X - B) / np.linalg.norm(B)
            assert r < tol, (nx, "lane", k, r)
            h.update(X.tobytes())
        if lu:  # same pattern, new values
            A = A.copy()
            A.data = A.data * np.random.default_rng(seed + 10).uniform(0.9, 1.1, size=A.nnz)
        else:
            A = (A + 0.25 * grid_matrix(nx, ny, dof, seed + 10)).tocsr()
        F.refactor(A)
    st = F.stats()
    print(nx, ny, dof, st["kind"], "negative pivots", st["negative_pivots"], "static", st["static_pivots"],
          "interchanges", st["row_interchanges"], h.hexdigest()[:16], flush=True)
print("digest", h.hexdigest())
