#!/usr/bin/env python3
"""
SHA-256 per case of what BasicLanczos.solve leaves behind -- lam0, Phi, alpha, beta, T, Y, indices, eig_res, m, N,
n_extra, factor.count -- and of psi from solve_adjoint(method="sibk") and (method="dl") on the real cases: bitwise
comparison of two versions of the Python host layer over ONE build of the library.  Public API only, and the package is
taken from PYTHONPATH where that names one, so the same file runs against a checkout of another commit:

    python tools/lanczos_digest.py > new.txt
    PYTHONPATH=/path/to/worktree-of-the-other-commit EIGD_LIB=$PWD/eigd_amd/lib/libeigd_hip.so \
        python tools/lanczos_digest.py > old.txt ; diff old.txt new.txt

Cases: the n = 900 (G4) and thermal (G3, a numerically repeated pair) fixtures, real, over full / selective
orthogonalisation and Ntarget None / 2, tol = 1e-12; the G1 buckling fixture; the complex-step fixture G6 with full
(tol = 0) and selective (tol = 1e-12) orthogonalisation.

    python tools/lanczos_digest.py --time

prints instead the wall-clock time of solve() on the G4 pencil and on G6 (m = 60): five repeats each, all of them and
their median.
"""
import hashlib
import os
import sys
import time
import warnings

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)                     # (behind PYTHONPATH: another checkout named there wins)
import eigd_amd as eg  # noqa: E402
from eigd_amd.device import default_context  # noqa: E402


def digest(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes() if isinstance(p, np.ndarray) else repr(p).encode())
    return h.hexdigest()[:16]


def golden(name):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))


def csr(g, prefix, parts=("_data",)):
    data = g[prefix + parts[0]] if len(parts) == 1 else g[prefix + parts[0]] + 1j * g[prefix + parts[1]]
    return sparse.csr_matrix((data, g[prefix + "_indices"], g[prefix + "_indptr"]),
                             shape=tuple(int(v) for v in g[prefix + "_shape"]))


def solve(A, B, fac, sigma, **kw):
    s = eg.BasicLanczos(**kw)
    fac.count = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s.solve(A, B, fac, sigma)
    return s


def report(name, s, fac, adjoint):
    fields = [np.asarray(getattr(s, f)) for f in ("lam0", "Phi", "alpha", "beta", "T", "Y", "indices", "eig_res")]
    line = f"{name:58s} m {s.m:2d} N {s.N:2d} extra {s.n_extra}  solve {digest(*fields, int(s.m), int(s.N), int(s.n_extra), int(fac.count))}"
    if adjoint:
        Phib = np.random.default_rng(7).uniform(-1, 1, size=(s.Phi.shape[0], s.N))
        for method in ("sibk", "dl"):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                psi, _ = s.solve_adjoint(Phib, method=method, rtol=1e-10)
            line += f"  {method} {digest(np.array(psi))}"
    print(line, flush=True)


def cases(ctx):
    g4, g3 = golden("g4_laplace900_basiclanczos"), golden("g3_thermal32_eps1e-8_basiclanczos")
    for label, g, sigma, N in (("g4", g4, float(g4["normal_sigma"]), 6), ("g3", g3, float(g3["sigma"]), 5)):
        K, M = csr(g, "K"), csr(g, "M")
        fac = eg.SpLuOperator((K - sigma * M).tocsc(), ctx=ctx)
        for ortho in ("full", "selective"):
            for Ntarget in (None, 2):
                s = solve(K, M, fac, sigma, N=N, m=60, tol=1e-12, ortho_type=ortho, Ntarget=Ntarget)
                report(f"{label} real {ortho} Ntarget={Ntarget}", s, fac, True)
    g1 = golden("g1_buckling50_basiclanczos")
    K, G, sigma = csr(g1, "K"), csr(g1, "G"), float(g1["sigma"])
    fac = eg.SpLuOperator((K + sigma * G).tocsc(), ctx=ctx)
    report("g1 buckling full", solve(G, K, fac, sigma, N=6, m=60, tol=0.0, mode="buckling"), fac, True)
    g6 = golden("g6_buckling50_complexstep")
    K, G, sigma = csr(g6, "K", ("_re", "_im")), csr(g6, "G", ("_re", "_im")), float(g6["sigma"])
    fac = eg.SpLuOperator((K + sigma * G).tocsc(), ctx=ctx)
    for ortho, tol in (("full", 0.0), ("selective", 1e-12)):
        s = solve(G, K, fac, sigma, N=6, m=60, tol=tol, mode="buckling", ortho_type=ortho)
        report(f"g6 complex-step {ortho}", s, fac, False)


def timings(ctx):
    g4, g6 = golden("g4_laplace900_basiclanczos"), golden("g6_buckling50_complexstep")
    K, M, sigma = csr(g4, "K"), csr(g4, "M"), float(g4["normal_sigma"])
    runs = [("g4 real N=6 m=60", (K, M, eg.SpLuOperator((K - sigma * M).tocsc(), ctx=ctx), sigma), dict(N=6, m=60))]
    K, G, sigma = csr(g6, "K", ("_re", "_im")), csr(g6, "G", ("_re", "_im")), float(g6["sigma"])
    runs.append(("g6 complex-step N=6 m=60", (G, K, eg.SpLuOperator((K + sigma * G).tocsc(), ctx=ctx), sigma),
                 dict(N=6, m=60, tol=0.0, mode="buckling")))
    for name, args, kw in runs:
        solve(*args, **kw)                 # (first use: kernels loaded, buffers allocated)
        ts = []
        for _ in range(5):
            ctx.sync()
            t0 = time.perf_counter()
            solve(*args, **kw)
            ctx.sync()
            ts.append(1e3 * (time.perf_counter() - t0))
        print(f"{name:28s} solve ms: {' '.join(f'{t:8.2f}' for t in ts)}   median {np.median(ts):8.2f}", flush=True)


def main():
    ctx = default_context()
    (timings if "--time" in sys.argv[1:] else cases)(ctx)
    ctx.sync()


if __name__ == "__main__":
    main()
