#!/usr/bin/env python3
"""
SHA-256 per case of what the adjoint solvers return -- psi, last_info, the callback's residual history, factor.count --
and, separately, of the integer counters adjoint.LAST_ROUND carries afterwards: bitwise comparison of two versions of
the Python host layer over ONE build of the library.  Public API and adjoint.LAST_ROUND only, and the package is taken
from PYTHONPATH where that names one, so the same file runs against a checkout of another commit:

    python tools/adjoint_digest.py > new.txt
    PYTHONPATH=/path/to/worktree-of-the-other-commit EIGD_LIB=$PWD/eigd_amd/lib/libeigd_hip.so \
        python tools/adjoint_digest.py > old.txt ; diff old.txt new.txt

Cases: solve_adjoint(method="sibk") on the n = 900 fixture (N = 6) and on BucklingColumn(90, 90, seed=2) with N = 24 and
N = 40, over recurrence auto / arnoldi, one and two Krylov steps per Gram-Schmidt pass and two with every pair rejected,
the solution from the z history or by its own recurrence, 1 and 3 streams, the default step limit and maxiter = 7 without
restarts; pgmres and pcpg through the solver; the module-level sibk(), pgmres(), pcpg().  Under streams = 3 several host
threads update the counters of LAST_ROUND: if the counter digest of such a case differs between two runs of ONE version,
leave it out of the comparison.
"""
import hashlib
import os
import sys
import warnings

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)                     # (behind PYTHONPATH: another checkout named there wins)
import eigd_amd as eg  # noqa: E402
from eigd_amd import adjoint as adj  # noqa: E402
from eigd_amd.device import default_context  # noqa: E402
from eigd_amd.problems import BucklingColumn  # noqa: E402

TUNING = ("recurrence", "steps_per_pass", "pair_defect_tol", "cg_solution_from_history")
DEFAULTS = {name: getattr(eg.tuning, name) for name in TUNING}


def digest(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes() if isinstance(p, np.ndarray) else repr(p).encode())
    return h.hexdigest()[:16]


def report(name, fac, psi, info, hist):
    counters = sorted((key, int(v)) for key, v in adj.LAST_ROUND.items() if isinstance(v, (int, np.integer)) and not isinstance(v, bool))
    info = [None if i is None else int(i) for i in info]
    print(f"{name:72s} result {digest(psi, info, np.asarray(hist, dtype=np.float64), int(fac.count))}"
          f"  counters {digest(counters)}  steps {sum(i for i in info if i is not None and i > 0):4d}"
          f"  {adj.LAST_ROUND.get('recurrence')}", flush=True)


def sibk_cases(label, s, fac, Phib, rtol):
    forms = [("auto", 2, DEFAULTS["pair_defect_tol"], hist_kept) for hist_kept in (True, False)]
    forms += [("arnoldi", spp, tol, True) for spp, tol in ((1, DEFAULTS["pair_defect_tol"]), (2, DEFAULTS["pair_defect_tol"]), (2, -1.0))]
    for recurrence, spp, defect_tol, from_history in forms:
        for streams in (1, 3):
            for limits in ({}, {"maxiter": 7, "nrestart": 0}):
                for name, v in zip(TUNING, (recurrence, spp, defect_tol, from_history)):
                    setattr(eg.tuning, name, v)
                adj.LAST_ROUND.clear()
                adj.LAST_ROUND.update({"steps_per_pass": None, "inner_projections": None})
                hist = []
                fac.count = 0
                psi, _ = s.solve_adjoint(Phib, method="sibk", rtol=rtol, callback=hist.append, streams=streams, **limits)
                what = f"{label} sibk {recurrence} spp={spp}{' rejected' if defect_tol < 0 else ''} " \
                       f"history={int(from_history)} streams={streams} {'maxiter=7' if limits else ''}"
                report(what, fac, np.array(psi), s.last_info, hist)
    for name, v in DEFAULTS.items():
        setattr(eg.tuning, name, v)


def main():
    ctx = default_context()
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "g4_laplace900_basiclanczos.npz")))

    def csr(prefix):
        return sparse.csr_matrix((g[prefix + "_data"], g[prefix + "_indices"], g[prefix + "_indptr"]),
                                 shape=tuple(int(v) for v in g[prefix + "_shape"]))

    K, M = csr("K"), csr("M")
    fac = eg.SpLuOperator((K + 0.1 * M).tocsc(), ctx=ctx)
    s = eg.BasicLanczos(N=6, m=60)
    s.solve(K, M, fac, -0.1)
    sibk_cases("laplace900 N=6", s, fac, g["Phib"], 1e-12)
    for method in ("pgmres", "pcpg"):
        hist = []
        fac.count = 0
        psi, _ = s.solve_adjoint(g["Phib"], method=method, rtol=1e-10, callback=hist.append)
        report(f"laplace900 N=6 {method}", fac, np.array(psi), s.last_info, hist)
    lam, Phi = g["normal_lam"], g["normal_Phi"]
    for fn in (eg.sibk, eg.pgmres, eg.pcpg):
        hist = []
        fac.count = 0
        psi, _, info = fn(g["Phib"], K, M, lam, Phi, factor=fac, sigma=-0.1, rtol=1e-10, callback=hist.append, ctx=ctx)
        report(f"laplace900 N=6 {fn.__name__}() of the module", fac, psi, info, hist)

    col = BucklingColumn(90, 90, seed=2)
    Kc = col.stiffness()
    u = col.full_vector(eg.SpLuOperator(Kc, ctx=ctx, check_symmetry=False)(col.f[col.reduced]))
    A, B, sigma = col.geometric_stiffness(u), Kc, 1.0
    facc = eg.SpLuOperator((B + sigma * A).tocsr(), ctx=ctx, check_symmetry=False)
    eg.tuning.iram_block = 4
    for N in (24, 40):
        sc = eg.IRAM(N=N, m=2 * N + 1, mode="buckling", ctx=ctx)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sc.solve(A, B, facc, sigma)
        Phib = np.random.default_rng(7).uniform(-1, 1, size=(B.shape[0], N))
        Phib[:, 3] = 0.0
        sibk_cases(f"column90x90 N={N}", sc, facc, Phib, 1e-10)
    ctx.sync()


if __name__ == "__main__":
    main()
