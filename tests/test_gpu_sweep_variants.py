"""
Every launch variant of the multi-RHS triangular sweep (csrc/factor.hip: sweep_launches, sweep) against a
reference: one parametrised test per case of tests/sweep_catalog.py states which kernels ran (the factor's launch
record) and checks what they computed -- forward error per replica block and column against scipy's LU refined twice
with residuals summed in extended precision, the row-wise backward error, and the bitwise invariants the design
promises (a column's result does not depend on the sweep width, its position, alpha in {-1, 2, 0.5}, the view it is
solved in, the solves before it, the stream it runs on).
"""
import contextlib
import os

import numpy as np
import pytest
from scipy.sparse.linalg import splu

from sweep_catalog import BIG_CASE, BIG_LD, CASES, matrix_of, scale_exponents

pytestmark = pytest.mark.gpu

# Tolerances, set from the largest values measured over all cases on an MI355X with a margin of at least 13x, tighter
# than the suite's other sweep tests (SPD 1e-11 / 1e-12; the Bunch-Kaufman factor alone 1e-9 / 1e-8):
#   SPD            forward error per block and column 1.2e-15 (hub7300), row-wise backward error 7.6e-15 (hub7300)
#   Bunch-Kaufman  forward error 3.7e-13 (grid24_x1024_bk), backward error 1.4e-12 (grid24_x1024_bk)
FWD_TOL = {None: 1e-13, "indefinite": 1e-10}
BWD_TOL = {None: 1e-13, "indefinite": 1e-10}
RHS_PERIOD = 64          # replicated cases: right-hand-side blocks repeat every 64 replicas (scales every 5)
INVARIANT_WIDTHS = (1, 5, 16, 17, 32, 33, 45, 64)


@pytest.fixture(scope="module")
def ctx():
    from eigd_amd.device import default_context

    return default_context()


@contextlib.contextmanager
def environment(pairs):
    old = {k: os.environ.get(k) for k, _ in pairs}
    os.environ.update(dict(pairs))
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def residual_ld(A, X, B, chunk_entries=1 << 24):
    """B - A X with every row sum accumulated in extended precision (np.longdouble)"""
    A = A.tocsr()
    assert (np.diff(A.indptr) > 0).all()              # (reduceat: no empty rows)
    out = np.empty(B.shape)
    step = max(1, chunk_entries // max(A.nnz, 1))
    data = A.data.astype(np.longdouble)[:, None]
    for c0 in range(0, X.shape[1], step):
        c1 = min(X.shape[1], c0 + step)
        s = np.add.reduceat(data * X[A.indices, c0:c1].astype(np.longdouble), A.indptr[:-1], axis=0)
        out[:, c0:c1] = (B[:, c0:c1].astype(np.longdouble) - s).astype(np.float64)
    return out


class HubSchur:
    """direct solver of [[G, C], [C^T, D]] (hub_matrix: grid block first, diagonal hub block last) by the dense Schur
    complement of the hub -- scipy's LU of the whole matrix would fill the hub densely"""

    def __init__(self, A, hub):
        ng = A.shape[0] - hub
        G, C, D = A[:ng, :ng].tocsc(), A[:ng, ng:].toarray(), A[ng:, ng:].toarray()
        self.ng, self.luG, self.C = ng, splu(G), C
        S = D - C.T @ self.luG.solve(C)
        from scipy.linalg import cho_factor

        self.cS = cho_factor(S)

    def solve(self, B):
        from scipy.linalg import cho_solve

        bg, bh = B[:self.ng], B[self.ng:]
        xh = cho_solve(self.cS, bh - self.C.T @ self.luG.solve(bg))
        return np.vstack([self.luG.solve(bg - self.C @ xh), xh])


def refined(A, solver, B, steps=2):
    X = solver.solve(B)
    for _ in range(steps):
        X = X + solver.solve(residual_ld(A, X, B))
    return X


class Prepared:
    """a catalog case on the device: matrix, factor, reference"""

    def __init__(self, ctx, case):
        from eigd_amd.device import Factor, Symbolic

        self.case = case
        self.A, self.A0, self.sigma = matrix_of(case)
        self.n = self.A.shape[0]
        self.n0 = self.A0.shape[0]
        self.R = case.replicas
        self.sym = Symbolic(self.A, **case.sym)
        with environment(case.env):
            self.F = Factor(ctx, self.A, symbolic=self.sym)
        assert (self.F.stats()["negative_pivots"] > 0) == (case.shift is not None)
        self._solver = None

    def fresh_factor(self, ctx):
        from eigd_amd.device import Factor

        with environment(self.case.env):
            return Factor(ctx, self.A, symbolic=self.sym)

    def rhs(self, k, seed=0):
        rng = np.random.default_rng(seed)
        if self.R == 1:
            return rng.normal(size=(self.n, k))
        blocks = rng.normal(size=(RHS_PERIOD, self.n0, k))
        return blocks[np.arange(self.R) % RHS_PERIOD].reshape(self.n, k)

    def reference(self, B):
        k = B.shape[1]
        if self.R == 1:
            if self._solver is None:
                self._solver = (HubSchur(self.A, self.case.hub) if self.case.reference == "schur"
                                else splu(self.A.tocsc()))
            return refined(self.A, self._solver, B)
        # replica i = 4**m_i A0: x_i = 4**-m_i A0^{-1} b_i, one solve per distinct right-hand-side block
        if self._solver is None:
            self._solver = splu(self.A0.tocsc())
        P = min(RHS_PERIOD, self.R)
        Bd = B.reshape(self.R, self.n0, k)[:P].transpose(1, 0, 2).reshape(self.n0, P * k)
        Xd = refined(self.A0, self._solver, Bd).reshape(self.n0, P, k).transpose(1, 0, 2)
        scale = 4.0 ** -scale_exponents(self.R)
        return (Xd[np.arange(self.R) % P] * scale[:, None, None]).reshape(self.n, k)


_prepared = {}


def prepared(ctx, case):
    """one case on the device at a time (the replicated ones hold a factor of 1.2 M rows)"""
    if case.name not in _prepared:
        _prepared.clear()
        _prepared[case.name] = Prepared(ctx, case)
    return _prepared[case.name]


def forward_errors(P, X, Xref):
    """relative 2-norm error of every (replica block, column): an error confined to one replica is not diluted"""
    nb = P.R
    d = (X - Xref).reshape(nb, -1, X.shape[1])
    r = Xref.reshape(nb, -1, X.shape[1])
    return np.linalg.norm(d, axis=1) / np.linalg.norm(r, axis=1)


def backward_error(A, X, B):
    """max over rows of |b - A x|_i / (|A| |x| + |b|)_i, per column"""
    R = np.abs(B - A @ X)
    D = abs(A) @ np.abs(X) + np.abs(B)
    return (R / D).max(axis=0)


def solve(ctx, F, B, alpha=1.0):
    return F.solve_inplace(ctx.from_host(B), alpha=alpha).get()


def launched(rec):
    return {(v, l) for v, l, _ in rec}


def assert_targets_ran(case, rec):
    got = launched(rec)
    names = {v for v, _ in got}
    missing = [(v, l) for v, l in case.targets if (v not in names if l is None else (v, l) not in got)]
    assert not missing, f"{case.name}: not launched {missing}; launched {sorted(got)}"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_sweep_variants_ran_and_match_the_reference(ctx, case):
    P = prepared(ctx, case)
    F = P.F
    B = P.rhs(max(case.widths), seed=1)
    X = {}
    with F.sweep_record() as rec:
        for w in case.widths:
            X[w] = solve(ctx, F, B[:, :w])
    assert_targets_ran(case, rec)
    assert {kb for _, _, kb in rec} == set(case.widths)
    with environment(case.env):                            # plan and launcher cannot drift apart
        for w in case.widths:
            assert [(v, l) for v, l, kb in rec if kb == w] == P.sym.sweep_plan(w, tri=case.shift is None), (case.name, w)
    kmax = max(case.widths)
    Xref = P.reference(B)
    fe = forward_errors(P, X[kmax], Xref)
    be = backward_error(P.A, X[kmax], B)
    print(f"{case.name}: forward error {fe.max():.2e}, row-wise backward error {be.max():.2e}")
    assert fe.max() < FWD_TOL[case.shift], (case.name, np.unravel_index(fe.argmax(), fe.shape), fe.max())
    assert be.max() < BWD_TOL[case.shift], (case.name, be.argmax(), be.max())
    for w in case.widths:                                  # the narrower kernels: same bits as the widest
        assert np.array_equal(X[w], X[kmax][:, :w]), (case.name, w)
    if P.R > 1 and case.shift is None:
        # exact oracle: replicas i and i + RHS_PERIOD solve equal right-hand sides with factors that are exact
        # power-of-two scalings of each other -- their solutions are too, bit for bit
        m = scale_exponents(P.R)
        Xb = X[kmax].reshape(P.R, P.n0, kmax)
        for i in (0, 1, 7, RHS_PERIOD - 1):
            for j in (i + RHS_PERIOD, i + 3 * RHS_PERIOD, P.R - RHS_PERIOD + i):
                assert np.array_equal(Xb[i] * 4.0 ** m[i], Xb[j] * 4.0 ** m[j]), (case.name, i, j)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_sweep_bitwise_invariants(ctx, case):
    P = prepared(ctx, case)
    F, n = P.F, P.n
    B = P.rhs(64, seed=2)
    fresh = P.fresh_factor(ctx)
    X64 = solve(ctx, fresh, B)                             # a factor that has solved nothing before
    del fresh
    # a column's result depends neither on the width of its block nor on its position there
    for kb in INVARIANT_WIDTHS:
        for cols in (np.arange(kb), np.r_[1:kb, 0]):      # column 0 of B at offset 0 and at offset kb - 1
            Xk = solve(ctx, F, B[:, cols])
            assert np.array_equal(Xk, X64[:, cols]), (case.name, kb, int(cols[0]))
    # alpha: powers of two scale the result exactly, 0.3 to rounding
    Bk = B[:, :17]
    for alpha in (-1.0, 2.0, 0.5):
        assert np.array_equal(solve(ctx, F, Bk, alpha), alpha * X64[:, :17]), (case.name, alpha)
    X03 = solve(ctx, F, Bk, 0.3)
    assert forward_errors(P, X03, 0.3 * X64[:, :17]).max() < FWD_TOL[case.shift], case.name
    # out of place, ldin != ldout: the input block is unchanged, and so are the columns of Out outside the view
    In = ctx.from_host(B[:, :40])
    sentinel = np.full((n, 50), 7.25)
    Out = ctx.from_host(sentinel)
    F.solve_to(In.cols(3, 20), Out.cols(30, 47))
    assert np.array_equal(In.get(), B[:, :40])
    out = Out.get()
    assert np.array_equal(out[:, 30:47], X64[:, 3:20])
    assert np.array_equal(out[:, :30], sentinel[:, :30]) and np.array_equal(out[:, 47:], sentinel[:, 47:])
    # a sequence of widths on one factor: the carry planes keep zeros where no child writes
    for kb in (32, 1, 16, 5, 32):
        assert np.array_equal(solve(ctx, F, B[:, 8:8 + kb]), X64[:, 8:8 + kb]), (case.name, "sequence", kb)
    # two lanes (other streams, own workspaces) solving concurrently on one factor
    side1, side2 = ctx.fork(1), ctx.fork(2)
    I1, I2 = side1.from_host(B[:, :32]), side2.from_host(B[:, 32:45])
    O1, O2 = side1.empty(n, 32), side2.empty(n, 13)
    side1.sync()
    side2.sync()
    with F.sweep_record() as rec:
        F.solve_to(I1, O1)
        F.solve_to(I2, O2)
        side1.sync()
        side2.sync()
    assert np.array_equal(O1.get(), X64[:, :32]) and np.array_equal(O2.get(), X64[:, 32:45])
    with F.sweep_record() as rec_main:
        X32 = solve(ctx, F, B[:, :32])
    assert np.array_equal(X32, X64[:, :32])
    assert [(v, l) for v, l, _ in rec[:len(rec_main)]] == [(v, l) for v, l, _ in rec_main]   # a lane runs the same kernels
    # refactor (4 A: an exact scaling) and refactor_device (back to A) are followed
    F.refactor(P.A * 4.0)
    assert np.array_equal(solve(ctx, F, B[:, :17]), X64[:, :17] / 4.0), case.name
    F.refactor_device(ctx.from_host(P.A.data.reshape(-1, 1)))
    assert np.array_equal(solve(ctx, F, B[:, :17]), X64[:, :17]), case.name


def test_thin_buffer_edge(ctx):
    """
    The forward thin kernels address the caller's block with 32-bit buffer offsets.  n = 65536 rows with ld = 8191
    (n ld 8 bytes just below 2**32, offsets of the last rows above 2**31) still takes them; ld = 8192 (2**32) takes the
    tile kernels.  Both give bitwise the columns of a compact block, and leave the other columns alone.
    """
    from eigd_amd.device import DeviceBlock, Factor

    A, _, _ = matrix_of(BIG_CASE)
    n = A.shape[0]
    assert n == 65536
    F = Factor(ctx, A)
    rng = np.random.default_rng(4)
    B = rng.normal(size=(n, 32))
    Xc = solve(ctx, F, B)
    Xref = splu(A.tocsc()).solve(B)
    assert np.abs(Xc - Xref).max() / np.abs(Xref).max() < 1e-11
    for ld in BIG_LD:
        big = DeviceBlock(ctx, n, ld)
        big.zero()
        view = big.cols(ld - 32, ld)                      # the last columns: byte offsets up to n ld 8
        view.set(B)
        assert np.array_equal(view.get(), B)
        with F.sweep_record() as rec:
            F.solve_inplace(view)
            F.solve_inplace(big.cols(ld - 48, ld - 32).copy_from(ctx.from_host(B[:, :16])))
        assert [(v, l) for v, l, _ in rec] == [
            p for w in (32, 16) for p in F.symbolic.sweep_plan(w, thin_buf=n * ld * 8 <= 0xFFFFFFF0)], ld
        names = {v for v, _, _ in rec}
        thin = {v for v in names if v.startswith("fwd_thin_kernel<")}
        if n * ld * 8 <= 0xFFFFFFF0:                      # kBufMax
            assert {v.split(",")[0] for v in thin} == {"fwd_thin_kernel<16", "fwd_thin_kernel<32"}, sorted(names)
        else:
            assert not thin, sorted(thin)
            assert_targets_ran(BIG_CASE, rec)
        assert np.array_equal(view.get(), Xc), ld
        assert np.array_equal(big.cols(ld - 48, ld - 32).get(), Xc[:, :16]), ld
        assert not big.cols(ld - 56, ld - 48).get().any()
        del big, view
