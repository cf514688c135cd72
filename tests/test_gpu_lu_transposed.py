"""
Transposed solves with the LU factor (SpLuOperator.T / .H / rmatvec / rmatmat; csrc/factor.hip:
eigd_factor_solve_transposed_to, csrc/sparse.hip: the transposed companion of a device matrix) against SuperLU's
``solve(B, 'T')`` of the same matrix.  A^T = UU^T LL^T: the sweep reads forward the U side, backward the L side, with the
kernels and the launch list of the untransposed solve -- the matrices, widths and gates are those of test_gpu_lu.py
(imported, not copied): the factor is the same, and neither its normwise backward error nor the 2-norm conditioning
depends on the direction.

The forward-error yardstick is ``splu(mat.tocsc()).solve(B, 'T')`` followed by ONE step of refinement on the host:
SuperLU's unrefined transposed solve has a row-wise backward error of 9.4e-13 on row_swaps and 7.1e-14 on
singular_panel (4.1e-15 and below on the other three), above the 5e-15 gate the refined device solves are held to;
refined once it is at 3.6e-16 and below on all five.

Largest values measured on an MI355X (the gates are test_gpu_lu.py's, which are about ten times ITS measurements):
On refined applications (op.T @ B, op.rmatmat(B); once, three times with static pivots):
  forward error per column   2.0e-13 (grid40_bk); 1.6e-14 on row_swaps, 2.7e-14 on singular_panel
  row-wise backward error    4.8e-16 (grid24_x1024_bk)
Of the unrefined transposed sweep (not gated where there are static pivots, 6.7e-7 on singular_panel):
  row-wise backward error    7.1e-12 (grid24_l16_bk); 8.3e-11 on row_swaps
Every case fits the gate of its forward counterpart.  For comparison, a factor of mat.T applied forward (what the
package could do before) against the same yardstick: forward 1.6e-14 / unrefined backward 6.9e-12 on row_swaps,
2.6e-14 / 1.2e-7 on singular_panel, 1.1e-15 / 2.8e-15 and below on the other three.
Duality (test_duality): 6.7e-16 at most.  The adjoint gradient of the end-to-end test: 1.7e-15.
"""
import numpy as np
import pytest
from scipy import sparse
from scipy.sparse.linalg import splu

from conftest import relerr
from sweep_catalog import CASES, matrix_of
from test_gpu_lu import (BWD_TOL, FWD_TOL, FWD_TOL_INTERCHANGES, RAW_BWD_TOL, RAW_BWD_TOL_INTERCHANGES, WIDTHS,
                         convection_diffusion_2d, convection_diffusion_3d, forward_backward, lu_matrix_of, lu_target,
                         pair_swapped, singular_leaf_matrix, structurally_unsymmetric, symmetrised_of)
from test_lu_transposed_cpu import ConvectionDesign
from test_symbolic_cpu import grid_matrix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from eigd_amd.device import default_context

    return default_context()


def splu_transposed_refined(lu, At, B):
    """the yardstick: SuperLU's transposed solve, refined once on the host (see the module's docstring)"""
    X = lu.solve(B, "T")
    return X + lu.solve(B - At @ X, "T")


def accuracy_matrix(ctx, name):
    if name == "convdiff2d":
        return convection_diffusion_2d(60, 52)
    if name == "convdiff3d":
        return convection_diffusion_3d(14)
    if name == "unsym_pattern":
        return structurally_unsymmetric()
    if name == "row_swaps":
        return pair_swapped(ctx)
    return singular_leaf_matrix()


@pytest.mark.parametrize("name", ["convdiff2d", "convdiff3d", "unsym_pattern", "row_swaps", "singular_panel"])
def test_accuracy_against_splu_transposed(ctx, name):
    import eigd_amd as eg

    mat = accuracy_matrix(ctx, name)
    n = mat.shape[0]
    At = mat.T.tocsr()
    op = eg.SpLuOperator(mat.tocsc(), ctx=ctx, leaf_size=24, symmetric=False)
    assert op.kind == "lu"
    if name == "row_swaps":
        assert op.row_interchanges > 0
    if name == "singular_panel":
        assert op.static_pivots > 0
    lu = splu(mat.tocsc())
    fwd_tol = FWD_TOL_INTERCHANGES if name == "row_swaps" else FWD_TOL
    rng = np.random.default_rng(11)
    worst, worst_raw = (0.0, 0.0), 0.0
    for k in WIDTHS:
        B = rng.normal(size=(n, k))
        raw = op.factor.solve_to(ctx.from_host(B), ctx.empty(n, k), trans=True).get()  # the factor alone, unrefined
        _, raw = forward_backward(At, raw, B, B)
        worst_raw = max(worst_raw, raw)
        Xref = splu_transposed_refined(lu, At, B)
        results = [op.T @ B, op.rmatmat(B)]  # (a real matrix: the adjoint is the transpose)
        for X in results:
            assert X.shape == (n, k)
            fwd, bwd = forward_backward(At, X, B, Xref)
            worst = (max(worst[0], fwd), max(worst[1], bwd))
            print(f"{name} k={k}: forward {fwd:.2e} backward {bwd:.2e} unrefined backward {raw:.2e}")
        if op.static_pivots == 0:
            assert raw < (RAW_BWD_TOL_INTERCHANGES if name == "row_swaps" else RAW_BWD_TOL), (k, raw)
        for X in results:
            fwd, bwd = forward_backward(At, X, B, Xref)
            assert fwd < fwd_tol and bwd < BWD_TOL, (k, fwd, bwd)
    print(f"{name}: transposed forward {worst[0]:.1e} backward {worst[1]:.1e} unrefined backward {worst_raw:.1e} "
          f"interchanges {op.row_interchanges} static {op.static_pivots}")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_sweep_variant_transposed(ctx, case, monkeypatch):
    from eigd_amd.device import CSRMatrix, Factor

    for k, v in case.env:
        monkeypatch.setenv(k, v)
    U, U0, s = lu_matrix_of(case)
    Ut = U.T.tocsr()
    n = U.shape[0]
    F = Factor(ctx, U, leaf_size=case.sym.get("leaf_size", 0), panel_width=case.sym.get("panel_width", 0), lu=True)
    st = F.stats()
    assert st["kind"] == "lu" and st["transposed_copies"] == 0
    lu0 = splu(U0.tocsc()) if case.reference == "splu" else None
    U0t = U0.T.tocsr()
    rng = np.random.default_rng(5)
    launched = set()
    worst, worst_raw = (0.0, 0.0), 0.0
    Ud = CSRMatrix(ctx, symmetrised_of(U))
    for kb in case.widths:
        B = rng.normal(size=(n, kb))
        Bd = ctx.from_host(B)
        Xd = ctx.empty(n, kb)
        with F.sweep_record() as rec:
            F.solve_to(Bd, Xd, trans=True)
        # the launches of the untransposed solve of the same width: an LU sweep has tri = False in either direction
        assert [(v, l) for v, l, _ in rec] == F.symbolic.sweep_plan(kb, tri=False, thin_buf=True), (case.name, kb)
        assert all(w == kb for _, _, w in rec)
        launched |= {(v, l) for v, l, _ in rec}
        _, raw = forward_backward(Ut, Xd.get(), B, B)  # the factor alone: refinement would hide a slightly wrong one
        worst_raw = max(worst_raw, raw)
        print(f"{case.name} kb={kb}: unrefined backward {raw:.2e}")
        if st["static_pivots"] == 0:
            assert raw < RAW_BWD_TOL, (kb, raw)
        F.refine(Ud, Bd, Xd, steps=F.STATIC_PIVOT_REFINEMENTS if st["static_pivots"] else 1, trans=True)
        X = Xd.get()
        _, bwd = forward_backward(Ut, X, B, X)
        print(f"{case.name} kb={kb}: refined backward {bwd:.2e}")
        assert bwd < BWD_TOL, (kb, bwd)
        worst = (worst[0], max(worst[1], bwd))
        if lu0 is not None:
            m0 = U0.shape[0]
            reps = case.replicas if s is not None else 1
            step = max(1, reps // 64)
            for r in range(0, reps, step):
                sl = slice(r * m0, (r + 1) * m0)
                Xr = splu_transposed_refined(lu0, U0t, B[sl]) / (s[r] if s is not None else 1.0)
                fwd = np.max(np.linalg.norm(X[sl] - Xr, axis=0) / np.linalg.norm(Xr, axis=0))
                worst = (max(worst[0], fwd), worst[1])
                assert fwd < FWD_TOL, (kb, r, fwd)
    assert F.stats()["transposed_copies"] == 1
    print(f"{case.name}: transposed forward {worst[0]:.1e} backward {worst[1]:.1e} unrefined backward {worst_raw:.1e}")
    for v, lvl in case.targets:
        v = lu_target(v)
        assert any(v == lv and (lvl is None or lvl == ll) for lv, ll in launched), (v, lvl)


def test_bitwise_invariants_transposed(ctx):
    from eigd_amd.device import Factor

    mat = convection_diffusion_2d(70, 66)
    n = mat.shape[0]
    F = Factor(ctx, mat, leaf_size=32, lu=True)
    rng = np.random.default_rng(3)
    B = rng.normal(size=(n, 64))

    def solve(fac, rhs, trans, c=None):
        c = ctx if c is None else c
        return fac.solve_to(c.from_host(np.ascontiguousarray(rhs)), c.empty(n, rhs.shape[1]), trans=trans)

    # the first transposed solve brings the U side's forward copies: the untransposed solve does not notice
    before = F.stats()
    fwd_before = solve(F, B, False).get()
    assert before["transposed_copies"] == 0
    ref = solve(F, B, True).get()
    after = F.stats()
    assert after["transposed_copies"] == 1 and after["device_bytes"] > before["device_bytes"]
    assert np.array_equal(solve(F, B, False).get(), fwd_before)
    assert not np.array_equal(ref, fwd_before)
    assert F.stats()["device_bytes"] == after["device_bytes"]  # (allocated once)
    # in place
    Xi = ctx.from_host(B)
    F.solve_inplace(Xi, trans=True)
    assert np.array_equal(Xi.get(), ref)
    # a column's result does not depend on the sweep width or on its position in the block
    for k in (1, 5, 16, 17, 32, 33):
        for c0 in (0, 64 - k):
            assert np.array_equal(solve(F, B[:, c0:c0 + k], True).get(), ref[:, c0:c0 + k]), (k, c0)
    # a lane solve equals a solve on the factor's own stream
    other = ctx.fork(1)
    Xo = solve(F, B, True, other)
    other.sync()
    assert np.array_equal(Xo.get(), ref)
    # ... also when the lane's is the factor's first transposed solve
    H = Factor(ctx, mat, symbolic=F.symbolic, lu=True)
    Xo = solve(H, B, True, other)
    other.sync()
    assert np.array_equal(Xo.get(), ref) and H.stats()["transposed_copies"] == 1
    # refactor with new values on the same pattern equals a freshly created factor
    mat2 = mat.copy()
    mat2.data = mat2.data * rng.uniform(0.9, 1.1, size=mat2.nnz)
    F.refactor(mat2)
    assert F.stats()["device_bytes"] == after["device_bytes"]
    G = Factor(ctx, mat2, symbolic=F.symbolic, lu=True)
    X1 = solve(F, B, True).get()
    X2 = solve(G, B, True).get()
    assert np.array_equal(X1, X2)
    assert not np.array_equal(X1, ref)
    # ... and the untransposed solve of the refactored factor is the fresh factor's too
    assert np.array_equal(solve(F, B, False).get(), solve(G, B, False).get())
    _, raw = forward_backward(mat2.T.tocsr(), X1, B, B)
    assert raw < RAW_BWD_TOL


@pytest.mark.parametrize("kind", ["cholesky", "bunch_kaufman"])
def test_symmetric_factor_transposed_is_forward(ctx, kind):
    from eigd_amd.device import Factor

    if kind == "cholesky":
        A, sym = grid_matrix(40, 36, 2, seed=9), {}
    else:
        case = next(c for c in CASES if c.name == "grid40_bk")
        A, sym = matrix_of(case)[0], case.sym
    n = A.shape[0]
    F = Factor(ctx, A, **sym)
    st = F.stats()
    assert st["kind"] == "ldlt" and (st["negative_pivots"] > 0) == (kind == "bunch_kaufman")
    B = np.random.default_rng(2).normal(size=(n, 33))
    with F.sweep_record() as rec_f:
        Xf = F.solve_to(ctx.from_host(B), ctx.empty(n, 33)).get()
    with F.sweep_record() as rec_t:
        Xt = F.solve_to(ctx.from_host(B), ctx.empty(n, 33), trans=True).get()
    assert np.array_equal(Xf, Xt) and rec_f == rec_t and len(rec_t) > 0
    Xi = ctx.from_host(B)
    F.solve_inplace(Xi, trans=True)
    assert np.array_equal(Xi.get(), Xf)
    assert F.stats() == st  # (device_bytes and transposed_copies among them)


def test_duality(ctx):
    """
    Y^T (op X) = (op^T Y)^T X.  Both sides are refined solves with forward errors below FWD_TOL, so by Cauchy-Schwarz
    they differ by at most the sum of the two gates, relative to |y| |op x| per pair of columns: no constant of its own.
    """
    import eigd_amd as eg

    for name, tol in (("convdiff2d", FWD_TOL), ("unsym_pattern", FWD_TOL), ("row_swaps", FWD_TOL_INTERCHANGES)):
        mat = accuracy_matrix(ctx, name)
        n = mat.shape[0]
        op = eg.SpLuOperator(mat.tocsc(), ctx=ctx, leaf_size=24, symmetric=False)
        rng = np.random.default_rng(6)
        X, Y = rng.normal(size=(n, 8)), rng.normal(size=(n, 8))
        Z = op @ X
        W = op.T @ Y
        lhs = np.einsum("ij,ij->j", Y, Z)
        rhs = np.einsum("ij,ij->j", W, X)
        rel = np.max(np.abs(lhs - rhs) / (np.linalg.norm(Y, axis=0) * np.linalg.norm(Z, axis=0)))
        print(f"duality {name}: {rel:.2e}")
        assert rel < 2.0 * tol, (name, rel)


def test_transposed_product(ctx):
    from eigd_amd.device import CSRMatrix

    A = structurally_unsymmetric()
    A.sort_indices()
    n = A.shape[0]
    At = A.T.tocsr()
    assert not np.array_equal(At.indptr, A.indptr)
    rng = np.random.default_rng(8)
    dA = CSRMatrix(ctx, A)
    dAt = dA.transposed()
    assert dA.transposed() is dAt and dAt.shape == (n, n) and dAt.nnz == A.nnz
    X1, X32 = rng.normal(size=(n, 1)), rng.normal(size=(n, 32))
    for X in (X1, X32):
        assert np.array_equal(dAt.apply(ctx.from_host(X)).get(), At @ X)
        assert np.array_equal(dA.apply(ctx.from_host(X)).get(), A @ X)
    # new values on the device: the companion is refreshed there (no upload of the transposed values)
    A2 = A.copy()
    A2.data = rng.normal(size=A.nnz)
    dA.update_values_device(ctx.from_host(A2.data.reshape(-1, 1)))
    A2t = A2.T.tocsr()
    for X in (X1, X32):
        assert np.array_equal(dAt.apply(ctx.from_host(X)).get(), A2t @ X)
        assert np.array_equal(dA.apply(ctx.from_host(X)).get(), A2 @ X)
    assert dA.transposed() is dAt
    # a rectangular map has no companion
    R = sparse.random(20, 30, density=0.2, random_state=1, format="csr")
    with pytest.raises(ValueError, match="square"):
        CSRMatrix(ctx, R).transposed()


def test_surface_transposed(ctx):
    import eigd_amd as eg
    from eigd_amd.device import CSRMatrix

    mat = convection_diffusion_2d(30, 30)
    n = mat.shape[0]
    At = mat.T.tocsr()
    op = eg.SpLuOperator(mat.tocsc(), ctx=ctx, symmetric=False)
    lu = splu(mat.tocsc())
    rng = np.random.default_rng(4)
    b = rng.normal(size=n)
    Bm = rng.normal(size=(n, 3))
    xt, Xt = splu_transposed_refined(lu, At, b), splu_transposed_refined(lu, At, Bm)
    assert op.T.shape == (n, n) and op.H.shape == (n, n) and op.H.dtype == np.float64
    x = op.rmatvec(b)
    assert x.shape == (n,) and op.count == 1
    assert relerr(x, xt) < FWD_TOL
    X = op.rmatmat(Bm)
    assert X.shape == (n, 3) and op.count == 4
    assert relerr(X, Xt) < FWD_TOL
    assert relerr(op.T @ b, xt) < FWD_TOL and op.count == 5
    assert relerr(op.H @ Bm, Xt) < FWD_TOL and op.count == 8 and op.H.count == 8
    assert (op.T @ Bm).shape == (n, 3) and (op.H @ b).shape == (n,) and op.count == 12
    # the one counter is shared with forward applications; op.H.H is op
    assert relerr(op @ b, lu.solve(b)) < FWD_TOL and op.count == 13
    assert relerr(op.H.H @ b, lu.solve(b)) < FWD_TOL and op.count == 14
    assert relerr(op.T.T @ b, lu.solve(b)) < FWD_TOL and op.count == 15
    # device blocks
    Xd = ctx.from_host(Bm)
    op.solve_device(Xd, alpha=2.0, count=2, trans=True)
    assert relerr(Xd.get(), 2.0 * Xt) < FWD_TOL and op.count == 17
    Xo = op.solve_device_to(ctx.from_host(Bm), ctx.empty(n, 3), trans=True)
    assert relerr(Xo.get(), Xt) < FWD_TOL and op.count == 20
    # a symmetric operator: the transposed application is the forward one
    S = grid_matrix(20, 18, 1, seed=3)
    sop = eg.SpLuOperator(S.tocsc(), ctx=ctx)
    bs = rng.normal(size=S.shape[0])
    assert np.array_equal(sop.T @ bs, sop @ bs) and np.array_equal(sop.rmatvec(bs), sop @ bs) and sop.count == 4
    # complex (complex-step) matrix: the dual-number path, against splu of the complex matrix
    dM = sparse.random(n, n, density=4.0 / n, random_state=2, format="csr") + sparse.identity(n)
    cmat = (mat + 1e-20j * dM).tocsc()
    cop = eg.SpLuOperator(cmat, ctx=ctx, symmetric=False)
    clu = splu(cmat)
    bc = rng.normal(size=n) + 1j * rng.normal(size=n)
    for what, got in (("T", cop.T @ bc), ("H", cop.H @ bc), ("H", cop.rmatvec(bc))):
        xr = clu.solve(bc, what)
        assert got.dtype == np.complex128 and got.shape == (n,)
        assert relerr(got.real, xr.real) < FWD_TOL and relerr(got.imag, xr.imag) < 1e-9, what
    Bc = rng.normal(size=(n, 2)) + 1j * rng.normal(size=(n, 2))
    xr = clu.solve(Bc, "H")
    got = cop.rmatmat(Bc)
    assert relerr(got.real, xr.real) < FWD_TOL and relerr(got.imag, xr.imag) < 1e-9
    # values that never visit the host: refactor_device with the device matrix, then a transposed application
    dmat = CSRMatrix(ctx, mat)
    vals = ctx.from_host(mat.data.reshape(-1, 1))
    op.refactor_device(vals, indefinite_matrix=dmat)
    old = op.T @ Bm                      # (makes dmat's transposed companion)
    assert relerr(old, Xt) < FWD_TOL
    mat2 = mat.copy()
    mat2.data = mat.data * rng.uniform(0.9, 1.1, size=mat.nnz)
    vals2 = ctx.from_host(mat2.data.reshape(-1, 1))
    dmat.update_values_device(vals2)
    op.refactor_device(vals2, indefinite_matrix=dmat)
    new = op.T @ Bm
    fresh = eg.SpLuOperator(mat2.tocsc(), ctx=ctx, symmetric=False, symbolic=op.symbolic)
    assert np.array_equal(new, fresh.T @ Bm)
    assert not np.array_equal(new, old)
    assert relerr(new, splu_transposed_refined(splu(mat2.tocsc()), mat2.T.tocsr(), Bm)) < FWD_TOL


GRADIENT_MEASURED = 1.69e-15            # relative error of g in the 2-norm, on an MI355X
GRADIENT_TOL = 10.0 * GRADIENT_MEASURED


def test_adjoint_gradient_of_an_unsymmetric_state_equation(ctx):
    """
    End to end: A(x) u = f with A(x) = D + sum_e x_e C_e on convection_diffusion_2d's grid (diffusion fixed, one
    convection strength per grid line), J = c^T u, gradient g_e = -psi^T C_e u with u = op @ f and psi = op.T @ c from
    ONE factor.  Against the same formula on the host with SuperLU (solve(f), solve(c, 'T')), whose own correctness
    test_lu_transposed_cpu.py checks against central differences.  The error carries the cancellation inside
    psi^T C_e u and cannot be derived in advance: measured 1.69e-15 (relative, 2-norm), gated at ten times that,
    1.69e-14.
    """
    import eigd_amd as eg

    model = ConvectionDesign(60, 52, seed=4)
    A = model.matrix(model.x0)
    assert abs(A - A.T).max() > 0.1
    op = eg.SpLuOperator(A.tocsc(), ctx=ctx, leaf_size=24, symmetric=False)
    bytes_one = op.factor.stats()["device_bytes"]
    u = op @ model.f
    psi = op.T @ model.c      # the same factor
    assert op.count == 2 and op.factor.stats()["transposed_copies"] == 1
    g = model.gradient(u, psi)
    J_host, g_host = model.host_gradient(model.x0)
    err = np.linalg.norm(g - g_host) / np.linalg.norm(g_host)
    print(f"adjoint gradient: relative error {err:.2e} (J {relerr(model.c @ u, J_host):.2e}); factor "
          f"{bytes_one} -> {op.factor.stats()['device_bytes']} bytes")
    assert err < GRADIENT_TOL
