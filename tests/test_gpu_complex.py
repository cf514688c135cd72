"""
Full complex arithmetic in SpLuOperator (complex_arithmetic="full" / "auto" on a genuinely complex matrix): the
real-equivalent LU and symmetric factors against scipy's complex splu refined once on the host, the adjoint surface, the
path selection, the complex product on split-layout blocks (csrc/sparse.hip: cspmv_stream_kernel, cspmm_tiled_kernel),
the value expansion (expand_values_kernel), refactorisation, the bitwise invariants and the refusals.

The gates are test_gpu_lu.py's for refined LU applications (FWD_TOL = 1e-11 per column, BWD_TOL = 5e-15 row-wise).
The complex product is gated bitwise on scipy's complex ``A @ X`` (test_complex_cpu.py records that scipy equals the
host restatement of the kernel's order bit for bit) and on the restatement where alpha and beta come in.

Largest values: not measured on an MI355X yet -- no device was available while this file was written (docs/LOG.md).
The tests print them per case and width (run with -s).  On the host, the real-equivalent LU form restated with SuperLU
reaches forward 1.2e-15 ... 2.0e-15 and backward 2.2e-16 ... 2.4e-16 after one refinement (unrefined <= 5.2e-15 /
4.6e-14), the symmetric form 2.5e-15 unrefined.
"""
import numpy as np
import pytest
from scipy import sparse
from scipy.sparse.linalg import splu

from conftest import relerr
from test_complex_cpu import complex_matrices, restated_product
from test_gpu_lu import BWD_TOL, FWD_TOL, WIDTHS, convection_diffusion_2d, forward_backward

pytestmark = pytest.mark.gpu

LEAF = 24


@pytest.fixture(scope="module")
def ctx():
    from eigd_amd.device import default_context

    return default_context()


def refined_splu(mat, B, trans="N"):
    """scipy's complex splu, refined once on the host: the yardstick"""
    lu = splu(mat.tocsc())
    M = {"N": mat, "T": mat.T.tocsr(), "H": mat.conj().T.tocsr()}[trans]
    X = lu.solve(B, trans)
    return X + lu.solve(B - M @ X, trans)


def complex_rhs(rng, n, k=None):
    shape = (n,) if k is None else (n, k)
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


@pytest.mark.parametrize("name,symmetric", [("damped", False), ("complex_shift", False), ("complex_convection", False),
                                            ("damped", True)])
def test_accuracy_against_complex_splu(ctx, name, symmetric):
    import eigd_amd as eg

    mat = complex_matrices()[name]
    n = mat.shape[0]
    op = eg.SpLuOperator(mat.tocsc(), ctx=ctx, leaf_size=LEAF, symmetric=symmetric)
    assert op.complex_arithmetic == "full" and op.dtype == np.complex128
    assert op.kind == ("ldlt" if symmetric else "lu")
    assert op.negative_pivots is None and op.negative_pivots_bounds is None
    rng = np.random.default_rng(11)
    worst = (0.0, 0.0)
    for k in WIDTHS:
        B = complex_rhs(rng, n, k)
        X = op(B)
        assert X.shape == (n, k) and X.dtype == np.complex128
        fwd, bwd = forward_backward(mat, X, B, refined_splu(mat, B))
        print(f"{name} symmetric={symmetric} k={k}: forward {fwd:.1e} backward {bwd:.1e}")
        assert fwd < FWD_TOL and bwd < BWD_TOL, (k, fwd, bwd)
        worst = (max(worst[0], fwd), max(worst[1], bwd))
    print(f"{name} symmetric={symmetric}: forward {worst[0]:.1e} backward {worst[1]:.1e} kind {op.kind} "
          f"interchanges {op.row_interchanges} static {op.static_pivots}")


@pytest.mark.parametrize("name,symmetric", [("complex_shift", False), ("complex_convection", False), ("damped", True)])
def test_adjoint_surface(ctx, name, symmetric):
    import eigd_amd as eg

    mat = complex_matrices()[name]
    n = mat.shape[0]
    op = eg.SpLuOperator(mat.tocsc(), ctx=ctx, leaf_size=LEAF, symmetric=symmetric)
    rng = np.random.default_rng(5)
    b, Bm = complex_rhs(rng, n), complex_rhs(rng, n, 4)

    def gate(x, rhs, trans):
        M = {"N": mat, "T": mat.T.tocsr(), "H": mat.conj().T.tocsr()}[trans]
        fwd, bwd = forward_backward(M, x.reshape(n, -1), rhs.reshape(n, -1), refined_splu(mat, rhs, trans).reshape(n, -1))
        print(f"{name} symmetric={symmetric} trans={trans}: forward {fwd:.1e} backward {bwd:.1e}")
        assert fwd < FWD_TOL and bwd < BWD_TOL, (trans, fwd, bwd)

    assert op.count == 0
    x = op(b)
    assert x.shape == (n,) and op.count == 1
    gate(x, b, "N")
    gate(op @ Bm, Bm, "N")
    assert op.count == 5
    xh = op.H @ b
    assert xh.shape == (n,) and xh.dtype == np.complex128 and op.count == 6
    gate(xh, b, "H")
    xt = op.T @ b
    assert op.count == 7
    gate(xt, b, "T")
    gate(op.rmatvec(b), b, "H")
    assert op.count == 8
    Xh = op.rmatmat(Bm)
    assert Xh.shape == (n, 4) and op.count == 12 and op.H.count == 12
    gate(Xh, Bm, "H")
    gate(op.T @ Bm, Bm, "T")
    gate(op.H.matmat(Bm), Bm, "H")
    assert op.H.H is op
    # duality: Y^H (op X) = (op.H Y)^H X
    X, Y = complex_rhs(rng, n, 4), complex_rhs(rng, n, 4)
    OX, OHY = op @ X, op.H @ Y
    for c in range(4):
        lhs, rhs = np.vdot(Y[:, c], OX[:, c]), np.vdot(OHY[:, c], X[:, c])
        assert abs(lhs - rhs) < 2 * FWD_TOL * np.linalg.norm(Y[:, c]) * np.linalg.norm(OX[:, c]), c
    # the device surface: halves of one block in place, two separate blocks through a copy
    from eigd_amd.device import complex_split

    Z = ctx.from_host(complex_split(Bm))
    before = op.count
    op.solve_device_dual(Z.cols(0, 4), Z.cols(4, 8), trans=True, conjugate=True)
    assert op.count == before + 4
    Xr, Xi = ctx.from_host(np.ascontiguousarray(Bm.real)), ctx.from_host(np.ascontiguousarray(Bm.imag))
    op.solve_device_dual(Xr, Xi, trans=True, conjugate=True)
    got = Z.get()
    assert np.array_equal(got[:, :4], Xr.get()) and np.array_equal(got[:, 4:], Xi.get())
    assert np.array_equal(got[:, :4] + 1j * got[:, 4:], Xh)


def test_path_selection(ctx):
    import eigd_amd as eg

    M = convection_diffusion_2d(30, 30)
    n = M.shape[0]
    dM = sparse.random(n, n, density=4.0 / n, random_state=2, format="csr") + sparse.identity(n)
    cmat = (M + 1e-20j * dM).tocsr()
    cmat.sort_indices()
    rng = np.random.default_rng(4)
    bc = complex_rhs(rng, n)
    auto = eg.SpLuOperator(cmat.tocsc(), ctx=ctx, symmetric=False)
    assert auto.complex_arithmetic == "dual" and auto.dtype == np.complex128
    xa = auto(bc)
    # the dual-number formula as it has always run, restated with a real operator and the matrices on the host:
    # x + i M^{-1}(db - dM x), x = M^{-1} b
    real = eg.SpLuOperator(sparse.csr_matrix((cmat.data.real.copy(), cmat.indices, cmat.indptr), shape=cmat.shape).tocsc(),
                           ctx=ctx, symmetric=False)
    assert real.complex_arithmetic is None
    xr = real(bc.real.copy())
    dMx = sparse.csr_matrix((cmat.data.imag.copy(), cmat.indices, cmat.indptr), shape=cmat.shape) @ xr
    xi = real(bc.imag - dMx)
    assert np.array_equal(xa.real, xr) and np.array_equal(xa.imag, xi)
    forced = eg.SpLuOperator(cmat.tocsc(), ctx=ctx, symmetric=False, complex_arithmetic="dual")
    assert forced.complex_arithmetic == "dual" and np.array_equal(forced(bc), xa)
    # forced "full" on the same matrix: the real part agrees with complex SuperLU; the imaginary part of the solution
    # (1e-20 of the real part from the matrix, plus the right-hand side's) is not resolved by the comparison -- for a real
    # right-hand side it lies below what double precision resolves next to the real part
    full = eg.SpLuOperator(cmat.tocsc(), ctx=ctx, symmetric=False, complex_arithmetic="full")
    assert full.complex_arithmetic == "full" and full.kind == "lu"
    xf = full(bc.real.copy())
    xs = splu(cmat.tocsc()).solve(bc.real.astype(np.complex128))
    assert xf.dtype == np.complex128 and relerr(xf.real, xs.real) < FWD_TOL
    assert np.max(np.abs(xf.imag)) < np.finfo(np.float64).eps * np.max(np.abs(xf.real))
    # a ratio of 1e-6 is a complex matrix
    c6 = (M + 1e-6j * dM).tocsc()
    op6 = eg.SpLuOperator(c6, ctx=ctx, symmetric=False)
    assert op6.complex_arithmetic == "full"
    fwd, bwd = forward_backward(c6.tocsr(), op6(bc).reshape(n, 1), bc.reshape(n, 1), refined_splu(c6.tocsr(), bc).reshape(n, 1))
    assert fwd < FWD_TOL and bwd < BWD_TOL
    d6 = eg.SpLuOperator(c6, ctx=ctx, symmetric=False, complex_arithmetic="dual")
    assert d6.complex_arithmetic == "dual"
    assert relerr(d6(bc).real, xr) < FWD_TOL          # (the real factor's answer: first order in dM only)
    with pytest.raises(ValueError):
        eg.SpLuOperator(c6, ctx=ctx, symmetric=False, complex_arithmetic="native")


@pytest.mark.parametrize("name", ["damped", "complex_shift", "complex_convection"])
def test_complex_product(ctx, name):
    from eigd_amd.device import ComplexCSRMatrix, complex_join, complex_split

    A = complex_matrices()[name]
    A.sort_indices()
    n = A.shape[0]
    Ad = ComplexCSRMatrix(ctx, A)
    rng = np.random.default_rng(8)

    def check(Adev, Ahost):
        Ah_host = Ahost.conj().T.tocsr()
        Ah_host.sort_indices()
        for k in (1, 4, 32, 33):
            X, Y0 = complex_rhs(rng, n, k), complex_rhs(rng, n, k)
            Xd = ctx.from_host(complex_split(X))
            for dev, host in ((Adev, Ahost), (Adev.conjugate_transposed(), Ah_host)):
                Y = complex_join(dev.apply(Xd).get())
                assert np.array_equal(Y, host @ X), (k, "scipy")
                assert np.array_equal(Y, restated_product(host, X)), (k, "restatement")
                Yd = ctx.from_host(complex_split(Y0))
                dev.apply(Xd, Yd, alpha=-1.0, beta=1.0)
                assert np.array_equal(complex_join(Yd.get()), restated_product(host, X, -1.0, 1.0, Y0)), (k, "alpha, beta")
        x = complex_rhs(rng, n)
        assert np.array_equal(Adev.matvec(x), Ahost @ x)

    check(Ad, A)
    Ad.conjugate_transposed()
    new = A.data * rng.uniform(0.5, 1.5, size=A.nnz) + 1j * rng.normal(size=A.nnz)
    Ad.update_values_device(ctx.from_host(np.ascontiguousarray(new).view(np.float64).reshape(A.nnz, 2)))
    check(Ad, sparse.csr_matrix((new, A.indices, A.indptr), shape=A.shape))
    assert Ad.spmm_bytes(4) == 20.0 * A.nnz + 4.0 * n + 32.0 * n * 4


@pytest.mark.parametrize("name,symmetric", [("complex_convection", False), ("damped", True)])
def test_refactorisation(ctx, name, symmetric):
    import eigd_amd as eg
    from eigd_amd.device import real_equivalent

    mat = complex_matrices()[name]
    mat.sort_indices()
    n = mat.shape[0]
    rng = np.random.default_rng(6)
    B = complex_rhs(rng, n, 4)
    if symmetric:   # (new values that keep the matrix complex symmetric)
        new = mat.data * (1.1 - 0.05j)
    else:
        new = mat.data * rng.uniform(0.9, 1.1, size=mat.nnz) + 0.01j * rng.normal(size=mat.nnz)
    mat2 = sparse.csr_matrix((new, mat.indices, mat.indptr), shape=mat.shape)
    op = eg.SpLuOperator(mat.tocsc(), ctx=ctx, leaf_size=LEAF, symmetric=symmetric)
    x1 = op(B)
    op.refactor(mat2)
    x2 = op(B)
    fresh = eg.SpLuOperator(mat2.tocsc(), ctx=ctx, leaf_size=LEAF, symmetric=symmetric)
    assert np.array_equal(x2, fresh(B)) and not np.array_equal(x2, x1)
    fwd, bwd = forward_backward(mat2, x2, B, refined_splu(mat2, B))
    assert fwd < FWD_TOL and bwd < BWD_TOL
    # from the device: an nnz x 2 block, real and imaginary part per entry in CSR order
    vals = ctx.from_host(np.ascontiguousarray(new).view(np.float64).reshape(mat.nnz, 2))
    dev = eg.SpLuOperator(mat.tocsc(), ctx=ctx, leaf_size=LEAF, symmetric=symmetric)
    expanded = dev.expand_values_device(vals).get()[:, 0]
    assert np.array_equal(expanded, real_equivalent(mat2, "symmetric" if symmetric else "lu").data)
    dev.refactor_device(vals)
    assert np.array_equal(dev(B), x2)
    assert np.array_equal(dev.H @ B, op.H @ B)
    from eigd_amd.device import ComplexCSRMatrix

    dev.refactor_device(ctx.from_host(np.ascontiguousarray(mat.data).view(np.float64).reshape(mat.nnz, 2)),
                        indefinite_matrix=ComplexCSRMatrix(ctx, mat))
    assert np.array_equal(dev(B), x1)


@pytest.mark.parametrize("name,symmetric", [("complex_shift", False), ("damped", True)])
def test_bitwise_invariants(ctx, name, symmetric):
    import eigd_amd as eg

    mat = complex_matrices()[name]
    n = mat.shape[0]
    op = eg.SpLuOperator(mat.tocsc(), ctx=ctx, leaf_size=LEAF, symmetric=symmetric)
    B = complex_rhs(np.random.default_rng(3), n, 33)
    ref, refh = op(B), op.H @ B
    for k in (1, 4, 32):
        for c0 in (0, 33 - k):
            cols = np.ascontiguousarray(B[:, c0:c0 + k])
            assert np.array_equal(op(cols), ref[:, c0:c0 + k]), (k, c0)
            assert np.array_equal(op.H @ cols, refh[:, c0:c0 + k]), (k, c0)
    assert np.array_equal(op(B[:, 7].copy()), ref[:, 7])


def test_refusals(ctx):
    import eigd_amd as eg

    mats = complex_matrices()
    shift = mats["complex_shift"]
    n = shift.shape[0]
    with pytest.raises(ValueError, match="symmetric=False"):
        eg.SpLuOperator(shift.tocsc(), ctx=ctx, leaf_size=LEAF)
    op = eg.SpLuOperator(shift.tocsc(), ctx=ctx, leaf_size=LEAF, symmetric=False)
    X = ctx.from_host(np.ones((n, 2)))
    with pytest.raises(TypeError):
        op.solve_device(X)
    with pytest.raises(TypeError):
        op.solve_device_to(X, ctx.empty(n, 2))
    assert op.count == 0
    with pytest.raises(ValueError):
        op.refactor(shift.real.tocsr())                       # "full" -> real / "dual"
    M = convection_diffusion_2d(30, 30)
    dual = eg.SpLuOperator((M + 1e-20j * M).tocsc(), ctx=ctx, symmetric=False)
    assert dual.complex_arithmetic == "dual"
    with pytest.raises(ValueError):
        dual.refactor((M + 0.3j * M).tocsr())                 # "dual" -> "full"
    realop = eg.SpLuOperator(M.tocsc(), ctx=ctx, symmetric=False)
    with pytest.raises(ValueError):
        realop.refactor((M + 0.3j * M).tocsr())
    with pytest.raises(TypeError):
        realop.solve_device_dual(X, X)
    sing = shift.tolil()
    sing[5, :] = 0.0
    sing = sing.tocsr()
    sing.eliminate_zeros()
    with pytest.raises(np.linalg.LinAlgError):
        eg.SpLuOperator(sing.tocsc(), ctx=ctx, leaf_size=LEAF, symmetric=False)
