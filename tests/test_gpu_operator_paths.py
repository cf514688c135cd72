"""
Every arithmetic of SpLuOperator against its application spelled out from public pieces -- ``Factor.solve_to`` on the
right view, the matrix's ``apply``, ``assign_lincomb``, ``Factor.STATIC_PIVOT_REFINEMENTS`` -- in the order the operator
has always made them: the results must be equal bit for bit (np.array_equal; the kernels are deterministic, see the
bitwise invariants of test_gpu_lu.py and test_gpu_complex.py).  Also the two public properties the drivers decide on
(``refined``, ``dual``) and adjoint._short_recurrence_applies for each kind of operator.
"""
import types

import numpy as np
import pytest
from scipy import sparse

from test_complex_cpu import small_complex
from test_gpu_lu import BWD_TOL, convection_diffusion_2d, forward_backward, singular_leaf_matrix

pytestmark = pytest.mark.gpu

WIDTHS = (1, 5)


@pytest.fixture(scope="module")
def ctx():
    from eigd_amd.device import default_context

    return default_context()


@pytest.fixture(scope="module")
def convdiff():
    return convection_diffusion_2d(30, 30)


def steps_of(op):
    return op.factor.STATIC_PIVOT_REFINEMENTS if op.static_pivots > 0 else 1


def refined_real(F, M, B, steps, trans=False):
    """X = M^{-1} B (``trans``: M^{-T} B) by the factor F, refined ``steps`` times against the device matrix M"""
    X = B.ctx.empty(B.n, B.k)
    F.solve_to(B, X, 1.0, trans=trans)
    Mt = M.transposed() if trans else M
    R = B.ctx.empty(B.n, B.k)
    for _ in range(steps):
        Mt.apply(X, R)
        R.assign_lincomb([(1.0, B), (-1.0, R)])
        F.solve_to(R, R, 1.0, trans=trans)
        X.assign_lincomb([(1.0, X), (1.0, R)])
    return X


def negate(block):
    block.assign_lincomb([(-1.0, block)])


def refined_complex(F, M, Z, steps, kind, trans, conjugate):
    """Z <- mat^{-1} Z (mat^{-T}, mat^{-H}) in place on a split-layout block, from the real-equivalent factor F"""
    from eigd_amd.device import interleaved_view

    k = Z.k // 2
    im = Z.cols(k, 2 * k)
    if kind == "lu":
        herm, wrap = trans, trans != conjugate
    else:
        herm, wrap = conjugate, False

    def raw(W):
        V, wim = interleaved_view(W), W.cols(k, 2 * k)
        if kind == "lu":
            F.solve_to(V, V, 1.0, trans=herm)
            return
        if not herm:
            negate(wim)
        F.solve_to(V, V, 1.0)
        if herm:
            negate(wim)

    if wrap:
        negate(im)
    B = Z.copy()
    raw(Z)
    Mh = M.conjugate_transposed() if herm else M
    R = Z.ctx.empty(Z.n, Z.k)
    for _ in range(steps):
        Mh.apply(Z, R)
        R.assign_lincomb([(1.0, B), (-1.0, R)])
        raw(R)
        Z.assign_lincomb([(1.0, Z), (1.0, R)])
    if wrap:
        negate(im)
    return Z


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("name", ["convdiff", "singular_panel"])
def test_real_refined_lu(ctx, convdiff, name, trans):
    import eigd_amd as eg
    from eigd_amd.device import CSRMatrix

    mat = convdiff if name == "convdiff" else singular_leaf_matrix()       # (static pivots: three refinement steps)
    n = mat.shape[0]
    op = eg.SpLuOperator(mat.tocsc(), ctx=ctx, leaf_size=24, symmetric=False)
    assert steps_of(op) == (1 if name == "convdiff" else 3)
    Md = CSRMatrix(ctx, mat)
    rng = np.random.default_rng(21)
    for k in WIDTHS:
        B = rng.normal(size=(n, k))
        want = refined_real(op.factor, Md, ctx.from_host(B), steps_of(op), trans).get()
        X = ctx.from_host(B)
        before = op.count
        op.solve_device(X, trans=trans)
        assert op.count == before + k
        assert np.array_equal(X.get(), want), k
        Y = ctx.empty(n, k)
        op.solve_device_to(ctx.from_host(B), Y, trans=trans)
        assert np.array_equal(Y.get(), want), k
        assert np.array_equal((op.T if trans else op) @ B, want), k


@pytest.mark.parametrize("mode", ["N", "T", "H"])
def test_dual(ctx, convdiff, mode):
    import eigd_amd as eg
    from eigd_amd.device import CSRMatrix

    n = convdiff.shape[0]
    dM = (sparse.random(n, n, density=4.0 / n, random_state=2, format="csr") + sparse.identity(n)).tocsr()
    cmat = (convdiff + 1e-20j * dM).tocsr()
    cmat.sort_indices()
    op = eg.SpLuOperator(cmat.tocsc(), ctx=ctx, leaf_size=24, symmetric=False)
    assert op.complex_arithmetic == "dual"
    Md = CSRMatrix(ctx, sparse.csr_matrix((cmat.data.real.copy(), cmat.indices, cmat.indptr), shape=cmat.shape))
    dMd = CSRMatrix(ctx, sparse.csr_matrix((cmat.data.imag.copy(), cmat.indices, cmat.indptr), shape=cmat.shape))
    trans, conjugate = mode != "N", mode == "H"
    rng = np.random.default_rng(22)
    for k in WIDTHS:
        Br, Bi = rng.normal(size=(n, k)), rng.normal(size=(n, k))
        xr = refined_real(op.factor, Md, ctx.from_host(Br), steps_of(op), trans)
        T = (dMd.transposed() if trans else dMd).apply(xr)
        rhs = ctx.from_host(Bi)
        rhs.assign_lincomb([(1.0, rhs), (1.0 if conjugate else -1.0, T)])
        xi = refined_real(op.factor, Md, rhs, steps_of(op), trans)
        Xr, Xi = ctx.from_host(Br), ctx.from_host(Bi)
        before = op.count
        op.solve_device_dual(Xr, Xi, trans=trans, conjugate=conjugate)
        assert op.count == before + k
        assert np.array_equal(Xr.get(), xr.get()) and np.array_equal(Xi.get(), xi.get()), k
        if mode != "T":
            got = (op.H if mode == "H" else op) @ (Br + 1j * Bi)
            assert np.array_equal(got, xr.get() + 1j * xi.get()), k


@pytest.mark.parametrize("symmetric,mode,forked", [(False, "N", False), (False, "H", False), (False, "T", False), (True, "N", False),
                                                   (True, "H", False), (True, "N", True), (True, "H", True)])
def test_full(ctx, symmetric, mode, forked):
    import eigd_amd as eg
    from eigd_amd.device import ComplexCSRMatrix, complex_join, complex_split

    mat = small_complex(4)
    if symmetric:
        mat = ((mat + mat.T) / 2).tocsr()
    mat.sort_indices()
    n = mat.shape[0]
    op = eg.SpLuOperator(mat.tocsc(), ctx=ctx, leaf_size=24, symmetric=symmetric, complex_arithmetic="full")
    assert op.complex_arithmetic == "full" and op.kind == ("ldlt" if symmetric else "lu")
    Md = ComplexCSRMatrix(ctx, mat)
    where = ctx.fork(1) if forked else ctx
    trans, herm = mode != "N", mode == "H"                # ("T" on the LU form: mat^{-H} between two conjugations)
    rng = np.random.default_rng(23)
    for k in WIDTHS:
        B = rng.normal(size=(n, k)) + 1j * rng.normal(size=(n, k))
        want = refined_complex(op.factor, Md, where.from_host(complex_split(B)), steps_of(op), op.kind, trans, herm)
        where.sync()
        want = want.get()
        Z = where.from_host(complex_split(B))
        before = op.count
        op.solve_device_dual(Z.cols(0, k), Z.cols(k, 2 * k), trans=trans, conjugate=herm)
        where.sync()
        assert op.count == before + k
        assert np.array_equal(Z.get(), want), k
        if not forked:
            assert np.array_equal({"N": op, "T": op.T, "H": op.H}[mode] @ B, complex_join(want)), k
            M = {"N": mat, "T": mat.T, "H": mat.conj().T}[mode].tocsr()     # (the spelled-out sequence solves the system)
            _, bwd = forward_backward(M, complex_join(want), B, B)
            assert bwd < BWD_TOL, (k, bwd)


def test_public_properties_and_short_recurrence(ctx, convdiff):
    import eigd_amd as eg
    from eigd_amd import adjoint
    from eigd_amd.operators import FactorApply

    sym = ((convdiff + convdiff.T) / 2).tocsr()
    n = sym.shape[0]
    ev = np.linalg.eigvalsh(sym.toarray())
    shift = 0.5 * (ev[3] + ev[4])
    ops = {
        "spd": (eg.SpLuOperator(sym.tocsc(), ctx=ctx), False, False),
        "indefinite": (eg.SpLuOperator((sym - shift * sparse.identity(n)).tocsc(), ctx=ctx), True, False),
        "lu": (eg.SpLuOperator(convdiff.tocsc(), ctx=ctx, symmetric=False), True, False),
        "dual": (eg.SpLuOperator((sym + 1e-20j * sym).tocsc(), ctx=ctx), False, True),
        "full": (eg.SpLuOperator((sym + 0.3j * sym).tocsc(), ctx=ctx), True, False),
    }
    assert ops["indefinite"][0].negative_pivots > 0 and ops["spd"][0].negative_pivots == 0
    csr = types.SimpleNamespace(csr=object())
    for name, (op, refined, dual) in ops.items():
        assert op.refined is refined and op.dual is dual, name
        for attr in ("refined", "dual"):
            with pytest.raises(AttributeError):
                setattr(op, attr, True)
        prob = types.SimpleNamespace(fac=FactorApply(ctx, op), opA=csr, opB=csr)
        # (the short recurrence needs a native, positive definite, real factor)
        assert adjoint._short_recurrence_applies(prob) is (name == "spd" and adjoint.tuning.recurrence != "arnoldi"), name
