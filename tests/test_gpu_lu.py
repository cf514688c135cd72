"""
LU factor of unsymmetric matrices (SpLuOperator(..., symmetric=False); csrc/factor.hip: lu_inv_kernel,
lu_update_kernel, the U side of the copies the sweeps read) against scipy's splu of the same matrix: forward error
per column and row-wise backward error over the sweep widths, every launch variant of the sweep catalog on an
unsymmetric matrix of the case's pattern, the bitwise invariants of the sweeps, the public surface and the end-to-end
adjoint on golden fixtures.

Largest values measured on an MI355X; the gates below are about ten times these.  On refined applications
(SpLuOperator refines every application of an LU factor once, three times with static pivots):
  forward error per column   7.5e-13 (grid40_bk: the catalog's indefinite blocks made unsymmetric); 8.3e-12 for the
                             matrix that needs row interchanges (row_swaps: its pivots are 1 % of the diagonal it had,
                             the error is the conditioning's -- the backward error stays at rounding level)
  row-wise backward error    4.8e-16 (grid24_l56_x512_bk)
Of the unrefined solve (the factor alone; not gated where there are static pivots, 3.1e-7 on singular_panel):
  row-wise backward error    2.4e-12 (grid40_bk); 6.9e-11 on row_swaps
"""
import numpy as np
import pytest
from scipy import sparse
from scipy.sparse.linalg import splu

from conftest import align_signs, csr_from, load_golden, relerr
from sweep_catalog import CASES, matrix_of, scale_exponents
from test_gpu_kernels import lap3d
from test_symbolic_cpu import grid_matrix

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-11
FWD_TOL_INTERCHANGES = 1e-10
BWD_TOL = 5e-15
RAW_BWD_TOL = 3e-11                 # unrefined solves (factors without static pivots)
RAW_BWD_TOL_INTERCHANGES = 1e-9
WIDTHS = (1, 4, 8, 16, 32, 33, 64)


@pytest.fixture(scope="module")
def ctx():
    from eigd_amd.device import default_context

    return default_context()


def skew(A, scale=0.3):
    """A + scale (tril(A, -1) - triu(A, 1)): numerically unsymmetric on A's pattern"""
    return (A + scale * (sparse.tril(A, -1) - sparse.triu(A, 1))).tocsr()


def convection_diffusion_2d(nx, ny, peclet=0.8):
    """5-point diffusion plus first-order upwinded convection (numerically unsymmetric, structurally symmetric)"""
    def op(m, eps):
        return sparse.diags([-1.0 - eps, 2.0 + eps, -1.0], [-1, 0, 1], shape=(m, m))
    Ix, Iy = sparse.identity(nx), sparse.identity(ny)
    return (sparse.kron(Iy, op(nx, peclet)) + sparse.kron(op(ny, 0.5 * peclet), Ix)).tocsr()


def convection_diffusion_3d(m, peclet=0.6):
    A = lap3d(m)
    n = A.shape[0]
    # skew-symmetric convection on the Laplacian's couplings (upwinded: the diagonal absorbs the outflow)
    C = sparse.triu(A, 1)
    return (A + peclet * (C.T - C) + sparse.diags(np.full(n, peclet))).tocsr()


def structurally_unsymmetric(nx=30, ny=28, seed=1):
    """a grid matrix plus one-directional couplings to nodes a few rows further on"""
    rng = np.random.default_rng(seed)
    A = grid_matrix(nx, ny, 1, seed=seed)
    n = A.shape[0]
    r = rng.integers(0, n - 3 * nx, size=n // 2)
    c = r + rng.integers(nx - 1, 3 * nx, size=r.size)
    E = sparse.csr_matrix((rng.uniform(-0.5, 0.5, size=r.size), (r, c)), shape=(n, n))
    out = (A + E).tocsr()
    assert (abs(out) > 0).astype(int).__ne__((abs(out.T) > 0).astype(int)).nnz > 0
    return out


def pair_swapped(ctx, nx=26, ny=24, seed=2):
    """
    a diagonally dominant matrix whose coupled pairs of dofs inside a front have their dominance moved off the
    diagonal (row a of the pair lives, in size, at row b): needs row interchanges, on the grid's own pattern
    """
    from eigd_amd.device import Symbolic, symmetrised_pattern

    A = grid_matrix(nx, ny, 1, seed=seed).tolil()
    sym = Symbolic(symmetrised_pattern(A.tocsr()), leaf_size=24)
    perm, c0, ns = sym.array("perm"), sym.array("f_c0"), sym.array("f_ns")
    swapped = 0
    for f in range(len(c0)):
        cols = perm[c0[f]: c0[f] + ns[f]]
        for a, b in zip(cols[0::2], cols[1::2]):
            if A[b, a] != 0.0:
                A[b, a] = 4.0 * abs(A[a, a])
                A[a, a] *= 0.01
                swapped += 1
    assert swapped > 10
    out = A.tocsr()
    out.sort_indices()
    return out


def forward_backward(mat, X, B, Xref):
    """(max forward error per column, max row-wise backward error)"""
    fwd = np.max(np.linalg.norm(X - Xref, axis=0) / np.linalg.norm(Xref, axis=0))
    absA = abs(mat)
    den = absA @ np.abs(X) + np.abs(B)
    bwd = np.max(np.abs(mat @ X - B) / np.maximum(den, 1e-300))
    return fwd, bwd


@pytest.mark.parametrize("name", ["convdiff2d", "convdiff3d", "unsym_pattern", "row_swaps", "singular_panel"])
def test_accuracy_against_splu(ctx, name):
    import eigd_amd as eg

    leaf = 24
    if name == "convdiff2d":
        mat = convection_diffusion_2d(60, 52)
    elif name == "convdiff3d":
        mat = convection_diffusion_3d(14)
    elif name == "unsym_pattern":
        mat = structurally_unsymmetric()
    elif name == "row_swaps":
        mat = pair_swapped(ctx)
    else:
        mat = singular_leaf_matrix()
    n = mat.shape[0]
    with pytest.raises(ValueError):
        eg.SpLuOperator(mat.tocsc(), ctx=ctx, leaf_size=leaf)
    op = eg.SpLuOperator(mat.tocsc(), ctx=ctx, leaf_size=leaf, symmetric=False)
    assert op.kind == "lu" and op.negative_pivots is None and op.negative_pivots_bounds is None
    if name == "row_swaps":
        assert op.row_interchanges > 0
    if name == "singular_panel":
        assert op.static_pivots > 0
    lu = splu(mat.tocsc())
    rng = np.random.default_rng(11)
    worst, worst_raw = (0.0, 0.0), 0.0
    for k in WIDTHS:
        B = rng.normal(size=(n, k))
        raw = op.factor.solve_to(ctx.from_host(B), ctx.empty(n, k)).get()  # the factor alone, unrefined
        _, raw = forward_backward(mat, raw, B, B)
        if op.static_pivots == 0:
            assert raw < (RAW_BWD_TOL_INTERCHANGES if name == "row_swaps" else RAW_BWD_TOL), (k, raw)
        worst_raw = max(worst_raw, raw)
        X = op(B)
        assert X.shape == (n, k)
        fwd, bwd = forward_backward(mat, X, B, lu.solve(B))
        assert fwd < (FWD_TOL_INTERCHANGES if name == "row_swaps" else FWD_TOL) and bwd < BWD_TOL, (k, fwd, bwd)
        worst = (max(worst[0], fwd), max(worst[1], bwd))
    print(f"{name}: forward {worst[0]:.1e} backward {worst[1]:.1e} unrefined backward {worst_raw:.1e} "
          f"interchanges {op.row_interchanges} "
          f"static {op.static_pivots}")


def singular_leaf_matrix():
    """(test_gpu_kernels: a leaf front singular by itself, the matrix not) made unsymmetric on the same pattern"""
    from eigd_amd.device import Symbolic

    K = grid_matrix(26, 22, 1, seed=4)
    n = K.shape[0]
    rng = np.random.default_rng(8)
    M = sparse.diags(rng.uniform(0.5, 1.5, size=n)).tocsr()
    sym = Symbolic(K, leaf_size=24)
    perm, c0, ns, lvl = sym.array("perm"), sym.array("f_c0"), sym.array("f_ns"), sym.array("f_level")
    leaf = int(np.flatnonzero(lvl == lvl.min())[0])
    idx = perm[c0[leaf]: c0[leaf] + ns[leaf]]
    Md = M.diagonal()
    Kl = K.toarray()[np.ix_(idx, idx)]
    ev = np.linalg.eigvalsh(np.diag(Md[idx] ** -0.5) @ Kl @ np.diag(Md[idx] ** -0.5))
    mat = (K - ev[0] * M).tocsr()
    # unsymmetric outside the singular leaf block: the leaf's own block stays singular
    inside = np.zeros(n, dtype=bool)
    inside[idx] = True
    S = skew(mat, 0.2).tocoo()
    keep = inside[S.row] & inside[S.col]
    T = mat.tocoo()
    Tk = inside[T.row] & inside[T.col]
    data = np.where(keep, 0.0, S.data)
    out = (sparse.csr_matrix((data, (S.row, S.col)), shape=(n, n))
           + sparse.csr_matrix((np.where(Tk, T.data, 0.0), (T.row, T.col)), shape=(n, n))).tocsr()
    out.sort_indices()
    assert np.linalg.matrix_rank(out.toarray()[np.ix_(idx, idx)]) < len(idx)
    return out


def lu_matrix_of(case):
    """(full unsymmetric matrix, its block U0 the reference factors, scales of the replicas)"""
    A, A0, sigma = matrix_of(case)
    U0 = skew(A0, 0.3)
    U0.sort_indices()
    if case.replicas > 1:
        s = 4.0 ** scale_exponents(case.replicas)
        U = sparse.kron(sparse.diags(s), U0).tocsr()
    else:
        s, U = None, U0
    U.sort_indices()
    return U, U0, s


def lu_target(name):
    """an LU factor has dense diagonal blocks on its forward side: the thin kernels run their TRI = false form"""
    if name.startswith(("fwd_thin_kernel", "bwd_thin_kernel")):
        return name.replace(", true>", ", false>")
    return name


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_sweep_variant(ctx, case, monkeypatch):
    from eigd_amd.device import Factor

    for k, v in case.env:
        monkeypatch.setenv(k, v)
    U, U0, s = lu_matrix_of(case)
    n = U.shape[0]
    F = Factor(ctx, U, leaf_size=case.sym.get("leaf_size", 0), panel_width=case.sym.get("panel_width", 0), lu=True)
    st = F.stats()
    assert st["kind"] == "lu" and st["negative_pivots"] == 0
    lu0 = splu(U0.tocsc()) if case.reference == "splu" else None
    rng = np.random.default_rng(5)
    launched = set()
    worst, worst_raw = (0.0, 0.0), 0.0
    from eigd_amd.device import CSRMatrix

    Ud = CSRMatrix(ctx, symmetrised_of(U))
    for kb in case.widths:
        B = rng.normal(size=(n, kb))
        Bd = ctx.from_host(B)
        Xd = ctx.empty(n, kb)
        with F.sweep_record() as rec:
            F.solve_to(Bd, Xd)
        launched |= {(v, l) for v, l, _ in rec}
        _, raw = forward_backward(U, Xd.get(), B, B)  # the factor alone: refinement would hide a slightly wrong one
        if st["static_pivots"] == 0:
            assert raw < RAW_BWD_TOL, (kb, raw)
        worst_raw = max(worst_raw, raw)
        F.refine(Ud, Bd, Xd, steps=F.STATIC_PIVOT_REFINEMENTS if st["static_pivots"] else 1)
        X = Xd.get()
        _, bwd = forward_backward(U, X, B, X)
        assert bwd < BWD_TOL, (kb, bwd)
        worst = (worst[0], max(worst[1], bwd))
        if lu0 is not None:
            m0 = U0.shape[0]
            reps = case.replicas if s is not None else 1
            step = max(1, reps // 64)
            for r in range(0, reps, step):
                sl = slice(r * m0, (r + 1) * m0)
                Xr = lu0.solve(B[sl]) / (s[r] if s is not None else 1.0)
                fwd = np.max(np.linalg.norm(X[sl] - Xr, axis=0) / np.linalg.norm(Xr, axis=0))
                assert fwd < FWD_TOL, (kb, r, fwd)
                worst = (max(worst[0], fwd), worst[1])
    print(f"{case.name}: forward {worst[0]:.1e} backward {worst[1]:.1e} unrefined backward {worst_raw:.1e}")
    for v, lvl in case.targets:
        v = lu_target(v)
        assert any(v == lv and (lvl is None or lvl == ll) for lv, ll in launched), (v, lvl)


def symmetrised_of(A):
    from eigd_amd.device import symmetrised_pattern

    return symmetrised_pattern(A)


def test_bitwise_invariants(ctx):
    from eigd_amd.device import Factor

    mat = convection_diffusion_2d(70, 66)
    n = mat.shape[0]
    F = Factor(ctx, mat, leaf_size=32, lu=True)
    rng = np.random.default_rng(3)
    B = rng.normal(size=(n, 64))
    ref = F.solve_to(ctx.from_host(B), ctx.empty(n, 64)).get()
    # a column's result does not depend on the sweep width or on its position in the block
    for k in (1, 5, 16, 17, 32, 33):
        for c0 in (0, 64 - k):
            X = F.solve_to(ctx.from_host(np.ascontiguousarray(B[:, c0:c0 + k])), ctx.empty(n, k)).get()
            assert np.array_equal(X, ref[:, c0:c0 + k]), (k, c0)
    # a lane solve equals a solve on the factor's own stream
    other = ctx.fork(1)
    Xo = other.empty(n, 64)
    F.solve_to(other.from_host(B), Xo)
    other.sync()
    assert np.array_equal(Xo.get(), ref)
    # refactor with new values on the same pattern equals a freshly created factor
    mat2 = mat.copy()
    mat2.data = mat2.data * rng.uniform(0.9, 1.1, size=mat2.nnz)
    F.refactor(mat2)
    G = Factor(ctx, mat2, symbolic=F.symbolic, lu=True)
    X1 = F.solve_to(ctx.from_host(B), ctx.empty(n, 64)).get()
    X2 = G.solve_to(ctx.from_host(B), ctx.empty(n, 64)).get()
    assert np.array_equal(X1, X2)
    assert not np.array_equal(X1, ref)


def test_lu_agrees_with_cholesky_on_spd(ctx):
    import eigd_amd as eg

    A = grid_matrix(40, 36, 2, seed=9)
    n = A.shape[0]
    B = np.random.default_rng(1).normal(size=(n, 8))
    chol = eg.SpLuOperator(A.tocsc(), ctx=ctx)
    lu = eg.SpLuOperator(A.tocsc(), ctx=ctx, symmetric=False)
    assert chol.kind == "ldlt" and lu.kind == "lu"
    assert chol.negative_pivots == 0 and lu.negative_pivots is None
    assert relerr(lu(B), chol(B)) < 1e-12


def test_surface(ctx):
    import eigd_amd as eg

    mat = convection_diffusion_2d(30, 30)
    n = mat.shape[0]
    with pytest.raises(ValueError, match="symmetric"):
        eg.SpLuOperator(mat.tocsc(), ctx=ctx)
    op = eg.SpLuOperator(mat.tocsc(), ctx=ctx, symmetric=False)
    lu = splu(mat.tocsc())
    rng = np.random.default_rng(4)
    b = rng.normal(size=n)
    x = op(b)
    assert x.shape == (n,) and op.count == 1
    assert relerr(x, lu.solve(b)) < FWD_TOL
    Bm = rng.normal(size=(n, 3))
    assert relerr(op(Bm), lu.solve(Bm)) < FWD_TOL and op.count == 4
    assert relerr(op @ b, lu.solve(b)) < FWD_TOL
    # complex (complex-step) matrix: the dual-number path with the real LU factor, against splu of the complex matrix
    dM = sparse.random(n, n, density=4.0 / n, random_state=2, format="csr") + sparse.identity(n)
    cmat = (mat + 1e-20j * dM).tocsc()
    cop = eg.SpLuOperator(cmat, ctx=ctx, symmetric=False)
    assert cop.dtype == np.complex128
    bc = rng.normal(size=n) + 1j * rng.normal(size=n)
    xr = splu(cmat).solve(bc)
    xc = cop(bc)
    assert relerr(xc.real, xr.real) < FWD_TOL and relerr(xc.imag, xr.imag) < 1e-9
    # an exactly singular matrix
    sing = mat.tolil()
    sing[5, :] = 0.0
    sing = sing.tocsr()
    sing.eliminate_zeros()
    with pytest.raises(np.linalg.LinAlgError):
        eg.SpLuOperator(sing.tocsc(), ctx=ctx, symmetric=False)


@pytest.mark.parametrize("name,solver", [("g1_buckling50_iram", "IRAM"), ("g1_buckling50_basiclanczos", "BasicLanczos"),
                                         ("g4_laplace900_iram", "IRAM"), ("g4_laplace900_basiclanczos", "BasicLanczos")])
def test_end_to_end_adjoint_on_golden(name, solver):
    """the recorded solver + sibk with the shifted matrix factored by LU (no inertia: the Arnoldi form of sibk)"""
    import warnings

    import eigd_amd as eg

    g = load_golden(name)
    if name.startswith("g1"):
        K, G = csr_from(g, "K"), csr_from(g, "G")
        sigma = float(g["sigma"])
        A, B, mat, mode, p, rhs, ref, rtol = G, K, K + sigma * G, "buckling", "", "Qrb", "psir", 1e-10
    else:
        K, M = csr_from(g, "K"), csr_from(g, "M")
        p = "normal_"
        sigma = float(g[p + "sigma"])
        A, B, mat, mode, rhs, ref, rtol = K, M, K - sigma * M, "normal", "Phib", p + "sibk_psi", 1e-12
    factor = eg.SpLuOperator(mat.tocsc(), symmetric=False)
    assert factor.kind == "lu" and factor.refined   # (adjoint._short_recurrence_applies: False)
    if solver == "IRAM":
        s = eg.IRAM(N=6, m=60 if mode == "buckling" else 40, mode=mode)
    else:
        s = eg.BasicLanczos(mode=mode, N=6, m=60, **({"tol": 0.0} if mode == "buckling" else {}))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lam, Phi = s.solve(A, B, factor, sigma)
    assert relerr(lam, g[p + "lam"]) < 1e-8
    _, sg = align_signs(Phi, g[p + "Phi"])
    psi, _ = s.solve_adjoint(g[rhs] * sg, method="sibk", rtol=rtol, update_guess=False, bs_target=1)
    assert relerr(psi * sg, g[ref]) < 1e-8
