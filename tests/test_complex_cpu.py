"""
Host side of the full complex path of SpLuOperator (no device): the real-equivalent builders against scipy.sparse.bmat
and the interleaving permutation, the split layout, the expansion tables, the two identities the operator rests on
(with SuperLU standing in for the factor), the path selection rule and the new ABI symbols.

Finding recorded here (test_scipy_product_is_the_restatement): scipy's complex ``A @ X`` equals the host restatement of
the device product -- CSR order per row, separate real and imaginary accumulators, products (ar xr) - (ai xi) and
(ar xi) + (ai xr) with every operation rounded on its own -- bit for bit on the three test matrices, at 1, 4, 32 and 33
columns.  The GPU tests therefore gate the complex product on scipy directly, as the real kernels are, and on the
restatement where alpha and beta come in.
"""
import types

import numpy as np
import pytest
from scipy import sparse
from scipy.sparse.linalg import splu

from test_gpu_lu import convection_diffusion_2d, structurally_unsymmetric

NX, NY = 60, 52


def complex_matrices():
    """the three genuinely complex matrices of the issue (n = 3120); the first is complex symmetric"""
    K = convection_diffusion_2d(NX, NY, peclet=0.0)       # the 5-point Laplacian of the grid
    cd = convection_diffusion_2d(NX, NY)
    I = sparse.identity(NX * NY, format="csr")
    return {
        "damped": (K - 0.37 * I + 1j * (0.05 * K + 0.02 * I)).tocsr(),
        "complex_shift": (cd - (0.4 + 0.3j) * I).tocsr(),
        "complex_convection": (0.1 * cd + 1j * convection_diffusion_2d(NX, NY, peclet=0.3)).tocsr(),
    }


def restated_product(A, X, alpha=1.0, beta=0.0, Y=None):
    """alpha A X + beta Y in the order of the device kernel (see the module docstring); A complex CSR, X complex (n, k)"""
    A = sparse.csr_matrix(A).astype(np.complex128)
    A.sort_indices()
    X = np.asarray(X, dtype=np.complex128).reshape(A.shape[1], -1)
    ip, ix, ar, ai = A.indptr, A.indices, A.data.real.copy(), A.data.imag.copy()
    xr, xi = X.real.copy(), X.imag.copy()
    ln = np.diff(ip)
    sr, si = np.zeros((A.shape[0], X.shape[1])), np.zeros((A.shape[0], X.shape[1]))
    for p in range(int(ln.max()) if ln.size else 0):
        rows = np.flatnonzero(ln > p)
        e = ip[rows] + p
        a, b, c = ar[e][:, None], ai[e][:, None], ix[e]
        p0, p1, p2, p3 = a * xr[c], b * xi[c], a * xi[c], b * xr[c]
        pr = p0 - p1
        pi = p2 + p3
        sr[rows] = sr[rows] + pr
        si[rows] = si[rows] + pi
    if beta == 0.0:
        return alpha * sr + 1j * (alpha * si)
    Y = np.asarray(Y, dtype=np.complex128).reshape(sr.shape)
    t0, t1 = alpha * sr, beta * Y.real
    u0, u1 = alpha * si, beta * Y.imag
    return (t0 + t1) + 1j * (u0 + u1)


def interleaving(n):
    """P with (P v)[2 i] = v[i], (P v)[2 i + 1] = v[n + i]: from (all real parts, all imaginary parts) to interleaved"""
    src = np.empty(2 * n, dtype=np.int64)
    src[0::2], src[1::2] = np.arange(n), n + np.arange(n)
    return sparse.csr_matrix((np.ones(2 * n), (np.arange(2 * n), src)), shape=(2 * n, 2 * n))


def small_complex(seed=0, unsym_pattern=False):
    rng = np.random.default_rng(seed)
    A = structurally_unsymmetric(9, 8, seed=seed + 1) if unsym_pattern else convection_diffusion_2d(9, 8)
    A = A.tocsr()
    A.sort_indices()
    data = A.data * rng.uniform(0.5, 1.5, size=A.nnz) + 1j * rng.normal(size=A.nnz)
    data[::7] = data[::7].real          # some purely real entries: stored zeros in the imaginary blocks
    return sparse.csr_matrix((data, A.indices, A.indptr), shape=A.shape)


@pytest.mark.parametrize("unsym_pattern", [False, True])
def test_builders_against_bmat(unsym_pattern):
    from eigd_amd.device import real_equivalent

    A = small_complex(3, unsym_pattern)
    n = A.shape[0]
    Ar, Ai = A.real.tocsr(), A.imag.tocsr()
    P = interleaving(n)
    for form, blocks in (("lu", [[Ar, -Ai], [Ai, Ar]]), ("symmetric", [[Ar, -Ai], [-Ai, -Ar]])):
        want = (P @ sparse.bmat(blocks, format="csr") @ P.T).toarray()
        R = real_equivalent(A, form)
        assert R.shape == (2 * n, 2 * n) and R.nnz == 4 * A.nnz and R.has_sorted_indices
        assert np.array_equal(R.toarray(), want)
        if form == "symmetric" and not unsym_pattern:
            S = sparse.csr_matrix((A + A.T) / 2)        # complex symmetric -> symmetric real-equivalent matrix
            Rs = real_equivalent(S, form)
            assert abs(Rs - Rs.T).max() == 0.0
    # the solution of the real-equivalent system is the complex one, interleaved
    rng = np.random.default_rng(1)
    b = rng.normal(size=n) + 1j * rng.normal(size=n)
    x = splu(A.tocsc()).solve(b)
    bi = np.ravel(np.column_stack([b.real, b.imag]))
    xi = splu(real_equivalent(A, "lu").tocsc()).solve(bi)
    assert np.linalg.norm(xi[0::2] + 1j * xi[1::2] - x) < 1e-13 * np.linalg.norm(x)


def test_split_layout_is_the_interleaved_block():
    from eigd_amd.device import complex_join, complex_split

    rng = np.random.default_rng(2)
    for shape in ((7,), (7, 1), (7, 5)):
        x = rng.normal(size=shape) + 1j * rng.normal(size=shape)
        Z = complex_split(x)
        k = 1 if len(shape) == 1 else shape[1]
        assert Z.shape == (7, 2 * k) and Z.dtype == np.float64 and Z.flags.c_contiguous
        assert np.array_equal(complex_join(Z), x.reshape(7, k))
        # (n, 2k) row-major is (2n, k) row-major with interleaved rows re_0, im_0, re_1, ...
        V = Z.reshape(14, k)
        assert np.shares_memory(V, Z)
        assert np.array_equal(V[0::2], x.reshape(7, k).real) and np.array_equal(V[1::2], x.reshape(7, k).imag)
    Zr = complex_split(rng.normal(size=(7, 3)))        # a real right-hand side: zero imaginary half
    assert np.array_equal(Zr[:, 3:], np.zeros((7, 3)))


@pytest.mark.parametrize("unsym_pattern", [False, True])
def test_expansion_tables(unsym_pattern):
    from eigd_amd.device import expand_values_host, real_equivalent, real_equivalent_pattern
    from eigd_amd.operators import SpLuOperator

    A = small_complex(5, unsym_pattern)
    n = A.shape[0]
    for form in ("lu", "symmetric"):
        ip2, ix2, table = real_equivalent_pattern(A.indptr, A.indices, form)
        R = real_equivalent(A, form)
        assert np.array_equal(ip2, R.indptr) and np.array_equal(ix2, R.indices)
        assert table.dtype == np.int32 and table.min() >= 0 and (table >> 2).max() == A.nnz - 1
        assert np.array_equal(expand_values_host(table, A.data), R.data)
        new = A.data * (1.5 - 0.25j)
        R2 = real_equivalent(sparse.csr_matrix((new, A.indices, A.indptr), shape=A.shape), form)
        assert np.array_equal(expand_values_host(table, new), R2.data)
    # the operator's own tables: on the pattern the factor is analysed on (symmetrised / with every diagonal entry)
    for symmetric in (False, True):
        B = A.tolil()
        B[3, 3] = 0.0
        B = B.tocsr()
        B.eliminate_zeros()
        B.sort_indices()
        req, table = SpLuOperator._real_equivalent_of(types.SimpleNamespace(symmetric=symmetric), B)
        assert np.array_equal(req.toarray(), real_equivalent(B, "symmetric" if symmetric else "lu").toarray())
        assert np.array_equal(expand_values_host(table, B.data), req.data)
        assert req.diagonal().shape == (2 * n,) and (table < 0).any()
        pat = sparse.csr_matrix((np.ones(req.nnz), req.indices, req.indptr), shape=req.shape)
        assert np.all(pat.diagonal() == 1.0)
        if not symmetric:
            assert abs(pat - pat.T).max() == 0.0


@pytest.mark.parametrize("name", ["damped", "complex_shift", "complex_convection"])
def test_identities_with_superlu(name):
    """the transposed real-equivalent solve is the complex 'H' solve; the symmetric form solves (br, -bi)"""
    from eigd_amd.device import complex_join, complex_split, real_equivalent

    A = complex_matrices()[name]
    n = A.shape[0]
    rng = np.random.default_rng(7)
    b = rng.normal(size=(n, 3)) + 1j * rng.normal(size=(n, 3))
    lu_c = splu(A.tocsc())
    lu_r = splu(real_equivalent(A, "lu").tocsc())
    V = complex_split(b).reshape(2 * n, 3)
    rel = lambda x, y: np.linalg.norm(x - y) / np.linalg.norm(y)  # noqa: E731
    assert rel(complex_join(lu_r.solve(V).reshape(n, 6)), lu_c.solve(b)) < 1e-13
    assert rel(complex_join(lu_r.solve(V, "T").reshape(n, 6)), lu_c.solve(b, "H")) < 1e-13
    xt = np.conj(complex_join(lu_r.solve(complex_split(np.conj(b)).reshape(2 * n, 3), "T").reshape(n, 6)))
    assert rel(xt, lu_c.solve(b, "T")) < 1e-13
    if name == "damped":
        assert abs(A - A.T).max() == 0.0
        lu_s = splu(real_equivalent(A, "symmetric").tocsc())
        Z = complex_split(b)
        Z[:, 3:] *= -1.0
        assert rel(complex_join(lu_s.solve(Z.reshape(2 * n, 3)).reshape(n, 6)), lu_c.solve(b)) < 1e-13
        # mat^{-H} of a complex symmetric matrix: the conjugations cancel the sign of the form, the result is conjugated
        Y = lu_s.solve(complex_split(b).reshape(2 * n, 3)).reshape(n, 6)
        Y[:, 3:] *= -1.0
        assert rel(complex_join(Y), lu_c.solve(b, "H")) < 1e-13


@pytest.mark.parametrize("name", ["damped", "complex_shift", "complex_convection"])
def test_scipy_product_is_the_restatement(name):
    A = complex_matrices()[name]
    n = A.shape[0]
    rng = np.random.default_rng(9)
    for k in (1, 4, 32, 33):
        X = rng.normal(size=(n, k)) + 1j * rng.normal(size=(n, k))
        assert np.array_equal(restated_product(A, X), A @ X), k
        assert np.array_equal(restated_product(A.conj().T.tocsr(), X), A.conj().T.tocsr() @ X), k


def test_auto_rule(monkeypatch):
    import eigd_amd.tuning as tuning
    from eigd_amd.operators import select_complex_arithmetic

    assert tuning.complex_step_ratio == 1e-12
    re = np.array([1.0, -3.0, 0.5])
    for ratio, want in ((0.0, "dual"), (1e-20, "dual"), (1e-13, "dual"), (1e-11, "full"), (1.0, "full")):
        data = re + 1j * ratio * np.array([0.2, 3.0, -1.0])
        assert select_complex_arithmetic(data) == want, ratio
        assert select_complex_arithmetic(data, "dual") == "dual" and select_complex_arithmetic(data, "full") == "full"
    with pytest.raises(ValueError):
        select_complex_arithmetic(re + 0j, "native")
    monkeypatch.setattr(tuning, "complex_step_ratio", 1e-10)
    assert select_complex_arithmetic(re + 1e-11j * re) == "dual"


def test_new_abi_symbols():
    from eigd_amd import _ffi

    L = _ffi.lib()
    for name in ("eigd_ccsr_upload", "eigd_ccsr_update_values_dev", "eigd_ccsr_conjugate_transpose",
                 "eigd_ccsr_conjugate_transpose_refresh", "eigd_ccsr_spmm_on", "eigd_expand_values"):
        assert name in _ffi.EXPORTED and hasattr(L, name), name
    assert L.eigd_ccsr_upload(None, 3, 0, None, None, None, None) == _ffi.EIGD_E_INVALID
    assert "null" in _ffi.last_error()
    assert L.eigd_expand_values(None, 0, 0, None, None, None) == _ffi.EIGD_E_INVALID
