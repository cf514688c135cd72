"""
Host-side checks of the transposed solves (SpLuOperator.T / .H / rmatvec / rmatmat): the C boundary declares the new
entries and the ctypes layer mirrors them, the transpose permutation behind ``CSRMatrix.transposed()`` agrees with
scipy, the operator defines what scipy's LinearOperator builds ``.T`` and ``.H`` on, and the host formula that the
end-to-end GPU test (test_gpu_lu_transposed.py) is gated against is itself right: the adjoint gradient of
``J = c^T u``, ``A(x) u = f`` against central differences.
"""
import os
import re

import numpy as np
from scipy import sparse
from scipy.sparse.linalg import splu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRIES = ("eigd_factor_solve_transposed_to", "eigd_factor_lane_solve_transposed_to", "eigd_csr_transpose_pattern",
               "eigd_csr_transpose", "eigd_csr_transpose_refresh")


def declared_arguments(name):
    """the argument types of ``name`` as include/eigd_hip.h declares them, as ctypes types"""
    from eigd_amd import _ffi

    text = open(os.path.join(ROOT, "include", "eigd_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared"
    out = []
    for arg in m.group(1).split(","):
        typ = " ".join(arg.split()[:-1]) if "*" not in arg else arg[: arg.rindex("*") + 1]
        typ = typ.replace("const", "").replace(" ", "")
        if typ.endswith("**"):
            out.append(_ffi.P(_ffi.c_vp))
        elif typ.endswith("*"):
            out.append(_ffi.c_vp)
        else:
            out.append({"int": _ffi.c_int, "double": _ffi.c_dbl, "int64_t": _ffi.c_i64, "size_t": _ffi.c_sz}[typ])
    return out


def test_new_entries_are_declared_bound_and_exported():
    from eigd_amd import _ffi

    L = _ffi.lib()
    for name in NEW_ENTRIES:
        assert _ffi._SIGNATURES[name] == declared_arguments(name), name
        assert hasattr(L, name), name
    # the transposed solves take what the untransposed ones take
    assert _ffi._SIGNATURES["eigd_factor_solve_transposed_to"] == _ffi._SIGNATURES["eigd_factor_solve_to"]
    assert _ffi._SIGNATURES["eigd_factor_lane_solve_transposed_to"] == _ffi._SIGNATURES["eigd_factor_lane_solve_to"]
    # (the parser reads the existing declarations the way the binding states them)
    for name in ("eigd_factor_solve_to", "eigd_csr_upload_rect", "eigd_factor_lane_create"):
        assert _ffi._SIGNATURES[name] == declared_arguments(name), name


def transpose_pattern(A):
    from eigd_amd import _ffi

    n, ncols = A.shape
    ip = np.ascontiguousarray(A.indptr, dtype=np.int32)
    ix = np.ascontiguousarray(A.indices, dtype=np.int32)
    tip = np.full(ncols + 1, -7, dtype=np.int32)
    tix = np.full(max(A.nnz, 1), -7, dtype=np.int32)
    perm = np.full(max(A.nnz, 1), -7, dtype=np.int32)
    _ffi.call("eigd_csr_transpose_pattern", n, ncols, _ffi.hptr(ip), _ffi.hptr(ix), _ffi.hptr(tip), _ffi.hptr(tix),
              _ffi.hptr(perm))
    return tip, tix[:A.nnz], perm[:A.nnz]


def unsymmetric_with_empty_lines(n=157, seed=3):
    """structurally unsymmetric, with empty rows, empty columns and a row that is empty in A and in A^T"""
    rng = np.random.default_rng(seed)
    A = sparse.random(n, n, density=0.04, random_state=seed, format="lil")
    A.setdiag(rng.uniform(1.0, 2.0, size=n))
    for r in (0, 11, n // 2, n - 1):
        A[r, :] = 0.0
    for c in (5, 11, n - 3):
        A[:, c] = 0.0
    A = A.tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    assert np.any(np.diff(A.indptr) == 0) and np.any(np.diff(A.T.tocsr().indptr) == 0)
    assert (abs(A) > 0).astype(int).__ne__((abs(A.T) > 0).astype(int)).nnz > 0
    return A


def test_transpose_permutation_against_scipy():
    from eigd_amd import _ffi

    for A in (unsymmetric_with_empty_lines(), unsymmetric_with_empty_lines(64, seed=5),
              sparse.random(40, 40, density=0.1, random_state=1, format="csr")):
        A.sort_indices()
        At = A.T.tocsr()
        tip, tix, perm = transpose_pattern(A)
        assert np.array_equal(tip, At.indptr) and np.array_equal(tix, At.indices)
        assert np.array_equal(A.data[perm], At.data)
        assert np.array_equal(np.sort(perm), np.arange(A.nnz))
    # rectangular patterns too (the host routine is general; the device companion is for square matrices)
    R = sparse.random(30, 50, density=0.1, random_state=2, format="csr")
    R.sort_indices()
    tip, tix, perm = transpose_pattern(R)
    Rt = R.T.tocsr()
    assert np.array_equal(tip, Rt.indptr) and np.array_equal(tix, Rt.indices) and np.array_equal(R.data[perm], Rt.data)
    # a column index out of range is refused
    bad_ip, bad_ix = np.array([0, 1], dtype=np.int32), np.array([3], dtype=np.int32)
    out = np.zeros(4, dtype=np.int32)
    rc = _ffi.lib().eigd_csr_transpose_pattern(1, 1, _ffi.hptr(bad_ip), _ffi.hptr(bad_ix), _ffi.hptr(out), _ffi.hptr(out),
                                               _ffi.hptr(out))
    assert rc == _ffi.EIGD_E_INVALID


def test_operator_defines_the_adjoint_surface():
    import inspect

    from scipy.sparse.linalg import LinearOperator

    import eigd_amd as eg
    from eigd_amd.device import CSRMatrix, Factor

    for name in ("_rmatvec", "_rmatmat", "_adjoint"):
        assert name in eg.SpLuOperator.__dict__, name
        assert getattr(eg.SpLuOperator, name) is not getattr(LinearOperator, name)
    for fn in (eg.SpLuOperator.solve_device, eg.SpLuOperator.solve_device_to, Factor.solve_to, Factor.solve_inplace,
               Factor.refine):
        assert inspect.signature(fn).parameters["trans"].default is False, fn
    assert callable(CSRMatrix.transposed)


class ConvectionDesign:
    """
    The state equation of the end-to-end test: A(x) u = f on convection_diffusion_2d's nx x ny grid,
    A(x) = D + sum_e x_e C_e with D the 5-point diffusion and one design variable per grid line -- x_e the strength of
    the first-order upwinded convection along line e (ny lines in x, then nx lines in y).  J = c^T u;
    dJ/dx_e = -psi^T C_e u with A^T psi = c.
    """

    def __init__(self, nx, ny, seed=0):
        self.nx, self.ny = nx, ny
        self.n = nx * ny
        lap = lambda m: sparse.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))  # noqa: E731
        self.Gx = sparse.diags([-1.0, 1.0], [-1, 0], shape=(nx, nx)).tocsr()  # upwind difference along a line
        self.Gy = sparse.diags([-1.0, 1.0], [-1, 0], shape=(ny, ny)).tocsr()
        self.D = (sparse.kron(sparse.identity(ny), lap(nx)) + sparse.kron(lap(ny), sparse.identity(nx))).tocsr()
        rng = np.random.default_rng(seed)
        self.f = rng.normal(size=self.n)
        self.c = rng.normal(size=self.n)
        self.x0 = rng.uniform(0.2, 1.0, size=ny + nx)

    def matrix(self, x):
        xs, ys = x[:self.ny], x[self.ny:]
        A = self.D + sparse.kron(sparse.diags(xs), self.Gx) + sparse.kron(self.Gy, sparse.diags(ys))
        A = A.tocsr()
        A.sort_indices()
        return A

    def gradient(self, u, psi):
        """g_e = -psi^T C_e u for every line e (grid arrays: row j is the j-th line in x)"""
        U, P = u.reshape(self.ny, self.nx), psi.reshape(self.ny, self.nx)
        gx = -np.einsum("ji,ji->j", P, (self.Gx @ U.T).T)
        gy = -np.einsum("ji,ji->i", P, self.Gy @ U)
        return np.concatenate([gx, gy])

    def host_gradient(self, x):
        lu = splu(self.matrix(x).tocsc())
        u = lu.solve(self.f)
        return self.c @ u, self.gradient(u, lu.solve(self.c, "T"))


def test_host_adjoint_gradient_against_central_differences():
    """
    The yardstick of the end-to-end GPU test.  Central differences of J along a random direction at steps h and h / 2:
    their distance to the adjoint gradient must fall by the factor of four of a second-order quotient (within a factor
    of two of it) -- a wrong gradient leaves a distance that does not move with h.
    """
    model = ConvectionDesign(30, 26, seed=4)
    x = model.x0
    J0, g = model.host_gradient(x)
    assert np.isfinite(J0)
    # the matrix is convection_diffusion_2d's for constant strengths
    from test_gpu_lu import convection_diffusion_2d

    xc = np.concatenate([np.full(model.ny, 0.8), np.full(model.nx, 0.4)])
    assert abs(model.matrix(xc) - convection_diffusion_2d(30, 26)).max() < 1e-14
    d = np.random.default_rng(9).normal(size=x.size)
    J = lambda y: model.host_gradient(y)[0]  # noqa: E731
    err = []
    for h in (2e-2, 1e-2):
        fd = (J(x + h * d) - J(x - h * d)) / (2.0 * h)
        err.append(abs(fd - g @ d) / abs(g @ d))
    print(f"central differences: relative distance {err[0]:.2e} at h, {err[1]:.2e} at h/2, ratio {err[0] / err[1]:.2f}")
    assert 2.0 < err[0] / err[1] < 8.0
