"""
Host logic of the un-restarted Lanczos eigensolver -- eigd_amd.lanczos.basic_lanczos_recurrence -- on numpy stand-ins for
the two device bases (same protocol as _LanczosDevice and _DualLanczosDevice): the calls it issues, step by step, in
both arithmetics and both orthogonalisations; its coefficients and eigenvalues against the oracle's BasicLanczos and, in
dual-number arithmetic, against the reference's own complex-step run (G6); early exit and the widening of N.
"""
import warnings

import numpy as np
import pytest
from scipy import sparse
from scipy.sparse.linalg import splu

from conftest import csr_from, load_golden, relerr
from eigd_amd.lanczos import basic_lanczos_recurrence, reduced_problem, wanted_pairs
from oracle import eigd_oracle as orc


class NumpyBasis:
    """real arithmetic: classical Gram-Schmidt passes in the B inner product against stored V and B V"""

    dtype = np.float64
    selective_passes = 1

    def __init__(self, B, solve, nvec):
        self.B, self.solve, self.n = sparse.csr_matrix(B), solve, B.shape[0]
        self.V, self.BV = np.zeros((self.n, nvec)), np.zeros((self.n, nvec))
        self.S = None

    def start(self, v0):
        self.v = np.array(v0, dtype=float)
        self.normalize_into(0)

    def apply_op(self, j):
        self.v = self.solve(self.BV[:, j])

    def subtract(self, coef, j):
        self.v -= coef * self.V[:, j]

    def project_out(self, j0, ns, passes):
        tot = np.zeros(ns)
        for _ in range(passes):
            h = self.BV[:, j0:j0 + ns].T @ self.v
            self.v -= self.V[:, j0:j0 + ns] @ h
            tot += h
        return tot

    def lock(self, Yc, m):
        self.S = self.ritz_vectors(Yc, m)
        self.BS = self.B @ self.S

    def unlock(self):
        self.S = None

    def project_locked(self):
        if self.S is not None:
            for _ in range(self.selective_passes):
                self.v -= self.S @ (self.BS.T @ self.v)

    def normalize_into(self, j):
        w = self.B @ self.v
        nrm = float(np.sqrt(self.v @ w))
        self.V[:, j], self.BV[:, j] = self.v / nrm, w / nrm
        return nrm

    def ritz_vectors(self, Y, m):
        return self.V[:, :m] @ Y


class NumpyDualBasis:
    """
    dual numbers as _DualLanczosDevice keeps them: every vector a (value, derivative) pair of real arrays, B = Br + i Bi,
    products without the term of two derivative factors, nothing conjugated.  ``solve`` applies the inverse of the REAL
    part of the shifted matrix, ``Ai`` is its imaginary part: (Ar + i Ai)^-1 (br + i bi) = xr + i Ar^-1 (bi - Ai xr).
    """

    dtype = np.complex128
    selective_passes = 2

    def __init__(self, Br, Bi, solve, Ai, nvec):
        self.Br, self.Bi, self.solve, self.Ai, self.n = sparse.csr_matrix(Br), sparse.csr_matrix(Bi), solve, Ai, Br.shape[0]
        self.Vr, self.Vi = np.zeros((self.n, nvec)), np.zeros((self.n, nvec))
        self.BVr, self.BVi = np.zeros((self.n, nvec)), np.zeros((self.n, nvec))
        self.S = None

    def _apply_B(self, xr, xi):
        return self.Br @ xr, self.Br @ xi + self.Bi @ xr

    def start(self, v0):
        self.vr, self.vi = np.array(v0, dtype=float), np.zeros(self.n)
        self.normalize_into(0)

    def apply_op(self, j):
        xr = self.solve(self.BVr[:, j])
        self.vr, self.vi = xr, self.solve(self.BVi[:, j] - self.Ai @ xr)

    def subtract(self, coef, j):
        self.vi -= coef.real * self.Vi[:, j] + coef.imag * self.Vr[:, j]
        self.vr -= coef.real * self.Vr[:, j]

    @staticmethod
    def _project(vr, vi, Sr, Si, BSr, BSi):
        """one pass v -= S (BS^T v) on pairs; returns the coefficients"""
        hr = BSr.T @ vr
        hi = BSr.T @ vi + BSi.T @ vr
        vi -= Sr @ hi + Si @ hr
        vr -= Sr @ hr
        return hr + 1j * hi

    def project_out(self, j0, ns, passes):
        cols = slice(j0, j0 + ns)
        tot = np.zeros(ns, dtype=complex)
        for _ in range(passes):
            tot += self._project(self.vr, self.vi, self.Vr[:, cols], self.Vi[:, cols], self.BVr[:, cols], self.BVi[:, cols])
        return tot

    def lock(self, Yc, m):
        S = self.ritz_vectors(Yc, m)
        Sr, Si = np.ascontiguousarray(S.real), np.ascontiguousarray(S.imag)
        self.S = (Sr, Si) + self._apply_B(Sr, Si)

    def unlock(self):
        self.S = None

    def project_locked(self):
        if self.S is not None:
            for _ in range(self.selective_passes):
                self._project(self.vr, self.vi, *self.S)

    def normalize_into(self, j):
        wr, wi = self._apply_B(self.vr, self.vi)
        re, im = self.vr @ wr, self.vr @ wi + self.vi @ wr
        br = np.sqrt(re)
        beta = complex(br, 0.5 * im / br)
        cr, ci = 1.0 / br, -beta.imag / (br * br)              # 1 / beta
        self.Vr[:, j], self.Vi[:, j] = cr * self.vr, cr * self.vi + ci * self.vr
        self.BVr[:, j], self.BVi[:, j] = cr * wr, cr * wi + ci * wr
        return beta

    def ritz_vectors(self, Y, m):
        Y = np.asarray(Y, dtype=complex)
        return self.Vr[:, :m] @ Y.real + 1j * (self.Vr[:, :m] @ Y.imag + self.Vi[:, :m] @ Y.real)


def real_basis(A, B, sigma, mode, nvec):
    """stand-in basis for real A x = lam B x with the reference's shifted matrix of ``mode``"""
    return NumpyBasis(B, splu(((A - sigma * B) if mode == "normal" else (B + sigma * A)).tocsc()).solve, nvec)


def dual_basis(A, B, sigma, nvec):
    """stand-in basis for a complex-step buckling pencil (shifted matrix B + sigma A)"""
    def parts(X):
        X = sparse.csc_matrix(X)
        return [sparse.csc_matrix((d.copy(), X.indices, X.indptr), shape=X.shape) for d in (X.data.real, X.data.imag)]

    (Ar, Ai), (Br, Bi) = parts(B + sigma * A), parts(B)
    return NumpyDualBasis(Br, Bi, splu(Ar).solve, Ai.tocsr(), nvec)


class Recording:
    """logs the protocol calls of a basis: name and the arguments that say WHICH vectors (no coefficient values)"""

    def __init__(self, basis):
        self.basis, self.calls = basis, []
        self.dtype, self.n, self.selective_passes = basis.dtype, basis.n, basis.selective_passes

    def _log(self, name, *args):
        self.calls.append((name,) + args)
        return getattr(self.basis, name)

    def start(self, v0):
        return self._log("start")(v0)

    def apply_op(self, j):
        return self._log("apply_op", j)(j)

    def subtract(self, coef, j):
        return self._log("subtract", j)(coef, j)

    def project_out(self, j0, ns, passes):
        return self._log("project_out", j0, ns, passes)(j0, ns, passes)

    def lock(self, Yc, m):
        return self._log("lock", Yc.shape[1], m)(Yc, m)

    def unlock(self):
        return self._log("unlock")()

    def project_locked(self):
        return self._log("project_locked")()

    def normalize_into(self, j):
        return self._log("normalize_into", j)(j)


def _expected_calls(ortho, sp):
    """three steps as BasicLanczos.solve and _solve_complex_step issued them before they became one recurrence (sp:
    the selective passes, 1 in real and 2 in dual arithmetic; full orthogonalisation makes 2 passes in both).  With
    tol = 1 every Ritz pair counts as converged for the selective lock (|beta y_last| < sqrt(tol), |beta| < 1 here): the
    i pairs of step i are locked from step 2 on."""
    if ortho == "full":
        return [("start",),
                ("apply_op", 0), ("project_out", 0, 1, 2), ("normalize_into", 1),
                ("apply_op", 1), ("subtract", 0), ("project_out", 0, 2, 2), ("normalize_into", 2),
                ("apply_op", 2), ("subtract", 1), ("project_out", 0, 3, 2), ("normalize_into", 3)]
    return [("start",),
            ("apply_op", 0), ("project_out", 0, 1, sp), ("project_locked",), ("normalize_into", 1),
            ("apply_op", 1), ("subtract", 0), ("project_out", 0, 2, sp), ("project_locked",), ("normalize_into", 2),
            ("lock", 2, 2),
            ("apply_op", 2), ("subtract", 1), ("project_out", 1, 2, sp), ("project_locked",), ("normalize_into", 3),
            ("lock", 3, 3)]


@pytest.mark.parametrize("ortho", ["full", "selective"])
@pytest.mark.parametrize("arith", ["real", "dual"])
def test_protocol_calls_of_three_steps(arith, ortho):
    n = 12
    K = sparse.diags([-1.0, 5.0, -1.0], [-1, 0, 1], shape=(n, n)).tocsr()    # |OP| = |K^-1 M| < 1/3 * 1.5: beta < 1
    M = sparse.diags(np.random.default_rng(0).uniform(0.5, 1.5, size=n)).tocsr()
    if arith == "real":
        basis = real_basis(K, M, 0.0, "normal", 4)
    else:
        basis = NumpyDualBasis(M, 1e-20 * M, splu(K.tocsc()).solve, 1e-20 * K, 4)
    rec = Recording(basis)
    # nchk = 4 > m_max: no early exit, whatever tol admits
    alpha, beta, m = basic_lanczos_recurrence(rec, 3, 4, 1.0, ortho, 0.0, "normal")
    assert rec.calls == _expected_calls(ortho, {"real": 1, "dual": 2}[arith])
    assert m == 3 and alpha.dtype == beta.dtype == basis.dtype and np.all(np.abs(beta) < 1.0)


def _real_case(name):
    """(A, B, sigma, solver parameters of the project's own tests on that fixture)"""
    g = load_golden(name)
    K, M = csr_from(g, "K"), csr_from(g, "M")
    if name.startswith("g4"):
        return K, M, float(g["normal_sigma"]), dict(N=6, m=60)             # (test_g4_method_matrix_basiclanczos)
    return K, M, float(g["sigma"]), dict(N=5, m=60, tol=1e-12)             # (test_selective_orthogonalisation_and_ntarget)


def _oracle_run(K, M, sigma, **kw):
    so = orc.BasicLanczos(**kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        so.solve(K, M, orc.SpLuOperator((K - sigma * M).tocsc()), sigma)
    return so


@pytest.mark.parametrize("name", ["g4_laplace900_basiclanczos", "g3_thermal32_eps1e-8_basiclanczos"])
def test_real_recurrence_against_the_oracle(name):
    K, M, sigma, kw = _real_case(name)
    # full orthogonalisation: the coefficients themselves
    so = _oracle_run(K, M, sigma, **kw)
    alpha, beta, m = basic_lanczos_recurrence(real_basis(K, M, sigma, "normal", kw["m"] + 1), kw["m"], so.N, so.tol, "full",
                                              sigma, "normal")
    scale = np.abs(so.alpha).max()
    print(f"{name} full: m {m} / {so.m}, alpha {np.abs(alpha - so.alpha).max() / scale:.2e}, "
          f"beta {np.abs(beta - so.beta).max() / scale:.2e} of max|alpha|")
    assert m == so.m
    assert np.abs(alpha - so.alpha).max() < 1e-8 * scale and np.abs(beta - so.beta).max() < 1e-8 * scale
    # selective: the eigenvalues (which Ritz pairs are locked when is decided at rounding level)
    kw = dict(kw, tol=1e-12)
    so = _oracle_run(K, M, sigma, ortho_type="selective", **kw)
    alpha, beta, m = basic_lanczos_recurrence(real_basis(K, M, sigma, "normal", kw["m"] + 1), kw["m"], so.N, so.tol,
                                              "selective", sigma, "normal")
    _, _, _, lam, indices = reduced_problem(alpha, beta, m, sigma, "normal")
    print(f"{name} selective: m {m} / {so.m}, lam {relerr(lam[indices[: so.N]], so.lam0):.2e}")
    assert abs(m - so.m) <= 1
    assert relerr(lam[indices[: so.N]], so.lam0) < 1e-7


def test_dual_recurrence_against_the_complex_step_reference():
    from test_oracle_golden import _complex_csr

    g = load_golden("g6_buckling50_complexstep")
    K, G = _complex_csr(g, "K"), _complex_csr(g, "G")
    sigma, mm, N = float(g["sigma"]), 60, int(g["N"])
    alpha, beta, m = basic_lanczos_recurrence(dual_basis(G, K, sigma, mm + 1), mm, N, 0.0, "full", sigma, "buckling")
    _, _, _, lam, indices = reduced_problem(alpha, beta, m, sigma, "buckling")
    lam0 = lam[indices[:N]]
    d_alpha = np.abs(alpha.real - g["alpha"].real).max() / np.abs(g["alpha"].real).max()
    d_re = np.abs(lam0.real - g["lam"].real).max() / np.abs(g["lam"].real).max()
    d_im = np.abs(lam0.imag - g["lam"].imag).max() / np.abs(g["lam"].imag).max()
    print(f"g6 dual: m {m}, alpha.real {d_alpha:.2e}, lam.real {d_re:.2e}, lam.imag {d_im:.2e}")
    assert m == int(g["m"]) and alpha.dtype == np.complex128
    assert d_alpha < 1e-8 and d_re < 1e-8
    assert d_im < 1e-6


def test_early_exit_and_ntarget_widening():
    """Ntarget = 2 ends the recurrence as soon as two pairs pass; N is then widened over the repeated pair behind that cut (ref 1615-1625)"""
    K, M, sigma, _ = _real_case("g3_thermal32_eps1e-8_basiclanczos")
    so = _oracle_run(K, M, sigma, Ntarget=2, m=60, tol=1e-12)
    alpha, beta, m = basic_lanczos_recurrence(real_basis(K, M, sigma, "normal", 61), 60, 2, 1e-12, "full", sigma, "normal")
    assert m == so.m < 60
    _, _, _, lam, indices = reduced_problem(alpha, beta, m, sigma, "normal")
    N = wanted_pairs(lam, indices, m, 10, 2, 1e-5)
    assert N == so.N == 3
