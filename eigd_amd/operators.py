"""
Operator layer: the drop-in ``SpLuOperator`` (reference eigd/eigenvector_derivatives.py:11-23)
and the adapters that let the device drivers apply A, B and ``factor`` to device blocks.
"""

import threading

import numpy as np
from scipy import sparse
from scipy.sparse.linalg import LinearOperator

from . import tuning
from .device import (ComplexCSRMatrix, CSRMatrix, DeviceBlock, Factor, ValueExpansion, complex_join, complex_split,
                     default_context, expand_values_host, interleaved_view, real_equivalent_pattern, refine,
                     symmetrised_pattern)

COMPLEX_ARITHMETIC = ("auto", "dual", "full")


def select_complex_arithmetic(data, requested="auto"):
    """
    the path a complex matrix with the values ``data`` takes: "dual" (a complex-step matrix: the real factor applied to a
    dual number) or "full" (true complex arithmetic).  "auto": "dual" where max|Im| <= tuning.complex_step_ratio max|Re|
    """
    if requested not in COMPLEX_ARITHMETIC:
        raise ValueError(f"complex_arithmetic must be one of {COMPLEX_ARITHMETIC}")
    if requested != "auto":
        return requested
    data = np.asarray(data)
    if data.size == 0:
        return "dual"
    return "dual" if np.max(np.abs(data.imag)) <= tuning.complex_step_ratio * np.max(np.abs(data.real)) else "full"


def _with_structural_diagonal(csr):
    """
    The symbolic analysis needs every diagonal entry stored.  A shift that annihilates one exactly (sigma = K_pp / M_pp:
    scipy's subtraction then drops the entry) is a legitimate interior shift: the entry is put back as an explicit zero.
    """
    n = csr.shape[0]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(csr.indptr))
    have = np.zeros(n, dtype=bool)
    have[rows[rows == csr.indices]] = True
    if have.all():
        return csr
    miss = np.flatnonzero(~have)
    coo = csr.tocoo()
    out = sparse.csr_matrix((np.concatenate([coo.data, np.zeros(len(miss))]),
                             (np.concatenate([coo.row, miss]), np.concatenate([coo.col, miss]))), shape=csr.shape)
    out.sort_indices()
    return out


def _check_symmetric(whole, parts):
    """``parts`` (the real matrix, or the real and the imaginary part of a complex one) against a random vector"""
    x = np.random.default_rng(0).uniform(-1.0, 1.0, size=whole.shape[0])
    for part in parts:
        d = part @ x - part.T @ x
        if np.linalg.norm(d) > 1e-10 * max(np.linalg.norm(whole @ x), 1e-300):
            raise ValueError("SpLuOperator (MI355X) needs a symmetric matrix; pass symmetric=False for an LU factor")


def complex_application(kind, trans, conjugate):
    """
    How a full-complex factor of ``kind`` applies mat^{-1} (``trans``: mat^{-T}; with ``conjugate`` as well: mat^{-H};
    ``conjugate`` alone: conj(mat)^{-1}): (herm, wrap) -- the raw solve is mat^{-H} instead of mat^{-1}; the right-hand
    side is conjugated before and the solution after
    """
    if kind == "lu":
        return bool(trans), bool(trans) != bool(conjugate)      # mat^{-T} = conj o mat^{-H} o conj
    return bool(conjugate), False                               # mat = mat^T


class _Backend:
    """
    What SpLuOperator needs of one arithmetic: the ``factor``, the raw solve with it (``raw``), the ``matrix`` of the
    refinement's residuals (with its adjoint companion), ``refactor`` / ``refactor_device`` and the way of a host array
    through the operator's device surface (``apply_host``).  ``solve`` is the one refined solve over them.
    """

    complex_arithmetic = None
    refined = True                   # (the real backend knows better: a positive definite matrix needs no refinement)
    negative_pivots = negative_pivots_bounds = None     # (no inertia but from a real symmetric factor)

    def _read_factor(self):
        """after every numeric phase: the figures SpLuOperator shows, and how often applications are refined"""
        st = self.factor.stats()
        self.kind, self.row_interchanges = st["kind"], st["row_interchanges"]
        self.static_pivots = st["static_pivots"]   # pivots singular inside their panel block, replaced by +-sqrt(eps)|A|
        self.steps = self.factor.STATIC_PIVOT_REFINEMENTS if self.static_pivots > 0 else 1
        return st

    def solve(self, X, alpha=1.0, Xin=None, adjoint=False):
        """
        X <- alpha mat^{-1} Xin (``Xin`` None: in place; ``adjoint``: with the transposed / conjugate-transposed matrix),
        refined against ``matrix`` where there is one: one step, three with static pivots.  Everything on X's context:
        with concurrent mode groups (streams > 1) X lives on a forked context whose stream and sweep lane must carry
        the whole application
        """
        if self.matrix is None:
            return self.raw(Xin, X, alpha, adjoint)
        B = X.copy() if Xin is None else Xin
        self.raw(Xin, X, alpha, adjoint)
        return refine(lambda R: self.raw(R, R, 1.0, adjoint), self.matrix.adjoint if adjoint else self.matrix, B, X,
                      alpha, self.steps)

    def solve_complex(self, Xr, Xi, trans, conjugate, counted):
        raise TypeError("solve_device_dual needs an operator built on a complex (complex-step) matrix")


class _RealBackend(_Backend):
    """
    The LDL^T or LU factor of a real matrix.  ``matrix`` is None where no refinement is due (a positive definite
    matrix); an indefinite or LU factor pivots inside its panels only, and every application is refined.
    """

    def __init__(self, ctx, csr, request, symmetric, check_symmetry, **analysis):
        self.ctx, self.request = ctx, request
        csr = csr.astype(np.float64)  # for a symmetric matrix CSC and CSR coincide
        csr.sort_indices()
        if symmetric:  # (the LU factor symmetrises the pattern itself; the refinement applies csr as it is)
            csr = _with_structural_diagonal(csr)
            if check_symmetry:
                _check_symmetric(csr, (csr,))
        self.factor = Factor(ctx, csr, lu=not symmetric, **analysis)
        self._read_factor()
        self.matrix = CSRMatrix(ctx, csr) if self.refined else None

    def raw(self, Xin, X, alpha, trans):
        if Xin is None:
            return self.factor.solve_inplace(X, alpha, trans=trans)
        return self.factor.solve_to(Xin, X, alpha, trans=trans)

    def _read_factor(self):
        st = super()._read_factor()
        # (an LU factor pivots inside its panels only: always refined, and it gives no inertia)
        self.refined = self.kind == "lu" or st["negative_pivots"] > 0 or self.static_pivots > 0
        if self.kind != "lu":
            self.negative_pivots = st["negative_pivots"]
            # a static pivot takes its sign from a diagonal entry at rounding level: the inertia is then known only up
            # to their number -- negative_pivots_bounds brackets the count of eigenvalues below the shift
            self.negative_pivots_bounds = (max(0, self.negative_pivots - self.static_pivots),
                                           self.negative_pivots + self.static_pivots)

    def solve(self, X, alpha=1.0, Xin=None, adjoint=False):
        # (a symmetric matrix is its own transpose)
        return super().solve(X, alpha, Xin, bool(adjoint) and self.kind == "lu")

    def refactor(self, mat):
        if np.issubdtype(mat.dtype, np.complexfloating) and select_complex_arithmetic(
                mat.tocsr().data, "dual" if self.request == "dual" else "auto") == "full":
            raise ValueError("this operator was not built for full complex arithmetic: make a new one for this matrix")
        csr = mat.tocsr().astype(np.float64)
        csr.sort_indices()
        self.factor.refactor(csr)
        self._read_factor()
        self.matrix = CSRMatrix(self.ctx, csr) if self.refined else None

    def refactor_device(self, vals, indefinite_matrix):
        self.factor.refactor_device(vals)
        self._read_factor()
        if self.refined and indefinite_matrix is None:
            raise ValueError("indefinite refactorisation: pass the device matrix for the refinement step")
        self.matrix = indefinite_matrix if self.refined else None
        if self.static_pivots > 0:
            self.factor.verify_static_pivots(self.matrix)

    def apply_host(self, op, x, adjoint):
        return op.solve_device(self.ctx.from_host(x.astype(np.float64)), trans=adjoint).get()


class _DualBackend(_RealBackend):
    """
    Complex-step matrices (reference 11-23 with a complex mat): mat = M + i dM with dM ~ 1e-20 M is a dual
    number -- products of two imaginary parts vanish below rounding -- so mat^{-1}(b + i db) = x + i M^{-1}(db - dM x)
    with x = M^{-1} b: the real backend of M, applied twice, and the device matrix of dM.
    """

    complex_arithmetic = "dual"

    def __init__(self, ctx, cm, *args, **analysis):
        self.imag = CSRMatrix(ctx, sparse.csr_matrix((cm.data.imag.copy(), cm.indices, cm.indptr), shape=cm.shape))
        super().__init__(ctx, sparse.csr_matrix((cm.data.real.copy(), cm.indices, cm.indptr), shape=cm.shape), *args,
                         **analysis)

    def solve_complex(self, Xr, Xi, trans, conjugate, counted):
        counted()
        self.solve(Xr, adjoint=trans)
        T = (self.imag.transposed() if trans else self.imag).apply(Xr)
        Xi.assign_lincomb([(1.0, Xi), (1.0 if conjugate else -1.0, T)])
        self.solve(Xi, adjoint=trans)

    def apply_host(self, op, x, adjoint):
        xc = x.astype(np.complex128)
        Xr, Xi = op.solve_device_dual(self.ctx.from_host(np.ascontiguousarray(xc.real)),
                                      self.ctx.from_host(np.ascontiguousarray(xc.imag)), trans=adjoint, conjugate=adjoint)
        return Xr.get() + 1j * Xi.get()


class _FullComplexBackend(_Backend):
    """
    True complex arithmetic through the real-equivalent system of order 2n with interleaved unknowns: the LU factor of
    the form [[a, -b], [b, a]] per entry, or for a complex symmetric matrix the Bunch-Kaufman factor of
    [[a, -b], [-b, -a]].  A complex block is n x 2k (real half, imaginary half): the memory of the 2n x k block the
    factor takes.  Every application is refined against the complex matrix itself (``matrix``).
    """

    complex_arithmetic = "full"

    def __init__(self, ctx, cm, request, symmetric, check_symmetry, coords=None, **analysis):
        self.ctx, self.symmetric = ctx, symmetric
        cm = self._canonical_complex(cm)
        if check_symmetry and symmetric:
            _check_symmetric(cm, (cm.real.tocsr(), cm.imag.tocsr()))
        req, self._table = self._real_equivalent_of(cm)
        self._pattern = (cm.indptr.copy(), cm.indices.copy())
        self._expansion = None
        if coords is not None:  # both unknowns of a dof sit at its node
            coords = np.repeat(np.asarray(coords, dtype=np.float64).reshape(cm.shape[0], -1), 2, axis=0)
        self.factor = Factor(ctx, req, coords=coords, lu=not symmetric, **analysis)
        self._read_factor()
        self.matrix = ComplexCSRMatrix(ctx, cm)

    def _real_equivalent_of(self, cm):
        """(real-equivalent CSR matrix of the canonical complex CSR matrix ``cm``, expansion table): on the pattern the
        factor is analysed on -- symmetrised for the LU form, with every diagonal entry for the symmetric form"""
        n = cm.shape[0]
        # where the entries of cm sit in that pattern: the pattern helpers carry the entry numbers along as values
        numbered = sparse.csr_matrix((np.arange(1.0, cm.nnz + 1.0), cm.indices, cm.indptr), shape=cm.shape)
        padded = _with_structural_diagonal(numbered) if self.symmetric else symmetrised_pattern(numbered)
        source = padded.data.astype(np.int64) - 1
        ip2, ix2, table = real_equivalent_pattern(padded.indptr, padded.indices, "symmetric" if self.symmetric else "lu",
                                                  source)
        return sparse.csr_matrix((expand_values_host(table, cm.data), ix2, ip2), shape=(2 * n, 2 * n)), table

    @staticmethod
    def _canonical_complex(mat):
        cm = sparse.csr_matrix(mat).astype(np.complex128)
        if not cm.has_canonical_format:
            cm = cm.copy()
            cm.sum_duplicates()
        return cm

    def raw(self, Xin, Z, alpha, herm):
        """Z <- alpha mat^{-1} Xin (``herm``: mat^{-H}; ``Xin`` None: Z) with the factor alone, on contiguous split-layout
        blocks: the factor works in place on Z"""
        if Xin is not None and Xin is not Z:
            Z.copy_from(Xin)
        k = Z.k // 2
        im = Z.cols(k, 2 * k)
        V = interleaved_view(Z)
        if not self.symmetric:  # (the transposed real-equivalent matrix is the real-equivalent of mat^H)
            return self.factor.solve_to(V, V, alpha, trans=herm)
        # symmetric form [[Ar, -Ai], [-Ai, -Ar]] (xr, xi) = (br, -bi); mat^{-H} = conj o mat^{-1} o conj for mat = mat^T: the
        # conjugation of the right-hand side and the sign of the form cancel, the solution is conjugated instead
        if not herm:
            im.assign_lincomb([(-1.0, im)])
        self.factor.solve_to(V, V, alpha)
        if herm:
            im.assign_lincomb([(-1.0, im)])
        return Z

    def solve_complex(self, Xr, Xi, trans, conjugate, counted):
        k = Xr.k
        if (Xi.n, Xi.k) != (Xr.n, k) or 2 * Xr.n != self.factor.n:
            raise ValueError("shape mismatch in the complex solve")
        counted()
        halves = Xr.buf is Xi.buf and Xr.ld == Xi.ld == 2 * k and Xi.offset == Xr.offset + k
        if halves:
            Z = DeviceBlock(Xr.ctx, Xr.n, 2 * k, Xr.buf, Xr.offset, 2 * k)
        else:
            Z = Xr.ctx.empty(Xr.n, 2 * k)
            Z.cols(0, k).copy_from(Xr)
            Z.cols(k, 2 * k).copy_from(Xi)
        herm, wrap = complex_application(self.kind, trans, conjugate)
        im = Z.cols(k, 2 * k)
        if wrap:
            im.assign_lincomb([(-1.0, im)])
        self.solve(Z, adjoint=herm)
        if wrap:
            im.assign_lincomb([(-1.0, im)])
        if not halves:
            Xr.copy_from(Z.cols(0, k))
            Xi.copy_from(Z.cols(k, 2 * k))

    def refactor(self, mat):
        if not np.issubdtype(mat.dtype, np.complexfloating):
            raise ValueError("this operator works in full complex arithmetic: refactor it with a complex matrix")
        cm = self._canonical_complex(mat)
        if not (np.array_equal(cm.indptr, self._pattern[0]) and np.array_equal(cm.indices, self._pattern[1])):
            raise ValueError("the complex matrix has a different sparsity pattern")
        req, _ = self._real_equivalent_of(cm)
        self.factor.refactor(req)
        self._read_factor()
        self.matrix = ComplexCSRMatrix(self.ctx, cm)

    def expand_values_device(self, vals):
        if self._expansion is None:
            self._expansion = ValueExpansion(self.ctx, self._table, len(self._pattern[1]))
        return self._expansion.expand(vals)

    def apply(self, X, Y=None):
        """the matrix the factor factors: the real-equivalent one of ``matrix``, applied to 2n x k blocks
        (Factor.verify_static_pivots takes the backend for it)"""
        if Y is None:
            Y = X.ctx.empty(X.n, X.k)
        Y2 = DeviceBlock(Y.ctx, Y.n // 2, 2 * Y.k, Y.buf, Y.offset, 2 * Y.k)
        self.matrix.apply(DeviceBlock(X.ctx, X.n // 2, 2 * X.k, X.buf, X.offset, 2 * X.k), Y2)
        if self.symmetric:  # (its second block row is the negated one)
            im = Y2.cols(Y.k, 2 * Y.k)
            im.assign_lincomb([(-1.0, im)])
        return Y

    def refactor_device(self, vals, indefinite_matrix):
        if indefinite_matrix is not None and not isinstance(indefinite_matrix, ComplexCSRMatrix):
            raise TypeError("full complex arithmetic: the refinement needs a ComplexCSRMatrix")
        self.factor.refactor_device(self.expand_values_device(vals))
        self._read_factor()
        if indefinite_matrix is not None:
            self.matrix = indefinite_matrix
        else:                        # (every application is refined: the operator's own matrix takes the new values)
            self.matrix.update_values_device(vals)
        if self.static_pivots > 0:
            self.factor.verify_static_pivots(self)

    def apply_host(self, op, x, adjoint):
        Z = self.ctx.from_host(complex_split(x))
        op.solve_device_dual(Z.cols(0, Z.k // 2), Z.cols(Z.k // 2, Z.k), trans=adjoint, conjugate=adjoint)
        return complex_join(Z.get())


class SpLuOperator(LinearOperator):
    """
    Shift-invert operator ``x -> mat^{-1} x`` factored and applied on the MI355X.

    Same surface as the reference class (``shape``, ``dtype``, ``count``, callable on
    ``(n,)`` and ``(n, k)`` numpy arrays).  By default ``mat`` must be symmetric (``symmetric=False``: any square
    matrix, see below).  The factorisation is
    ``P mat P^T = L S L^T`` with ``S = diag(+-1)``: plain Cholesky for the positive definite
    shifts of the reference's examples (K - sigma M below the spectrum, K + sigma G below the
    first buckling load); for a shift inside the spectrum (the reference's CRM example, sigma = omega_0^2) the numeric
    phase is repeated with Bunch-Kaufman pivoting (1 x 1 and 2 x 2 pivots, interchanges inside the 64-column panel of
    a front, so the symbolic structure is kept; ``negative_pivots`` = number of eigenvalues of the pencil below the
    shift) and every application is followed by one step of iterative refinement.  Pivots are not delayed to the parent
    front; a column that is singular inside its panel block -- a front whose own block is singular by itself, which
    SuperLU's partial pivoting over whole columns survives -- gets a static pivot of +-sqrt(eps) |mat| instead
    (``static_pivots`` counts them; SuperLU_DIST and PARDISO do the same) and every application is then refined three
    times against the true matrix.  A matrix that is singular to working precision as a whole is told apart by one
    refined solve of a random system at factorisation time and raises ``NotPositiveDefiniteError`` (a
    ``numpy.linalg.LinAlgError``): the shift sits on an eigenvalue.

    ``symmetric=False`` factors ``P mat P^T = LL UU`` instead, for any square real (or complex-step) matrix, on the
    pattern of ``mat + 0 mat^T``: partial pivoting (row interchanges, counted in ``row_interchanges``) inside the
    64-column panels, static pivots as above, and every application refined once against the true matrix (three
    times with static pivots).  An LU factor gives no inertia: ``negative_pivots`` is ``None``; ``kind`` is ``"lu"``
    (``"ldlt"`` for the symmetric factor).

    The transposed operator comes from the same factor: ``op.T``, ``op.H``, ``op.rmatvec`` and ``op.rmatmat`` apply
    ``mat^{-T}`` (the adjoint of a state equation with an unsymmetric matrix), refined like the forward application
    and counted in the same ``count``.  An LU factor allocates the copies only the transposed sweep reads on its first
    transposed application; for a symmetric operator the transposed application is the forward one.

    Complex matrices take one of two paths (``complex_arithmetic``; the one taken is ``op.complex_arithmetic``, ``None``
    for a real matrix).  ``"dual"``: ``mat = M + i dM`` is a complex-step matrix, a dual number: ``M`` alone is factored
    and ``mat^{-1}(b + i db) = x + i M^{-1}(db - dM x)``, exact to first order in ``dM``.  ``"full"``: true complex
    arithmetic through the real-equivalent system of order 2n with interleaved unknowns, every entry ``a + ib`` a
    block ``[[a, -b], [b, a]]``, factored by the LU path (``symmetric=False``), or for a complex *symmetric* matrix
    (``mat == mat^T``, e.g. a damped dynamic stiffness; ``symmetric=True``) ``[[a, -b], [-b, -a]]`` factored by the
    Bunch-Kaufman path with half the factor bytes -- its inertia is always (n, n), so ``negative_pivots`` is ``None``.
    Every application is refined against the complex matrix itself.  ``"auto"`` (the default) takes ``"dual"`` where
    ``max|Im| <= tuning.complex_step_ratio max|Re|`` (1e-12; complex-step perturbations are of relative size 1e-20)
    and ``"full"`` otherwise.  In ``"full"`` mode ``op.H`` applies ``mat^{-H}`` and ``op.T`` ``mat^{-T}``;
    ``solve_device_dual`` is the complex solve on device blocks and ``solve_device`` / ``solve_device_to`` raise.

    Structure: the constructor chooses one backend per arithmetic (``_RealBackend``, ``_DualBackend`` -- the real one
    plus the imaginary-part matrix --, ``_FullComplexBackend``).  A backend owns the factor, the matrix of the
    refinement's residuals, the raw solve, the refactorisations and the layout of a host array on the device; every
    application is ``_Backend.solve``, the one refined solve, over ``device.refine``.  The operator keeps the counter,
    the scipy surface and read-only views of the factor's figures (``kind``, the inertia, ...).  ``refined`` tells
    whether applications are refined (an indefinite, LU or full-complex factor), ``dual`` whether the operator is a
    complex-step one.
    """

    def __init__(self, mat, ctx=None, symbolic=None, leaf_size=0, panel_width=0, check_symmetry=True, coords=None,
                 symmetric=True, complex_arithmetic="auto"):
        if complex_arithmetic not in COMPLEX_ARITHMETIC:
            raise ValueError(f"complex_arithmetic must be one of {COMPLEX_ARITHMETIC}")
        if not sparse.issparse(mat):
            mat = sparse.csr_matrix(mat)
        if mat.shape[0] != mat.shape[1]:
            raise ValueError("expected a square matrix")
        self.ctx = ctx if ctx is not None else default_context()
        self.shape = mat.shape
        self.dtype = np.dtype(np.float64)
        self.count = 0
        self._count_lock = threading.Lock()  # mode groups on different streams share the counter
        self.symmetric = bool(symmetric)
        csr = mat.tocsr()
        backend = _RealBackend
        if np.issubdtype(mat.dtype, np.complexfloating):
            csr.sort_indices()
            self.dtype = np.dtype(np.complex128)
            full = select_complex_arithmetic(csr.data, complex_arithmetic) == "full"
            backend = _FullComplexBackend if full else _DualBackend
        # coords (optional, one row per dof): geometric nested dissection; without it the ordering is algebraic
        self._backend = backend(self.ctx, csr, complex_arithmetic, self.symmetric, check_symmetry, symbolic=symbolic,
                                leaf_size=leaf_size, panel_width=panel_width, coords=coords)
        self.complex_arithmetic = backend.complex_arithmetic
        self.factor = self._backend.factor
        self.symbolic = self.factor.symbolic

    # the factor's figures and whether applications are refined: the backend's, as of its last numeric phase
    kind = property(lambda self: self._backend.kind)
    row_interchanges = property(lambda self: self._backend.row_interchanges)
    static_pivots = property(lambda self: self._backend.static_pivots)
    negative_pivots = property(lambda self: self._backend.negative_pivots)
    negative_pivots_bounds = property(lambda self: self._backend.negative_pivots_bounds)
    refined = property(lambda self: self._backend.refined)
    _pivoted = refined.fget          # (the name the drivers used to read)
    dual = property(lambda self: self.complex_arithmetic == "dual")
    _real_equivalent_of = _FullComplexBackend._real_equivalent_of   # (test_complex_cpu.py restates the tables through it)

    def expand_values_device(self, vals):
        """("full") the real-equivalent CSR values the factor takes, from complex values on the device (nnz x 2 block)"""
        return self._backend.expand_values_device(vals)

    def _counted(self, k, count):
        with self._count_lock:
            self.count += k if count is None else int(count)

    # -- device path (used by the drivers) ------------------------------------
    def solve_device(self, X, alpha=1.0, count=None, trans=False):
        """
        X <- alpha * mat^{-1} X in place on a device block (``trans``: alpha * mat^{-T} X).  ``count`` is the number of
        columns that carry a live right-hand side (finished modes of a lock-step block are zero columns);
        the counter then means what the reference's does: applications per mode (ref 19-22).
        """
        self._no_real_block("solve_device")
        self._counted(X.k, count)
        return self._backend.solve(X, alpha, adjoint=trans)

    def _no_real_block(self, name):
        if self.complex_arithmetic == "full":
            raise TypeError(f"{name}: a real block has no imaginary half; a full-complex operator takes solve_device_dual")

    def solve_device_to(self, Xin, Xout, alpha=1.0, count=None, trans=False):
        """Xout <- alpha * mat^{-1} Xin on device blocks, Xin untouched (``trans``: alpha * mat^{-T} Xin)"""
        self._no_real_block("solve_device_to")
        self._counted(Xin.k, count)
        return self._backend.solve(Xout, alpha, Xin, adjoint=trans)

    def refactor_device(self, vals, indefinite_matrix=None):
        """
        numeric refactorisation from CSR values on the device (``ElementAssembler.assemble``; the pattern must be the
        one this operator was built on).  The positive definite case needs nothing else; for an indefinite result pass
        the device CSRMatrix holding the same values (``indefinite_matrix``) for the refinement step.  Full complex
        arithmetic: ``vals`` is an nnz x 2 block (real and imaginary part per entry, CSR order of the matrix the operator
        was built on), ``indefinite_matrix`` a ComplexCSRMatrix holding them (None: the operator's own takes them).
        """
        self._backend.refactor_device(vals, indefinite_matrix)

    def refactor(self, mat):
        """numeric refactorisation with new values on the same sparsity pattern (a complex matrix stays on the path --
        ``complex_arithmetic`` -- the operator was built on: switching between "dual" and "full" raises)"""
        self._backend.refactor(mat)

    def solve_device_dual(self, Xr, Xi, count=None, trans=False, conjugate=False):
        """
        complex-step operand (Xr + i Xi) <- mat^{-1} (Xr + i Xi) in place on two device blocks (see _DualBackend).
        ``trans``: mat^{-T}, i.e. x + i M^{-T}(db - dM^T x) with x = M^{-T} b; with ``conjugate`` mat^{-H}: + dM^T x.
        Full complex arithmetic: the true complex solve; in place without a copy when Xr and Xi are the two halves of
        one contiguous n x 2k block (``Z.cols(0, k)``, ``Z.cols(k, 2 k)``), else through such a block
        """
        self._backend.solve_complex(Xr, Xi, trans, conjugate, lambda: self._counted(Xr.k, count))
        return Xr, Xi

    # -- host path (reference call surface) ------------------------------------
    def _apply_host(self, x, adjoint):
        x = np.asarray(x)
        out = self._backend.apply_host(self, x.reshape(self.shape[0], -1), adjoint)
        return out[:, 0] if x.ndim == 1 else out

    def _matvec(self, x):
        return self._apply_host(x, False)

    def _matmat(self, X):
        return self._apply_host(X, False)

    # mat^{-H} x: scipy's LinearOperator builds op.H, op.T, rmatvec and rmatmat on these (op.T conjugates around them)
    def _rmatvec(self, x):
        return self._apply_host(x, True)

    def _rmatmat(self, X):
        return self._apply_host(X, True)

    def _adjoint(self):
        return _AdjointSpLuOperator(self)


class _AdjointSpLuOperator(LinearOperator):
    """``op.H``: applies ``mat^{-H}`` with ``op``'s factor and counts in ``op.count``; ``.H`` gives ``op`` back"""

    def __init__(self, op):
        self.op = op
        self.shape = op.shape
        self.dtype = op.dtype

    @property
    def count(self):
        return self.op.count

    def _matvec(self, x):
        return self.op._rmatvec(x)

    def _matmat(self, X):
        return self.op._rmatmat(X)

    def _rmatvec(self, x):
        return self.op._matvec(x)

    def _rmatmat(self, X):
        return self.op._matmat(X)

    def _adjoint(self):
        return self.op


# ---------------------------------------------------------------------------
class DeviceOperator:
    """y = A x on device blocks for a scipy sparse matrix (device CSR) or a host LinearOperator."""

    def __init__(self, ctx, A):
        self.ctx = ctx
        self.shape = A.shape
        self.host = None
        self.csr = None
        if isinstance(A, CSRMatrix):
            self.csr = A
        elif sparse.issparse(A):
            self.csr = CSRMatrix(ctx, A)
        elif hasattr(A, "A") and sparse.issparse(getattr(A, "A")):  # scipy MatrixLinearOperator
            self.csr = CSRMatrix(ctx, A.A)
        elif isinstance(A, np.ndarray):
            self.csr = CSRMatrix(ctx, sparse.csr_matrix(A))
        else:
            self.host = A  # foreign operator: applied on the host, block copied both ways

    def apply(self, X, Y=None):
        if self.csr is not None:
            return self.csr.apply(X, Y)
        out = np.asarray(self.host @ X.get())
        if Y is None:
            return self.ctx.from_host(out)
        Y.set(out)
        return Y


class FactorApply:
    """X <- alpha factor(X) on device blocks for our SpLuOperator or any foreign callable."""

    def __init__(self, ctx, factor):
        self.ctx = ctx
        self.factor = factor
        self.native = isinstance(factor, SpLuOperator)

    def __call__(self, X, alpha=1.0, count=None):
        if self.native:
            return self.factor.solve_device(X, alpha, count)
        out = np.asarray(self.factor(X.get()))  # honours a user-supplied operator
        X.set(alpha * out.reshape(X.n, X.k))
        return X

    def apply_to(self, Xin, Xout, alpha=1.0, count=None):
        """Xout <- alpha factor(Xin)"""
        if self.native:
            return self.factor.solve_device_to(Xin, Xout, alpha, count)
        out = np.asarray(self.factor(Xin.get()))
        Xout.set(alpha * out.reshape(Xin.n, Xin.k))
        return Xout

    def count_applications(self, n):
        """``n`` applications per mode that were enqueued with ``count=0`` (the lock-step loops learn only afterwards how
        many modes a sweep served) go into the native factor's counter; a foreign factor keeps its own count"""
        if self.native:
            self.factor._counted(0, n)

