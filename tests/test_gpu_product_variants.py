"""
Every launch variant of the sparse products (csrc/sparse.hip) against exact references: one parametrised test per case
of tests/product_catalog.py (tests/test_product_catalog_cpu.py holds the restated dispatch against the cases' targets:
which kernel each width launches) checks that every width gives the bits of
the restated sum -- storage order, every multiply and add rounded on its own -- for the matrix, its transposed (complex:
conjugate-transposed) companion, and both again after new values on the device.  The long-row branch of
spmv_stream_kernel, which does not sum in storage order, is gated against the exactly rounded row sum.

Gates that are not bitwise (eps = 2**-52); the tests print the ratio error / gate of every case (run with -s):
  long-row SpMV   (ceil(L / 256) + 10) eps sum |a_e x_e|: the strided partial sums of the 256 lanes (one fused
                  multiply-add per term), the eight-level tree, one contraction
  alpha, beta     2 eps (|alpha s| + |beta y0|) against the exact alpha s + beta y0 of the bit-exact sum s: two
                  products (one may be fused) and an add, three roundings at most
Largest ratios on an MI355X: not measured yet -- no device was available while this file was written (docs/LOG.md).
"""
import math

import numpy as np
import pytest
from scipy import sparse

from product_catalog import BY_NAME, CASES, exact_row_sum, long_rows, product_plan, restated_real, with_values
from test_complex_cpu import restated_product

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
SENT = 7.25
measured = {"long_row": 0.0, "alpha_beta": 0.0}


@pytest.fixture(scope="module")
def ctx():
    from eigd_amd.device import default_context

    return default_context()


def bits(a):
    a = np.ascontiguousarray(a)
    return (a.view(np.float64) if np.iscomplexobj(a) else a.astype(np.float64, copy=False)).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Side:
    """one matrix on the device (a case's matrix or a companion) with its host copy, the way blocks go in and out for
    its arithmetic, and the restatement of its product"""

    def __init__(self, dev, host, kind):
        self.dev, self.host, self.kind = dev, sparse.csr_matrix(host), kind
        self.cols = 2 if kind == "complex" else 1

    def operand(self, k, seed=0):
        rng = np.random.default_rng(seed)
        X = rng.normal(size=(self.host.shape[1], k))
        return X + 1j * rng.normal(size=X.shape) if self.kind == "complex" else X

    def to_block(self, X):
        from eigd_amd.device import complex_split

        return complex_split(X) if self.kind == "complex" else np.ascontiguousarray(X, dtype=np.float64)

    def from_block(self, Y):
        from eigd_amd.device import complex_join

        return complex_join(Y) if self.kind == "complex" else Y

    def restated(self, X, alpha=1.0, beta=0.0, Y=None):
        if self.kind == "complex":
            assert self.host.has_sorted_indices          # (restated_product sorts; the complex cases are canonical)
            return restated_product(self.host, X, alpha, beta, Y)
        return restated_real(self.host, X, alpha, beta, Y)

    def apply(self, ctx, X, alpha=1.0, beta=0.0, Y0=None):
        """contiguous blocks: X (n, k) -> Y (n, k), host arrays in the side's arithmetic"""
        dX = ctx.from_host(self.to_block(X))
        dY = None if Y0 is None else ctx.from_host(self.to_block(Y0))
        return self.from_block(self.dev.apply(dX, dY, alpha, beta).get())

    def apply_in_views(self, ctx, X, offx, ldx, offy, ldy, same_parent=False):
        """X and Y as column ranges [off, off + block columns) of wider blocks; everything else must stay as it was"""
        Xb = self.to_block(X)
        w = Xb.shape[1]
        n, m = self.host.shape
        px = np.full((m, ldx), SENT)
        px[:, offx:offx + w] = Xb
        dPx = ctx.from_host(px)
        if same_parent:
            assert n == m and ldx == ldy and (offx + w <= offy or offy + w <= offx)
            dPy, py = dPx, px
        else:
            py = np.full((n, ldy), np.nan)
            dPy = ctx.from_host(py)
        self.dev.apply(dPx.cols(offx, offx + w), dPy.cols(offy, offy + w))
        out = dPy.get()
        keep = np.ones(ldy, dtype=bool)
        keep[offy:offy + w] = False
        assert same_bits(out[:, keep], py[:, keep]), "columns outside the view were written"
        if not same_parent:
            assert same_bits(dPx.get(), px), "the operand was written"
        return self.from_block(np.ascontiguousarray(out[:, offy:offy + w]))


def upload(ctx, case, A):
    from eigd_amd.device import ComplexCSRMatrix, CSRMatrix

    return (ComplexCSRMatrix if case.kind == "complex" else CSRMatrix)(ctx, A)


def adjoint_of(A, kind):
    return (A.conj().T if kind == "complex" else A.T).tocsr()


def check_long_rows(side, x, y, ref):
    """rows of the real SpMV that are summed as strided partial sums and a tree: against the exactly rounded sum; the
    other rows bitwise.  Returns the rows"""
    rows = long_rows(side.host)
    for r in rows:
        L = int(np.diff(side.host.indptr)[r])
        exact, sabs = exact_row_sum(side.host, x, r)
        gate = (math.ceil(L / 256) + 10) * EPS * sabs
        ratio = abs(float(y[r, 0]) - exact) / gate
        measured["long_row"] = max(measured["long_row"], ratio)
        print(f"long row {r} of {L} non-zeros: error / gate = {ratio:.3g}")
        assert ratio <= 1.0, (r, L, y[r, 0], exact, gate)
    rest = np.setdiff1d(np.arange(side.host.shape[0]), rows)
    assert same_bits(y[rest], ref[rest])
    return rows


def check_side(ctx, case, side, widths, seed):
    """products of one matrix at the given widths"""
    kmax = max(widths)
    X = side.operand(kmax, seed)
    ref = side.restated(X)
    if case.scipy_bitwise:
        assert same_bits(ref, np.asarray(side.host @ X))
    for k in widths:
        for unit in ((True, False) if (k == 1 and side.kind == "real") else (False,)):
            if k == 1 and side.kind == "real" and not unit:    # a single column with ld > 1: no SpMV
                Y = side.apply_in_views(ctx, X[:, :1], 1, 3, 2, 5)
            else:
                Y = side.apply(ctx, X[:, :k])
            if unit:
                check_long_rows(side, X[:, 0], Y, ref[:, :1])
            else:
                assert same_bits(Y, ref[:, :k]), (case.name, k, unit)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_case_every_width(ctx, case):
    A = case.build()
    dA = upload(ctx, case, A)
    side = Side(dA, A, case.kind)
    check_side(ctx, case, side, case.widths, seed=1)
    if A.nnz == 0:                                            # Y = beta Y0
        for k in case.widths:
            Y0 = side.operand(k, 9)
            assert same_bits(side.apply(ctx, side.operand(k, 8), 3.0, 2.0, Y0), 2.0 * Y0)
            assert not side.apply(ctx, side.operand(k, 8), 3.0, 0.0, np.full(Y0.shape, np.nan)).any()
        return
    if A.shape[0] != A.shape[1]:
        return
    # the companion: made from the pattern once, refreshed on the device when the values change
    companion = dA.conjugate_transposed() if case.kind == "complex" else dA.transposed()
    tside = Side(companion, adjoint_of(A, case.kind), case.kind)
    check_side(ctx, case, tside, case.widths, seed=2)
    rng = np.random.default_rng(3)
    v2 = rng.normal(size=A.nnz) + (1j * rng.normal(size=A.nnz) if case.kind == "complex" else 0.0)
    blk = np.column_stack([v2.real, v2.imag]) if case.kind == "complex" else v2.reshape(-1, 1)
    dA.update_values_device(ctx.from_host(np.ascontiguousarray(blk)))
    A2 = with_values(A, v2)
    few = sorted({min(case.widths), max(case.widths)})
    check_side(ctx, case, Side(dA, A2, case.kind), few, seed=4)
    check_side(ctx, case, Side(companion, adjoint_of(A2, case.kind), case.kind), few, seed=5)


def test_long_rows_of_the_stream_kernels(ctx):
    """real: the exactly rounded sum within the counted bound (arrow2200: 2170 non-zeros, row_block_edges: 2047, one more
    than a staged block holds -- and the row of exactly 2046 is bitwise); complex: sequential, chunk by chunk, bitwise"""
    for name, nlong in (("arrow2200", 1), ("row_block_edges", 1)):
        case = BY_NAME[name]
        A = case.build()
        side = Side(upload(ctx, case, A), A, "real")
        for seed in (6, 7):
            X = side.operand(1, seed)
            assert len(check_long_rows(side, X[:, 0], side.apply(ctx, X), side.restated(X))) == nlong
    for name in ("carrow2731", "carrow4230"):
        case = BY_NAME[name]
        A = case.build()
        side = Side(upload(ctx, case, A), A, "complex")
        assert np.diff(A.indptr).max() > 2048
        X = side.operand(1, 6)
        assert same_bits(side.apply(ctx, X), side.restated(X))
    print(f"largest long-row error / gate: {measured['long_row']:.3g}")


# one width per launch family
FAMILIES = [("grid", 1, "spmv_stream_kernel"), ("grid", 5, "spmm_tiled_kernel<8, 8>"),
            ("band8", 33, "spmm_tiled_kernel<64, 8>"), ("band20_thin", 32, "spmm_tiled_kernel<32, 8>"),
            ("arrow2200", 5, "spmm_rows_kernel<8>"), ("cgrid", 1, "cspmv_stream_kernel"),
            ("cgrid", 4, "cspmm_tiled_kernel<true>"), ("carrow2731", 4, "cspmm_tiled_kernel<false>")]


@pytest.mark.parametrize("name,k,variant", FAMILIES, ids=[f"{n}-{k}" for n, k, _ in FAMILIES])
def test_alpha_and_beta(ctx, name, k, variant):
    case = BY_NAME[name]
    A = case.build()
    dA = upload(ctx, case, A)
    side = Side(dA, A, case.kind)
    assert [v for v, _, _ in product_plan(A, k, case.kind, unit_ld=(k == 1 and case.kind == "real"))[0]] == [variant]
    X, Y0 = side.operand(k, 1), side.operand(k, 2)
    if case.kind == "real" and k == 1:                        # (a long row is not summed in storage order)
        assert not len(long_rows(A))
    s = side.restated(X)
    # powers of two: both products are exact, one rounding, fused or not
    for alpha, beta in ((-1.0, 2.0), (2.0, 0.5), (0.5, -1.0), (2.0, 0.0), (-1.0, 0.0)):
        Y = side.apply(ctx, X, alpha, beta, Y0)
        assert same_bits(Y, side.restated(X, alpha, beta, Y0)), (alpha, beta)
        assert same_bits(Y, alpha * s + beta * Y0) or beta == 0.0
    # general values: the compiler may fuse either product
    L = np.longdouble
    parts = (lambda Z: (Z.real, Z.imag)) if case.kind == "complex" else (lambda Z: (Z,))
    for alpha, beta in ((-0.37, 1.9), (1.9, -0.37)):
        Y = side.apply(ctx, X, alpha, beta, Y0)
        for y, sp, y0 in zip(parts(Y), parts(s), parts(Y0)):
            exact = L(alpha) * sp.astype(L) + L(beta) * y0.astype(L)
            gate = 2.0 * EPS * (np.abs(alpha * sp) + np.abs(beta * y0))
            ratio = float(np.max(np.abs(y.astype(L) - exact) / gate))
            measured["alpha_beta"] = max(measured["alpha_beta"], ratio)
            print(f"{name} k={k} alpha={alpha} beta={beta}: largest error / gate = {ratio:.3g}")
            assert ratio <= 1.0
    # beta = 0: Y is not read
    Y = side.apply(ctx, X, 1.0, 0.0, np.full(Y0.shape, np.nan))
    assert same_bits(Y, s)
    Y = side.apply(ctx, X, -0.37, 0.0, np.full(Y0.shape, np.nan))
    assert not np.isnan(Y).any() and same_bits(Y, -0.37 * s)
    print(f"largest alpha/beta error / gate so far: {measured['alpha_beta']:.3g}")


@pytest.mark.parametrize("name", ["grid", "band8", "arrow2200", "cgrid", "carrow2731"])
def test_products_in_column_views(ctx, name):
    case = BY_NAME[name]
    A = case.build()
    dA = upload(ctx, case, A)
    side = Side(dA, A, case.kind)
    c = side.cols
    X = side.operand(33, 1)
    ref = side.restated(X)
    k = 5 if c == 1 else 3                                    # ld 7: 5 real columns, or 3 complex ones (6 doubles)
    assert same_bits(side.apply_in_views(ctx, X[:, :k], 1, 7, 0, 7), ref[:, :k])
    k = 33 if c == 1 else 16                                  # ld 70, odd offsets
    assert same_bits(side.apply_in_views(ctx, X[:, :k], 3, 70, 5, 70), ref[:, :k])
    k = 16 if c == 1 else 8                                   # disjoint ranges of one parent
    assert same_bits(side.apply_in_views(ctx, X[:, :k], 1, 70, 35, 70, same_parent=True), ref[:, :k])
    assert same_bits(side.apply_in_views(ctx, X[:, :k], 37, 70, 3, 70, same_parent=True), ref[:, :k])
    # in place: refused on the host, before any launch
    dX = ctx.from_host(side.to_block(X[:, :4]))
    with pytest.raises(ValueError, match="in place"):
        dA.apply(dX, dX)
    assert same_bits(dX.get(), side.to_block(X[:, :4]))


CG_RUNS = [(c.name, k) for c in CASES for k in c.cg_widths]


@pytest.mark.parametrize("name,k", CG_RUNS, ids=[f"{n}-{k}" for n, k in CG_RUNS])
def test_conjugate_gradient_sums_of_the_product_pass(ctx, name, k):
    """eigd_spmm_cg, fused (5 <= k <= 32 on a tile that fits) and as product plus eigd_cg_coefficients: y is the plain
    product bit for bit, the coefficients are within the bound of test_gpu_krylov_steps (its helper, its gate), and a
    second run gives the same bits"""
    import test_gpu_krylov_steps as ks

    case = BY_NAME[name]
    A = case.build()
    dA = upload(ctx, case, A)
    plan, stats = product_plan(A, k, "cg")
    print(f"{name} k={k}: {plan}")
    for first in (1, 0):
        pc = ks.product_pass_case(A, k, first, seed=100 + k)
        assert same_bits(pc["Y"], restated_real(A, pc["Z"]))
        y1, s1 = ks.run_product_pass(ctx, dA, pc)
        y2, s2 = ks.run_product_pass(ctx, dA, pc)
        assert same_bits(y1, y2) and same_bits(s1, s2)
        assert same_bits(y1, Side(dA, A, "real").apply(ctx, pc["Z"]))


def test_value_expansion_with_absent_entries(ctx):
    """a table entry < 0 (the target pattern has an entry the source has not) gives 0.0, whatever the block held"""
    from eigd_amd.device import ValueExpansion, expand_values_host

    rng = np.random.default_rng(12)
    nsrc, nout = 1000, 5003
    table = ((rng.integers(0, nsrc, size=nout) << 2) | rng.integers(0, 4, size=nout)).astype(np.int32)
    table[rng.random(nout) < 0.1] = -1
    table[[0, nout - 1]] = -1
    vals = rng.normal(size=nsrc) + 1j * rng.normal(size=nsrc)
    out = ctx.from_host(np.full((nout + 5, 1), np.nan))
    ValueExpansion(ctx, table, nsrc).expand(ctx.from_host(np.column_stack([vals.real, vals.imag])), out)
    got = out.get()[:, 0]
    assert same_bits(got[:nout], expand_values_host(table, vals))
    assert np.isnan(got[nout:]).all() and not got[:nout][table < 0].any()
