"""
Catalog of the launch variants of the sparse products (csrc/sparse.hip): which small matrix
makes the launch plan pick which kernel at which block width, and which branch inside the kernels it reaches.  Plain
data and builders, no GPU import.

Each Case names a builder, the kind of product ("real": CSRMatrix.apply, with ``cg_widths`` also eigd_spmm_cg;
"complex": ComplexCSRMatrix.apply on split-layout blocks), the widths it runs, the (variant, columns of the launch)
pairs its plans must hold and the statistics of the pattern it claims (umax, direct tiles, long rows ...).
tests/test_product_catalog_cpu.py asks ``product_plan`` below -- the dispatch of sparse.hip restated on the host -- whether
the claims hold and whether the targets of all cases together are exactly the product kernels the library instantiates;
tests/test_gpu_product_variants.py runs the cases and compares with the references below.

References: ``restated_real`` here and ``restated_product`` of test_complex_cpu.py sum in CSR storage order with every
multiply and add rounded on its own, as the kernels do (all but the long-row branch of spmv_stream_kernel, see
``exact_row_sum``).  ``scipy_bitwise``: scipy's ``A @ X`` gives the same bits on the host the CPU test ran on; the GPU
test then gates on scipy as well.

The constants the builders aim at (sparse.hip): tiles of 32 rows; a real tile of KP columns stages umax rows of X of
KP + 4 doubles (KP + 1 below 8 columns) in 40 KiB -- 75 rows at 64 columns, 142 at 32; a complex tile 2 KP + 1 doubles
per row in 64 KiB -- 126 rows at 32 columns, 248 at 16, 481 at 8, 910 at 4, 1638 at 2, 2730 at 1; tiles of more than
1024 non-zeros read them from global memory ("direct"); row blocks of the stream kernels hold at most 2046 non-zeros
and 256 rows, a longer row is a block of its own (complex: longer than 2048).
"""
import math
from dataclasses import dataclass, field

import numpy as np
from scipy import sparse

from krylov_reference import two_prod_terms
from test_symbolic_cpu import grid_matrix


@dataclass(frozen=True)
class Case:
    name: str
    build: object                         # () -> scipy CSR matrix, as the device is to store it
    kind: str = "real"                    # "real" or "complex"
    widths: tuple = ()                    # block widths of the plain product (k = 1: contiguous and as a column view)
    cg_widths: tuple = ()                 # widths eigd_spmm_cg runs at (real, square, diagonally dominant cases)
    targets: tuple = ()                   # ((variant name, columns of that launch), ...), over all widths
    stats: dict = field(default_factory=dict)   # claims on the plan's statistics
    scipy_bitwise: bool = True            # scipy's A @ X has the restatement's bits (checked on the host)
    note: str = ""


def _csr(rows, cols, n, ncols=None, seed=0, dtype=float):
    """CSR matrix with one entry per (row, col) pair in the order given within each row, values seeded normal"""
    rows, cols = np.asarray(rows), np.asarray(cols)
    order = np.argsort(rows, kind="stable")
    rows, cols = rows[order], cols[order]
    rng = np.random.default_rng(seed)
    vals = rng.normal(size=len(rows))
    if dtype is complex:
        vals = vals + 1j * rng.normal(size=len(rows))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return sparse.csr_matrix((vals, cols.astype(np.int32), indptr.astype(np.int32)), shape=(n, ncols or n))


def dominant_diagonal(A):
    """a diagonal of twice the absolute sum of the rest of the row (the conjugate-gradient cases: z.Az is dominated by
    its positive terms); every diagonal entry must be stored"""
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    diag = rows == A.indices
    assert diag.sum() == A.shape[0]
    A.data[diag] = 0.0
    A.data[diag] = 2.0 * np.abs(A).sum(axis=1).A1 + 1.0
    return A


def band(n, half, thin=(), seed=0, dominant=False):
    """band matrix of half-width ``half``; rows in ``thin`` keep only their diagonal"""
    r = np.repeat(np.arange(n), 2 * half + 1)
    c = r + np.tile(np.arange(-half, half + 1), n)
    ok = (c >= 0) & (c < n) & ~(np.isin(r, list(thin)) & (r != c))
    A = _csr(r[ok], c[ok], n, seed=seed)
    return dominant_diagonal(A) if dominant else A


def arrow(n, umax, row=5, seed=0, dtype=float):
    """tridiagonal matrix whose row ``row`` has extra far columns, so that the first tile touches exactly ``umax``
    distinct columns (33 of the tridiagonal part, the rest in that row)"""
    assert row < 31 and n >= umax + 40
    i = np.arange(n)
    r = np.concatenate([i[1:], i, i[:-1], np.full(umax - 33, row)])
    c = np.concatenate([i[1:] - 1, i, i[:-1] + 1, 40 + np.arange(umax - 33)])
    order = np.lexsort((c, r))
    return _csr(r[order], c[order], n, seed=seed, dtype=dtype)


def row_block_edges():
    """row 0: one entry, so the block of row 1 (exactly 2046 non-zeros, the most a staged block holds) starts at an odd
    entry; row 2: 2047 non-zeros, one more, a long row; rows 3..302: empty (a block is cut at 256 rows); then a
    tridiagonal tail"""
    n = 2600
    r = [np.zeros(1, int), np.full(2046, 1), np.full(2047, 2)]
    c = [np.array([7]), np.arange(2046) + 3, np.arange(2047) + 500]
    t = np.arange(303, n)
    r += [t, t, t[:-1]]
    c += [t - 1, t, t[:-1] + 1]
    r, c = np.concatenate(r), np.concatenate(c)
    order = np.lexsort((c, r))
    return _csr(r[order], c[order], n, seed=3)


def wide_tile(square, dtype=float):
    """the 32 rows of the first tile touch 70 000 distinct columns, more than a 16-bit position can name: no tile lists"""
    ncols = 70000
    n = ncols if square else 64
    i = np.arange(32)
    r = np.repeat(i, 2200)
    c = (np.repeat(i * 2200, 2200) + np.tile(np.arange(2200), 32)) % ncols
    t = np.arange(32, n)
    r, c = np.concatenate([r, t, t]), np.concatenate([c, t, (t * 7 + 3) % ncols])
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    keep = np.concatenate([[True], (r[1:] != r[:-1]) | (c[1:] != c[:-1])])
    return _csr(r[keep], c[keep], n, ncols, seed=4, dtype=dtype)


def noncanonical():
    """the grid matrix with every 11th entry stored twice, the columns of every row shuffled and an explicit zero"""
    A = grid_matrix(61, 47, 2)
    rng = np.random.default_rng(5)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    dup = np.arange(0, A.nnz, 11)
    r = np.concatenate([rows, rows[dup]])
    c = np.concatenate([A.indices, A.indices[dup]])
    v = np.concatenate([A.data, rng.normal(size=len(dup))])
    v[17] = 0.0
    order = np.lexsort((rng.random(len(r)), r))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=A.shape[0]))])
    B = sparse.csr_matrix((v[order], c[order].astype(np.int32), indptr.astype(np.int32)), shape=A.shape)
    assert not B.has_canonical_format
    return B


def tridiag(n):
    i = np.arange(n)
    A = sparse.diags([-np.ones(n - 1), 2.5 + 0.25 * np.cos(i), -np.ones(n - 1)], [-1, 0, 1]).tocsr()
    A.sort_indices()
    return A


def grid_dominant():
    A = grid_matrix(61, 47, 2, seed=1)
    return (A + A.T).tocsr()


def _tiled(kp, cols, dots=False):
    return (f"spmm_tiled_kernel<{kp}, 8, true>" if dots else f"spmm_tiled_kernel<{kp}, 8>", cols)


def _rows(kp, cols):
    return (f"spmm_rows_kernel<{kp}>", cols)


SPMV, REDUCE, CSPMV = "spmv_stream_kernel", "tile_dots_reduce_kernel", "cspmv_stream_kernel"
CSTAGED, CDIRECT = "cspmm_tiled_kernel<true>", "cspmm_tiled_kernel<false>"

CASES = [
    # all tiles staged; above 32 columns the 64-column tile does not fit (umax 108 > 75) and the block goes in chunks of 32
    Case("grid", lambda: grid_matrix(61, 47, 2), widths=(1, 2, 3, 5, 16, 32, 33, 40, 70),
         targets=((SPMV, 1), _tiled(2, 1), _tiled(2, 2), _tiled(4, 3), _tiled(8, 5), _tiled(16, 16), _tiled(32, 32),
                  _tiled(8, 8), _tiled(8, 6)),
         stats=dict(tiles=180, umax=108, tnz_cap=576, direct_tiles=0, long_row_blocks=0)),
    Case("grid_cg", grid_dominant, widths=(3, 5, 16, 32, 40), cg_widths=(3, 5, 16, 32, 40),
         targets=(_tiled(8, 5, True), _tiled(16, 16, True), _tiled(32, 32, True), (REDUCE, 5), (REDUCE, 16), (REDUCE, 32),
                  _tiled(4, 3), _tiled(8, 8)),
         stats=dict(tiles=180, umax=108, direct_tiles=0)),
    # 33 tiles (not a multiple of 8), the last one of 27 rows; umax 48 fits the 64-column tile
    Case("band8", lambda: band(1051, 8), widths=(33, 64, 70),
         targets=(_tiled(64, 33), _tiled(64, 64), _tiled(8, 6)),
         stats=dict(tiles=33, umax=48, tnz_cap=544, direct_tiles=0)),
    # tiles of 32 x 41 = 1312 non-zeros are direct; the tile of the thinned rows and the last one (3 rows) are staged
    Case("band20_thin", lambda: band(1059, 20, thin=range(96, 128), dominant=True), widths=(5, 32, 48),
         cg_widths=(5, 16, 32),
         targets=(_tiled(8, 5), _tiled(32, 32), _tiled(64, 48), _tiled(8, 5, True), _tiled(16, 16, True),
                  _tiled(32, 32, True)),
         stats=dict(tiles=34, umax=72, tnz_cap=1024, direct_tiles=32)),
    # the LDS limit of the 32-wide tile: 142 rows of 36 doubles are 40 896 bytes, 143 are 41 184
    Case("arrow142", lambda: arrow(600, 142), widths=(32, 64), targets=(_tiled(32, 32),),
         stats=dict(umax=142, direct_tiles=0)),
    Case("arrow143", lambda: dominant_diagonal(arrow(600, 143)), widths=(16, 32, 64), cg_widths=(32,),
         targets=(_tiled(16, 16), _rows(32, 32), _rows(64, 64)), stats=dict(umax=143, direct_tiles=0)),
    # umax 2200 fits no real tile; the arrow row holds 2170 non-zeros: a long row of both stream kernels
    Case("arrow2200", lambda: arrow(2400, 2200), widths=(1, 2, 3, 5, 16, 32, 64),
         targets=((SPMV, 1), _rows(2, 1), _rows(2, 2), _rows(4, 3), _rows(8, 5), _rows(16, 16), _rows(32, 32), _rows(64, 64)),
         stats=dict(umax=2200, direct_tiles=1, long_row_blocks=1)),
    Case("row_block_edges", row_block_edges, widths=(1, 3), targets=((SPMV, 1),),
         stats=dict(long_row_blocks=1, row_blocks=14)),
    Case("wide_tile", lambda: wide_tile(False), widths=(1, 3, 40),
         targets=((SPMV, 1), _rows(2, 1), _rows(4, 3), _rows(64, 40)),
         stats=dict(tiles=0, umax=0, tnz_cap=0, direct_tiles=0)),
    Case("noncanonical", noncanonical, widths=(1, 5, 32), targets=((SPMV, 1), _tiled(8, 5), _tiled(32, 32)),
         stats=dict(tiles=180, umax=108),
         note="duplicate and unsorted columns, an explicit zero: the sums run in storage order"),
    Case("empty", lambda: sparse.csr_matrix((70, 70)), widths=(1, 3), targets=((SPMV, 1), _tiled(2, 1), _tiled(4, 3)),
         stats=dict(tiles=3, umax=0, tnz_cap=0, row_blocks=1)),
    # more than 1024 x 4 tiles: at 32 columns (64 sums, 4 tiles per trip) a workgroup of tile_dots_reduce_kernel makes a
    # second trip; 1024 groups
    Case("tridiag_131105", lambda: tridiag(131105), widths=(5, 32), cg_widths=(5, 32),
         targets=(_tiled(32, 32, True), (REDUCE, 32), _tiled(8, 5, True), (REDUCE, 5)),
         stats=dict(tiles=4098, umax=34, direct_tiles=0)),
]

# complex arrows: the widest chunk whose staged rows fit 64 KiB, by umax
CHUNK_OF_UMAX = ((126, 32), (127, 16), (249, 8), (482, 4), (911, 2), (1639, 1), (2730, 1))
CASES += [
    Case(f"carrow{u}", (lambda u=u: arrow(3000, u, dtype=complex)), kind="complex", widths=(1, 4, 33),
         targets=((CSPMV, 1), (CSTAGED, min(4, ch)), (CSTAGED, ch), (CSTAGED, 33 % ch or ch)),
         stats=dict(umax=u, long_row_blocks=int(u - 30 > 2048)))     # (the arrow row holds u - 30 non-zeros)
    for u, ch in CHUNK_OF_UMAX
] + [
    Case("carrow2731", lambda: arrow(3000, 2731, dtype=complex), kind="complex", widths=(1, 4, 33),
         targets=((CSPMV, 1), (CDIRECT, 4), (CDIRECT, 32), (CDIRECT, 1)), stats=dict(umax=2731, long_row_blocks=1)),
    # a row of 4200 non-zeros: three chunks of cspmv_stream_kernel's staging (2048, 2048, 104)
    Case("carrow4230", lambda: arrow(4400, 4230, dtype=complex), kind="complex", widths=(1, 2),
         targets=((CSPMV, 1), (CDIRECT, 2)), stats=dict(umax=4230, long_row_blocks=1)),
    Case("cgrid", lambda: _complex_grid(), kind="complex", widths=(1, 4, 32, 33),
         targets=((CSPMV, 1), (CSTAGED, 4), (CSTAGED, 32), (CSTAGED, 1)), stats=dict(tiles=180, umax=108)),
    Case("cwide_tile", lambda: wide_tile(True, dtype=complex), kind="complex", widths=(1, 4, 33),
         targets=((CSPMV, 1), (CDIRECT, 4), (CDIRECT, 32), (CDIRECT, 1)), stats=dict(tiles=0, umax=0)),
]


def _complex_grid():
    A = grid_matrix(61, 47, 2)
    rng = np.random.default_rng(6)
    return sparse.csr_matrix((A.data + 1j * rng.normal(size=A.nnz), A.indices, A.indptr), shape=A.shape)


BY_NAME = {c.name: c for c in CASES}


def all_targets():
    return {v for c in CASES for v, _ in c.targets}


def widths_planned(case):
    """(kind of plan, k, unit_ld) of every plan a case's runs ask for"""
    out = []
    for k in case.widths:
        if case.kind == "complex":
            out.append(("complex", k, False))
        else:
            out += [("real", k, u) for u in ((True, False) if k == 1 else (False,))]
    return out + [("cg", k, False) for k in case.cg_widths]


# ---- the dispatch of sparse.hip, restated on the host ----------------------------------------------------------------
# eigd_csr_upload_rect's analysis of the pattern and the conditions of eigd_spmm_on, eigd_spmm_cg and eigd_ccsr_spmm_on,
# restated from the source: which kernel instantiation a block of k columns launches on which column range.  The
# library has no query of its own for this, so the restatement is what the catalog is checked against.

PRODUCT_VARIANTS = (
    ["spmv_stream_kernel"] + [f"spmm_tiled_kernel<{kp}, 8>" for kp in (2, 4, 8, 16, 32, 64)]
    + [f"spmm_tiled_kernel<{kp}, 8, true>" for kp in (8, 16, 32)] + ["tile_dots_reduce_kernel"]
    + [f"spmm_rows_kernel<{kp}>" for kp in (2, 4, 8, 16, 32, 64)]
    + ["cspmv_stream_kernel", "cspmm_tiled_kernel<true>", "cspmm_tiled_kernel<false>"])

TILE_ROWS, TILE_LDS, TILE_NNZ, NNZ_TILE, MAX_ROWS_TILE, CTILE_LDS = 32, 40 * 1024, 1024, 2048, 256, 64 * 1024


def pattern_stats(A, kind="real"):
    """tiles, umax, tnz_cap, direct tiles, row blocks and long-row blocks as eigd_csr_upload_rect finds them"""
    A = sparse.csr_matrix(A)
    n = A.shape[0]
    ip, ix = A.indptr.astype(np.int64), A.indices
    ln = np.diff(ip)
    nblocks = nlong = r = 0
    limit = NNZ_TILE if kind == "complex" else NNZ_TILE - 2
    while r < n:
        start, cnt = r, 0
        while r < n and r - start < MAX_ROWS_TILE and cnt + ln[r] <= NNZ_TILE - 2:
            cnt += ln[r]
            r += 1
        if r == start:
            r += 1
        nblocks += 1
        nlong += int(ip[r] - ip[start] > limit)
    ntiles = -(-n // TILE_ROWS)
    edges = ip[np.minimum(np.arange(ntiles + 1) * TILE_ROWS, n)]
    tnz = np.diff(edges)
    umax = max((len(np.unique(ix[edges[t]:edges[t + 1]])) for t in range(ntiles)), default=0)
    st = dict(tiles=ntiles, umax=int(umax), tnz_cap=int(min(TILE_NNZ, (tnz.max() + 7) & ~7)), row_blocks=nblocks,
              long_row_blocks=nlong)
    if umax > 65535:                                       # no tile lists
        st.update(tiles=0, umax=0, tnz_cap=0)
    st["direct_tiles"] = int((tnz > st["tnz_cap"]).sum()) if st["tiles"] else 0
    return st


def _pow2(v):
    p = 1
    while p < v:
        p *= 2
    return p


def product_plan(A, k, kind="real", unit_ld=False, stats=None):
    """(launches as (variant, first column, columns) in launch order, statistics with ``fused_dots``) of a product with a
    block of k columns; kind "real", "cg" (eigd_spmm_cg) or "complex" (k complex columns)"""
    st = dict(stats if stats is not None else pattern_stats(A, "complex" if kind == "complex" else "real"))
    ntiles, umax = st["tiles"], st["umax"]
    st["fused_dots"] = 0
    if kind == "complex":
        if k == 1:
            return [("cspmv_stream_kernel", 0, 1)], st
        lds = lambda kp: 8 * umax * (2 * kp + 1)           # noqa: E731
        chunk = 32
        while chunk > 1 and (ntiles == 0 or lds(chunk) > CTILE_LDS):
            chunk //= 2
        staged = ntiles > 0 and lds(chunk) <= CTILE_LDS
        if not staged:
            chunk = 32
        name = "cspmm_tiled_kernel<true>" if staged else "cspmm_tiled_kernel<false>"
        return [(name, c0, min(chunk, k - c0)) for c0 in range(0, k, chunk)], st
    if k == 1 and unit_ld:
        return [("spmv_stream_kernel", 0, 1)], st
    fits = lambda kp: ntiles > 0 and 8 * umax * (kp + 4 if kp >= 16 else kp + 1) <= TILE_LDS     # noqa: E731
    if kind == "cg":
        kp = max(2, _pow2(k))
        if 8 <= kp <= 32 and fits(kp):
            st["fused_dots"] = 1
            return [(f"spmm_tiled_kernel<{kp}, 8, true>", 0, k), ("tile_dots_reduce_kernel", 0, k)], st
    chunk = 32 if (k > 32 and not fits(64) and fits(32)) else 64
    plan = []
    for c0 in range(0, k, chunk):
        kb = min(chunk, k - c0)
        kp = max(2, _pow2(kb))
        plan.append((f"spmm_tiled_kernel<{kp}, 8>" if fits(kp) else f"spmm_rows_kernel<{kp}>", c0, kb))
    return plan, st


# ---- references ---------------------------------------------------------------------------------------------------------

def restated_real(A, X, alpha=1.0, beta=0.0, Y=None):
    """alpha A X + beta Y as the real kernels form it: per (row, column) the sum over the row's entries in storage order
    from 0.0, multiply and add rounded separately; then alpha s (beta == 0) or alpha s + beta y with three roundings
    (the device may fuse one product: exact for alpha, beta powers of two).  A is taken as stored"""
    A = sparse.csr_matrix(A)
    X = np.asarray(X, dtype=np.float64).reshape(A.shape[1], -1)
    ip, ix, av = A.indptr, A.indices, A.data
    ln = np.diff(ip)
    s = np.zeros((A.shape[0], X.shape[1]))
    for p in range(int(ln.max()) if ln.size else 0):
        rows = np.flatnonzero(ln > p)
        e = ip[rows] + p
        prod = av[e][:, None] * X[ix[e]]
        s[rows] = s[rows] + prod
    if beta == 0.0:
        return alpha * s
    t0, t1 = alpha * s, beta * np.asarray(Y, dtype=np.float64).reshape(s.shape)
    return t0 + t1


def with_values(A, vals):
    return sparse.csr_matrix((np.asarray(vals, dtype=A.dtype), A.indices, A.indptr), shape=A.shape)


def exact_row_sum(A, x, row):
    """(the exactly rounded sum_e a_e x_e of one row, sum_e |a_e x_e|): math.fsum over the error-free products"""
    A = sparse.csr_matrix(A)
    a = A.data[A.indptr[row]:A.indptr[row + 1]]
    xe = np.asarray(x, dtype=np.float64).ravel()[A.indices[A.indptr[row]:A.indptr[row + 1]]]
    return math.fsum(two_prod_terms(a, xe)), math.fsum(np.abs(a * xe).tolist())


def long_rows(A, limit=2046):
    """rows spmv_stream_kernel sums as strided partial sums and a tree instead of in CSR order"""
    return np.flatnonzero(np.diff(sparse.csr_matrix(A).indptr) > limit)
