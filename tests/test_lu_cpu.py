"""
Host side of the LU factor (SpLuOperator(..., symmetric=False)): the scatter map of the strictly upper entries the
symbolic analysis builds for it, and the new entry point of the C ABI.  No GPU needed.
"""
import os
import re

import numpy as np
from scipy import sparse

from eigd_amd import _ffi
from eigd_amd.device import Symbolic, symmetrised_pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unsymmetric_pattern(nx=14, ny=11, seed=0):
    """a 5-point grid matrix plus one-directional couplings (structurally unsymmetric), rows sorted"""
    rng = np.random.default_rng(seed)
    n = nx * ny
    T = lambda m: sparse.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))  # noqa: E731
    A = (sparse.kron(sparse.identity(ny), T(nx)) + sparse.kron(T(ny), sparse.identity(nx))).tocsr()
    r = rng.integers(0, n, size=3 * n)
    c = np.minimum(n - 1, r + rng.integers(2, 3 * nx, size=r.size))  # couplings i -> j > i only, some far away
    A = (A + sparse.csr_matrix((rng.uniform(0.1, 1.0, size=r.size), (r, c)), shape=(n, n))).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    assert (A != A.T).nnz > 0
    return A


def front_of(foff, dst):
    return np.searchsorted(foff, dst, side="right") - 1


def test_upper_and_lower_maps_cover_every_entry_once():
    """(an LU factor is analysed on the symmetrised pattern of its matrix: Factor(..., lu=True))"""
    for seed in (0, 1):
        pattern = symmetrised_pattern(unsymmetric_pattern(seed=seed))
        sym = Symbolic(pattern, leaf_size=16)
        a_src, u_src = sym.array("a_src"), sym.array("u_src")
        assert len(u_src) == pattern.nnz - sym.sizes["nlower"] > 0
        src = np.sort(np.concatenate([a_src, u_src]))
        np.testing.assert_array_equal(src, np.arange(pattern.nnz))


def test_upper_destination_is_the_transposed_lower_one():
    """the upper triangle is kept transposed (FU): an upper entry goes where its transpose goes in the lower fronts"""
    A = symmetrised_pattern(unsymmetric_pattern(seed=3))
    sym = Symbolic(A, leaf_size=16)
    ns, bs, foff = sym.array("f_ns"), sym.array("f_bs"), sym.array("f_foff")
    a_src, a_dst = sym.array("a_src"), sym.array("a_dst")
    u_src, u_dst = sym.array("u_src"), sym.array("u_dst")
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    cols = A.indices
    # the lower destination of every (row, column) pair
    lower = {(int(rows[e]), int(cols[e])): int(d) for e, d in zip(a_src, a_dst)}
    iperm = sym.array("iperm")
    assert (iperm[rows[u_src]] < iperm[cols[u_src]]).all()      # strictly upper in the permuted numbering
    for e, d in zip(u_src, u_dst):
        t = lower[(int(cols[e]), int(rows[e]))]                 # where the transposed entry goes
        f = front_of(foff, t)
        dq = int(ns[f] + bs[f])
        loc = t - foff[f]
        i, j = loc % dq, loc // dq                              # (row, column) of the transposed entry's place
        assert j < ns[f] and i >= j
        assert d == t
    # within each buffer (F: a_dst, FU: u_dst) every destination is distinct, and the two cover every entry once
    assert len(np.unique(a_dst)) == len(a_dst)
    assert len(np.unique(u_dst)) == len(u_dst)
    assert len(a_dst) + len(u_dst) == A.nnz
    assert u_dst.min() >= 0 and u_dst.max() < sym.sizes["front_doubles"]


def test_shared_analysis_keeps_its_lower_map():
    """building the upper map (first LU factor on a shared analysis) leaves what the symmetric factors read alone"""
    A = symmetrised_pattern(unsymmetric_pattern(seed=5))
    sym = Symbolic(A, leaf_size=16)
    before = (sym.array("a_src").copy(), sym.array("a_dst").copy(), dict(sym.sizes))
    sym.array("u_dst")
    np.testing.assert_array_equal(before[0], sym.array("a_src"))
    np.testing.assert_array_equal(before[1], sym.array("a_dst"))
    assert before[2] == sym.sizes


def test_symmetrised_pattern():
    A = unsymmetric_pattern(seed=7)
    S = symmetrised_pattern(A)
    assert S.has_canonical_format
    P = S.copy()
    P.data[:] = 1.0
    assert (P != P.T).nnz == 0                                  # structurally symmetric
    assert (S.diagonal() == A.diagonal()).all() and np.count_nonzero(np.diff(S.indptr)) == A.shape[0]
    assert abs(S - A).max() == 0.0                              # same values, explicit zeros added
    assert S.nnz >= A.nnz


def test_lu_entry_point_is_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "eigd_hip.h")).read()
    assert re.search(r"int eigd_factor_create_lu\(eigd_ctx\* ctx, eigd_symbolic\* s, const double\* hdata, "
                     r"eigd_factor\*\* out\);", text)
    assert "eigd_factor_create_lu" in _ffi.EXPORTED
    assert hasattr(_ffi.lib(), "eigd_factor_create_lu")
