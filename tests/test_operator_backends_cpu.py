"""
Host side of SpLuOperator's backends (no device): the table (kind, trans, conjugate) -> (herm, wrap) of the full-complex
application, restated on a dense 6 x 6 complex matrix with numpy's solve standing in for the factor, and the library's symbol
list.

Gate: 1e-12 relative -- far above the rounding of a well conditioned 6 x 6 solve (1e-15), far below a wrong branch of
the table, which applies another matrix and is off by O(1).
"""
import numpy as np
import pytest

TOL = 1e-12


def dense_complex(kind, seed=0):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(6, 6)) + 1j * rng.normal(size=(6, 6)) + 6.0 * np.eye(6)
    return (A + A.T) / 2 if kind == "ldlt" else A          # the symmetric form factors complex symmetric matrices


@pytest.mark.parametrize("kind", ["lu", "ldlt"])
def test_application_table(kind):
    from eigd_amd.operators import complex_application

    A = dense_complex(kind)
    if kind == "ldlt":
        assert np.array_equal(A, A.T) and not np.allclose(A, A.conj().T)
    rng = np.random.default_rng(1)
    B = rng.normal(size=(6, 3)) + 1j * rng.normal(size=(6, 3))
    want = {(False, False): A, (True, False): A.T, (True, True): A.conj().T, (False, True): A.conj()}
    seen = set()
    for trans in (False, True):
        for conjugate in (False, True):
            for as_int in (False, True):                   # the drivers pass flags and 0 / 1 alike
                t, c = (int(trans), int(conjugate)) if as_int else (trans, conjugate)
                herm, wrap = complex_application(kind, t, c)
                assert isinstance(herm, bool) and isinstance(wrap, bool)
                Z = B.conj() if wrap else B.copy()
                Z = np.linalg.solve(A.conj().T if herm else A, Z)      # the raw solve: mat^{-1} or mat^{-H}
                X = Z.conj() if wrap else Z
                ref = np.linalg.solve(want[(trans, conjugate)], B)
                assert np.linalg.norm(X - ref) <= TOL * np.linalg.norm(ref), (kind, trans, conjugate)
                seen.add((trans, conjugate, as_int))
    assert len(seen) == 8
    if kind == "ldlt":                                     # mat = mat^T: never between conjugations
        assert all(not complex_application(kind, t, c)[1] for t in (0, 1) for c in (0, 1))


def test_exported_symbols_unchanged():
    """the operator layer is Python over an unchanged library: the symbol list is the one it was (a change of the C ABI
    moves this pin with it)"""
    import hashlib

    from eigd_amd import _ffi

    names = sorted(_ffi.EXPORTED)
    assert len(names) == len(set(names)) == 107
    assert hashlib.blake2b("\n".join(names).encode(), digest_size=8).hexdigest() == "8617eaffc6fe1632"
