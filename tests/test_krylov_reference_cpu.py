"""
The host reference of the short-recurrence step kernels (tests/krylov_reference.py) checked without a GPU, before
tests/test_gpu_krylov_steps.py lets it judge a kernel: driven as a solver it is the three-term CG of
tests/test_cg_solution_cpu.py and solves the system, a frozen column stays frozen, the exact dots are exact, and every
crafted state of the branch tests lands in the branch it was crafted for.
"""
import math

import numpy as np
import pytest

import krylov_reference as kr
from krylov_reference import ROWS
from test_cg_solution_cpu import _problem, _three_term_cg


def _drive(F, K, alpha, B, tol2, steps):
    """the reference as a solver on the columns of B: (psi, r, state, log, psi after every step)"""
    n, k = B.shape
    st = kr.blank_state(k, alpha, tol2)
    r, r_old = B.copy(), np.full((n, k), np.nan)
    psi, psi_old = np.zeros((n, k)), np.full((n, k), np.nan)
    log = np.zeros((2 * steps, k))
    norm2, trail = None, []
    for j in range(1, steps + 1):
        z = F @ r
        y = K @ z
        rz, _ = kr.exact_dots(r, z)
        zy, _ = kr.exact_dots(z, y)
        cs = kr.coef_step(st, rz, zy, norm2, j, j == 1)
        st = cs.state
        log[2 * (j - 1): 2 * j] = cs.log
        rn, _, pn, _ = kr.update_step(r, r_old, psi, psi_old, z, y, st[ROWS["gam_now"]], st[ROWS["rho_now"]],
                                      st[ROWS["alpha"]], j == 1)
        r, r_old = rn.astype(np.float64), r
        psi, psi_old = pn.astype(np.float64), psi
        norm2 = np.sum(r * r, axis=0)
        trail.append(psi.copy())
    return psi, r, st, log, trail


def test_the_reference_driven_as_a_solver_is_the_three_term_cg_and_solves_the_system():
    F, K, alpha, b = _problem()
    steps = 25
    psi_ref, _, log_ref, r_ref = _three_term_cg(F, K, alpha, b, steps)
    psi, r, st, log, _ = _drive(F, K, alpha, b[:, None], 0.0, steps)
    assert np.linalg.norm(psi[:, 0] - psi_ref) <= 1e-12 * np.linalg.norm(psi_ref)
    assert np.linalg.norm(r[:, 0] - r_ref) <= 1e-12 * np.linalg.norm(b)
    assert np.allclose(log[:, 0], log_ref[: 2 * steps, 0], rtol=1e-9, atol=0)     # (the scalars feel the conditioning of q)
    assert st[ROWS["flag"], 0] == 0.0 and st[ROWS["done"], 0] == 0.0
    res = b - (np.eye(len(b)) - alpha * K @ F) @ np.linalg.solve(F, psi[:, 0])
    assert np.linalg.norm(res) <= 1e-8 * np.linalg.norm(b)


def test_a_column_frozen_by_its_norm_keeps_its_iterate_bitwise():
    F, K, alpha, b = _problem(seed=1)
    B = np.stack([b, 0.5 * b[::-1]], axis=1)
    tol2 = np.array([1e-6 * (b @ b), 0.0])                    # column 0 freezes early, column 1 never
    psi, r, st, log, trail = _drive(F, K, alpha, B, tol2, 16)
    assert st[ROWS["done"], 0] == 1.0 and st[ROWS["done"], 1] == 0.0
    s = int(st[ROWS["steps"], 0])
    assert 1 <= s < 14
    for later in trail[s:]:                                   # trail[s - 1] is the iterate after step s
        assert np.array_equal(later[:, 0], trail[s - 1][:, 0])
    assert not np.array_equal(trail[s - 2][:, 0], trail[s - 1][:, 0])
    assert not log[2 * s:: 2, 0].any() and np.all(log[: 2 * s: 2, 0] > 0.0)
    assert not np.array_equal(trail[-1][:, 1], trail[-2][:, 1])


@pytest.mark.parametrize("n,k", [(1, 1), (257, 3), (4001, 2)])
def test_exact_dots_are_the_rounded_exact_sums(n, k):
    from fractions import Fraction

    rng = np.random.default_rng(n)
    X, Y = rng.normal(size=(n, k)), rng.normal(size=(n, k))
    if n > 2:
        X[0], Y[0] = 1e10, 1.0 + rng.uniform(size=k)
        X[n // 2], Y[n // 2] = -1e10, Y[0]
    d, s = kr.exact_dots(X, Y)
    for c in range(k):
        exact = sum(Fraction(a) * Fraction(b) for a, b in zip(X[:, c].tolist(), Y[:, c].tolist()))
        assert d[c] == float(exact)
        assert d[c] == math.fsum(kr.two_prod_terms(X[:, c], Y[:, c]))     # the array form is the scalar one
        sabs = float(sum(abs(Fraction(a) * Fraction(b)) for a, b in zip(X[:, c].tolist(), Y[:, c].tolist())))
        assert sabs <= s[c] <= sabs * (1.0 + 1e-11)                          # a scale for bounds: never below the sum


@pytest.mark.parametrize("name", kr.BRANCH_CASES)
def test_crafted_states_land_in_their_branches(name):
    case = kr.branch_case(name)
    st = case["state"]
    seen = set()
    for call in case["calls"]:
        rz, _ = kr.exact_dots(call["R"], call["Z"])
        zy, _ = kr.exact_dots(call["Z"], call["Y"])
        cs = kr.coef_step(st, rz, zy, call["norm2"], call["step"], call["first"])
        assert cs.branch == call["expect"], (name, cs.branch)
        # well inside its branch: no rounding of a device sum can move it across (the sums are exact to 1e-13 relative)
        for c, b in enumerate(cs.branch):
            if b == "restart":
                assert cs.q[c] < -1.0
            if b == "moves" and not call["first"]:
                assert cs.q[c] > 0.1
            if b == "breakdown":
                assert min(rz[c], float(cs.den[c])) < -1e-3 * abs(rz[c])
        st = cs.state
        seen.update(cs.branch)
    want = {"restart": {"restart", "moves"}, "den": {"breakdown", "moves"}, "rr_neg": {"breakdown", "moves"},
            "vanished": {"vanished", "moves"}, "frozen": {"frozen-now", "frozen-before", "moves"}}[name]
    assert seen == want
    if name in ("den", "rr_neg"):                              # the record is the first occurrence's
        assert np.all(st[ROWS["bad_step"], 1:] == 4.0) and st[ROWS["bad_step"], 0] == 0.0
        assert np.all(st[ROWS["flag"], 1:] == 2.0) and st[ROWS["flag"], 0] == 0.0
        if name == "den":
            assert np.all(st[ROWS["bad_rr"], 1:] > 0.0) and np.all(st[ROWS["bad_den"], 1:] < 0.0)
        else:
            assert np.all(st[ROWS["bad_rr"], 1:] < 0.0)
    if name == "restart":
        assert list(st[ROWS["flag"]]) == [1.0, 2.0, 1.0, 0.0, 1.0, 1.0]
        assert np.all(st[ROWS["rho"], [0, 1, 2, 4, 5]] == 1.0) and st[ROWS["rho"], 3] != 1.0
    if name == "frozen":
        assert list(st[ROWS["done"]]) == [0.0, 1.0, 0.0, 1.0, 1.0, 0.0]
        assert list(st[ROWS["steps"]]) == [0.0, 5.0, 0.0, 2.0, 5.0, 0.0]


def test_the_pair_references_orthogonalise():
    rng = np.random.default_rng(4)
    n, k, ns = 200, 3, 5
    Q = [np.linalg.qr(rng.normal(size=(n, ns)))[0] for _ in range(k)]
    S = [np.stack([Q[c][:, j] for c in range(k)], axis=1) for j in range(ns)]
    T = rng.normal(size=(n, 2 * k))
    H, Tn = kr.cgs2_pair_ref(S, T)
    Tn = Tn.astype(np.float64)
    for c in range(2 * k):
        assert np.abs(Q[c % k].T @ Tn[:, c]).max() < 1e-13
    n1 = np.sum(Tn[:, :k] ** 2, axis=0)
    n1[1] = 0.0
    W1, T2n, W2, out = kr.pair_orthonormalise_ref(Tn, n1, [False, False, True])
    W1, T2n, W2 = (a.astype(np.float64) for a in (W1, T2n, W2))
    assert abs(W1[:, 0] @ W1[:, 0] - 1) < 1e-14 and abs(W2[:, 0] @ W2[:, 0] - 1) < 1e-14 and abs(W1[:, 0] @ W2[:, 0]) < 1e-14
    assert not W1[:, 1:].any() and not T2n[:, 1:].any() and not W2[:, 1:].any()
    assert not out[2 * k + 1:3 * k].any() and not out[3 * k + 1:].any() and np.all(np.isfinite(out.astype(np.float64)))
