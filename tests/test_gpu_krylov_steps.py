"""
The per-step kernels of the short-recurrence sibk (csrc/krylov.hip: cg_dots / cg_coef / cg_update / cg_norm through
eigd_cg_coefficients, eigd_spmm_cg, eigd_cg_update) and the two-steps-per-pass Gram-Schmidt form (csrc/dense.hip:
eigd_stack_cgs2_pair, eigd_pair_orthonormalise, eigd_stack_axpy_dev) against tests/krylov_reference.py, one call at a
time.  Every expectation is step-local: formed from exactly rounded inner products and from what the device itself held
before the call, with tolerances derived from the launch geometry (krylov_reference.cg_chain), never from what the device
returned.

Every block is wider than its k columns (pad columns of NaN), state and log are passed as base + C0 inside rows of 64
filled with a sentinel, and all of that must come back bitwise unchanged.
"""
import ctypes as C
import functools

import numpy as np
import pytest
from scipy import sparse

import krylov_reference as kr
from krylov_reference import EPS, NROWS, ROWS

pytestmark = pytest.mark.gpu

C0 = 5              # first column of the block inside the state / log rows
PAD = 3             # pad columns of every block
SENT = -7.25e77     # what state / log hold outside the block
MOVING = ("moves", "restart")


@pytest.fixture(scope="module")
def ctx():
    from eigd_amd import _ffi
    from eigd_amd.device import default_context

    assert int(_ffi.lib().eigd_cg_state_rows()) == NROWS
    return default_context()


def call(name, *args):
    from eigd_amd._ffi import call as c

    c(name, *args)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


class Rows64:
    """rows of 64 doubles (the state block, the log) handed to the library as base + C0; one spare row for k > 59"""

    def __init__(self, ctx, nrows, k, block=None):
        self.nrows, self.k = nrows, k
        self.idx = 64 * np.arange(nrows)[:, None] + C0 + np.arange(k)[None, :]
        host = np.full((nrows + 1) * 64, SENT)
        if block is not None:
            host[self.idx] = block
        self.dev = ctx.from_host(host.reshape(nrows + 1, 64))
        self.ptr = self.dev.cols(C0, 64).ptr

    def flat(self):
        return self.dev.get().ravel().copy()

    def block(self, flat):
        return flat[self.idx]

    def set_block(self, block):
        host = self.flat()
        host[self.idx] = block
        self.dev.set(host.reshape(self.nrows + 1, 64))

    def only_changed(self, before, after, rows):
        """nothing but columns [C0, C0 + k) of `rows` differs between the two flat copies"""
        keep = np.ones(before.size, dtype=bool)
        keep[self.idx[list(rows)].ravel()] = False
        return np.array_equal(bits(before)[keep], bits(after)[keep])


class Padded:
    """an n x k block inside an n x (k + PAD) allocation whose pad columns hold NaN"""

    def __init__(self, ctx, A):
        n, k = A.shape
        self.k = k
        self.full = np.full((n, k + PAD), np.nan)
        self.full[:, :k] = A
        self.dev = ctx.from_host(self.full)
        self.v = self.dev.cols(0, k)

    def get(self):
        out = self.dev.get()
        assert same_bits(out[:, self.k:], self.full[:, self.k:]), "pad columns were written"
        return np.array(out[:, :self.k])

    def set(self, A):
        self.full[:, :self.k] = A
        self.dev.set(self.full)


SHAPES = [(1, 1), (7, 5), (4099, 3), (4099, 17), (20011, 32),
          (22403, 64),    # 700 workgroups of cg_dots: one unrolled trip of wave_sum_partials (512) plus its remainder
          (40003, 33),    # grid cap: 1024 workgroups, two grid-stride trips
          (40003, 64)]


@functools.lru_cache(maxsize=None)
def inputs(n, k):
    """r, z = f r (f > 0: r.z is a sum of positive terms), y = g z (g > 0: z.y likewise), alpha < 0: den = rr + |alpha| z.y
    does not cancel either; every entry its own seeded number, no two columns alike.  The exact dots are formed once."""
    rng = np.random.default_rng(1000 * n + k)
    R = rng.normal(size=(n, k))
    Z = rng.uniform(0.5, 2.0, size=(n, k)) * R
    Y = rng.uniform(0.5, 2.0, size=(n, k)) * Z
    alpha = -rng.uniform(0.1, 0.5, size=k)
    rz, s_rz = kr.exact_dots(R, Z)
    zy, s_zy = kr.exact_dots(Z, Y)
    return {"R": R, "Z": Z, "Y": Y, "alpha": alpha, "rz": rz, "s_rz": s_rz, "zy": zy, "s_zy": s_zy,
            "Rold": rng.normal(size=(n, k)), "Psi": rng.normal(size=(n, k)), "PsiOld": rng.normal(size=(n, k)), "rng": rng}


def previous_state(inp, k, first):
    st = kr.blank_state(k, inp["alpha"])
    if not first:   # a hand-written previous step: (gam/gam')(rr/rr')/rho' <= (1/0.8)(1/2) -- q stays above 0.3
        rng = np.random.default_rng(k)
        st[ROWS["rr"]] = inp["rz"] * rng.uniform(2.0, 4.0, size=k)
        st[ROWS["gam"]] = rng.uniform(0.8, 1.2, size=k)
        st[ROWS["rho"]] = rng.uniform(1.0, 1.3, size=k)
    return st


def check_coef(state, log, s_before, s_after, l_before, l_after, cs, tol, step):
    """the state block and the two log rows of `step` against the reference within tol = (e_rr, e_gam, e_rho) per column"""
    k = state.k
    dev, ref = state.block(s_after), cs.state
    moving = np.array([b in MOVING for b in cs.branch])
    e_rr, e_gam, e_rho = (np.where(moving & np.isfinite(e), e + 2 * EPS, 0.0) for e in tol[:3])
    for row, e in (("rr", e_rr), ("gam", e_gam), ("rho", e_rho), ("gam_now", e_gam), ("rho_now", e_rho)):
        d, r = dev[ROWS[row]], ref[ROWS[row]]
        err = np.abs(d - r)
        print(f"step {step} row {row}: max err / bound = {np.max(err / np.maximum(e * np.abs(r), 1e-300) * (e > 0)):.3g}")
        assert np.all(err <= e * np.abs(r)), (row, d, r, e)
    for row in ("done", "tol2", "alpha", "steps", "flag", "bad_step"):
        assert same_bits(dev[ROWS[row]], ref[ROWS[row]]), (row, dev[ROWS[row]], ref[ROWS[row]])
    for c in range(k):
        if cs.branch[c] in MOVING:   # the two copies of this step's numbers are one number
            assert dev[ROWS["gam_now"], c] == dev[ROWS["gam"], c] and dev[ROWS["rho_now"], c] == dev[ROWS["rho"], c]
    assert state.only_changed(s_before, s_after, range(NROWS))
    lrows = [2 * (step - 1), 2 * (step - 1) + 1]
    assert log.only_changed(l_before, l_after, lrows)
    assert same_bits(log.block(l_after)[lrows], dev[[ROWS["gam_now"], ROWS["rho_now"]]])


def coef_tolerances(cs, st, inp, m):
    tol = kr.coef_bounds(cs, st, inp["rz"], inp["s_rz"], inp["zy"], inp["s_zy"], m)
    moving = np.array([b in MOVING for b in cs.branch])
    worst = max(float(np.max(np.where(moving & np.isfinite(e), e, 0.0))) for e in tol[:3])
    return tol, worst


@pytest.mark.parametrize("first", [1, 0])
@pytest.mark.parametrize("n,k", SHAPES)
def test_coefficients_of_one_step_against_exact_dots(ctx, n, k, first):
    """eigd_cg_coefficients: rr, gam, rho, gamNow, rhoNow and the log rows within the bound of the launch geometry"""
    inp = inputs(n, k)
    step = 1 if first else 4
    st = previous_state(inp, k, first)
    norm2 = None if first else 1e6 * np.ones(k)              # (given and far above the tolerance, or null)
    cs = kr.coef_step(st, inp["rz"], inp["zy"], norm2, step, first)
    assert all(b == "moves" for b in cs.branch)
    # longest chain of additions of cg_dots_kernel + wave_sum_partials for this shape: the rows one thread walks
    # (ceil(n / (workgroups RP)), 8 below the grid cap), the RP partial sums of a workgroup added by one thread, the
    # partials one lane of the coefficient kernel walks (every 64th workgroup), the 6 levels of the shuffle tree;
    # coef_bounds adds the rounding of the product
    m = kr.cg_chain(n, k, 8)
    tol, worst = coef_tolerances(cs, st, inp, m)
    print(f"n={n} k={k} geometry {kr.cg_geometry(n, k, 8)} chain {m} worst relative bound {worst:.3g}")
    assert worst < 1e-12
    R, Z, Y = (Padded(ctx, inp[x]) for x in "RZY")
    state, log = Rows64(ctx, NROWS, k, st), Rows64(ctx, 8, k)
    n2 = None if norm2 is None else Padded(ctx, norm2[None, :])
    s0, l0 = state.flat(), log.flat()
    call("eigd_cg_coefficients", ctx.h, n, k, Z.v.ptr, Z.v.ld, R.v.ptr, R.v.ld, Y.v.ptr, Y.v.ld,
         None if n2 is None else n2.v.ptr, state.ptr, step, first, log.ptr)
    check_coef(state, log, s0, state.flat(), l0, log.flat(), cs, tol, step)
    for blk, x in ((R, "R"), (Z, "Z"), (Y, "Y")):
        assert same_bits(blk.get(), inp[x])


def product_pass_case(A, k, first, seed=None):
    """host side of one eigd_spmm_cg call on the matrix A (z.Az dominated by its positive terms): inputs, exact inner
    products, the expected step and its tolerances (shared with tests/test_gpu_product_variants.py)"""
    n = A.shape[0]
    rng = np.random.default_rng(k if seed is None else seed)
    Rh = rng.normal(size=(n, k))
    Zh = rng.uniform(0.5, 2.0, size=(n, k)) * Rh
    Yh = A @ Zh
    inp = {"alpha": -rng.uniform(0.1, 0.5, size=k)}
    inp["rz"], inp["s_rz"] = kr.exact_dots(Rh, Zh)
    inp["zy"], inp["s_zy"] = kr.exact_dots(Zh, Yh)
    step = 1 if first else 3
    st = previous_state(inp, k, first)
    cs = kr.coef_step(st, inp["rz"], inp["zy"], None, step, first)
    # chain of the fused pass: one product-and-add per lane (a tile row), 3 shuffle levels over the 8 rows of a wave, the
    # 4 waves of the tile, then tile_dots_reduce_kernel (tiles per thread, `per` partial sums) and wave_sum_partials
    ntiles = -(-n // 32)
    groups, per = min(ntiles, 1024), 256 // (2 * k)
    m_fused = 1 + 3 + 4 + -(-ntiles // (groups * per)) + per + -(-groups // 64) + 6
    m = max(m_fused, kr.cg_chain(n, k, 8))                    # (whichever form the library picks for this matrix)
    tol, worst = coef_tolerances(cs, st, inp, m)
    print(f"k={k} chain {m} worst relative bound {worst:.3g}")
    assert worst < 1e-12
    return {"k": k, "first": first, "step": step, "R": Rh, "Z": Zh, "Y": Yh, "st": st, "cs": cs, "tol": tol}


def run_product_pass(ctx, dA, case):
    """one eigd_spmm_cg call for a product_pass_case: y bitwise the plain product, coefficients within the bound; returns
    (y, the state block) as the device left them"""
    k, step, first = case["k"], case["step"], case["first"]
    n = case["R"].shape[0]
    R, Z, Y = Padded(ctx, case["R"]), Padded(ctx, case["Z"]), Padded(ctx, np.full((n, k), np.nan))
    state, log = Rows64(ctx, NROWS, k, case["st"]), Rows64(ctx, 8, k)
    s0, l0 = state.flat(), log.flat()
    call("eigd_spmm_cg", ctx.h, dA.h, k, Z.v.ptr, Z.v.ld, Y.v.ptr, Y.v.ld, R.v.ptr, R.v.ld, None, state.ptr, step, first,
         log.ptr)
    y = Y.get()
    assert same_bits(y, case["Y"])
    s1 = state.flat()
    check_coef(state, log, s0, s1, l0, log.flat(), case["cs"], case["tol"], step)
    return y, state.block(s1)


@pytest.mark.parametrize("first", [1, 0])
@pytest.mark.parametrize("k", [5, 17, 32])
def test_coefficients_out_of_the_product_pass_against_exact_dots(ctx, k, first):
    """eigd_spmm_cg on a tiled matrix (5 <= k <= 32): y bitwise the plain product, coefficients within the bound"""
    from eigd_amd.device import CSRMatrix
    from test_symbolic_cpu import grid_matrix

    A = grid_matrix(61, 47, 2, seed=k)
    A = (A + A.T).tocsr()                                     # diagonally dominant: z.Az is dominated by positive terms
    run_product_pass(ctx, CSRMatrix(ctx, A), product_pass_case(A, k, first))


# ---- the update ---------------------------------------------------------------------------------------------------------

def update_case(inp, k, shift):
    """per column: 0 a three-term step (rho != 1), 1 a two-term step (rho == 1.0 exactly), 2 a column that does not move"""
    kind = (np.arange(k) + shift) % 3
    rng = np.random.default_rng(7 * k + shift)
    gam = np.where(kind == 2, 0.0, rng.uniform(0.3, 0.9, size=k))
    rho = np.where(kind == 0, rng.uniform(1.05, 1.4, size=k), 1.0)
    return kind, gam, rho


_norm_cache = {}


def exact_norm2(r):
    """exact squared column norms, formed once per distinct block (the PSI-on and PSI-off residuals are the same bits)"""
    key = r.tobytes()
    if key not in _norm_cache:
        if len(_norm_cache) > 4:
            _norm_cache.clear()
        _norm_cache[key] = kr.exact_dots(r, r)[0]
    return _norm_cache[key]


def check_update(ctx, n, k, inp, kind, gam, rho, first, with_psi, with_norm, expect=None):
    alpha = inp["alpha"]
    three = (kind == 0) & (not first)
    moves = kind != 2
    # what the kernel must not read holds NaN: r_old / psi_old outside the three-term columns (the solver hands
    # uninitialised memory there), y and z where the column does not move
    Rold = np.where(three, inp["Rold"], np.nan)
    PsiOld = np.where(three, inp["PsiOld"], np.nan)
    Yh, Zh = np.where(moves, inp["Y"], np.nan), np.where(moves, inp["Z"], np.nan)
    st = kr.blank_state(k, alpha)
    st[ROWS["gam_now"]], st[ROWS["rho_now"]] = gam, rho
    st[ROWS["gam"]], st[ROWS["rho"]], st[ROWS["rr"]] = 0.77, 1.9, 3.3     # (rows of the previous step: not the update's)
    if expect is None:                                        # (the residual's reference is the same with and without psi)
        expect = kr.update_step(inp["R"], Rold, inp["Psi"], PsiOld, Zh, Yh, gam, rho, alpha, first)
    rn, ra, pn, pa = expect
    R, Y, Z, Psi = Padded(ctx, inp["R"]), Padded(ctx, Yh), Padded(ctx, Zh), Padded(ctx, inp["Psi"])
    state = Rows64(ctx, NROWS, k, st)
    s0 = state.flat()
    runs = []
    for _ in range(2):
        Ro, Po = Padded(ctx, Rold), Padded(ctx, PsiOld)
        n2 = Padded(ctx, np.full((1, k), np.nan)) if with_norm else None
        call("eigd_cg_update", ctx.h, n, k, R.v.ptr, R.v.ld, Ro.v.ptr, Ro.v.ld, Psi.v.ptr if with_psi else None, Psi.v.ld,
             Po.v.ptr, Po.v.ld, Z.v.ptr, Z.v.ld, Y.v.ptr, Y.v.ld, state.ptr, first, n2.v.ptr if with_norm else None)
        runs.append((Ro.get(), Po.get(), n2.get()[0] if with_norm else None))
    assert same_bits(state.flat(), s0)
    for blk, ref in ((R, inp["R"]), (Y, Yh), (Z, Zh), (Psi, inp["Psi"])):
        assert same_bits(blk.get(), ref)
    r_new, p_new, norm2 = runs[0]
    assert same_bits(r_new, runs[1][0]) and same_bits(p_new, runs[1][1])          # no atomics: repeats are bitwise equal
    # eight roundings at most on the way to an entry (1 - rho, the products, the sums; fused multiply-adds remove some)
    err = np.abs(r_new.astype(np.longdouble) - rn)
    assert np.all(np.isfinite(r_new)) and np.all(err <= 8 * EPS * ra), float(np.max(err / ra))
    assert same_bits(r_new[:, ~moves], inp["R"][:, ~moves])                       # a column that does not move is a copy
    if with_psi:
        err = np.abs(p_new.astype(np.longdouble) - pn)
        assert np.all(np.isfinite(p_new)) and np.all(err <= 8 * EPS * pa), float(np.max(err / pa))
        assert same_bits(p_new[:, ~moves], inp["Psi"][:, ~moves])
    else:
        assert same_bits(p_new, PsiOld)                                           # untouched
    if with_norm:
        assert same_bits(norm2, runs[1][2])
        exact = exact_norm2(r_new)
        # cg_update_kernel walks 4 rows per thread below the grid cap; the chain is that of the dots otherwise, and one
        # more rounding for the square
        m = kr.cg_chain(n, k, 4) + 1
        bound = m * EPS / (1 - m * EPS) * exact + 2 * EPS * exact
        assert np.all(np.abs(norm2 - exact) <= bound), (norm2, exact, m)
    return r_new, expect


@pytest.mark.parametrize("with_norm", [True, False])
@pytest.mark.parametrize("n,k", SHAPES)
def test_update_of_one_step(ctx, n, k, with_norm):
    """
    eigd_cg_update with and without the solution recurrence (PSI on / off), first and later steps, over a mix of
    three-term, two-term (rho == 1.0) and non-moving columns.  The residual of the PSI-off instantiation is compared with
    the PSI-on one under the same bound (and, as the assertion below records, found bitwise equal: the residual's
    arithmetic is the same expression in both instantiations).
    """
    inp = inputs(n, k)
    for shift in (range(3) if k < 3 else (0,)):
        kind, gam, rho = update_case(inp, k, shift)
        for first in (0, 1):
            r_on, ref = check_update(ctx, n, k, inp, kind, gam, rho, first, True, with_norm)
            r_off, _ = check_update(ctx, n, k, inp, kind, gam, rho, first, False, with_norm, ref)
            print(f"n={n} k={k} first={first}: PSI off bitwise equal to PSI on: {same_bits(r_on, r_off)}")
            assert same_bits(r_on, r_off)


# ---- the branches of the coefficient kernel -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", kr.BRANCH_CASES)
def test_branches_of_the_coefficient_kernel(ctx, name):
    """restart (q <= 0), breakdown by den <= 0 and by rr < 0 (first occurrence recorded), vanished residual, freezing by
    the norm (strict comparison): one call each from a crafted state; a following update copies what does not move"""
    case = kr.branch_case(name)
    st = case["state"]
    k = st.shape[1]
    state, log = Rows64(ctx, NROWS, k, st), Rows64(ctx, 16, k)
    for cl in case["calls"]:
        n = cl["R"].shape[0]
        inp = {"alpha": st[ROWS["alpha"]]}
        inp["rz"], inp["s_rz"] = kr.exact_dots(cl["R"], cl["Z"])
        inp["zy"], inp["s_zy"] = kr.exact_dots(cl["Z"], cl["Y"])
        s0, l0 = state.flat(), log.flat()
        before = state.block(s0)
        cs = kr.coef_step(before, inp["rz"], inp["zy"], cl["norm2"], cl["step"], cl["first"])
        assert cs.branch == cl["expect"]
        tol = kr.coef_bounds(cs, before, inp["rz"], inp["s_rz"], inp["zy"], inp["s_zy"], kr.cg_chain(n, k, 8))
        R, Z, Y = Padded(ctx, cl["R"]), Padded(ctx, cl["Z"]), Padded(ctx, cl["Y"])
        n2 = None if cl["norm2"] is None else Padded(ctx, cl["norm2"][None, :])
        call("eigd_cg_coefficients", ctx.h, n, k, Z.v.ptr, Z.v.ld, R.v.ptr, R.v.ld, Y.v.ptr, Y.v.ld,
             None if n2 is None else n2.v.ptr, state.ptr, cl["step"], cl["first"], log.ptr)
        s1 = state.flat()
        check_coef(state, log, s0, s1, l0, log.flat(), cs, tol, cl["step"])
        dev = state.block(s1)
        for c, b in enumerate(cs.branch):
            if b == "restart":
                assert dev[ROWS["rho"], c] == 1.0 and dev[ROWS["rho_now"], c] == 1.0 and dev[ROWS["gam_now"], c] > 0.0
                assert dev[ROWS["flag"], c] == (1.0 if before[ROWS["flag"], c] == 0.0 else before[ROWS["flag"], c])
                assert dev[ROWS["rr"], c] != before[ROWS["rr"], c] and dev[ROWS["gam"], c] != before[ROWS["gam"], c]
            if b == "breakdown":
                assert dev[ROWS["flag"], c] == 2.0 and dev[ROWS["gam_now"], c] == 0.0 and dev[ROWS["rho_now"], c] == 1.0
                assert same_bits(dev[[0, 1, 2], c], before[[0, 1, 2], c])             # rr, gam, rho of the last good step
                bad = dev[[ROWS["bad_rr"], ROWS["bad_den"]], c]
                if before[ROWS["flag"], c] == 2.0:                                    # not the first occurrence: kept
                    assert same_bits(bad, before[[ROWS["bad_rr"], ROWS["bad_den"]], c])
                else:
                    ref = cs.state[[ROWS["bad_rr"], ROWS["bad_den"]], c]      # within the bounds of the two sums
                    assert np.all(np.abs(bad - ref) <= (np.array([tol[0][c], tol[3][c]]) + 2 * EPS) * np.abs(ref)) and np.min(bad) < 0.0
            if b == "vanished":
                assert dev[ROWS["flag"], c] == 0.0 and dev[ROWS["gam_now"], c] == 0.0 and dev[ROWS["done"], c] == 0.0
            if b == "frozen-now":
                assert dev[ROWS["done"], c] == 1.0 and dev[ROWS["steps"], c] == cl["step"] - 1 and dev[ROWS["gam_now"], c] == 0.0
            if b == "frozen-before":
                assert dev[ROWS["done"], c] == 1.0 and dev[ROWS["steps"], c] == before[ROWS["steps"], c]
        # the update that follows: what does not move is copied, bitwise
        rng = np.random.default_rng(1)
        Ro = Padded(ctx, rng.normal(size=(n, k)))
        call("eigd_cg_update", ctx.h, n, k, R.v.ptr, R.v.ld, Ro.v.ptr, Ro.v.ld, None, 0, None, 0, None, 0, Y.v.ptr, Y.v.ld,
             state.ptr, cl["first"], None)
        still = np.array([b not in MOVING for b in cs.branch])
        out = Ro.get()
        assert same_bits(out[:, still], cl["R"][:, still])
        assert not np.any(np.all(out[:, ~still] == cl["R"][:, ~still], axis=0))
    final = state.block(state.flat())
    if name in ("den", "rr_neg"):
        assert np.all(final[ROWS["bad_step"], 1:] == 4.0) and final[ROWS["bad_step"], 0] == 0.0


def test_a_denominator_of_exactly_zero_is_a_restart(ctx):
    """
    The boundary of the restart branch, q == 0: the same call twice, first as a first step and then as a later one.  The
    sums are bitwise reproducible (no atomics), so the second call sees gam/gam' == 1, rr/rr' == 1, rho' == 1 and
    q = 1 - 1 == 0 exactly: not positive, hence rho = 1 and flag 1 -- not a division by zero.
    """
    n, k = 4099, 17
    inp = inputs(n, k)
    R, Z, Y = (Padded(ctx, inp[x]) for x in "RZY")
    state, log = Rows64(ctx, NROWS, k, kr.blank_state(k, inp["alpha"])), Rows64(ctx, 4, k)
    for step, first in ((1, 1), (2, 0)):
        call("eigd_cg_coefficients", ctx.h, n, k, Z.v.ptr, Z.v.ld, R.v.ptr, R.v.ld, Y.v.ptr, Y.v.ld, None, state.ptr, step, first,
             log.ptr)
        dev = state.block(state.flat())
        if first:
            one = dev.copy()
            assert np.all(dev[ROWS["flag"]] == 0.0) and np.all(dev[ROWS["gam_now"]] > 0.0)
    assert same_bits(dev[[0, 1, 2]], one[[0, 1, 2]])           # rr, gam the same bits; rho = 1 again
    assert np.all(dev[ROWS["rho_now"]] == 1.0) and np.all(dev[ROWS["flag"]] == 1.0)
    lg = log.block(log.flat())
    assert same_bits(lg[0:2], lg[2:4])


# ---- several steps in a row -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [6, 32, 48])
def test_steps_in_a_row_freeze_their_columns_and_keep_the_invariants(ctx, k):
    """
    F a positive diagonal, K a negative definite tridiagonal matrix (y = K z on the host), alpha > 0, the buffers swapped as
    adjoint.py swaps them; tolerances spread over sixteen decades so that the columns freeze at different steps.  Every
    call is checked step-locally as in the single-step tests; at the end the bookkeeping (done, steps), the residual
    invariant, the frozen columns and the solution formed from the z history and the log.
    """
    n, maxsteps = 20011, 30
    rng = np.random.default_rng(k)
    f = rng.uniform(0.5, 2.0, size=n)
    K = -sparse.diags([-np.ones(n - 1), 2.1 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr")
    alpha = rng.uniform(0.2, 0.3, size=k)                     # C = I - alpha K F: eigenvalues in [1, 3.5] in the F inner product
    B = rng.normal(size=(n, k))
    b2 = np.sum(B * B, axis=0)
    tol2 = b2 * 10.0 ** -np.linspace(4.0, 20.0, k)
    st = kr.blank_state(k, alpha, tol2)
    state, log = Rows64(ctx, NROWS, k, st), Rows64(ctx, 2 * maxsteps, k)
    nan = np.full((n, k), np.nan)
    r, r_old, psi, psi_old = Padded(ctx, B), Padded(ctx, nan), Padded(ctx, np.zeros((n, k))), Padded(ctx, nan)
    Z, Y = Padded(ctx, nan), Padded(ctx, nan)
    n2 = [Padded(ctx, np.full((1, k), np.nan)) for _ in range(2)]
    hist = ctx.stack(maxsteps, n, k + PAD)
    rh, ph = B.copy(), np.zeros((n, k))
    norms, frozen_r, frozen_psi = [], {}, {}
    m8, m4 = kr.cg_chain(n, k, 8), kr.cg_chain(n, k, 4) + 1
    nsteps = 0
    for j in range(1, maxsteps + 1):
        first = 1 if j == 1 else 0
        zh = f[:, None] * rh
        yh = K @ zh
        Z.set(zh)
        Y.set(yh)
        s0, l0 = state.flat(), log.flat()
        before = state.block(s0)
        norm2_in = None if j == 1 else norms[-1]
        call("eigd_cg_coefficients", ctx.h, n, k, Z.v.ptr, Z.v.ld, r.v.ptr, r.v.ld, Y.v.ptr, Y.v.ld,
             None if j == 1 else n2[j % 2].v.ptr, state.ptr, j, first, log.ptr)
        s1 = state.flat()
        live = np.flatnonzero(before[ROWS["done"]] == 0.0)    # (a frozen column's sums are looked at by nobody)
        inp = {x: np.zeros(k) for x in ("rz", "s_rz", "zy", "s_zy")}
        inp["rz"][live], inp["s_rz"][live] = kr.exact_dots(rh[:, live], zh[:, live])
        inp["zy"][live], inp["s_zy"][live] = kr.exact_dots(zh[:, live], yh[:, live])
        cs = kr.coef_step(before, inp["rz"], inp["zy"], norm2_in, j, first)
        assert set(cs.branch) <= {"moves", "frozen-now", "frozen-before"}, cs.branch
        check_coef(state, log, s0, s1, l0, log.flat(), cs, kr.coef_bounds(cs, before, inp["rz"], inp["s_rz"], inp["zy"], inp["s_zy"], m8), j)
        dev = state.block(s1)
        gam, rho = dev[ROWS["gam_now"]], dev[ROWS["rho_now"]]
        slab = np.full((n, k + PAD), np.nan)                  # the history keeps z only where the column moved
        slab[:, :k] = np.where(gam != 0.0, zh, np.nan)
        hist[j - 1].set(slab)
        for c in np.flatnonzero(gam == 0.0):
            frozen_r.setdefault(int(c), rh[:, c].copy())
            frozen_psi.setdefault(int(c), ph[:, c].copy())
        call("eigd_cg_update", ctx.h, n, k, r.v.ptr, r.v.ld, r_old.v.ptr, r_old.v.ld, psi.v.ptr, psi.v.ld, psi_old.v.ptr,
             psi_old.v.ld, Z.v.ptr, Z.v.ld, Y.v.ptr, Y.v.ld, state.ptr, first, n2[(j + 1) % 2].v.ptr)
        rn, ra, pn, pa = kr.update_step(rh, r_old.full[:, :k] if j == 1 else rh_old, ph, psi_old.full[:, :k] if j == 1 else ph_old,
                                        zh, yh, gam, rho, alpha, first)
        r_new, p_new = r_old.get(), psi_old.get()
        assert np.all(np.abs(r_new.astype(np.longdouble) - rn) <= 8 * EPS * ra)
        assert np.all(np.abs(p_new.astype(np.longdouble) - pn) <= 8 * EPS * pa)
        for c in frozen_r:
            assert same_bits(r_new[:, c], frozen_r[c]) and same_bits(p_new[:, c], frozen_psi[c])
        nrm = n2[(j + 1) % 2].get()[0]
        exact = np.array(exact) if j > 1 else np.zeros(k)     # (a column that was copied has the norm it had)
        fresh = np.flatnonzero(gam != 0.0) if j > 1 else np.arange(k)
        if len(fresh):
            exact[fresh] = kr.exact_dots(r_new[:, fresh], r_new[:, fresh])[0]
        assert np.all(np.abs(nrm - exact) <= (m4 * EPS / (1 - m4 * EPS) + 2 * EPS) * exact)
        norms.append(nrm)
        rh_old, ph_old, rh, ph = rh, ph, r_new, p_new
        r, r_old, psi, psi_old = r_old, r, psi_old, psi
        nsteps = j
        if np.all(dev[ROWS["done"]] == 1.0):
            break
    final = state.block(state.flat())
    assert np.all(final[ROWS["done"]] == 1.0), (nsteps, final[ROWS["done"]])
    assert np.all(final[ROWS["flag"]] == 0.0)
    met = np.array([1 + next(i for i, v in enumerate(norms) if v[c] < tol2[c]) for c in range(k)])
    assert np.array_equal(final[ROWS["steps"]], met.astype(float))
    assert len(set(met.tolist())) > 2                          # (they did freeze at different steps)
    # both buffers of a frozen column hold what it held when it froze
    for blk, froz in ((r, frozen_r), (r_old, frozen_r), (psi, frozen_psi), (psi_old, frozen_psi)):
        out = blk.get()
        assert all(same_bits(out[:, c], froz[c]) for c in range(k))
    # r = b - (I - alpha K F) F^-1 psi
    w = ph / f[:, None]
    res = B - (w - alpha * (K @ (f[:, None] * w)))
    assert np.all(np.linalg.norm(res - rh, axis=0) <= 1e-12 * np.sqrt(b2))
    # psi = sum_j s_j z_j from the log; slab entries of steps in which a column did not move are NaN and must be skipped
    Sd = ctx.empty(nsteps, k)
    call("eigd_cg_solution_coefficients", ctx.h, k, log.ptr, nsteps, Sd.ptr)
    Sh = Sd.get()
    gl = log.block(log.flat())[0:2 * nsteps:2]
    assert np.array_equal(Sh != 0.0, gl != 0.0) and np.all(Sh >= 0.0)
    for form in ("device", "host"):
        out = Padded(ctx, np.zeros((n, k)))
        if form == "device":
            call("eigd_stack_axpy_dev", ctx.h, n, k, nsteps, hist.ptr, hist.slab, hist.k, Sd.ptr, out.v.ptr, out.v.ld, 1.0)
        else:
            call("eigd_stack_axpy", ctx.h, n, k, nsteps, hist.ptr, hist.slab, hist.k, Sh.ctypes.data_as(C.c_void_p), out.v.ptr,
                 out.v.ld, 1.0)
        got = out.get()
        assert np.all(np.isfinite(got)), form
        assert np.all(np.linalg.norm(got - ph, axis=0) <= 1e-12 * np.linalg.norm(ph, axis=0)), form


# ---- the paired Gram-Schmidt step ---------------------------------------------------------------------------------------

GS_C0 = 9


@functools.lru_cache(maxsize=2)
def basis(n):
    """Q[c] (n x 41): an orthonormal basis of its own for every stack column (an independent QR per column)"""
    rng = np.random.default_rng(n)
    return [np.linalg.qr(rng.normal(size=(n, min(n, 41))))[0] for _ in range(32 + GS_C0)]


@pytest.mark.parametrize("ns", [1, 7, 32, 33, 40])
@pytest.mark.parametrize("k", [1, 5, 16, 32])
@pytest.mark.parametrize("n", [333, 20011])
def test_paired_gram_schmidt_step(ctx, n, k, ns):
    """
    eigd_stack_cgs2_pair (two passes up to 32 slabs, three beyond) and eigd_pair_orthonormalise.  Column c of T1 and
    column c of T2 both meet stack column C0 + c, whose basis is no other column's: a kernel that took slab column c'
    for c leaves components of 1e3 behind.  T2 = 0.7 T1 + noise before the step (T1.T2 does not cancel, so its relative
    rounding is that of a sum of mostly positive terms).
    """
    Q = basis(n)
    kw = k + GS_C0
    rng = np.random.default_rng(100 * k + ns)
    st = ctx.stack(ns + 1, n, kw)                             # (one slab more than the step may look at)
    for j in range(ns + 1):
        st[j].set(np.stack([Q[c][:, j] for c in range(kw)], axis=1))
    S = [np.stack([Q[GS_C0 + c][:, j] for c in range(k)], axis=1) for j in range(ns)]
    T1 = rng.normal(size=(n, k))
    T0 = np.concatenate([T1, 0.7 * T1 + rng.normal(size=(n, k))], axis=1)
    for c in range(2 * k):
        T0[:, c] += Q[GS_C0 + c % k][:, :ns] @ rng.normal(size=ns) * 1e3     # large components along the basis
    T = Padded(ctx, T0)
    H, passes = st.cgs2_pair(T.v, ns, c0=GS_C0, tol=1e-13)
    assert passes in ((2, 3) if ns <= 32 else (3, 4))          # one pass more beyond 32 slabs; the last one only if measured
    Tn = T.get()
    href, _ = kr.cgs2_pair_ref(S, T0)
    href = href.astype(np.float64)
    assert H.shape == (ns, 2 * k)
    assert np.linalg.norm(H - href) <= 1e-12 * np.linalg.norm(href)
    assert np.all(np.abs(H - href) <= 1e-12 * np.linalg.norm(href, axis=0))      # ... column by column
    Tref = T0 - sum(np.concatenate([S[j], S[j]], axis=1) * href[j] for j in range(ns))
    assert np.linalg.norm(Tn - Tref) <= 1e-9 * np.linalg.norm(Tref)
    left = np.array([np.sum(np.concatenate([S[j], S[j]], axis=1) * Tn, axis=0) for j in range(ns)])
    assert np.abs(left).max() < 1e-10 * np.abs(T0).max()
    # the pair itself, with the edge columns: skipped, |T1| = 0 with T1 = 0, T2 = 0 exactly
    edges = [(1, 2, 3)] if k >= 5 else [(0, None, None), (None, 0, None), (None, None, 0)]
    for skipc, zero1, zero2 in edges:
        Tp = Tn.copy()
        skip = np.zeros(k, dtype=bool)
        if skipc is not None:
            skip[skipc] = True
        if zero1 is not None:
            Tp[:, zero1] = 0.0
        if zero2 is not None:
            Tp[:, k + zero2] = 0.0
        T.set(Tp)
        norm2 = T.v.colnorm2_dev()
        n2h = norm2.get()[0]
        W1, W2 = Padded(ctx, np.full((n, k), np.nan)), Padded(ctx, np.full((n, k), np.nan))
        out = T.v.pair_orthonormalise(norm2, W1.v, W2.v, skip)
        fetched = ctx.fetch_colnorm2(4 * k)
        oh = out.get()[0]
        assert same_bits(fetched, oh)
        rW1, rT2, rW2, rout = kr.pair_orthonormalise_ref(Tp, n2h, skip)
        Tafter, w1, w2 = T.get(), W1.get(), W2.get()
        assert same_bits(Tafter[:, :k], Tp[:, :k])             # T1 is read only
        for got, ref in ((w1, rW1), (Tafter[:, k:], rT2), (w2, rW2)):
            assert np.all(np.isfinite(got))
            ref = ref.astype(np.float64)
            assert np.all(np.linalg.norm(got - ref, axis=0) <= 1e-13 * np.linalg.norm(ref, axis=0))
        assert np.all(np.isfinite(oh))
        rout = rout.astype(np.float64)
        assert same_bits(oh[:k], n2h[:k])
        assert np.all(np.abs(oh[k:3 * k] - rout[k:3 * k]) <= 1e-13 * np.abs(rout[k:3 * k]))
        assert np.all(np.abs(oh[3 * k:] - rout[3 * k:]) <= 1e-13 * np.linalg.norm(Tp[:, k:], axis=0))
        for c in (skipc, zero1):
            if c is not None:                                  # the documented zeros
                assert not w1[:, c].any() and not Tafter[:, k + c].any() and not w2[:, c].any()
                assert oh[2 * k + c] == 0.0 and oh[3 * k + c] == 0.0
        if zero1 is not None:
            assert oh[zero1] == 0.0 and oh[k + zero1] == 0.0
        if zero2 is not None:
            assert not w2[:, zero2].any() and not Tafter[:, k + zero2].any() and oh[2 * k + zero2] == 0.0
            assert abs(np.linalg.norm(w1[:, zero2]) - 1.0) < 1e-14
